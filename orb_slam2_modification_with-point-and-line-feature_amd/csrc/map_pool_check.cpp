// Stand-alone check of map_pool.h (make pool_check, host code under
// AddressSanitizer + UBSan, no device call): two hand-built maps of different
// shape in one pool, every packed value against the value written out here, and
// what unpack changes of the callers' arrays. The entries of an array past a
// keyframe's n or a map's M are the guards: unpack must leave them alone.
#include <cstring>
#include <vector>

#include "map_pool.h"
#include "check_common.h"

using orbpl::MapPool;

template <class T>
static bool eq(const std::vector<T>& v, std::initializer_list<typename std::vector<T>::value_type> want) {
  return v == std::vector<T>(want);
}

int main() {
  // A: keyframe 0 full with a short ordered list, keyframe 1 with n = 2 of 3,
  // keyframe 2 with n = 0 and no ordered list; one point (the arrays hold two)
  TinyMap A;
  A.kf[1].n = 2;
  A.kf[2].n = 0;
  A.m.M = 1;
  A.kf_ord[0][2] = 2;                        // behind the list's end
  A.ur[1][2] = 55, A.mp[1][2] = 0;           // behind keyframe 1's n
  A.kdesc[0][0] = 7, A.kdesc[1][63] = 9, A.kdesc[1][64] = 1, A.desc[31] = 5, A.desc[32] = 6;
  A.bad[1] = 9;
  for (int i = 0; i < 2; i++) A.rep[i] = A.nobs[i] = A.src[2 * i] = A.src[2 * i + 1] = -7;
  for (int i = 0; i < 128; i++) A.obs[i] = -7;
  // B: one keyframe of one feature, no point, no point array
  float TB[16] = {}, urB[1] = {77};
  orbpl_keypoint kpB[1] = {};
  uint8_t descB[32] = {};
  int32_t mpB[1] = {-1};
  orblm_map_keyframe kfB = {3, TB, 1, kpB, urB, descB, mpB, nullptr};
  orblm_map B = {1, &kfB};

  MapPool H;
  H.add(A.m, 2);
  H.add(B, 0);
  EXPECT(eq(H.prob, {0, 3, 0, 1, 2, 3, 1, 1, 0, 0}));
  EXPECT(H.nkf == 4 && H.nmp == 1 && H.pitch == 3 && H.M() == 1);
  EXPECT(H.kf0(1) == 3 && H.mp0(1) == 1 && H.kf0(0) == 0 && H.mp0(0) == 0);
  H.pack(MapPool::kId | MapPool::kN | MapPool::kUright | MapPool::kKfDesc | MapPool::kMp | MapPool::kOrdered |
         MapPool::kXyz | MapPool::kDesc | MapPool::kBad | MapPool::kNVisible | MapPool::kNObs | MapPool::kObs);
  EXPECT(eq(H.id, {0, 5, 9, 3}) && eq(H.n, {3, 2, 0, 1}));
  EXPECT(eq(H.uright, {300, -1, 100, 290, 50, -1, -1, -1, -1, 77, -1, -1}));
  EXPECT(eq(H.mp, {0, -1, -1, 0, 1, -1, -1, -1, -1, -1, -1, -1}));
  EXPECT(H.ordered.size() == 4 * 64 && H.ordered[0] == 1 && H.ordered[64] == 0);
  for (size_t i = 0; i < H.ordered.size(); i++) EXPECT(i == 0 || i == 64 || H.ordered[i] == -1);
  EXPECT(H.kf_desc.size() == 4 * 3 * 32 && H.kf_desc[0] == 7 && H.kf_desc[(3 + 1) * 32 + 31] == 9);
  for (size_t i = 0; i < H.kf_desc.size(); i++) EXPECT(i == 0 || i == (3 + 1) * 32 + 31 || H.kf_desc[i] == 0);
  EXPECT(eq(H.xyz, {0, 0, 4}) && eq(H.bad, {0}) && eq(H.n_visible, {3}) && eq(H.n_obs, {0}));
  EXPECT(H.desc.size() == 32 && H.desc[31] == 5 && H.desc[0] == 0);
  EXPECT(H.obs == std::vector<int16_t>(64, 0));
  // the columns not asked for are not packed
  EXPECT(H.Tcw.empty() && H.kps_un.empty() && H.normal.empty() && H.min_dist.empty() && H.max_dist.empty() &&
         H.ref_kf.empty() && H.n_found.empty() && H.replaced_by.empty() && H.desc_src.empty());

  // no point at all: one row of padding
  MapPool E;
  E.add(B, 0);
  E.pack(MapPool::kTcw | MapPool::kKpsUn | MapPool::kUright | MapPool::kMp | MapPool::kNormal | MapPool::kRefKf |
         MapPool::kBad | MapPool::kNFound | MapPool::kReplacedBy | MapPool::kDescSrc);
  EXPECT(eq(E.prob, {0, 1, 0, 0, 0}) && E.nmp == 0 && E.M() == 1 && E.pitch == 1);
  EXPECT(eq(E.bad, {1}) && eq(E.ref_kf, {0}) && eq(E.n_found, {0}) && eq(E.normal, {0, 0, 0}));
  EXPECT(eq(E.replaced_by, {0}) && eq(E.desc_src, {0, 0}) && eq(E.uright, {77}) && eq(E.mp, {-1}));
  EXPECT(E.Tcw.size() == 16 && E.kps_un.size() == 1 && E.id.empty() && E.obs.empty());

  // unpack: the named columns, the first n / M entries, nothing else
  for (size_t i = 0; i < H.mp.size(); i++) H.mp[i] = 40 + (int32_t)i;
  H.bad = {1};
  H.n_obs = {8};
  H.n_visible = {6};
  H.obs.assign(64, 3);
  H.unpack(MapPool::kMp | MapPool::kBad | MapPool::kObs);
  const TinyMap fresh;
  EXPECT(A.mp[0][0] == 40 && A.mp[0][1] == 41 && A.mp[0][2] == 42);
  EXPECT(A.mp[1][0] == 43 && A.mp[1][1] == 44 && A.mp[1][2] == 0);
  EXPECT(!memcmp(A.mp[2], fresh.mp[2], sizeof(A.mp[2])) && mpB[0] == 49);
  EXPECT(A.bad[0] == 1 && A.bad[1] == 9);
  for (int i = 0; i < 128; i++) EXPECT(A.obs[i] == (i < 64 ? 3 : -7));
  EXPECT(A.nobs[0] == -7 && A.rep[0] == -7 && A.src[0] == -7 && A.vis[0] == 3 && A.vis[1] == 4);
  EXPECT(!memcmp(A.normal, fresh.normal, sizeof(A.normal)) && !memcmp(A.ref, fresh.ref, sizeof(A.ref)));
  H.unpack(MapPool::kNObs | MapPool::kNVisible);
  EXPECT(A.nobs[0] == 8 && A.nobs[1] == -7 && A.vis[0] == 6 && A.vis[1] == 4 && A.mp[1][2] == 0);

  // the ownership test
  EXPECT(H.owned == std::vector<const void*>({A.mp[0], A.mp[1], mpB}) && !H.shares_an_array());
  H.owned.push_back(A.mp[0]);
  EXPECT(H.shares_an_array());
  printf("map_pool_check: ok\n");
  return 0;
}
