// Stand-alone check of the host side of orblm_keyframe_culling and
// orblm_cull_recent (make cull_check, host code under AddressSanitizer +
// UBSan): the map and graph validation, the flattening into the staged pools
// and the failure path of a machine without a device, where the first hipMalloc
// fails after the pools were packed. With a device present the refusals are
// still checked. The library's reporters are replaced by stand-ins: they are
// not what is under test.
#include <cstring>
#include <vector>

#include "keyframe_culling.hip"
#include "check_common.h"

namespace {

// the map of three keyframes with its graph (keyframe 2 is the current one, its
// list [1, 0]), the recent lists and the line table
struct CullMap : TinyMap {
  float depth[3][3] = {{1, 1, 1}, {1, 1, 1}, {1, 1, 1}};
  const float* dptr[3] = {depth[0], depth[1], depth[2]};
  int32_t cw[9] = {0, 1, 1, 1, 0, 1, 1, 1, 0};
  int32_t ord[3 * 64];
  int32_t parent[3] = {-1, 0, 1};
  uint8_t not_erase[3] = {0, 0, 0}, kf_bad[3] = {0, 0, 0}, tbe[3] = {9, 9, 9};
  float Tcp[48] = {};
  // the recent lists and the line table
  int32_t first_kf[2] = {9, 7}, recent[2] = {1, 0}, reason[2] = {-1, -1};
  int32_t nl[3] = {2, 0, 1}, ml0[2] = {0, 1}, ml2[1] = {1};
  int32_t* ml[3] = {ml0, nullptr, ml2};
  uint8_t lbad[2] = {0, 0};
  int32_t lvis[2] = {3, 3}, lfound[2] = {2, 2}, lfirst[2] = {-1, 9}, lnobs[2] = {2, 5};
  int32_t rlines[2] = {0, 1}, lreason[2] = {-1, -1};

  CullMap() {
    for (int i = 0; i < 3 * 64; i++) ord[i] = -1;
    ord[0] = 1, ord[1] = 2, ord[64] = 0, ord[65] = 2, ord[128] = 1, ord[129] = 0;
  }
  orblm_kfc_problem kfc() {
    orblm_kfc_problem p{};
    p.map = m;
    p.cur = 2;
    p.depth = dptr;
    p.conn_w = cw;
    p.ordered = ord;
    p.parent = parent;
    p.not_erase = not_erase;
    p.kf_bad = kf_bad;
    p.to_be_erased = tbe;
    p.Tcp = Tcp;
    return p;
  }
  orblm_recent_problem rc() {
    orblm_recent_problem p{};
    p.map = m;
    p.cur_id = 9;
    p.first_kf = first_kf;
    p.recent = recent;
    p.n_recent = 2;
    p.reason = reason;
    p.L = 2;
    p.nl = nl;
    p.ml = ml;
    p.line_bad = lbad;
    p.line_n_visible = lvis;
    p.line_n_found = lfound;
    p.line_first_kf = lfirst;
    p.line_n_obs = lnobs;
    p.recent_lines = rlines;
    p.n_recent_lines = 2;
    p.line_reason = lreason;
    return p;
  }
};

const orbpl_camera kCam = {517.f, 516.f, 318.f, 255.f, 0, 0, 0, 0, 0, 40.f, 3.f, 640, 480};

}  // namespace

int main() {
#define KFC_REFUSED(edit, text)                                        \
  do {                                                                 \
    CullMap t;                                                         \
    orblm_kfc_problem p = t.kfc();                                     \
    edit;                                                              \
    EXPECT(orblm_keyframe_culling(&kCam, 8, &p, 1) == ORBPL_ERR_ARG);  \
    EXPECT(g_msg == text);                                             \
  } while (0)
  // the map itself, as orblm_search_in_neighbors refuses it
  KFC_REFUSED(t.mp[1][2] = 0, "map point twice in one keyframe");
  KFC_REFUSED(t.kf[1].id = 9, "two keyframes of a map with one id");
  KFC_REFUSED(t.kp[0][2].octave = 8, "keypoint octave outside [0, nlevels)");
  KFC_REFUSED(t.mp[0][1] = 2, "slot index outside [-1, M)");
  KFC_REFUSED(t.ref[1] = 0, "good map point whose ref_kf does not observe it");
  KFC_REFUSED(p.map.nkf = 65, "map with no keyframe or more than 64");
  KFC_REFUSED(p.map.obs = nullptr, "NULL map point arrays");
  KFC_REFUSED(t.kf[0].n = 2049, "keyframe with more than 2048 features");
  // the graph
  KFC_REFUSED(p.cur = 3, "current keyframe outside the table");
  KFC_REFUSED(p.conn_w = nullptr, "NULL graph arrays");
  KFC_REFUSED(p.depth = nullptr, "NULL graph arrays");
  KFC_REFUSED(t.dptr[1] = nullptr, "NULL graph arrays");
  KFC_REFUSED(p.Tcp = nullptr, "NULL graph arrays");
  KFC_REFUSED(t.cw[5] = -1, "negative covisibility weight");
  KFC_REFUSED(t.cw[4] = 2, "non-zero diagonal of conn_w");
  KFC_REFUSED(t.ord[64] = 3, "ordered entry outside the table or naming its own keyframe");
  KFC_REFUSED(t.ord[64] = 1, "ordered entry outside the table or naming its own keyframe");
  KFC_REFUSED(t.ord[65] = 0, "ordered list names a keyframe twice");
  KFC_REFUSED(t.parent[2] = 3, "parent outside the table or naming its own keyframe");
  KFC_REFUSED(t.parent[2] = 2, "parent outside the table or naming its own keyframe");
  KFC_REFUSED(t.parent[2] = -2, "parent outside the table or naming its own keyframe");
  KFC_REFUSED(t.parent[1] = -1, "good keyframe with id != 0 and no parent");
  {
    CullMap t;
    orblm_kfc_problem two[2] = {t.kfc(), t.kfc()};
    EXPECT(orblm_keyframe_culling(&kCam, 8, two, 2) == ORBPL_ERR_ARG);
    EXPECT(g_msg == "a keyframe, point or graph array belongs to two problems");
    EXPECT(orblm_keyframe_culling(&kCam, 17, two, 1) == ORBPL_ERR_ARG && g_msg == "nlevels outside [1, 16]");
    EXPECT(orblm_keyframe_culling(nullptr, 8, two, 1) == ORBPL_ERR_ARG && g_msg == "NULL camera");
    orblm_kfc_device_batch b{};
    EXPECT(orblm_keyframe_culling_batch_device(&kCam, &b, 1, nullptr) == ORBPL_ERR_ARG);
    b.nkf = b.kp_pitch = 1;
    EXPECT(orblm_keyframe_culling_batch_device(&kCam, &b, 1, nullptr) == ORBPL_ERR_ARG);
    EXPECT(g_msg == "NULL device array");
  }
#define RC_REFUSED(edit, text)                               \
  do {                                                       \
    CullMap t;                                               \
    orblm_recent_problem p = t.rc();                         \
    edit;                                                    \
    EXPECT(orblm_cull_recent(8, &p, 1) == ORBPL_ERR_ARG);    \
    EXPECT(g_msg == text);                                   \
  } while (0)
  RC_REFUSED(t.mp[1][2] = 0, "map point twice in one keyframe");
  RC_REFUSED(t.recent[1] = 1, "recent entry repeats");
  RC_REFUSED(t.recent[1] = 2, "recent entry outside [0, M)");
  RC_REFUSED(t.recent[1] = -1, "recent entry outside [0, M)");
  RC_REFUSED(t.rlines[1] = 0, "recent line entry repeats");
  RC_REFUSED(t.rlines[1] = 2, "recent line entry outside [0, L)");
  RC_REFUSED(p.L = 64 * 256 + 1, "map lines outside [0, 64 * 256]");
  RC_REFUSED(t.nl[0] = 257, "keyframe with more than 256 lines");
  RC_REFUSED(t.ml0[1] = 2, "line slot outside [-1, L)");
  RC_REFUSED(t.ml[2] = nullptr, "NULL culling arrays");
  RC_REFUSED(p.first_kf = nullptr, "NULL culling arrays");
  RC_REFUSED(p.line_n_obs = nullptr, "NULL culling arrays");
  RC_REFUSED(p.reason = nullptr, "NULL culling arrays");
  RC_REFUSED(p.n_recent = -1, "negative list length");
  {
    CullMap t;
    orblm_recent_problem two[2] = {t.rc(), t.rc()};
    EXPECT(orblm_cull_recent(8, two, 2) == ORBPL_ERR_ARG);
    EXPECT(g_msg == "a keyframe, point or graph array belongs to two problems");
  }
  // a valid problem: packed into the pools, then staged
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) {
    printf("a device is present: the refusals hold, the staging failure path was not run\n");
    return 0;
  }
  {
    CullMap t;
    const CullMap before;
    orblm_kfc_problem p = t.kfc();
    EXPECT(orblm_keyframe_culling(&kCam, 8, &p, 1) == ORBPL_ERR_HIP);
    EXPECT(!memcmp(t.mp, before.mp, sizeof(t.mp)) && !memcmp(t.cw, before.cw, sizeof(t.cw)));
    EXPECT(!memcmp(t.tbe, before.tbe, sizeof(t.tbe)) && !memcmp(t.parent, before.parent, sizeof(t.parent)));
    orblm_recent_problem r = t.rc();
    EXPECT(orblm_cull_recent(8, &r, 1) == ORBPL_ERR_HIP);
    EXPECT(r.n_recent == 2 && r.n_recent_lines == 2 && t.reason[0] == -1 && t.lreason[1] == -1);
    EXPECT(!memcmp(t.ml0, before.ml0, sizeof(t.ml0)) && !memcmp(t.bad, before.bad, sizeof(t.bad)));
    EXPECT(orblm_keyframe_culling(&kCam, 8, nullptr, 0) == ORBPL_OK);
    EXPECT(orblm_cull_recent(8, nullptr, 0) == ORBPL_OK);
  }
  printf("keyframe_culling_check: ok\n");
  return 0;
}
