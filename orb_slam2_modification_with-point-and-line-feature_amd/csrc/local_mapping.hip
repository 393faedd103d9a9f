// LocalMapping::CreateNewMapPoints and CreateNewMapLines (LocalMapping.cc:346-665,
// 668-916) on gfx950, batched
// over independent (current keyframe, <= 10 neighbours) problems: one
// 256-thread workgroup per problem walks the neighbours in order (a point
// created with neighbour i occupies KF1's feature for the neighbours after
// it), so a problem needs no launch per neighbour and nothing goes back to the
// host. Per neighbour:
//   1. lane 0: the baseline test, ComputeF12, the epipole (localmap_core.h);
//   2. ORBmatcher::SearchForTriangulation (ORBmatcher.cc:884-1095): both
//      FeatureVectors sorted by (node, index) in LDS as match_bow_body does
//      (KF1's once per problem); every free KF1 feature computes, in
//      parallel, its four best candidates over its node's KF2 run, a candidate
//      being a free KF2 feature with Hamming <= 50 that passes the epipole and
//      epipolar-line tests (none of which depends on the search's state); the
//      reference's `dist > bestDist` with bestDist moving only on a pass leaves
//      "smallest distance, latest index" among them, so the lists are ordered
//      by (distance, -index); one lane per node then replays the in-order
//      claims and rescans the run exactly when a full list is all claimed;
//   3. one thread per pair triangulates (the 4x4 Jacobi in registers); the
//      record order (neighbour, then KF1 index) comes from a workgroup prefix
//      scan per 256 features, never from an atomic counter.
// Then CreateNewMapLines, again neighbour by neighbour:
//   4. pKF2->ComputeSceneMedianDepth(2): the depths of the neighbour's map
//      points, those the point stage just created with it included, sorted in
//      LDS (each in its feature's slot, so no counter orders anything);
//   5. LineMatcher::SearchForTriangulation: k_line_bf_knn's knnMatch body, one
//      KF1 line per thread; both medians of lineDescriptorMAD are ranks in a
//      257-bin histogram (the distances are integers);
//   6. one thread per line pair runs the two 4x4 SVDs; record order by prefix
//      scan.
// Descriptors are read as uint4 from L2; every store is a vector store.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/orbpl.h"
#include "block_ops.h"
#include "localmap_core.h"
#include "match_common.h"
#include "host_rows.h"
#include "host_stage.h"
#include "orbpl_runtime.h"

namespace orbpl {
namespace {

constexpr int kLmThreads = 256;
constexpr uint32_t kNoKey = 0xFFFFFFFFu;

struct LmArgs {
  lm::Consts c;
  orblm_device_batch b;
  int match_only;      // 1: ORBmatcher::SearchForTriangulation alone, 2: LineMatcher's: pairs to pairs_out
  int only_stereo, check_ori;
  int32_t* pairs_out;  // match_only: 2 * kp_pitch per problem
  float* f12_out;      // match_only: 9 per problem, or NULL
  int use_f12;         // match_only 1: the caller's F12 instead of ComputeF12's
  float f12_in[9];
};

struct LmShared {
  uint32_t s1[lm::kMaxKp], s2[lm::kMaxKp];    // (node << 11 | index), sorted
  alignas(16) uint32_t cand[lm::kMaxKp][4];   // by sorted KF1 position: (dist << 11 | 2047 - idx2)
  int16_t m12[lm::kMaxKp];                    // KF1 feature -> KF2 feature, -1
  int8_t bin1[lm::kMaxKp];                    // rotation bin of KF1's match, -1
  uint8_t occ1[lm::kMaxKp];                   // KF1 feature holds a map point
  uint8_t claimed2[lm::kMaxKp];               // vbMatched2
  int hist[32];
  int ind[3];
  int wsum[4];
  int skip;
  int lhist[2][260];                                     // counts of d12 and of |d12 - median|
  int l_med;
  double l_thr;
  float M1[12], M2[12];                                  // K * Tcw
  float F[9];
  float ex, ey;
  lm::Pose P1, P2;
};

// [b, e) of the features of `node` in the sorted keys s[0, ns) (the padding
// kNoKey sorts above every node: ids are < 2^21 - 1)
__device__ __forceinline__ void node_run(const uint32_t* s, int ns, uint32_t node, int* b, int* e) {
  int lo = 0, hi = ns;
  while (lo < hi) {
    const int m = (lo + hi) >> 1;
    if ((s[m] >> 11) < node) lo = m + 1;
    else hi = m;
  }
  int x = lo, h2 = ns;
  while (x < h2) {
    const int m = (x + h2) >> 1;
    if ((s[m] >> 11) <= node) x = m + 1;
    else h2 = m;
  }
  *b = lo;
  *e = x;
}

struct KfView {
  int n, id;
  const KeyPointD* kps;
  const KeyPointD* kps_un;
  const float* uright;
  const float* depth;
  const uint4* desc;
  const int32_t* node;
  const uint8_t* has_mp;
  const float* mp_xyz;
  int nl;
  const orbpl_keyline* klines;
  const uint4* ldesc;
  const double* lcoef;
};

__device__ __forceinline__ KfView kf_view(const orblm_device_batch& b, int k) {
  const long long o = (long long)k * b.kp_pitch;
  KfView v;
  v.n = max(0, min(b.d_kf_n[k], min(b.kp_pitch, lm::kMaxKp)));
  v.id = b.d_kf_id[k];
  v.kps = reinterpret_cast<const KeyPointD*>(b.d_kps) + o;
  v.kps_un = reinterpret_cast<const KeyPointD*>(b.d_kps_un) + o;
  v.uright = b.d_uright + o;
  v.depth = b.d_depth + o;
  v.desc = reinterpret_cast<const uint4*>(b.d_desc + o * 32);
  v.node = b.d_feat_node + o;
  v.has_mp = b.d_has_mp + o;
  v.mp_xyz = b.d_mp_xyz + o * 3;
  const long long lo = (long long)k * b.line_pitch;
  v.nl = max(0, min(b.d_kf_nl[k], min(b.line_pitch, lm::kMaxLines)));
  v.klines = b.d_klines + lo;
  v.ldesc = reinterpret_cast<const uint4*>(b.d_ldesc + lo * 32);
  v.lcoef = b.d_lcoef + lo * 3;
  return v;
}

__device__ __forceinline__ int clamp_level(const lm::Consts& c, int o) {
  return max(0, min(o, c.nlevels - 1));
}

// order-preserving key of a float (kNoKey sorts last)
__device__ __forceinline__ uint32_t float_key(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// the value at `rank` (0-based) of the multiset counted in hist[0..256]
__device__ __forceinline__ int hist_rank(const int* hist, int rank) {
  int acc = 0;
  for (int v = 0; v <= 256; v++) {
    acc += hist[v];
    if (acc > rank) return v;
  }
  return 256;
}

// the candidate key of (KF1 feature i1, KF2 feature i2), kNoKey when it cannot
// be taken whatever the state of the search
__device__ __forceinline__ uint32_t cand_key(const LmArgs& a, const LmShared& S, const KfView& K2,
                                             float x1, float y1, bool stereo1, const uint4 k0,
                                             const uint4 k1, int i2) {
  if (K2.has_mp[i2]) return kNoKey;
  const bool stereo2 = K2.uright[i2] >= 0.0f;
  if (a.only_stereo && !stereo2) return kNoKey;
  const int d = hamming256(k0, k1, K2.desc + 2 * i2);
  if (d > lm::kThLow) return kNoKey;
  const KeyPointD kp2 = K2.kps_un[i2];
  if (!lm::pair_geometry(a.c, S.F, S.ex, S.ey, x1, y1, stereo1, kp2.x, kp2.y,
                         clamp_level(a.c, kp2.octave), stereo2))
    return kNoKey;
  return ((uint32_t)d << 11) | (uint32_t)(2047 - i2);
}

__global__ void __launch_bounds__(kLmThreads) k_create_new_map_features(LmArgs a) {
  __shared__ LmShared S;
  const int t = threadIdx.x, p = blockIdx.x;
  const orblm_device_batch& b = a.b;
  const long long ob = (long long)p * b.kp_pitch;
  const int cur = b.d_cur[p];
  const long long lb = (long long)p * b.line_pitch;
  if (t < lm::kNeighbours) {
    b.d_pairs[p * lm::kNeighbours + t] = -1;
    b.d_line_pairs[p * lm::kNeighbours + t] = -1;
  }
  for (int i = t; i < b.line_pitch; i += kLmThreads) b.d_kf1_line_record[lb + i] = -1;
  if (cur < 0 || cur >= b.nkf) {
    if (t == 0) {
      b.d_n_points[p] = 0;
      b.d_n_lines[p] = 0;
    }
    for (int i = t; i < b.kp_pitch; i += kLmThreads) b.d_kf1_point_record[ob + i] = -1;
    return;
  }
  const KfView K1 = kf_view(b, cur);
  const int n1 = K1.n;
  for (int i = t; i < b.kp_pitch; i += kLmThreads) b.d_kf1_point_record[ob + i] = -1;
  for (int i = t; i < lm::kMaxKp; i += kLmThreads) {
    S.s1[i] = (i < n1 && K1.node[i] >= 0) ? ((uint32_t)K1.node[i] << 11) | (uint32_t)i : kNoKey;
    S.occ1[i] = i < n1 ? (K1.has_mp[i] ? 1 : 0) : 1;
  }
  if (t == 0) {
    lm::make_pose(b.d_kf_Tcw + (long long)cur * 16, &S.P1);
    lm::projection_matrix(a.c, S.P1.T, S.M1);
  }
  __syncthreads();
  int ns1 = 64;
  while (ns1 < n1) ns1 <<= 1;
  bitonic_sort(S.s1, ns1, kLmThreads);
  int nrec = 0;
  for (int nb = 0; nb < lm::kNeighbours && a.match_only != 2; nb++) {
    const int k2 = b.d_neigh[p * lm::kNeighbours + nb];
    if (k2 < 0) break;
    if (k2 >= b.nkf) continue;
    __syncthreads();   // the previous neighbour's readers of S.skip, S.P2, S.F are done
    if (t == 0) {
      lm::make_pose(b.d_kf_Tcw + (long long)k2 * 16, &S.P2);
      const float base[3] = {S.P2.Ow[0] - S.P1.Ow[0], S.P2.Ow[1] - S.P1.Ow[1],
                             S.P2.Ow[2] - S.P1.Ow[2]};
      const float baseline = (float)lm::norm3d(base);
      S.skip = !a.match_only && baseline < a.c.mb;
      lm::compute_f12(a.c, S.P1.T, S.P2.T, S.F);
      if (a.use_f12)
        for (int k = 0; k < 9; k++) S.F[k] = a.f12_in[k];
      lm::epipole(a.c, S.P1.Ow, S.P2.T, &S.ex, &S.ey);
    }
    __syncthreads();
    if (S.skip) continue;
    const KfView K2 = kf_view(b, k2);
    const int n2 = K2.n;
    for (int i = t; i < lm::kMaxKp; i += kLmThreads) {
      S.s2[i] = (i < n2 && K2.node[i] >= 0) ? ((uint32_t)K2.node[i] << 11) | (uint32_t)i : kNoKey;
      S.claimed2[i] = 0;
      S.m12[i] = -1;
      S.bin1[i] = -1;
    }
    if (t < 32) S.hist[t] = 0;
    __syncthreads();
    int ns2 = 64;
    while (ns2 < n2) ns2 <<= 1;
    bitonic_sort(S.s2, ns2, kLmThreads);
    // candidate lists, one free KF1 feature per lane
    for (int q = t; q < n1; q += kLmThreads) {
      const uint32_t key = S.s1[q];
      uint32_t c0 = kNoKey, c1 = kNoKey, c2 = kNoKey, c3 = kNoKey;
      if (key != kNoKey) {
        const int i1 = (int)(key & 0x7FF);
        const bool stereo1 = K1.uright[i1] >= 0.0f;
        if (!S.occ1[i1] && !(a.only_stereo && !stereo1)) {
          int fb, fe;
          node_run(S.s2, ns2, key >> 11, &fb, &fe);
          const KeyPointD kp1 = K1.kps_un[i1];
          const uint4 k0 = K1.desc[2 * i1], k1 = K1.desc[2 * i1 + 1];
          for (int r = fb; r < fe; r++) {
            const uint32_t k = cand_key(a, S, K2, kp1.x, kp1.y, stereo1, k0, k1,
                                        (int)(S.s2[r] & 0x7FF));
            c3 = min(c3, max(c2, k));
            c2 = min(c2, max(c1, k));
            c1 = min(c1, max(c0, k));
            c0 = min(c0, k);
          }
        }
      }
      *reinterpret_cast<uint4*>(S.cand[q]) = make_uint4(c0, c1, c2, c3);
    }
    __syncthreads();
    // in-order claims, one lane per KF1 node run
    for (int q0 = t; q0 < n1; q0 += kLmThreads) {
      const uint32_t key0 = S.s1[q0];
      if (key0 == kNoKey) continue;
      const uint32_t node = key0 >> 11;
      if (q0 > 0 && (S.s1[q0 - 1] >> 11) == node) continue;   // not the run's first
      int fb, fe;
      node_run(S.s2, ns2, node, &fb, &fe);
      if (fb == fe) continue;
      for (int q = q0; q < n1 && S.s1[q] != kNoKey && (S.s1[q] >> 11) == node; q++) {
        const int i1 = (int)(S.s1[q] & 0x7FF);
        const uint4 cv = *reinterpret_cast<const uint4*>(S.cand[q]);
        if (cv.x == kNoKey) continue;   // occupied, filtered, or no candidate
        const uint32_t cl[4] = {cv.x, cv.y, cv.z, cv.w};
        uint32_t best = kNoKey;
#pragma unroll
        for (int k = 0; k < 4; k++)
          if (best == kNoKey && cl[k] != kNoKey && !S.claimed2[2047 - (int)(cl[k] & 0x7FF)])
            best = cl[k];
        if (best == kNoKey && cl[3] != kNoKey && fe - fb > 4) {
          // a full list, all claimed: the rest of the run decides, exactly
          const bool stereo1 = K1.uright[i1] >= 0.0f;
          const KeyPointD kp1 = K1.kps_un[i1];
          const uint4 k0 = K1.desc[2 * i1], k1 = K1.desc[2 * i1 + 1];
          for (int r = fb; r < fe; r++) {
            const int i2 = (int)(S.s2[r] & 0x7FF);
            if (S.claimed2[i2]) continue;
            best = min(best, cand_key(a, S, K2, kp1.x, kp1.y, stereo1, k0, k1, i2));
          }
        }
        if (best == kNoKey) continue;
        const int i2 = 2047 - (int)(best & 0x7FF);
        S.m12[i1] = (int16_t)i2;
        S.claimed2[i2] = 1;
        if (a.check_ori) {
          const int bin = rotation_bin(K1.kps_un[i1].angle, K2.kps_un[i2].angle);
          S.bin1[i1] = (int8_t)bin;
          atomicAdd(&S.hist[bin], 1);
        }
      }
    }
    __syncthreads();
    if (a.check_ori) {
      if (t == 0) three_maxima(S.hist, S.ind[0], S.ind[1], S.ind[2]);
      __syncthreads();
      for (int i = t; i < n1; i += kLmThreads) {
        const int bn = S.bin1[i];
        if (bn >= 0 && bn != S.ind[0] && bn != S.ind[1] && bn != S.ind[2]) S.m12[i] = -1;
      }
      __syncthreads();
    }
    int np = 0;
    for (int i = t; i < n1; i += kLmThreads) np += S.m12[i] >= 0;
    np = block_sum<4>(np, S.wsum);
    if (t == 0) b.d_pairs[p * lm::kNeighbours + nb] = np;
    if (a.match_only == 1) {
      // vMatchedPairs, in KF1 index order
      int base = 0;
      for (int i0 = 0; i0 < n1; i0 += kLmThreads) {
        const int i = i0 + t;
        const bool f = i < n1 && S.m12[i] >= 0;
        int tot;
        const int pos = block_prefix<4>(f, S.wsum, &tot);
        if (f)
          *reinterpret_cast<int2*>(a.pairs_out + 2 * (ob + base + pos)) = make_int2(i, (int)S.m12[i]);
        base += tot;
      }
      if (a.f12_out && t < 9) a.f12_out[p * 9 + t] = S.F[t];
      break;
    }
    // triangulation, one thread per pair, records in KF1 index order
    const bool kf1_first = K1.id < K2.id;
    for (int i0 = 0; i0 < n1; i0 += kLmThreads) {
      const int i = i0 + t;
      bool made = false;
      lm::PointOut o;
      int i2 = -1;
      if (i < n1 && S.m12[i] >= 0) {
        i2 = S.m12[i];
        const KeyPointD u1 = K1.kps_un[i], u2 = K2.kps_un[i2];
        const KeyPointD r1 = K1.kps[i], r2 = K2.kps[i2];
        made = lm::triangulate_pair(a.c, S.P1, S.P2, u1.x, u1.y, clamp_level(a.c, u1.octave), r1.x,
                                    r1.y, K1.uright[i], K1.depth[i], u2.x, u2.y,
                                    clamp_level(a.c, u2.octave), r2.x, r2.y, K2.uright[i2],
                                    K2.depth[i2], kf1_first, &o);
      }
      int tot;
      const int pos = block_prefix<4>(made, S.wsum, &tot);
      if (made) {
        const int r = nrec + pos;
        float4* dst = reinterpret_cast<float4*>(b.d_points + ob + r);
        dst[0] = make_float4(__int_as_float(nb), __int_as_float(i), __int_as_float(i2),
                             __int_as_float(kf1_first ? 0 : 1));
        dst[1] = make_float4(o.xyz[0], o.xyz[1], o.xyz[2], o.normal[0]);
        dst[2] = make_float4(o.normal[1], o.normal[2], o.min_dist, o.max_dist);
        b.d_kf1_point_record[ob + i] = r;
        S.occ1[i] = 1;   // AddMapPoint: taken for the neighbours after this one
      }
      nrec += tot;
    }
  }
  if (t == 0) b.d_n_points[p] = nrec;
  if (a.match_only == 1) {
    if (t == 0) b.d_n_lines[p] = 0;
    return;
  }
  // ---- CreateNewMapLines ----
  const int nl1 = K1.nl;
  orblm_line_record* lines = b.d_lines + (long long)p * lm::kNeighbours * b.line_pitch;
  int nlrec = 0;
  for (int nb = 0; nb < lm::kNeighbours; nb++) {
    const int k2 = b.d_neigh[p * lm::kNeighbours + nb];
    if (k2 < 0) break;
    if (k2 >= b.nkf) continue;
    __syncthreads();
    if (t == 0) {
      lm::make_pose(b.d_kf_Tcw + (long long)k2 * 16, &S.P2);
      const float base[3] = {S.P2.Ow[0] - S.P1.Ow[0], S.P2.Ow[1] - S.P1.Ow[1],
                             S.P2.Ow[2] - S.P1.Ow[2]};
      S.skip = a.match_only != 2 && (float)lm::norm3d(base) < a.c.mb;
      lm::projection_matrix(a.c, S.P2.T, S.M2);
    }
    for (int i = t; i < 2 * 260; i += kLmThreads) (&S.lhist[0][0])[i] = 0;
    __syncthreads();
    if (S.skip) continue;
    const KfView K2 = kf_view(b, k2);
    const int nl2 = K2.nl;
    // pKF2->ComputeSceneMedianDepth(2), after the point stage
    float median = 0.0f;
    int ndep = 0;
    if (a.match_only != 2) {
      for (int i = t; i < lm::kMaxKp; i += kLmThreads)
        S.s2[i] = (i < K2.n && K2.has_mp[i]) ? float_key(lm::scene_depth(S.P2.T, K2.mp_xyz + 3 * i))
                                            : kNoKey;
      __syncthreads();
      for (int r = t; r < nrec; r += kLmThreads) {
        const float4* src = reinterpret_cast<const float4*>(b.d_points + ob + r);
        const float4 h = src[0], x = src[1];
        if (__float_as_int(h.x) == nb) {
          const float X[3] = {x.x, x.y, x.z};
          S.s2[__float_as_int(h.z)] = float_key(lm::scene_depth(S.P2.T, X));
        }
      }
      __syncthreads();
      int cnt = 0;
      for (int i = t; i < K2.n; i += kLmThreads) cnt += S.s2[i] != kNoKey;
      ndep = block_sum<4>(cnt, S.wsum);
      int ns = 64;
      while (ns < K2.n) ns <<= 1;
      bitonic_sort(S.s2, ns, kLmThreads);
      if (ndep) median = key_float(S.s2[(ndep - 1) / 2]);
    }
    // LineMatcher::SearchForTriangulation: knnMatch k = 2 and the two medians
    const bool can = nl1 > 0 && nl2 >= 2 && (a.match_only == 2 || ndep > 0);
    int d12 = 0, best = -1;
    if (can && t < nl1) {
      const uint4 a0 = K1.ldesc[2 * t], a1 = K1.ldesc[2 * t + 1];
      int bi = -1, si = -1, db = 0, ds = 0;
      for (int j = 0; j < nl2; j++) {
        const int d = hamming256(a0, a1, K2.ldesc + 2 * j);
        if (bi < 0 || d < db) {
          si = bi;
          ds = db;
          bi = j;
          db = d;
        } else if (si < 0 || d < ds) {
          si = j;
          ds = d;
        }
      }
      best = bi;
      d12 = ds - db;
      atomicAdd(&S.lhist[0][d12], 1);
    }
    __syncthreads();
    if (t == 0 && can) S.l_med = hist_rank(S.lhist[0], nl1 / 2);
    __syncthreads();
    if (can && t < nl1) atomicAdd(&S.lhist[1][abs(d12 - S.l_med)], 1);
    __syncthreads();
    if (t == 0 && can) S.l_thr = lm::line_nn12_threshold(hist_rank(S.lhist[1], nl1 / 2));
    __syncthreads();
    const bool pass = can && t < nl1 && (double)(float)d12 > S.l_thr;
    const int np = block_sum<4>(pass ? 1 : 0, S.wsum);
    if (t == 0) b.d_line_pairs[p * lm::kNeighbours + nb] = np;
    if (a.match_only == 2) {
      int tot;
      const int pos = block_prefix<4>(pass, S.wsum, &tot);
      if (pass) *reinterpret_cast<int2*>(a.pairs_out + 2 * (lb + pos)) = make_int2(t, best);
      break;
    }
    bool made = false;
    float x6[6];
    if (pass) {
      const orbpl_keyline kl = K1.klines[t];
      made = lm::triangulate_line(a.c, S.P1, S.P2, S.M1, S.M2, K1.lcoef + 3 * t, K2.lcoef + 3 * best,
                                  kl.startPointX, kl.startPointY, kl.endPointX, kl.endPointY,
                                  median, x6);
    }
    int tot;
    const int pos = block_prefix<4>(made, S.wsum, &tot);
    if (made) {
      const int r = nlrec + pos;
      float4* dst = reinterpret_cast<float4*>(lines + r);
      dst[0] = make_float4(__int_as_float(nb), __int_as_float(t), __int_as_float(best),
                           __int_as_float(K1.id < K2.id ? 0 : 1));
      dst[1] = make_float4(x6[0], x6[1], x6[2], x6[3]);
      dst[2] = make_float4(x6[4], x6[5], 0.0f, 0.0f);
      b.d_kf1_line_record[lb + t] = r;   // AddMapLine: the last one owns the slot
    }
    nlrec += tot;
  }
  if (t == 0) b.d_n_lines[p] = nlrec;
}

int make_lm_consts(const orbpl_camera* cam, const float* scale, const float* sigma2, int nlevels,
                   lm::Consts* out) {
  if (!cam || !scale || !sigma2) return arg_fail("NULL camera or scale tables");
  if (nlevels < 2 || nlevels > lm::kMaxLevels) return arg_fail("nlevels outside [2, 16]");
  lm::Consts c{};
  c.fx = cam->fx; c.fy = cam->fy; c.cx = cam->cx; c.cy = cam->cy;
  c.invfx = 1.0f / cam->fx;
  c.invfy = 1.0f / cam->fy;
  c.bf = cam->bf;
  c.mb = cam->bf / cam->fx;
  c.ratio_factor = 1.5f * scale[1];
  c.nlevels = nlevels;
  for (int l = 0; l < nlevels; l++) {
    c.scale[l] = scale[l];
    c.sigma2[l] = sigma2[l];
  }
  *out = c;
  return ORBPL_OK;
}

int check_batch(const orblm_device_batch* b) {
  if (!b) return arg_fail("NULL batch");
  if (b->nkf < 1 || b->kp_pitch < 1 || b->kp_pitch > lm::kMaxKp)
    return arg_fail("nkf < 1 or kp_pitch outside [1, 2048]");
  if (b->line_pitch < 1 || b->line_pitch > lm::kMaxLines)
    return arg_fail("line_pitch outside [1, 256]");
  if (!b->d_kf_id || !b->d_kf_n || !b->d_kf_Tcw || !b->d_kps || !b->d_kps_un || !b->d_uright ||
      !b->d_depth || !b->d_desc || !b->d_feat_node || !b->d_has_mp || !b->d_mp_xyz ||
      !b->d_kf_nl || !b->d_klines || !b->d_ldesc || !b->d_lcoef || !b->d_cur || !b->d_neigh ||
      !b->d_points || !b->d_n_points || !b->d_kf1_point_record || !b->d_pairs || !b->d_lines ||
      !b->d_n_lines || !b->d_kf1_line_record || !b->d_line_pairs)
    return arg_fail("NULL device array");
  return ORBPL_OK;
}

}  // namespace
}  // namespace orbpl

using namespace orbpl;

namespace {

int check_keyframe(const orblm_keyframe& k, int nlevels, int reads) {
  if (!k.Tcw) return arg_fail("NULL keyframe pose");
  if (reads & kReadPoints) {
    if (k.n < 0 || k.n > lm::kMaxKp) return arg_fail("keyframe with more than 2048 features");
    if (k.n > 0 && (!k.kps || !k.kps_un || !k.uright || !k.depth || !k.desc || !k.feat_node ||
                    !k.has_mp || ((reads & kReadMapPoints) && !k.mp_xyz)))
      return arg_fail("NULL keyframe arrays");
    for (int i = 0; i < k.n; i++) {
      if (k.kps_un[i].octave < 0 || k.kps_un[i].octave >= nlevels)
        return arg_fail("keypoint octave outside [0, nlevels)");
      if (k.feat_node[i] >= (1 << 21) - 1) return arg_fail("vocabulary node id >= 2^21 - 1");
    }
  }
  if (reads & kReadLines) {
    if (k.nl < 0 || k.nl > lm::kMaxLines) return arg_fail("keyframe with more than 256 lines");
    if (k.nl > 0 && (!k.klines || !k.ldesc || !k.lcoef)) return arg_fail("NULL keyframe line arrays");
  }
  return ORBPL_OK;
}

// the pool of a host call (LmRows) with its staging
struct HostPool : LmRows {
  HostStage st;
  orblm_device_batch b{};

  // packs and stages the pool and the outputs of its problems into b; returns st.rc()
  int upload() {
    pack();
    b.nkf = (int)kfs.size();
    b.kp_pitch = pitch;
    b.line_pitch = lpitch;
    b.d_kf_id = st.in(id);
    b.d_kf_n = st.in(n);
    b.d_kf_Tcw = st.in(Tcw);
    b.d_kps = st.in(kps);
    b.d_kps_un = st.in(kps_un);
    b.d_uright = st.in(uright);
    b.d_depth = st.in(depth);
    b.d_desc = st.in(desc);
    b.d_feat_node = st.in(feat_node);
    b.d_has_mp = st.in(has_mp);
    b.d_mp_xyz = st.in(mp_xyz);
    b.d_kf_nl = st.in(nl);
    b.d_klines = st.in(klines);
    b.d_ldesc = st.in(ldesc);
    b.d_lcoef = st.in(lcoef);
    b.d_cur = st.in(cur);
    b.d_neigh = st.in(neigh);
    b.d_points = st.out(points);
    b.d_n_points = st.out(n_points);
    b.d_kf1_point_record = st.out(point_record);
    b.d_pairs = st.out(pairs);
    b.d_lines = st.out(lines);
    b.d_n_lines = st.out(n_lines);
    b.d_kf1_line_record = st.out(line_record);
    b.d_line_pairs = st.out(line_pairs);
    return st.rc();
  }
};

void launch(const LmArgs& a, int n, hipStream_t s) {
  hipLaunchKernelGGL(k_create_new_map_features, dim3(n), dim3(kLmThreads), 0, s, a);
}

}  // namespace

extern "C" {

int orblm_create_new_map_features_batch_device(const orbpl_camera* cam, const float* scale_factors,
                                               const float* level_sigma2, int nlevels,
                                               const orblm_device_batch* b, int n, void* stream) {
  LmArgs a{};
  int rc = make_lm_consts(cam, scale_factors, level_sigma2, nlevels, &a.c);
  if (rc) return rc;
  if (n < 0) return arg_fail("bad argument");
  rc = check_batch(b);
  if (rc) return rc;
  if (n == 0) return ORBPL_OK;
  a.b = *b;
  launch(a, n, static_cast<hipStream_t>(stream));
  HIP_CHECK(hipGetLastError());
  return ORBPL_OK;
}

int orblm_create_new_map_features(const orbpl_camera* cam, const float* scale_factors,
                                  const float* level_sigma2, int nlevels, orblm_problem* problems,
                                  int n) {
  LmArgs a{};
  int rc = make_lm_consts(cam, scale_factors, level_sigma2, nlevels, &a.c);
  if (rc) return rc;
  if (n < 0 || (n > 0 && !problems)) return arg_fail("bad argument");
  HostPool H;
  for (int p = 0; p < n; p++) {
    const orblm_problem& r = problems[p];
    if (r.n_neigh < 0 || r.n_neigh > lm::kNeighbours) return arg_fail("more than 10 neighbours");
    if (r.n_neigh > 0 && !r.neigh) return arg_fail("NULL neighbour list");
    if ((rc = check_keyframe(r.cur, nlevels, H.reads))) return rc;
    if (r.cur.n > 0 && (!r.points || !r.kf1_point_record)) return arg_fail("NULL output arrays");
    if (r.cur.nl > 0 && (!r.lines || !r.kf1_line_record)) return arg_fail("NULL output arrays");
    for (int k = 0; k < r.n_neigh; k++)
      if ((rc = check_keyframe(r.neigh[k], nlevels, H.reads))) return rc;
    H.add_problem(&r.cur, r.neigh, r.n_neigh);
  }
  if (n == 0) return ORBPL_OK;
  if ((rc = H.upload())) return rc;
  a.b = H.b;
  launch(a, n, nullptr);   // host-pointer APIs use the null stream
  H.st.launched();
  H.st.back_outs();
  if (H.st.rc()) return H.st.rc();
  H.unpack(problems);
  return ORBPL_OK;
}

int orbm_search_for_triangulation(const orbpl_camera* cam, const float* scale_factors,
                                  const float* level_sigma2, int nlevels,
                                  const orblm_keyframe* kf1, const orblm_keyframe* kf2,
                                  const float* f12_in, int only_stereo, int check_ori,
                                  int32_t* pairs, int* npairs, float* f12_out) {
  LmArgs a{};
  int rc = make_lm_consts(cam, scale_factors, level_sigma2, nlevels, &a.c);
  if (rc) return rc;
  if (!kf1 || !kf2 || !npairs) return arg_fail("bad argument");
  HostPool H;
  H.reads = kReadPoints;
  if ((rc = check_keyframe(*kf1, nlevels, H.reads)) || (rc = check_keyframe(*kf2, nlevels, H.reads)))
    return rc;
  if (kf1->n > 0 && !pairs) return arg_fail("NULL pairs");
  H.add_problem(kf1, kf2, 1);
  H.upload();
  a.b = H.b;
  a.match_only = 1;
  a.only_stereo = only_stereo != 0;
  a.check_ori = check_ori != 0;
  a.pairs_out = H.st.out<int32_t>(2 * (size_t)H.pitch);
  a.f12_out = H.st.out<float>(9);
  if (f12_in) {
    a.use_f12 = 1;
    std::copy(f12_in, f12_in + 9, a.f12_in);
  }
  if (H.st.rc()) return H.st.rc();
  launch(a, 1, nullptr);
  H.st.launched();
  H.st.back(H.pairs);
  if (H.st.rc()) return H.st.rc();
  *npairs = std::max(H.pairs.at(0), 0);
  H.st.back(pairs, a.pairs_out, 2 * (size_t)*npairs);
  if (f12_out) H.st.back(f12_out, a.f12_out, 9);
  return H.st.rc();
}

int orbl_search_for_triangulation(int nl1, const uint8_t* ldesc1, int nl2, const uint8_t* ldesc2,
                                  int32_t* pairs, int* npairs) {
  if (nl1 < 0 || nl2 < 0 || !npairs) return arg_fail("bad argument");
  if (nl1 > lm::kMaxLines || nl2 > lm::kMaxLines) return arg_fail("more than 256 lines");
  if ((nl1 > 0 && (!ldesc1 || !pairs)) || (nl2 > 0 && !ldesc2)) return arg_fail("NULL line arrays");
  // the matcher reads the descriptors only: a pose and empty geometry stand in
  const float eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  std::vector<orbpl_keyline> kl(std::max(1, std::max(nl1, nl2)));
  std::vector<double> lc((size_t)kl.size() * 3, 0.0);
  orblm_keyframe k1{}, k2{};
  k1.Tcw = k2.Tcw = eye;
  k1.nl = nl1;
  k1.ldesc = ldesc1;
  k2.nl = nl2;
  k2.ldesc = ldesc2;
  k1.klines = k2.klines = kl.data();
  k1.lcoef = k2.lcoef = lc.data();
  LmArgs a{};
  a.c.nlevels = 1;
  HostPool H;
  H.reads = kReadLines;
  H.add_problem(&k1, &k2, 1);
  H.upload();
  a.b = H.b;
  a.match_only = 2;
  a.pairs_out = H.st.out<int32_t>(2 * (size_t)H.lpitch);
  if (H.st.rc()) return H.st.rc();
  launch(a, 1, nullptr);
  H.st.launched();
  H.st.back(H.line_pairs);
  if (H.st.rc()) return H.st.rc();
  *npairs = std::max(H.line_pairs.at(0), 0);
  H.st.back(pairs, a.pairs_out, 2 * (size_t)*npairs);
  return H.st.rc();
}

}  // extern "C"
