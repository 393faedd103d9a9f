// The LocalMapping calls' view of a map (orblm_map), shared by
// search_neighbors.hip and keyframe_culling.hip: what a problem owns of the
// device pools, the observation rows derived from the keyframes' slot arrays,
// and the host-side refusals of one map.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/orbpl.h"
#include "orbpl_runtime.h"

namespace orbpl {

constexpr int kMapKF = ORBLM_MAX_MAP_KF;
constexpr int kMapMaxKp = ORBLM_MAX_KEYPOINTS;
constexpr int kMapMaxPoints = ORBLM_MAX_MAP_KF * ORBLM_MAX_KEYPOINTS;

// what a problem owns of the pools (d_prob: 5 ints per problem)
struct SnView {
  int kf0, nkf, mp0, nmp, cur;
};

__device__ __forceinline__ SnView load_view(const int32_t* d_prob, int p) {
  SnView V;
  V.kf0 = d_prob[5 * p];
  V.nkf = d_prob[5 * p + 1];
  V.mp0 = d_prob[5 * p + 2];
  V.nmp = d_prob[5 * p + 3];
  V.cur = d_prob[5 * p + 4];
  return V;
}

// a range inside pools of nkf keyframes and nmp points
__device__ __forceinline__ bool view_in_pools(const SnView& V, int nkf, int nmp) {
  return !(V.kf0 < 0 || V.nkf < 1 || V.nkf > kMapKF || V.kf0 + V.nkf > nkf || V.mp0 < 0 ||
           V.nmp < 0 || V.nmp > kMapMaxPoints || V.mp0 + V.nmp > nmp);
}

// the pools the observation rows are derived from (d_mp, per keyframe at
// kp_pitch) and into (d_obs: 64 feature indices per point, d_n_obs); d_kf_bad,
// if given: a bad keyframe keeps its slots, but its points do not observe it
struct MapRows {
  const int32_t* d_kf_n;
  const float* d_uright;
  int32_t* d_mp;
  int32_t* d_n_obs;
  int16_t* d_obs;
  int kp_pitch;
  const uint8_t* d_kf_bad;
};

__device__ __forceinline__ int kf_count(const int32_t* d_kf_n, int kp_pitch, const SnView& V, int k) {
  return max(0, min(d_kf_n[V.kf0 + k], min(kp_pitch, kMapMaxKp)));
}

// every row of the problem to "no observation", by a block of NT threads
template <int NT>
__device__ __forceinline__ void clear_observation_rows(const MapRows& r, const SnView& V) {
  for (long long i = threadIdx.x; i < (long long)V.nmp * 8; i += NT)
    reinterpret_cast<uint4*>(r.d_obs + (long long)V.mp0 * kMapKF)[i] =
        make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
}

// The rows and Observations() (a stereo observation counts 2) from the slot
// arrays. The caller has cleared the rows, zeroed d_n_obs and synchronised the
// block; a slot index outside the problem's points is set to -1.
template <int NT>
__device__ __forceinline__ void derive_observation_rows(const MapRows& r, const SnView& V) {
  for (int k = 0; k < V.nkf; k++) {
    const long long kb = (long long)(V.kf0 + k) * r.kp_pitch;
    const int nk = kf_count(r.d_kf_n, r.kp_pitch, V, k);
    if (r.d_kf_bad && r.d_kf_bad[V.kf0 + k]) continue;
    for (int i = threadIdx.x; i < nk; i += NT) {
      const int m = r.d_mp[kb + i];
      if (m < 0) continue;
      if (m >= V.nmp) {
        r.d_mp[kb + i] = -1;
        continue;
      }
      const long long gm = (long long)V.mp0 + m;
      r.d_obs[gm * kMapKF + k] = (int16_t)i;
      atomicAdd(&r.d_n_obs[gm], r.d_uright[kb + i] >= 0.0f ? 2 : 1);
    }
  }
}

// rank[k] of every keyframe in id order (table order on equal ids) and its
// inverse, by the first nkf threads; id[] is in LDS and synchronised
__device__ __forceinline__ void rank_by_id(const int* id, int nkf, int* by_id, int* rank_of) {
  const int t = threadIdx.x;
  if (t < nkf) {
    int rank = 0;
    for (int j = 0; j < nkf; j++) rank += id[j] < id[t] || (id[j] == id[t] && j < t);
    by_id[rank] = t;
    if (rank_of) rank_of[t] = rank;
  }
}

// the refusals of one map (before any device call)
inline int check_map(const orblm_map& m, int nlevels) {
  if (m.nkf < 1 || m.nkf > kMapKF) return arg_fail("map with no keyframe or more than 64");
  if (!m.kf) return arg_fail("NULL keyframe table");
  if (m.M < 0 || m.M > kMapMaxPoints) return arg_fail("map points outside [0, 64 * 2048]");
  if (m.M > 0 && (!m.xyz || !m.normal || !m.min_dist || !m.max_dist || !m.desc || !m.ref_kf ||
                  !m.bad || !m.n_visible || !m.n_found || !m.replaced_by || !m.n_obs || !m.obs ||
                  !m.desc_src))
    return arg_fail("NULL map point arrays");
  std::vector<int32_t> stamp((size_t)m.M, -1);   // the last keyframe a point was met in
  std::vector<uint8_t> ref_seen((size_t)m.M, 0);
  for (int k = 0; k < m.nkf; k++) {
    const orblm_map_keyframe& f = m.kf[k];
    if (!f.Tcw) return arg_fail("NULL keyframe pose");
    if (f.n < 0 || f.n > kMapMaxKp) return arg_fail("keyframe with more than 2048 features");
    if (f.n > 0 && (!f.kps_un || !f.uright || !f.desc || !f.mp)) return arg_fail("NULL keyframe arrays");
    for (int j = 0; j < k; j++)
      if (m.kf[j].id == f.id) return arg_fail("two keyframes of a map with one id");
    for (int i = 0; i < f.n; i++) {
      if (f.kps_un[i].octave < 0 || f.kps_un[i].octave >= nlevels)
        return arg_fail("keypoint octave outside [0, nlevels)");
      const int p = f.mp[i];
      if (p < -1 || p >= m.M) return arg_fail("slot index outside [-1, M)");
      if (p < 0) continue;
      if (stamp[p] == k) return arg_fail("map point twice in one keyframe");
      stamp[p] = k;
      if (m.ref_kf[p] == k) ref_seen[p] = 1;
    }
    if (f.ordered)
      for (int x = 0; x < kMapKF && f.ordered[x] >= 0; x++)
        if (f.ordered[x] >= m.nkf || f.ordered[x] == k)
          return arg_fail("ordered entry outside the table or naming its own keyframe");
  }
  for (int p = 0; p < m.M; p++)
    if (!m.bad[p] && !ref_seen[p]) return arg_fail("good map point whose ref_kf does not observe it");
  return ORBPL_OK;
}

}  // namespace orbpl
