// LocalMapping::KeyFrameCulling (LocalMapping.cc:1224-1319) with
// KeyFrame::SetBadFlag / EraseConnection / UpdateBestCovisibles (KeyFrame.cc:
// 526-650) and MapPoint::EraseObservation / SetBadFlag (MapPoint.cc:111-168),
// and LocalMapping::MapPointCulling / MapLineCulling (LocalMapping.cc:246-340),
// on gfx950, batched over independent maps of at most 64 keyframes: one
// 256-thread workgroup per map, the map mutated in device memory (DESIGN.md
// P48-P52). The observation rows are derived from the slot arrays at entry
// (map_rows.h, shared with search_neighbors.hip).
//
// k_keyframe_culling holds the map's weight rows (conn_w, 64 x 64) in LDS and
// walks the current keyframe's covisibility list in order. Per entry:
//   1. count, one slot per thread: the gates (null, bad, depth), nMPs, and for
//      a point with Observations() > 3 the observers at `octave <= level + 1`;
//      two block sums. Nothing is written.
//   2. the decision `nRedundant > 0.9 * nMPs` in double, uniform.
//   3. SetBadFlag: EraseConnection with one keyframe per wave (a lane per
//      candidate of its weight row, ranked by (weight, id) over 64 shuffles);
//      EraseObservation with one slot per thread (the slot points of a keyframe
//      are distinct, so the threads touch disjoint rows and slots); the
//      spanning-tree loop on wave 0, a lane per keyframe.
// Every store is a vector store.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/orbpl.h"
#include "block_ops.h"
#include "host_stage.h"
#include "map_pool.h"
#include "map_rows.h"
#include "orbpl_runtime.h"
#include "track_common.h"

namespace orbpl {
namespace {

constexpr int kKcThreads = 256;
constexpr int kKcList = ORBLM_MAX_CULL_LIST;
constexpr int kKcMaxLines = ORBLM_MAX_MAP_LINES;

struct KcShared {
  int cw[kMapKF * kMapKF];   // mConnectedKeyFrameWeights: row k at 64 k
  int id[kMapKF];
  int by_id[kMapKF];         // table index of the keyframe with id rank r
  int rank[kMapKF];
  int list[kKcList + 1];
  int wsum[4];
  int n_list;
};

// KeyFrame::EraseConnection(k) on every keyframe of k's weight row, one
// keyframe per wave: the keyframe drops k from its row and rebuilds its list
// from the whole row, weight descending, id descending on ties
__device__ void erase_connections(const orblm_kfc_device_batch& b, const SnView& V, KcShared& S, int k,
                                  int lane, int wave) {
  for (int j = wave; j < V.nkf; j += kKcThreads / 64) {
    if (S.cw[k * kMapKF + j] <= 0 || S.cw[j * kMapKF + k] <= 0) continue;   // uniform in the wave
    const int w = (lane < V.nkf && lane != k) ? S.cw[j * kMapKF + lane] : 0;
    const long long key = w > 0 ? ((long long)w << 6) | S.rank[lane] : -1;
    int pos = 0;
    for (int x = 0; x < kMapKF; x++) pos += __shfl(key, x, 64) > key;
    const int n = __popcll(__ballot(key >= 0));
    int32_t* ord = b.d_ordered + (long long)(V.kf0 + j) * kMapKF;
    if (key >= 0) ord[pos] = lane;
    if (lane >= n) ord[lane] = -1;
    if (lane == 0) S.cw[j * kMapKF + k] = 0;
  }
}

// MapPoint::EraseObservation(k) on every slot point of keyframe k, one slot
// per thread; returns the number of points this thread set bad
__device__ int erase_observations(const orblm_kfc_device_batch& b, const SnView& V, KcShared& S, int k) {
  const long long kb = (long long)(V.kf0 + k) * b.kp_pitch;
  const int nk = kf_count(b.d_kf_n, b.kp_pitch, V, k);
  int nbad = 0;
  for (int i = threadIdx.x; i < nk; i += kKcThreads) {
    const int m = b.d_mp[kb + i];
    if (m < 0) continue;
    const long long gm = (long long)V.mp0 + m;
    int16_t* row = b.d_obs + gm * kMapKF;
    const int idx = row[k];
    if (idx < 0) continue;   // the point does not observe the keyframe
    const int nobs = b.d_n_obs[gm] - (b.d_uright[kb + idx] >= 0.0f ? 2 : 1);
    b.d_n_obs[gm] = nobs;
    row[k] = -1;
    if (b.d_ref_kf[gm] == k) {   // the remaining observer with the lowest id, -1 none
      int nr = -1;
      for (int r = 0; r < V.nkf && nr < 0; r++) {
        const int kk = S.by_id[r];
        if (kk != k && row[kk] >= 0) nr = kk;
      }
      b.d_ref_kf[gm] = nr;
    }
    if (nobs <= 2) {   // MapPoint::SetBadFlag
      nbad += b.d_bad[gm] == 0;
      b.d_bad[gm] = 1;
      for (int kk = 0; kk < V.nkf; kk++) {
        const int i2 = kk == k ? -1 : (int)row[kk];
        if (i2 < 0) continue;
        b.d_mp[(long long)(V.kf0 + kk) * b.kp_pitch + i2] = -1;
        row[kk] = -1;
      }
    }
  }
  return nbad;
}

// the spanning-tree loop of KeyFrame::SetBadFlag, mTcp and mbBad, by wave 0:
// a lane per keyframe
__device__ void update_spanning_tree(const orblm_kfc_device_batch& b, const SnView& V, KcShared& S, int k,
                                     int lane) {
  int p0 = b.d_parent[V.kf0 + k];
  if (p0 >= V.nkf || p0 == k) p0 = -1;
  const bool in = lane < V.nkf;
  unsigned long long children = __ballot(in && lane != k && b.d_parent[V.kf0 + lane] == k);
  unsigned long long cand = p0 >= 0 ? 1ull << p0 : 0ull;
  const bool mybad = in ? b.d_kf_bad[V.kf0 + lane] != 0 : true;
  while (children) {
    long long key = -1;
    int myP = -1;
    if (((children >> lane) & 1) && !mybad) {
      int mx = -1;
      const int32_t* ord = b.d_ordered + (long long)(V.kf0 + lane) * kMapKF;
      for (int x = 0; x < kMapKF; x++) {
        const int c = ord[x];
        if (c < 0) break;
        if (c >= V.nkf || !((cand >> c) & 1)) continue;
        const int w = S.cw[lane * kMapKF + c];   // GetWeight: 0 if absent
        if (w > mx) {
          mx = w;
          myP = c;
        }
      }
      // the first child in id order wins a tie
      if (mx >= 0) key = ((long long)mx << 6) | (63 - S.rank[lane]);
    }
    long long best = key;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) best = max(best, __shfl_xor(best, o, 64));
    if (best < 0) break;
    const int C = S.by_id[63 - (int)(best & 63)];
    if (lane == C) b.d_parent[V.kf0 + lane] = myP;   // ChangeParent
    cand |= 1ull << C;
    children &= ~(1ull << C);
  }
  if ((children >> lane) & 1) b.d_parent[V.kf0 + lane] = p0;
  if (lane == 0) {
    if (p0 >= 0) {   // mTcp = Tcw * mpParent->GetPoseInverse()
      float Twc[16], Tcp[16];
      pose_inverse(b.d_kf_Tcw + (long long)(V.kf0 + p0) * 16, Twc);
      gemm44(b.d_kf_Tcw + (long long)(V.kf0 + k) * 16, Twc, Tcp);
      float4* dst = reinterpret_cast<float4*>(b.d_Tcp + (long long)(V.kf0 + k) * 16);
      for (int r = 0; r < 4; r++) dst[r] = make_float4(Tcp[4 * r], Tcp[4 * r + 1], Tcp[4 * r + 2], Tcp[4 * r + 3]);
    }
    b.d_kf_bad[V.kf0 + k] = 1;
  }
}

__global__ void __launch_bounds__(kKcThreads) k_keyframe_culling(orblm_kfc_device_batch b, float th_depth) {
  __shared__ KcShared S;
  const int t = threadIdx.x, p = blockIdx.x, lane = t & 63, wave = t >> 6;
  const SnView V = load_view(b.d_prob, p);
  orblm_kfc_result* R = b.d_result + p;
  int32_t* Ri = reinterpret_cast<int32_t*>(R);
  for (int i = t; i < (int)(sizeof(orblm_kfc_result) / 4); i += kKcThreads) Ri[i] = 0;
  // a range outside the pools, or no current keyframe: not run
  if (!view_in_pools(V, b.nkf, b.nmp) || V.cur < 0 || V.cur >= V.nkf) {
    if (t == 0) atomicOr(b.d_err, 1);
    return;
  }
  // ---- the map as the call sees it: observation rows from the slots ----
  const MapRows rows = {b.d_kf_n, b.d_uright, b.d_mp, b.d_n_obs, b.d_obs, b.kp_pitch, b.d_kf_bad};
  clear_observation_rows<kKcThreads>(rows, V);
  for (int m = t; m < V.nmp; m += kKcThreads) b.d_n_obs[V.mp0 + m] = 0;
  if (t < V.nkf) {
    S.id[t] = b.d_kf_id[V.kf0 + t];
    b.d_to_be_erased[V.kf0 + t] = 0;
  }
  for (int i = t; i < kMapKF * kMapKF; i += kKcThreads) {
    const int r = i >> 6, c = i & 63;
    S.cw[i] = (r < V.nkf && c < V.nkf && r != c) ? max(0, b.d_conn_w[(long long)(V.kf0 + r) * kMapKF + c]) : 0;
  }
  __syncthreads();
  rank_by_id(S.id, V.nkf, S.by_id, S.rank);
  derive_observation_rows<kKcThreads>(rows, V);
  // vpLocalKeyFrames, as copied before the loop
  if (t == 0) {
    const int32_t* o = b.d_ordered + (long long)(V.kf0 + V.cur) * kMapKF;
    unsigned long long seen = 1ull << V.cur;
    int n = 0;
    for (int x = 0; x < kMapKF; x++) {
      const int k = o[x];
      if (k < 0) break;
      if (k >= V.nkf || ((seen >> k) & 1)) continue;
      seen |= 1ull << k;
      S.list[n] = k;
      R->list[n++] = k;
    }
    S.n_list = n;
    R->n_list = n;
  }
  __syncthreads();
  const KeyPointD* kps = reinterpret_cast<const KeyPointD*>(b.d_kps_un);
  const int n_list = S.n_list;
  int nbad = 0;
  for (int e = 0; e < n_list; e++) {
    const int k = S.list[e];
    if (S.id[k] == 0) {
      if (t == 0) R->action[e] = ORBLM_KFC_FIRST;
      continue;
    }
    // ---- 1. the count: nothing is written ----
    const long long kb = (long long)(V.kf0 + k) * b.kp_pitch;
    const int nk = kf_count(b.d_kf_n, b.kp_pitch, V, k);
    int nmps = 0, nred = 0;
    for (int i = t; i < nk; i += kKcThreads) {
      const int m = b.d_mp[kb + i];
      if (m < 0) continue;
      const long long gm = (long long)V.mp0 + m;
      if (b.d_bad[gm]) continue;
      const float d = b.d_depth[kb + i];
      if (d > th_depth || d < 0.0f) continue;   // a NaN depth passes
      nmps++;
      if (b.d_n_obs[gm] > 3) {
        const int level = kps[kb + i].octave;
        const int16_t* row = b.d_obs + gm * kMapKF;
        int cnt = 0;
        for (int kk = 0; kk < V.nkf; kk++) {
          const int i2 = row[kk];
          if (kk == k || i2 < 0) continue;
          cnt += kps[(long long)(V.kf0 + kk) * b.kp_pitch + i2].octave <= level + 1;
        }
        nred += cnt >= 3;
      }
    }
    nmps = block_sum<kKcThreads / 64>(nmps, S.wsum);
    nred = block_sum<kKcThreads / 64>(nred, S.wsum);
    // ---- 2. the decision ----
    int action = ORBLM_KFC_KEPT;
    if ((double)nred > 0.9 * (double)nmps)
      action = b.d_not_erase[V.kf0 + k] ? ORBLM_KFC_DEFERRED : ORBLM_KFC_CULLED;
    if (t == 0) {
      R->n_mps[e] = nmps;
      R->n_redundant[e] = nred;
      R->action[e] = action;
      if (action == ORBLM_KFC_DEFERRED) b.d_to_be_erased[V.kf0 + k] = 1;
    }
    if (action != ORBLM_KFC_CULLED) continue;
    // ---- 3. KeyFrame::SetBadFlag ----
    erase_connections(b, V, S, k, lane, wave);
    __syncthreads();
    nbad += erase_observations(b, V, S, k);
    if (wave == 0) {
      update_spanning_tree(b, V, S, k, lane);
    } else if (wave == 1) {   // mConnectedKeyFrameWeights.clear(), mvpOrderedConnectedKeyFrames.clear()
      S.cw[k * kMapKF + lane] = 0;
      b.d_ordered[(long long)(V.kf0 + k) * kMapKF + lane] = -1;
    }
    __syncthreads();   // the map and the graph, before the next entry's count
  }
  nbad = block_sum<kKcThreads / 64>(nbad, S.wsum);
  if (t == 0) R->n_points_bad = nbad;
  for (int i = t; i < V.nkf * kMapKF; i += kKcThreads)
    b.d_conn_w[(long long)V.kf0 * kMapKF + i] = S.cw[i];
}

// ---------------------------------------------------------------------------
// MapPointCulling, then MapLineCulling
// ---------------------------------------------------------------------------
struct RcArgs {
  int nkf, kp_pitch, nmp, line_pitch;
  const int32_t* d_prob;    // (kf0, nkf, mp0, nmp, cur_id)
  const int32_t* d_ext;     // 6 per problem: recent offset / count, line offset / count, recent-line offset / count
  const int32_t* d_kf_n;
  const uint8_t* d_kf_bad;
  const float* d_uright;
  int32_t* d_mp;
  uint8_t* d_bad;
  const int32_t* d_n_visible;
  const int32_t* d_n_found;
  const int32_t* d_first_kf;
  int32_t* d_n_obs;
  int16_t* d_obs;
  const int32_t* d_recent;
  int32_t* d_recent_out;
  int32_t* d_reason;
  const int32_t* d_kf_nl;
  int32_t* d_ml;
  uint8_t* d_line_bad;
  const int32_t* d_line_n_visible;
  const int32_t* d_line_n_found;
  const int32_t* d_line_first_kf;
  const int32_t* d_line_n_obs;
  uint8_t* d_line_mark;     // zeroed: lines the call set bad
  const int32_t* d_recent_lines;
  int32_t* d_recent_lines_out;
  int32_t* d_line_reason;
  int32_t* d_n_out;         // 2 per problem: what remains of the two lists
};

// the four branches of the culling loops, in the reference's order
__device__ __forceinline__ int recent_reason(bool bad, int found, int visible, int age, int nobs) {
  if (bad) return ORBLM_RC_WAS_BAD;
  // GetFoundRatio(): float division; inf and NaN are not < 0.25f
  if ((float)found / (float)visible < 0.25f) return ORBLM_RC_FOUND_RATIO;
  if (age >= 2 && nobs <= 3) return ORBLM_RC_FEW_OBSERVATIONS;
  if (age >= 3) return ORBLM_RC_AGED_OUT;
  return ORBLM_RC_STAYS;
}

__global__ void __launch_bounds__(kKcThreads) k_cull_recent(RcArgs a) {
  __shared__ int wsum[4];
  const int t = threadIdx.x, p = blockIdx.x;
  const SnView V = load_view(a.d_prob, p);
  if (!view_in_pools(V, a.nkf, a.nmp)) return;
  const int cur_id = V.cur;
  const int32_t* ext = a.d_ext + 6 * p;
  const MapRows rows = {a.d_kf_n, a.d_uright, a.d_mp, a.d_n_obs, a.d_obs, a.kp_pitch, a.d_kf_bad};
  clear_observation_rows<kKcThreads>(rows, V);
  for (int m = t; m < V.nmp; m += kKcThreads) a.d_n_obs[V.mp0 + m] = 0;
  __syncthreads();
  derive_observation_rows<kKcThreads>(rows, V);
  __syncthreads();
  // ---- MapPointCulling: one list entry per thread, the rest an ordered compaction ----
  int nout = 0;
  for (int e0 = 0; e0 < ext[1]; e0 += kKcThreads) {
    const int e = e0 + t;
    bool stays = false;
    int m = -1;
    if (e < ext[1]) {
      m = a.d_recent[ext[0] + e];
      int reason = ORBLM_RC_WAS_BAD;
      if (m >= 0 && m < V.nmp) {
        const long long gm = (long long)V.mp0 + m;
        reason = recent_reason(a.d_bad[gm] != 0, a.d_n_found[gm], a.d_n_visible[gm],
                               cur_id - a.d_first_kf[gm], a.d_n_obs[gm]);
        if (reason == ORBLM_RC_FOUND_RATIO || reason == ORBLM_RC_FEW_OBSERVATIONS) {
          a.d_bad[gm] = 1;   // MapPoint::SetBadFlag: n_obs is kept
          int16_t* row = a.d_obs + gm * kMapKF;
          for (int kk = 0; kk < V.nkf; kk++) {
            const int i2 = row[kk];
            if (i2 < 0) continue;
            a.d_mp[(long long)(V.kf0 + kk) * a.kp_pitch + i2] = -1;
            row[kk] = -1;
          }
        }
      }
      a.d_reason[ext[0] + e] = reason;
      stays = reason == ORBLM_RC_STAYS;
    }
    int tot;
    const int pos = block_prefix<kKcThreads / 64>(stays, wsum, &tot);
    if (stays) a.d_recent_out[ext[0] + nout + pos] = m;
    nout += tot;
  }
  if (t == 0) a.d_n_out[2 * p] = nout;
  // ---- MapLineCulling ----
  const int l0 = ext[2], L = ext[3];
  nout = 0;
  for (int e0 = 0; e0 < ext[5]; e0 += kKcThreads) {
    const int e = e0 + t;
    bool stays = false;
    int l = -1;
    if (e < ext[5]) {
      l = a.d_recent_lines[ext[4] + e];
      int reason = ORBLM_RC_WAS_BAD;
      if (l >= 0 && l < L) {
        const int gl = l0 + l;
        reason = recent_reason(a.d_line_bad[gl] != 0, a.d_line_n_found[gl], a.d_line_n_visible[gl],
                               cur_id - a.d_line_first_kf[gl], a.d_line_n_obs[gl]);
        if (reason == ORBLM_RC_FOUND_RATIO || reason == ORBLM_RC_FEW_OBSERVATIONS) {
          a.d_line_bad[gl] = 1;
          a.d_line_mark[gl] = 1;
        }
      }
      a.d_line_reason[ext[4] + e] = reason;
      stays = reason == ORBLM_RC_STAYS;
    }
    int tot;
    const int pos = block_prefix<kKcThreads / 64>(stays, wsum, &tot);
    if (stays) a.d_recent_lines_out[ext[4] + nout + pos] = l;
    nout += tot;
  }
  if (t == 0) a.d_n_out[2 * p + 1] = nout;
  __syncthreads();   // the marks
  // MapLine::SetBadFlag's EraseMapLineMatch: every slot that names a line set bad
  for (int k = 0; k < V.nkf; k++) {
    const int nl = max(0, min(a.d_kf_nl[V.kf0 + k], a.line_pitch));
    int32_t* ml = a.d_ml + (long long)(V.kf0 + k) * a.line_pitch;
    for (int j = t; j < nl; j += kKcThreads) {
      const int l = ml[j];
      if (l >= L) ml[j] = -1;
      else if (l >= 0 && a.d_line_mark[l0 + l]) ml[j] = -1;
    }
  }
}

int check_kfc_batch(const orblm_kfc_device_batch* b) {
  if (!b) return arg_fail("NULL batch");
  if (b->nkf < 1 || b->kp_pitch < 1 || b->kp_pitch > kMapMaxKp)
    return arg_fail("nkf < 1 or kp_pitch outside [1, 2048]");
  if (b->nmp < 0) return arg_fail("nmp < 0");
  if (!b->d_prob || !b->d_kf_id || !b->d_kf_n || !b->d_kf_Tcw || !b->d_kps_un || !b->d_uright ||
      !b->d_depth || !b->d_mp || !b->d_conn_w || !b->d_ordered || !b->d_parent || !b->d_not_erase ||
      !b->d_kf_bad || !b->d_to_be_erased || !b->d_Tcp || !b->d_ref_kf || !b->d_bad || !b->d_n_obs ||
      !b->d_obs || !b->d_result || !b->d_err)
    return arg_fail("NULL device array");
  return ORBPL_OK;
}

}  // namespace
}  // namespace orbpl

using namespace orbpl;

namespace {

// the refusals of one problem's graph state (the map itself: check_map)
int check_graph(const orblm_kfc_problem& q) {
  const orblm_map& m = q.map;
  const int K = m.nkf;
  if (q.cur < 0 || q.cur >= K) return arg_fail("current keyframe outside the table");
  if (!q.depth || !q.conn_w || !q.ordered || !q.parent || !q.not_erase || !q.kf_bad || !q.to_be_erased ||
      !q.Tcp)
    return arg_fail("NULL graph arrays");
  for (int k = 0; k < K; k++) {
    if (m.kf[k].n > 0 && !q.depth[k]) return arg_fail("NULL graph arrays");
    for (int j = 0; j < K; j++) {
      if (q.conn_w[k * K + j] < 0) return arg_fail("negative covisibility weight");
      if (j == k && q.conn_w[k * K + j] != 0) return arg_fail("non-zero diagonal of conn_w");
    }
    unsigned long long seen = 0;
    for (int x = 0; x < kMapKF && q.ordered[k * kMapKF + x] >= 0; x++) {
      const int o = q.ordered[k * kMapKF + x];
      if (o >= K || o == k) return arg_fail("ordered entry outside the table or naming its own keyframe");
      if ((seen >> o) & 1) return arg_fail("ordered list names a keyframe twice");
      seen |= 1ull << o;
    }
    const int par = q.parent[k];
    if (par < -1 || par >= K || par == k)
      return arg_fail("parent outside the table or naming its own keyframe");
    if (par == -1 && m.kf[k].id != 0 && !q.kf_bad[k])
      return arg_fail("good keyframe with id != 0 and no parent");
  }
  return ORBPL_OK;
}

int shared_fail() { return arg_fail("a keyframe, point or graph array belongs to two problems"); }

// what both calls write of the map: the slots and bad (in/out), the observation rows (out)
constexpr uint32_t kCullIo = MapPool::kMp | MapPool::kBad, kCullOut = MapPool::kNObs | MapPool::kObs;

// after the launch: the device's copies of those columns into the pool, then
// back to the maps with the columns of `more`
int cull_download(MapPool& H, HostStage& st, uint32_t more, const int32_t* d_mp, const uint8_t* d_bad,
                  const int32_t* d_n_obs, const int16_t* d_obs) {
  H.pack(kCullOut);
  st.back(H.mp, d_mp);
  st.back(H.bad, d_bad);
  st.back(H.n_obs, d_n_obs);
  st.back(H.obs, d_obs);
  if (st.rc()) return st.rc();
  H.unpack(kCullIo | kCullOut | more);
  return ORBPL_OK;
}

}  // namespace

extern "C" {

int orblm_keyframe_culling_batch_device(const orbpl_camera* cam, const orblm_kfc_device_batch* b,
                                        int n, void* stream) {
  if (!cam) return arg_fail("NULL camera");
  if (n < 0) return arg_fail("bad argument");
  const int rc = check_kfc_batch(b);
  if (rc) return rc;
  if (n == 0) return ORBPL_OK;
  hipLaunchKernelGGL(k_keyframe_culling, dim3(n), dim3(kKcThreads), 0, static_cast<hipStream_t>(stream),
                     *b, cam->th_depth);
  HIP_CHECK(hipGetLastError());
  return ORBPL_OK;
}

int orblm_keyframe_culling(const orbpl_camera* cam, int nlevels, orblm_kfc_problem* problems, int n) {
  if (!cam) return arg_fail("NULL camera");
  if (nlevels < 1 || nlevels > 16) return arg_fail("nlevels outside [1, 16]");
  if (n < 0 || (n > 0 && !problems)) return arg_fail("bad argument");
  int rc;
  MapPool H;
  for (int p = 0; p < n; p++) {
    const orblm_kfc_problem& q = problems[p];
    const orblm_map& m = q.map;
    if ((rc = check_map(m, nlevels))) return rc;
    if ((rc = check_graph(q))) return rc;
    if (m.M) H.owned.push_back(m.bad);
    H.owned.insert(H.owned.end(), {q.conn_w, q.ordered, q.parent, q.kf_bad, q.to_be_erased, q.Tcp});
    H.add(m, q.cur);
  }
  if (H.shares_an_array()) return shared_fail();
  if (n == 0) return ORBPL_OK;
  H.pack(MapPool::kId | MapPool::kN | MapPool::kTcw | MapPool::kKpsUn | MapPool::kUright | MapPool::kRefKf |
         kCullIo);
  const size_t K = H.K(), P = H.P(), M = H.M(), N = (size_t)n;
  // the graph columns, at the pool's keyframe offsets
  std::vector<int32_t> hcw(K * kMapKF, 0), hord(K * kMapKF, -1), hpar(K);
  std::vector<float> hdepth(K * P, -1.0f);
  std::vector<uint8_t> hne(K), hkb(K);
  for (int p = 0; p < n; p++) {
    const orblm_kfc_problem& q = problems[p];
    const orblm_map& m = q.map;
    size_t g = H.kf0(p);
    for (int k = 0; k < m.nkf; k++, g++) {
      if (m.kf[k].n) memcpy(&hdepth[g * P], q.depth[k], (size_t)m.kf[k].n * 4);
      memcpy(&hcw[g * kMapKF], q.conn_w + (size_t)k * m.nkf, (size_t)m.nkf * 4);
      for (int x = 0; x < kMapKF && q.ordered[k * kMapKF + x] >= 0; x++)
        hord[g * kMapKF + x] = q.ordered[k * kMapKF + x];
      hpar[g] = q.parent[k];
      hne[g] = q.not_erase[k];
      hkb[g] = q.kf_bad[k];
    }
  }
  HostStage st;
  orblm_kfc_device_batch b{};
  b.nkf = H.nkf;
  b.kp_pitch = H.pitch;
  b.nmp = H.nmp;
  b.d_prob = st.in(H.prob);
  b.d_kf_id = st.in(H.id);
  b.d_kf_n = st.in(H.n);
  b.d_kf_Tcw = st.in(H.Tcw);
  b.d_kps_un = st.in(H.kps_un);
  b.d_uright = st.in(H.uright);
  b.d_depth = st.in(hdepth);
  b.d_mp = st.in(H.mp);
  b.d_conn_w = st.in(hcw);
  b.d_ordered = st.in(hord);
  b.d_parent = st.in(hpar);
  b.d_not_erase = st.in(hne);
  b.d_kf_bad = st.in(hkb);
  b.d_to_be_erased = st.zeros<uint8_t>(K);
  b.d_Tcp = st.zeros<float>(K * 16);
  b.d_ref_kf = st.in(H.ref_kf);
  b.d_bad = st.in(H.bad);
  b.d_n_obs = st.out<int32_t>(M);
  b.d_obs = st.out<int16_t>(M * kMapKF);
  b.d_result = st.out<orblm_kfc_result>(N);
  b.d_err = st.zeros<int32_t>(1);
  if (st.rc()) return st.rc();
  hipLaunchKernelGGL(k_keyframe_culling, dim3(n), dim3(kKcThreads), 0, nullptr, b, cam->th_depth);
  st.launched();
  std::vector<orblm_kfc_result> hres(N);
  std::vector<float> hTcp(K * 16);
  std::vector<uint8_t> htbe(K);
  st.back(hres, b.d_result);
  st.back(hcw, b.d_conn_w);
  st.back(hord, b.d_ordered);
  st.back(hpar, b.d_parent);
  st.back(hkb, b.d_kf_bad);
  st.back(htbe, b.d_to_be_erased);
  st.back(hTcp, b.d_Tcp);
  st.back(H.ref_kf, b.d_ref_kf);
  if ((rc = cull_download(H, st, MapPool::kRefKf, b.d_mp, b.d_bad, b.d_n_obs, b.d_obs))) return rc;
  for (int p = 0; p < n; p++) {
    orblm_kfc_problem& q = problems[p];
    const orblm_map& m = q.map;
    const size_t g0 = H.kf0(p);
    size_t g = g0;
    for (int k = 0; k < m.nkf; k++, g++) {
      memcpy(q.conn_w + (size_t)k * m.nkf, &hcw[g * kMapKF], (size_t)m.nkf * 4);
      memcpy(q.ordered + (size_t)k * kMapKF, &hord[g * kMapKF], kMapKF * 4);
      q.parent[k] = hpar[g];
      q.kf_bad[k] = hkb[g];
      q.to_be_erased[k] = htbe[g];
    }
    q.result = hres[p];
    for (int e = 0; e < q.result.n_list; e++)
      if (q.result.action[e] == ORBLM_KFC_CULLED) {
        const int k = q.result.list[e];
        memcpy(q.Tcp + (size_t)k * 16, &hTcp[(g0 + k) * 16], 64);
      }
  }
  return ORBPL_OK;
}

int orblm_cull_recent(int nlevels, orblm_recent_problem* problems, int n) {
  if (nlevels < 1 || nlevels > 16) return arg_fail("nlevels outside [1, 16]");
  if (n < 0 || (n > 0 && !problems)) return arg_fail("bad argument");
  int rc;
  std::vector<int32_t> ext;
  std::vector<uint8_t> seen;
  MapPool H;
  int nrec = 0, nlines = 0, nrl = 0, lpitch = 1;
  for (int p = 0; p < n; p++) {
    const orblm_recent_problem& q = problems[p];
    const orblm_map& m = q.map;
    if ((rc = check_map(m, nlevels))) return rc;
    if (q.n_recent < 0 || q.n_recent_lines < 0) return arg_fail("negative list length");
    if (q.L < 0 || q.L > kKcMaxLines) return arg_fail("map lines outside [0, 64 * 256]");
    if ((m.M > 0 && !q.first_kf) || (q.n_recent > 0 && (!q.recent || !q.reason)) ||
        (q.n_recent_lines > 0 && (!q.recent_lines || !q.line_reason)) || !q.nl || !q.ml ||
        (q.L > 0 && (!q.line_bad || !q.line_n_visible || !q.line_n_found || !q.line_first_kf ||
                     !q.line_n_obs)))
      return arg_fail("NULL culling arrays");
    seen.assign((size_t)m.M, 0);
    for (int e = 0; e < q.n_recent; e++) {
      const int x = q.recent[e];
      if (x < 0 || x >= m.M) return arg_fail("recent entry outside [0, M)");
      if (seen[x]) return arg_fail("recent entry repeats");
      seen[x] = 1;
    }
    seen.assign((size_t)q.L, 0);
    for (int e = 0; e < q.n_recent_lines; e++) {
      const int x = q.recent_lines[e];
      if (x < 0 || x >= q.L) return arg_fail("recent line entry outside [0, L)");
      if (seen[x]) return arg_fail("recent line entry repeats");
      seen[x] = 1;
    }
    for (int k = 0; k < m.nkf; k++) {
      if (q.nl[k] < 0 || q.nl[k] > ORBLM_MAX_LINES) return arg_fail("keyframe with more than 256 lines");
      if (q.nl[k] > 0 && !q.ml[k]) return arg_fail("NULL culling arrays");
      for (int j = 0; j < q.nl[k]; j++)
        if (q.ml[k][j] < -1 || q.ml[k][j] >= q.L) return arg_fail("line slot outside [-1, L)");
      if (q.nl[k]) H.owned.push_back(q.ml[k]);
      lpitch = std::max(lpitch, q.nl[k]);
    }
    if (m.M) H.owned.push_back(m.bad);
    if (q.L) H.owned.push_back(q.line_bad);
    if (q.n_recent) H.owned.insert(H.owned.end(), {q.recent, q.reason});
    if (q.n_recent_lines) H.owned.insert(H.owned.end(), {q.recent_lines, q.line_reason});
    ext.insert(ext.end(), {nrec, q.n_recent, nlines, q.L, nrl, q.n_recent_lines});
    nrec += q.n_recent;
    nlines += q.L;
    nrl += q.n_recent_lines;
    H.add(m, q.cur_id);
  }
  if (H.shares_an_array()) return shared_fail();
  if (n == 0) return ORBPL_OK;
  H.pack(MapPool::kN | MapPool::kUright | MapPool::kNVisible | MapPool::kNFound | kCullIo);
  const size_t K = H.K(), M = H.M(), LP = (size_t)lpitch, NL = (size_t)std::max(nlines, 1), N = (size_t)n;
  std::vector<int32_t> hfirst(M, 0), hrec((size_t)std::max(nrec, 1)), hnl(K), hml(K * LP, -1), hlvis(NL, 0),
      hlfound(NL, 0), hlfirst(NL, 0), hlnobs(NL, 0), hrl((size_t)std::max(nrl, 1));
  std::vector<uint8_t> hlbad(NL, 1), hkb(K, 0);
  for (int p = 0; p < n; p++) {
    const orblm_recent_problem& q = problems[p];
    const orblm_map& m = q.map;
    const size_t l0 = (size_t)ext[6 * p + 2];
    size_t g = H.kf0(p);
    if (m.M) memcpy(&hfirst[H.mp0(p)], q.first_kf, (size_t)m.M * 4);
    if (q.n_recent) memcpy(&hrec[(size_t)ext[6 * p]], q.recent, (size_t)q.n_recent * 4);
    if (q.n_recent_lines) memcpy(&hrl[(size_t)ext[6 * p + 4]], q.recent_lines, (size_t)q.n_recent_lines * 4);
    if (q.L) {
      const size_t nL = (size_t)q.L;
      memcpy(&hlbad[l0], q.line_bad, nL);
      memcpy(&hlvis[l0], q.line_n_visible, nL * 4);
      memcpy(&hlfound[l0], q.line_n_found, nL * 4);
      memcpy(&hlfirst[l0], q.line_first_kf, nL * 4);
      memcpy(&hlnobs[l0], q.line_n_obs, nL * 4);
    }
    for (int k = 0; k < m.nkf; k++, g++) {
      hnl[g] = q.nl[k];
      hkb[g] = q.kf_bad ? q.kf_bad[k] : 0;
      if (q.nl[k]) memcpy(&hml[g * LP], q.ml[k], (size_t)q.nl[k] * 4);
    }
  }
  HostStage st;
  RcArgs a{};
  a.nkf = H.nkf;
  a.kp_pitch = H.pitch;
  a.nmp = H.nmp;
  a.line_pitch = lpitch;
  a.d_prob = st.in(H.prob);
  a.d_ext = st.in(ext);
  a.d_kf_n = st.in(H.n);
  a.d_kf_bad = st.in(hkb);
  a.d_uright = st.in(H.uright);
  a.d_mp = st.in(H.mp);
  a.d_bad = st.in(H.bad);
  a.d_n_visible = st.in(H.n_visible);
  a.d_n_found = st.in(H.n_found);
  a.d_first_kf = st.in(hfirst);
  a.d_n_obs = st.out<int32_t>(M);
  a.d_obs = st.out<int16_t>(M * kMapKF);
  a.d_recent = st.in(hrec);
  a.d_recent_out = st.out<int32_t>(hrec.size());
  a.d_reason = st.out<int32_t>(hrec.size());
  a.d_kf_nl = st.in(hnl);
  a.d_ml = st.in(hml);
  a.d_line_bad = st.in(hlbad);
  a.d_line_n_visible = st.in(hlvis);
  a.d_line_n_found = st.in(hlfound);
  a.d_line_first_kf = st.in(hlfirst);
  a.d_line_n_obs = st.in(hlnobs);
  a.d_line_mark = st.zeros<uint8_t>(NL);
  a.d_recent_lines = st.in(hrl);
  a.d_recent_lines_out = st.out<int32_t>(hrl.size());
  a.d_line_reason = st.out<int32_t>(hrl.size());
  a.d_n_out = st.out<int32_t>(2 * N);
  if (st.rc()) return st.rc();
  hipLaunchKernelGGL(k_cull_recent, dim3(n), dim3(kKcThreads), 0, nullptr, a);
  st.launched();
  std::vector<int32_t> orec(hrec.size()), oreason(hrec.size()), orl(hrl.size()), olreason(hrl.size()),
      onout(2 * N);
  st.back(orec, a.d_recent_out);
  st.back(oreason, a.d_reason);
  st.back(orl, a.d_recent_lines_out);
  st.back(olreason, a.d_line_reason);
  st.back(onout, a.d_n_out);
  st.back(hml, a.d_ml);
  st.back(hlbad, a.d_line_bad);
  if ((rc = cull_download(H, st, 0, a.d_mp, a.d_bad, a.d_n_obs, a.d_obs))) return rc;
  for (int p = 0; p < n; p++) {
    orblm_recent_problem& q = problems[p];
    size_t g = H.kf0(p);
    const size_t r0 = (size_t)ext[6 * p], l0 = (size_t)ext[6 * p + 2], rl0 = (size_t)ext[6 * p + 4];
    if (q.n_recent) memcpy(q.reason, &oreason[r0], (size_t)q.n_recent * 4);
    if (q.n_recent_lines) memcpy(q.line_reason, &olreason[rl0], (size_t)q.n_recent_lines * 4);
    if (onout[2 * p]) memcpy(q.recent, &orec[r0], (size_t)onout[2 * p] * 4);
    if (onout[2 * p + 1]) memcpy(q.recent_lines, &orl[rl0], (size_t)onout[2 * p + 1] * 4);
    q.n_recent = onout[2 * p];
    q.n_recent_lines = onout[2 * p + 1];
    if (q.L) memcpy(q.line_bad, &hlbad[l0], (size_t)q.L);
    for (int k = 0; k < q.map.nkf; k++, g++)
      if (q.nl[k]) memcpy(q.ml[k], &hml[g * LP], (size_t)q.nl[k] * 4);
  }
  return ORBPL_OK;
}

}  // extern "C"
