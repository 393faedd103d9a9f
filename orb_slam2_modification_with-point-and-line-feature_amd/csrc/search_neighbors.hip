// LocalMapping::SearchInNeighbors (LocalMapping.cc:922-1103, the point half)
// with ORBmatcher::Fuse (ORBmatcher.cc:1107-1277), MapPoint::Replace
// (MapPoint.cc:177-229) and KeyFrame::UpdateConnections on gfx950, batched over
// independent maps of at most 64 keyframes: one 256-thread workgroup per map
// runs the up to 61 Fuse calls in list order and mutates the map in device
// memory. A map point's observations are a dense row of 64
// feature indices (one per keyframe of the table, -1 none), derived from the
// keyframes' slot arrays at entry.
//
// One Fuse call:
//   1. the keyframe's 64 x 48 cell table in LDS (build_frame_grid: cell starts
//      plus the keypoint indices sorted by (cell, index));
//   2. search, one list entry per thread: projection, the image / distance /
//      view gates, PredictScale, GetFeaturesInArea's window in (cell column,
//      cell row, index) order, the level and chi-square gates and the best
//      Hamming distance, first on ties. Nothing here depends on what the call
//      has done so far: a point's position, normal and distances never change
//      in Fuse, and its descriptor changes only when it survives a Replace,
//      after which it sits in the keyframe and is skipped;
//   3. commit, wave 0 alone, 64 entries at a time: the entries whose search
//      passed are visited in list order; isBad / IsInKeyFrame are lane
//      registers that every commit updates for the lanes behind it. Replace is
//      one lane per keyframe (each observation of the loser touches another
//      keyframe's slot), then ComputeDistinctiveDescriptors of the survivor as
//      an N x N Hamming block of the wave (descriptors exchanged by shuffles,
//      each lane sorts its own row in LDS; compute_distinctive's pin: median
//      index (int)(0.5 (N - 1)), first observer in keyframe-id order on ties).
// Then the backward candidate list (per target an ordered block compaction;
// a point sits once in a keyframe, so first-occurrence dedup only has to look
// at earlier targets: a mark byte per point), one more Fuse into the current
// keyframe, ComputeDistinctiveDescriptors + UpdateNormalAndDepth of the
// current keyframe's points (one wave per point) and UpdateConnections.
// update_normal_depth / compute_distinctive of map_kernels.hip read the map
// model's pools (observation lists in creation order, the first one the
// reference keyframe); here the reference keyframe is a field and the
// observations a dense row, so both are restated on that layout.
// Every store is a vector store.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/orbpl.h"
#include "block_ops.h"
#include "host_stage.h"
#include "lsd_math.h"
#include "map_pool.h"
#include "map_rows.h"
#include "match_common.h"
#include "orbpl_runtime.h"
#include "track_kernels.h"

namespace orbpl {
namespace {

constexpr int kSnThreads = 256;
constexpr int kSnKF = ORBLM_MAX_MAP_KF;
constexpr int kSnMaxKp = ORBLM_MAX_KEYPOINTS;
constexpr int kSnThLow = 50;          // ORBmatcher::TH_LOW
constexpr int kSearchPass = 15;       // the search found bestDist <= TH_LOW

struct SnArgs {
  TrackConsts c;
  float log_scale;
  orblm_sin_device_batch b;
  int fuse_only;     // orbm_fuse: one Fuse(kf, d_list[0, n_list), th) per problem
  int fuse_kf, fuse_n;
  float th;
  int32_t* d_fuse_out;   // fuse_only: 3 * list_pitch per problem (best_idx, best_dist, reason)
  long long* d_ticks;    // profiling: 3 per problem (search, commit, whole call), 100 MHz ticks, or NULL
};

struct SnShared {
  union {
    struct {
      int cell_start[kGridCols * kGridRows + 1];
      int fill[kGridCols * kGridRows];
    } g;
    uint16_t drow_hi[kSnThreads / 64 - 1][64 * 64];   // step 5, waves 1-3: the grid is done with
  } u;
  uint16_t items[kSnMaxKp];
  int16_t gc[kSnMaxKp];
  uint16_t drow0[64 * 64];                   // [j * 64 + lane]: lane's distance row (wave 0)
  int ob[kSnThreads / 64][64];               // [wave][i]: i-th observer (keyframe << 16 | feature)
  float Ow[kSnKF][3];
  int by_id[kSnKF];                          // table index of the keyframe with id rank r
  int id[kSnKF];
  int cnt[kSnKF];
  int targets[ORBLM_MAX_TARGETS];
  int wsum[4];
  int n_targets, n_fused;
  long long ticks[2];
};

__device__ __forceinline__ int pack_search(int reason, int dist, int idx) {
  return (reason << 24) | (dist << 12) | (idx & 0xfff);
}

// the wave's global and LDS stores so far are visible to its other lanes
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int kf_count(const orblm_sin_device_batch& b, const SnView& V, int k) {
  return kf_count(b.d_kf_n, b.kp_pitch, V, k);
}

// The observers of point m (global index gm) in keyframe-id order, one per
// lane: returns N; lane i < N gets observer i as (keyframe << 16 | feature).
__device__ __forceinline__ int wave_observers(const orblm_sin_device_batch& b, const SnView& V,
                                              SnShared& S, long long gm, int lane, int wave,
                                              int* mine) {
  const int k = lane < V.nkf ? S.by_id[lane] : -1;
  const int idx = k >= 0 ? (int)b.d_obs[gm * kSnKF + k] : -1;
  const unsigned long long mask = __ballot(idx >= 0);
  const int N = __popcll(mask);
  if (idx >= 0) S.ob[wave][__popcll(mask & ((1ull << lane) - 1ull))] = (k << 16) | idx;
  wave_sync();
  *mine = lane < N ? S.ob[wave][lane] : -1;
  wave_sync();
  return N;
}

// MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:256-321) of point m by
// one wave
__device__ void wave_distinctive(const orblm_sin_device_batch& b, const SnView& V, SnShared& S,
                                 int m, int lane, int wave) {
  const long long gm = (long long)V.mp0 + m;
  int mine;
  const int N = wave_observers(b, V, S, gm, lane, wave, &mine);
  if (N == 0) return;
  uint4 x0 = make_uint4(0, 0, 0, 0), x1 = x0;
  if (mine >= 0) {
    const uint4* d = reinterpret_cast<const uint4*>(
        b.d_desc + ((long long)(V.kf0 + (mine >> 16)) * b.kp_pitch + (mine & 0xffff)) * 32);
    x0 = d[0];
    x1 = d[1];
  }
  uint16_t* row = wave == 0 ? S.drow0 : S.u.drow_hi[wave - 1];
  for (int j = 0; j < N; j++) {
    uint4 y0, y1;
    y0.x = __shfl(x0.x, j, 64); y0.y = __shfl(x0.y, j, 64);
    y0.z = __shfl(x0.z, j, 64); y0.w = __shfl(x0.w, j, 64);
    y1.x = __shfl(x1.x, j, 64); y1.y = __shfl(x1.y, j, 64);
    y1.z = __shfl(x1.z, j, 64); y1.w = __shfl(x1.w, j, 64);
    row[j * 64 + lane] = (uint16_t)hamming256(x0, x1, y0, y1);
  }
  int key = 0x7fffffff;
  if (lane < N) {
    for (int x = 1; x < N; x++) {
      const uint16_t v = row[x * 64 + lane];
      int y = x - 1;
      while (y >= 0 && row[y * 64 + lane] > v) {
        row[(y + 1) * 64 + lane] = row[y * 64 + lane];
        y--;
      }
      row[(y + 1) * 64 + lane] = v;
    }
    const int med = (int)(0.5 * (double)(N - 1));
    key = ((int)row[med * 64 + lane] << 8) | lane;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) key = min(key, __shfl_xor(key, o, 64));
  if (lane == (key & 0xff)) {
    uint4* dst = reinterpret_cast<uint4*>(b.d_mp_desc + gm * 32);
    dst[0] = x0;
    dst[1] = x1;
    *reinterpret_cast<int2*>(b.d_desc_src + gm * 2) = make_int2(mine >> 16, mine & 0xffff);
  }
  wave_sync();
}

// MapPoint::UpdateNormalAndDepth (MapPoint.cc:344-385, P25) of point m by one
// wave, with the explicit reference keyframe
__device__ void wave_normal_depth(const SnArgs& a, const SnView& V, SnShared& S, int m, int lane,
                                  int wave) {
  const orblm_sin_device_batch& b = a.b;
  const long long gm = (long long)V.mp0 + m;
  int mine;
  const int N = wave_observers(b, V, S, gm, lane, wave, &mine);
  if (N == 0) return;
  const float X[3] = {b.d_xyz[gm * 3], b.d_xyz[gm * 3 + 1], b.d_xyz[gm * 3 + 2]};
  float v[3] = {0.f, 0.f, 0.f};
  if (mine >= 0) {
    const float* Ow = S.Ow[mine >> 16];
    const float d[3] = {X[0] - Ow[0], X[1] - Ow[1], X[2] - Ow[2]};
    const float inv =
        (float)(1.0 / sqrt((double)d[0] * d[0] + (double)d[1] * d[1] + (double)d[2] * d[2]));
    for (int q = 0; q < 3; q++) v[q] = d[q] * inv;
  }
  float nrm[3] = {0.f, 0.f, 0.f};
  for (int r = 0; r < N; r++)
    for (int q = 0; q < 3; q++) nrm[q] = nrm[q] + __shfl(v[q], r, 64);
  if (lane == 0) {
    const int rk = max(0, min(b.d_ref_kf[gm], V.nkf - 1));
    const int ridx = max(0, (int)b.d_obs[gm * kSnKF + rk]);
    const float* Ow = S.Ow[rk];
    const float PC[3] = {X[0] - Ow[0], X[1] - Ow[1], X[2] - Ow[2]};
    const float dist =
        (float)sqrt((double)PC[0] * PC[0] + (double)PC[1] * PC[1] + (double)PC[2] * PC[2]);
    const KeyPointD* kp =
        reinterpret_cast<const KeyPointD*>(b.d_kps_un) + (long long)(V.kf0 + rk) * b.kp_pitch + ridx;
    const int level = max(0, min(kp->octave, a.c.nlevels - 1));
    const float mx = dist * a.c.scale[level];
    b.d_max_dist[gm] = mx;
    b.d_min_dist[gm] = mx / a.c.scale[a.c.nlevels - 1];
    const float fn = (float)N;
    b.d_normal[gm * 3] = nrm[0] / fn;
    b.d_normal[gm * 3 + 1] = nrm[1] / fn;
    b.d_normal[gm * 3 + 2] = nrm[2] / fn;
  }
}

// loser->Replace(survivor) by one wave, one lane per keyframe
__device__ void wave_replace(const orblm_sin_device_batch& b, const SnView& V, SnShared& S, int loser,
                             int surv, int lane, int wave) {
  const long long gl = (long long)V.mp0 + loser, gs = (long long)V.mp0 + surv;
  int add = 0;
  if (lane < V.nkf) {
    const int idx = b.d_obs[gl * kSnKF + lane];
    if (idx >= 0) {
      const long long slot = (long long)(V.kf0 + lane) * b.kp_pitch + idx;
      if (b.d_obs[gs * kSnKF + lane] >= 0) {
        b.d_mp[slot] = -1;   // EraseMapPointMatch: the survivor is in this keyframe already
      } else {
        b.d_mp[slot] = surv;   // ReplaceMapPointMatch + AddObservation
        b.d_obs[gs * kSnKF + lane] = (int16_t)idx;
        add = b.d_uright[slot] >= 0.0f ? 2 : 1;
      }
      b.d_obs[gl * kSnKF + lane] = -1;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) add += __shfl_xor(add, o, 64);
  if (lane == 0) {
    b.d_n_obs[gs] += add;
    b.d_n_obs[gl] = 0;
    b.d_bad[gl] = 1;
    b.d_replaced_by[gl] = surv;
    b.d_n_found[gs] += b.d_n_found[gl];
    b.d_n_visible[gs] += b.d_n_visible[gl];
  }
  wave_sync();
  wave_distinctive(b, V, S, surv, lane, wave);
}

// steps 1 and 2 of a Fuse call into keyframe k over list[0, n): d_search per entry
__device__ void fuse_search(const SnArgs& a, const SnView& V, SnShared& S, int k, const int32_t* list,
                            int n, int32_t* search, float th) {
  const orblm_sin_device_batch& b = a.b;
  const TrackConsts& c = a.c;
  const int t = threadIdx.x;
  const long long kb = (long long)(V.kf0 + k) * b.kp_pitch;
  const KeyPointD* kps = reinterpret_cast<const KeyPointD*>(b.d_kps_un) + kb;
  const float* uright = b.d_uright + kb;
  const uint4* kdesc = reinterpret_cast<const uint4*>(b.d_desc + kb * 32);
  const int nk = kf_count(b, V, k);
  build_frame_grid<kSnThreads>(S.u.g.cell_start, S.items, S.gc, S.u.g.fill, S.wsum, nk, [&](int i) {
    const KeyPointD kp = kps[i];
    // Frame::PosInGrid (Frame.cc:527-538)
    const int px = (int)roundf((kp.x - c.minX) * c.gridInvW);
    const int py = (int)roundf((kp.y - c.minY) * c.gridInvH);
    return (px < 0 || px >= kGridCols || py < 0 || py >= kGridRows) ? -1 : px * kGridRows + py;
  });
  const float* T = b.d_kf_Tcw + (long long)(V.kf0 + k) * 16;
  const float* Ow = S.Ow[k];
  for (int e = t; e < n; e += kSnThreads) {
    const int m = list[e];
    if (m < 0 || m >= V.nmp) {
      search[e] = pack_search(ORBM_FUSE_NULL, 256, -1);
      continue;
    }
    const long long gm = (long long)V.mp0 + m;
    const float P[3] = {b.d_xyz[gm * 3], b.d_xyz[gm * 3 + 1], b.d_xyz[gm * 3 + 2]};
    float Pc[3];
    gemm_R_x_plus_t(T, P, Pc);
    int reason = kSearchPass, best_dist = 256, best_idx = -1;
    do {
      if (Pc[2] < 0.0f) {
        reason = ORBM_FUSE_BEHIND;
        break;
      }
      const float invz = 1.0f / Pc[2];
      const float x = Pc[0] * invz, y = Pc[1] * invz;
      const float u = c.fx * x + c.cx, v = c.fy * y + c.cy;
      if (!(u >= c.minX && u < c.maxX && v >= c.minY && v < c.maxY)) {
        reason = ORBM_FUSE_OUT_OF_IMAGE;
        break;
      }
      const float ur = u - c.bf * invz;
      const float maxd = 1.2f * b.d_max_dist[gm], mind = 0.8f * b.d_min_dist[gm];
      const float PO[3] = {P[0] - Ow[0], P[1] - Ow[1], P[2] - Ow[2]};
      // cv::norm (P16): double squares, one rounding
      const float dist =
          (float)sqrt((double)PO[0] * PO[0] + (double)PO[1] * PO[1] + (double)PO[2] * PO[2]);
      if (dist < mind || dist > maxd) {
        reason = ORBM_FUSE_DISTANCE;
        break;
      }
      // Mat::dot (P16): float products, double sum; the comparison is in double
      double dot = 0;
      for (int q = 0; q < 3; q++) dot += (double)(float)(PO[q] * b.d_normal[gm * 3 + q]);
      if (dot < 0.5 * (double)dist) {
        reason = ORBM_FUSE_VIEW;
        break;
      }
      int level = 0;
      if (c.nlevels > 1) {   // MapPoint::PredictScale (MapPoint.cc:399-414, P15)
        const float ratio = b.d_max_dist[gm] / dist;
        level = (int)ceilf((float)lsdm::log_((double)ratio) / a.log_scale);
        level = level < 0 ? 0 : (level >= c.nlevels ? c.nlevels - 1 : level);
      }
      const float r = th * c.scale[level];
      int cx0, cx1, cy0, cy1;
      bool any = false;
      if (grid_window(c, u, v, r, &cx0, &cx1, &cy0, &cy1)) {
        const uint4* md = reinterpret_cast<const uint4*>(b.d_mp_desc + gm * 32);
        const uint4 d0 = md[0], d1 = md[1];
        for (int ix = cx0; ix <= cx1; ix++)
          for (int iy = cy0; iy <= cy1; iy++) {
            const int cell = ix * kGridRows + iy;
            for (int q = S.u.g.cell_start[cell]; q < S.u.g.cell_start[cell + 1]; q++) {
              const int idx = S.items[q];
              const KeyPointD kp = kps[idx];
              if (!(fabsf(kp.x - u) < r && fabsf(kp.y - v) < r)) continue;
              any = true;
              if (kp.octave < level - 1 || kp.octave > level) continue;
              const float inv_s2 = c.inv_sigma2[max(0, min(kp.octave, c.nlevels - 1))];
              const float ex = u - kp.x, ey = v - kp.y;
              const float kr = uright[idx];
              if (kr >= 0.0f) {
                const float er = ur - kr;
                const float e2 = ex * ex + ey * ey + er * er;
                if ((double)(e2 * inv_s2) > 7.8) continue;
              } else {
                const float e2 = ex * ex + ey * ey;
                if ((double)(e2 * inv_s2) > 5.99) continue;
              }
              const int d = hamming256(d0, d1, kdesc + 2 * idx);
              if (d < best_dist) {
                best_dist = d;
                best_idx = idx;
              }
            }
          }
      }
      if (!any) reason = ORBM_FUSE_EMPTY_WINDOW;
      else if (best_dist > kSnThLow) reason = ORBM_FUSE_NO_MATCH;
    } while (false);
    search[e] = pack_search(reason, best_dist, best_idx);
  }
  __syncthreads();
}

// step 3 of a Fuse call, by wave 0; returns nFused on every lane of wave 0
__device__ int fuse_commit(const SnArgs& a, const SnView& V, SnShared& S, int k, const int32_t* list,
                           int n, const int32_t* search, int32_t* out, int lane) {
  const orblm_sin_device_batch& b = a.b;
  const long long kb = (long long)(V.kf0 + k) * b.kp_pitch;
  int nfused = 0;
  for (int base = 0; base < n; base += 64) {
    const int e = base + lane;
    const int pk = e < n ? search[e] : pack_search(ORBM_FUSE_NULL, 256, -1);
    int m = e < n ? list[e] : -1;
    if (m >= V.nmp) m = -1;
    const int greason = pk >> 24;
    int st_bad = 0, st_in = 0, fin = -1;
    if (m >= 0) {
      const long long gm = (long long)V.mp0 + m;
      st_bad = b.d_bad[gm] != 0;
      st_in = b.d_obs[gm * kSnKF + k] >= 0;
    }
    unsigned long long pending = __ballot(m >= 0 && greason == kSearchPass);
    while (pending) {
      const int p = __ffsll((long long)pending) - 1;
      pending &= pending - 1;
      if (__shfl(st_bad, p, 64) || __shfl(st_in, p, 64)) continue;
      const int mm = __shfl(m, p, 64);
      const int bi = __shfl(pk, p, 64) & 0xfff;
      const int q = b.d_mp[kb + bi];
      int code, lost = -1, gained = mm;
      if (q >= 0 && q < V.nmp) {
        if (!b.d_bad[V.mp0 + q]) {
          if (b.d_n_obs[V.mp0 + q] > b.d_n_obs[V.mp0 + mm]) {
            wave_replace(b, V, S, mm, q, lane, 0);
            code = ORBM_FUSE_REPLACED;
            lost = mm;
            gained = q;
          } else {
            wave_replace(b, V, S, q, mm, lane, 0);
            code = ORBM_FUSE_REPLACES;
            lost = q;
          }
        } else {
          code = ORBM_FUSE_BAD_SLOT;
          gained = -1;
        }
      } else {
        if (lane == 0) {
          b.d_obs[((long long)V.mp0 + mm) * kSnKF + k] = (int16_t)bi;
          b.d_mp[kb + bi] = mm;
          b.d_n_obs[V.mp0 + mm] += b.d_uright[kb + bi] >= 0.0f ? 2 : 1;
        }
        wave_sync();
        code = ORBM_FUSE_ADDED;
      }
      nfused++;
      if (lane == p) fin = code;
      if (lane > p && m >= 0) {
        if (m == lost) st_bad = 1;
        if (m == gained) st_in = 1;
      }
    }
    if (out && e < n) {
      int reason = fin;
      if (m < 0) reason = ORBM_FUSE_NULL;
      else if (fin < 0) reason = st_bad ? ORBM_FUSE_BAD : st_in ? ORBM_FUSE_IN_KF : greason;
      const bool ran = reason >= ORBM_FUSE_NO_MATCH;
      const int bi = pk & 0xfff;
      out[e] = ran && bi != 0xfff ? bi : -1;
      out[b.list_pitch + e] = ran ? (pk >> 12) & 0xfff : 256;
      out[2 * b.list_pitch + e] = reason;
    }
    wave_sync();
  }
  return nfused;
}

// ORBmatcher::Fuse(keyframe k, list[0, n), th): nFused in S.n_fused
__device__ void fuse_call(const SnArgs& a, const SnView& V, SnShared& S, int k, const int32_t* list,
                          int n, int32_t* search, int32_t* out, float th) {
  const long long t0 = a.d_ticks ? (long long)wall_clock64() : 0;
  fuse_search(a, V, S, k, list, n, search, th);
  const long long t1 = a.d_ticks ? (long long)wall_clock64() : 0;
  if (threadIdx.x < 64) {
    const int nf = fuse_commit(a, V, S, k, list, n, search, out, threadIdx.x);
    if (threadIdx.x == 0) S.n_fused = nf;
  }
  __syncthreads();
  if (a.d_ticks && threadIdx.x == 0) {
    S.ticks[0] += t1 - t0;
    S.ticks[1] += (long long)wall_clock64() - t1;
  }
}

__global__ void __launch_bounds__(kSnThreads) k_search_in_neighbors(SnArgs a) {
  __shared__ SnShared S;
  const orblm_sin_device_batch& b = a.b;
  const int t = threadIdx.x, p = blockIdx.x, lane = t & 63, wave = t >> 6;
  const SnView V = load_view(b.d_prob, p);
  orblm_sin_result* R = b.d_result + p;
  int32_t* Ri = reinterpret_cast<int32_t*>(R);
  for (int i = t; i < (int)(sizeof(orblm_sin_result) / 4); i += kSnThreads) Ri[i] = 0;
  // a range outside the pools, or no current keyframe: nothing to do
  if (!view_in_pools(V, b.nkf, b.nmp)) return;
  const int kf = a.fuse_only ? a.fuse_kf : V.cur;
  if (kf < 0 || kf >= V.nkf) return;
  int32_t* list = b.d_list + (long long)p * b.list_pitch;
  int32_t* search = b.d_search + (long long)p * b.list_pitch;
  // ---- the map as the call sees it: observation rows from the slots ----
  const MapRows rows = {b.d_kf_n, b.d_uright, b.d_mp, b.d_n_obs, b.d_obs, b.kp_pitch, nullptr};
  clear_observation_rows<kSnThreads>(rows, V);
  for (int m = t; m < V.nmp; m += kSnThreads) {
    const long long gm = (long long)V.mp0 + m;
    b.d_replaced_by[gm] = -1;
    b.d_n_obs[gm] = 0;
    b.d_mark[gm] = 0;
    *reinterpret_cast<int2*>(b.d_desc_src + gm * 2) = make_int2(-1, -1);
  }
  const long long t_begin = a.d_ticks ? (long long)wall_clock64() : 0;
  if (t == 0) S.ticks[0] = S.ticks[1] = 0;
  if (t < kSnKF) {
    S.cnt[t] = 0;
    if (t < V.nkf) {
      gemm_neg_Rt_t(b.d_kf_Tcw + (long long)(V.kf0 + t) * 16, S.Ow[t]);
      S.id[t] = b.d_kf_id[V.kf0 + t];
    }
  }
  __syncthreads();
  rank_by_id(S.id, V.nkf, S.by_id, nullptr);
  derive_observation_rows<kSnThreads>(rows, V);
  __syncthreads();
  if (a.fuse_only) {
    const int n = max(0, min(a.fuse_n, b.list_pitch));
    fuse_call(a, V, S, kf, list, n, search, a.d_fuse_out + (long long)p * 3 * b.list_pitch, a.th);
    if (t == 0) R->n_fused[0] = S.n_fused;
    return;
  }
  // ---- vpTargetKFs (LocalMapping.cc:931-965): only first neighbours are marked ----
  const int cur = V.cur;
  if (t == 0) {
    unsigned long long marked = 0;
    int nt = 0;
    const int32_t* o1 = b.d_ordered + (long long)(V.kf0 + cur) * kSnKF;
    for (int x = 0; x < 10; x++) {
      const int k1 = o1[x];
      if (k1 < 0) break;
      if (k1 >= V.nkf || k1 == cur || ((marked >> k1) & 1)) continue;
      S.targets[nt++] = k1;
      marked |= 1ull << k1;
      const int32_t* o2 = b.d_ordered + (long long)(V.kf0 + k1) * kSnKF;
      for (int y = 0; y < 5; y++) {
        const int k2 = o2[y];
        if (k2 < 0) break;
        if (k2 >= V.nkf || k2 == cur || ((marked >> k2) & 1)) continue;
        S.targets[nt++] = k2;
      }
    }
    S.n_targets = nt;
    R->n_targets = nt;
    for (int x = 0; x < nt; x++) R->targets[x] = S.targets[x];
  }
  // vpMapPointMatches, as copied before the loop
  const long long cb = (long long)(V.kf0 + cur) * b.kp_pitch;
  const int ncur = kf_count(b, V, cur);
  for (int i = t; i < ncur; i += kSnThreads) list[i] = b.d_mp[cb + i];
  __syncthreads();
  const int nt = S.n_targets;
  for (int x = 0; x < nt; x++) {
    fuse_call(a, V, S, S.targets[x], list, ncur, search, nullptr, a.th);
    if (t == 0) R->n_fused[x] = S.n_fused;
  }
  // ---- vpFuseCandidates: target by target, slot by slot, first occurrence ----
  int ncand = 0;
  bool over = false;
  for (int x = 0; x < nt; x++) {
    const int k = S.targets[x];
    const long long kb = (long long)(V.kf0 + k) * b.kp_pitch;
    const int nk = kf_count(b, V, k);
    for (int i0 = 0; i0 < nk; i0 += kSnThreads) {
      const int i = i0 + t;
      const int m = i < nk ? b.d_mp[kb + i] : -1;
      const bool f = m >= 0 && !b.d_bad[V.mp0 + m] && !b.d_mark[V.mp0 + m];
      int tot;
      const int pos = block_prefix<4>(f, S.wsum, &tot);
      if (f) {
        b.d_mark[V.mp0 + m] = 1;
        if (ncand + pos < b.list_pitch) list[ncand + pos] = m;
        else over = true;
      }
      ncand = min(ncand + tot, b.list_pitch);
    }
    __syncthreads();   // the marks, before the next target reads them
  }
  if (over) atomicOr(b.d_err, 1);
  if (t == 0) R->n_candidates = ncand;
  __syncthreads();
  fuse_call(a, V, S, cur, list, ncand, search, nullptr, a.th);
  if (t == 0) R->n_fused[nt] = S.n_fused;
  // ---- step 5: every good point of the current keyframe, one wave per point ----
  for (int i = wave; i < ncur; i += kSnThreads / 64) {
    const int m = b.d_mp[cb + i];
    if (m < 0 || b.d_bad[V.mp0 + m]) continue;
    wave_distinctive(b, V, S, m, lane, wave);
    wave_normal_depth(a, V, S, m, lane, wave);
  }
  __syncthreads();
  // ---- step 6: KeyFrame::UpdateConnections of the current keyframe ----
  for (int i = t; i < ncur; i += kSnThreads) {
    const int m = b.d_mp[cb + i];
    if (m < 0 || b.d_bad[V.mp0 + m]) continue;
    const int16_t* row = b.d_obs + ((long long)V.mp0 + m) * kSnKF;
    for (int k = 0; k < V.nkf; k++)
      if (k != cur && row[k] >= 0) atomicAdd(&S.cnt[k], 1);
  }
  __syncthreads();
  if (t == 0) {
    int nmax = 0, kmax = -1, np = 0;
    int* pw = S.ob[0];   // in id order: ascending (weight, id) after the sort
    int* pk = S.ob[1];
    for (int r = 0; r < V.nkf; r++) {
      const int k = S.by_id[r];
      const int w = S.cnt[k];
      R->conn_w[k] = w;
      if (w <= 0) continue;
      if (w > nmax) {
        nmax = w;
        kmax = k;
      }
      if (w >= 15) {
        pw[np] = w;
        pk[np++] = k;
        R->add_conn[k] = w;
      }
    }
    if (kmax < 0) {
      R->n_ordered = -1;
    } else {
      if (np == 0) {
        pw[np] = nmax;
        pk[np++] = kmax;
        R->add_conn[kmax] = nmax;
      }
      // stable insertion sort by weight: equal weights stay in id order
      for (int x = 1; x < np; x++) {
        const int vw = pw[x], vk = pk[x];
        int y = x - 1;
        while (y >= 0 && pw[y] > vw) {
          pw[y + 1] = pw[y];
          pk[y + 1] = pk[y];
          y--;
        }
        pw[y + 1] = vw;
        pk[y + 1] = vk;
      }
      for (int x = 0; x < np; x++) {
        R->ordered[x] = pk[np - 1 - x];
        R->ordered_w[x] = pw[np - 1 - x];
      }
      R->n_ordered = np;
    }
    if (a.d_ticks) {
      a.d_ticks[3 * p] = S.ticks[0];
      a.d_ticks[3 * p + 1] = S.ticks[1];
      a.d_ticks[3 * p + 2] = (long long)wall_clock64() - t_begin;
    }
  }
}

int make_sn_args(const orbpl_camera* cam, const float* scale, const float* sigma2, int nlevels,
                 SnArgs* a) {
  if (!cam || !scale || !sigma2) return arg_fail("NULL camera or scale tables");
  if (nlevels < 1 || nlevels > kMaxLevelsT) return arg_fail("nlevels outside [1, 16]");
  float inv[kMaxLevelsT];
  for (int l = 0; l < nlevels; l++) inv[l] = 1.0f / sigma2[l];   // mvInvLevelSigma2
  const int rc = make_consts(cam, scale, inv, nlevels, &a->c);
  if (rc) return rc;
  a->log_scale = log_scale_of(scale, nlevels);
  a->th = 3.0f;
  return ORBPL_OK;
}

int check_sn_batch(const orblm_sin_device_batch* b) {
  if (!b) return arg_fail("NULL batch");
  if (b->nkf < 1 || b->kp_pitch < 1 || b->kp_pitch > kSnMaxKp)
    return arg_fail("nkf < 1 or kp_pitch outside [1, 2048]");
  if (b->nmp < 0 || b->list_pitch < b->kp_pitch) return arg_fail("nmp < 0 or list_pitch < kp_pitch");
  if (!b->d_prob || !b->d_kf_id || !b->d_kf_n || !b->d_kf_Tcw || !b->d_kps_un || !b->d_uright ||
      !b->d_desc || !b->d_mp || !b->d_ordered || !b->d_xyz || !b->d_normal || !b->d_min_dist ||
      !b->d_max_dist || !b->d_mp_desc || !b->d_ref_kf || !b->d_bad || !b->d_n_visible ||
      !b->d_n_found || !b->d_replaced_by || !b->d_n_obs || !b->d_obs || !b->d_desc_src ||
      !b->d_mark || !b->d_result || !b->d_list || !b->d_search || !b->d_err)
    return arg_fail("NULL device array");
  return ORBPL_OK;
}

}  // namespace
}  // namespace orbpl

using namespace orbpl;

namespace {

// The staged pools of a host call: the pool's packed columns on the device.
struct SnStaged {
  MapPool H;
  HostStage st;
  orblm_sin_device_batch b{};

  // after every H.add; extra_list: a list of the caller's that d_list has to hold
  int upload(int extra_list) {
    H.pack(MapPool::kIn);
    int list_pitch = std::max(H.pitch, extra_list);
    for (const orblm_map* m : H.maps) list_pitch = std::max(list_pitch, m->M);
    const size_t M = H.M(), N = H.maps.size(), L = (size_t)list_pitch;
    b.nkf = H.nkf;
    b.kp_pitch = H.pitch;
    b.nmp = H.nmp;
    b.list_pitch = list_pitch;
    b.d_prob = st.in(H.prob);
    b.d_kf_id = st.in(H.id);
    b.d_kf_n = st.in(H.n);
    b.d_kf_Tcw = st.in(H.Tcw);
    b.d_kps_un = st.in(H.kps_un);
    b.d_uright = st.in(H.uright);
    b.d_desc = st.in(H.kf_desc);
    b.d_mp = st.in(H.mp);
    b.d_ordered = st.in(H.ordered);
    b.d_xyz = st.in(H.xyz);
    b.d_normal = st.in(H.normal);
    b.d_min_dist = st.in(H.min_dist);
    b.d_max_dist = st.in(H.max_dist);
    b.d_mp_desc = st.in(H.desc);
    b.d_ref_kf = st.in(H.ref_kf);
    b.d_bad = st.in(H.bad);
    b.d_n_visible = st.in(H.n_visible);
    b.d_n_found = st.in(H.n_found);
    b.d_replaced_by = st.out<int32_t>(M);
    b.d_n_obs = st.out<int32_t>(M);
    b.d_obs = st.out<int16_t>(M * kSnKF);
    b.d_desc_src = st.out<int32_t>(M * 2);
    b.d_mark = st.out<uint8_t>(M);
    b.d_result = st.out<orblm_sin_result>(N);
    b.d_list = st.out<int32_t>(N * L);
    b.d_search = st.out<int32_t>(N * L);
    b.d_err = st.zeros<int32_t>(1);
    return st.rc();
  }

  // the maps' in/out and out arrays back to the caller; err: the device flag
  int download(int* err) {
    H.pack(MapPool::kOut);
    st.back(H.mp, b.d_mp);
    st.back(H.normal, b.d_normal);
    st.back(H.min_dist, b.d_min_dist);
    st.back(H.max_dist, b.d_max_dist);
    st.back(H.desc, b.d_mp_desc);
    st.back(H.bad, b.d_bad);
    st.back(H.n_visible, b.d_n_visible);
    st.back(H.n_found, b.d_n_found);
    st.back(H.replaced_by, b.d_replaced_by);
    st.back(H.n_obs, b.d_n_obs);
    st.back(H.obs, b.d_obs);
    st.back(H.desc_src, b.d_desc_src);
    st.back(err, b.d_err, 1);
    if (st.rc()) return st.rc();
    H.unpack((MapPool::kIn | MapPool::kOut) & ~(MapPool::kXyz | MapPool::kRefKf));   // what the call writes
    return ORBPL_OK;
  }
};

int overflow_fail() {
  arg_fail("kernel capacity overflow (fuse candidate list)");
  return ORBPL_ERR_OVERFLOW;
}

void launch(const SnArgs& a, int n, hipStream_t s) {
  hipLaunchKernelGGL(k_search_in_neighbors, dim3(n), dim3(kSnThreads), 0, s, a);
}

// the device-pool entry; phases: with in-kernel time stamps into d_ticks
int sn_device(const orbpl_camera* cam, const float* scale_factors, const float* level_sigma2, int nlevels,
              const orblm_sin_device_batch* b, int n, void* stream, bool phases, long long* d_ticks) {
  SnArgs a{};
  int rc = make_sn_args(cam, scale_factors, level_sigma2, nlevels, &a);
  if (rc) return rc;
  if (n < 0 || (phases && !d_ticks)) return arg_fail("bad argument");
  if ((rc = check_sn_batch(b))) return rc;
  if (n == 0) return ORBPL_OK;
  a.b = *b;
  a.d_ticks = d_ticks;
  launch(a, n, static_cast<hipStream_t>(stream));
  HIP_CHECK(hipGetLastError());
  return ORBPL_OK;
}

}  // namespace

extern "C" {

int orblm_search_in_neighbors_batch_device(const orbpl_camera* cam, const float* scale_factors,
                                           const float* level_sigma2, int nlevels,
                                           const orblm_sin_device_batch* b, int n, void* stream) {
  return sn_device(cam, scale_factors, level_sigma2, nlevels, b, n, stream, false, nullptr);
}

int orblm_debug_search_in_neighbors_phases(const orbpl_camera* cam, const float* scale_factors,
                                           const float* level_sigma2, int nlevels,
                                           const orblm_sin_device_batch* b, int n, void* stream,
                                           long long* d_ticks) {
  return sn_device(cam, scale_factors, level_sigma2, nlevels, b, n, stream, true, d_ticks);
}

int orblm_search_in_neighbors(const orbpl_camera* cam, const float* scale_factors,
                              const float* level_sigma2, int nlevels, orblm_sin_problem* problems,
                              int n) {
  SnArgs a{};
  int rc = make_sn_args(cam, scale_factors, level_sigma2, nlevels, &a);
  if (rc) return rc;
  if (n < 0 || (n > 0 && !problems)) return arg_fail("bad argument");
  SnStaged S;
  for (int p = 0; p < n; p++) {
    const orblm_map& m = problems[p].map;
    if ((rc = check_map(m, nlevels))) return rc;
    if (problems[p].cur < 0 || problems[p].cur >= m.nkf)
      return arg_fail("current keyframe outside the table");
    if (m.M) S.H.owned.push_back(m.xyz);
    S.H.add(m, problems[p].cur);
  }
  if (S.H.shares_an_array()) return arg_fail("a keyframe or point array belongs to two problems");
  if (n == 0) return ORBPL_OK;
  if ((rc = S.upload(0))) return rc;
  a.b = S.b;
  launch(a, n, nullptr);   // host-pointer APIs use the null stream
  S.st.launched();
  std::vector<orblm_sin_result> hres((size_t)n);
  S.st.back(hres, S.b.d_result);
  int err = 0;
  if ((rc = S.download(&err))) return rc;
  for (int p = 0; p < n; p++) problems[p].result = hres[p];
  return err ? overflow_fail() : ORBPL_OK;
}

int orbm_fuse(const orbpl_camera* cam, const float* scale_factors, const float* level_sigma2,
              int nlevels, orblm_map* map, int kf, const int32_t* list, int n_list, float th,
              int* n_fused, int32_t* best_idx, int32_t* best_dist, int32_t* reason) {
  SnArgs a{};
  int rc = make_sn_args(cam, scale_factors, level_sigma2, nlevels, &a);
  if (rc) return rc;
  if (!map || !n_fused || n_list < 0) return arg_fail("bad argument");
  if (n_list > 0 && (!list || !best_idx || !best_dist || !reason)) return arg_fail("NULL list arrays");
  if ((rc = check_map(*map, nlevels))) return rc;
  if (kf < 0 || kf >= map->nkf) return arg_fail("keyframe outside the table");
  for (int i = 0; i < n_list; i++)
    if (list[i] < -1 || list[i] >= map->M) return arg_fail("list entry outside [-1, M)");
  SnStaged S;
  S.H.add(*map, kf);
  if ((rc = S.upload(n_list))) return rc;
  const size_t L = (size_t)S.b.list_pitch;
  a.b = S.b;
  a.fuse_only = 1;
  a.fuse_kf = kf;
  a.fuse_n = n_list;
  a.th = th;
  a.d_fuse_out = S.st.out<int32_t>(3 * L);
  if (S.st.rc()) return S.st.rc();
  if (n_list) HIP_CHECK(hipMemcpy(S.b.d_list, list, (size_t)n_list * 4, hipMemcpyHostToDevice));
  launch(a, 1, nullptr);
  S.st.launched();
  orblm_sin_result res;
  S.st.back(&res, S.b.d_result, 1);
  S.st.back(best_idx, a.d_fuse_out, (size_t)n_list);
  S.st.back(best_dist, a.d_fuse_out + L, (size_t)n_list);
  S.st.back(reason, a.d_fuse_out + 2 * L, (size_t)n_list);
  int err = 0;
  if ((rc = S.download(&err))) return rc;
  *n_fused = res.n_fused[0];
  return ORBPL_OK;
}

}  // extern "C"
