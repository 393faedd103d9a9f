// ORBmatcher::SearchBySim3 (ORBmatcher.cc:1441-1693) on gfx950, batched over
// keyframe pairs: one 256-thread workgroup per pair.
//   1. vbAlreadyMatched2 in LDS from matched12 (vbAlreadyMatched1 is
//      matched12[i] != -1 itself)
//   2. keyframe 2's 64 x 48 cell table in LDS (build_frame_grid), then every
//      feature of keyframe 1 in parallel: its point through Tcw1 and the
//      inverse Sim3 into camera 2, the z < 0 / IsInImage / distance tests,
//      PredictScale, KeyFrame::GetFeaturesInArea in cell and insertion order
//      with the octave gate, first minimum wins -> vnMatch1 and its reason
//   3. the same from keyframe 2 into keyframe 1 with the Sim3 itself
//   4. the agreement step; matched12 is written where both directions agree
// No feature's outcome depends on another's, so there is no sequential phase.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/orbpl.h"
#include "block_ops.h"
#include "host_rows.h"
#include "host_stage.h"
#include "lsd_math.h"
#include "match_common.h"
#include "orbpl_runtime.h"
#include "sim3_core.h"
#include "track_kernels.h"

namespace orbpl {
namespace {

constexpr int kSbsThreads = 256;
constexpr int kSbsMax = ORBM_SIM3_MAX_FEATURES;
constexpr int kSbsCells = kGridCols * kGridRows;
constexpr int kSbsThHigh = 100;  // ORBmatcher::TH_HIGH
static_assert(kSbsMax <= 65536, "items are 16-bit");

struct SbsShared {
  int cell_start[kSbsCells + 1];
  int fill[kSbsCells];
  uint16_t items[kSbsMax];
  int16_t gc[kSbsMax];
  uint8_t am2[kSbsMax];  // vbAlreadyMatched2
  int wsum[kSbsThreads / 64];
};

struct SbsKf {
  int n;
  const KeyPointD* kps;
  const uint4* desc;
  const uint8_t* valid;
  const float* xyz;
  const float* mind;
  const float* maxd;
  const uint8_t* mp_desc;
  const float* Tcw;
};

// one direction: src's points into dst's image through x -> R x + t
template <class Already>
__device__ void sbs_direction(const TrackConsts& c, SbsShared& S, const SbsKf& src,
                              const SbsKf& dst, const float* R, const float* t, float th,
                              float log_scale, Already already, int32_t* vn, int32_t* reason) {
  const int tid = threadIdx.x;
  build_frame_grid<kSbsThreads>(S.cell_start, S.items, S.gc, S.fill, S.wsum, dst.n, [&](int i) {
    const KeyPointD kp = dst.kps[i];
    // Frame::PosInGrid (Frame.cc:527-538), as KeyFrame's copy of the grid holds it
    const int px = (int)roundf((kp.x - c.minX) * c.gridInvW);
    const int py = (int)roundf((kp.y - c.minY) * c.gridInvH);
    return (px < 0 || px >= kGridCols || py < 0 || py >= kGridRows) ? -1 : px * kGridRows + py;
  });
  for (int i = tid; i < src.n; i += kSbsThreads) {
    int why = ORBM_SIM3_MATCHED, best_dist = INT_MAX, best_idx = -1;
    do {
      if (!src.valid[i]) {
        why = ORBM_SIM3_NO_POINT;
        break;
      }
      if (already(i)) {
        why = ORBM_SIM3_ALREADY;
        break;
      }
      float Pa[3], Pb[3];
      gemm_R_x_plus_t(src.Tcw, src.xyz + 3 * (long long)i, Pa);
      sim3::transform(R, t, Pa, Pb);
      if (Pb[2] < 0.0f) {
        why = ORBM_SIM3_BEHIND;
        break;
      }
      const float invz = (float)(1.0 / (double)Pb[2]);
      const float x = Pb[0] * invz, y = Pb[1] * invz;
      const float u = c.fx * x + c.cx, v = c.fy * y + c.cy;
      // KeyFrame::IsInImage; false for a coordinate that is not a number
      if (!(u >= c.minX && u < c.maxX && v >= c.minY && v < c.maxY)) {
        why = ORBM_SIM3_OUT_OF_IMAGE;
        break;
      }
      const float maxd = 1.2f * src.maxd[i], mind = 0.8f * src.mind[i];
      // cv::norm (P16): double squares, one rounding
      const float dist = (float)sqrt((double)Pb[0] * Pb[0] + (double)Pb[1] * Pb[1] +
                                     (double)Pb[2] * Pb[2]);
      if (dist < mind || dist > maxd) {
        why = ORBM_SIM3_DISTANCE;
        break;
      }
      int level = 0;
      if (c.nlevels > 1) {  // MapPoint::PredictScale (MapPoint.cc:399-414, P15)
        const float ratio = src.maxd[i] / dist;
        level = (int)ceilf((float)lsdm::log_((double)ratio) / log_scale);
        level = level < 0 ? 0 : (level >= c.nlevels ? c.nlevels - 1 : level);
      }
      const float r = th * c.scale[level];
      int cx0, cx1, cy0, cy1;
      bool any = false;
      if (grid_window(c, u, v, r, &cx0, &cx1, &cy0, &cy1)) {
        const uint4* md = reinterpret_cast<const uint4*>(src.mp_desc + (long long)i * 32);
        const uint4 d0 = md[0], d1 = md[1];
        for (int ix = cx0; ix <= cx1; ix++)
          for (int iy = cy0; iy <= cy1; iy++) {
            const int cell = ix * kGridRows + iy;
            for (int q = S.cell_start[cell]; q < S.cell_start[cell + 1]; q++) {
              const int idx = S.items[q];
              const KeyPointD kp = dst.kps[idx];
              if (!(fabsf(kp.x - u) < r && fabsf(kp.y - v) < r)) continue;
              any = true;
              if (kp.octave < level - 1 || kp.octave > level) continue;
              const int d = hamming256(d0, d1, dst.desc + 2 * idx);
              if (d < best_dist) {
                best_dist = d;
                best_idx = idx;
              }
            }
          }
      }
      if (!any) why = ORBM_SIM3_EMPTY_AREA;
      else if (best_dist > kSbsThHigh) why = ORBM_SIM3_NO_MATCH;
    } while (false);
    vn[i] = why == ORBM_SIM3_MATCHED ? best_idx : -1;
    reason[i] = why;
  }
  __syncthreads();
}

__global__ __launch_bounds__(kSbsThreads) void k_search_by_sim3(TrackConsts c,
                                                                 orbm_sim3_device_batch b,
                                                                 float th, float log_scale) {
  __shared__ SbsShared S;
  const int p = blockIdx.x, tid = threadIdx.x;
  const int n1 = min(min(max(b.d_n1[p], 0), kSbsMax), b.pitch1);
  const int n2 = min(min(max(b.d_n2[p], 0), kSbsMax), b.pitch2);
  const long long o1 = (long long)p * b.pitch1, o2 = (long long)p * b.pitch2;
  const SbsKf k1{n1, reinterpret_cast<const KeyPointD*>(b.d_kps_un1) + o1,
                 reinterpret_cast<const uint4*>(b.d_desc1 + o1 * 32), b.d_valid1 + o1,
                 b.d_xyz1 + 3 * o1, b.d_min_dist1 + o1, b.d_max_dist1 + o1, b.d_mp_desc1 + o1 * 32,
                 b.d_Tcw1 + 16LL * p};
  const SbsKf k2{n2, reinterpret_cast<const KeyPointD*>(b.d_kps_un2) + o2,
                 reinterpret_cast<const uint4*>(b.d_desc2 + o2 * 32), b.d_valid2 + o2,
                 b.d_xyz2 + 3 * o2, b.d_min_dist2 + o2, b.d_max_dist2 + o2, b.d_mp_desc2 + o2 * 32,
                 b.d_Tcw2 + 16LL * p};
  int32_t* matched12 = b.d_matched12 + o1;
  int32_t* vn1 = b.d_vn_match1 + o1;
  int32_t* vn2 = b.d_vn_match2 + o2;
  // sR12, sR21, t21 (P58): sim3_core.h's expansion of (R12, t12, s12)
  sim3::Hyp h;
  for (int j = 0; j < 9; j++) h.R[j] = b.d_R12[9LL * p + j];
  for (int j = 0; j < 3; j++) h.t[j] = b.d_t12[3LL * p + j];
  h.s = b.d_s12[p];
  sim3::Xf x;
  sim3::expand(h, x);
  // step 2 of the reference: the already-matched marks
  for (int i = tid; i < n2; i += kSbsThreads) S.am2[i] = 0;
  __syncthreads();
  for (int i = tid; i < n1; i += kSbsThreads) {
    const int m = matched12[i];
    if (m >= 0 && m < n2) S.am2[m] = 1;  // idx2 is honoured only inside [0, N2)
  }
  __syncthreads();
  sbs_direction(c, S, k1, k2, x.sRi, x.ti, th, log_scale,
                [&](int i) { return matched12[i] != -1; }, vn1, b.d_reason1 + o1);
  sbs_direction(c, S, k2, k1, x.sR, x.t, th, log_scale, [&](int i) { return S.am2[i] != 0; }, vn2,
                b.d_reason2 + o2);
  // step 5: agreement (the workgroup's own global writes are visible after the barrier)
  int found = 0;
  for (int i = tid; i < n1; i += kSbsThreads) {
    const int idx2 = vn1[i];
    if (idx2 >= 0 && vn2[idx2] == i) {
      matched12[i] = idx2;
      found++;
    }
  }
  found = block_sum<kSbsThreads / 64>(found, S.wsum);
  if (tid == 0) b.d_n_found[p] = found;
}

}  // namespace
}  // namespace orbpl

using namespace orbpl;

extern "C" {

int orbm_search_by_sim3_batch_device(const orbpl_camera* cam, const float* scale_factors,
                                     int nlevels, const orbm_sim3_device_batch* b, int npairs,
                                     float th, void* stream) {
  if (!cam || !scale_factors || !b || npairs < 0) return arg_fail("bad argument");
  if (b->pitch1 < 1 || b->pitch2 < 1 || b->pitch1 > kSbsMax || b->pitch2 > kSbsMax)
    return arg_fail("pitch outside [1, 2048] (the matcher capacity)");
  if (!b->d_n1 || !b->d_n2 || !b->d_kps_un1 || !b->d_desc1 || !b->d_valid1 || !b->d_xyz1 ||
      !b->d_min_dist1 || !b->d_max_dist1 || !b->d_mp_desc1 || !b->d_Tcw1 || !b->d_kps_un2 ||
      !b->d_desc2 || !b->d_valid2 || !b->d_xyz2 || !b->d_min_dist2 || !b->d_max_dist2 ||
      !b->d_mp_desc2 || !b->d_Tcw2 || !b->d_s12 || !b->d_R12 || !b->d_t12 || !b->d_matched12 ||
      !b->d_n_found || !b->d_vn_match1 || !b->d_vn_match2 || !b->d_reason1 || !b->d_reason2)
    return arg_fail("NULL device array");
  TrackConsts c;
  int rc = make_consts(cam, scale_factors, nullptr, nlevels, &c);
  if (rc) return rc;
  if (npairs == 0) return ORBPL_OK;
  hipLaunchKernelGGL(k_search_by_sim3, dim3(npairs), dim3(kSbsThreads), 0, (hipStream_t)stream, c,
                     *b, th, log_scale_of(scale_factors, nlevels));
  HIP_CHECK(hipGetLastError());
  return ORBPL_OK;
}

int orbm_search_by_sim3(const orbpl_camera* cam, const float* scale_factors, int nlevels,
                        const orbm_sim3_pair* P, int npairs, float th) {
  if (!cam || !scale_factors || npairs < 0 || (npairs > 0 && !P)) return arg_fail("bad argument");
  size_t p1 = 1, p2 = 1;
  for (int p = 0; p < npairs; p++) {
    const orbm_sim3_pair& r = P[p];
    for (const orbm_sim3_keyframe* k : {&r.kf1, &r.kf2}) {
      if (k->n < 0 || k->n > kSbsMax) return arg_fail("keyframe with more than 2048 features");
      if (!k->Tcw) return arg_fail("NULL pose");
      if (k->n > 0 && (!k->kps_un || !k->desc || !k->valid || !k->xyz || !k->min_dist ||
                       !k->max_dist || !k->mp_desc))
        return arg_fail("NULL keyframe arrays");
    }
    if (!r.R12 || !r.t12 || !r.n_found) return arg_fail("NULL Sim3 or count");
    if (r.kf1.n > 0 && (!r.matched12 || !r.vn_match1 || !r.reason1))
      return arg_fail("NULL keyframe 1 outputs");
    if (r.kf2.n > 0 && (!r.vn_match2 || !r.reason2)) return arg_fail("NULL keyframe 2 outputs");
    // (an index at or above n2 is a match that marks nothing in keyframe 2)
    for (int i = 0; i < r.kf1.n; i++)
      if (r.matched12[i] < -2) return arg_fail("matched12 entry below -2");
    p1 = std::max(p1, (size_t)r.kf1.n);
    p2 = std::max(p2, (size_t)r.kf2.n);
  }
  if (npairs == 0) {  // still refuses a bad camera or level count
    TrackConsts c;
    return make_consts(cam, scale_factors, nullptr, nlevels, &c);
  }
  SbsRows R(P, npairs, p1, p2);
  HostStage st;
  orbm_sim3_device_batch d{};
  d.d_n1 = st.in(R.k1.n);
  d.d_n2 = st.in(R.k2.n);
  d.pitch1 = (int)p1;
  d.pitch2 = (int)p2;
  d.d_kps_un1 = st.in(R.k1.kps_un);
  d.d_desc1 = st.in(R.k1.desc);
  d.d_valid1 = st.in(R.k1.valid);
  d.d_xyz1 = st.in(R.k1.xyz);
  d.d_min_dist1 = st.in(R.k1.min_dist);
  d.d_max_dist1 = st.in(R.k1.max_dist);
  d.d_mp_desc1 = st.in(R.k1.mp_desc);
  d.d_Tcw1 = st.in(R.k1.Tcw);
  d.d_kps_un2 = st.in(R.k2.kps_un);
  d.d_desc2 = st.in(R.k2.desc);
  d.d_valid2 = st.in(R.k2.valid);
  d.d_xyz2 = st.in(R.k2.xyz);
  d.d_min_dist2 = st.in(R.k2.min_dist);
  d.d_max_dist2 = st.in(R.k2.max_dist);
  d.d_mp_desc2 = st.in(R.k2.mp_desc);
  d.d_Tcw2 = st.in(R.k2.Tcw);
  d.d_s12 = st.in(R.s12);
  d.d_R12 = st.in(R.R12);
  d.d_t12 = st.in(R.t12);
  d.d_matched12 = st.inout(R.matched12);
  d.d_n_found = st.out(R.n_found);
  d.d_vn_match1 = st.out(R.k1.vn_match);
  d.d_vn_match2 = st.out(R.k2.vn_match);
  d.d_reason1 = st.out(R.k1.reason);
  d.d_reason2 = st.out(R.k2.reason);
  if (st.rc()) return st.rc();
  // the device form refuses the rest (camera, nlevels), launches on the null
  // stream as the host-pointer APIs do and checks the launch
  int rc = orbm_search_by_sim3_batch_device(cam, scale_factors, nlevels, &d, npairs, th, nullptr);
  if (rc) return rc;
  st.back_outs();
  if (st.rc()) return st.rc();
  R.unpack();
  return ORBPL_OK;
}

}  // extern "C"
