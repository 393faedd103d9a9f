// Sim3Solver (Sim3Solver.cc) on gfx950, batched: one 256-thread workgroup per
// solver.
//   k_sim3_setup   - the constructor (:37-112): the accepted features of
//                    keyframe 1 in ascending order (an ordered block
//                    compaction), their points in both cameras and images and
//                    the truncated thresholds
//   k_sim3_iterate - iterate() (:140-207)
//     phase A - every hypothesis the call may run, min(nIterations,
//               mRansacMaxIts - mnIterations) of them, is independent of the
//               others (hypothesis k uses draws 3k .. 3k+2): one lane per
//               hypothesis samples its three points and runs Horn's closed
//               form (sim3_core.h), then one wave per hypothesis counts its
//               inliers over all N points with ballots
//     phase B - every thread walks the counts in order with the reference's
//               bookkeeping (>= replaces the best, > min_inliers returns); the
//               mask is recomputed lane-parallel for the one hypothesis that
//               ends as the best, which is also the one returned
// Every loop is bounded: the Jacobi sweeps by sim3::kMaxSweeps, the walk by
// the hypothesis count.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/orbpl.h"
#include "block_ops.h"
#include "host_rows.h"
#include "host_stage.h"
#include "orbpl_runtime.h"
#include "sim3_core.h"

namespace orbpl {

namespace {

constexpr int kSim3Threads = 256;
constexpr int kSim3Waves = kSim3Threads / 64;
constexpr int kSim3MaxPoints = ORBSIM3_MAX_POINTS;
constexpr int kSim3MaxIts = ORBSIM3_MAX_ITERATIONS;
constexpr int kSim3MaxLevels = 16;

__global__ __launch_bounds__(kSim3Threads) void k_sim3_setup(orbsim3_setup_device_batch a) {
  __shared__ int wsum[kSim3Waves];
  __shared__ float sig[kSim3MaxLevels];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int n1 = min(min(max(a.d_n1[s], 0), kSim3MaxPoints), a.pitch1);
  const int n2 = min(min(max(a.d_n2[s], 0), kSim3MaxPoints), a.pitch2);
  const int nlev = min(max(a.nlevels, 1), kSim3MaxLevels);
  const long long o1 = (long long)s * a.pitch1, o2 = (long long)s * a.pitch2;
  if (tid < nlev) sig[tid] = a.d_level_sigma2[tid];
  float T1[12], T2[12], cam[4];
  for (int j = 0; j < 12; j++) {
    T1[j] = a.d_Tcw1[16 * s + j];
    T2[j] = a.d_Tcw2[16 * s + j];
  }
  for (int j = 0; j < 4; j++) cam[j] = a.d_cam[4 * s + j];
  const float R1[9] = {T1[0], T1[1], T1[2], T1[4], T1[5], T1[6], T1[8], T1[9], T1[10]};
  const float R2[9] = {T2[0], T2[1], T2[2], T2[4], T2[5], T2[6], T2[8], T2[9], T2[10]};
  const float t1[3] = {T1[3], T1[7], T1[11]}, t2[3] = {T2[3], T2[7], T2[11]};
  __syncthreads();
  int base = 0;
  for (int i0 = 0; i0 < n1; i0 += kSim3Threads) {  // uniform trip count
    const int i = i0 + tid;
    int m = -1;
    bool ok = false;
    if (i < n1) {
      m = a.d_matched12[o1 + i];
      ok = sim3::accepts(m, a.d_valid1[o1 + i] != 0, n2, a.d_valid2 + o2);
    }
    int total;
    const int pos = base + block_prefix<kSim3Waves>(ok, wsum, &total);
    if (ok) {
      const long long w = o1 + pos;  // pos <= i < pitch1
      float Xc[3], uv[2];
      a.d_indices1[w] = i;
      sim3::transform(R1, t1, a.d_xyz1 + 3 * (o1 + i), Xc);
      sim3::to_image(Xc, cam, uv);
      for (int j = 0; j < 3; j++) a.d_X3Dc1[3 * w + j] = Xc[j];
      for (int j = 0; j < 2; j++) a.d_P1im1[2 * w + j] = uv[j];
      sim3::transform(R2, t2, a.d_xyz2 + 3 * (o2 + m), Xc);
      sim3::to_image(Xc, cam, uv);
      for (int j = 0; j < 3; j++) a.d_X3Dc2[3 * w + j] = Xc[j];
      for (int j = 0; j < 2; j++) a.d_P2im2[2 * w + j] = uv[j];
      const int l1 = min(max(a.d_octave1[o1 + i], 0), nlev - 1);
      const int l2 = min(max(a.d_octave2[o2 + m], 0), nlev - 1);
      a.d_max_error1[w] = sim3::max_error(sig[l1]);
      a.d_max_error2[w] = sim3::max_error(sig[l2]);
    }
    base += total;
  }
  if (tid == 0) a.d_n[s] = base;
}

struct Sim3Shared {
  sim3::Hyp hyp[kSim3MaxIts];
  int cnt[kSim3MaxIts];  // mnInliersi per hypothesis
};

__global__ __launch_bounds__(kSim3Threads) void k_sim3_iterate(orbsim3_device_batch a,
                                                                int n_iterations,
                                                                double rand_max_p1) {
  __shared__ Sim3Shared sh;
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = min(min(max(a.d_n[s], 0), kSim3MaxPoints), a.pt_pitch);
  const int min_inl = max(a.d_min_inliers[s], 3), max_its = a.d_max_its[s];
  const int it0 = a.d_iterations[s];
  const bool fix_scale = a.d_fix_scale[s] != 0;
  const long long po = (long long)s * a.pt_pitch;
  const float* X1 = a.d_X3Dc1 + 3 * po;
  const float* X2 = a.d_X3Dc2 + 3 * po;
  const float* im1 = a.d_P1im1 + 2 * po;
  const float* im2 = a.d_P2im2 + 2 * po;
  const int* me1 = a.d_max_error1 + po;
  const int* me2 = a.d_max_error2 + po;
  uint8_t* out_inl = a.d_inliers + po;
  uint8_t* st_best = a.d_best_mask + po;
  float cam[4];
  for (int j = 0; j < 4; j++) cam[j] = a.d_cam[4 * s + j];

  for (int i = tid; i < N; i += kSim3Threads) out_inl[i] = 0;
  if (N < min_inl) {  // iterate()'s early return: nothing consumed, the state as it was
    if (tid == 0) {
      for (int j = 0; j < 16; j++) a.d_T12[16 * s + j] = 0.0f;
      a.d_result[s] = 0;
      a.d_no_more[s] = 1;
      a.d_n_inliers[s] = 0;
      a.d_draws_consumed[s] = 0;
    }
    return;
  }
  // while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations)
  const long long want = std::min((long long)n_iterations, (long long)max_its - it0);
  const int H = (int)std::min(std::max(want, 0LL),
                              (long long)std::min(kSim3MaxIts, a.draw_pitch / 3));
  const int* draws = a.d_draws + (long long)s * a.draw_pitch;

  // ---- phase A: the hypotheses ----
  for (int h = tid; h < H; h += kSim3Threads) {
    int idx[3];
    sim3::sample3(draws + 3 * h, N, rand_max_p1, idx);
    float P1[3][3], P2[3][3];
    for (int c = 0; c < 3; c++)
      for (int r = 0; r < 3; r++) {
        P1[r][c] = X1[3 * idx[c] + r];
        P2[r][c] = X2[3 * idx[c] + r];
      }
    sim3::Hyp hy;
    sim3::compute_sim3(P1, P2, fix_scale, hy);
    sh.hyp[h] = hy;
  }
  __syncthreads();
  for (int h = wave; h < H; h += kSim3Waves) {
    sim3::Xf x;
    sim3::expand(sh.hyp[h], x);
    int c = 0;
    for (int i0 = 0; i0 < N; i0 += 64) {
      const int i = i0 + lane;
      float e[2];
      const bool in = i < N && sim3::is_inlier(x, cam, X1 + 3 * i, X2 + 3 * i, im1 + 2 * i,
                                               im2 + 2 * i, me1[i], me2[i], e);
      c += __popcll(__ballot(in));
    }
    if (lane == 0) sh.cnt[h] = c;
  }
  __syncthreads();

  // ---- phase B: the reference's bookkeeping, in order, the same in every thread ----
  int best = a.d_best_inliers[s];
  int ran = 0, result = 0, best_k = -1;
  for (int k = 0; k < H; k++) {
    ran = k + 1;
    const int c = sh.cnt[k];
    if (c >= best) {  // a later tie replaces the best
      best = c;
      best_k = k;
      if (c > min_inl) {
        result = 1;
        break;
      }
    }
  }
  if (best_k >= 0) {  // mvbBestInliers, and vbInliers when this hypothesis is returned
    sim3::Xf x;
    sim3::expand(sh.hyp[best_k], x);
    for (int i = tid; i < N; i += kSim3Threads) {
      float e[2];
      const bool in = sim3::is_inlier(x, cam, X1 + 3 * i, X2 + 3 * i, im1 + 2 * i, im2 + 2 * i,
                                      me1[i], me2[i], e);
      st_best[i] = in;
      if (result) out_inl[i] = in;
    }
  }
  if (tid == 0) {
    const int its = it0 + ran;
    float T[16];
    for (int j = 0; j < 16; j++) T[j] = 0.0f;
    if (best_k >= 0) {
      const sim3::Hyp& hb = sh.hyp[best_k];
      sim3::to_T12(hb, T);
      for (int j = 0; j < 16; j++) a.d_best_T12[16 * s + j] = T[j];
      for (int j = 0; j < 9; j++) a.d_best_R[9 * s + j] = hb.R[j];
      for (int j = 0; j < 3; j++) a.d_best_t[3 * s + j] = hb.t[j];
      a.d_best_s[s] = hb.s;
    }
    for (int j = 0; j < 16; j++) a.d_T12[16 * s + j] = result ? T[j] : 0.0f;
    a.d_iterations[s] = its;
    a.d_best_inliers[s] = best;
    a.d_result[s] = result;
    a.d_no_more[s] = (!result && its >= max_its) ? 1 : 0;
    a.d_n_inliers[s] = result ? best : 0;
    a.d_draws_consumed[s] = 3 * ran;
  }
}

// hypotheses iterate(n_iterations) runs at most from this state
long long sim3_hypotheses(int n, int min_inliers, int max_its, int iterations, int n_iterations) {
  if (n < min_inliers) return 0;
  return std::max(0LL, std::min((long long)n_iterations, (long long)max_its - iterations));
}

}  // namespace

}  // namespace orbpl

using namespace orbpl;

extern "C" {

int orbsim3_ransac_parameters(int n, double probability, int min_inliers, int max_iterations,
                              int32_t* out_max_its) {
  if (n < 0 || !out_max_its) return arg_fail("bad argument");
  // Sim3Solver::SetRansacParameters (:114-138)
  const float epsilon = (float)min_inliers / n;
  const int nIterations = min_inliers == n ? 1 : ransac_iterations(probability, epsilon);
  *out_max_its = std::max(1, std::min(nIterations, max_iterations));
  return ORBPL_OK;
}

int orbsim3_setup(const orbsim3_pair* P, int npairs, const float* level_sigma2, int nlevels) {
  if (npairs < 0 || (npairs > 0 && !P)) return arg_fail("bad argument");
  if (nlevels < 1 || nlevels > kSim3MaxLevels) return arg_fail("nlevels outside [1, 16]");
  if (!level_sigma2) return arg_fail("NULL level_sigma2");
  for (int p = 0; p < npairs; p++) {
    const orbsim3_pair& r = P[p];
    if (r.n1 < 0 || r.n1 > kSim3MaxPoints || r.n2 < 0 || r.n2 > kSim3MaxPoints)
      return arg_fail("keyframe with more than 2048 features");
    if (!r.Tcw1 || !r.Tcw2 || !r.n) return arg_fail("NULL pose or count");
    if (r.n1 > 0 && (!r.matched12 || !r.valid1 || !r.xyz1 || !r.octave1 || !r.indices1 ||
                     !r.X3Dc1 || !r.X3Dc2 || !r.P1im1 || !r.P2im2 || !r.max_error1 ||
                     !r.max_error2))
      return arg_fail("NULL keyframe 1 or output arrays");
    if (r.n2 > 0 && (!r.valid2 || !r.xyz2 || !r.octave2)) return arg_fail("NULL keyframe 2 arrays");
    for (int i = 0; i < r.n1; i++) {
      if (r.matched12[i] < -2 || r.matched12[i] >= r.n2)
        return arg_fail("matched12 entry outside [-2, n2)");
      if (r.octave1[i] < 0 || r.octave1[i] >= nlevels)
        return arg_fail("keypoint octave outside [0, nlevels)");
    }
    for (int j = 0; j < r.n2; j++)
      if (r.octave2[j] < 0 || r.octave2[j] >= nlevels)
        return arg_fail("keypoint octave outside [0, nlevels)");
  }
  for (int p = 0; p < npairs; p++) {
    const orbsim3_pair& r = P[p];
    const float cam[4] = {r.fx, r.fy, r.cx, r.cy};
    float R1[9], R2[9], t1[3], t2[3];
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 3; j++) {
        R1[3 * i + j] = r.Tcw1[4 * i + j];
        R2[3 * i + j] = r.Tcw2[4 * i + j];
      }
      t1[i] = r.Tcw1[4 * i + 3];
      t2[i] = r.Tcw2[4 * i + 3];
    }
    int n = 0;
    for (int i = 0; i < r.n1; i++) {
      const int m = r.matched12[i];
      if (!sim3::accepts(m, r.valid1[i] != 0, r.n2, r.valid2)) continue;
      r.indices1[n] = i;
      sim3::transform(R1, t1, r.xyz1 + 3 * i, r.X3Dc1 + 3 * n);
      sim3::to_image(r.X3Dc1 + 3 * n, cam, r.P1im1 + 2 * n);
      sim3::transform(R2, t2, r.xyz2 + 3 * m, r.X3Dc2 + 3 * n);
      sim3::to_image(r.X3Dc2 + 3 * n, cam, r.P2im2 + 2 * n);
      r.max_error1[n] = sim3::max_error(level_sigma2[r.octave1[i]]);
      r.max_error2[n] = sim3::max_error(level_sigma2[r.octave2[m]]);
      n++;
    }
    *r.n = n;
  }
  return ORBPL_OK;
}

int orbsim3_setup_batch_device(const orbsim3_setup_device_batch* b, int npairs, void* stream) {
  if (!b || npairs < 0) return arg_fail("bad argument");
  if (npairs == 0) return ORBPL_OK;
  if (!b->d_n1 || !b->d_n2 || !b->d_matched12 || !b->d_valid1 || !b->d_xyz1 || !b->d_octave1 ||
      !b->d_valid2 || !b->d_xyz2 || !b->d_octave2 || !b->d_Tcw1 || !b->d_Tcw2 || !b->d_cam ||
      !b->d_level_sigma2 || !b->d_n || !b->d_indices1 || !b->d_X3Dc1 || !b->d_X3Dc2 ||
      !b->d_P1im1 || !b->d_P2im2 || !b->d_max_error1 || !b->d_max_error2)
    return arg_fail("NULL device array");
  if (b->pitch1 < 0 || b->pitch2 < 0) return arg_fail("negative pitch");
  if (b->nlevels < 1 || b->nlevels > kSim3MaxLevels) return arg_fail("nlevels outside [1, 16]");
  hipLaunchKernelGGL(k_sim3_setup, dim3(npairs), dim3(kSim3Threads), 0, (hipStream_t)stream, *b);
  HIP_CHECK(hipGetLastError());
  return ORBPL_OK;
}

int orbsim3_iterate_batch_device(const orbsim3_device_batch* b, int nsolvers, int n_iterations,
                                 void* stream) {
  if (!b || nsolvers < 0) return arg_fail("bad argument");
  if (nsolvers == 0) return ORBPL_OK;
  if (!b->d_n || !b->d_cam || !b->d_X3Dc1 || !b->d_X3Dc2 || !b->d_P1im1 || !b->d_P2im2 ||
      !b->d_max_error1 || !b->d_max_error2 || !b->d_min_inliers || !b->d_max_its ||
      !b->d_fix_scale || !b->d_draws || !b->d_iterations || !b->d_best_inliers ||
      !b->d_best_mask || !b->d_best_T12 || !b->d_best_R || !b->d_best_t || !b->d_best_s ||
      !b->d_T12 || !b->d_result || !b->d_no_more || !b->d_n_inliers || !b->d_inliers ||
      !b->d_draws_consumed)
    return arg_fail("NULL device array");
  if (b->pt_pitch < 0 || b->draw_pitch < 0) return arg_fail("negative pitch");
  hipLaunchKernelGGL(k_sim3_iterate, dim3(nsolvers), dim3(kSim3Threads), 0, (hipStream_t)stream,
                     *b, n_iterations, (double)RAND_MAX + 1.0);
  HIP_CHECK(hipGetLastError());
  return ORBPL_OK;
}

int orbsim3_iterate(const orbsim3_problem* P, int nsolvers, int n_iterations) {
  if (nsolvers < 0 || (nsolvers > 0 && !P)) return arg_fail("bad argument");
  if (nsolvers == 0) return ORBPL_OK;
  size_t ptp = 1, drp = 3;
  std::vector<size_t> nd(nsolvers);   // the draws a problem can consume
  for (int p = 0; p < nsolvers; p++) {
    const orbsim3_problem& r = P[p];
    if (r.n < 0 || r.n > kSim3MaxPoints) return arg_fail("more than 2048 correspondences");
    if (r.min_inliers < 3) return arg_fail("min_inliers below the minimal set of 3");
    if (!r.iterations || !r.best_inliers || !r.best_T12 || !r.best_R || !r.best_t || !r.best_s ||
        !r.T12 || !r.result || !r.no_more || !r.n_inliers || !r.draws_consumed)
      return arg_fail("NULL state or output");
    if (r.n > 0 && (!r.X3Dc1 || !r.X3Dc2 || !r.P1im1 || !r.P2im2 || !r.max_error1 ||
                    !r.max_error2 || !r.best_mask || !r.inliers))
      return arg_fail("NULL correspondence arrays");
    if (*r.iterations < 0) return arg_fail("negative iteration count");
    const long long H = sim3_hypotheses(r.n, r.min_inliers, r.max_its, *r.iterations, n_iterations);
    if (H > kSim3MaxIts) return arg_fail("more hypotheses in one call than ORBSIM3_MAX_ITERATIONS");
    if (r.n_draws < 0 || r.n_draws < 3 * H || (r.n_draws > 0 && !r.draws))
      return arg_fail("fewer draws than 3 per hypothesis");
    ptp = std::max(ptp, (size_t)r.n);
    drp = std::max(drp, nd[p] = (size_t)(3 * H));
  }
  Sim3Rows R(P, nsolvers, ptp, drp, nd);
  HostStage st;
  orbsim3_device_batch a{};
  a.d_n = st.in(R.n);
  a.d_cam = st.in(R.cam);
  a.d_X3Dc1 = st.in(R.X3Dc1);
  a.d_X3Dc2 = st.in(R.X3Dc2);
  a.d_P1im1 = st.in(R.P1im1);
  a.d_P2im2 = st.in(R.P2im2);
  a.d_max_error1 = st.in(R.max_error1);
  a.d_max_error2 = st.in(R.max_error2);
  a.pt_pitch = (int)ptp;
  a.d_min_inliers = st.in(R.min_inliers);
  a.d_max_its = st.in(R.max_its);
  a.d_fix_scale = st.in(R.fix_scale);
  a.d_draws = st.in(R.draws);
  a.draw_pitch = (int)drp;
  a.d_iterations = st.inout(R.iterations);
  a.d_best_inliers = st.inout(R.best_inliers);
  a.d_best_mask = st.inout(R.best_mask);
  a.d_best_T12 = st.inout(R.best_T12);
  a.d_best_R = st.inout(R.best_R);
  a.d_best_t = st.inout(R.best_t);
  a.d_best_s = st.inout(R.best_s);
  a.d_T12 = st.out(R.T12);
  a.d_result = st.out(R.result);
  a.d_no_more = st.out(R.no_more);
  a.d_n_inliers = st.out(R.n_inliers);
  a.d_inliers = st.out(R.inliers);
  a.d_draws_consumed = st.out(R.draws_consumed);
  if (st.rc()) return st.rc();
  // host-pointer APIs use the null stream
  hipLaunchKernelGGL(k_sim3_iterate, dim3(nsolvers), dim3(kSim3Threads), 0, nullptr, a,
                     n_iterations, (double)RAND_MAX + 1.0);
  st.launched();
  st.back_outs();
  if (st.rc()) return st.rc();
  R.unpack();
  return ORBPL_OK;
}

int orbpl_test_sim3_hypothesis(const float* P1, const float* P2, int fix_scale, const float* cam,
                               int n, const float* X3Dc1, const float* X3Dc2, const float* P1im1,
                               const float* P2im2, const int32_t* max_error1,
                               const int32_t* max_error2, float* R, float* t, float* s, float* T12,
                               float* err, uint8_t* inliers) {
  if (!P1 || !P2 || !cam || !R || !t || !s || !T12 || n < 0) return arg_fail("bad argument");
  float A[3][3], B[3][3];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      A[r][c] = P1[3 * c + r];
      B[r][c] = P2[3 * c + r];
    }
  sim3::Hyp h;
  sim3::compute_sim3(A, B, fix_scale != 0, h);
  std::copy(h.R, h.R + 9, R);
  std::copy(h.t, h.t + 3, t);
  *s = h.s;
  sim3::to_T12(h, T12);
  sim3::Xf x;
  sim3::expand(h, x);
  for (int i = 0; i < n; i++)
    inliers[i] = sim3::is_inlier(x, cam, X3Dc1 + 3 * i, X3Dc2 + 3 * i, P1im1 + 2 * i,
                                 P2im2 + 2 * i, max_error1[i], max_error2[i], err + 2 * i);
  return ORBPL_OK;
}

}  // extern "C"
