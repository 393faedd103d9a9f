// PnPsolver::iterate (PnPsolver.cc:165-258) on gfx950, batched: one 256-thread
// workgroup per solver.
//   phase A - every hypothesis the call may run, max(mRansacMaxIts -
//             mnIterations, nIterations) of them, is independent of the others
//             (hypothesis k uses draws 4k .. 4k+3): one thread per hypothesis
//             samples its four points and runs the 4-point EPnP in double
//             (pnp_core.h), then one wave per hypothesis counts its inliers
//             over all N points, lane-parallel with a ballot
//   phase B - the workgroup walks the hypotheses in order with the reference's
//             bookkeeping. Refine() depends only on the best-so-far set, so it
//             runs when that set changed: an N-point EPnP whose reductions
//             over the points are 256 strided partials added in ascending
//             order - the order pnp_core.h's one-thread path also follows -
//             with the points streamed from global memory (alphas and pcs are
//             recomputed, never stored). It stops at the first success.
// Every loop is bounded: the Jacobi sweeps by kMaxSweeps, the walk by the
// hypothesis count.
#include <hip/hip_runtime.h>

#include <limits.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/orbpl.h"
#include "host_rows.h"
#include "host_stage.h"
#include "orbpl_runtime.h"
#include "pnp_core.h"
#include "reloc_kernels.h"

namespace orbpl {

namespace {

constexpr int kPnpThreads = 256;
constexpr int kPnpWaves = kPnpThreads / 64;
static_assert(kPnpThreads == pnp::kParts, "one thread per partial sum of a reduction");
static_assert(kPnpMaxPoints == ORBPNP_MAX_POINTS && kPnpMaxIts == ORBPNP_MAX_ITERATIONS, "caps");

struct PnpShared {
  double hyp[kPnpMaxIts][12];          // R (row-major), t per hypothesis
  double parts[kPnpThreads][9];        // partial sums of the running reduction
  pnp::Work work;                      // Refine()'s small matrices
  int cnt[kPnpMaxIts];                 // mnInliersi per hypothesis
  uint16_t idx[kPnpMaxPoints];         // Refine()'s vIndices
  uint8_t best[kPnpMaxPoints];         // mvbBestInliers
  uint8_t refined[kPnpMaxPoints];      // mvbRefinedInliers
  float best_Tcw[16];
  int n_refined;
  int n_idx;
};

// the four sampled correspondences of a hypothesis
struct Pts4 {
  double pw[4][3], uv[4][2];
  __device__ void get(int i, double* p, double* u) const {
    p[0] = pw[i][0];
    p[1] = pw[i][1];
    p[2] = pw[i][2];
    u[0] = uv[i][0];
    u[1] = uv[i][1];
  }
};

// Refine()'s correspondences: the best inlier set in index order
struct PtsRef {
  const uint16_t* idx;
  const float* p3d;
  const float* p2d;
  __device__ void get(int i, double* p, double* u) const {
    const int k = idx[i];
    p[0] = p3d[3 * k];
    p[1] = p3d[3 * k + 1];
    p[2] = p3d[3 * k + 2];
    u[0] = p2d[2 * k];
    u[1] = p2d[2 * k + 1];
  }
};

// P28's reduction across the workgroup: thread j owns partial j
struct WgReduce {
  double (*parts)[9];
  __device__ bool leader() const { return threadIdx.x == 0; }
  template <int C, class F>
  __device__ void run(int n, F f, double* out) {
    static_assert(C <= 9, "parts holds 9 sums per thread");
    const int tid = threadIdx.x;
    __syncthreads();  // the leader's writes since the last reduction
    double part[C];
#pragma unroll
    for (int c = 0; c < C; c++) part[c] = 0.0;
    for (int i = tid; i < n; i += pnp::kParts) f(i, part);
#pragma unroll
    for (int c = 0; c < C; c++) parts[tid][c] = part[c];
    __syncthreads();
    if (tid < C) {
      double tot = 0.0;
      for (int j = 0; j < pnp::kParts; j++) tot = tot + parts[j][tid];
      out[tid] = tot;
    }
    __syncthreads();
  }
};

__device__ __forceinline__ void pose_to_Tcw(const double* R, const double* t, float* T) {
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) T[4 * r + c] = (float)R[3 * r + c];
    T[4 * r + 3] = (float)t[r];
  }
  T[12] = T[13] = T[14] = 0.0f;
  T[15] = 1.0f;
}

__global__ __launch_bounds__(kPnpThreads) void k_pnp_iterate(PnpArgs a) {
  __shared__ PnpShared sh;
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = min(min(max(a.n[s], 0), kPnpMaxPoints), a.pt_pitch);
  const int min_inl = a.min_inliers[s], max_its = a.max_its[s];
  const int it0 = a.iterations[s];
  const long long po = (long long)s * a.pt_pitch;
  const float* p3d = a.p3d + 3 * po;
  const float* p2d = a.p2d + 2 * po;
  const float* max_err = a.max_error + po;
  uint8_t* out_inl = a.inliers + po;
  uint8_t* st_best = a.best_mask + po;
  double cam[4];
  for (int j = 0; j < 4; j++) cam[j] = (double)a.cam[4 * s + j];

  for (int i = tid; i < N; i += kPnpThreads) out_inl[i] = 0;
  if (N < min_inl || N < 4) {  // iterate()'s early return: nothing consumed
    if (tid == 0) {
      for (int j = 0; j < 16; j++) a.Tcw[16 * s + j] = 0.0f;
      a.result[s] = 0;
      a.no_more[s] = 1;
      a.n_inliers[s] = 0;
      a.draws_consumed[s] = 0;
    }
    return;
  }
  long long want = std::max((long long)max_its - it0, (long long)a.n_iterations);
  // (a caller that keeps a cursor into the solver's draws passes it as draw_off)
  const int doff = a.draw_off ? min(max(a.draw_off[s], 0), a.draw_pitch) : 0;
  const int H = (int)std::min(std::max(want, 0LL),
                              (long long)std::min(kPnpMaxIts, (a.draw_pitch - doff) / 4));
  const int* draws = a.draws + (long long)s * a.draw_pitch + doff;

  for (int i = tid; i < N; i += kPnpThreads) sh.best[i] = st_best[i];
  if (tid < 16) sh.best_Tcw[tid] = a.best_Tcw[16 * s + tid];

  // ---- phase A: the hypotheses ----
  for (int h = tid; h < H; h += kPnpThreads) {
    int idx[4];
    pnp::sample4(draws + 4 * h, N, a.rand_max_p1, idx);
    Pts4 P;
    for (int i = 0; i < 4; i++) {
      for (int j = 0; j < 3; j++) P.pw[i][j] = p3d[3 * idx[i] + j];
      for (int j = 0; j < 2; j++) P.uv[i][j] = p2d[2 * idx[i] + j];
    }
    pnp::Work w;
    for (int j = 0; j < 4; j++) w.cam[j] = cam[j];
    pnp::SeqReduce red;
    pnp::compute_pose(P, 4, red, w);
    for (int j = 0; j < 9; j++) sh.hyp[h][j] = w.R[j];
    for (int j = 0; j < 3; j++) sh.hyp[h][9 + j] = w.t[j];
  }
  __syncthreads();
  for (int h = wave; h < H; h += kPnpWaves) {
    int c = 0;
    for (int i0 = 0; i0 < N; i0 += 64) {
      const int i = i0 + lane;
      const bool in = i < N && pnp::is_inlier(sh.hyp[h], sh.hyp[h] + 9, cam, p3d + 3 * i,
                                              p2d + 2 * i, max_err[i]);
      c += __popcll(__ballot(in));
    }
    if (lane == 0) sh.cnt[h] = c;
  }
  __syncthreads();

  // ---- phase B: the reference's bookkeeping, in order ----
  pnp::Work& w = sh.work;
  if (tid < 4) w.cam[tid] = cam[tid];
  int best = a.best_count[s];
  int ran = 0, result = 0;
  bool stale = true, refine_ok = false;  // stale: the best set changed since the last Refine()
  for (int k = 0; k < H; k++) {
    ran = k + 1;
    const int c = sh.cnt[k];
    if (c < min_inl) continue;
    if (c > best) {
      best = c;
      for (int i = tid; i < N; i += kPnpThreads)
        sh.best[i] = pnp::is_inlier(sh.hyp[k], sh.hyp[k] + 9, cam, p3d + 3 * i, p2d + 2 * i,
                                    max_err[i]);
      if (tid == 0) pose_to_Tcw(sh.hyp[k], sh.hyp[k] + 9, sh.best_Tcw);
      stale = true;
    }
    if (stale) {
      stale = false;
      __syncthreads();
      if (wave == 0) {  // vIndices, ascending
        int base = 0;
        for (int i0 = 0; i0 < N; i0 += 64) {
          const int i = i0 + lane;
          const bool in = i < N && sh.best[i];
          const unsigned long long b = __ballot(in);
          if (in) sh.idx[base + __popcll(b & ((1ull << lane) - 1ull))] = (uint16_t)i;
          base += __popcll(b);
        }
        if (lane == 0) {
          sh.n_idx = base;
          sh.n_refined = 0;
        }
      }
      __syncthreads();
      const int nref = sh.n_idx;
      refine_ok = false;
      if (nref > 0) {
        PtsRef P{sh.idx, p3d, p2d};
        WgReduce red{sh.parts};
        pnp::compute_pose(P, nref, red, w);
        __syncthreads();
        int cr = 0;
        for (int i0 = 0; i0 < N; i0 += kPnpThreads) {
          const int i = i0 + tid;
          const bool in = i < N && pnp::is_inlier(w.R, w.t, cam, p3d + 3 * i, p2d + 2 * i,
                                                  max_err[i]);
          if (i < N) sh.refined[i] = in;
          cr += __popcll(__ballot(in));
        }
        if (lane == 0) atomicAdd(&sh.n_refined, cr);
        __syncthreads();
        refine_ok = sh.n_refined > min_inl;
      }
    }
    if (refine_ok) {
      result = 1;
      break;
    }
  }
  __syncthreads();

  const int its = it0 + ran;
  for (int i = tid; i < N; i += kPnpThreads) st_best[i] = sh.best[i];
  int no_more = 0, n_inl = 0;
  if (result == 1) {
    n_inl = sh.n_refined;
    for (int i = tid; i < N; i += kPnpThreads) out_inl[i] = sh.refined[i];
  } else if (its >= max_its) {
    no_more = 1;
    if (best >= min_inl) {
      result = 2;
      n_inl = best;
      for (int i = tid; i < N; i += kPnpThreads) out_inl[i] = sh.best[i];
    }
  }
  if (tid == 0) {
    float T[16];
    if (result == 1) pose_to_Tcw(w.R, w.t, T);
    for (int j = 0; j < 16; j++) {
      a.Tcw[16 * s + j] = result == 1 ? T[j] : (result == 2 ? sh.best_Tcw[j] : 0.0f);
      a.best_Tcw[16 * s + j] = sh.best_Tcw[j];
    }
    a.iterations[s] = its;
    a.best_count[s] = best;
    a.result[s] = result;
    a.no_more[s] = no_more;
    a.n_inliers[s] = n_inl;
    a.draws_consumed[s] = 4 * ran;
  }
}

}  // namespace

void launch_pnp_iterate(const PnpArgs& a, int nsolvers, hipStream_t s) {
  if (nsolvers <= 0) return;
  hipLaunchKernelGGL(k_pnp_iterate, dim3(nsolvers), dim3(kPnpThreads), 0, s, a);
}

}  // namespace orbpl

using namespace orbpl;

namespace {
// hypotheses iterate(n_iterations) runs at most from this state
long long pnp_hypotheses(int n, int min_inliers, int max_its, int iterations, int n_iterations) {
  if (n < min_inliers) return 0;
  return std::max(0LL, std::max((long long)max_its - iterations, (long long)n_iterations));
}
}  // namespace

extern "C" {

int orbpnp_ransac_parameters(int n, double probability, int min_inliers, int max_iterations,
                             int min_set, float epsilon, float th2, const float* sigma2,
                             int32_t* out_min_inliers, int32_t* out_max_its, float* out_epsilon,
                             float* max_error) {
  if (n < 0 || !out_min_inliers || !out_max_its || !out_epsilon)
    return arg_fail("bad argument");
  if (max_error && !sigma2 && n > 0) return arg_fail("max_error needs sigma2");
  // PnPsolver::SetRansacParameters (:121-157)
  int nMinInliers = (int)(n * epsilon);
  if (nMinInliers < min_inliers) nMinInliers = min_inliers;
  if (nMinInliers < min_set) nMinInliers = min_set;
  float eps = epsilon;
  if (eps < (float)nMinInliers / n) eps = (float)nMinInliers / n;
  const int nIterations = nMinInliers == n ? 1 : ransac_iterations(probability, eps);
  *out_min_inliers = nMinInliers;
  *out_max_its = std::max(1, std::min(nIterations, max_iterations));
  *out_epsilon = eps;
  if (max_error)
    for (int i = 0; i < n; i++) max_error[i] = sigma2[i] * th2;
  return ORBPL_OK;
}

int orbpnp_iterate_batch_device(const orbpnp_device_batch* b, int nsolvers, int n_iterations,
                                void* stream) {
  if (!b || nsolvers < 0) return arg_fail("bad argument");
  if (nsolvers == 0) return ORBPL_OK;
  if (!b->d_n || !b->d_cam || !b->d_p2d || !b->d_p3d || !b->d_max_error || !b->d_min_inliers ||
      !b->d_max_its || !b->d_draws || !b->d_iterations || !b->d_best_inliers || !b->d_best_mask ||
      !b->d_best_Tcw || !b->d_Tcw || !b->d_result || !b->d_no_more || !b->d_n_inliers ||
      !b->d_inliers || !b->d_draws_consumed)
    return arg_fail("NULL device array");
  if (b->pt_pitch < 0 || b->draw_pitch < 0) return arg_fail("negative pitch");
  PnpArgs a{b->d_n, b->d_cam, b->d_p2d, b->d_p3d, b->d_max_error, b->pt_pitch, b->d_min_inliers,
            b->d_max_its, b->d_draws, b->draw_pitch, (double)RAND_MAX + 1.0, n_iterations,
            b->d_iterations, b->d_best_inliers, b->d_best_mask, b->d_best_Tcw, b->d_Tcw,
            b->d_result, b->d_no_more, b->d_n_inliers, b->d_inliers, b->d_draws_consumed};
  launch_pnp_iterate(a, nsolvers, (hipStream_t)stream);
  HIP_CHECK(hipGetLastError());
  return ORBPL_OK;
}

int orbpnp_iterate(const orbpnp_problem* P, int nsolvers, int n_iterations) {
  if (nsolvers < 0 || (nsolvers > 0 && !P)) return arg_fail("bad argument");
  if (nsolvers == 0) return ORBPL_OK;
  size_t ptp = 1, drp = 4;
  std::vector<size_t> nd(nsolvers);   // the draws a problem can consume
  for (int p = 0; p < nsolvers; p++) {
    const orbpnp_problem& r = P[p];
    if (r.n < 0 || r.n > kPnpMaxPoints) return arg_fail("more than 2048 correspondences");
    if (r.min_inliers < 4) return arg_fail("min_inliers below the minimal set of 4");
    if (!r.iterations || !r.best_inliers || !r.best_Tcw || !r.Tcw || !r.result || !r.no_more ||
        !r.n_inliers || !r.draws_consumed)
      return arg_fail("NULL state or output");
    if (r.n > 0 && (!r.p2d || !r.p3d || !r.max_error || !r.best_mask || !r.inliers))
      return arg_fail("NULL correspondence arrays");
    if (*r.iterations < 0) return arg_fail("negative iteration count");
    const long long H = pnp_hypotheses(r.n, r.min_inliers, r.max_its, *r.iterations, n_iterations);
    if (H > kPnpMaxIts) return arg_fail("more hypotheses in one call than ORBPNP_MAX_ITERATIONS");
    if (r.n_draws < 0 || r.n_draws < 4 * H || (r.n_draws > 0 && !r.draws))
      return arg_fail("fewer draws than 4 per hypothesis");
    ptp = std::max(ptp, (size_t)r.n);
    drp = std::max(drp, nd[p] = (size_t)(4 * H));
  }
  PnpRows R(P, nsolvers, ptp, drp, nd);
  HostStage st;
  PnpArgs a{st.in(R.n),
            st.in(R.cam),
            st.in(R.p2d),
            st.in(R.p3d),
            st.in(R.max_error),
            (int)ptp,
            st.in(R.min_inliers),
            st.in(R.max_its),
            st.in(R.draws),
            (int)drp,
            (double)RAND_MAX + 1.0,
            n_iterations,
            st.inout(R.iterations),
            st.inout(R.best_inliers),
            st.inout(R.best_mask),
            st.inout(R.best_Tcw),
            st.out(R.Tcw),
            st.out(R.result),
            st.out(R.no_more),
            st.out(R.n_inliers),
            st.out(R.inliers),
            st.out(R.draws_consumed)};
  if (st.rc()) return st.rc();
  launch_pnp_iterate(a, nsolvers, nullptr);   // host-pointer APIs use the null stream
  st.launched();
  st.back_outs();
  if (st.rc()) return st.rc();
  R.unpack();
  return ORBPL_OK;
}

}  // extern "C"
