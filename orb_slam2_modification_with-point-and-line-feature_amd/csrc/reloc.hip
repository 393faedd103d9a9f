// Tracking::Relocalization (Tracking.cc:2049-2269) on gfx950 as one batched
// call over many lost frames, each with its own keyframe database (DESIGN.md
// P30-P32). Every (frame p, candidate c) pair advances side by side; the
// reference's sequential order survives only in k_reloc_select.
//   place recognition   k_kfdb_reloc (kfdb.hip)
//   per pair, once      k_reloc_bow (match_local.hip), k_reloc_setup
//   per round           k_reloc_begin, k_pnp_iterate(5), k_reloc_after_pnp,
//                       k_pose, stage 1, k_match_kf(10, 100), stage 2, k_pose,
//                       stage 3, k_match_kf(3, 64), stage 4, k_pose, stage 5,
//                       k_reloc_select
// k_pose, k_match_kf and k_pnp_iterate take no per-pair indirection, so each
// pair holds its own copy of the small arrays they read, and the counts a
// pair that does not take part in a launch shows to them are 0. The kernels
// here are bookkeeping: one workgroup per pair (or per problem), ballots and
// ordered prefix sums. The host reads one 4-byte count per round.
#include <hip/hip_runtime.h>

#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../include/orbpl.h"
#include "block_ops.h"
#include "host_rows.h"
#include "host_stage.h"
#include "orbpl_runtime.h"
#include "reloc_kernels.h"
#include "track_kernels.h"

namespace orbpl {

namespace {

constexpr int kRelocThreads = 256;
static_assert(kKfdbMaxKf == 64, "one lane per candidate in the per-problem kernels");
static_assert(kRelocRec == ORBRL_REC_INTS, "record layout");

// outputs cleared (P32), the batch's largest candidate count
__global__ void __launch_bounds__(kRelocThreads) k_reloc_init(RelocDev d) {
  const int p = blockIdx.x, t = threadIdx.x;
  const int nc = min(max(d.ncand[p], 0), kKfdbMaxKf);
  if (t == 0) {
    d.done[p] = nc == 0;
    d.status[p] = nc == 0 ? ORBRL_NO_CANDIDATES : ORBRL_FAILED;
    d.ok[p] = 0;
    d.winner[p] = -1;
    d.rounds[p] = 0;
    d.n_good[p] = 0;
    d.n_live[p] = 0;
    d.exh_at[p] = kKfdbMaxKf;
    atomicMax(d.maxc, nc);
  }
  if (t < 16) d.out_Tcw[16 * p + t] = 0.0f;
  for (int i = t; i < d.kp_pitch; i += kRelocThreads) {
    d.out_match[(long long)p * d.kp_pitch + i] = -1;
    d.out_outlier[(long long)p * d.kp_pitch + i] = 0;
  }
  for (int i = t; i < kKfdbMaxKf * kRelocRec; i += kRelocThreads) {
    const int k = i % kRelocRec;
    d.rec[(long long)p * kKfdbMaxKf * kRelocRec + i] = k >= kRecG1 ? -1 : 0;
  }
}

// Tracking.cc:2086-2117 for one pair: the nmatches < 15 test, the solver's
// correspondences in keypoint order (PnPsolver.cc:36-83), SetRansacParameters
// from the table, the solver's state zeroed, and the pair's copies
__global__ void __launch_bounds__(kRelocThreads) k_reloc_setup(RelocDev d) {
  __shared__ int wsum[4];
  const int q = blockIdx.x, t = threadIdx.x, p = q / d.C, c = q - p * d.C;
  int* rw = d.rec_w + (long long)q * kRelocRec;
  int* rc = d.rec + ((long long)p * kKfdbMaxKf + c) * kRelocRec;
  const bool is_cand = c < d.ncand[p];
  const int nm = is_cand ? d.bow_nm[q] : 0;
  const bool live = is_cand && nm >= 15;
  if (t == 0) {
    for (int k = 0; k < kRelocRec; k++) rw[k] = k >= kRecG1 ? -1 : 0;
    rw[kRecBow] = nm;
    rw[kRecDisc] = live ? 0 : 1;
    if (is_cand)
      for (int k = 0; k < kRelocRec; k++) rc[k] = rw[k];
    d.live[q] = d.live_w[q] = live;
    d.run[q] = 0;
    d.win[q] = 0;
    d.stage[q] = 0;
    d.want[q] = 0;
    d.n_run[q] = 0;
    d.n_corr[q] = 0;
    d.mk_cur_n[q] = 0;
    d.mk_kf_n[q] = 0;
    d.cursor[q] = 0;
    d.iterations[q] = 0;
    d.best_count[q] = 0;
    d.ngood[q] = 0;
    d.avail[q] = (live && c < d.n_streams[p]) ? d.draw_pitch : 0;
    d.min_inl[q] = d.table[0];
    d.max_its[q] = d.table[1];
    d.pn[q] = 0;
    d.pkf_n[q] = 0;
  }
  // (a pair that is not live is never run, but the solver's launch still
  // loads its scalars before its N == 0 return: they hold defined values)
  if (t < 4) d.pcam[4 * q + t] = d.cam[t];
  if (t < 16) d.best_Tcw[16 * q + t] = 0.0f;
  if (!live) return;
  const int P = d.kp_pitch;
  const long long fb = (long long)p * P, qb = (long long)q * P;
  const int slot = d.kf_first[p] + d.cand[p * kKfdbMaxKf + c];
  const long long kb = (long long)slot * P;
  const int n = min(max(d.n[p], 0), P), nk = min(max(d.kf_n[slot], 0), P);
  if (t == 0) {
    d.pn[q] = n;
    d.pkf_n[q] = nk;
  }
  for (int i = t; i < n; i += kRelocThreads) {
    d.pkps[qb + i] = d.kps_un[fb + i];
    d.puright[qb + i] = d.uright[fb + i];
    d.match[qb + i] = -1;
    d.outlier[qb + i] = 0;
    d.best_mask[qb + i] = 0;
  }
  {
    const uint4* s4 = reinterpret_cast<const uint4*>(d.desc + fb * 32);
    uint4* o4 = reinterpret_cast<uint4*>(d.pdesc + qb * 32);
    for (int i = t; i < 2 * n; i += kRelocThreads) o4[i] = s4[i];
    s4 = reinterpret_cast<const uint4*>(d.mp_desc + kb * 32);
    o4 = reinterpret_cast<uint4*>(d.pmp_desc + qb * 32);
    for (int i = t; i < 2 * nk; i += kRelocThreads) o4[i] = s4[i];
  }
  for (int j = t; j < nk; j += kRelocThreads) {
    d.pkf_angle[qb + j] = d.kf_angle[kb + j];
    d.pkf_valid[qb + j] = d.kf_valid[kb + j];
    d.pmp_min[qb + j] = d.mp_min_dist[kb + j];
    d.pmp_max[qb + j] = d.mp_max_dist[kb + j];
    d.kf_found[qb + j] = 0;
  }
  for (int j = t; j < 3 * nk; j += kRelocThreads) d.pmp_xyz[3 * qb + j] = d.mp_xyz[3 * kb + j];
  if (c < d.n_streams[p]) {
    const int* src = d.draws + ((long long)p * d.stream_pitch + c) * d.draw_pitch;
    for (int i = t; i < d.draw_pitch; i += kRelocThreads)
      d.pdraws[(long long)q * d.draw_pitch + i] = src[i];
  }
  // the correspondences, ascending keypoint index
  int N = 0;
  for (int base = 0; base < n; base += kRelocThreads) {
    const int i = base + t;
    const int m = i < n ? d.bow_match[qb + i] : -1;
    const bool has = m >= 0 && m < nk;
    int tot;
    const int k = N + block_prefix<4>(has, wsum, &tot);
    if (has) {
      const KeyPointD kp = d.pkps[qb + i];
      d.p2d[2 * (qb + k)] = kp.x;
      d.p2d[2 * (qb + k) + 1] = kp.y;
      for (int a = 0; a < 3; a++) d.p3d[3 * (qb + k) + a] = d.mp_xyz[3 * (kb + m) + a];
      // mvMaxError[i] = mvSigma2[i] * th2 (one float product)
      d.max_error[qb + k] = d.sigma2[min(max(kp.octave, 0), kMaxLevelsT - 1)] * 5.991f;
      d.kp_index[qb + k] = i;
    }
    N += tot;
  }
  if (t == 0) {
    d.n_corr[q] = N;
    const int e = min(N, kRelocTableN);
    d.min_inl[q] = d.table[2 * e];
    d.max_its[q] = d.table[2 * e + 1];
  }
}

// the top of a round (Tracking.cc:2128-2134) for one problem, lane = candidate:
// who runs, and P31's test of the draws each next iterate(5) may need
__global__ void __launch_bounds__(64) k_reloc_begin(RelocDev d) {
  const int p = blockIdx.x, c = threadIdx.x;
  if (p == 0 && c == 0) *d.undecided = 0;
  const bool in = c < d.C;
  const int q = p * d.C + (in ? c : 0);
  const bool active = in && !d.done[p] && c < d.ncand[p] && d.live[q];
  bool exh = false;
  if (active) {
    const long long need = 4LL * max(d.max_its[q] - d.iterations[q], 5);
    exh = need > (long long)(d.avail[q] - d.cursor[q]);
  }
  const unsigned long long em = __ballot(exh), am = __ballot(active);
  const int e = em ? __ffsll((long long)em) - 1 : kKfdbMaxKf;
  if (in) {
    const bool run = active && c < e;
    d.run[q] = run;
    d.n_run[q] = run ? d.n_corr[q] : 0;
    d.live_w[q] = d.live[q];
    d.win[q] = 0;
    d.stage[q] = 0;
    d.want[q] = 0;
    d.mk_cur_n[q] = 0;
    d.mk_kf_n[q] = 0;
  }
  if (c == 0) {
    d.exh_at[p] = e;
    if (am) d.rounds[p] += 1;
  }
}

// Tracking.cc:2148-2178 for one pair: bNoMore, the pose and the inliers'
// assignments into the candidate's view of mCurrentFrame, sFound
__global__ void __launch_bounds__(kRelocThreads) k_reloc_after_pnp(RelocDev d) {
  const int q = blockIdx.x, t = threadIdx.x;
  if (!d.run[q]) return;
  int* rw = d.rec_w + (long long)q * kRelocRec;
  const int res = d.result[q];
  const long long qb = (long long)q * d.kp_pitch;
  const int n = d.pn[q], nk = d.pkf_n[q], N = d.n_corr[q];
  if (t == 0) {
    d.cursor[q] += d.consumed[q];
    rw[kRecCalls] += 1;
    rw[kRecIts] = d.iterations[q];
    rw[kRecDraws] = d.cursor[q];
    rw[kRecResult] = res;
    rw[kRecNoMore] = d.no_more[q];
    rw[kRecInl] = d.n_inliers[q];
    for (int k = kRecG1; k < kRelocRec; k++) rw[k] = -1;
    if (d.no_more[q]) {
      d.live_w[q] = 0;
      rw[kRecDisc] = 1;
    }
    d.stage[q] = res > 0 ? 1 : 0;
    d.want[q] = res > 0 ? 1 : 0;
  }
  if (res <= 0) return;
  if (t < 16) d.Tcw[16 * q + t] = d.pnp_Tcw[16 * q + t];
  for (int i = t; i < n; i += kRelocThreads) d.match[qb + i] = -1;
  for (int j = t; j < nk; j += kRelocThreads) d.kf_found[qb + j] = 0;
  __syncthreads();
  for (int j = t; j < N; j += kRelocThreads) {
    if (!d.inliers[qb + j]) continue;
    const int i = d.kp_index[qb + j];
    const int m = d.bow_match[qb + i];
    d.match[qb + i] = m;
    d.kf_found[qb + m] = 1;
  }
}

// Tracking.cc:2181-2252 for one pair, cut where the reference calls the
// optimiser or the projection matcher. phase = the call that just returned:
// 1, 3, 5 PoseOptimization; 2, 4 SearchByProjection.
__global__ void __launch_bounds__(kRelocThreads) k_reloc_stage(RelocDev d, int phase) {
  __shared__ int sh_stage;
  const int q = blockIdx.x, t = threadIdx.x;
  // thread 0 rewrites stage[q] below: every thread decides on the value latched here
  if (t == 0) sh_stage = d.stage[q];
  __syncthreads();
  if (!d.run[q] || sh_stage != phase) {
    if (t == 0 && d.run[q]) d.want[q] = 0;
    return;
  }
  int* rw = d.rec_w + (long long)q * kRelocRec;
  const long long qb = (long long)q * d.kp_pitch;
  const int n = d.pn[q], nk = d.pkf_n[q];
  int next = 0, want = 0, win = 0, search = 0;
  if (phase == 1 || phase == 3 || phase == 5) {
    const int g = d.ninl[q];
    const bool sweep = phase != 3 && !(phase == 1 && g < 10);   // :2188-2190, :2236-2238
    if (sweep)
      for (int i = t; i < n; i += kRelocThreads)
        if (d.outlier[qb + i]) d.match[qb + i] = -1;
    if (phase == 1) {
      if (g >= 50) win = 1;
      else if (g >= 10) next = 2, search = 1;
    } else if (phase == 3) {
      if (g >= 50) win = 1;
      else if (g > 30) next = 4, search = 1;
    } else {
      win = g >= 50;
    }
    if (phase == 3 && search) {   // sFound from every assignment, outliers included (:2219-2222)
      for (int j = t; j < nk; j += kRelocThreads) d.kf_found[qb + j] = 0;
      __syncthreads();
      for (int i = t; i < n; i += kRelocThreads) {
        const int m = d.match[qb + i];
        if (m >= 0) d.kf_found[qb + m] = 1;
      }
    }
    if (search)
      for (int i = t; i < n; i += kRelocThreads) d.has_mp[qb + i] = d.match[qb + i] >= 0;
    if (t == 0) {
      rw[phase == 1 ? kRecG1 : (phase == 3 ? kRecG2 : kRecG3)] = g;
      d.ngood[q] = g;
    }
  } else {
    const int nadd = d.add_n[q];
    for (int i = t; i < n; i += kRelocThreads) {
      const int m = d.add_match[qb + i];
      if (m >= 0) d.match[qb + i] = m;
    }
    if (nadd + d.ngood[q] >= 50) next = phase + 1, want = 1;
    if (t == 0) rw[phase == 2 ? kRecAdd1 : kRecAdd2] = nadd;
  }
  if (t == 0) {
    d.stage[q] = next;
    d.want[q] = want;
    d.win[q] = win;
    d.mk_cur_n[q] = search ? n : 0;
    d.mk_kf_n[q] = search ? nk : 0;
  }
}

// the pairs of the next launch_pose, ascending
__global__ void __launch_bounds__(kRelocThreads) k_reloc_list(RelocDev d) {
  __shared__ int wsum[4];
  const int npairs = d.np * d.C, t = threadIdx.x;
  int cnt = 0;
  for (int base = 0; base < npairs; base += kRelocThreads) {
    const int q = base + t;
    const bool f = q < npairs && d.run[q] && d.want[q];
    int tot;
    const int k = cnt + block_prefix<4>(f, wsum, &tot);
    if (f) d.list[k] = q;
    cnt += tot;
  }
  if (t == 0) *d.list_n = cnt;
}

// the end of a round for one problem: the ordered selection of P32
__global__ void __launch_bounds__(kRelocThreads) k_reloc_select(RelocDev d) {
  __shared__ int sh_w, sh_done;
  const int p = blockIdx.x, t = threadIdx.x;
  // thread 0 sets done[p] below: every thread decides on the value latched here
  if (t == 0) sh_done = d.done[p];
  __syncthreads();
  if (sh_done) return;
  const int nc = min(d.ncand[p], d.C);
  if (t < 64) {
    const int q = p * d.C + (t < nc ? t : 0);
    const bool won = t < nc && d.run[q] && d.win[q];
    const unsigned long long wm = __ballot(won);
    const int w = wm ? __ffsll((long long)wm) - 1 : -1;
    const int lim = w >= 0 ? w + 1 : d.exh_at[p];
    // candidates up to the winner (or before the one out of draws) ran
    if (t < nc && t < lim && d.run[q]) {
      int* rc = d.rec + ((long long)p * kKfdbMaxKf + t) * kRelocRec;
      const int* rw = d.rec_w + (long long)q * kRelocRec;
      for (int k = 0; k < kRelocRec; k++) rc[k] = rw[k];
      d.live[q] = d.live_w[q];
    }
    const unsigned long long lm = __ballot(t < nc && d.live[q]);
    if (t == 0) {
      sh_w = w;
      const int nlive = __popcll(lm);
      d.n_live[p] = nlive;
      if (w >= 0) {
        d.ok[p] = 1;
        d.status[p] = ORBRL_OK;
        d.winner[p] = d.cand[p * kKfdbMaxKf + w];
        d.n_good[p] = d.ngood[p * d.C + w];
        d.done[p] = 1;
      } else if (lim < kKfdbMaxKf) {
        d.status[p] = ORBRL_DRAW_EXHAUSTED;
        d.done[p] = 1;
      } else if (nlive == 0) {
        d.status[p] = ORBRL_FAILED;
        d.done[p] = 1;
      } else {
        atomicAdd(d.undecided, 1);
      }
    }
  }
  __syncthreads();
  const int w = sh_w;
  if (w < 0) return;
  const int q = p * d.C + w;
  const long long qb = (long long)q * d.kp_pitch, pb = (long long)p * d.kp_pitch;
  if (t < 16) d.out_Tcw[16 * p + t] = d.Tcw[16 * q + t];
  const int n = d.pn[q];
  for (int i = t; i < n; i += kRelocThreads) {
    const int m = d.match[qb + i];
    d.out_match[pb + i] = m;
    d.out_outlier[pb + i] = m >= 0 ? d.outlier[qb + i] : 0;
  }
}

}  // namespace

void launch_reloc_init(const RelocDev& d, hipStream_t s) {
  if (d.np <= 0) return;
  hipLaunchKernelGGL(k_reloc_init, dim3(d.np), dim3(kRelocThreads), 0, s, d);
}
void launch_reloc_setup(const RelocDev& d, hipStream_t s) {
  hipLaunchKernelGGL(k_reloc_setup, dim3(d.np * d.C), dim3(kRelocThreads), 0, s, d);
}
void launch_reloc_begin(const RelocDev& d, hipStream_t s) {
  hipLaunchKernelGGL(k_reloc_begin, dim3(d.np), dim3(64), 0, s, d);
}
void launch_reloc_after_pnp(const RelocDev& d, hipStream_t s) {
  hipLaunchKernelGGL(k_reloc_after_pnp, dim3(d.np * d.C), dim3(kRelocThreads), 0, s, d);
  hipLaunchKernelGGL(k_reloc_list, dim3(1), dim3(kRelocThreads), 0, s, d);
}
void launch_reloc_stage(const RelocDev& d, int phase, hipStream_t s) {
  hipLaunchKernelGGL(k_reloc_stage, dim3(d.np * d.C), dim3(kRelocThreads), 0, s, d, phase);
  if (phase == 2 || phase == 4) hipLaunchKernelGGL(k_reloc_list, dim3(1), dim3(kRelocThreads), 0, s, d);
}
void launch_reloc_select(const RelocDev& d, hipStream_t s) {
  hipLaunchKernelGGL(k_reloc_select, dim3(d.np), dim3(kRelocThreads), 0, s, d);
}

}  // namespace orbpl

using namespace orbpl;

namespace {

// a device buffer that only grows
struct Grow {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t need(size_t bytes) {
    if (bytes <= cap && p) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    const hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
    if (e == hipSuccess) cap = bytes;
    return e;
  }
  ~Grow() {
    if (p) (void)hipFree(p);
  }
  template <class T>
  T* as() const { return reinterpret_cast<T*>(p); }
};

// grow g to h's size and copy h into it; does nothing once *e is a failure
template <class T>
T* upload(Grow& g, const std::vector<T>& h, hipError_t* e) {
  if (*e == hipSuccess) *e = g.need(h.size() * sizeof(T));
  if (*e == hipSuccess) *e = hipMemcpy(g.p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice);
  return g.as<T>();
}

// a column's size, and the whole of it back from its device array
template <class T>
size_t bytes(const Rows<T>& c) {
  return c.h.size() * sizeof(T);
}
template <class T>
hipError_t download(Rows<T>& c, const T* d) {
  return hipMemcpy(c.h.data(), d, bytes(c), hipMemcpyDeviceToHost);
}

constexpr int kNumIn = 28, kNumPair = 52, kNumProb = 16;

}  // namespace

struct orbrl_handle {
  TrackConsts consts;
  float log_scale;
  float sigma2[kMaxLevelsT];
  float cam[4];
  int max_problems, kp_pitch, draw_pitch;
  Grow table;
  Grow in[kNumIn], pair[kNumPair], prob[kNumProb];
};

namespace {

// the rounds of one batch over the device arrays of d (inputs, cand / ncand
// and the per-problem outputs in place); sizes the per-pair workspace
int run_reloc(orbrl_handle* h, RelocDev& d, hipStream_t s) {
  const size_t np = d.np, P = d.kp_pitch;
  Grow* w = h->prob;
  int k = 0;
#define PROB(field, T, count)                        \
  HIP_CHECK(w[k].need(np * (count) * sizeof(T)));    \
  d.field = w[k++].as<T>()
  PROB(exh_at, int, 1);
  PROB(done, int, 1);
  PROB(undecided, int, 1);
  PROB(maxc, int, 1);
#undef PROB
  HIP_CHECK(hipMemsetAsync(d.maxc, 0, 4, s));
  launch_reloc_init(d, s);
  HIP_CHECK(hipGetLastError());
  int C = 0;
  HIP_CHECK(hipMemcpyAsync(&C, d.maxc, 4, hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
  if (C <= 0) return ORBPL_OK;
  C = std::min(C, kKfdbMaxKf);
  d.C = C;
  const size_t Q = np * C;
  w = h->pair;
  k = 0;
#define PAIR(field, T, count)                       \
  HIP_CHECK(w[k].need(Q * (count) * sizeof(T)));    \
  d.field = w[k++].as<T>()
  PAIR(bow_match, int, P);
  PAIR(bow_nm, int, 1);
  PAIR(p2d, float, 2 * P);
  PAIR(p3d, float, 3 * P);
  PAIR(max_error, float, P);
  PAIR(kp_index, int, P);
  PAIR(n_corr, int, 1);
  PAIR(n_run, int, 1);
  PAIR(min_inl, int, 1);
  PAIR(max_its, int, 1);
  PAIR(pcam, float, 4);
  PAIR(pdraws, int, d.draw_pitch);
  PAIR(avail, int, 1);
  PAIR(cursor, int, 1);
  PAIR(iterations, int, 1);
  PAIR(best_count, int, 1);
  PAIR(best_mask, uint8_t, P);
  PAIR(best_Tcw, float, 16);
  PAIR(pnp_Tcw, float, 16);
  PAIR(result, int, 1);
  PAIR(no_more, int, 1);
  PAIR(n_inliers, int, 1);
  PAIR(inliers, uint8_t, P);
  PAIR(consumed, int, 1);
  PAIR(pn, int, 1);
  PAIR(pkps, KeyPointD, P);
  PAIR(puright, float, P);
  PAIR(pdesc, uint8_t, 32 * P);
  PAIR(pkf_n, int, 1);
  PAIR(pkf_angle, float, P);
  PAIR(pkf_valid, uint8_t, P);
  PAIR(pmp_xyz, float, 3 * P);
  PAIR(pmp_min, float, P);
  PAIR(pmp_max, float, P);
  PAIR(pmp_desc, uint8_t, 32 * P);
  PAIR(match, int, P);
  PAIR(has_mp, uint8_t, P);
  PAIR(outlier, uint8_t, P);
  PAIR(kf_found, uint8_t, P);
  PAIR(Tcw, float, 16);
  PAIR(ninl, int, 1);
  PAIR(add_match, int, P);
  PAIR(add_n, int, 1);
  PAIR(mk_cur_n, int, 1);
  PAIR(mk_kf_n, int, 1);
  PAIR(run, uint8_t, 1);
  PAIR(live, uint8_t, 1);
  PAIR(live_w, uint8_t, 1);
  PAIR(win, uint8_t, 1);
  PAIR(stage, int, 1);
  PAIR(want, int, 1);
  PAIR(ngood, int, 1);
#undef PAIR
  static_assert(kNumPair == 52, "one Grow per PAIR line");
  Grow& g_rec = h->prob[4];
  Grow& g_list = h->prob[5];
  Grow& g_edges = h->prob[6];
  HIP_CHECK(g_rec.need(Q * kRelocRec * sizeof(int)));
  d.rec_w = g_rec.as<int>();
  HIP_CHECK(g_list.need((Q + 1) * sizeof(int)));
  d.list = g_list.as<int>();
  d.list_n = d.list + Q;
  HIP_CHECK(g_edges.need(Q * (size_t)kPoseMaxEdges * pose_edge_bytes()));

  launch_reloc_bow(d, s);
  launch_reloc_setup(d, s);
  HIP_CHECK(hipGetLastError());

  PnpArgs pa{d.n_run, d.pcam, d.p2d, d.p3d, d.max_error, (int)P, d.min_inl, d.max_its, d.pdraws,
             d.draw_pitch, (double)RAND_MAX + 1.0, 5, d.iterations, d.best_count, d.best_mask,
             d.best_Tcw, d.pnp_Tcw, d.result, d.no_more, d.n_inliers, d.inliers, d.consumed};
  pa.draw_off = d.cursor;
  PoseLaunch pl{};
  pl.kps_un = d.pkps;
  pl.uright = d.puright;
  pl.match = d.match;
  pl.has_mp = nullptr;
  pl.mp_xyz = d.pmp_xyz;
  pl.n = d.pn;
  pl.kp_pitch = (int)P;
  pl.nl = 0;
  pl.Tcw = d.Tcw;
  pl.pose_stride = 16;
  pl.outlier = d.outlier;
  pl.ninliers = d.ninl;
  pl.nm_stride = 1;
  pl.active = nullptr;
  pl.edges = reinterpret_cast<PoseEdge*>(g_edges.p);
  pl.list = d.list;
  pl.list_n = d.list_n;
  MatchKfArgs ma{};
  ma.cur_kps_un = d.pkps;
  ma.cur_desc = d.pdesc;
  ma.cur_has_mp = d.has_mp;
  ma.cur_n = d.mk_cur_n;
  ma.kp_pitch = (int)P;
  ma.kf_angle = d.pkf_angle;
  ma.kf_valid = d.pkf_valid;
  ma.kf_found = d.kf_found;
  ma.mp_xyz = d.pmp_xyz;
  ma.mp_min_dist = d.pmp_min;
  ma.mp_max_dist = d.pmp_max;
  ma.mp_desc = d.pmp_desc;
  ma.kf_n = d.mk_kf_n;
  ma.kf_pitch = (int)P;
  ma.Tcw = d.Tcw;
  ma.pose_stride = 16;
  ma.match = d.add_match;
  ma.nmatches = d.add_n;
  ma.nm_stride = 1;
  ma.check_ori = 1;     // ORBmatcher matcher2(0.9, true)
  ma.log_scale = h->log_scale;

  // a solver that runs consumes at least one hypothesis' 4 draws a round, and
  // one with fewer than 20 left ends its problem (P31)
  const int max_rounds = d.draw_pitch / 4 + 2;
  for (int r = 0; r < max_rounds; r++) {
    launch_reloc_begin(d, s);
    launch_pnp_iterate(pa, (int)Q, s);
    launch_reloc_after_pnp(d, s);
    launch_pose(h->consts, pl, (int)Q, s);
    launch_reloc_stage(d, 1, s);
    ma.th = 10.0f;
    ma.orb_dist = 100;
    launch_match_kf(h->consts, ma, (int)Q, s);
    launch_reloc_stage(d, 2, s);
    launch_pose(h->consts, pl, (int)Q, s);
    launch_reloc_stage(d, 3, s);
    ma.th = 3.0f;
    ma.orb_dist = 64;
    launch_match_kf(h->consts, ma, (int)Q, s);
    launch_reloc_stage(d, 4, s);
    launch_pose(h->consts, pl, (int)Q, s);
    launch_reloc_stage(d, 5, s);
    launch_reloc_select(d, s);
    HIP_CHECK(hipGetLastError());
    int undecided = 0;
    HIP_CHECK(hipMemcpyAsync(&undecided, d.undecided, 4, hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
    if (undecided == 0) return ORBPL_OK;
  }
  return arg_fail("relocalisation did not terminate within its draws");
}

}  // namespace

extern "C" {

int orbrl_create(const orbpl_camera* cam, const float* scale_factors, const float* level_sigma2,
                 int nlevels, int max_problems, int kp_pitch, int draw_pitch, orbrl_handle** out) {
  if (!cam || !scale_factors || !level_sigma2 || !out) return arg_fail("NULL argument");
  if (max_problems < 1) return arg_fail("max_problems < 1");
  if (kp_pitch != 1024 && kp_pitch != 2048) return arg_fail("kp_pitch must be 1024 or 2048");
  if (draw_pitch < 20 || draw_pitch > 4 * ORBPNP_MAX_ITERATIONS || draw_pitch % 4)
    return arg_fail("draw_pitch must be a multiple of 4 in [20, 1280]");
  if (nlevels < 1 || nlevels > kMaxLevelsT) return arg_fail("nlevels out of range");
  orbrl_handle* h = new orbrl_handle();
  float inv[kMaxLevelsT];
  for (int l = 0; l < nlevels; l++) {
    h->sigma2[l] = level_sigma2[l];
    inv[l] = 1.0f / level_sigma2[l];   // ORBextractor's mvInvLevelSigma2
  }
  for (int l = nlevels; l < kMaxLevelsT; l++) h->sigma2[l] = level_sigma2[nlevels - 1];
  int rc = make_consts(cam, scale_factors, inv, nlevels, &h->consts);
  if (rc) {
    delete h;
    return rc;
  }
  h->log_scale = log_scale_of(scale_factors, nlevels);   // as orbm_search_by_projection_kf takes it
  h->cam[0] = cam->fx;
  h->cam[1] = cam->fy;
  h->cam[2] = cam->cx;
  h->cam[3] = cam->cy;
  h->max_problems = max_problems;
  h->kp_pitch = kp_pitch;
  h->draw_pitch = draw_pitch;
  // SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991) depends only on N
  std::vector<int32_t> tab(2 * (kRelocTableN + 1));
  for (int n = 0; n <= kRelocTableN; n++) {
    float eps;
    rc = orbpnp_ransac_parameters(n, 0.99, 10, 300, 4, 0.5f, 5.991f, nullptr, &tab[2 * n],
                                  &tab[2 * n + 1], &eps, nullptr);
    if (rc) {
      delete h;
      return rc;
    }
  }
  hipError_t e = h->table.need(tab.size() * 4);
  if (e == hipSuccess) e = hipMemcpy(h->table.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    delete h;
    return hip_fail(e, "orbrl_create", __LINE__);
  }
  *out = h;
  return ORBPL_OK;
}

void orbrl_destroy(orbrl_handle* h) { delete h; }

int orbrl_ransac_table(int32_t* min_inliers, int32_t* max_its, int n_entries) {
  if (!min_inliers || !max_its || n_entries < 0 || n_entries > kRelocTableN + 1)
    return arg_fail("bad argument");
  for (int n = 0; n < n_entries; n++) {
    float eps;
    const int rc = orbpnp_ransac_parameters(n, 0.99, 10, 300, 4, 0.5f, 5.991f, nullptr,
                                            &min_inliers[n], &max_its[n], &eps, nullptr);
    if (rc) return rc;
  }
  return ORBPL_OK;
}

int orbrl_relocalize_batch_device(orbrl_handle* h, const orbrl_device_batch* b, int n, int scoring,
                                  void* stream) {
  if (scoring != 0) return arg_fail("only the vocabulary's L1 scoring (L1_NORM = 0) is built");
  if (!h || !b || n < 0) return arg_fail("bad argument");
  if (n > h->max_problems) return arg_fail("more problems than the handle was created for");
  if (n == 0) return ORBPL_OK;
  if (!b->d_nkf || !b->d_kf_off || !b->d_kf_words || !b->d_kf_vals || !b->d_covis ||
      !b->d_reloc_score || !b->d_q_n || !b->d_q_words || !b->d_q_vals || !b->d_kf_first ||
      !b->d_kf_n || !b->d_kf_angle || !b->d_kf_feat_node || !b->d_kf_desc || !b->d_kf_valid ||
      !b->d_mp_xyz || !b->d_mp_min_dist || !b->d_mp_max_dist || !b->d_mp_desc || !b->d_n ||
      !b->d_kps_un || !b->d_uright || !b->d_desc || !b->d_feat_node || !b->d_draws ||
      !b->d_n_streams || !b->d_cand || !b->d_ncand || !b->d_ok || !b->d_status || !b->d_winner ||
      !b->d_rounds || !b->d_n_good || !b->d_n_candidates || !b->d_Tcw || !b->d_mp_kf_feature ||
      !b->d_outlier || !b->d_records)
    return arg_fail("NULL device array");
  if (b->ent_pitch < 0 || b->q_pitch < 0 || b->stream_pitch < 0 || b->stream_pitch > kKfdbMaxKf)
    return arg_fail("bad pitch");
  RelocDev d{};
  d.np = n;
  d.C = 0;
  d.kp_pitch = h->kp_pitch;
  d.draw_pitch = h->draw_pitch;
  d.stream_pitch = b->stream_pitch;
  d.n = b->d_n;
  d.kps_un = reinterpret_cast<const KeyPointD*>(b->d_kps_un);
  d.uright = b->d_uright;
  d.desc = b->d_desc;
  d.feat_node = b->d_feat_node;
  d.kf_first = b->d_kf_first;
  d.kf_n = b->d_kf_n;
  d.kf_angle = b->d_kf_angle;
  d.kf_feat_node = b->d_kf_feat_node;
  d.kf_desc = b->d_kf_desc;
  d.kf_valid = b->d_kf_valid;
  d.mp_xyz = b->d_mp_xyz;
  d.mp_min_dist = b->d_mp_min_dist;
  d.mp_max_dist = b->d_mp_max_dist;
  d.mp_desc = b->d_mp_desc;
  d.draws = b->d_draws;
  d.n_streams = b->d_n_streams;
  d.cand = b->d_cand;
  d.ncand = b->d_ncand;
  d.table = h->table.as<int>();
  for (int l = 0; l < kMaxLevelsT; l++) d.sigma2[l] = h->sigma2[l];
  for (int j = 0; j < 4; j++) d.cam[j] = h->cam[j];
  d.ok = b->d_ok;
  d.status = b->d_status;
  d.winner = b->d_winner;
  d.rounds = b->d_rounds;
  d.n_good = b->d_n_good;
  d.n_live = b->d_n_candidates;
  d.out_Tcw = b->d_Tcw;
  d.out_match = b->d_mp_kf_feature;
  d.out_outlier = b->d_outlier;
  d.rec = b->d_records;
  hipStream_t s = (hipStream_t)stream;
  KfdbArgs ka{b->d_nkf, b->d_kf_off, b->d_kf_words, b->d_kf_vals, (long long)b->ent_pitch,
              b->d_covis, b->d_reloc_score, b->d_q_n, b->d_q_words, b->d_q_vals,
              (long long)b->q_pitch, b->d_cand, b->d_ncand, nullptr};
  launch_kfdb_reloc(ka, n, s);
  HIP_CHECK(hipGetLastError());
  return run_reloc(h, d, s);
}

int orbrl_relocalize(orbrl_handle* h, orbrl_problem* probs, int n, int scoring) {
  if (scoring != 0) return arg_fail("only the vocabulary's L1 scoring (L1_NORM = 0) is built");
  if (!h || n < 0 || (n > 0 && !probs)) return arg_fail("bad argument");
  if (n > h->max_problems) return arg_fail("more problems than the handle was created for");
  if (n == 0) return ORBPL_OK;
  const size_t P = h->kp_pitch, NP = n;
  size_t entp = 1, qp = 1, sp = 1;
  for (int p = 0; p < n; p++) {
    const orbrl_problem& r = probs[p];
    if (const char* no = kfdb_refusal(r, "offsets must start at 0", &entp, &qp)) return arg_fail(no);
    if (r.n < 0 || r.n > (int)P) return arg_fail("more keypoints than kp_pitch");
    if (r.n > 0 && (!r.kps_un || !r.uright || !r.desc || !r.feat_node || !r.mp_kf_feature ||
                    !r.outlier))
      return arg_fail("NULL frame arrays");
    if (!r.records) return arg_fail("NULL output");
    if (r.n_draw_streams < 0 || r.n_draw_streams > kKfdbMaxKf || (r.n_draw_streams > 0 && !r.draws))
      return arg_fail("bad draw streams");
    sp = std::max(sp, (size_t)r.n_draw_streams);
    if (!r.nkf) continue;
    if (!r.kf_feat_off) return arg_fail("NULL keyframe arrays");
    if (r.kf_feat_off[0] != 0) return arg_fail("offsets must start at 0");
    for (int k = 0; k < r.nkf; k++) {
      const int nf = r.kf_feat_off[k + 1] - r.kf_feat_off[k];
      if (nf < 0 || nf > (int)P) return arg_fail("a keyframe has more features than kp_pitch");
    }
    if (r.kf_feat_off[r.nkf] > 0 &&
        (!r.kf_angle || !r.kf_feat_node || !r.kf_desc || !r.kf_valid || !r.mp_xyz ||
         !r.mp_min_dist || !r.mp_max_dist || !r.mp_desc))
      return arg_fail("NULL keyframe feature arrays");
  }
  RelocRows R(probs, NP, P, h->draw_pitch, entp, qp, sp);
  Grow* g = h->in;
  int gi = 0;
  hipError_t e = hipSuccess;
  orbrl_device_batch b{};
  b.d_nkf = upload(g[gi++], R.db.nkf.h, &e);
  b.d_kf_off = upload(g[gi++], R.db.kf_off.h, &e);
  b.d_covis = upload(g[gi++], R.db.covis.h, &e);
  b.d_q_n = upload(g[gi++], R.db.q_n.h, &e);
  b.d_n = upload(g[gi++], R.n.h, &e);
  b.d_feat_node = upload(g[gi++], R.feat_node.h, &e);
  b.d_kf_n = upload(g[gi++], R.kf_n.h, &e);
  b.d_kf_feat_node = upload(g[gi++], R.kf_feat_node.h, &e);
  b.d_draws = upload(g[gi++], R.draws.h, &e);
  b.d_n_streams = upload(g[gi++], R.n_streams.h, &e);
  b.d_kf_words = upload(g[gi++], R.db.kf_words.h, &e);
  b.d_q_words = upload(g[gi++], R.db.q_words.h, &e);
  b.d_kf_vals = upload(g[gi++], R.db.kf_vals.h, &e);
  b.d_q_vals = upload(g[gi++], R.db.q_vals.h, &e);
  b.d_reloc_score = upload(g[gi++], R.db.reloc_score.h, &e);
  b.d_uright = upload(g[gi++], R.uright.h, &e);
  b.d_kf_angle = upload(g[gi++], R.kf_angle.h, &e);
  b.d_mp_xyz = upload(g[gi++], R.mp_xyz.h, &e);
  b.d_mp_min_dist = upload(g[gi++], R.mp_min_dist.h, &e);
  b.d_mp_max_dist = upload(g[gi++], R.mp_max_dist.h, &e);
  b.d_kps_un = upload(g[gi++], R.kps_un.h, &e);
  b.d_desc = upload(g[gi++], R.desc.h, &e);
  b.d_kf_desc = upload(g[gi++], R.kf_desc.h, &e);
  b.d_kf_valid = upload(g[gi++], R.kf_valid.h, &e);
  b.d_mp_desc = upload(g[gi++], R.mp_desc.h, &e);
  b.d_kf_first = upload(g[gi++], R.kf_first.h, &e);
  HIP_CHECK(e);
  Grow& g_cand = g[gi++];
  Grow& g_nc = g[gi++];
  static_assert(kNumIn == 28, "one Grow per input array");
  HIP_CHECK(g_cand.need(bytes(R.cand)));
  HIP_CHECK(g_nc.need(bytes(R.ncand)));
  // ---- per-problem outputs ----
  Grow* o = h->prob + 7;
  HIP_CHECK(o[0].need(bytes(R.scalars)));
  HIP_CHECK(o[1].need(bytes(R.Tcw)));
  HIP_CHECK(o[2].need(bytes(R.mp_kf_feature)));
  HIP_CHECK(o[3].need(bytes(R.outlier)));
  HIP_CHECK(o[4].need(bytes(R.records)));
  b.ent_pitch = (int64_t)entp;
  b.q_pitch = (int64_t)qp;
  b.stream_pitch = (int32_t)sp;
  b.d_cand = g_cand.as<int32_t>();
  b.d_ncand = g_nc.as<int32_t>();
  b.d_ok = o[0].as<int32_t>();
  b.d_status = b.d_ok + NP;
  b.d_winner = b.d_ok + 2 * NP;
  b.d_rounds = b.d_ok + 3 * NP;
  b.d_n_good = b.d_ok + 4 * NP;
  b.d_n_candidates = b.d_ok + 5 * NP;
  b.d_Tcw = o[1].as<float>();
  b.d_mp_kf_feature = o[2].as<int32_t>();
  b.d_outlier = o[3].as<uint8_t>();
  b.d_records = o[4].as<int32_t>();
  const int rc = orbrl_relocalize_batch_device(h, &b, n, scoring, nullptr);   // the null stream
  if (rc) return rc;
  HIP_CHECK(download(R.scalars, b.d_ok));
  HIP_CHECK(download(R.cand, b.d_cand));
  HIP_CHECK(download(R.ncand, b.d_ncand));
  HIP_CHECK(download(R.mp_kf_feature, b.d_mp_kf_feature));
  HIP_CHECK(download(R.outlier, b.d_outlier));
  HIP_CHECK(download(R.records, b.d_records));
  HIP_CHECK(download(R.Tcw, b.d_Tcw));
  HIP_CHECK(download(R.db.reloc_score, b.d_reloc_score));
  const bool exhausted = R.unpack();
  return exhausted ? ORBPL_ERR_OVERFLOW : ORBPL_OK;
}

}  // extern "C"
