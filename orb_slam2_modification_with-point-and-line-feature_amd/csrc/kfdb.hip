// KeyFrameDatabase::DetectRelocalizationCandidates (KeyFrameDatabase.cc:274-412)
// on gfx950, batched: one 256-thread workgroup per (database, query) problem.
//   stage    - the query's BowVector (words, values) into LDS
//   pass 1   - one wave per keyframe: every entry of the keyframe's BowVector
//              looks its word up in the query (binary search in LDS); the wave
//              reduces mnRelocWords and the first shared word
//   order    - wave 0, lane = keyframe: lKFsSharingWords is ordered by (first
//              shared word, database index) - the reference walks the query's
//              words ascending and each inverted-file list in insertion order -
//              so a keyframe's list position is its rank by that key;
//              maxCommonWords, minCommonWords = int(max * 0.8f)
//   pass 2   - one wave per scored keyframe: L1Scoring::score
//              (ScoringObject.cpp:23-68). The terms of 64 entries are computed
//              in parallel; every addition happens in ascending word order
//              (the ballot's set lanes, lowest first), in double
//   groups   - wave 0, lane = list position: the float sum over the ordered
//              covisibles that share a word, best of group with strict >
//   result   - lane 0: bestAccScore, 0.75f threshold, first occurrences kept
// mRelocScore persists across queries: a keyframe scored here
// is overwritten, every other entry is read as it came in.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "../../include/orbpl.h"
#include "block_ops.h"
#include "host_rows.h"
#include "host_stage.h"
#include "orbpl_runtime.h"
#include "reloc_kernels.h"

namespace orbpl {

namespace {

constexpr int kKfdbThreads = 256;
constexpr int kKfdbWaves = kKfdbThreads / 64;
static_assert(kKfdbMaxKf == 64, "one lane per keyframe in the ordered passes");

struct KfdbShared {
  double qv[kKfdbMaxWords];
  uint32_t qw[kKfdbMaxWords];
  int words[kKfdbMaxKf];        // mnRelocWords
  uint32_t first[kKfdbMaxKf];   // first shared word
  float score[kKfdbMaxKf];      // mRelocScore
  int order[kKfdbMaxKf];        // lKFsSharingWords
  int scored[kKfdbMaxKf];
  float acc[kKfdbMaxKf];        // lAccScoreAndMatch, by list position
  int best[kKfdbMaxKf];
  int nshare;
};

// position of word w in the ascending qw[0, qn), or -1
__device__ __forceinline__ int find_word(const uint32_t* qw, int qn, uint32_t w) {
  int lo = 0, hi = qn;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (qw[mid] < w) lo = mid + 1;
    else hi = mid;
  }
  return (lo < qn && qw[lo] == w) ? lo : -1;
}

}  // namespace

__global__ void __launch_bounds__(kKfdbThreads) k_kfdb_reloc(KfdbArgs a) {
  __shared__ KfdbShared S;
  const int p = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63;
  const int nk = min(max(a.nkf[p], 0), kKfdbMaxKf);
  const int qn = min(max(a.q_n[p], 0), kKfdbMaxWords);
  const int* off = a.kf_off + (long long)p * (kKfdbMaxKf + 1);
  const uint32_t* kw = a.kf_words + (long long)p * a.ent_pitch;
  const double* kv = a.kf_vals + (long long)p * a.ent_pitch;
  const int* covis = a.covis + (long long)p * kKfdbMaxKf * kKfdbCovis;
  float* rscore = a.reloc_score + (long long)p * kKfdbMaxKf;
  int* cand = a.cand + (long long)p * kKfdbMaxKf;
  for (int i = t; i < qn; i += kKfdbThreads) {
    S.qw[i] = a.q_words[(long long)p * a.q_pitch + i];
    S.qv[i] = a.q_vals[(long long)p * a.q_pitch + i];
  }
  if (t < kKfdbMaxKf) {
    S.words[t] = 0;
    S.first[t] = 0xFFFFFFFFu;
    S.scored[t] = 0;
    S.score[t] = t < nk ? rscore[t] : 0.0f;
  }
  __syncthreads();
  // ---- pass 1: mnRelocWords and the first shared word of every keyframe ----
  for (int kf = wave; kf < nk; kf += kKfdbWaves) {
    const int b = off[kf], e = off[kf + 1];
    int cnt = 0;
    uint32_t fw = 0xFFFFFFFFu;
    for (int i = b + lane; i < e; i += 64) {
      const uint32_t w = kw[i];
      if (find_word(S.qw, qn, w) >= 0) {
        cnt++;
        fw = min(fw, w);
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      cnt += __shfl_xor(cnt, o, 64);
      fw = min(fw, (uint32_t)__shfl_xor((int)fw, o, 64));
    }
    if (lane == 0) {
      S.words[kf] = cnt;
      S.first[kf] = fw;
    }
  }
  __syncthreads();
  // ---- list order, maxCommonWords, who is scored ----
  if (wave == 0) {
    const int w = lane < nk ? S.words[lane] : 0;
    const bool share = w > 0;
    const unsigned long long key = ((unsigned long long)S.first[lane] << 6) | (unsigned)lane;
    int rank = 0;
    for (int k = 0; k < nk; k++) {
      const unsigned long long kk = ((unsigned long long)S.first[k] << 6) | (unsigned)k;
      rank += (S.words[k] > 0 && kk < key) ? 1 : 0;
    }
    if (share) S.order[rank] = lane;
    int maxw = w;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) maxw = max(maxw, __shfl_xor(maxw, o, 64));
    const int minCommon = (int)((float)maxw * 0.8f);
    S.scored[lane] = (share && w > minCommon) ? 1 : 0;
    const unsigned long long sm = __ballot(share);
    if (lane == 0) S.nshare = __popcll(sm);
    if (a.common_words && lane < nk) a.common_words[(long long)p * kKfdbMaxKf + lane] = w;
  }
  __syncthreads();
  const int nshare = S.nshare;
  if (nshare == 0) {
    if (t == 0) a.ncand[p] = 0;
    return;
  }
  // ---- pass 2: L1 score of the scored keyframes ----
  for (int kf = wave; kf < nk; kf += kKfdbWaves) {
    if (!S.scored[kf]) continue;
    const int b = off[kf], e = off[kf + 1];
    double sum = 0;
    for (int base = b; base < e; base += 64) {
      const int i = base + lane;
      double term = 0;
      bool hit = false;
      if (i < e) {
        const int q = find_word(S.qw, qn, kw[i]);
        if (q >= 0) {
          const double vi = S.qv[q], wi = kv[i];
          term = fabs(vi - wi) - fabs(vi) - fabs(wi);
          hit = true;
        }
      }
      unsigned long long m = __ballot(hit);
      while (m) {
        const int l = __ffsll((long long)m) - 1;
        sum += __shfl(term, l, 64);
        m &= m - 1;
      }
    }
    const float si = (float)(-sum / 2.0);
    if (lane == 0) {
      S.score[kf] = si;
      rscore[kf] = si;
    }
  }
  __syncthreads();
  // ---- covisibility groups, threshold, de-duplication ----
  if (wave == 0) {
    int bestKF = -1;
    float accScore = 0;
    if (lane < nshare) {
      const int kf = S.order[lane];
      if (S.scored[kf]) {
        float bestScore = S.score[kf];
        accScore = bestScore;
        bestKF = kf;
        for (int c = 0; c < kKfdbCovis; c++) {
          const int k2 = covis[kf * kKfdbCovis + c];
          if (k2 < 0 || k2 >= nk || S.words[k2] <= 0) continue;
          const float s2 = S.score[k2];
          accScore += s2;
          if (s2 > bestScore) {
            bestKF = k2;
            bestScore = s2;
          }
        }
      }
    }
    S.acc[lane] = accScore;
    S.best[lane] = bestKF;
    lds_wave_sync();
    if (lane == 0) {
      float bestAcc = 0;
      for (int r = 0; r < nshare; r++)
        if (S.best[r] >= 0 && S.acc[r] > bestAcc) bestAcc = S.acc[r];
      const float minScoreToRetain = 0.75f * bestAcc;
      unsigned long long added = 0;
      int n = 0;
      for (int r = 0; r < nshare; r++) {
        const int k = S.best[r];
        if (k < 0 || !(S.acc[r] > minScoreToRetain)) continue;
        if ((added >> k) & 1ull) continue;
        added |= 1ull << k;
        cand[n++] = k;
      }
      a.ncand[p] = n;
    }
  }
}

void launch_kfdb_reloc(const KfdbArgs& a, int nq, hipStream_t s) {
  if (nq <= 0) return;
  hipLaunchKernelGGL(k_kfdb_reloc, dim3(nq), dim3(kKfdbThreads), 0, s, a);
}

}  // namespace orbpl

using namespace orbpl;

extern "C" {

int orbkf_detect_reloc_batch_device(const orbkf_device_batch* b, int nq, int scoring,
                                    void* stream) {
  if (scoring != 0) return arg_fail("only the vocabulary's L1 scoring (L1_NORM = 0) is built");
  if (!b || nq < 0) return arg_fail("bad argument");
  if (nq == 0) return ORBPL_OK;
  if (!b->d_nkf || !b->d_kf_off || !b->d_kf_words || !b->d_kf_vals || !b->d_covis ||
      !b->d_reloc_score || !b->d_q_n || !b->d_q_words || !b->d_q_vals || !b->d_cand || !b->d_ncand)
    return arg_fail("NULL device array");
  if (b->ent_pitch < 0 || b->q_pitch < 0) return arg_fail("negative pitch");
  KfdbArgs a{b->d_nkf, b->d_kf_off, b->d_kf_words, b->d_kf_vals, b->ent_pitch, b->d_covis,
             b->d_reloc_score, b->d_q_n, b->d_q_words, b->d_q_vals, b->q_pitch, b->d_cand,
             b->d_ncand, b->d_common_words};
  launch_kfdb_reloc(a, nq, (hipStream_t)stream);
  HIP_CHECK(hipGetLastError());
  return ORBPL_OK;
}

int orbkf_detect_reloc(const orbkf_problem* P, int nq, int scoring) {
  if (scoring != 0) return arg_fail("only the vocabulary's L1 scoring (L1_NORM = 0) is built");
  if (nq < 0 || (nq > 0 && !P)) return arg_fail("bad argument");
  if (nq == 0) return ORBPL_OK;
  size_t entp = 1, qp = 1;
  for (int p = 0; p < nq; p++) {
    if (const char* no = kfdb_refusal(P[p], "kf_off[0] != 0", &entp, &qp)) return arg_fail(no);
    if (!P[p].cand || !P[p].ncand) return arg_fail("NULL output");
  }
  KfdbCallRows R(P, nq, entp, qp);
  HostStage st;
  KfdbArgs a{st.in(R.db.nkf),
             st.in(R.db.kf_off),
             st.in(R.db.kf_words),
             st.in(R.db.kf_vals),
             (long long)entp,
             st.in(R.db.covis),
             st.inout(R.db.reloc_score),
             st.in(R.db.q_n),
             st.in(R.db.q_words),
             st.in(R.db.q_vals),
             (long long)qp,
             st.out(R.cand),
             st.out(R.ncand),
             st.zeros(R.common_words)};
  if (st.rc()) return st.rc();
  launch_kfdb_reloc(a, nq, nullptr);   // host-pointer APIs use the null stream
  st.launched();
  st.back_outs();
  if (st.rc()) return st.rc();
  R.unpack();
  return ORBPL_OK;
}

}  // extern "C"
