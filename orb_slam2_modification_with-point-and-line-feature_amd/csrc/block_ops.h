// Device-only wave and block helpers shared by the kernels: the 256-bit
// descriptor distance, block sums / ordered compaction / counter scans over
// 64-lane waves, the LDS bitonic sort and the one-wave LDS fence.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace orbpl {

// Hamming distance of two 256-bit descriptors (ORB, LBD), each as two 16-byte
// halves (ORBmatcher::DescriptorDistance, ORBmatcher.cc:2082-2099)
__device__ __forceinline__ int hamming256(const uint4 a0, const uint4 a1, const uint4 b0,
                                          const uint4 b1) {
  return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
         __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// one descriptor held in registers, the other in memory (two 16-byte loads)
__device__ __forceinline__ int hamming256(const uint4 a0, const uint4 a1, const uint4* b) {
  const uint4 b0 = b[0], b1 = b[1];
  return hamming256(a0, a1, b0, b1);
}

// both in memory, 16-byte aligned
__device__ __forceinline__ int hamming256(const uint8_t* a, const uint8_t* b) {
  const uint4 a0 = *reinterpret_cast<const uint4*>(a);
  const uint4 a1 = *reinterpret_cast<const uint4*>(a + 16);
  return hamming256(a0, a1, reinterpret_cast<const uint4*>(b));
}

// the wave's LDS operations so far are complete and the compiler moves no
// memory access across (one wave: LDS executes its operations in order). Unlike
// a workgroup fence it does not wait for the wave's outstanding global loads
// (phase B's next-chunk prefetch).
__device__ __forceinline__ void lds_wave_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// sum of v over a block of kWaves waves (wsum: kWaves ints of LDS)
template <int kWaves = 4>
__device__ __forceinline__ int block_sum(int v, int* wsum) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  if (lane == 0) wsum[wave] = v;
  __syncthreads();
  int r = 0;
#pragma unroll
  for (int w = 0; w < kWaves; w++) r += wsum[w];
  __syncthreads();
  return r;
}

// ordered block compaction: position of this thread's flagged element among
// the block's flagged ones (thread order); the block's total in *total
template <int kWaves = 4>
__device__ __forceinline__ int block_prefix(bool flag, int* wsum, int* total) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const unsigned long long m = __ballot(flag);
  if (lane == 0) wsum[wave] = __popcll(m);
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < kWaves; w++) {
    if (w < wave) off += wsum[w];
    tot += wsum[w];
  }
  __syncthreads();
  *total = tot;
  return off + __popcll(m & ((1ull << lane) - 1ull));
}

// Exclusive scan of kPer * NT counters in LDS by a block of NT threads, kPer
// consecutive counters per thread: counts[] becomes the starts, fill[] (if
// given) a second copy of them, counts[kPer * NT] the grand total. The caller
// has synchronised the counts; the results are synchronised on return.
template <int kPer, int NT>
__device__ __forceinline__ void block_exclusive_scan(int* counts, int* wsum, int* fill) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  int loc[kPer];
  int sum = 0;
#pragma unroll
  for (int k = 0; k < kPer; k++) {
    loc[k] = counts[t * kPer + k];
    sum += loc[k];
  }
  int incl = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(incl, o, 64);
    if (lane >= o) incl += u;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int run = incl - sum;
  for (int w = 0; w < wave; w++) run += wsum[w];
#pragma unroll
  for (int k = 0; k < kPer; k++) {
    counts[t * kPer + k] = run;
    if (fill) fill[t * kPer + k] = run;
    run += loc[k];
  }
  if (t == NT - 1) counts[kPer * NT] = run;
  __syncthreads();
}

// ascending bitonic sort of n (a power of two) keys in LDS by the whole block
// of `stride` threads
template <class T>
__device__ __forceinline__ void bitonic_sort(T* keys, int n, int stride) {
  for (int k = 2; k <= n; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < n; i += stride) {
        const int l = i ^ j;
        if (l > i) {
          const T x = keys[i], y = keys[l];
          if (((i & k) == 0) ? (x > y) : (x < y)) {
            keys[i] = y;
            keys[l] = x;
          }
        }
      }
      __syncthreads();
    }
}

}  // namespace orbpl
