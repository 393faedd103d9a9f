// Pieces of ORBmatcher shared by the projection matchers (k_match_last,
// k_match_local, k_match_kf) and the BoW matcher: the frame grid in LDS, the
// GetFeaturesInArea cell window, the kept candidate list and the rotation
// consistency check.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_ops.h"
#include "track_common.h"

namespace orbpl {

constexpr int kTopK = 4;        // candidates kept per map point in phase A
constexpr int kRotBins = 30;    // HISTO_LENGTH (ORBmatcher.cc:38)

// The cell window of Frame::GetFeaturesInArea(u, v, r) (Frame.cc:406-428);
// false when it lies outside the grid.
__device__ __forceinline__ bool grid_window(const TrackConsts& c, float u, float v, float r,
                                            int* cx0, int* cx1, int* cy0, int* cy1) {
  *cx0 = max(0, (int)floorf((u - c.minX - r) * c.gridInvW));
  *cx1 = min(kGridCols - 1, (int)ceilf((u - c.minX + r) * c.gridInvW));
  *cy0 = max(0, (int)floorf((v - c.minY - r) * c.gridInvH));
  *cy1 = min(kGridRows - 1, (int)ceilf((v - c.minY + r) * c.gridInvH));
  return !(*cx0 >= kGridCols || *cx1 < 0 || *cy0 >= kGridRows || *cy1 < 0);
}

// Stable insertion of v = dist << 16 | idx into tk[kTopK] (ascending distance,
// -1 = empty): equal distances keep scan order; once inserted, the displaced
// entries shift down one place each
__device__ __forceinline__ void topk_insert(int* tk, int v) {
  bool ins = false;
#pragma unroll
  for (int q = 0; q < kTopK; q++) {
    const int cur = tk[q];
    if (ins || cur < 0 || (v >> 16) < (cur >> 16)) {
      tk[q] = v;
      v = cur;
      ins = true;
      if (v < 0) break;
    }
  }
}

// rotation histogram bin of a match (ORBmatcher.cc:1836-1844)
__device__ __forceinline__ int rotation_bin(float angle_a, float angle_b) {
  float rot = angle_a - angle_b;
  if (rot < 0.0f) rot += 360.0f;
  int b = (int)roundf(rot * (kRotBins / 360.0f));
  if (b == kRotBins) b = 0;
  return b;
}

// ORBmatcher::ComputeThreeMaxima (ORBmatcher.cc:2035-2077) over the bin sizes
__device__ __forceinline__ void three_maxima(const int* hist, int& ind1, int& ind2, int& ind3) {
  int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;
  for (int i = 0; i < kRotBins; i++) {
    const int sz = hist[i];
    if (sz > max1) {
      max3 = max2; max2 = max1; max1 = sz; i3 = i2; i2 = i1; i1 = i;
    } else if (sz > max2) {
      max3 = max2; max2 = sz; i3 = i2; i2 = i;
    } else if (sz > max3) {
      max3 = sz; i3 = i;
    }
  }
  if (max2 < 0.1f * (float)max1) {
    i2 = -1; i3 = -1;
  } else if (max3 < 0.1f * (float)max1) {
    i3 = -1;
  }
  ind1 = i1; ind2 = i2; ind3 = i3;
}

// The rotation consistency check of the projection matchers by a block of NT
// threads: bin[i] >= 0 is the histogram bin of point i's match and sel[i] the
// keypoint it took. Marks the keypoints of matches outside the three largest
// bins in removed[] and returns how many. hist[] (zeroed) and misc[1..4] are
// LDS scratch.
template <int NT>
__device__ __forceinline__ int rotation_filter(const int* bin, const int* sel, int n, int* hist,
                                               uint32_t* removed, int* misc) {
  const int t = threadIdx.x;
  for (int i = t; i < n; i += NT)
    if (bin[i] >= 0) atomicAdd(&hist[bin[i]], 1);
  __syncthreads();
  if (t == 0) {
    int ind1, ind2, ind3;
    three_maxima(hist, ind1, ind2, ind3);
    misc[1] = ind1; misc[2] = ind2; misc[3] = ind3;
    misc[4] = 0;
  }
  __syncthreads();
  const int ind1 = misc[1], ind2 = misc[2], ind3 = misc[3];
  int nrem = 0;
  for (int i = t; i < n; i += NT) {
    const int b = bin[i];
    if (b >= 0 && b != ind1 && b != ind2 && b != ind3) {
      const int k = sel[i];
      atomicOr(&removed[k >> 5], 1u << (k & 31));
      nrem++;
    }
  }
  if (nrem) atomicAdd(&misc[4], nrem);
  __syncthreads();
  return misc[4];
}

// Frame::AssignFeaturesToGrid (Frame.cc:265-287) in LDS by a block of NT
// threads: a stable counting sort of the n keypoints by grid cell, cells
// numbered column-major (ix * kGridRows + iy) so that one grid column's cells
// are one contiguous run of items, each cell's keypoints in index order as the
// reference's mGrid[ix][iy] vectors. cell_of(i) does the caller's own
// per-keypoint work and returns keypoint i's cell or -1. cell_start has
// kGridCols * kGridRows + 1 entries; fill (as many counters as cells) is
// scratch.
template <int NT, class F>
__device__ __forceinline__ void build_frame_grid(int* cell_start, uint16_t* items, int16_t* gc,
                                                 int* fill, int* wsum, int n, F&& cell_of) {
  constexpr int kCells = kGridCols * kGridRows;
  static_assert(kCells % NT == 0, "cell scan split");
  const int t = threadIdx.x;
  for (int i = t; i < kCells; i += NT) cell_start[i] = 0;
  __syncthreads();
  for (int i = t; i < n; i += NT) {
    const int g = cell_of(i);
    gc[i] = (int16_t)g;
    if (g >= 0) atomicAdd(&cell_start[g], 1);
  }
  __syncthreads();
  block_exclusive_scan<kCells / NT, NT>(cell_start, wsum, fill);
  // place items (any order), then sort each cell by index
  for (int i = t; i < n; i += NT) {
    const int g = gc[i];
    if (g >= 0) items[atomicAdd(&fill[g], 1)] = (uint16_t)i;
  }
  __syncthreads();
  for (int cell = t; cell < kCells; cell += NT) {
    const int b = cell_start[cell], e = cell_start[cell + 1];
    for (int q = b + 1; q < e; q++) {
      const uint16_t v = items[q];
      int r = q - 1;
      while (r >= b && items[r] > v) {
        items[r + 1] = items[r];
        r--;
      }
      items[r + 1] = v;
    }
  }
  __syncthreads();
}

}  // namespace orbpl
