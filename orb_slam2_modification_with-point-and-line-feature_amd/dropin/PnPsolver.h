// ORB_SLAM2::PnPsolver with the reference's public signatures
// (include/PnPsolver.h:64-76), backed by orbpnp_iterate: the RANSAC hypotheses
// and Refine() run on the device, the persistent state (mnIterations,
// mnBestInliers, mvbBestInliers, mBestTcw) is kept here between calls.
// The reference draws from the process-wide rand(); so does this class,
// through a process-wide look-ahead queue: a call is handed 4 raw rand()
// values per hypothesis it may run, the ones it did not consume stay queued
// for the next call of any solver.
#pragma once
#include <cstdint>
#include <vector>

#include "Frame.h"
#include "MapPoint.h"

namespace ORB_SLAM2 {

class PnPsolver {
 public:
  PnPsolver(const Frame& F, const std::vector<MapPoint*>& vpMapPointMatches);
  ~PnPsolver();

  void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300,
                           int minSet = 4, float epsilon = 0.4, float th2 = 5.991);

  cv::Mat find(std::vector<bool>& vbInliers, int& nInliers);

  cv::Mat iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers);

 private:
  std::vector<MapPoint*> mvpMapPointMatches;
  std::vector<float> mvP2D, mvSigma2, mvP3Dw, mvMaxError;  // x y / sigma2 / x y z per correspondence
  std::vector<size_t> mvKeyPointIndices;
  float fu, fv, uc, vc;
  int N = 0;
  // adjusted RANSAC parameters
  int mRansacMinInliers = 0, mRansacMaxIts = 0;
  float mRansacEpsilon = 0;
  // state across iterate() calls
  int32_t mnIterations = 0, mnBestInliers = 0;
  std::vector<uint8_t> mvbBestInliers;
  float mBestTcw[16] = {0};
};

}  // namespace ORB_SLAM2
