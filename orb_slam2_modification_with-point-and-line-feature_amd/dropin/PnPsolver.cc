#include "PnPsolver.h"

#include <algorithm>
#include <cstdlib>
#include <deque>
#include <mutex>
#include <stdexcept>

#include "orbpl.h"

namespace ORB_SLAM2 {

namespace {
// raw rand() values drawn ahead and not yet consumed, process-wide like rand()
std::deque<int32_t> g_draws;
std::mutex g_draws_mutex;
}  // namespace

PnPsolver::PnPsolver(const Frame& F, const std::vector<MapPoint*>& vpMapPointMatches)
    : mvpMapPointMatches(vpMapPointMatches) {
  // PnPsolver.cc:67-110
  for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {
    MapPoint* pMP = vpMapPointMatches[i];
    if (!pMP || pMP->isBad()) continue;
    const cv::KeyPoint& kp = F.mvKeysUn[i];
    mvP2D.push_back(kp.pt.x);
    mvP2D.push_back(kp.pt.y);
    mvSigma2.push_back(F.mvLevelSigma2[kp.octave]);
    cv::Mat Pos = pMP->GetWorldPos();
    for (int k = 0; k < 3; k++) mvP3Dw.push_back(Pos.at<float>(k, 0));
    mvKeyPointIndices.push_back(i);
  }
  fu = F.fx;
  fv = F.fy;
  uc = F.cx;
  vc = F.cy;
  SetRansacParameters();
}

PnPsolver::~PnPsolver() {}

void PnPsolver::SetRansacParameters(double probability, int minInliers, int maxIterations,
                                    int minSet, float epsilon, float th2) {
  if (minSet != ORBPNP_MIN_SET) throw std::runtime_error("PnPsolver: only minSet = 4 is built");
  N = (int)mvSigma2.size();
  mvMaxError.resize(N);
  int32_t mi, mx;
  if (orbpnp_ransac_parameters(N, probability, minInliers, maxIterations, minSet, epsilon, th2,
                               mvSigma2.data(), &mi, &mx, &mRansacEpsilon,
                               mvMaxError.data()) != ORBPL_OK)
    throw std::runtime_error(orbpl_last_error());
  mRansacMinInliers = mi;
  mRansacMaxIts = mx;
  mvbBestInliers.resize(N, 0);
}

cv::Mat PnPsolver::find(std::vector<bool>& vbInliers, int& nInliers) {
  bool bFlag;
  return iterate(mRansacMaxIts, bFlag, vbInliers, nInliers);
}

cv::Mat PnPsolver::iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers,
                           int& nInliers) {
  bNoMore = false;
  vbInliers.clear();
  nInliers = 0;
  if (N < mRansacMinInliers) {
    bNoMore = true;
    return cv::Mat();
  }
  const int H = std::max(0, std::max(mRansacMaxIts - mnIterations, nIterations));
  std::lock_guard<std::mutex> lock(g_draws_mutex);
  while ((int)g_draws.size() < 4 * H) g_draws.push_back(rand());
  std::vector<int32_t> draws(g_draws.begin(), g_draws.begin() + 4 * H);
  std::vector<uint8_t> inliers(N);
  float Tcw[16];
  int32_t result, no_more, n_inliers, consumed;
  orbpnp_problem P{};
  P.fx = fu;
  P.fy = fv;
  P.cx = uc;
  P.cy = vc;
  P.n = N;
  P.p2d = mvP2D.data();
  P.sigma2 = mvSigma2.data();
  P.p3d = mvP3Dw.data();
  P.min_inliers = mRansacMinInliers;
  P.max_its = mRansacMaxIts;
  P.max_error = mvMaxError.data();
  P.n_draws = (int32_t)draws.size();
  P.draws = draws.data();
  P.iterations = &mnIterations;
  P.best_inliers = &mnBestInliers;
  P.best_mask = mvbBestInliers.data();
  P.best_Tcw = mBestTcw;
  P.Tcw = Tcw;
  P.result = &result;
  P.no_more = &no_more;
  P.n_inliers = &n_inliers;
  P.inliers = inliers.data();
  P.draws_consumed = &consumed;
  if (orbpnp_iterate(&P, 1, nIterations) != ORBPL_OK) throw std::runtime_error(orbpl_last_error());
  g_draws.erase(g_draws.begin(), g_draws.begin() + consumed);
  bNoMore = no_more != 0;
  if (!result) return cv::Mat();
  nInliers = n_inliers;
  vbInliers = std::vector<bool>(mvpMapPointMatches.size(), false);
  for (int i = 0; i < N; i++)
    if (inliers[i]) vbInliers[mvKeyPointIndices[i]] = true;
  cv::Mat T(4, 4, cv::CV_32F);
  for (int r = 0; r < 4; r++)
    for (int c = 0; c < 4; c++) T.at<float>(r, c) = Tcw[4 * r + c];
  return T;
}

}  // namespace ORB_SLAM2
