// Minimal ORB_SLAM2::KeyFrame stand-in (include/KeyFrame.h, src/KeyFrame.cc:
// 36-80): the members TrackReferenceKeyFrame's matchers read from the
// reference keyframe - its undistorted keypoints, descriptors, map point
// matches and FeatureVector (ORBmatcher::SearchByBoW, ORBmatcher.cc:247-410),
// its key lines, line descriptors and map lines (LineMatcher::
// SearchByProjection(Frame&, KeyFrame*), LineMatcher.cpp:527-721) - copied
// from the Frame it is made of, as KeyFrame::KeyFrame(Frame&, ...) does; the
// relocalisation state KeyFrameDatabase::DetectRelocalizationCandidates keeps
// in it (mnRelocQuery, mnRelocWords, mRelocScore) and the ordered covisibles
// it reads, set by the caller (SetOrderedCovisibles). The covisibility graph,
// spanning tree and map bookkeeping stay the caller's.
#pragma once
#include <stdexcept>
#include <vector>

#include "Frame.h"

namespace ORB_SLAM2 {

class KeyFrame {
 public:
  explicit KeyFrame(const Frame& F)
      : mnFrameId(F.mnId), N(F.N), NL(F.NL), mvKeys(F.mvKeys), mvKeysUn(F.mvKeysUn),
        mvuRight(F.mvuRight), mvDepth(F.mvDepth), mDescriptors(F.mDescriptors.clone()),
        mBowVec(F.mBowVec), mFeatVec(F.mFeatVec), mvKeyLines(F.mvKeyLines),
        mvKeyLinesUn(F.mvKeyLinesUn), mLineDescriptors(F.mLineDescriptors.clone()),
        mvpMapLines(F.mvpMapLines), mvScaleFactors(F.mvScaleFactors),
        mpORBvocabulary(F.mpORBvocabulary), mvpMapPoints(F.mvpMapPoints),
        Tcw(F.mTcw.clone()) {
    mnId = nNextId++;
    fx = Frame::fx; fy = Frame::fy; cx = Frame::cx; cy = Frame::cy;
    invfx = 1.0f / fx;
    invfy = 1.0f / fy;
    mbf = F.mbf;
    mb = mbf / fx;
    mvLevelSigma2 = F.mvLevelSigma2;
  }

  // KeyFrame::ComputeBoW (KeyFrame.cc:67-80)
  void ComputeBoW() {
    if (!mpORBvocabulary) throw std::runtime_error("KeyFrame::ComputeBoW: no vocabulary");
    if (mBowVec.empty() || mFeatVec.empty())
      mpORBvocabulary->transform(toDescriptorVector(mDescriptors), mBowVec, mFeatVec, 4);
  }
  std::vector<MapPoint*> GetMapPointMatches() const { return mvpMapPoints; }
  std::vector<MapLine*> GetMapLineMatches() const { return mvpMapLines; }
  MapPoint* GetMapPoint(const size_t& idx) const { return mvpMapPoints[idx]; }
  cv::Mat GetPose() const { return Tcw.clone(); }
  const float* TcwData() const { return Tcw.ptr<float>(); }
  // what both SearchForTriangulation and LocalMapping::ComputeF12 read
  // (KeyFrame.cc:56-131): Rcw, tcw and Ow = -Rwc * tcw (double accumulation,
  // one rounding: DESIGN.md P6)
  cv::Mat GetRotation() const {
    cv::Mat R(3, 3, cv::CV_32F);
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) R.at<float>(r, c) = Tcw.at<float>(r, c);
    return R;
  }
  cv::Mat GetTranslation() const {
    cv::Mat t(3, 1, cv::CV_32F);
    for (int r = 0; r < 3; r++) t.at<float>(r, 0) = Tcw.at<float>(r, 3);
    return t;
  }
  cv::Mat GetCameraCenter() const {
    cv::Mat Ow(3, 1, cv::CV_32F);
    for (int r = 0; r < 3; r++) {
      double s = (double)Tcw.at<float>(0, r) * Tcw.at<float>(0, 3);
      s += (double)Tcw.at<float>(1, r) * Tcw.at<float>(1, 3);
      s += (double)Tcw.at<float>(2, r) * Tcw.at<float>(2, 3);
      Ow.at<float>(r, 0) = (float)(s * -1.0);
    }
    return Ow;
  }
  bool isBad() const { return mbBad; }
  void SetBadFlag() { mbBad = true; }
  // KeyFrame::GetBestCovisibilityKeyFrames (KeyFrame.cc:250-258): the first N
  // of the ordered covisibles, which the caller's covisibility graph sets
  // (mvpOrderedConnectedKeyFrames after UpdateBestCovisibles)
  void SetOrderedCovisibles(const std::vector<KeyFrame*>& v) { mvpOrderedConnectedKeyFrames = v; }
  std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) const {
    if ((int)mvpOrderedConnectedKeyFrames.size() < N) return mvpOrderedConnectedKeyFrames;
    return std::vector<KeyFrame*>(mvpOrderedConnectedKeyFrames.begin(),
                                  mvpOrderedConnectedKeyFrames.begin() + N);
  }

  static long unsigned int nNextId;
  long unsigned int mnId = 0;
  const long unsigned int mnFrameId;
  // KeyFrameDatabase::DetectRelocalizationCandidates' per-keyframe state
  // (KeyFrame.h:226-228). The reference never initialises mRelocScore
  // (KeyFrame.cc:32); pinned: it starts at 0.0f
  long unsigned int mnRelocQuery = 0;
  int mnRelocWords = 0;
  float mRelocScore = 0.0f;
  const int N, NL;
  const std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
  const std::vector<float> mvuRight, mvDepth;
  const cv::Mat mDescriptors;
  DBoW2::BowVector mBowVec;
  DBoW2::FeatureVector mFeatVec;
  const std::vector<KeyLine> mvKeyLines, mvKeyLinesUn;
  const cv::Mat mLineDescriptors;
  std::vector<MapLine*> mvpMapLines;   // public in the fork (LineMatcher.cpp:561)
  const std::vector<float> mvScaleFactors;
  std::vector<float> mvLevelSigma2;
  float fx = 0, fy = 0, cx = 0, cy = 0, invfx = 0, invfy = 0, mbf = 0, mb = 0;
  ORBVocabulary* mpORBvocabulary;

 private:
  std::vector<MapPoint*> mvpMapPoints;
  cv::Mat Tcw;
  std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
  bool mbBad = false;
};

}  // namespace ORB_SLAM2
