// Drop-in ORB_SLAM2::Tracking::Relocalization (see Tracking.h).
#include "Tracking.h"

#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>

namespace ORB_SLAM2 {

Tracking::Tracking(ORBVocabulary* pVoc, KeyFrameDatabase* pKFDB, int drawPitch)
    : mpKeyFrameDB(pKFDB), mpORBVocabulary(pVoc), mnDrawPitch(drawPitch) {}

Tracking::~Tracking() { orbrl_destroy(mpHandle); }

static std::vector<int32_t> nodes_of(const DBoW2::FeatureVector& fv, int n) {
  std::vector<int32_t> node(n > 0 ? n : 1, -1);
  for (const auto& kv : fv)
    for (unsigned i : kv.second)
      if ((int)i < n) node[i] = (int32_t)kv.first;
  return node;
}

bool Tracking::Relocalization() {
  Frame& F = mCurrentFrame;
  std::vector<KeyFrame*> vpKFs;
  for (KeyFrame* pKF : mpKeyFrameDB->GetKeyFrames())
    if (!pKF->isBad()) vpKFs.push_back(pKF);
  const int nkf = (int)vpKFs.size();
  if (nkf > ORBKF_MAX_KEYFRAMES) throw std::runtime_error("more than 64 keyframes in the database");
  // P30: one stream per database keyframe, in order. Drawn before anything
  // else: the values that follow the caller's srand() go to the solvers,
  // whatever the first use of the device does with rand()
  std::vector<int32_t> draws((size_t)(nkf > 0 ? nkf : 1) * mnDrawPitch);
  for (size_t i = 0; i < (size_t)nkf * mnDrawPitch; i++) draws[i] = rand();
  // Step 1 (Tracking.cc:2054)
  F.ComputeBoW();
  int most = F.N;
  for (KeyFrame* pKF : vpKFs) most = std::max(most, pKF->N);
  const int pitch = most <= 1024 ? 1024 : 2048;
  if (most > 2048) throw std::runtime_error("more than 2048 keypoints");
  if (!mpHandle || mnHandlePitch != pitch) {
    orbrl_destroy(mpHandle);
    mpHandle = nullptr;
    const orbpl_camera cam = F.Camera();
    if (orbrl_create(&cam, F.mvScaleFactors.data(), F.mvLevelSigma2.data(), F.mnScaleLevels, 1,
                     pitch, mnDrawPitch, &mpHandle) != ORBPL_OK)
      throw std::runtime_error(orbpl_last_error());
    mnHandlePitch = pitch;
  }
  // ---- the database and its keyframes' features ----
  std::map<const KeyFrame*, int> index;
  for (int k = 0; k < nkf; k++) index[vpKFs[k]] = k;
  std::vector<int32_t> off(nkf + 1, 0), foff(nkf + 1, 0), kfnode;
  std::vector<int32_t> covis((size_t)(nkf > 0 ? nkf : 1) * ORBKF_COVISIBLES, -1);
  std::vector<uint32_t> words;
  std::vector<double> vals;
  std::vector<float> score(nkf > 0 ? nkf : 1, 0.0f), angle, xyz, dmin, dmax;
  std::vector<uint8_t> kdesc, valid, mpdesc;
  for (int k = 0; k < nkf; k++) {
    KeyFrame* pKF = vpKFs[k];
    for (const auto& wv : pKF->mBowVec) {
      words.push_back(wv.first);
      vals.push_back(wv.second);
    }
    off[k + 1] = (int32_t)words.size();
    const std::vector<KeyFrame*> vpNeighs = pKF->GetBestCovisibilityKeyFrames(ORBKF_COVISIBLES);
    for (size_t c = 0; c < vpNeighs.size() && c < ORBKF_COVISIBLES; c++) {
      const auto it = index.find(vpNeighs[c]);
      if (it != index.end()) covis[(size_t)k * ORBKF_COVISIBLES + c] = it->second;
    }
    score[k] = pKF->mRelocScore;
    const int M = pKF->N;
    foff[k + 1] = foff[k] + M;
    const std::vector<int32_t> node = nodes_of(pKF->mFeatVec, M);
    kfnode.insert(kfnode.end(), node.begin(), node.begin() + M);
    const std::vector<MapPoint*> vpMPs = pKF->GetMapPointMatches();
    for (int j = 0; j < M; j++) {
      angle.push_back(pKF->mvKeysUn[j].angle);
      const uint8_t* d = pKF->mDescriptors.data + 32 * (size_t)j;
      kdesc.insert(kdesc.end(), d, d + 32);
      MapPoint* pMP = j < (int)vpMPs.size() ? vpMPs[j] : nullptr;
      const bool ok = pMP && !pMP->isBad();
      valid.push_back(ok ? 1 : 0);
      float X[3] = {0, 0, 0};
      uint8_t md[32] = {0};
      if (ok) {
        const cv::Mat P = pMP->GetWorldPos(), D = pMP->GetDescriptor();
        for (int a = 0; a < 3; a++) X[a] = P.at<float>(a, 0);
        std::memcpy(md, D.data, 32);
      }
      xyz.insert(xyz.end(), X, X + 3);
      dmin.push_back(ok ? pMP->GetMinDistance() : 0.0f);
      dmax.push_back(ok ? pMP->GetMaxDistance() : 0.0f);
      mpdesc.insert(mpdesc.end(), md, md + 32);
    }
  }
  // ---- the frame ----
  const int N = F.N;
  const std::vector<int32_t> fnode = nodes_of(F.mFeatVec, N);
  std::vector<uint32_t> qw;
  std::vector<double> qv;
  for (const auto& wv : F.mBowVec) {
    qw.push_back(wv.first);
    qv.push_back(wv.second);
  }
  std::vector<float> uright(N > 0 ? N : 1, -1.0f);
  for (int i = 0; i < N && i < (int)F.mvuRight.size(); i++) uright[i] = F.mvuRight[i];
  std::vector<int32_t> match(N > 0 ? N : 1, -1), records(64 * ORBRL_REC_INTS, 0);
  std::vector<uint8_t> outlier(N > 0 ? N : 1, 0);
  orbrl_problem P{};
  P.nkf = nkf;
  P.kf_off = off.data();
  P.kf_words = words.data();
  P.kf_vals = vals.data();
  P.covis = covis.data();
  P.reloc_score = score.data();
  P.kf_feat_off = foff.data();
  P.kf_angle = angle.data();
  P.kf_feat_node = kfnode.data();
  P.kf_desc = kdesc.data();
  P.kf_valid = valid.data();
  P.mp_xyz = xyz.data();
  P.mp_min_dist = dmin.data();
  P.mp_max_dist = dmax.data();
  P.mp_desc = mpdesc.data();
  P.n = N;
  P.kps_un = reinterpret_cast<const orbpl_keypoint*>(F.mvKeysUn.data());
  P.uright = uright.data();
  P.desc = F.mDescriptors.data;
  P.feat_node = fnode.data();
  P.nq_words = (int32_t)qw.size();
  P.q_words = qw.data();
  P.q_vals = qv.data();
  P.n_draw_streams = nkf;
  P.draws = draws.data();
  P.mp_kf_feature = match.data();
  P.outlier = outlier.data();
  P.records = records.data();
  int info[6] = {0, 0, 0, 0, 0, 0};
  if (mpORBVocabulary && mpORBVocabulary->handle() &&
      orbv_info(mpORBVocabulary->handle(), info) != ORBPL_OK)
    throw std::runtime_error(orbpl_last_error());
  const int rc = orbrl_relocalize(mpHandle, &P, 1, info[2]);
  if (rc != ORBPL_OK && rc != ORBPL_ERR_OVERFLOW) throw std::runtime_error(orbpl_last_error());
  for (int k = 0; k < nkf; k++) vpKFs[k]->mRelocScore = score[k];
  mnRelocStatus = P.status;
  mnRelocRounds = P.rounds;
  mnRelocGood = P.n_good;
  mvpRelocCandidates.clear();
  for (int c = 0; c < P.ncand; c++) mvpRelocCandidates.push_back(vpKFs[P.cand[c]]);
  mvRelocRecords.assign(records.begin(), records.begin() + (size_t)P.ncand * ORBRL_REC_INTS);
  F.mvpMapPoints.assign(N, nullptr);
  F.mvbOutlier.assign(N, false);
  mpRelocKF = nullptr;
  if (!P.ok) return false;
  mpRelocKF = vpKFs[P.winner];
  cv::Mat Tcw;
  Tcw.create(4, 4, cv::CV_32F);
  std::memcpy(Tcw.ptr<float>(), P.Tcw, 64);
  F.SetPose(Tcw);
  for (int i = 0; i < N; i++) {
    if (match[i] < 0) continue;
    F.mvpMapPoints[i] = mpRelocKF->GetMapPoint(match[i]);
    F.mvbOutlier[i] = outlier[i] != 0;
  }
  mnLastRelocFrameId = F.mnId;
  return true;
}

}  // namespace ORB_SLAM2
