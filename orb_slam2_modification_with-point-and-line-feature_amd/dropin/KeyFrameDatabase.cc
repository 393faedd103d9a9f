// Drop-in ORB_SLAM2::KeyFrameDatabase (see KeyFrameDatabase.h).
#include "KeyFrameDatabase.h"

#include <algorithm>
#include <map>
#include <stdexcept>

namespace ORB_SLAM2 {

KeyFrameDatabase::KeyFrameDatabase(const ORBVocabulary& voc) : mpVoc(&voc) {}

void KeyFrameDatabase::add(KeyFrame* pKF) {
  std::unique_lock<std::mutex> lock(mMutex);
  mvKeyFrames.push_back(pKF);
}

void KeyFrameDatabase::erase(KeyFrame* pKF) {
  std::unique_lock<std::mutex> lock(mMutex);
  mvKeyFrames.erase(std::remove(mvKeyFrames.begin(), mvKeyFrames.end(), pKF), mvKeyFrames.end());
}

void KeyFrameDatabase::clear() {
  std::unique_lock<std::mutex> lock(mMutex);
  mvKeyFrames.clear();
}

std::vector<KeyFrame*> KeyFrameDatabase::DetectRelocalizationCandidates(Frame* F) {
  std::unique_lock<std::mutex> lock(mMutex);
  const int nkf = (int)mvKeyFrames.size();
  std::map<const KeyFrame*, int> index;
  for (int k = 0; k < nkf; k++) index[mvKeyFrames[k]] = k;
  std::vector<int32_t> off(nkf + 1, 0), covis((size_t)(nkf > 0 ? nkf : 1) * ORBKF_COVISIBLES, -1);
  std::vector<uint32_t> words;
  std::vector<double> vals;
  std::vector<float> score(nkf > 0 ? nkf : 1, 0.0f);
  for (int k = 0; k < nkf; k++) {
    KeyFrame* pKF = mvKeyFrames[k];
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
  }
  std::vector<uint32_t> qw;
  std::vector<double> qv;
  for (const auto& wv : F->mBowVec) {
    qw.push_back(wv.first);
    qv.push_back(wv.second);
  }
  std::vector<int32_t> cand(ORBKF_MAX_KEYFRAMES, -1), common(nkf > 0 ? nkf : 1, 0);
  int32_t ncand = 0;
  const orbkf_problem P{nkf, off.data(), words.data(), vals.data(), covis.data(), score.data(),
                        (int32_t)qw.size(), qw.data(), qv.data(), cand.data(), &ncand,
                        common.data()};
  int info[6] = {0, 0, 0, 0, 0, 0};
  if (mpVoc->handle() && orbv_info(mpVoc->handle(), info) != ORBPL_OK)
    throw std::runtime_error(orbpl_last_error());
  if (orbkf_detect_reloc(&P, 1, info[2]) != ORBPL_OK) throw std::runtime_error(orbpl_last_error());
  for (int k = 0; k < nkf; k++) {
    KeyFrame* pKF = mvKeyFrames[k];
    if (common[k] > 0) {
      pKF->mnRelocQuery = F->mnId;
      pKF->mnRelocWords = common[k];
    }
    pKF->mRelocScore = score[k];
  }
  std::vector<KeyFrame*> vpRelocCandidates;
  vpRelocCandidates.reserve(ncand);
  for (int i = 0; i < ncand; i++) vpRelocCandidates.push_back(mvKeyFrames[cand[i]]);
  return vpRelocCandidates;
}

}  // namespace ORB_SLAM2
