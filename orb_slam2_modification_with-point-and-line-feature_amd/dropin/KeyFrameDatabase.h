// Drop-in ORB_SLAM2::KeyFrameDatabase (include/KeyFrameDatabase.h,
// src/KeyFrameDatabase.cc) reduced to relocalisation: add / erase / clear and
// DetectRelocalizationCandidates(Frame*) (KeyFrameDatabase.cc:274-412) over
// orbkf_detect_reloc. The database is the list of its keyframes in add()
// order, which is the order of every inverted-file list of the reference; the
// query runs on the MI355X. DetectLoopCandidates belongs to LoopClosing and is
// not part of the drop-in. At most 64 keyframes (the tracker's keyframe table).
#pragma once
#include <mutex>
#include <vector>

#include "Frame.h"
#include "KeyFrame.h"
#include "ORBVocabulary.h"

namespace ORB_SLAM2 {

class KeyFrameDatabase {
 public:
  KeyFrameDatabase(const ORBVocabulary& voc);

  void add(KeyFrame* pKF);
  void erase(KeyFrame* pKF);
  void clear();

  // Relocalization: sets mnRelocQuery / mnRelocWords of every keyframe that
  // shares a word with F and mRelocScore of every scored one, as the reference
  // does; mRelocScore starts at 0.0f and persists
  std::vector<KeyFrame*> DetectRelocalizationCandidates(Frame* F);
  // the keyframes in add() order (Tracking::Relocalization packs them)
  std::vector<KeyFrame*> GetKeyFrames() {
    std::unique_lock<std::mutex> lock(mMutex);
    return mvKeyFrames;
  }

 protected:
  const ORBVocabulary* mpVoc;
  std::vector<KeyFrame*> mvKeyFrames;   // add() order
  std::mutex mMutex;
};

}  // namespace ORB_SLAM2
