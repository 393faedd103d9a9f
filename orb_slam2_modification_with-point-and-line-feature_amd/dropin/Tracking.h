// Minimal drop-in ORB_SLAM2::Tracking (include/Tracking.h): the members
// Tracking::Relocalization (src/Tracking.cc:2049-2269) reads and writes, and
// the function itself as one orbrl_relocalize call: place
// recognition, SearchByBoW, the PnP rounds, PoseOptimization and both
// projection searches for every candidate keyframe run on the MI355X side by
// side. The rest of Tracking (Track(), the motion model, the local map) stays
// the caller's.
//
// The database's keyframes are the non-bad ones in add() order (erase a
// keyframe when it goes bad, P27). Draws (P30): stream c of draw_pitch raw
// rand() values belongs to candidate c; one stream is drawn per database
// keyframe (at most 64) before the call, in order, straight from rand() (not
// through PnPsolver's look-ahead queue), so no second place-recognition pass is
// needed to count the candidates. A relocalisation that runs out of draws
// (P31) returns false with mnRelocStatus = ORBRL_DRAW_EXHAUSTED.
// On success mCurrentFrame has the pose (SetPose), mvpMapPoints from the
// winning keyframe, mvbOutlier where a map point is assigned, and
// mnLastRelocFrameId = mCurrentFrame.mnId. On failure mvpMapPoints is all
// NULL and the pose is left as it was (P32: the reference leaves the last
// candidate's leftovers, which no caller reads). mRelocScore of the keyframes
// is updated as DetectRelocalizationCandidates does; mnRelocQuery /
// mnRelocWords are not (the call does not return them).
#pragma once
#include <cstdint>
#include <vector>

#include "Frame.h"
#include "KeyFrame.h"
#include "KeyFrameDatabase.h"
#include "ORBVocabulary.h"

struct orbrl_handle;

namespace ORB_SLAM2 {

class Tracking {
 public:
  Tracking(ORBVocabulary* pVoc, KeyFrameDatabase* pKFDB, int drawPitch = 1280);
  ~Tracking();
  Tracking(const Tracking&) = delete;
  Tracking& operator=(const Tracking&) = delete;

  bool Relocalization();

  Frame mCurrentFrame;
  KeyFrameDatabase* mpKeyFrameDB;
  ORBVocabulary* mpORBVocabulary;
  unsigned int mnLastRelocFrameId = 0;

  // what the last Relocalization() did (extension)
  int mnRelocStatus = 0, mnRelocRounds = 0, mnRelocGood = 0;
  KeyFrame* mpRelocKF = nullptr;                 // the winning keyframe
  std::vector<KeyFrame*> mvpRelocCandidates;     // vpCandidateKFs
  std::vector<int32_t> mvRelocRecords;           // ORBRL_REC_INTS per candidate

 private:
  int mnDrawPitch;
  orbrl_handle* mpHandle = nullptr;
  int mnHandlePitch = 0;
};

}  // namespace ORB_SLAM2
