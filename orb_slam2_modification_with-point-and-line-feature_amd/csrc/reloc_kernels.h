// Device launchers of the pieces of Tracking::Relocalization
// (Tracking.cc:2049-2269) that are not shared with the tracking step
// (launch_pnp_iterate, the PnP solver, is declared at the end):
//   launch_kfdb_reloc : KeyFrameDatabase::DetectRelocalizationCandidates
//                       (KeyFrameDatabase.cc:274-412), kfdb.hip
//   launch_match_kf   : ORBmatcher::SearchByProjection(Frame&, KeyFrame*,
//                       const set<MapPoint*>&, th, ORBdist)
//                       (ORBmatcher.cc:1891-2024), match_local.hip
// Both take pitched device arrays, one problem per workgroup, so a batched
// tracker can call them per lost stream without a host round trip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "track_common.h"

namespace orbpl {

constexpr int kKfdbMaxKf = 64;       // keyframes per database (ORBPL_MAP_KF's maximum)
constexpr int kKfdbMaxWords = 4096;  // BowVector entries per vector (orbv_transform's cap)
constexpr int kKfdbCovis = 10;       // GetBestCovisibilityKeyFrames(10)

// Problem p = blockIdx.x. Per-keyframe arrays have kKfdbMaxKf entries per
// problem (kf_off kKfdbMaxKf + 1, covis kKfdbMaxKf x 10).
struct KfdbArgs {
  const int* nkf;              // [nq] keyframes in the database, <= kKfdbMaxKf
  const int* kf_off;           // CSR offsets into the problem's entry arrays (off[0] = 0)
  const uint32_t* kf_words;    // entries of problem p at p * ent_pitch: ascending per keyframe
  const double* kf_vals;
  long long ent_pitch;
  const int* covis;            // database indices of the 10 best covisibles, -1 = none
  float* reloc_score;          // mRelocScore, in/out
  const int* q_n;              // [nq] query BowVector entries, <= kKfdbMaxWords
  const uint32_t* q_words;     // query of problem p at p * q_pitch, ascending
  const double* q_vals;
  long long q_pitch;
  int* cand;                   // kKfdbMaxKf per problem, the reference's return order
  int* ncand;                  // [nq]
  int* common_words;           // mnRelocWords per keyframe (0: shares no word); may be NULL
};
void launch_kfdb_reloc(const KfdbArgs& a, int nq, hipStream_t s);

// Problem b = blockIdx.x; current-frame arrays at b * kp_pitch, keyframe arrays
// at b * kf_pitch, poses at b * pose_stride floats.
struct MatchKfArgs {
  const KeyPointD* cur_kps_un;   // CurrentFrame.mvKeysUn
  const uint8_t* cur_desc;       // CurrentFrame.mDescriptors, 32 B rows
  const uint8_t* cur_has_mp;     // CurrentFrame.mvpMapPoints[i] != NULL on entry
  const int* cur_n;
  int kp_pitch;
  const float* kf_angle;         // pKF->mvKeysUn[j].angle
  const uint8_t* kf_valid;       // map point exists and is not bad
  const uint8_t* kf_found;       // map point is in sAlreadyFound
  const float* mp_xyz;
  const float* mp_min_dist;      // raw mfMinDistance / mfMaxDistance
  const float* mp_max_dist;
  const uint8_t* mp_desc;
  const int* kf_n;
  int kf_pitch;
  const float* Tcw;
  int pose_stride;
  int* match;                    // per current keypoint: keyframe feature index or -1
  int* nmatches;                 // [batch * nm_stride]
  int nm_stride;
  float th;
  int orb_dist;
  int check_ori;
  float log_scale;               // Frame::mfLogScaleFactor (P15)
};
void launch_match_kf(const TrackConsts& c, const MatchKfArgs& a, int batch, hipStream_t s);

//   launch_pnp_iterate : PnPsolver::iterate (PnPsolver.cc:165-258), pnp.hip
constexpr int kPnpMaxPoints = 2048;  // correspondences per solver (ORBPNP_MAX_POINTS)
constexpr int kPnpMaxIts = 320;      // hypotheses per call (ORBPNP_MAX_ITERATIONS)

// Solver s = blockIdx.x; its correspondences at s * pt_pitch, its draws at
// s * draw_pitch. n is clamped to kPnpMaxPoints, the hypotheses of the call to
// min(kPnpMaxIts, draw_pitch / 4).
struct PnpArgs {
  const int* n;                // [ns] correspondences
  const float* cam;            // [ns][4] fx fy cx cy
  const float* p2d;            // [pt_pitch][2] per solver
  const float* p3d;            // [pt_pitch][3]
  const float* max_error;      // mvMaxError
  int pt_pitch;
  const int* min_inliers;      // mRansacMinInliers, adjusted
  const int* max_its;          // mRansacMaxIts, adjusted
  const int* draws;            // raw rand() values, 4 per hypothesis (P29)
  int draw_pitch;
  double rand_max_p1;          // (double)RAND_MAX + 1.0
  int n_iterations;            // iterate()'s argument
  int* iterations;             // mnIterations, in/out
  int* best_count;             // mnBestInliers, in/out
  uint8_t* best_mask;          // mvbBestInliers, in/out, pt_pitch per solver
  float* best_Tcw;             // mBestTcw, in/out, 16 per solver
  float* Tcw;                  // 16 per solver; zero when result == 0
  int* result;                 // 0 empty, 1 refined, 2 best at exhaustion
  int* no_more;
  int* n_inliers;
  uint8_t* inliers;            // pt_pitch per solver
  int* draws_consumed;
  const int* draw_off = nullptr;  // optional: solver s reads its draws from draws[s] + draw_off[s]
                                  // (and runs at most (draw_pitch - draw_off[s]) / 4 hypotheses)
};
void launch_pnp_iterate(const PnpArgs& a, int nsolvers, hipStream_t s);

//   launch_reloc_* : Tracking::Relocalization itself (Tracking.cc:2049-2269,
//                    DESIGN.md P30-P32), reloc.hip. The unit of work is a pair
//                    q = p * C + c: problem (lost frame) p, candidate slot c < C,
//                    C = the largest candidate count of the batch.
constexpr int kRelocRec = 13;   // ints per candidate record (ORBRL_REC_*)
enum { kRecBow, kRecDisc, kRecCalls, kRecIts, kRecDraws, kRecResult, kRecNoMore, kRecInl,
       kRecG1, kRecAdd1, kRecG2, kRecAdd2, kRecG3 };
constexpr int kRelocTableN = 2048;   // SetRansacParameters table: N = 0 .. 2048

struct RelocDev {
  int np, C, kp_pitch, draw_pitch, stream_pitch;
  // ---- inputs: the lost frames, problem p at p * kp_pitch ----
  const int* n;
  const KeyPointD* kps_un;
  const float* uright;
  const uint8_t* desc;
  const int* feat_node;
  // the databases' keyframes: keyframe k of problem p is slot kf_first[p] + k,
  // its feature arrays at slot * kp_pitch
  const int* kf_first;
  const int* kf_n;
  const float* kf_angle;
  const int* kf_feat_node;
  const uint8_t* kf_desc;
  const uint8_t* kf_valid;
  const float* mp_xyz;
  const float* mp_min_dist;
  const float* mp_max_dist;
  const uint8_t* mp_desc;
  // P30: stream c of problem p at (p * stream_pitch + c) * draw_pitch
  const int* draws;
  const int* n_streams;
  // place recognition's result (k_kfdb_reloc)
  const int* cand;     // kKfdbMaxKf per problem
  const int* ncand;
  // constants
  const int* table;    // [kRelocTableN + 1][2]: min_inliers, max_its
  float sigma2[kMaxLevelsT];
  float cam[4];
  // ---- per pair, arrays at q * kp_pitch ----
  int* bow_match;
  int* bow_nm;
  float* p2d;
  float* p3d;
  float* max_error;
  int* kp_index;
  int* n_corr;
  int* n_run;          // n_corr where the pair runs this round, else 0
  int* min_inl;
  int* max_its;
  float* pcam;
  int* pdraws;         // q * draw_pitch
  int* avail;          // draws of the pair's stream (0: the problem has no stream c)
  int* cursor;
  int* iterations;
  int* best_count;
  uint8_t* best_mask;
  float* best_Tcw;
  float* pnp_Tcw;
  int* result;
  int* no_more;
  int* n_inliers;
  uint8_t* inliers;
  int* consumed;
  // the candidate's copy of the frame and of its keyframe (k_pose, k_match_kf)
  int* pn;
  KeyPointD* pkps;
  float* puright;
  uint8_t* pdesc;
  int* pkf_n;
  float* pkf_angle;
  uint8_t* pkf_valid;
  float* pmp_xyz;
  float* pmp_min;
  float* pmp_max;
  uint8_t* pmp_desc;
  // the candidate's view of mCurrentFrame
  int* match;          // mvpMapPoints as keyframe feature indices
  uint8_t* has_mp;
  uint8_t* outlier;
  uint8_t* kf_found;   // sFound
  float* Tcw;
  int* ninl;           // k_pose's count
  int* add_match;      // k_match_kf's output
  int* add_n;
  int* mk_cur_n;       // counts k_match_kf sees: 0 unless the pair searches
  int* mk_kf_n;
  // director state
  uint8_t* run;
  uint8_t* live;       // committed !vbDiscarded
  uint8_t* live_w;
  uint8_t* win;
  int* stage;
  int* want;           // the pair is in the next launch_pose
  int* ngood;
  int* rec_w;          // kRelocRec per pair
  int* list;
  int* list_n;
  int* exh_at;         // per problem: first candidate out of draws (64: none)
  int* done;
  int* undecided;
  int* maxc;
  // ---- outputs per problem ----
  int* ok;
  int* status;
  int* winner;
  int* rounds;
  int* n_good;
  int* n_live;
  float* out_Tcw;
  int* out_match;      // kp_pitch per problem
  uint8_t* out_outlier;
  int* rec;            // kKfdbMaxKf x kRelocRec per problem
};
void launch_reloc_bow(const RelocDev& d, hipStream_t s);       // match_local.hip
void launch_reloc_init(const RelocDev& d, hipStream_t s);      // outputs cleared, maxc
void launch_reloc_setup(const RelocDev& d, hipStream_t s);
void launch_reloc_begin(const RelocDev& d, hipStream_t s);
void launch_reloc_after_pnp(const RelocDev& d, hipStream_t s);
void launch_reloc_stage(const RelocDev& d, int phase, hipStream_t s);   // then the pose list
void launch_reloc_select(const RelocDev& d, hipStream_t s);

}  // namespace orbpl
