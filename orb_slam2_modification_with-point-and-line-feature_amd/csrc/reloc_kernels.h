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
};
void launch_pnp_iterate(const PnpArgs& a, int nsolvers, hipStream_t s);

}  // namespace orbpl
