/*
 * orbpl.h — C-ABI of the MI355X-native ORB-SLAM2 point+line front-end.
 *
 * Every entry point is plain C: pointers + sizes, int status return
 * (0 = ok, < 0 = error, see ORBPL_ERR_*), caller-owned output buffers.
 * No torch / OpenCV / Eigen types cross this boundary. Each function names
 * the reference interface it replaces (file:line in
 * wolfcanli/ORB_SLAM2_Modification_with-point-and-line-feature).
 *
 * Threading: a handle (orbx_ctx / orbpl_tracker) owns one HIP stream on one
 * device and must be used by one host thread at a time — the same contract as
 * one ORB_SLAM2::ORBextractor instance per thread (Frame.cc:152-155).
 */
#ifndef ORBPL_H
#define ORBPL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORBPL_OK 0
#define ORBPL_ERR_ARG (-1)       /* bad argument / unsupported geometry      */
#define ORBPL_ERR_CAPACITY (-2)  /* caller buffer or internal cap too small  */
#define ORBPL_ERR_HIP (-3)       /* HIP runtime error (message: orbpl_last_error) */
#define ORBPL_ERR_NODEVICE (-4)  /* no HIP device visible                    */
#define ORBPL_ERR_OVERFLOW (-5)  /* kernel-side capacity overflow flag set   */

/* Mirror of cv::KeyPoint (28 bytes): pt.x, pt.y, size, angle, response,
 * octave, class_id. */
typedef struct orbpl_keypoint {
  float x, y, size, angle, response;
  int32_t octave, class_id;
} orbpl_keypoint;

/* Mirror of cv::line_descriptor::KeyLine (opencv_contrib 3.4, 68 bytes),
 * the element type of Frame::mvKeyLines (Frame.h, LineExtractor.h:27). */
typedef struct orbpl_keyline {
  float angle;
  int32_t class_id;
  int32_t octave;
  float pt_x, pt_y;
  float response;
  float size;
  float startPointX, startPointY, endPointX, endPointY;
  float sPointInOctaveX, sPointInOctaveY, ePointInOctaveX, ePointInOctaveY;
  float lineLength;
  int32_t numOfPixels;
} orbpl_keyline;

/* ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST,
 * int minThFAST) — ORBextractor.h:52-53, values from the settings YAML
 * (Tracking.cc:113-125; Examples/RGB-D/TUM1.yaml: 1000, 1.2, 8, 20, 7). */
typedef struct orbpl_orb_params {
  int32_t nfeatures;
  float scale_factor;
  int32_t nlevels;
  int32_t ini_th_fast;
  int32_t min_th_fast;
} orbpl_orb_params;

/* Last error message of the calling thread (static storage). */
const char* orbpl_last_error(void);
/* Number of visible HIP devices. */
int orbpl_device_count(int* n);
/* Hardware queues as recorded when the library was loaded (no HIP call):
 * queues = GPU_MAX_HW_QUEUES the HIP runtime runs with; runtime_started = 1
 * when the runtime was already up (another HIP user came first, so the
 * library changed nothing); set_by_library = 1 when the library filled in
 * the variable (it was unset, or ORBPL_HW_QUEUES asked). lsd_split_1024 = 1
 * when a 1024-stream lines tracker would split its LSD batch (needs >= 8
 * queues; ORBPL_LSD_SPLIT=0/1 overrides). Any pointer may be NULL. */
int orbpl_hw_queue_state(int* queues, int* runtime_started, int* set_by_library,
                         int* lsd_split_1024);
/* Library build tag ("orbpl gfx950 r4").
 * r4: orbpl_frame_is_in_frustum takes the RAW mfMinDistance / mfMaxDistance
 *     (MapPoint::GetMinDistance / GetMaxDistance) and applies the 0.8f / 1.2f
 *     of GetMin/MaxDistanceInvariance itself; r3 callers that pass the
 *     pre-scaled invariance values must switch to the raw ones.
 * r3: orbpl_tracker_timings writes 11 floats per step,
 *     orbpl_tracker_stereo_timings 4 (r1: 9 and 2); size the buffers from
 *     orbpl_tracker_timing_counts. */
const char* orbpl_version(void);

/* Device memory plumbing for hosts without their own GPU allocator (the
 * reference's C++ Tracking, ctypes tests, bench). Synchronous copies. */
int orbpl_dev_malloc(int device, int64_t bytes, void** out);
int orbpl_dev_free(int device, void* ptr);
/* page-locked host memory (hipHostMalloc): the source of asynchronous
 * host-to-device frame copies (orbpl_tracker_step_host) */
int orbpl_host_alloc(int64_t bytes, void** out);
int orbpl_host_free(void* ptr);
int orbpl_memcpy_htod(int device, void* dst, const void* src, int64_t bytes);
int orbpl_memcpy_dtoh(int device, void* dst, const void* src, int64_t bytes);
int orbpl_memset_d(int device, void* dst, int value, int64_t bytes);
int orbpl_device_synchronize(int device);

/* ------------------------------------------------------------------------
 * ORB extraction  — replaces ORB_SLAM2::ORBextractor (include/ORBextractor.h,
 * src/ORBextractor.cc:410-1132).
 * ---------------------------------------------------------------------- */
typedef struct orbx_ctx orbx_ctx;

/* ORBextractor::ORBextractor (ORBextractor.cc:410). width/height fix the
 * image geometry; max_batch frames can be extracted per launch. */
int orbx_create(const orbpl_orb_params* params, int width, int height, int max_batch,
                int device, orbx_ctx** out);
int orbx_destroy(orbx_ctx* ctx);

/* GetLevels / GetScaleFactors / GetInverseScaleFactors / GetScaleSigmaSquares
 * / GetInverseScaleSigmaSquares (ORBextractor.h:60-78). Arrays have nlevels
 * entries; any pointer may be NULL. */
int orbx_get_scale_info(const orbx_ctx* ctx, int* nlevels, float* scale, float* inv_scale,
                        float* sigma2, float* inv_sigma2);
/* Per-level content size and keypoint budget (mnFeaturesPerLevel). */
int orbx_get_level_info(const orbx_ctx* ctx, int* w, int* h, int* nfeatures_per_level);
/* Maximum keypoints one frame can produce (size for kps/desc buffers). */
int orbx_max_keypoints(const orbx_ctx* ctx);
/* Device-free geometry query (no HIP call): per-level sizes and budgets that
 * orbx_create would use, and the per-frame keypoint capacity. Arrays have
 * params->nlevels entries; any pointer may be NULL. */
int orbx_describe(const orbpl_orb_params* params, int width, int height, int* lw, int* lh,
                  int* nfeatures_per_level, float* scale, int* max_keypoints);

/* ORBextractor::operator()(image, mask, keypoints, descriptors)
 * (ORBextractor.cc:1043-1105). Host buffers in and out; synchronous.
 * kps[cap], desc[cap*32] (row i = descriptor of kps[i]); *n = keypoint count.
 * Empty image (NULL or 0 size) returns ORBPL_OK with *n = 0. */
int orbx_extract(orbx_ctx* ctx, const uint8_t* img, int width, int height, int stride,
                 orbpl_keypoint* kps, uint8_t* desc, int cap, int* n);

/* Batched, device-resident form (throughput path). d_imgs: batch frames of
 * width x height u8 in device memory, frame f at d_imgs + f*frame_pitch with
 * row stride `stride`. Outputs are device buffers: d_kps[batch*kp_pitch],
 * d_desc[batch*kp_pitch*32], d_n[batch]. Asynchronous on the ctx stream. */
int orbx_extract_batch_device(orbx_ctx* ctx, const uint8_t* d_imgs, int batch, int stride,
                              int64_t frame_pitch, orbpl_keypoint* d_kps, uint8_t* d_desc,
                              int kp_pitch, int32_t* d_n);

/* The public mvImagePyramid (ORBextractor.h:83; read by Frame.cc:895-1002):
 * copy level `level` of frame `frame` of the last extraction to host. With
 * padded != 0 the (w+38)x(h+38) bordered buffer is returned, else the w x h
 * content; blurred != 0 returns the GaussianBlur(7x7, 2) working image. */
int orbx_get_pyramid(orbx_ctx* ctx, int frame, int level, int padded, int blurred, uint8_t* out,
                     int out_cap, int* w, int* h);

/* Debug/parity: pre-octree FAST candidates (vToDistributeKeys,
 * ORBextractor.cc:820-825) of frame 0 of the last extraction, concatenated by
 * level as (x, y, response) float triples relative to minBorder. */
int orbx_get_candidates(orbx_ctx* ctx, float* xyr, int cap, int* level_counts, int* total);

/* Wait for the ctx stream; returns ORBPL_ERR_OVERFLOW if a kernel reported a
 * capacity overflow since the last call. */
int orbx_synchronize(orbx_ctx* ctx);
/* Device-side timing of the last orbx_extract*: per-stage milliseconds
 * (pyramid, blur, fast, octree, desc) measured with hipEvents on the ctx
 * stream. */
int orbx_last_stage_ms(const orbx_ctx* ctx, float* ms5);
/* Debug: k_pyramid phase times (ns) of block (band 0, frame 0) in the last
 * launch, 4 per level (content, side borders, mirror rows, blur); needs
 * ORBPL_PYR_PROFILE in the environment when the context is created. */
int orbx_debug_pyr_profile(orbx_ctx* ctx, long long* out, int cap, int* n);
/* Debug: k_octree per-level block of frame 0 in the last launch (ORBPL_OCT_PROFILE
 * set before the first launch): 8 values per level (setup ns, pass loop ns, 0,
 * retain ns, passes, candidates, final list size, 0), 16 levels. */
int orbx_debug_octree_profile(orbx_ctx* ctx, long long* out128);


/* ------------------------------------------------------------------------
 * Camera / Frame glue — Frame constructors (Frame.cc:135-205): undistortion
 * (UndistortKeyPoints :737-764, cv::undistortPoints 5 iterations), image
 * bounds (ComputeImageBounds :847-885), RGB-D depth association
 * (ComputeStereoFromRGBD :1065-1117) and the 64x48 grid (PosInGrid :527-538).
 * ---------------------------------------------------------------------- */
typedef struct orbpl_camera {
  float fx, fy, cx, cy;        /* Camera.fx/fy/cx/cy                          */
  float k1, k2, p1, p2, k3;    /* Camera.k1..k3 (OpenCV order)                */
  float bf;                    /* mbf = Camera.bf                             */
  float th_depth;              /* mThDepth = bf * ThDepth / fx (Tracking.cc:134-138) */
  int32_t width, height;
} orbpl_camera;

/* Tracking::Tracking's settings (Tracking.cc:53-147) read from the
 * reference's OpenCV FileStorage YAML files (Examples/RGB-D/TUM1.yaml:8-55):
 * the flat "Key.name: value" subset, with OpenCV 3.4's FileNode conversions
 * (a missing key reads 0). sensor: System::eSensor. cam.th_depth = mbf *
 * ThDepth / fx for stereo / RGB-D (0 monocular); fps 0 -> 30 and max_frames
 * = mMaxFrames (orbpl_tracker_set_fps takes fps); depth_map_factor =
 * mDepthMapFactor = 1 / DepthMapFactor (1 when |DepthMapFactor| < 1e-5 or
 * not RGB-D); cam.width / height from Camera.width / height when present
 * (the reference takes them from the images). */
#define ORBPL_SENSOR_MONOCULAR 0
#define ORBPL_SENSOR_STEREO 1
#define ORBPL_SENSOR_RGBD 2
typedef struct orbpl_settings {
  orbpl_orb_params orb;
  orbpl_camera cam;
  float fps;
  int32_t max_frames;
  float depth_map_factor;      /* mDepthMapFactor (1 / DepthMapFactor)       */
  float depth_map_factor_setting;  /* DepthMapFactor as read (orbpl_tracker_step_host) */
  int32_t rgb;                 /* Camera.RGB */
} orbpl_settings;
int orbpl_settings_load(const char* path, int sensor, orbpl_settings* out);

#define ORBPL_GRID_COLS 64     /* FRAME_GRID_COLS (Frame.h:41) */
#define ORBPL_GRID_ROWS 48     /* FRAME_GRID_ROWS (Frame.h:40) */

/* Per-frame glue on the GPU. Inputs: raw keypoints kps[n] from orbx_extract,
 * optional depth image (float metres, width x height, row stride = width;
 * NULL for monocular: depth/uright = -1). Outputs (caller-owned, n entries):
 * kps_un (mvKeysUn), depth (mvDepth), uright (mvuRight), grid_cell
 * (gx + 64*gy, -1 if PosInGrid fails). bounds[4] = mnMinX, mnMaxX, mnMinY,
 * mnMaxY. */
int orbpl_frame_prepare(const orbpl_camera* cam, const orbpl_keypoint* kps, int n,
                        const float* depth, orbpl_keypoint* kps_un, float* depth_out,
                        float* uright_out, int32_t* grid_cell, float* bounds);

/* ------------------------------------------------------------------------
 * ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame,
 * float th, bool bMono)  (ORBmatcher.cc:1710-1879), with ORBmatcher(0.9, true)
 * as Tracking::TrackWithMotionModel builds it (Tracking.cc:1216).
 * ---------------------------------------------------------------------- */
typedef struct orbpl_match_current {
  int32_t n;
  const float* Tcw;            /* 4x4 row-major (mTcw, predicted pose)        */
  const orbpl_keypoint* kps_un;/* mvKeysUn                                    */
  const uint8_t* desc;         /* mDescriptors, n x 32                        */
  const float* uright;         /* mvuRight                                    */
} orbpl_match_current;

typedef struct orbpl_match_last {
  int32_t n;
  const float* Tcw;            /* LastFrame.mTcw                              */
  const orbpl_keypoint* kps_un;/* LastFrame.mvKeysUn (angle, octave used)     */
  const uint8_t* has_mp;       /* LastFrame.mvpMapPoints[i] != NULL           */
  const uint8_t* outlier;      /* LastFrame.mvbOutlier                        */
  const float* mp_xyz;         /* pMP->GetWorldPos(), n x 3                   */
  const uint8_t* mp_desc;      /* pMP->GetDescriptor(), n x 32                */
  const int32_t* mp_nobs;      /* pMP->Observations()                         */
} orbpl_match_last;

/* match[i] = index j of the last-frame map point assigned to current keypoint
 * i (CurrentFrame.mvpMapPoints[i] = LastFrame.mvpMapPoints[j]) or -1.
 * *nmatches = the function's return value. Refused: more than 2048 keypoints
 * in either frame, NULL arrays of a frame that has keypoints, a keypoint octave
 * of either frame outside [0, nlevels) ("keypoint octave outside the pyramid"). */
int orbm_search_by_projection_last(const orbpl_camera* cam, const float* scale_factors,
                                   int nlevels, const orbpl_match_current* cur,
                                   const orbpl_match_last* last, float th, int mono,
                                   int check_orientation, int32_t* match, int* nmatches);

/* Frame::ComputeStereoMatches (Frame.cc:886-1063) for a stereo pair whose
 * left / right images were extracted by `left` / `right` (batch frame
 * `frame`; their pyramids are the reference's mvImagePyramid): uRight and
 * depth per left keypoint (-1: none). kl / kr = mvKeys / mvKeysRight as
 * returned by orbx_extract, octaves inside the extractors' 1 to 16 levels.
 * n, nr <= 4096, image height <= 1024; the two extractors share size and
 * level count. */
int orbpl_stereo_matches(const orbpl_camera* cam, orbx_ctx* left, orbx_ctx* right, int frame,
                         const orbpl_keypoint* kl, const uint8_t* dl, int n,
                         const orbpl_keypoint* kr, const uint8_t* dr, int nr, float* uright,
                         float* depth);

/* ------------------------------------------------------------------------
 * Tracking::SearchLocalPoints pieces (TrackLocalMap)
 * ---------------------------------------------------------------------- */
/* Frame::IsInFrustum(MapPoint*, view_cos_limit) (Frame.cc:345-401) for n map
 * points (world xyz, normal, and the raw mfMinDistance / mfMaxDistance: the
 * range test applies GetMin/MaxDistanceInvariance's 0.8f / 1.2f, MapPoint.cc:
 * 387-397, and PredictScale's ratio is mfMaxDistance / dist, MapPoint.cc:
 * 416-431); outputs the mTrack* fields:
 * in_view (mbTrackInView), proj_x/y, proj_xr (u - bf/z), level
 * (mnTrackScaleLevel, -1 when not in view), view_cos (mTrackViewCos).
 * scale_factor = ORBextractor scale factor (mfLogScaleFactor = logf of it). */
int orbpl_frame_is_in_frustum(const orbpl_camera* cam, float scale_factor, int nlevels,
                              const float* Tcw, int n, const float* xyz, const float* normal,
                              const float* min_dist, const float* max_dist, float view_cos_limit,
                              uint8_t* in_view, float* proj_x, float* proj_y, float* proj_xr,
                              int32_t* level, float* view_cos);
/* ORBmatcher(nnratio).SearchByProjection(F, vpLocalMapPoints, th)
 * (ORBmatcher.cc:72-183): radius RadiusByViewingCos(view_cos) (x th when
 * th != 1) x scale[level], levels [level-1, level], best and second by
 * Hamming, TH_HIGH 100, ratio test only when both are on the same level.
 * cur_nobs[i] = Observations() of the map point already at keypoint i (0 or
 * NULL: none); keypoints holding one with Observations() > 0 are skipped, as
 * are keypoints claimed during the call. match[i] = index of the last local
 * map point assigned to keypoint i in this call (the reference overwrites
 * F.mvpMapPoints[i]), -1 = unchanged. *nmatches = return value. Refused: a
 * level of an in-view point or a keypoint octave outside [0, nlevels). */
int orbm_search_by_projection_local(const orbpl_camera* cam, const float* scale_factors,
                                    int nlevels, const orbpl_match_current* cur, int nmp,
                                    const uint8_t* in_view, const float* proj_x,
                                    const float* proj_y, const float* proj_xr,
                                    const int32_t* level, const float* view_cos,
                                    const uint8_t* mp_desc, const int32_t* mp_nobs,
                                    const int32_t* cur_nobs, float th, float nnratio,
                                    int32_t* match, int* nmatches);

/* ---- DBoW2 ORB vocabulary (ORBVocabulary = TemplatedVocabulary<FORB::
 * TDescriptor, FORB>, Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h) ---- */
typedef struct orbv_vocab orbv_vocab;
/* TemplatedVocabulary::loadFromTextFile (TemplatedVocabulary.h:1338-1420),
 * System.cc:65: "k L scoring weighting" then one node per line (parent,
 * isLeaf, 32 descriptor bytes, weight). A line without tokens (the one after a
 * final '\n') makes no node (pinned P19). Host-only; word ids follow the
 * isLeaf lines in node order. */
int orbv_load_text(const char* path, orbv_vocab** out);
/* The same vocabulary from flat node arrays (node 0 = root, parent[i] < i):
 * a rank's copy of the vocabulary rank 0 loaded and broadcast. */
int orbv_create(int k, int L, int scoring, int weighting, int n_nodes, const int32_t* parent,
                const uint8_t* leaf_flag, const uint8_t* desc, const double* weight,
                orbv_vocab** out);
int orbv_destroy(orbv_vocab* v);
/* out6 = k, L, scoring, weighting, n_nodes, n_words */
int orbv_info(const orbv_vocab* v, int* out6);
/* the flat node arrays orbv_create takes (n_nodes entries; desc 32 B rows) */
int orbv_export(const orbv_vocab* v, int32_t* parent, uint8_t* leaf_flag, uint8_t* desc,
                double* weight);
/* copy the tree to `device` (CSR children, descriptors, words, weights) */
int orbv_upload(orbv_vocab* v, int device);
/* TemplatedVocabulary::transform(features, BowVector, FeatureVector, levelsup)
 * (TemplatedVocabulary.h:1127-1205, 1226-1262) as Frame::ComputeBoW calls it
 * (Frame.cc:730, levelsup 4): the BowVector as bow_n (word, value) pairs in
 * word order, the FeatureVector as the node (at level L - levelsup) of every
 * feature, -1 for a stopped word (weight 0). n <= 4096; bow buffers >= n. */
int orbv_transform(orbv_vocab* v, int device, const uint8_t* desc, int n, int levelsup,
                   uint32_t* bow_words, double* bow_vals, int* bow_n, int32_t* feat_node);
/* The same for nframes device-resident frames: frame f's descriptors at
 * d_desc + f * desc_pitch * 32 (d_n[f] of them, <= max_n <= 4096); outputs
 * per frame at f * out_pitch (feature word / weight / node, BowVector), the
 * BowVector length in d_bow_n[f]; a frame with d_n[f] > max_n is cut to its
 * first max_n features and sets *d_err |= 2. At most 2^20 - 1 words.
 * `stream` = a hipStream_t (NULL: the vocabulary's own stream). */
int orbv_transform_batch_device(orbv_vocab* v, const uint8_t* d_desc, int64_t desc_pitch,
                                const int* d_n, int nframes, int max_n, int levelsup,
                                int32_t* d_feat_node, int32_t* d_feat_word, double* d_feat_weight,
                                uint32_t* d_bow_words, double* d_bow_vals, int* d_bow_n,
                                int64_t out_pitch, int* d_err, void* stream);

/* ORBmatcher(nnratio, checkOri).SearchByBoW(pKF, F, vpMapPointMatches)
 * (ORBmatcher.cc:247-410). The DBoW2 FeatureVectors are passed as one
 * vocabulary node id per feature (-1: none; ids < 2^21 - 1): features meet
 * only within a node, keyframe features in index order, a frame feature taken
 * earlier in the call is skipped; TH_LOW 50 and best < nnratio * second; then
 * the 30-bin rotation check (kf_angle = mvKeysUn, f_angle = mvKeys). kf_valid
 * = the keyframe's map point exists and is not bad. match[j] = keyframe
 * feature index whose map point goes to frame feature j, or -1. n <= 2048. */
int orbm_search_by_bow(int nkf, const int32_t* kf_node, const uint8_t* kf_valid,
                       const uint8_t* kf_desc, const float* kf_angle, int nf, const int32_t* f_node,
                       const uint8_t* f_desc, const float* f_angle, float nnratio, int check_ori,
                       int32_t* match, int* nmatches);

/* ------------------------------------------------------------------------
 * Tracking::Relocalization (Tracking.cc:2049-2269): its place recognition and
 * its projection matcher and its PnP solver. With orbv_transform
 * (Frame::ComputeBoW), orbm_search_by_bow and orbpl_pose_optimization these
 * are all the building blocks of the function.
 * ---------------------------------------------------------------------- */
#define ORBKF_MAX_KEYFRAMES 64   /* keyframes per database (ORBPL_MAP_KF's maximum) */
#define ORBKF_MAX_WORDS 4096     /* BowVector entries per vector (orbv_transform's cap) */
#define ORBKF_COVISIBLES 10      /* GetBestCovisibilityKeyFrames(10) */
/* KeyFrameDatabase::DetectRelocalizationCandidates(Frame*)
 * (KeyFrameDatabase.cc:274-412) for one (database, query) pair. The database
 * is its nkf keyframes in add() order (erased or bad keyframes are absent):
 * their BowVectors as CSR (kf_off[nkf + 1], kf_off[0] = 0; words ascending
 * within a keyframe), covis[nkf][10] = GetBestCovisibilityKeyFrames(10) as
 * database indices in that order (-1: padding, or a neighbour that is not in
 * the database), reloc_score[nkf] = mRelocScore: in/out, per-keyframe state
 * that persists across queries and starts at 0.0f (the reference never
 * initialises it) - a keyframe scored in this query is
 * overwritten, every other entry is kept. The query is F->mBowVec (words
 * ascending). Outputs: cand[64] / *ncand = the returned vector as database
 * indices in the reference's order; common_words[nkf] (may be NULL) =
 * mnRelocWords, 0 for a keyframe that shares no word. */
typedef struct orbkf_problem {
  int32_t nkf;
  const int32_t* kf_off;
  const uint32_t* kf_words;
  const double* kf_vals;
  const int32_t* covis;
  float* reloc_score;
  int32_t nq_words;
  const uint32_t* q_words;
  const double* q_vals;
  int32_t* cand;
  int32_t* ncand;
  int32_t* common_words;
} orbkf_problem;
/* nq independent problems in one launch (one lost frame per stream, each with
 * its own map). scoring = the vocabulary's ScoringType (orbv_info): only
 * L1_NORM = 0 (ORBvoc's) is built, anything else returns ORBPL_ERR_ARG, as do
 * more than 64 keyframes or more than 4096 entries in a vector. */
int orbkf_detect_reloc(const orbkf_problem* problems, int nq, int scoring);
/* The same over pitched device arrays, asynchronous on `stream` (a
 * hipStream_t, NULL = the null stream). Per-keyframe arrays hold 64 entries
 * per problem (d_kf_off 65, d_covis 64 x 10); problem p's keyframe entries
 * start at p * ent_pitch, its query at p * q_pitch. Counts above the caps
 * are clamped. d_common_words may be NULL. */
typedef struct orbkf_device_batch {
  const int32_t* d_nkf;
  const int32_t* d_kf_off;
  const uint32_t* d_kf_words;
  const double* d_kf_vals;
  int64_t ent_pitch;
  const int32_t* d_covis;
  float* d_reloc_score;
  const int32_t* d_q_n;
  const uint32_t* d_q_words;
  const double* d_q_vals;
  int64_t q_pitch;
  int32_t* d_cand;
  int32_t* d_ncand;
  int32_t* d_common_words;
} orbkf_device_batch;
int orbkf_detect_reloc_batch_device(const orbkf_device_batch* b, int nq, int scoring,
                                    void* stream);

/* ORBmatcher(nnratio, checkOri).SearchByProjection(Frame& CurrentFrame,
 * KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, th, ORBdist)
 * (ORBmatcher.cc:1891-2024; Tracking.cc:2201, 2215). cur->Tcw = the pose the
 * PnP solver / the optimiser gave (cur->uright is not read). cur_has_mp[i] =
 * CurrentFrame.mvpMapPoints[i] != NULL on entry. Per keyframe feature j <
 * nkf: kf_angle = mvKeysUn[j].angle, kf_valid = its map point exists and is
 * not bad, kf_found = it is in sAlreadyFound, the point's world position,
 * raw mfMinDistance / mfMaxDistance (the 0.8f / 1.2f applied inside, as in
 * orbpl_frame_is_in_frustum) and descriptor. Keyframe features in index
 * order; a keypoint that holds a map point - on entry or claimed earlier in
 * the call - is skipped; the first minimum wins and is accepted on bestDist
 * <= orb_dist; searched levels [level - 1, level + 1], radius th *
 * scale[level]; then the 30-bin rotation check. mfLogScaleFactor is taken
 * from scale_factors[1]. match[i] = keyframe feature assigned to keypoint i
 * in this call, or -1; *nmatches = the return value. n, nkf <= 2048. The
 * reference has no invzc < 0 test here; a projection that is not a number is
 * rejected. */
int orbm_search_by_projection_kf(const orbpl_camera* cam, const float* scale_factors, int nlevels,
                                 const orbpl_match_current* cur, const uint8_t* cur_has_mp,
                                 int nkf, const float* kf_angle, const uint8_t* kf_valid,
                                 const uint8_t* kf_found, const float* mp_xyz,
                                 const float* mp_min_dist, const float* mp_max_dist,
                                 const uint8_t* mp_desc, float th, int orb_dist, int check_ori,
                                 int32_t* match, int* nmatches);
/* The same for `batch` problems over pitched device arrays, asynchronous on
 * `stream`: problem b's current-frame arrays start at b * kp_pitch entries
 * (d_cur_n[b] of them), its keyframe arrays at b * kf_pitch (d_kf_n[b]), its
 * pose at d_Tcw + 16 b; d_match is per current keypoint, d_nmatches[batch].
 * Pitches <= 2048; counts above a pitch are clamped. */
typedef struct orbm_kf_device_batch {
  int32_t kp_pitch;
  const int32_t* d_cur_n;
  const float* d_Tcw;
  const orbpl_keypoint* d_cur_kps_un;
  const uint8_t* d_cur_desc;
  const uint8_t* d_cur_has_mp;
  int32_t kf_pitch;
  const int32_t* d_kf_n;
  const float* d_kf_angle;
  const uint8_t* d_kf_valid;
  const uint8_t* d_kf_found;
  const float* d_mp_xyz;
  const float* d_mp_min_dist;
  const float* d_mp_max_dist;
  const uint8_t* d_mp_desc;
  int32_t* d_match;
  int32_t* d_nmatches;
} orbm_kf_device_batch;
int orbm_search_by_projection_kf_batch_device(const orbpl_camera* cam, const float* scale_factors,
                                              int nlevels, const orbm_kf_device_batch* b,
                                              int batch, float th, int orb_dist, int check_ori,
                                              void* stream);

/* PnPsolver (PnPsolver.cc): EPnP inside RANSAC, one
 * solver per (lost frame, candidate keyframe), any number of solvers in one
 * launch. */
#define ORBPNP_MAX_POINTS 2048      /* correspondences per solver */
#define ORBPNP_MAX_ITERATIONS 320   /* hypotheses one call may run per solver */
#define ORBPNP_MIN_SET 4            /* mRansacMinSet; no other value is built */
/* PnPsolver::SetRansacParameters (:121-157) for n correspondences, on the
 * host, no device needed: the adjusted mRansacMinInliers, mRansacMaxIts and
 * mRansacEpsilon, and, if max_error is not NULL, mvMaxError[i] = sigma2[i] *
 * th2 (n entries each). log / pow are the platform's. A quotient that is not
 * a finite int (n == 0, epsilon^3 below 2^-53) counts as INT_MIN, so max_its
 * is 1. */
int orbpnp_ransac_parameters(int n, double probability, int min_inliers, int max_iterations,
                             int min_set, float epsilon, float th2, const float* sigma2,
                             int32_t* out_min_inliers, int32_t* out_max_its, float* out_epsilon,
                             float* max_error);
/* One solver. Inputs: the camera, the n correspondences (p2d[n][2] =
 * mvP2D, sigma2[n] = mvSigma2 (not read, may be NULL), p3d[n][3] = mvP3Dw),
 * the adjusted RANSAC parameters (min_inliers >= 4, max_its, max_error[n]) and
 * n_draws raw rand() values in [0, RAND_MAX]: hypothesis k of a call uses
 * draws[4k .. 4k+3], a call may run max(max_its - *iterations, n_iterations)
 * hypotheses and n_draws must cover them. State, in/out, zero before the first
 * call: *iterations = mnIterations, *best_inliers = mnBestInliers,
 * best_mask[n] = mvbBestInliers, best_Tcw[16] = mBestTcw. Outputs: Tcw[16]
 * (row-major; all zero when *result == 0), *result (0 = empty cv::Mat, 1 =
 * the refined pose, 2 = mBestTcw at exhaustion), *no_more = bNoMore,
 * *n_inliers, inliers[n] per correspondence, *draws_consumed = 4 x the
 * hypotheses the reference would have run before it returned. */
typedef struct orbpnp_problem {
  float fx, fy, cx, cy;
  int32_t n;
  const float* p2d;
  const float* sigma2;
  const float* p3d;
  int32_t min_inliers;
  int32_t max_its;
  const float* max_error;
  int32_t n_draws;
  const int32_t* draws;
  int32_t* iterations;
  int32_t* best_inliers;
  uint8_t* best_mask;
  float* best_Tcw;
  float* Tcw;
  int32_t* result;
  int32_t* no_more;
  int32_t* n_inliers;
  uint8_t* inliers;
  int32_t* draws_consumed;
} orbpnp_problem;
/* PnPsolver::iterate(n_iterations, ...) for nsolvers independent solvers in
 * one launch. ORBPL_ERR_ARG: n above ORBPNP_MAX_POINTS, min_inliers below 4, a
 * call that may run more than ORBPNP_MAX_ITERATIONS hypotheses, or too few
 * draws. */
int orbpnp_iterate(const orbpnp_problem* problems, int nsolvers, int n_iterations);
/* The same over pitched device arrays, asynchronous on `stream`: solver s's
 * correspondences, masks and max_error start at s * pt_pitch entries, its
 * draws at s * draw_pitch, its camera at d_cam + 4 s (fx fy cx cy), its poses
 * at 16 s. Counts above the caps are clamped, the hypotheses of a call also to
 * draw_pitch / 4. */
typedef struct orbpnp_device_batch {
  const int32_t* d_n;
  const float* d_cam;
  const float* d_p2d;
  const float* d_p3d;
  const float* d_max_error;
  int32_t pt_pitch;
  const int32_t* d_min_inliers;
  const int32_t* d_max_its;
  const int32_t* d_draws;
  int32_t draw_pitch;
  int32_t* d_iterations;
  int32_t* d_best_inliers;
  uint8_t* d_best_mask;
  float* d_best_Tcw;
  float* d_Tcw;
  int32_t* d_result;
  int32_t* d_no_more;
  int32_t* d_n_inliers;
  uint8_t* d_inliers;
  int32_t* d_draws_consumed;
} orbpnp_device_batch;
int orbpnp_iterate_batch_device(const orbpnp_device_batch* b, int nsolvers, int n_iterations,
                                void* stream);

/* Sim3Solver (Sim3Solver.cc): Horn's closed form on three
 * correspondences inside RANSAC, one solver per (current keyframe, loop
 * candidate), any number of solvers in one launch. */
#define ORBSIM3_MAX_POINTS 2048      /* features per keyframe, correspondences per solver */
#define ORBSIM3_MAX_ITERATIONS 320   /* hypotheses one call may run per solver */
/* Sim3Solver::SetRansacParameters (:114-138) for n correspondences, on the
 * host, no device needed: *out_max_its = mRansacMaxIts. log / pow are the
 * platform's. A quotient that is not a finite int counts as INT_MIN, so
 * max_its is 1. */
int orbsim3_ransac_parameters(int n, double probability, int min_inliers, int max_iterations,
                              int32_t* out_max_its);
/* The constructor (:37-112) for one keyframe pair, on the host, no device
 * needed. Inputs per feature i of keyframe 1 (n1 of them): matched12[i] = the
 * index in keyframe 2 of the point matched to it (-1: no match, -2: a match
 * whose point keyframe 2 does not observe), valid1[i] = the feature has a map
 * point and it is not bad, xyz1[i][3] = its world position, octave1[i] =
 * mvKeysUn[i].octave. Per feature j of keyframe 2 (n2): valid2[j] = its point
 * is not bad, xyz2[j][3], octave2[j]. level_sigma2[nlevels] = mvLevelSigma2,
 * Tcw1 / Tcw2 [16] row-major, the camera fx fy cx cy. Outputs, compacted in
 * ascending i, room for n1 entries each: *n, indices1 = mvnIndices1, X3Dc1 /
 * X3Dc2 [.][3], P1im1 / P2im2 [.][2], max_error1 / max_error2 = mvnMaxError1/2
 * (9.210 * sigma2 truncated toward zero, as the reference's vector<size_t>
 * holds it). ORBPL_ERR_ARG: n1 or n2 above ORBSIM3_MAX_POINTS, nlevels outside
 * [1, 16], matched12 outside [-2, n2), an octave outside [0, nlevels). */
typedef struct orbsim3_pair {
  int32_t n1;
  const int32_t* matched12;
  const uint8_t* valid1;
  const float* xyz1;
  const int32_t* octave1;
  int32_t n2;
  const uint8_t* valid2;
  const float* xyz2;
  const int32_t* octave2;
  const float* Tcw1;
  const float* Tcw2;
  float fx, fy, cx, cy;
  int32_t* n;
  int32_t* indices1;
  float* X3Dc1;
  float* X3Dc2;
  float* P1im1;
  float* P2im2;
  int32_t* max_error1;
  int32_t* max_error2;
} orbsim3_pair;
int orbsim3_setup(const orbsim3_pair* pairs, int npairs, const float* level_sigma2, int nlevels);
/* The same in one launch over pitched device arrays, asynchronous on
 * `stream`: pair s's keyframe-1 arrays and its outputs start at s * pitch1
 * entries, its keyframe-2 arrays at s * pitch2, its poses at 16 s, its camera
 * at 4 s. The outputs are the input arrays of orbsim3_device_batch with
 * pt_pitch = pitch1. Counts are clamped to the pitches and the cap, octaves to
 * [0, nlevels), and a matched12 entry outside [0, n2) is no match. */
typedef struct orbsim3_setup_device_batch {
  const int32_t* d_n1;
  const int32_t* d_n2;
  int32_t pitch1;
  int32_t pitch2;
  const int32_t* d_matched12;
  const uint8_t* d_valid1;
  const float* d_xyz1;
  const int32_t* d_octave1;
  const uint8_t* d_valid2;
  const float* d_xyz2;
  const int32_t* d_octave2;
  const float* d_Tcw1;
  const float* d_Tcw2;
  const float* d_cam;
  const float* d_level_sigma2;   /* [nlevels], shared by all pairs */
  int32_t nlevels;
  int32_t* d_n;
  int32_t* d_indices1;
  float* d_X3Dc1;
  float* d_X3Dc2;
  float* d_P1im1;
  float* d_P2im2;
  int32_t* d_max_error1;
  int32_t* d_max_error2;
} orbsim3_setup_device_batch;
int orbsim3_setup_batch_device(const orbsim3_setup_device_batch* b, int npairs, void* stream);
/* One solver. Inputs: the camera, the n compacted correspondences of
 * orbsim3_setup, min_inliers (>= 3), max_its (orbsim3_ransac_parameters),
 * fix_scale = mbFixScale, and n_draws raw rand() values in [0, RAND_MAX]:
 * hypothesis k of a call uses draws[3k .. 3k+2], a call may run min(n_iterations,
 * max_its - *iterations) hypotheses and n_draws must cover them. State, in/out,
 * zero before the first call: *iterations = mnIterations, *best_inliers =
 * mnBestInliers, best_mask[n] = mvbBestInliers, best_T12[16] = mBestT12,
 * best_R[9] = mBestRotation, best_t[3] = mBestTranslation, *best_s =
 * mBestScale. Outputs: T12[16] (row-major; all zero when *result == 0),
 * *result (0 = empty cv::Mat, 1 = a Sim3), *no_more = bNoMore, *n_inliers,
 * inliers[n] per compacted correspondence (the caller scatters them through
 * mvnIndices1), *draws_consumed = 3 x the hypotheses the reference would have
 * run before it returned. */
typedef struct orbsim3_problem {
  float fx, fy, cx, cy;
  int32_t n;
  const float* X3Dc1;
  const float* X3Dc2;
  const float* P1im1;
  const float* P2im2;
  const int32_t* max_error1;
  const int32_t* max_error2;
  int32_t min_inliers;
  int32_t max_its;
  int32_t fix_scale;
  int32_t n_draws;
  const int32_t* draws;
  int32_t* iterations;
  int32_t* best_inliers;
  uint8_t* best_mask;
  float* best_T12;
  float* best_R;
  float* best_t;
  float* best_s;
  float* T12;
  int32_t* result;
  int32_t* no_more;
  int32_t* n_inliers;
  uint8_t* inliers;
  int32_t* draws_consumed;
} orbsim3_problem;
/* Sim3Solver::iterate(n_iterations, ...) for nsolvers independent solvers in
 * one launch. ORBPL_ERR_ARG: n above ORBSIM3_MAX_POINTS, min_inliers below 3, a
 * call that may run more than ORBSIM3_MAX_ITERATIONS hypotheses, or too few
 * draws. */
int orbsim3_iterate(const orbsim3_problem* problems, int nsolvers, int n_iterations);
/* The same over pitched device arrays, asynchronous on `stream`: solver s's
 * correspondences and masks start at s * pt_pitch entries, its draws at s *
 * draw_pitch, its camera at d_cam + 4 s, its T12s at 16 s, best_R at 9 s,
 * best_t at 3 s. n is clamped to the cap and the pitch, min_inliers below 3
 * counts as 3, and the hypotheses of a call are clamped to
 * ORBSIM3_MAX_ITERATIONS and to draw_pitch / 3. */
typedef struct orbsim3_device_batch {
  const int32_t* d_n;
  const float* d_cam;
  const float* d_X3Dc1;
  const float* d_X3Dc2;
  const float* d_P1im1;
  const float* d_P2im2;
  const int32_t* d_max_error1;
  const int32_t* d_max_error2;
  int32_t pt_pitch;
  const int32_t* d_min_inliers;
  const int32_t* d_max_its;
  const int32_t* d_fix_scale;
  const int32_t* d_draws;
  int32_t draw_pitch;
  int32_t* d_iterations;
  int32_t* d_best_inliers;
  uint8_t* d_best_mask;
  float* d_best_T12;
  float* d_best_R;
  float* d_best_t;
  float* d_best_s;
  float* d_T12;
  int32_t* d_result;
  int32_t* d_no_more;
  int32_t* d_n_inliers;
  uint8_t* d_inliers;
  int32_t* d_draws_consumed;
} orbsim3_device_batch;
int orbsim3_iterate_batch_device(const orbsim3_device_batch* b, int nsolvers, int n_iterations,
                                 void* stream);

/* ORBmatcher::SearchBySim3 (ORBmatcher.cc:1441-1693), batched
 * over keyframe pairs: one launch, one workgroup per pair. Each keyframe's
 * points are projected into the other through the Sim3 (s12, R12, t12), the
 * best descriptor within the radius th * mvScaleFactors[level] and the octaves
 * [level - 1, level] is taken on bestDist <= TH_HIGH (100), and a match is
 * kept where both directions agree. reason1 / reason2 say, per feature and
 * direction, where the reference left it: */
#define ORBM_SIM3_MATCHED 0        /* vnMatch is set                           */
#define ORBM_SIM3_NO_POINT 1       /* no map point, or a bad one               */
#define ORBM_SIM3_ALREADY 2        /* vbAlreadyMatched                         */
#define ORBM_SIM3_BEHIND 3         /* z < 0 in the other camera                */
#define ORBM_SIM3_OUT_OF_IMAGE 4   /* !IsInImage(u, v) (also z == 0, NaN)      */
#define ORBM_SIM3_DISTANCE 5       /* outside [0.8 min, 1.2 max]               */
#define ORBM_SIM3_EMPTY_AREA 6     /* GetFeaturesInArea returned nothing       */
#define ORBM_SIM3_NO_MATCH 7       /* bestDist > TH_HIGH (INT_MAX: all gated)  */
#define ORBM_SIM3_MAX_FEATURES 2048
/* One keyframe: kps_un = mvKeysUn (x, y, octave are read), desc[n][32] =
 * mDescriptors, valid[n] = the feature has a map point and it is not bad, and
 * of that point xyz[n][3], min_dist / max_dist[n] = raw mfMinDistance /
 * mfMaxDistance (the 0.8f / 1.2f are applied inside), mp_desc[n][32] =
 * GetDescriptor(); Tcw[16] row-major. */
typedef struct orbm_sim3_keyframe {
  int32_t n;
  const orbpl_keypoint* kps_un;
  const uint8_t* desc;
  const uint8_t* valid;
  const float* xyz;
  const float* min_dist;
  const float* max_dist;
  const uint8_t* mp_desc;
  const float* Tcw;
} orbm_sim3_keyframe;
/* matched12[n1], in/out, in the encoding of orbsim3_pair (the index in
 * keyframe 2 of the matched point, -1 none, -2 a point keyframe 2 does not
 * observe): written only where the reference writes vpMatches12. Outputs:
 * *n_found, vn_match1[n1] / vn_match2[n2] = vnMatch1 / vnMatch2, reason1[n1] /
 * reason2[n2]. */
typedef struct orbm_sim3_pair {
  orbm_sim3_keyframe kf1;
  orbm_sim3_keyframe kf2;
  float s12;
  const float* R12;   /* [9] row-major */
  const float* t12;   /* [3] */
  int32_t* matched12;
  int32_t* n_found;
  int32_t* vn_match1;
  int32_t* vn_match2;
  int32_t* reason1;
  int32_t* reason2;
} orbm_sim3_pair;
/* ORBPL_ERR_ARG: a keyframe with more than ORBM_SIM3_MAX_FEATURES features,
 * nlevels outside [1, 16], a matched12 entry below -2 (one at or above n2 is a
 * match that marks no feature of keyframe 2, as idx2 >= N2 in the reference). */
int orbm_search_by_sim3(const orbpl_camera* cam, const float* scale_factors, int nlevels,
                        const orbm_sim3_pair* pairs, int npairs, float th);
/* The same over pitched device arrays, asynchronous on `stream`: pair p's
 * keyframe-1 arrays start at p * pitch1 entries, its keyframe-2 arrays at p *
 * pitch2, its poses at 16 p, R12 at 9 p, t12 at 3 p. Counts are clamped to the
 * pitches; the pitches lie in [1, ORBM_SIM3_MAX_FEATURES]. */
typedef struct orbm_sim3_device_batch {
  const int32_t* d_n1;
  const int32_t* d_n2;
  int32_t pitch1;
  int32_t pitch2;
  const orbpl_keypoint* d_kps_un1;
  const uint8_t* d_desc1;
  const uint8_t* d_valid1;
  const float* d_xyz1;
  const float* d_min_dist1;
  const float* d_max_dist1;
  const uint8_t* d_mp_desc1;
  const float* d_Tcw1;
  const orbpl_keypoint* d_kps_un2;
  const uint8_t* d_desc2;
  const uint8_t* d_valid2;
  const float* d_xyz2;
  const float* d_min_dist2;
  const float* d_max_dist2;
  const uint8_t* d_mp_desc2;
  const float* d_Tcw2;
  const float* d_s12;
  const float* d_R12;
  const float* d_t12;
  int32_t* d_matched12;
  int32_t* d_n_found;
  int32_t* d_vn_match1;
  int32_t* d_vn_match2;
  int32_t* d_reason1;
  int32_t* d_reason2;
} orbm_sim3_device_batch;
int orbm_search_by_sim3_batch_device(const orbpl_camera* cam, const float* scale_factors,
                                     int nlevels, const orbm_sim3_device_batch* b, int npairs,
                                     float th, void* stream);

/* ------------------------------------------------------------------------
 * Tracking::Relocalization (Tracking.cc:2049-2269) as one batched call over
 * many lost frames, each with its own keyframe database:
 * place recognition, SearchByBoW against every candidate, and then rounds of
 * PnPsolver::iterate(5), PoseOptimization and the two SearchByProjection
 * refinements for all candidates of all frames side by side, with the
 * reference's sequential order restored by an ordered selection per round.
 * The host reads back one count per round.
 * ---------------------------------------------------------------------- */
#define ORBRL_OK 0               /* relocalised: Tcw, assignments, winner are set */
#define ORBRL_NO_CANDIDATES 1    /* DetectRelocalizationCandidates returned none */
#define ORBRL_FAILED 2           /* every candidate was discarded */
#define ORBRL_DRAW_EXHAUSTED 3   /* P31: a solver's next iterate(5) may need more draws than remain */
/* per-candidate record, int32 each; -1 = stage not reached in the last call */
#define ORBRL_REC_BOW_MATCHES 0  /* SearchByBoW's return value */
#define ORBRL_REC_DISCARDED 1    /* vbDiscarded */
#define ORBRL_REC_CALLS 2        /* iterate() calls */
#define ORBRL_REC_ITERATIONS 3   /* mnIterations */
#define ORBRL_REC_DRAWS_USED 4   /* the stream's cursor */
#define ORBRL_REC_RESULT 5       /* last call: 0 empty, 1 refined, 2 best at exhaustion */
#define ORBRL_REC_NO_MORE 6
#define ORBRL_REC_N_INLIERS 7
#define ORBRL_REC_G1 8           /* nGood after the first PoseOptimization */
#define ORBRL_REC_NADD1 9        /* SearchByProjection(th 10, ORBdist 100) */
#define ORBRL_REC_G2 10
#define ORBRL_REC_NADD2 11       /* SearchByProjection(th 3, ORBdist 64) */
#define ORBRL_REC_G3 12
#define ORBRL_REC_INTS 13
typedef struct orbrl_handle orbrl_handle;
/* The handle owns SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991)'s table
 * for N = 0..2048 (orbpnp_ransac_parameters, P28) and the workspace, which
 * grows with the batch. level_sigma2 = mvLevelSigma2; kp_pitch 1024 or 2048 =
 * the most keypoints of a frame or a keyframe; draw_pitch = raw rand() values
 * per candidate stream (P30), a multiple of 4 in [20, 1280]. */
int orbrl_create(const orbpl_camera* cam, const float* scale_factors, const float* level_sigma2,
                 int nlevels, int max_problems, int kp_pitch, int draw_pitch, orbrl_handle** out);
void orbrl_destroy(orbrl_handle* h);
/* the table's first n_entries rows (host only) */
int orbrl_ransac_table(int32_t* min_inliers, int32_t* max_its, int n_entries);
/* One lost frame and its database, host pointers. The database fields are
 * orbkf_problem's (reloc_score in/out). Keyframe k's features are the entries
 * kf_feat_off[k] .. kf_feat_off[k + 1] of the concatenated per-feature arrays:
 * mvKeysUn angle, FeatureVector node id (-1 none), descriptor, kf_valid = the
 * feature's map point exists (bad ones are absent, P27), and that point's
 * world position, raw mfMinDistance / mfMaxDistance and descriptor. The
 * frame: n keypoints (mvKeysUn, mvuRight, descriptors, node ids), its
 * BowVector, and n_draw_streams streams of draw_pitch raw rand() values:
 * candidate c draws from stream c (a candidate without a stream is out of
 * draws at once). Outputs: ok, status (ORBRL_*), winner = database index or
 * -1, rounds = passes of the reference's while loop begun, Tcw, n_good,
 * n_candidates = nCandidates at the end, ncand / cand = place recognition's
 * result, mp_kf_feature[n] = mvpMapPoints as the winner's feature indices (-1
 * none), outlier[n] = mvbOutlier where a map point is assigned (0 elsewhere),
 * records[64][ORBRL_REC_INTS]. On failure Tcw is zero, every assignment -1. */
typedef struct orbrl_problem {
  int32_t nkf;
  const int32_t* kf_off;
  const uint32_t* kf_words;
  const double* kf_vals;
  const int32_t* covis;
  float* reloc_score;
  const int32_t* kf_feat_off;
  const float* kf_angle;
  const int32_t* kf_feat_node;
  const uint8_t* kf_desc;
  const uint8_t* kf_valid;
  const float* mp_xyz;
  const float* mp_min_dist;
  const float* mp_max_dist;
  const uint8_t* mp_desc;
  int32_t n;
  const orbpl_keypoint* kps_un;
  const float* uright;
  const uint8_t* desc;
  const int32_t* feat_node;
  int32_t nq_words;
  const uint32_t* q_words;
  const double* q_vals;
  int32_t n_draw_streams;
  const int32_t* draws;
  int32_t ok, status, winner, rounds, n_good, n_candidates, ncand;
  int32_t cand[64];
  float Tcw[16];
  int32_t* mp_kf_feature;
  uint8_t* outlier;
  int32_t* records;
} orbrl_problem;
/* n <= max_problems problems in one call. ORBPL_ERR_ARG: more than 64
 * keyframes, more than 4096 words, more keypoints or keyframe features than
 * kp_pitch, scoring other than L1_NORM = 0. ORBPL_ERR_OVERFLOW: some problem
 * ended with ORBRL_DRAW_EXHAUSTED (every problem's outputs are still set). */
int orbrl_relocalize(orbrl_handle* h, orbrl_problem* problems, int n, int scoring);
/* The same over pitched device arrays on `stream` (a hipStream_t, NULL = the
 * null stream); orbrl_relocalize packs its problems into this layout and
 * calls it. The call returns when the batch is decided: it waits for the
 * stream once before the rounds and once per round, for 4 bytes each time.
 * Databases as in orbkf_device_batch. Keyframe k of problem p is slot
 * d_kf_first[p] + k: d_kf_n[slot] features at slot * kp_pitch of the
 * per-feature arrays. Frame p: d_n[p] keypoints at p * kp_pitch. Draw stream
 * c of problem p at (p * stream_pitch + c) * draw_pitch, d_n_streams[p] <=
 * stream_pitch <= 64 of them. Outputs per problem: d_cand 64, d_Tcw 16,
 * d_mp_kf_feature / d_outlier kp_pitch, d_records 64 x ORBRL_REC_INTS, the
 * rest one int32. A problem out of draws shows in d_status only. */
typedef struct orbrl_device_batch {
  const int32_t* d_nkf;
  const int32_t* d_kf_off;
  const uint32_t* d_kf_words;
  const double* d_kf_vals;
  int64_t ent_pitch;
  const int32_t* d_covis;
  float* d_reloc_score;
  const int32_t* d_q_n;
  const uint32_t* d_q_words;
  const double* d_q_vals;
  int64_t q_pitch;
  const int32_t* d_kf_first;
  const int32_t* d_kf_n;
  const float* d_kf_angle;
  const int32_t* d_kf_feat_node;
  const uint8_t* d_kf_desc;
  const uint8_t* d_kf_valid;
  const float* d_mp_xyz;
  const float* d_mp_min_dist;
  const float* d_mp_max_dist;
  const uint8_t* d_mp_desc;
  const int32_t* d_n;
  const orbpl_keypoint* d_kps_un;
  const float* d_uright;
  const uint8_t* d_desc;
  const int32_t* d_feat_node;
  const int32_t* d_draws;
  const int32_t* d_n_streams;
  int32_t stream_pitch;
  int32_t* d_cand;
  int32_t* d_ncand;
  int32_t* d_ok;
  int32_t* d_status;
  int32_t* d_winner;
  int32_t* d_rounds;
  int32_t* d_n_good;
  int32_t* d_n_candidates;
  float* d_Tcw;
  int32_t* d_mp_kf_feature;
  uint8_t* d_outlier;
  int32_t* d_records;
} orbrl_device_batch;
int orbrl_relocalize_batch_device(orbrl_handle* h, const orbrl_device_batch* b, int n, int scoring,
                                  void* stream);

/* ------------------------------------------------------------------------
 * LocalMapping::CreateNewMapPoints() then CreateNewMapLines()
 * (LocalMapping.cc:346-665, 668-916) with ORBmatcher(0.6,
 * false).SearchForTriangulation (ORBmatcher.cc:884-1095), ComputeF12
 * (:1106-1127) and LineMatcher::SearchForTriangulation
 * (LineMatcher.cpp:1174-1204), non-monocular (nn = 10), for many independent
 * (current keyframe, <= 10 covisible neighbours) problems in one launch
 * (DESIGN.md P33-P39). Not called by orbpl_tracker_step (P23 stays).
 * ---------------------------------------------------------------------- */
#define ORBLM_MAX_KEYPOINTS 2048   /* per keyframe */
#define ORBLM_MAX_LINES 256        /* per keyframe */
#define ORBLM_MAX_NEIGHBOURS 10    /* GetBestCovisibilityKeyFrames(10) */
/* A keyframe as the block reads it: mnId (observation order, P24), Tcw (16
 * floats, row-major), n features: mvKeys (UnprojectStereo reads the raw
 * keypoint), mvKeysUn, mvuRight, mvDepth, descriptors (32 B rows), the
 * FeatureVector as one node id per feature (orbm_search_by_bow's encoding: -1
 * none, ids < 2^21 - 1), has_mp = the feature holds a map point and mp_xyz
 * that point's world position (3 floats per feature, read where has_mp);
 * nl lines: mvKeyLines (raw), LBD rows (32 B) and mvKeyLineCoefficient (3
 * doubles per line). */
typedef struct orblm_keyframe {
  int32_t id;
  const float* Tcw;
  int32_t n;
  const orbpl_keypoint* kps;
  const orbpl_keypoint* kps_un;
  const float* uright;
  const float* depth;
  const uint8_t* desc;
  const int32_t* feat_node;
  const uint8_t* has_mp;
  const float* mp_xyz;
  int32_t nl;
  const orbpl_keyline* klines;
  const uint8_t* ldesc;
  const double* lcoef;
} orblm_keyframe;
/* A created map point (48 bytes), in the order of creation: by neighbour,
 * then by KF1 feature index. desc_from: 0 = KF1's descriptor, 1 = the
 * neighbour's (ComputeDistinctiveDescriptors with two observations: the
 * lower-id keyframe's). normal, min_dist, max_dist: UpdateNormalAndDepth with
 * KF1 as the reference keyframe (P25). */
typedef struct orblm_point_record {
  int32_t neighbour, idx1, idx2, desc_from;
  float xyz[3];
  float normal[3];
  float min_dist, max_dist;
} orblm_point_record;
/* A created map line (48 bytes), by neighbour, then by KF1 line index: the
 * end points and, as the map model stores a map line, its descriptor's
 * source (desc_from as above) with Observations() = 2. */
typedef struct orblm_line_record {
  int32_t neighbour, idx1, idx2, desc_from;
  float xyz6[6];
  int32_t reserved[2];
} orblm_line_record;
/* One problem, host pointers. neigh: n_neigh <= 10 distinct keyframes in
 * GetBestCovisibilityKeyFrames order. Outputs: points[cur.n] (the first
 * n_points are set), kf1_point_record[cur.n] = the record that occupies
 * KF1's feature (-1 none), pairs[10] = SearchForTriangulation's pairs per
 * neighbour (-1: the neighbour was skipped for its baseline, or is absent);
 * lines[10 * cur.nl] (n_lines set), kf1_line_record[cur.nl] = the last record
 * created for KF1's line (AddMapLine overwrites; every record is kept),
 * line_pairs[10] = LineMatcher::SearchForTriangulation's pairs (-1 as above;
 * 0 also where the neighbour holds no map point, P39). */
typedef struct orblm_problem {
  orblm_keyframe cur;
  int32_t n_neigh;
  const orblm_keyframe* neigh;
  orblm_point_record* points;
  int32_t n_points;
  int32_t* kf1_point_record;
  int32_t pairs[ORBLM_MAX_NEIGHBOURS];
  orblm_line_record* lines;
  int32_t n_lines;
  int32_t* kf1_line_record;
  int32_t line_pairs[ORBLM_MAX_NEIGHBOURS];
} orblm_problem;
/* ORBPL_ERR_ARG: more than 2048 features or 256 lines in a keyframe, more
 * than 10 neighbours, an octave outside [0, nlevels), a node id >= 2^21 - 1,
 * nlevels outside [2, 16] (mfScaleFactor = scale_factors[1]), NULL arrays. */
int orblm_create_new_map_features(const orbpl_camera* cam, const float* scale_factors,
                                  const float* level_sigma2, int nlevels, orblm_problem* problems,
                                  int n);
/* The same over a pitched pool of nkf keyframes in device memory (keyframe k's
 * features at k * kp_pitch, its lines at k * line_pitch of the per-feature /
 * per-line arrays, d_kf_Tcw 16 floats each). Problem p: current keyframe
 * d_cur[p], neighbours d_neigh[p * 10 ..] (-1 = none; the list ends at the
 * first -1). Outputs per problem: d_points[p * kp_pitch ..], d_n_points[p],
 * d_kf1_point_record[p * kp_pitch ..], d_pairs[p * 10 ..], d_lines[p * 10 *
 * line_pitch ..], d_n_lines[p], d_kf1_line_record[p * line_pitch ..],
 * d_line_pairs[p * 10 ..]. Record arrays are 16-byte aligned. Asynchronous on
 * `stream` (a hipStream_t, NULL = the null stream), no readback. Counts above
 * a pitch and pool indices outside [0, nkf) are clamped / skipped on the
 * device. */
typedef struct orblm_device_batch {
  int32_t nkf, kp_pitch, line_pitch;
  const int32_t* d_kf_id;
  const int32_t* d_kf_n;
  const float* d_kf_Tcw;
  const orbpl_keypoint* d_kps;
  const orbpl_keypoint* d_kps_un;
  const float* d_uright;
  const float* d_depth;
  const uint8_t* d_desc;
  const int32_t* d_feat_node;
  const uint8_t* d_has_mp;
  const float* d_mp_xyz;
  const int32_t* d_kf_nl;
  const orbpl_keyline* d_klines;
  const uint8_t* d_ldesc;
  const double* d_lcoef;
  const int32_t* d_cur;
  const int32_t* d_neigh;
  orblm_point_record* d_points;
  int32_t* d_n_points;
  int32_t* d_kf1_point_record;
  int32_t* d_pairs;
  orblm_line_record* d_lines;
  int32_t* d_n_lines;
  int32_t* d_kf1_line_record;
  int32_t* d_line_pairs;
} orblm_device_batch;
int orblm_create_new_map_features_batch_device(const orbpl_camera* cam, const float* scale_factors,
                                               const float* level_sigma2, int nlevels,
                                               const orblm_device_batch* b, int n, void* stream);
/* ORBmatcher(nnratio, check_ori).SearchForTriangulation(pKF1, pKF2, F12,
 * vMatchedPairs, only_stereo) alone: the one problem, one neighbour case of
 * the same kernel without the triangulation. f12_in: F12 row-major (9
 * floats), NULL = ComputeF12(pKF1, pKF2). pairs[2 * kf1->n]: (idx1, idx2) in
 * KF1 index order; f12_out (9 floats, the matrix used) may be NULL. The
 * keyframes' line fields and mp_xyz are not read. */
int orbm_search_for_triangulation(const orbpl_camera* cam, const float* scale_factors,
                                  const float* level_sigma2, int nlevels,
                                  const orblm_keyframe* kf1, const orblm_keyframe* kf2,
                                  const float* f12_in, int only_stereo, int check_ori,
                                  int32_t* pairs, int* npairs, float* f12_out);
/* LineMatcher::SearchForTriangulation(pKF1, pKF2, vMatchedPairs, .) alone
 * (the flag is not read by the reference): pairs[2 * nl1] in KF1 line order.
 * Only the line descriptors are read. nl1, nl2 <= 256. */
int orbl_search_for_triangulation(int nl1, const uint8_t* ldesc1, int nl2, const uint8_t* ldesc2,
                                  int32_t* pairs, int* npairs);

/* ------------------------------------------------------------------------
 * LocalMapping::SearchInNeighbors() (LocalMapping.cc:922-1103, the point
 * half; the line half is commented out in the reference), non-monocular
 * (nn = 10), with ORBmatcher::Fuse(pKF, vpMapPoints, th) (ORBmatcher.cc:
 * 1107-1277), MapPoint::Replace (MapPoint.cc:177-229) and
 * KeyFrame::UpdateConnections of the current keyframe, for many independent
 * maps in one launch. The call mutates the map it is
 * given. Not called by orbpl_tracker_step (P23 stays).
 * ---------------------------------------------------------------------- */
#define ORBLM_MAX_MAP_KF 64        /* keyframes of one map (the map model's bound) */
#define ORBLM_MAX_TARGETS 60       /* 10 first neighbours + 5 second each */
/* ORBmatcher::Fuse: the branch that ended a list entry's iteration */
#define ORBM_FUSE_NULL 0           /* !pMP                                    */
#define ORBM_FUSE_BAD 1            /* pMP->isBad()                            */
#define ORBM_FUSE_IN_KF 2          /* pMP->IsInKeyFrame(pKF)                  */
#define ORBM_FUSE_BEHIND 3         /* z < 0                                   */
#define ORBM_FUSE_OUT_OF_IMAGE 4   /* !pKF->IsInImage(u, v)                   */
#define ORBM_FUSE_DISTANCE 5       /* outside [0.8 min, 1.2 max]              */
#define ORBM_FUSE_VIEW 6           /* PO.dot(Pn) < 0.5 * dist3D               */
#define ORBM_FUSE_EMPTY_WINDOW 7   /* GetFeaturesInArea returned nothing      */
#define ORBM_FUSE_NO_MATCH 8       /* bestDist > TH_LOW after the gates       */
#define ORBM_FUSE_ADDED 9          /* AddObservation + AddMapPoint            */
#define ORBM_FUSE_REPLACED 10      /* pMP->Replace(pMPinKF): the keyframe's point survives */
#define ORBM_FUSE_REPLACES 11      /* pMPinKF->Replace(pMP): the projected point survives  */
#define ORBM_FUSE_BAD_SLOT 12      /* the keypoint holds a bad point: counted, nothing done */
/* A keyframe of a map: mnId (distinct within a map; observation order, P24),
 * Tcw, n <= ORBLM_MAX_KEYPOINTS features (mvKeysUn, mvuRight, descriptors),
 * mp[n] = the map point in each feature's slot as an index into the map's
 * points (-1 none; in/out), ordered = its covisible keyframes in
 * UpdateBestCovisibles order as indices into the map's keyframe table, ended
 * by -1 or by its 64th entry (NULL = none; only the first 10 / 5 are read). */
typedef struct orblm_map_keyframe {
  int32_t id;
  const float* Tcw;
  int32_t n;
  const orbpl_keypoint* kps_un;
  const float* uright;
  const uint8_t* desc;
  int32_t* mp;
  const int32_t* ordered;
} orblm_map_keyframe;
/* A map: nkf <= 64 keyframes and M <= 64 * 2048 map points. In/out per point:
 * xyz[3], normal[3], min_dist / max_dist (the raw mfMinDistance /
 * mfMaxDistance), desc[32], ref_kf (mpRefKF as a table index), bad,
 * n_visible, n_found. The observations are derived from the slot arrays at
 * entry. Out per point: replaced_by (mpReplaced, -1 none), n_obs
 * (Observations()), obs[64] (the feature index in each keyframe of the table,
 * -1 none), desc_src[2] = the (keyframe, feature) whose descriptor the point
 * took when the call last recomputed it (-1, -1: not recomputed). A replaced
 * point keeps its own n_visible / n_found, the survivor gains them. */
typedef struct orblm_map {
  int32_t nkf;
  orblm_map_keyframe* kf;
  int32_t M;
  float* xyz;
  float* normal;
  float* min_dist;
  float* max_dist;
  uint8_t* desc;
  int32_t* ref_kf;
  uint8_t* bad;
  int32_t* n_visible;
  int32_t* n_found;
  int32_t* replaced_by;
  int32_t* n_obs;
  int16_t* obs;
  int32_t* desc_src;
} orblm_map;
/* What SearchInNeighbors reports besides the map: vpTargetKFs as built
 * (duplicates kept), nFused of each forward Fuse and then of the backward one
 * (n_fused[n_targets]), the size of vpFuseCandidates, and the current
 * keyframe's UpdateConnections: conn_w[k] = KFcounter of table keyframe k,
 * ordered / ordered_w = mvpOrderedConnectedKeyFrames / mvOrderedWeights
 * (n_ordered entries; -1 = KFcounter was empty and the lists stay as they
 * were), add_conn[k] = the weight keyframe k receives through AddConnection
 * (0 none); the other keyframes' own lists are not updated (reported only). */
typedef struct orblm_sin_result {
  int32_t targets[ORBLM_MAX_TARGETS];
  int32_t n_targets;
  int32_t n_fused[ORBLM_MAX_TARGETS + 1];
  int32_t n_candidates;
  int32_t conn_w[ORBLM_MAX_MAP_KF];
  int32_t ordered[ORBLM_MAX_MAP_KF];
  int32_t ordered_w[ORBLM_MAX_MAP_KF];
  int32_t n_ordered;
  int32_t add_conn[ORBLM_MAX_MAP_KF];
} orblm_sin_result;
typedef struct orblm_sin_problem {
  orblm_map map;
  int32_t cur;              /* mpCurrentKeyFrame as a table index */
  orblm_sin_result result;  /* out */
} orblm_sin_problem;
/* n problems, host pointers, one launch. ORBPL_ERR_ARG before any device
 * call: NULL arrays, nkf outside [1, 64], more than 2048 features in a
 * keyframe, M outside [0, 64 * 2048], two keyframes of a map with one id, an
 * octave outside [0, nlevels), a slot index outside [-1, M), a point that sits
 * twice in one keyframe, a good point whose ref_kf does not observe it, an
 * ordered entry outside the table or naming its own keyframe, nlevels outside
 * [1, 16], and an array that two problems of the call share (each keyframe
 * and each point belongs to exactly one problem: the call writes them). */
int orblm_search_in_neighbors(const orbpl_camera* cam, const float* scale_factors,
                              const float* level_sigma2, int nlevels,
                              orblm_sin_problem* problems, int n);
/* The same over pools in device memory. Problem p owns the keyframes
 * [kf0, kf0 + nkf) and the points [mp0, mp0 + nmp) of the pools, d_prob[5 * p
 * ..] = (kf0, nkf, mp0, nmp, cur); slot, ordered, ref_kf, replaced_by and
 * cur are indices relative to the problem's own range. The ranges of two
 * problems of one call must not overlap: every problem writes its own. Per
 * keyframe g: d_kf_id[g], d_kf_n[g], d_kf_Tcw[16 g], features at g * kp_pitch
 * of d_kps_un / d_uright / d_desc (32 B rows, 16-byte aligned) / d_mp,
 * d_ordered[64 g ..]. Per point m: d_xyz[3 m], d_normal[3 m], d_min_dist,
 * d_max_dist, d_mp_desc[32 m], d_ref_kf, d_bad, d_n_visible, d_n_found
 * (in/out); d_replaced_by, d_n_obs, d_obs[64 m], d_desc_src[2 m] (out),
 * d_mark[m] (scratch). Per problem: d_result[p], and list_pitch entries each of
 * the scratch d_list / d_search (list_pitch >= kp_pitch; a backward candidate
 * list longer than list_pitch is cut there and sets *d_err, which the caller
 * zeroes beforehand and which the host entry turns into ORBPL_ERR_OVERFLOW).
 * Asynchronous on `stream`, no readback. Counts above a pitch and indices
 * outside a problem's range are clamped / skipped on the device. */
typedef struct orblm_sin_device_batch {
  int32_t nkf, kp_pitch, nmp, list_pitch;
  const int32_t* d_prob;
  const int32_t* d_kf_id;
  const int32_t* d_kf_n;
  const float* d_kf_Tcw;
  const orbpl_keypoint* d_kps_un;
  const float* d_uright;
  const uint8_t* d_desc;
  int32_t* d_mp;
  const int32_t* d_ordered;
  float* d_xyz;
  float* d_normal;
  float* d_min_dist;
  float* d_max_dist;
  uint8_t* d_mp_desc;
  int32_t* d_ref_kf;
  uint8_t* d_bad;
  int32_t* d_n_visible;
  int32_t* d_n_found;
  int32_t* d_replaced_by;
  int32_t* d_n_obs;
  int16_t* d_obs;
  int32_t* d_desc_src;
  uint8_t* d_mark;
  orblm_sin_result* d_result;
  int32_t* d_list;
  int32_t* d_search;
  int32_t* d_err;
} orblm_sin_device_batch;
int orblm_search_in_neighbors_batch_device(const orbpl_camera* cam, const float* scale_factors,
                                           const float* level_sigma2, int nlevels,
                                           const orblm_sin_device_batch* b, int n, void* stream);
/* Profiling: the same launch with in-kernel time stamps. d_ticks (device, 3
 * per problem): the time spent in the search phases of all Fuse calls, in
 * their commit phases, and in the whole workgroup, in ticks of the 100 MHz
 * constant clock. The stamps add a few instructions per Fuse call. */
int orblm_debug_search_in_neighbors_phases(const orbpl_camera* cam, const float* scale_factors,
                                           const float* level_sigma2, int nlevels,
                                           const orblm_sin_device_batch* b, int n, void* stream,
                                           long long* d_ticks);
/* ORBmatcher::Fuse(pKF, vpMapPoints, th) alone on such a map: keyframe `kf`
 * of the table and a list of n_list point indices (-1 = a null entry; an entry
 * may repeat). The map is updated in place as above. Per list entry: reason
 * (ORBM_FUSE_*), and where the search ran to its end (NO_MATCH, ADDED,
 * REPLACED, REPLACES, BAD_SLOT) best_idx / best_dist (-1 / 256 when no
 * candidate passed the gates), else -1 / 256. The one-call case of the same
 * kernel. Refusals as orblm_search_in_neighbors, and list entries outside
 * [-1, M). */
int orbm_fuse(const orbpl_camera* cam, const float* scale_factors, const float* level_sigma2,
              int nlevels, orblm_map* map, int kf, const int32_t* list, int n_list, float th,
              int* n_fused, int32_t* best_idx, int32_t* best_dist, int32_t* reason);

/* ------------------------------------------------------------------------
 * LocalMapping::KeyFrameCulling() (LocalMapping.cc:1224-1319), non-monocular,
 * with KeyFrame::SetBadFlag / EraseConnection / UpdateBestCovisibles
 * (KeyFrame.cc:526-650) and MapPoint::EraseObservation / SetBadFlag
 * (MapPoint.cc:111-168), for many independent maps in one launch (DESIGN.md
 * P48-P51). The call mutates the map and the covisibility graph it is given.
 * Not called by orbpl_tracker_step (P23 stays). Map lines are not touched:
 * the fork's KeyFrame::SetBadFlag leaves mvpMapLines alone, so lines keep
 * observing a culled keyframe. After a call a map may hold bad keyframes:
 * orblm_search_in_neighbors assumes none is (P41), so a caller who chains the
 * two must take the culled keyframes out of the table it passes there.
 * ---------------------------------------------------------------------- */
#define ORBLM_MAX_CULL_LIST 63     /* the current keyframe's covisibles: every other keyframe */
#define ORBLM_KFC_KEPT 0           /* nRedundantObservations <= 0.9 * nMPs              */
#define ORBLM_KFC_CULLED 1         /* SetBadFlag ran to its end                         */
#define ORBLM_KFC_FIRST 2          /* mnId == 0: skipped before the count               */
#define ORBLM_KFC_DEFERRED 3       /* redundant, but mbNotErase: mbToBeErased set only  */
/* vpLocalKeyFrames as copied at entry (table indices) and, per list entry,
 * nMPs, nRedundantObservations and what became of it; n_points_bad = the
 * number of map points the call set bad. */
typedef struct orblm_kfc_result {
  int32_t list[ORBLM_MAX_CULL_LIST];
  int32_t n_list;
  int32_t n_mps[ORBLM_MAX_CULL_LIST];
  int32_t n_redundant[ORBLM_MAX_CULL_LIST];
  int32_t action[ORBLM_MAX_CULL_LIST];
  int32_t n_points_bad;
} orblm_kfc_result;
/* A map, its current keyframe and the graph state orblm_map lacks, per map of
 * nkf keyframes: depth[k] = mvDepth of keyframe k (map.kf[k].n floats; in);
 * conn_w[nkf * nkf], row k = keyframe k's mConnectedKeyFrameWeights (0 = not
 * connected; need not be symmetric; in/out); ordered[nkf * 64] = every
 * keyframe's mvpOrderedConnectedKeyFrames as table indices, ended by -1 or
 * the 64th entry (state of its own, not derived from conn_w; in/out;
 * map.kf[k].ordered is not read); parent[nkf] = mpParent (-1 none; in/out);
 * not_erase[nkf] = mbNotErase (in); kf_bad[nkf] = mbBad (in/out);
 * to_be_erased[nkf] = mbToBeErased (out: 1 where the call deferred a cull);
 * the observations are derived from the slot arrays at entry, those of a
 * keyframe that is bad at entry left out (SetBadFlag does not clear a culled
 * keyframe's own slots, but its points no longer observe it);
 * Tcp[16 * nkf] = mTcp, written only for a keyframe the call culled. Of the
 * map the call writes the slot arrays, ref_kf, bad, n_obs and obs. */
typedef struct orblm_kfc_problem {
  orblm_map map;
  int32_t cur;
  const float* const* depth;
  int32_t* conn_w;
  int32_t* ordered;
  int32_t* parent;
  const uint8_t* not_erase;
  uint8_t* kf_bad;
  uint8_t* to_be_erased;
  float* Tcp;
  orblm_kfc_result result;  /* out */
} orblm_kfc_problem;
/* n problems, host pointers, one launch; th_depth is cam->th_depth.
 * ORBPL_ERR_ARG before any device call: everything orblm_search_in_neighbors
 * refuses for the map itself, and NULL graph arrays, a negative weight, a
 * non-zero diagonal of conn_w, an ordered or parent entry outside the table or
 * naming its own keyframe, an ordered list that names a keyframe twice, a
 * keyframe with id != 0 and parent == -1 that is not bad, and an array that
 * two problems share. */
int orblm_keyframe_culling(const orbpl_camera* cam, int nlevels, orblm_kfc_problem* problems, int n);
/* The same over pools in device memory, with the conventions of
 * orblm_sin_device_batch: d_prob[5 * p ..] = (kf0, nkf, mp0, nmp, cur), every
 * index relative to the problem's own range, ranges of two problems disjoint.
 * Per keyframe g: d_kf_id, d_kf_n, d_kf_Tcw[16 g], d_kps_un / d_uright /
 * d_depth / d_mp at g * kp_pitch, d_conn_w[64 g + j] = its weight towards
 * keyframe j of its own map, d_ordered[64 g ..], d_parent, d_not_erase,
 * d_kf_bad, d_to_be_erased (zeroed by the call), d_Tcp[16 g]. Per point m:
 * d_ref_kf, d_bad (in/out), d_n_obs, d_obs[64 m] (out). Per problem:
 * d_result[p]. A problem whose range lies outside the pools is not run and
 * sets *d_err, which the caller zeroes beforehand. Asynchronous on `stream`,
 * no readback; counts above a pitch are clamped on the device. */
typedef struct orblm_kfc_device_batch {
  int32_t nkf, kp_pitch, nmp;
  const int32_t* d_prob;
  const int32_t* d_kf_id;
  const int32_t* d_kf_n;
  const float* d_kf_Tcw;
  const orbpl_keypoint* d_kps_un;
  const float* d_uright;
  const float* d_depth;
  int32_t* d_mp;
  int32_t* d_conn_w;
  int32_t* d_ordered;
  int32_t* d_parent;
  const uint8_t* d_not_erase;
  uint8_t* d_kf_bad;
  uint8_t* d_to_be_erased;
  float* d_Tcp;
  int32_t* d_ref_kf;
  uint8_t* d_bad;
  int32_t* d_n_obs;
  int16_t* d_obs;
  orblm_kfc_result* d_result;
  int32_t* d_err;
} orblm_kfc_device_batch;
int orblm_keyframe_culling_batch_device(const orbpl_camera* cam, const orblm_kfc_device_batch* b,
                                        int n, void* stream);

/* ------------------------------------------------------------------------
 * LocalMapping::MapPointCulling() then MapLineCulling() (LocalMapping.cc:
 * 246-340), non-monocular (nThObs = 3), on the recently added points and
 * lines of many independent maps in one launch. Host entry
 * only. Per list entry, in the reference's order: already bad (dropped from
 * the list), GetFoundRatio() < 0.25f (SetBadFlag, dropped), age >= 2 and
 * Observations() <= 3 (SetBadFlag, dropped), age >= 3 (dropped), else it
 * stays. SetBadFlag: bad = 1, the slot in every observer goes to -1, n_obs is
 * kept.
 * ---------------------------------------------------------------------- */
#define ORBLM_MAX_MAP_LINES (ORBLM_MAX_MAP_KF * ORBLM_MAX_LINES)
#define ORBLM_RC_WAS_BAD 0
#define ORBLM_RC_FOUND_RATIO 1
#define ORBLM_RC_FEW_OBSERVATIONS 2
#define ORBLM_RC_AGED_OUT 3
#define ORBLM_RC_STAYS 4
/* map: as above (the call writes the slot arrays, bad, n_obs, obs); kf_bad[nkf]
 * = mbBad per keyframe (NULL: none is; a bad keyframe's slots give no
 * observations, as in orblm_keyframe_culling); cur_id =
 * mpCurrentKeyFrame->mnId; first_kf[M] = mnFirstKFid; recent[n_recent] =
 * mlpRecentAddedMapPoints as point indices (in/out: what remains, in order;
 * no entry may repeat) with reason[] per entry as passed in (out). Lines: L <=
 * 64 * 256 of them; nl[k] <= 256 line features of keyframe k with their slot
 * array ml[k] (-1 none; in/out); line_bad (in/out), line_n_visible,
 * line_n_found, line_first_kf (may be -1), line_n_obs (the caller's nObs, not
 * derived; in); recent_lines / n_recent_lines / line_reason the same way. */
typedef struct orblm_recent_problem {
  orblm_map map;
  const uint8_t* kf_bad;
  int32_t cur_id;
  const int32_t* first_kf;
  int32_t* recent;
  int32_t n_recent;      /* in/out */
  int32_t* reason;
  int32_t L;
  const int32_t* nl;
  int32_t* const* ml;
  uint8_t* line_bad;
  const int32_t* line_n_visible;
  const int32_t* line_n_found;
  const int32_t* line_first_kf;
  const int32_t* line_n_obs;
  int32_t* recent_lines;
  int32_t n_recent_lines;  /* in/out */
  int32_t* line_reason;
} orblm_recent_problem;
/* ORBPL_ERR_ARG before any device call: what orblm_search_in_neighbors refuses
 * for the map, NULL arrays, list entries outside the tables, a list entry that
 * repeats, L outside [0, 64 * 256], nl outside [0, 256], a line slot outside
 * [-1, L), and an array that two problems share. */
int orblm_cull_recent(int nlevels, orblm_recent_problem* problems, int n);

/* ------------------------------------------------------------------------
 * Optimizer::PoseOptimization / PoseOptimizationWithLines
 * (Optimizer.cc:375-619, 2132-2486): 4 rounds x 10 Levenberg-Marquardt
 * iterations on one SE3 vertex, Huber kernel in rounds 0-2, chi2 outlier
 * re-labelling after each round. Point edge i exists if has_mp[i]; it is
 * monocular if uright[i] < 0 else stereo. Line edge j exists if has_ml[j].
 * ---------------------------------------------------------------------- */
typedef struct orbpl_pose_problem {
  int32_t n;                   /* points: N                                   */
  const orbpl_keypoint* kps_un;
  const float* uright;
  const uint8_t* has_mp;
  const float* mp_xyz;         /* n x 3                                       */
  int32_t nl;                  /* lines: NL (0 for PoseOptimization)          */
  const float* kl_obs;         /* nl x 4: startX, startY, endX, endY (mvKeyLinesUn) */
  const int32_t* kl_octave;    /* nl                                          */
  const uint8_t* has_ml;       /* nl                                          */
  const float* ml_xyz;         /* nl x 6: world start, world end              */
  const float* inv_sigma2;     /* mvInvLevelSigma2, nlevels                   */
  int32_t nlevels;
} orbpl_pose_problem;

/* Tcw: in = pFrame->mTcw, out = optimised pose (4x4 row-major float).
 * outlier[n] / line_outlier[nl]: in = pFrame->mvbOutlier / mvbLineOutlier,
 * out = after the call. *n_inliers = return value of the reference
 * (nInitialCorrespondences - nBad, 0 if < 3 correspondences). */
int orbpl_pose_optimization(const orbpl_camera* cam, const orbpl_pose_problem* prob, float* Tcw,
                            uint8_t* outlier, uint8_t* line_outlier, int* n_inliers);
/* Pose options. ORBPL_POSE_FIXED_LINE_JAC: the analytic EdgeLineOnlyPose
 * Jacobian ("--fixed-line-jacobian") instead of the
 * reference's as-written one (types_line_expmap.h:138-152: row 0 overwritten
 * by the end point, row 1 uninitialised -> 0 (pinned P7), +fx*cy in dI_dLc,
 * R*v in place of n_c in dLc_ddelta): de_i/dl = ((x_i - l0 N_i/ln^2)/ln,
 * (y_i - l1 N_i/ln^2)/ln, 1/ln), l = K_line n_c, dn_c/d(w,u) =
 * [-[n_c]x | -[v_c]x] under g2o's left update exp(d) * T. */
#define ORBPL_POSE_FIXED_LINE_JAC 1
int orbpl_pose_optimization_ex(const orbpl_camera* cam, const orbpl_pose_problem* prob, int flags,
                               float* Tcw, uint8_t* outlier, uint8_t* line_outlier,
                               int* n_inliers);


/* ------------------------------------------------------------------------
 * Batched RGB-D tracker: the per-frame hot path of Tracking::Track for
 * n_streams independent camera streams on one device, one
 * TrackWithMotionModel step per call (Tracking.cc:1212-1330):
 *   Frame(RGB-D) extraction + glue -> constant-velocity prediction ->
 *   SearchByProjection(cur, last, th=15, retry 2*th if < 20) ->
 *   PoseOptimization -> discard outliers -> velocity update.
 * Every frame then acts as the keyframe of the next one: its keypoints with
 * depth become map points (StereoInitialization-style, Tracking.cc:608-660);
 * local mapping / loop closing are out of scope.
 * ---------------------------------------------------------------------- */
typedef struct orbpl_tracker orbpl_tracker;

int orbpl_tracker_create(const orbpl_orb_params* orb, const orbpl_camera* cam, int n_streams,
                         int device, orbpl_tracker** out);
/* Tracker flags. ORBPL_TRACK_LINES: the point-and-line variant of the
 * reference's RGB-D tracking (Tracking.cc:1210-1320 with mbUseLines):
 * LineExtractor per frame (lsdx_*), UndistortKeyLines + line depths,
 * LineMatcher::SearchByProjection against the last frame's map lines,
 * PoseOptimization with line edges, line outlier discard and map lines. */
#define ORBPL_TRACK_LINES 1
/* ORBPL_TRACK_STEREO: the reference's stereo tracking (Tracking::GrabImageStereo,
 * Tracking.cc:180-208): Frame(imLeft, imRight) runs ORB on both images
 * concurrently (Frame.cc:88-91), UndistortKeyPoints, ComputeStereoMatches
 * (Frame.cc:886-1063) for depth / uRight; SearchByProjection uses th = 7
 * (Tracking.cc:1238-1241). Images up to 1024 rows.
 * ORBPL_TRACK_STEREO | ORBPL_TRACK_LINES (BASELINE configs[3], a DEFINED mode:
 * the reference's stereo Frame extracts no lines but PoseOptimizationWithLines
 * loops over NL, Optimizer.cc:2287-2303): LineExtractor on both images, line
 * end-point depths from the best LBD match on the right image whose line
 * passes the angle / length / row-overlap / disparity tests,
 * then the RGB-D line path (line matching, line edges, map lines). */
#define ORBPL_TRACK_STEREO 2
/* ORBPL_TRACK_LOCAL_MAP: Tracking::TrackLocalMap after TrackWithMotionModel
 * (Tracking.cc:1332-1420): the local map is the map points / lines of the last
 * 4 frames (every tracked frame is a keyframe) minus those the
 * frame already holds or rejected; SearchLocalPoints (IsInFrustum 0.5,
 * ORBmatcher(0.8).SearchByProjection th 3 RGB-D / 1 stereo, 5 for the first
 * frames), SearchLocalLines (LineMatcher(0.8) local-map overload with its
 * relaxed retry), a second PoseOptimizationWithLines over all matches and the
 * mnMatchesInliers / mnLineMatchesInliers decision. */
#define ORBPL_TRACK_LOCAL_MAP 4
/* ORBPL_TRACK_FIXED_LINE_JAC: PoseOptimizationWithLines with the analytic line
 * Jacobian (ORBPL_POSE_FIXED_LINE_JAC) in every tracker pose. */
#define ORBPL_TRACK_FIXED_LINE_JAC 8
/* ORBPL_TRACK_REFKF: Tracking::Track's choice between TrackWithMotionModel
 * and TrackReferenceKeyFrame (Tracking.cc:324-338, 942-1032; needs a
 * vocabulary, orbpl_tracker_set_vocabulary): the first frame after the
 * initial one (no velocity) and every frame whose motion-model tracking
 * fails are tracked against the reference keyframe (the last frame, P18) by
 * ORBmatcher(0.7, true).SearchByBoW + LineMatcher's reference-keyframe
 * overload from the pose of the last frame, then PoseOptimizationWithLines
 * and the outlier discard; success = 10 map inliers (and, with lines, a
 * line count of 10 after the reference's outlier decrement). Pinned P22. */
#define ORBPL_TRACK_REFKF 16
/* ORBPL_TRACK_MAP: Tracking::Track with the reference's map model
 * (Tracking.cc:283-599; RGB-D streams): StereoInitialization (> 500 keypoints:
 * the first keyframe, a map point per keypoint with depth, a map line per line
 * with both end-point depths), UpdateLastFrame's temporal VO points / lines,
 * TrackWithMotionModel against the last frame's map points / lines,
 * TrackReferenceKeyFrame against the reference keyframe (with
 * ORBPL_TRACK_REFKF and a vocabulary), TrackLocalMap over the covisibility
 * graph (UpdateLocalKeyFrames / UpdateLocalPoints / UpdateLocalLines,
 * SearchLocalPoints / SearchLocalLines, the second pose), NeedNewKeyFrame,
 * CreateNewKeyFrame and LocalMapping::ProcessNewKeyFrame (observations,
 * distinctive descriptors, normals, UpdateConnections), the LOST state and the
 * reset of a map with <= 5 keyframes. Per stream a keyframe table (32 by
 * default; ORBPL_MAP_KF in the environment at creation, 2..64) and point / line
 * pools of keyframes x keypoint capacity / x 80 in HBM: with F keyframe slots
 * and K keypoints per frame about F*K*(160 + 4*F) + F*80*112 bytes per stream
 * (the observation table grows with F^2: K = 1000 gives ~9.5 MB at F = 32,
 * ~27 MB at F = 64, i.e. ~10 / ~28 GB for 1024 streams). A stream whose map
 * needs a keyframe beyond its F slots declines it and raises capacity flag 1
 * (orbpl_tracker_get_map_errors): size F above the keyframes a run inserts
 * (at most one per step). Pinned P23-P25
 * (DESIGN.md): LocalMapping = its ProcessNewKeyFrame run synchronously,
 * Relocalization fails; pointer-ordered containers in keyframe id order.
 * Replaces ORBPL_TRACK_LOCAL_MAP (its P18 local map). With ORBPL_TRACK_STEREO
 * the same Track() on stereo frames (orbpl_tracker_step_stereo: depths from
 * ComputeStereoMatches, line depths P17) with the reference's STEREO branches:
 * motion-model radius 7, local-map radius 1, outlier matches dropped after
 * TrackLocalMap's pose (Tracking.cc:1238-1241, 1374-1401, 1801-1809). */
#define ORBPL_TRACK_MAP 32
int orbpl_tracker_create_ex(const orbpl_orb_params* orb, const orbpl_camera* cam, int n_streams,
                            int device, int flags, orbpl_tracker** out);
int orbpl_tracker_destroy(orbpl_tracker* tr);
/* Forget all stream state; the next step initialises every stream with pose
 * Tcw0 (n_streams x 16 floats row-major, NULL = identity). */
int orbpl_tracker_reset(orbpl_tracker* tr, const float* Tcw0);
/* mVelocity = cv::Mat() for every stream s with mask[s] != 0 (n_streams
 * bytes): the state Tracking holds after its initialisation or a
 * relocalisation, so the stream's next step runs TrackReferenceKeyFrame
 * instead of TrackWithMotionModel (Tracking.cc:324-338; with
 * ORBPL_TRACK_REFKF and a vocabulary; without them the next prediction uses
 * zero velocity). Waits for the tracker's queued steps. Used to time and test
 * TrackReferenceKeyFrame under load. */
int orbpl_tracker_clear_velocity(orbpl_tracker* tr, const uint8_t* mask);
/* Camera.fps of the settings (ORBPL_TRACK_MAP trackers): mMaxFrames = fps,
 * 0 -> 30 (Tracking.cc:81-87), read by NeedNewKeyFrame and TrackLocalMap's
 * recent-relocalisation test. Default 30 (TUM); KITTI's settings say 10. */
int orbpl_tracker_set_fps(orbpl_tracker* tr, float fps);
/* One step for all streams. d_gray: n_streams frames of width*height u8;
 * d_depth: n_streams frames of width*height float metres (device memory,
 * contiguous). Asynchronous on the tracker's stream. */
int orbpl_tracker_step(orbpl_tracker* tr, const uint8_t* d_gray, const float* d_depth);
/* Stereo step (ORBPL_TRACK_STEREO trackers): d_left / d_right hold n_streams
 * rectified frames of width*height u8 each (device memory, contiguous). */
int orbpl_tracker_step_stereo(orbpl_tracker* tr, const uint8_t* d_left, const uint8_t* d_right);
/* Tracking::GrabImageRGBD from host buffers (Tracking.cc:225-248): n_streams
 * gray frames and n_streams 16-bit depth maps (TUM PNG depth, raw units),
 * copied asynchronously on the tracker's copy stream into one of 3 device
 * slots (pinned memory from orbpl_host_alloc makes the copy overlap the
 * previous steps' kernels), depth converted as imDepth.convertTo(CV_32F,
 * 1.0f / depth_map_factor) (pinned P21: float(v) * (1.0f / factor); TUM:
 * DepthMapFactor 5000), then the step. The host buffers may be reused after
 * the next orbpl_tracker_synchronize. */
int orbpl_tracker_step_host(orbpl_tracker* tr, const uint8_t* h_gray, const uint16_t* h_depth,
                            float depth_map_factor);
int orbpl_tracker_synchronize(orbpl_tracker* tr);
/* on != 0: extraction of step t+1 may overlap matching/pose of step t (two
 * HIP streams, three frame buffers). Results are identical either way. */
int orbpl_tracker_set_pipelined(orbpl_tracker* tr, int on);
/* Results of the last step, per stream (any pointer may be NULL):
 * Tcw (16 floats), keypoints, SearchByProjection matches, PoseOptimization
 * inliers, map matches after outlier removal. */
int orbpl_tracker_get_state(orbpl_tracker* tr, float* Tcw, int* nkeypoints, int* nmatches,
                            int* ninliers, int* nmatches_map);
/* hipEvent times of the last step (ms): extract, glue, match, pose, finish. */
int orbpl_tracker_stage_ms(orbpl_tracker* tr, float* ms5);
/* Per-kernel device times (ms, hipEvents on the tracker stream) of the last
 * min(max_steps, 64) steps, 11 per step: pyramid (+ borders + blur, one
 * launch), blur (0), fast, octree, orient+desc, glue+predict, match, pose,
 * finish, local_map (TrackLocalMap: gather, IsInFrustum, local point and line
 * search, second pose, counts; 0 without ORBPL_TRACK_LOCAL_MAP), bow
 * (KeyFrame::ComputeBoW; 0 without a vocabulary). Stereo matching counts in
 * glue. */
int orbpl_tracker_timings(orbpl_tracker* tr, int max_steps, float* ms, int* n_steps);
int orbpl_tracker_timings_reset(orbpl_tracker* tr);
/* Floats per step written by orbpl_tracker_timings, _line_timings,
 * _lsd_timings, _stereo_timings and _kernel_timings (in that order): 11, 3, 7,
 * 4, 4. A caller sizes its buffers max_steps x these. */
int orbpl_tracker_timing_counts(int* counts5);
/* Frames one launch of the extraction kernels (pyramid, FAST, octree,
 * orient+desc) and of the LSD kernels processes. Both equal the stream count
 * unless the tracker splits that batch into two offset halves on two streams
 * (ORBPL_ORB_SPLIT=1; ORBPL_LSD_SPLIT, by default from 1024 streams when the
 * HIP runtime has GPU_MAX_HW_QUEUES >= 8): then the first half's, whose
 * launches the stage timings above bracket. lsd_frames is 0 without lines. */
int orbpl_tracker_launch_frames(const orbpl_tracker* tr, int* orb_frames, int* lsd_frames);
/* Per-kernel device times (ms) of the last min(max_steps, 64) steps, 4 per
 * step, each launch bracketed by its own hipEvents on the tracking stream:
 * k_pose of TrackWithMotionModel, k_pose of TrackReferenceKeyFrame (0 without
 * ORBPL_TRACK_REFKF), k_pose of TrackLocalMap and k_match_local (0 without
 * ORBPL_TRACK_LOCAL_MAP). Summed per kernel they give a kernel's GPU time per
 * step across the stages it runs in. */
int orbpl_tracker_kernel_timings(orbpl_tracker* tr, int max_steps, float* ms, int* n_steps);
/* Debug (ORBPL_POSE_PROFILE set): stream 0's PoseOptimization phase times of
 * the last step in ns (edges, linearize reduction, solve+exp, trial errors,
 * classify), the LM iteration / trial counts, the linearize edge loop (ns). */
int orbpl_tracker_debug_pose_profile(orbpl_tracker* tr, long long* out8);
/* Debug (ORBPL_MATCH_PROFILE set): stream 0's last-frame SearchByProjection
 * phase times of the last step in ns (grid, candidates, ordered claims,
 * rotation check, output). */
int orbpl_tracker_debug_match_profile(orbpl_tracker* tr, long long* out5);
/* Per-stream frame outputs of the last step (host copies, kp_cap entries per
 * stream, see orbpl_tracker_kp_capacity): undistorted keypoints, descriptors,
 * match (last-frame index per keypoint or -1), outlier flags. */
int orbpl_tracker_kp_capacity(const orbpl_tracker* tr);
int orbpl_tracker_get_frame(orbpl_tracker* tr, int stream, orbpl_keypoint* kps_un, uint8_t* desc,
                            int32_t* match, uint8_t* outlier, int* n);
/* Tracking outcome of the last step per stream: ok (TrackWithMotionModel's
 * return), lines of the frame, LineMatcher matches (every passing pair
 * counts, as in the reference), line map matches after outlier discard
 * (outliers decrement, Tracking.cc:1306). Line counts are 0 without lines. */
int orbpl_tracker_get_status(orbpl_tracker* tr, int* ok, int* nlines, int* line_matches,
                             int* line_nmatches_map);
/* Line outputs of the last step (kLineKeep = 80 entries per stream):
 * undistorted KeyLines, LBD rows, matched last-frame line (-1 none), outlier
 * flags. ORBPL_TRACK_LINES trackers only. */
int orbpl_tracker_get_lines(orbpl_tracker* tr, int stream, orbpl_keyline* kl_un, uint8_t* desc,
                            int32_t* lmatch, uint8_t* loutlier, int* n);
/* Line stage device times (ms) of the last min(max_steps, 64) steps, 3 per
 * step: LSD, KeyLines + LBD + UndistortKeyLines, line SearchByProjection. */
int orbpl_tracker_line_timings(orbpl_tracker* tr, int max_steps, float* ms, int* n_steps);
/* Per-step history of every stream, recorded on the device by D2D copies at
 * the end of each step (no host synchronisation inside a step): the next
 * max_steps steps after the call are kept (0 = off; a new call clears it).
 * get_history returns stream `stream`'s first min(max_steps, recorded) steps:
 * Tcw (16 floats per step) and 12 counts per step in the oracle's order:
 * nkeypoints, nmatches, ninliers, nmatches_map, ok, nlines, line_matches,
 * line_nmatches_map, then the TrackLocalMap counts (0 when it did not run):
 * local matches, mnMatchesInliers, local line matches, mnLineMatchesInliers. */
int orbpl_tracker_set_history(orbpl_tracker* tr, int max_steps);
int orbpl_tracker_get_history(orbpl_tracker* tr, int stream, int max_steps, float* Tcw,
                              int* counts12, int* n_steps);
/* ORBPL_TRACK_MAP trackers: the recorded steps' 24 counts per step in the
 * oracle's order (oracle_map_step): the 12 of get_history, then keyframe
 * created (1, 2 = the initial one), keyframes, map points, map lines,
 * temporal points, TrackReferenceKeyFrame ran, reference keyframe (-1 none),
 * state (0 not initialised, 1 OK, 2 LOST), local keyframes, local map points
 * searched, local map lines searched, temporal lines. */
int orbpl_tracker_get_map_history(orbpl_tracker* tr, int stream, int max_steps, int* counts24,
                                  int* n_steps);
/* ORBPL_TRACK_MAP trackers: capacity flags of each stream's map since the last
 * reset (1 keyframe table full: NeedNewKeyFrame declined; 2 point / line pool
 * full; 4 local list full); 0 = the map matches the reference's. */
int orbpl_tracker_get_map_errors(orbpl_tracker* tr, int* err);
/* ORBPL_TRACK_MAP trackers, one stream's map after the last step (host copies):
 * keyframes (n_kf; per keyframe its spanning-tree parent (-1 none), the number
 * of ordered connections and the first `cap` of them (GetVectorCovisibleKeyFrames
 * order, -1 padded)); map points (n_mp; the first `cap`: Observations(),
 * GetDescriptor(), world position, GetNormal(), [mfMinDistance,
 * mfMaxDistance]); map lines (n_ml; Observations(), descriptor, end points).
 * Any output pointer may be NULL. */
int orbpl_tracker_get_map_keyframes(orbpl_tracker* tr, int stream, int* parent, int* ord, int cap,
                                    int* nord, int* n_kf);
int orbpl_tracker_get_map_points(orbpl_tracker* tr, int stream, int cap, int* nobs, uint8_t* desc,
                                 float* xyz, float* normal, float* dist2, int* n_mp);
int orbpl_tracker_get_map_lines(orbpl_tracker* tr, int stream, int cap, int* nobs, uint8_t* desc,
                                float* pos6, int* n_ml);
/* KeyFrame::ComputeBoW (KeyFrame.cc:67; every tracked frame is a keyframe,
 * P18) with `voc` (uploaded to the tracker's device; not owned, must outlive
 * the tracker or be unset with NULL): each step transforms the frame's
 * descriptors on the extraction stream (levelsup: Frame::ComputeBoW's 4). */
int orbpl_tracker_set_vocabulary(orbpl_tracker* tr, orbv_vocab* voc, int levelsup);
/* the last step's BowVector / FeatureVector of one stream (buffers of the
 * tracker's keypoint capacity); n = its keypoints */
int orbpl_tracker_get_bow(orbpl_tracker* tr, int stream, uint32_t* bow_words, double* bow_vals,
                          int* bow_n, int32_t* feat_node, int* n);
/* per stream: 1 when the last step ran TrackReferenceKeyFrame (ORBPL_TRACK_REFKF) */
int orbpl_tracker_get_trk(orbpl_tracker* tr, int* trk);
/* TrackLocalMap outcome of the last step per stream (ORBPL_TRACK_LOCAL_MAP; 0
 * where it did not run): SearchLocalPoints matches, mnMatchesInliers,
 * SearchLocalLines matches (every passing pair counts), mnLineMatchesInliers. */
int orbpl_tracker_get_local_stats(orbpl_tracker* tr, int* local_matches, int* local_inliers,
                                  int* local_line_matches, int* local_line_inliers);
/* LSD / LineExtractor kernel times (ms) of the last min(max_steps, 64) steps,
 * 7 per step (line stream): k_lsd_blur + k_lsd_resize + k_lsd_grad, the
 * pseudo-ordering sort (k_lsd_sort + k_lsd_sort_local), the seed loop
 * (k_lsd_spec), NFA validation + compaction, KeyLines (k_keylines), blur5 +
 * Sobel + LBD, UndistortKeyLines + line depths. */
int orbpl_tracker_lsd_timings(orbpl_tracker* tr, int max_steps, float* ms, int* n_steps);
/* Stereo stage device times (ms) of the last min(max_steps, 64) steps, 4 per
 * step: right-image ORB extraction, ComputeStereoMatches (KeyFrame::ComputeBoW
 * is the bow entry of orbpl_tracker_timings), and with
 * ORBPL_TRACK_LINES the right-image LineExtractor and the stereo line depths
 * (k_stereo_lines); 0 without lines. */
int orbpl_tracker_stereo_timings(orbpl_tracker* tr, int max_steps, float* ms, int* n_steps);

/* ------------------------------------------------------------------------
 * Line tracking, single frame, host pointers (n <= 80 = LineExtractor's cap)
 * ---------------------------------------------------------------------- */
/* Frame::UndistortKeyLines (Frame.cc:769-845) + the line part of
 * ComputeStereoFromRGBD (Frame.cc:1090-1116): undistorted key lines, depth
 * at the distorted end points (-1 = none; imDepth.at<float>(int(v), int(u))
 * on the row-major image) and uRight = x_un - bf / depth (-1 = none). depth
 * may be NULL (no depth: all -1). */
int orbpl_line_frame_prepare(const orbpl_camera* cam, const orbpl_keyline* kl, int n,
                             const float* depth, orbpl_keyline* kl_un, float* dstart, float* dend,
                             float* ur_start, float* ur_end);
/* LineMatcher(0.9, true).SearchByProjection(CurrentFrame, LastFrame)
 * (LineMatcher.cpp:72-269): last-frame map lines (has_ml, outlier flags,
 * world start/end xyz x6, LBD rows) projected with Tcw and Liang-Barsky
 * clipped to the image bounds; every (projected, current) pair passing
 * LineMatching counts, the last passing one wins; one relaxed retry when
 * matches / ncur < 0.2. match[j] = last-frame index or -1. */
int orbl_search_by_projection_last(const orbpl_camera* cam, const float* Tcw, int ncur,
                                   const orbpl_keyline* cur_kl_un, const uint8_t* cur_desc,
                                   int nlast, const orbpl_keyline* last_kl_un,
                                   const uint8_t* has_ml, const uint8_t* last_outlier,
                                   const float* ml_xyz6, const uint8_t* last_desc, int32_t* match,
                                   int* nmatches);

/* Frame::IsInFrustum(MapLine*) (Frame.cc:403-430): in_view unless both
 * world end points (xyz6 = start, end) are behind the camera. */
int orbl_frame_is_in_frustum(const float* Tcw, int n, const float* xyz6, uint8_t* in_view);
/* LineMatcher::SearchByProjection(F, vpLocalMapLines) (LineMatcher.cpp:755-952,
 * valid = mbTrackInView) and SearchByProjection(F, RefKF) (:527-721, valid =
 * mvpMapLines[i] != NULL): any number of map lines (world xyz6, LBD rows).
 * Current lines whose map line has Observations() > 0 (cur_nobs, NULL: none)
 * are skipped in the first pass. match[j] = map line index assigned to
 * current line j, -1 = unchanged; *wiped = 1 when the relaxed retry ran, which
 * first clears every F.mvpMapLines entry (-1 then means NULL). */
int orbl_search_by_projection_list(const orbpl_camera* cam, const float* Tcw, int ncur,
                                   const orbpl_keyline* cur_kl_un, const uint8_t* cur_desc,
                                   const int32_t* cur_nobs, int nml, const uint8_t* valid,
                                   const float* ml_xyz6, const uint8_t* ml_desc, int32_t* match,
                                   int* nmatches, int* wiped);
/* The reference's harness overloads, which also return new_kls (the
 * projected, clipped KeyLines, appended by the caller) and match_indices
 * (every passing (projected i, current j) pair; the relaxed retry clears
 * them): mode 0 = SearchByProjection(Frame&, const Frame&, new_kls,
 * match_indices) (include/LineMatcher.h:51, LineMatcher.cpp:272-487, called by
 * Test/LastFrameProjection.cpp:293): projected KeyLines are copies of
 * base_kl[i] (LastFrame.mvKeyLinesUn) rebuilt by UpdateKeyLineData,
 * Observations() > 0 is tested per pair on the map line current line j holds
 * at that moment (cur_nobs initially, ml_nobs of a map line a pass assigned),
 * retry when matches * 1.0 / NL < 0.2; mode 1 = SearchByProjection(Frame&,
 * const vector<MapLine*>&, new_kls, match_indices) (LineMatcher.h:66,
 * LineMatcher.cpp:954-1170, Test/LocalMapProjectionTest.cpp:334): fresh
 * (zeroed) KeyLines, the Observations() skip per current line, retry when
 * matches <= 0.2 NL. valid = mvpMapLines[i] && !mvbLineOutlier[i] && !isBad()
 * (mode 0) / mbTrackInView && !isBad() (mode 1). Outputs: proj_kl / proj_src
 * (nml capacity; *nproj), pairs as int (i, j) (pair_cap capacity; *npairs =
 * the full count), match[j] = map line assigned by the final pass or -1,
 * *wiped = 1 when the retry ran (every assignment cleared first). cur_nobs,
 * base_kl and ml_nobs may be NULL. (LineMatcher.h:59 declares a reference-
 * keyframe variant the reference never defines.) */
int orbl_search_by_projection_pairs(const orbpl_camera* cam, const float* Tcw, int mode, int ncur,
                                    const orbpl_keyline* cur_kl_un, const uint8_t* cur_desc,
                                    const int32_t* cur_nobs, int nml, const uint8_t* valid,
                                    const orbpl_keyline* base_kl, const float* ml_xyz6,
                                    const uint8_t* ml_desc, const int32_t* ml_nobs,
                                    orbpl_keyline* proj_kl, int32_t* proj_src, int* nproj,
                                    int32_t* pairs, int pair_cap, int* npairs, int32_t* match,
                                    int* nmatches, int* wiped);
/* SearchByProjection(Frame&, KeyFrame*, vector<MapLine*>& vpMapLineMatches)
 * (LineMatcher.h:56, LineMatcher.cpp:492-525): cv::BFMatcher(NORM_HAMMING)
 * knnMatch(keyframe line descriptors = queries, current line descriptors =
 * train, k = 2) and best / second < 0.75 (float): out[j] = the last query
 * whose best train line is j, or -1; *nmatches counts every passing query.
 * Ties go to the lower train index; a query with fewer than two train lines
 * has no match (pinned: the reference reads past the end). nq <= 256. */
int orbl_match_bf_knn(int nq, const uint8_t* qdesc, int nt, const uint8_t* tdesc, int32_t* out,
                      int* nmatches);
/* Stereo line end-point depths, the defined mode P17 of DESIGN.md (the
 * reference's stereo Frame extracts no lines): left line i takes the right
 * line with the smallest LBD Hamming distance (the first on ties) among those
 * passing, in this order, Hamming <= 45, |angle difference| <= 10 degrees,
 * min / max length >= 0.45f, both lines non-horizontal (|dy| >= 0.25 length),
 * row overlap >= 0.5 of the shorter row span and both end-point disparities in
 * (0, bf / mb). dstart / dend = bf / disparity, -1 without a match. kl / kr:
 * the left / right (rectified) KeyLines with their LBD rows; nl, nr <= 80. */
int orbl_stereo_line_depths(const orbpl_camera* cam, const orbpl_keyline* kl, const uint8_t* desc,
                            int nl, const orbpl_keyline* kr, const uint8_t* desc_r, int nr,
                            float* dstart, float* dend);

/* ------------------------------------------------------------------------
 * Hamming distance — ORBmatcher::DescriptorDistance (ORBmatcher.cc:2083-2103)
 * ---------------------------------------------------------------------- */
int orbpl_descriptor_distance(const uint8_t* a32, const uint8_t* b32);

/* ------------------------------------------------------------------------
 * Line features: LineExtractor::ExtractLineSegment (LineExtractor.cpp:12-74)
 *   LSDDetector::detect(img, keylines, 1, 1)   -> lsdx_detect*
 * One lsdx_ctx per (device, image geometry, max batch); asynchronous on its
 * own HIP stream.
 * ---------------------------------------------------------------------- */
typedef struct lsdx_ctx lsdx_ctx;

int lsdx_create(int width, int height, int max_batch, int device, lsdx_ctx** out);
int lsdx_destroy(lsdx_ctx* ctx);
/* Device-free geometry query (no HIP call): the 0.8-scaled size and the
 * smallest region the detector fits for a width x height image, as
 * lsdx_create would use them. Any pointer may be NULL. */
int lsdx_describe(int width, int height, int* sw, int* sh, int* min_reg_size);
/* LineSegmentDetector::detect (LSD_REFINE_ADV, scale 0.8) on one host image:
 * segments (x1, y1, x2, y2) in detection order. ORBPL_ERR_CAPACITY if more
 * than cap segments (n_out holds the count). */
int lsdx_detect(lsdx_ctx* ctx, const uint8_t* img, int width, int height, int stride,
                float* lines, int cap, int* n_out);
/* The same for `batch` device-resident frames (frame f at d_imgs + f*frame_pitch). */
int lsdx_detect_batch_device(lsdx_ctx* ctx, const uint8_t* d_imgs, int batch, int stride,
                             int64_t frame_pitch);
int lsdx_synchronize(lsdx_ctx* ctx);
/* LineExtractor::ExtractLineSegment(img, key_lines, line_descriptor,
 * keyline_coefficients) (LineExtractor.cpp:12-74): LSD, KeyLines sorted by
 * response and cut to the 80 longest when more were found, LBD descriptors
 * (32 bytes per row, rows follow the KeyLine order), normalised homogeneous
 * line coefficients (3 doubles per line). */
int lsdx_extract(lsdx_ctx* ctx, const uint8_t* img, int width, int height, int stride,
                 orbpl_keyline* keylines, uint8_t* desc, double* coef, int cap, int* n_out);
int lsdx_extract_batch_device(lsdx_ctx* ctx, const uint8_t* d_imgs, int batch, int stride,
                              int64_t frame_pitch);
int lsdx_get_keylines(lsdx_ctx* ctx, int frame, orbpl_keyline* keylines, uint8_t* desc,
                      double* coef, int cap, int* n_out);
/* Device buffers of the last extraction: frame f's lines start at
 * f*80 KeyLines / f*80*32 bytes / f*80*3 doubles; d_n[f] is the count. */
int lsdx_device_outputs(lsdx_ctx* ctx, orbpl_keyline** d_keylines, uint8_t** d_desc,
                        double** d_coef, int32_t** d_n);
int lsdx_get_lines(lsdx_ctx* ctx, int frame, float* lines, int cap, int* n_out);
/* Intermediate stages of the last run (parity tests): 0.8-scaled 8-bit image
 * (sw*sh), fastAtan2 degrees per pixel (-1 = NOTDEF), pseudo-ordered pixels
 * (x | y << 16, (sw-1)*(sh-1) entries). Any pointer may be NULL. */
int lsdx_get_stages(lsdx_ctx* ctx, int frame, uint8_t* scaled, float* deg, uint32_t* order,
                    int* sw, int* sh, int* n_order);
/* Test hook: the device replica of std::sort(records, key greater) on keys
 * in [0, 1023]; perm receives the record indices in sorted order. */
int orbpl_test_introsort(const int32_t* keys, int n, int32_t* perm);
/* Test hook, host only: ComputeSim3 on the three sampled points P1 / P2
 * [3][3] (point c at 3 c) and CheckInliers over n correspondences with that
 * hypothesis, through the header the kernel shares (sim3_core.h). err[n][2] =
 * err1, err2. */
int orbpl_test_sim3_hypothesis(const float* P1, const float* P2, int fix_scale, const float* cam,
                               int n, const float* X3Dc1, const float* X3Dc2, const float* P1im1,
                               const float* P2im2, const int32_t* max_error1,
                               const int32_t* max_error2, float* R, float* t, float* s, float* T12,
                               float* err, uint8_t* inliers);
/* Debug: batch-mean shader-clock counters of the LSD seed loop of the last
 * run. Speculative loop (default): growing cycles, rounds, speculative
 * regions, total cycles, fit + refinement cycles, validate + commit
 * cycles, critical-path grow steps | cooperative regions << 40, rectangles
 * passed to NFA validation. Wave-serial loop: growing cycles, fit +
 * refinement cycles, 0, total cycles, region pixels, prefetches, prefetch
 * cycles, rectangles. */
int lsdx_debug_profile(lsdx_ctx* ctx, long long* out8);
/* on != 0: run the wave-serial seed loop (one region at a time, the direct
 * restatement) instead of the speculative lane-parallel one. Both give the
 * same lines; the switch exists for testing and measurement. */
int lsdx_set_serial_grow(lsdx_ctx* ctx, int on);


#ifdef __cplusplus
}
#endif

#endif /* ORBPL_H */
