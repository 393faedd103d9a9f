// Host runtime + C-ABI of the tracking half of the hot path: the batched
// device-resident orbpl_tracker. (The single-frame host-pointer forms are in
// track_host.cpp.)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/orbpl.h"
#include "host_stage.h"
#include "orb_kernels.h"
#include "orbpl_runtime.h"
#include "track_kernels.h"
#include "lsd_kernels.h"
#include "map_kernels.h"

using namespace orbpl;

namespace {

// streams from which the RGB-D lines tracker splits its LSD batch in two
// offset halves (ORBPL_LSD_SPLIT overrides)
constexpr int kLsdSplitMin = 1024;
// likewise the ORB extraction batch (ORBPL_ORB_SPLIT=1 turns it on): the
// second half's pyramid beside the first half's FAST, and so on down the
// chain. Off by default: at 16 queues points +1.8 % and rig +3.5 % (within
// the run-to-run spread), lines -2 %
constexpr int kOrbSplitMin = 1 << 30;

// the HIP runtime runs with >= 8 hardware queues (recorded at library load,
// orbpl_runtime.cpp): with the default 4, extra streams share queues and
// serialise
bool enough_hw_queues() { return hw_queues() >= 8; }
// a split switch: env "0" off, "1" on, else on from `min_streams` when the
// runtime has the queues for it
bool split_on(const char* env, int n_streams, int min_streams) {
  if (n_streams < 2) return false;   // two halves need a frame each, even when forced
  const char* e = getenv(env);
  return e ? e[0] == '1' : n_streams >= min_streams && enough_hw_queues();
}

}  // namespace

bool orbpl::lsd_split_decision(int n_streams) {
  return split_on("ORBPL_LSD_SPLIT", n_streams, kLsdSplitMin);
}

// ---------------------------------------------------------------------------
// Batched tracker
// ---------------------------------------------------------------------------
struct FrameBufs {
  KeyPointD* kps = nullptr;
  uint8_t* desc = nullptr;
  int* n = nullptr;
  KeyPointD* kps_un = nullptr;
  float* depth = nullptr;
  float* uright = nullptr;
  int* gcell = nullptr;
  int* match = nullptr;
  uint8_t* outlier = nullptr;
  uint8_t* has_mp = nullptr;
  float* mp_xyz = nullptr;
  int* nobs = nullptr;
  // lines (kLineKeep per stream)
  orbpl_keyline* kl = nullptr;
  orbpl_keyline* kl_un = nullptr;
  uint8_t* ldesc = nullptr;
  double* lcoef = nullptr;
  int* nl = nullptr;
  float* dstart = nullptr;
  float* dend = nullptr;
  int* lmatch = nullptr;
  uint8_t* loutlier = nullptr;
  uint8_t* has_ml = nullptr;
  float* ml_xyz = nullptr;
  // map model (ORBPL_TRACK_MAP): the frame's map elements (pool id, -1, or a
  // temporal element -2 - slot) and, as the last frame, the map point / line
  // descriptors the matchers read
  int* mpid = nullptr;
  uint8_t* mp_desc = nullptr;
  int* mlid = nullptr;
  uint8_t* ml_desc = nullptr;
  // DBoW2 (orbpl_tracker_set_vocabulary): KeyFrame::ComputeBoW of the frame
  int32_t* feat_node = nullptr;   // FeatureVector: node per keypoint, -1 = stopped
  int32_t* feat_word = nullptr;
  double* feat_weight = nullptr;
  uint32_t* bow_words = nullptr;  // BowVector (word order)
  double* bow_vals = nullptr;
  int* bow_n = nullptr;
};

// map-mode scratch of the matchers (local lists, reference-keyframe lines)
struct MapExtra {
  uint8_t* l_inview;
  float *l_px, *l_py, *l_pxr, *l_vcos;
  int* l_level;
  int4* l_scratch;
  uint8_t* ll_valid;
  orbpl_keyline* ll_proj;
  int* ll_src;
  orbpl_keyline* trk_proj;
  int* trk_src;
};

struct orbpl_tracker {
  orbx_ctx* ex = nullptr;
  int device = 0;
  int S = 0;
  int W = 0, H = 0;
  int kp_cap = 0;
  // Two HIP streams: extraction (+ frame glue) of step t+1 runs on `stream`
  // while matching / pose / finish of step t run on `tstream`. Three frame
  // buffers: step t extracts into fb[t%3] and tracks against fb[(t-1)%3].
  hipStream_t stream = nullptr;    // owned by the extractor context
  hipStream_t tstream = nullptr;   // tracking stream
  TrackConsts consts{};
  FrameBufs fb[3];
  hipEvent_t ev_free[3] = {};      // fb[b] no longer read as "last frame"
  bool free_pending[3] = {};
  int pipelined = 0;               // 0: every stage on `stream`
  // line features (ORBPL_TRACK_LINES): LSD + LBD + UndistortKeyLines run on
  // their own stream, concurrently with the ORB extraction of the same step
  int lines = 0;
  lsdx_ctx* lx = nullptr;
  hipStream_t lstream = nullptr;
  hipEvent_t ev_in = nullptr;      // step start on `stream`
  // split LSD (ORBPL_LSD_SPLIT, lines at >= kLsdSplitMin streams): the
  // first lsplit frames on lstream_a (context lx), the rest on lstream_b
  // (lx2) started once the first half's pseudo-ordering sort is done, so the
  // halves' chains run offset: one half's latency-bound sort and validation
  // beside the other's VALU-bound seed loop. The line glue then runs on
  // lstream after both.
  int lsplit = 0;
  // split ORB extraction (points / RGB-D lines at >= kOrbSplitMin streams):
  // the first osplit frames on `stream` (context ex), the rest on stream2
  // (ex2) once the first half's pyramid is done
  int osplit = 0;
  orbx_ctx* ex2 = nullptr;
  hipStream_t stream2 = nullptr;   // owned by ex2
  hipEvent_t ev_ob_done = nullptr;
  lsdx_ctx* lx2 = nullptr;
  hipStream_t lstream_a = nullptr, lstream_b = nullptr;
  hipEvent_t ev_la_sort = nullptr, ev_la_done = nullptr, ev_lb_done = nullptr;
  // stereo (ORBPL_TRACK_STEREO): the right image's ORB extraction runs on the
  // right extractor's stream, concurrently with the left one; the batched
  // ComputeStereoMatches then fills depth / uRight on the extraction stream
  int stereo = 0;
  int fixed_line_jac = 0;          // ORBPL_TRACK_FIXED_LINE_JAC
  orbx_ctx* exr = nullptr;
  hipStream_t rstream = nullptr;   // owned by exr
  hipEvent_t ev_rin = nullptr;     // step start on `stream`
  KeyPointD* r_kps = nullptr;      // right keypoints (S x kp_cap), one buffer
  uint8_t* r_desc = nullptr;
  int* r_n = nullptr;
  int* st_sad = nullptr;           // stereo scratch: SAD per left keypoint
  uint16_t* st_entries = nullptr;  // stereo scratch: row-band entries
  int st_entry_cap = 0;            // entries per frame
  int* d_err = nullptr;            // stereo capacity flag
  // stereo + lines (P17): LineExtractor on the right images on its own
  // stream, then k_stereo_lines on the line stream
  lsdx_ctx* lxr = nullptr;
  hipStream_t rlstream = nullptr;
  hipEvent_t ev_rlin = nullptr;    // step start on `stream`
  hipEvent_t ev_sl_done = nullptr; // k_stereo_lines finished reading the right lines
  orbpl_keyline* r_kl = nullptr;   // right KeyLines (S x kLineKeep), one buffer
  uint8_t* r_ldesc = nullptr;
  double* r_lcoef = nullptr;
  int* r_nl = nullptr;
  StreamState* d_state = nullptr;
  PoseEdge* d_edges = nullptr;
  static constexpr int kRing = 64;   // steps kept in the timing ring
  static constexpr int kEvGlue = 36 + kKernelBrackets;   // glue start (frame_prepare)
  static constexpr int kEvXdone = kEvGlue + 1;            // extraction done (glue on ts)
  static constexpr int kEv = kEvXdone + 1;   // events per step (28..35: kernel brackets,
                                             // 36..: extraction launch brackets)
  std::vector<hipEvent_t> ring;      // kRing * kEv events
  int ring_pos = 0, ring_count = 0;
  // TrackLocalMap (ORBPL_TRACK_LOCAL_MAP): ring of the last kLmK keyframes'
  // maps, the gathered local lists and the second pose's buffers
  static constexpr int kLmK = 4;
  int local_map = 0;
  int refkf = 0;                   // ORBPL_TRACK_REFKF (needs a vocabulary)
  int glue_on_ts = 0;              // pipelined RGB-D: glue + BoW on the tracking stream
  int *trk_lcur = nullptr, *trk_nobs = nullptr, *trk_lm = nullptr, *trk_nml = nullptr;
  orbpl_keyline* trk_proj = nullptr;
  int* trk_src = nullptr;
  int lm_step = 0;                 // frames since reset (Frame::mnId)
  // host-buffer ingress (orbpl_tracker_step_host): 3 device slots of gray,
  // u16 depth and converted f32 depth, filled on a copy stream
  static constexpr int kIn = 3;
  hipStream_t cstream = nullptr;
  uint8_t* in_gray[kIn] = {};
  uint16_t* in_d16[kIn] = {};
  float* in_depth[kIn] = {};
  hipEvent_t in_copied[kIn] = {}, in_done_s[kIn] = {}, in_done_l[kIn] = {};
  bool in_used[kIn] = {};
  int in_pos = 0;
  orbv_vocab* voc = nullptr;       // orbpl_tracker_set_vocabulary (not owned)
  int voc_levelsup = 4;
  int* d_bow_err = nullptr;
  float scale_factor = 1.2f;
  long long lp = 0, llp = 0;
  float *kr_xyz = nullptr, *kr_nrm = nullptr, *kr_dmin = nullptr, *kr_dmax = nullptr;
  uint8_t *kr_has = nullptr, *kr_desc = nullptr;
  int* kr_n = nullptr;
  float* rl_xyz = nullptr;
  uint8_t *rl_has = nullptr, *rl_desc = nullptr;
  int* rl_n = nullptr;
  float *l_xyz = nullptr, *l_nrm = nullptr, *l_dmin = nullptr, *l_dmax = nullptr;
  uint8_t* l_desc = nullptr;
  int* l_n = nullptr;
  uint8_t* l_inview = nullptr;
  float *l_px = nullptr, *l_py = nullptr, *l_pxr = nullptr, *l_vcos = nullptr;
  int* l_level = nullptr;
  int4* l_scratch = nullptr;
  float* ll_xyz = nullptr;
  uint8_t *ll_desc = nullptr, *ll_valid = nullptr;
  int* ll_n = nullptr;
  orbpl_keyline* ll_proj = nullptr;
  int* ll_src = nullptr;
  int *cur_nobs = nullptr, *cur_nobs_l = nullptr, *lm_match = nullptr, *llm_match = nullptr;
  int *match2 = nullptr, *lmatch2 = nullptr;
  float *xyz2 = nullptr, *lxyz2 = nullptr;
  uint8_t *outlier2 = nullptr, *loutlier2 = nullptr;
  // per-step history (orbpl_tracker_set_history): StreamState and keypoint /
  // line counts of every stream after each step, device-side D2D copies on
  // the tracking stream (no host synchronisation inside a step)
  int hist_cap = 0, hist_count = 0;
  StreamState* d_hist_state = nullptr;
  int* d_hist_n = nullptr;
  int* d_hist_nl = nullptr;
  // map model (ORBPL_TRACK_MAP, map_kernels.hip): keyframe table and point /
  // line pools per stream, the reference keyframe staged as a frame, the
  // pose inputs in current-frame index space
  int map = 0;
  int map_kfc = 0;
  MapArgs ma{};
  MapExtra mx{};
  std::vector<void*> map_allocs;
  std::vector<void*> allocs;
};

namespace orbpl {
hipStream_t orbx_stream(orbx_ctx* c);
}

static int tr_alloc(orbpl_tracker* t, void** p, size_t bytes) {
  hipError_t e = hipMalloc(p, bytes ? bytes : 1);
  if (e != hipSuccess) return hip_fail(e, "hipMalloc", __LINE__);
  t->allocs.push_back(*p);
  return hipMemset(*p, 0, bytes ? bytes : 1) == hipSuccess ? ORBPL_OK : ORBPL_ERR_HIP;
}

// Map-model buffers for `kfc` keyframes per stream (pools of kfc x keypoint
// capacity points and kfc x 80 lines, the local lists of the same sizes);
// replaces earlier ones. Per-stream state is reset by the caller.

static int map_alloc(orbpl_tracker* t, int kfc) {
  MapExtra* x = &t->mx;
  for (void* p : t->map_allocs) (void)hipFree(p);
  t->map_allocs.clear();
  const size_t S = t->S, K = t->kp_cap, L = kLineKeep, F = (size_t)kfc;
  const size_t MPC = F * K, MLC = F * L;
  auto A = [&](void** p, size_t bytes) -> int {
    hipError_t e = hipMalloc(p, bytes ? bytes : 1);
    if (e != hipSuccess) return hip_fail(e, "hipMalloc (map model)", __LINE__);
    t->map_allocs.push_back(*p);
    return ORBPL_OK;
  };
#define MA(ptr, bytes)                                  \
  do {                                                  \
    int _r = A((void**)&(ptr), (bytes));                \
    if (_r) return _r;                                  \
  } while (0)
  MapArgs& m = t->ma;
  m.kfc = kfc;
  m.kp_pitch = (int)K;
  m.mpc = (long long)MPC;
  m.mlc = (long long)MLC;
  m.lines = t->lines;
  m.stereo = t->stereo;
  m.max_frames = 30;   // Camera.fps 30 (TUM); orbpl_tracker_set_fps
  m.lp = (long long)MPC;
  m.llp = (long long)MLC;
  MA(m.ms, S * sizeof(MapState));
  MA(m.kf_T, S * F * 16 * 4);
  MA(m.kf_Ow, S * F * 4 * 4);
  MA(m.kf_N, S * F * 4);
  MA(m.kf_NL, S * F * 4);
  MA(m.kf_frame, S * F * 4);
  MA(m.kf_mp, S * F * K * 4);
  MA(m.kf_kp, S * F * K * sizeof(KeyPointD));
  MA(m.kf_ur, S * F * K * 4);
  MA(m.kf_desc, S * F * K * 32);
  MA(m.kf_node, S * F * K * 4);
  MA(m.kf_ml, S * F * L * 4);
  MA(m.kf_ldesc, S * F * L * 32);
  MA(m.kf_ds, S * F * L * 4);
  MA(m.kf_de, S * F * L * 4);
  MA(m.kf_w, S * F * F * 4);
  MA(m.kf_ord, S * F * F);
  MA(m.kf_nord, S * F * 4);
  MA(m.kf_parent, S * F * 4);
  MA(m.kf_first, S * F * 4);
  MA(m.kf_child, S * F * 8);
  MA(m.mp_pos, S * MPC * 16);
  MA(m.mp_nrm, S * MPC * 16);
  MA(m.mp_dist, S * MPC * 8);
  MA(m.mp_desc, S * MPC * 32);
  MA(m.mp_nobs, S * MPC * 4);
  MA(m.mp_nob, S * MPC * 4);
  MA(m.mp_obs, S * MPC * F * 4);
  MA(m.mp_seen, S * MPC * 4);
  MA(m.mp_tref, S * MPC * 4);
  MA(m.ml_pos, S * MLC * 24);
  MA(m.ml_desc, S * MLC * 32);
  MA(m.ml_nobs, S * MLC * 4);
  MA(m.ml_seen, S * MLC * 4);
  MA(m.ml_tref, S * MLC * 4);
  MA(m.r_n, S * 4);
  MA(m.r_kps_un, S * K * sizeof(KeyPointD));
  MA(m.r_desc, S * K * 32);
  MA(m.r_has_mp, S * K);
  MA(m.r_mp_xyz, S * K * 12);
  MA(m.r_node, S * K * 4);
  MA(m.r_mpid, S * K * 4);
  MA(m.r_nl, S * 4);
  MA(m.r_has_ml, S * L);
  MA(m.r_ml_xyz, S * L * 24);
  MA(m.r_ml_desc, S * L * 32);
  MA(m.r_mlid, S * L * 4);
  MA(m.trk_cur_nobs, S * L * 4);
  MA(m.trk_lm, S * L * 4);
  MA(m.trk_nml, S * 4);
  MA(m.trk_list, S * 4);
  MA(m.trk_count, 4);
  MA(m.m2, S * K * 4);
  MA(m.pxyz, S * K * 12);
  MA(m.lm2, S * L * 4);
  MA(m.lpxyz, S * L * 24);
  MA(m.l_xyz, S * MPC * 12);
  MA(m.l_nrm, S * MPC * 12);
  MA(m.l_dmin, S * MPC * 4);
  MA(m.l_dmax, S * MPC * 4);
  MA(m.l_ldesc_pts, S * MPC * 32);
  MA(m.l_count, S * 4);
  MA(m.l_id, S * MPC * 4);
  MA(m.ll_xyz, S * MLC * 24);
  MA(m.ll_desc, S * MLC * 32);
  MA(m.ll_count, S * 4);
  MA(m.ll_id, S * MLC * 4);
  MA(m.cur_nobs, S * K * 4);
  MA(m.cur_nobs_l, S * L * 4);
  MA(x->l_inview, S * MPC);
  MA(x->l_px, S * MPC * 4);
  MA(x->l_py, S * MPC * 4);
  MA(x->l_pxr, S * MPC * 4);
  MA(x->l_vcos, S * MPC * 4);
  MA(x->l_level, S * MPC * 4);
  MA(x->l_scratch, S * MPC * sizeof(int4));
  MA(x->ll_valid, S * MLC);
  MA(x->ll_proj, S * MLC * sizeof(orbpl_keyline));
  MA(x->ll_src, S * MLC * 4);
  MA(x->trk_proj, S * L * sizeof(orbpl_keyline));
  MA(x->trk_src, S * L * 4);
  int* lm_match = nullptr;
  int* llm_match = nullptr;
  MA(lm_match, S * K * 4);
  MA(llm_match, S * L * 4);
  m.lm_match = lm_match;
  m.llm_match = llm_match;
#undef MA
  if (hipMemset(m.kf_w, 0, S * F * F * 4) != hipSuccess) return hip_fail(hipErrorUnknown, "hipMemset", __LINE__);
  t->map_kfc = kfc;
  return ORBPL_OK;
}

extern "C" {

int orbpl_tracker_destroy(orbpl_tracker* t) {
  if (!t) return ORBPL_OK;
  (void)hipSetDevice(t->device);
  for (void* p : t->allocs) (void)hipFree(p);
  for (void* p : t->map_allocs) (void)hipFree(p);
  if (t->tstream) (void)hipStreamSynchronize(t->tstream);
  for (auto& e : t->ring)
    if (e) (void)hipEventDestroy(e);
  for (auto& e : t->ev_free)
    if (e) (void)hipEventDestroy(e);
  if (t->lstream) (void)hipStreamSynchronize(t->lstream);
  if (t->rstream) (void)hipStreamSynchronize(t->rstream);
  if (t->rlstream) (void)hipStreamSynchronize(t->rlstream);
  if (t->ev_rlin) (void)hipEventDestroy(t->ev_rlin);
  if (t->ev_sl_done) (void)hipEventDestroy(t->ev_sl_done);
  if (t->rlstream) (void)hipStreamDestroy(t->rlstream);
  if (t->lxr) lsdx_destroy(t->lxr);
  if (t->ev_in) (void)hipEventDestroy(t->ev_in);
  if (t->ev_rin) (void)hipEventDestroy(t->ev_rin);
  if (t->exr) orbx_destroy(t->exr);
  if (t->cstream) {
    (void)hipStreamSynchronize(t->cstream);
    (void)hipStreamDestroy(t->cstream);
  }
  for (int k = 0; k < orbpl_tracker::kIn; k++) {
    if (t->in_copied[k]) (void)hipEventDestroy(t->in_copied[k]);
    if (t->in_done_s[k]) (void)hipEventDestroy(t->in_done_s[k]);
    if (t->in_done_l[k]) (void)hipEventDestroy(t->in_done_l[k]);
  }
  if (t->tstream) (void)hipStreamDestroy(t->tstream);
  if (t->lstream_a) (void)hipStreamSynchronize(t->lstream_a);
  if (t->lstream_b) (void)hipStreamSynchronize(t->lstream_b);
  if (t->lstream) (void)hipStreamDestroy(t->lstream);
  if (t->lstream_a) (void)hipStreamDestroy(t->lstream_a);
  if (t->lstream_b) (void)hipStreamDestroy(t->lstream_b);
  for (hipEvent_t e : {t->ev_la_sort, t->ev_la_done, t->ev_lb_done})
    if (e) (void)hipEventDestroy(e);
  if (t->lx) lsdx_destroy(t->lx);
  if (t->lx2) lsdx_destroy(t->lx2);
  if (t->ex) orbx_destroy(t->ex);
  if (t->ex2) orbx_destroy(t->ex2);
  if (t->ev_ob_done) (void)hipEventDestroy(t->ev_ob_done);
  delete t;
  return ORBPL_OK;
}

int orbpl_tracker_create(const orbpl_orb_params* orb, const orbpl_camera* cam, int n_streams,
                         int device, orbpl_tracker** out) {
  return orbpl_tracker_create_ex(orb, cam, n_streams, device, 0, out);
}

int orbpl_tracker_create_ex(const orbpl_orb_params* orb, const orbpl_camera* cam, int n_streams,
                            int device, int flags, orbpl_tracker** out) {
  if (!orb || !cam || !out || n_streams <= 0) return arg_fail("bad argument");
  if (flags & ~(ORBPL_TRACK_LINES | ORBPL_TRACK_STEREO | ORBPL_TRACK_LOCAL_MAP |
                ORBPL_TRACK_FIXED_LINE_JAC | ORBPL_TRACK_REFKF | ORBPL_TRACK_MAP))
    return arg_fail("unknown tracker flag");
  // ORBPL_TRACK_LINES | ORBPL_TRACK_STEREO: the defined stereo line mode (P17;
  // the reference's stereo Frame extracts no lines, Frame.cc:70-131)
  if ((flags & ORBPL_TRACK_STEREO) && cam->height > 1024)
    return arg_fail("stereo tracking supports images up to 1024 rows");
  *out = nullptr;
  orbpl_tracker* t = new orbpl_tracker();
  t->device = device;
  t->lines = (flags & ORBPL_TRACK_LINES) ? 1 : 0;
  t->stereo = (flags & ORBPL_TRACK_STEREO) ? 1 : 0;
  t->fixed_line_jac = (flags & ORBPL_TRACK_FIXED_LINE_JAC) ? 1 : 0;
  t->local_map = (flags & ORBPL_TRACK_LOCAL_MAP) ? 1 : 0;
  t->refkf = (flags & ORBPL_TRACK_REFKF) ? 1 : 0;
  t->map = (flags & ORBPL_TRACK_MAP) ? 1 : 0;
  if (t->map) t->local_map = 0;   // the map model has its own TrackLocalMap
  t->scale_factor = orb->scale_factor;
  t->S = n_streams;
  t->W = cam->width;
  t->H = cam->height;
  const bool osplit = !(flags & ORBPL_TRACK_STEREO) && split_on("ORBPL_ORB_SPLIT", n_streams, kOrbSplitMin);
  t->osplit = osplit ? (n_streams + 1) / 2 : 0;
  int rc = orbx_create(orb, cam->width, cam->height, osplit ? t->osplit : n_streams, device, &t->ex);
  if (rc) {
    delete t;
    return rc;
  }
  if (osplit) {
    rc = orbx_create(orb, cam->width, cam->height, n_streams - t->osplit, device, &t->ex2);
    if (!rc && hipEventCreateWithFlags(&t->ev_ob_done, hipEventDisableTiming) != hipSuccess)
      rc = hip_fail(hipErrorUnknown, "hipEventCreate", __LINE__);
    if (rc) {
      orbpl_tracker_destroy(t);
      return rc;
    }
    t->stream2 = orbpl::orbx_stream(t->ex2);
  }
  t->kp_cap = orbx_max_keypoints(t->ex);
  if (t->kp_cap > kMatchMaxKp) {
    orbpl_tracker_destroy(t);
    return arg_fail("nfeatures too large for the tracker (max 2048 keypoints per frame)");
  }
  float scale[16], inv_sigma2[16];
  int nlev = 0;
  orbx_get_scale_info(t->ex, &nlev, scale, nullptr, nullptr, inv_sigma2);
  rc = make_consts(cam, scale, inv_sigma2, nlev, &t->consts);
  if (rc) {
    orbpl_tracker_destroy(t);
    return rc;
  }
  t->stream = orbpl::orbx_stream(t->ex);
  const size_t S = n_streams, K = t->kp_cap;
#define TA(ptr, bytes)                                        \
  do {                                                        \
    int _r = tr_alloc(t, (void**)&(ptr), (bytes));            \
    if (_r) { orbpl_tracker_destroy(t); return _r; }          \
  } while (0)
  for (int b = 0; b < 3; b++) {
    FrameBufs& f = t->fb[b];
    TA(f.kps, S * K * sizeof(KeyPointD));
    TA(f.desc, S * K * 32);
    TA(f.n, S * 4);
    TA(f.kps_un, S * K * sizeof(KeyPointD));
    TA(f.depth, S * K * 4);
    TA(f.uright, S * K * 4);
    TA(f.gcell, S * K * 4);
    TA(f.match, S * K * 4);
    TA(f.outlier, S * K);
    TA(f.has_mp, S * K);
    TA(f.mp_xyz, S * K * 12);
    TA(f.nobs, S * K * 4);
    if (t->map) {
      TA(f.mpid, S * K * 4);
      TA(f.mp_desc, S * K * 32);
      TA(f.mlid, S * kLineKeep * 4);
      TA(f.ml_desc, S * kLineKeep * 32);
    }
    if (t->lines) {
      const size_t L = S * kLineKeep;
      TA(f.kl, L * sizeof(orbpl_keyline));
      TA(f.kl_un, L * sizeof(orbpl_keyline));
      TA(f.ldesc, L * 32);
      TA(f.lcoef, L * 3 * sizeof(double));
      TA(f.nl, S * 4);
      TA(f.dstart, L * 4);
      TA(f.dend, L * 4);
      TA(f.lmatch, L * 4);
      TA(f.loutlier, L);
      TA(f.has_ml, L);
      TA(f.ml_xyz, L * 6 * 4);
    }
  }
  TA(t->d_state, S * sizeof(StreamState));
  if (t->local_map) {
    const size_t R = S * orbpl_tracker::kLmK * K, RL = S * orbpl_tracker::kLmK * kLineKeep;
    t->lp = (long long)orbpl_tracker::kLmK * K;
    t->llp = (long long)orbpl_tracker::kLmK * kLineKeep;
    const size_t LP = S * (size_t)t->lp, LLP = S * (size_t)t->llp;
    TA(t->kr_xyz, R * 12);
    TA(t->kr_nrm, R * 12);
    TA(t->kr_dmin, R * 4);
    TA(t->kr_dmax, R * 4);
    TA(t->kr_has, R);
    TA(t->kr_desc, R * 32);
    TA(t->kr_n, S * orbpl_tracker::kLmK * 4);
    TA(t->l_xyz, LP * 12);
    TA(t->l_nrm, LP * 12);
    TA(t->l_dmin, LP * 4);
    TA(t->l_dmax, LP * 4);
    TA(t->l_desc, LP * 32);
    TA(t->l_n, S * 4);
    TA(t->l_inview, LP);
    TA(t->l_px, LP * 4);
    TA(t->l_py, LP * 4);
    TA(t->l_pxr, LP * 4);
    TA(t->l_vcos, LP * 4);
    TA(t->l_level, LP * 4);
    TA(t->l_scratch, LP * sizeof(int4));
    TA(t->cur_nobs, S * K * 4);
    TA(t->lm_match, S * K * 4);
    TA(t->match2, S * K * 4);
    TA(t->xyz2, S * K * 12);
    TA(t->outlier2, S * K);
    if (t->lines) {
      TA(t->rl_xyz, RL * 24);
      TA(t->rl_has, RL);
      TA(t->rl_desc, RL * 32);
      TA(t->rl_n, S * orbpl_tracker::kLmK * 4);
      TA(t->ll_xyz, LLP * 24);
      TA(t->ll_desc, LLP * 32);
      TA(t->ll_valid, LLP);
      TA(t->ll_n, S * 4);
      TA(t->ll_proj, LLP * sizeof(orbpl_keyline));
      TA(t->ll_src, LLP * 4);
      TA(t->cur_nobs_l, S * kLineKeep * 4);
      TA(t->llm_match, S * kLineKeep * 4);
      TA(t->lmatch2, S * kLineKeep * 4);
      TA(t->lxyz2, S * kLineKeep * 24);
      TA(t->loutlier2, S * kLineKeep);
    }
  }
  TA(t->d_edges, S * kPoseMaxEdges * pose_edge_bytes());
  if (t->refkf) {
    const size_t L = S * kLineKeep;
    TA(t->trk_lcur, L * 4);
    TA(t->trk_nobs, L * 4);
    TA(t->trk_lm, L * 4);
    TA(t->trk_nml, S * 4);
    TA(t->trk_proj, L * sizeof(orbpl_keyline));
    TA(t->trk_src, L * 4);
  }
  if (t->stereo) {
    // a right keypoint at scale s enters ceil(y + 2s) - floor(y - 2s) + 1 <= 4s + 3
    // rows: 20 per keypoint hold every pyramid whose top scale is at most 4.25
    // (8 levels of 1.2: 3.58); a taller one can raise the step's error flag
    t->st_entry_cap = (int)K * 20;
    // test hook: a smaller row-band capacity forces the overflow path
    if (const char* e = getenv("ORBPL_STEREO_ENTRY_CAP")) {
      const int v = atoi(e);
      if (v > 0 && v < t->st_entry_cap) t->st_entry_cap = v;
    }
    TA(t->r_kps, S * K * sizeof(KeyPointD));
    TA(t->r_desc, S * K * 32);
    TA(t->r_n, S * 4);
    TA(t->st_sad, S * K * 4);
    TA(t->st_entries, S * (size_t)t->st_entry_cap * 2);
    TA(t->d_err, 4);
    if (t->lines) {
      const size_t L = S * kLineKeep;
      TA(t->r_kl, L * sizeof(orbpl_keyline));
      TA(t->r_ldesc, L * 32);
      TA(t->r_lcoef, L * 3 * sizeof(double));
      TA(t->r_nl, S * 4);
    }
  }
#undef TA
  if (const char* e = getenv("ORBPL_GLUE_ON_TRACK")) t->glue_on_ts = e[0] != '0';
  if (t->map) {
    int kfc = 32;
    if (const char* e = getenv("ORBPL_MAP_KF")) kfc = atoi(e);
    if (kfc < 2 || kfc > kMapMaxKF) {
      orbpl_tracker_destroy(t);
      return arg_fail("ORBPL_MAP_KF out of [2, 64]");
    }
    rc = map_alloc(t, kfc);
    if (rc) {
      orbpl_tracker_destroy(t);
      return rc;
    }
  }
  t->ring.assign(orbpl_tracker::kRing * orbpl_tracker::kEv, nullptr);
  for (auto& e : t->ring)
    if (hipEventCreate(&e) != hipSuccess) {
      orbpl_tracker_destroy(t);
      return hip_fail(hipErrorUnknown, "hipEventCreate", __LINE__);
    }
  for (auto& e : t->ev_free)
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
      orbpl_tracker_destroy(t);
      return hip_fail(hipErrorUnknown, "hipEventCreate", __LINE__);
    }
  if (hipStreamCreateWithFlags(&t->tstream, hipStreamNonBlocking) != hipSuccess) {
    orbpl_tracker_destroy(t);
    return hip_fail(hipErrorUnknown, "hipStreamCreate", __LINE__);
  }
  if (t->lines) {
    // "0" off, "1" on, else by size when the HIP runtime has the hardware
    // queues for the extra streams (with the default 4, streams share queues
    // and the halves serialise with the ORB stream: measured no gain)
    // (stereo: the left image's batch; the right one has its own stream and
    // context. KITTI leg, 1024 pairs: 4.9k -> 5.2k frames/s)
    const bool split = split_on("ORBPL_LSD_SPLIT", n_streams, kLsdSplitMin);
    t->lsplit = split ? (n_streams + 1) / 2 : 0;
    rc = lsdx_create(cam->width, cam->height, split ? t->lsplit : n_streams, device, &t->lx);
    if (!rc && split) rc = lsdx_create(cam->width, cam->height, n_streams - t->lsplit, device, &t->lx2);
    if (rc) {
      orbpl_tracker_destroy(t);
      return rc;
    }
    if (hipStreamCreateWithFlags(&t->lstream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&t->ev_in, hipEventDisableTiming) != hipSuccess) {
      orbpl_tracker_destroy(t);
      return hip_fail(hipErrorUnknown, "hipStreamCreate", __LINE__);
    }
    if (split && (hipStreamCreateWithFlags(&t->lstream_a, hipStreamNonBlocking) != hipSuccess ||
                  hipStreamCreateWithFlags(&t->lstream_b, hipStreamNonBlocking) != hipSuccess ||
                  hipEventCreateWithFlags(&t->ev_la_sort, hipEventDisableTiming) != hipSuccess ||
                  hipEventCreateWithFlags(&t->ev_la_done, hipEventDisableTiming) != hipSuccess ||
                  hipEventCreateWithFlags(&t->ev_lb_done, hipEventDisableTiming) != hipSuccess)) {
      orbpl_tracker_destroy(t);
      return hip_fail(hipErrorUnknown, "hipStreamCreate", __LINE__);
    }
  }
  if (t->stereo) {
    rc = orbx_create(orb, cam->width, cam->height, n_streams, device, &t->exr);
    if (rc) {
      orbpl_tracker_destroy(t);
      return rc;
    }
    t->rstream = orbpl::orbx_stream(t->exr);
    if (hipEventCreateWithFlags(&t->ev_rin, hipEventDisableTiming) != hipSuccess) {
      orbpl_tracker_destroy(t);
      return hip_fail(hipErrorUnknown, "hipEventCreate", __LINE__);
    }
    if (t->lines) {
      rc = lsdx_create(cam->width, cam->height, n_streams, device, &t->lxr);
      if (rc) {
        orbpl_tracker_destroy(t);
        return rc;
      }
      if (hipStreamCreateWithFlags(&t->rlstream, hipStreamNonBlocking) != hipSuccess ||
          hipEventCreateWithFlags(&t->ev_rlin, hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&t->ev_sl_done, hipEventDisableTiming) != hipSuccess) {
        orbpl_tracker_destroy(t);
        return hip_fail(hipErrorUnknown, "hipStreamCreate", __LINE__);
      }
    }
  }
  rc = orbpl_tracker_reset(t, nullptr);
  if (rc) {
    orbpl_tracker_destroy(t);
    return rc;
  }
  *out = t;
  return ORBPL_OK;
}

int orbpl_tracker_reset(orbpl_tracker* t, const float* Tcw0) {
  if (!t) return arg_fail("NULL tracker");
  HIP_CHECK(hipSetDevice(t->device));
  std::vector<StreamState> st(t->S);
  for (int s = 0; s < t->S; s++) {
    StreamState z{};
    for (int k = 0; k < 16; k++) z.Tcw[k] = Tcw0 ? Tcw0[s * 16 + k] : (k % 5 == 0 ? 1.f : 0.f);
    st[s] = z;
  }
  if (t->cstream) HIP_CHECK(hipStreamSynchronize(t->cstream));
  HIP_CHECK(hipStreamSynchronize(t->stream));
  if (t->tstream) HIP_CHECK(hipStreamSynchronize(t->tstream));
  if (t->lstream) HIP_CHECK(hipStreamSynchronize(t->lstream));
  if (t->rstream) HIP_CHECK(hipStreamSynchronize(t->rstream));
  if (t->rlstream) HIP_CHECK(hipStreamSynchronize(t->rlstream));
  HIP_CHECK(hipMemcpy(t->d_state, st.data(), sizeof(StreamState) * t->S, hipMemcpyHostToDevice));
  if (t->d_err) HIP_CHECK(hipMemset(t->d_err, 0, 4));
  if (t->map) {
    // every stream starts uninitialised; the first frame takes its Tcw0
    float* dT0 = nullptr;
    if (Tcw0) {
      HIP_CHECK(hipMalloc(&dT0, (size_t)t->S * 64));
      HIP_CHECK(hipMemcpy(dT0, Tcw0, (size_t)t->S * 64, hipMemcpyHostToDevice));
    }
    launch_map_reset(t->ma, dT0, t->S, nullptr);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    if (dT0) HIP_CHECK(hipFree(dT0));
  }
  t->hist_count = 0;
  t->lm_step = 0;
  return ORBPL_OK;
}

int orbpl_tracker_set_fps(orbpl_tracker* t, float fps) {
  if (!t) return arg_fail("NULL tracker");
  if (!t->map) return arg_fail("tracker created without ORBPL_TRACK_MAP");
  if (!(fps >= 0.0f) || fps > 1e6f) return arg_fail("orbpl_tracker_set_fps: fps out of range");
  // Tracking::Tracking: if(fps==0) fps=30; mMaxFrames = fps (Tracking.cc:81-87)
  t->ma.max_frames = (int)(fps == 0.0f ? 30.0f : fps);
  return ORBPL_OK;
}

int orbpl_tracker_clear_velocity(orbpl_tracker* t, const uint8_t* mask) {
  if (!t || !mask) return arg_fail("orbpl_tracker_clear_velocity: NULL argument");
  HIP_CHECK(hipSetDevice(t->device));
  if (t->cstream) HIP_CHECK(hipStreamSynchronize(t->cstream));
  HIP_CHECK(hipStreamSynchronize(t->stream));
  if (t->tstream) HIP_CHECK(hipStreamSynchronize(t->tstream));
  HostStage st;
  const uint8_t* d_mask = st.in(mask, t->S, t->S);
  if (st.rc()) return st.rc();
  launch_clear_velocity(t->map ? t->ma.ms : nullptr, t->d_state, d_mask, t->S, nullptr);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipDeviceSynchronize());
  return ORBPL_OK;
}

}  // extern "C"

// Tracking::Track with the map model (ORBPL_TRACK_MAP) on the tracking stream:
// the map kernels (map_kernels.hip) around the batched matchers and k_pose.
// ev: the step's events (brackets as in the P18 path).
static int map_track(orbpl_tracker* t, FrameBufs& C, FrameBufs& L, const LineTrackArgs& la0,
                      hipEvent_t* ev, hipStream_t ts) {
  const int S = t->S, K = t->kp_cap;
  const int pstride = (int)(sizeof(StreamState) / sizeof(float));
  char* stb = reinterpret_cast<char*>(t->d_state);
  float* dTcw = reinterpret_cast<float*>(stb + offsetof(StreamState, Tcw));
  float* dTlast = reinterpret_cast<float*>(stb + offsetof(StreamState, Tlast));
  auto field = [&](size_t off) { return reinterpret_cast<int*>(stb + off); };
  MapArgs a = t->ma;
  a.st = t->d_state;
  a.lines = t->lines;
  a.refkf = t->refkf;
  a.vocab = t->voc ? 1 : 0;
  a.n = C.n; a.kps_un = C.kps_un; a.depth = C.depth; a.uright = C.uright; a.desc = C.desc;
  a.feat_node = C.feat_node; a.match = C.match; a.outlier = C.outlier; a.mpid = C.mpid;
  a.nl = C.nl; a.kl_un = C.kl_un; a.dstart = C.dstart; a.dend = C.dend; a.ldesc = C.ldesc;
  a.lmatch = C.lmatch; a.loutlier = C.loutlier; a.mlid = C.mlid;
  a.l_n = L.n; a.l_kps_un = L.kps_un; a.l_depth = L.depth; a.l_desc = L.desc; a.l_mpid = L.mpid;
  a.l_has_mp = L.has_mp; a.l_mp_xyz = L.mp_xyz; a.l_mp_desc = L.mp_desc; a.l_nobs = L.nobs;
  a.l_nl = L.nl; a.l_kl_un = L.kl_un; a.l_dstart = L.dstart; a.l_dend = L.dend; a.l_ldesc = L.ldesc;
  a.l_mlid = L.mlid; a.l_has_ml = L.has_ml; a.l_ml_xyz = L.ml_xyz; a.l_ml_desc = L.ml_desc;
  const MapExtra& x = t->mx;
  // ---- frame id, path, UpdateLastFrame, the constant-velocity prediction ----
  launch_map_begin(t->consts, a, S, ts);
  // ---- TrackWithMotionModel (Tracking.cc:1212-1330) ----
  MatchLaunch m{};
  m.cur_kps_un = C.kps_un;
  m.cur_desc = C.desc;
  m.cur_uright = C.uright;
  m.cur_gcell = C.gcell;
  m.cur_n = C.n;
  m.last_kps_un = L.kps_un;
  m.last_has_mp = L.has_mp;
  m.last_outlier = L.outlier;
  m.last_xyz = L.mp_xyz;
  m.last_desc = L.mp_desc;     // pMP->GetDescriptor()
  m.last_nobs = L.nobs;
  m.last_n = L.n;
  m.kp_pitch = K;
  m.Tcw = dTcw;
  m.Tlw = dTlast;
  m.pose_stride = pstride;
  m.match = C.match;
  m.nmatches = field(offsetof(StreamState, nmatches));
  m.nm_stride = pstride;
  m.th = t->stereo ? 7.0f : 15.0f;   // Tracking.cc:1238-1241
  m.mono = 0;
  m.check_ori = 1;
  m.retry = 1;
  m.active = t->d_state;
  launch_match_last(t->consts, m, S, ts);
  HIP_CHECK(hipEventRecord(ev[8], ts));
  if (t->lines) {
    LineTrackArgs la = la0;
    la.last_desc = L.ml_desc;  // the map lines' descriptors
    launch_line_match(t->consts, la, t->d_state, S, ts);
  }
  HIP_CHECK(hipEventRecord(ev[14], ts));
  PoseLaunch p{};
  p.kps_un = C.kps_un;
  p.uright = C.uright;
  p.match = C.match;
  p.mp_xyz = L.mp_xyz;
  p.n = C.n;
  p.kp_pitch = K;
  p.Tcw = dTcw;
  p.pose_stride = pstride;
  p.outlier = C.outlier;
  p.ninliers = field(offsetof(StreamState, ninliers));
  p.nm_stride = pstride;
  p.active = t->d_state;
  p.edges = t->d_edges;
  if (t->lines) {
    p.t_kl_un = C.kl_un;
    p.t_lmatch = C.lmatch;
    p.t_ml_xyz = L.ml_xyz;
    p.t_nl = C.nl;
    p.t_loutlier = C.loutlier;
    p.lpitch = kLineKeep;
  }
  p.fixed_line_jac = t->fixed_line_jac;
  HIP_CHECK(hipEventRecord(ev[28], ts));
  launch_pose(t->consts, p, S, ts);
  HIP_CHECK(hipEventRecord(ev[29], ts));
  launch_map_resolve_motion(a, S, ts);
  // the later poses read the frame's map elements in its own index space
  PoseLaunch pm = p;
  pm.match = a.m2;
  pm.mp_xyz = a.pxyz;
  if (t->lines) {
    pm.t_lmatch = a.lm2;
    pm.t_ml_xyz = a.lpxyz;
  }
  HIP_CHECK(hipEventRecord(ev[30], ts));
  if (t->refkf) {
    // ---- TrackReferenceKeyFrame (Tracking.cc:942-1032) ----
    TrkArgs ta{};
    ta.st = t->d_state;
    ta.kp_pitch = K;
    ta.lines = t->lines;
    ta.n = C.n;
    ta.match = C.match;
    ta.kps_un = C.kps_un;
    ta.desc = C.desc;
    ta.feat_node = C.feat_node;
    ta.last_n = a.r_n;
    ta.last_kps_un = a.r_kps_un;
    ta.last_desc = a.r_desc;
    ta.last_has_mp = a.r_has_mp;
    ta.last_feat_node = a.r_node;
    ta.list = a.trk_list;      // only the streams k_map_resolve_motion listed
    ta.list_n = a.trk_count;
    launch_trk_bow(ta, S, ts);
    if (t->lines) {
      LineListArgs lr{};
      lr.Tcw = dTcw;
      lr.cur_kl_un = C.kl_un;
      lr.cur_desc = C.ldesc;
      lr.cur_nobs = a.trk_cur_nobs;
      lr.valid = a.r_has_ml;
      lr.ml_xyz6 = a.r_ml_xyz;
      lr.ml_desc = a.r_ml_desc;
      lr.proj_kl = x.trk_proj;
      lr.proj_src = x.trk_src;
      lr.match = a.trk_lm;
      lr.nmatches = field(offsetof(StreamState, trk_nlm));
      lr.wiped = field(offsetof(StreamState, trk_wiped));
      lr.refkf = 1;
      lr.ncur_arr = C.nl;
      lr.nml_arr = a.trk_nml;
      lr.cur_pitch = kLineKeep;
      lr.ml_pitch = kLineKeep;
      lr.pose_stride = pstride;
      lr.nm_stride = pstride;
      lr.list = a.trk_list;
      lr.list_n = a.trk_count;
      launch_line_match_list(t->consts, lr, ts, S);
    }
    launch_map_trk_merge(a, S, ts);
    PoseLaunch pt = pm;
    pt.gate_lm = 2;
    pt.list = a.trk_list;
    pt.list_n = a.trk_count;
    launch_pose(t->consts, pt, S, ts);
  }
  HIP_CHECK(hipEventRecord(ev[31], ts));
  launch_map_resolve_trk(a, S, ts);
  HIP_CHECK(hipEventRecord(ev[9], ts));
  // ---- TrackLocalMap (Tracking.cc:1332-1420) ----
  launch_map_local(a, S, ts);
  InFrustumArgs fa{};
  fa.Tcw = dTcw;
  fa.xyz = a.l_xyz;
  fa.normal = a.l_nrm;
  fa.min_dist = a.l_dmin;
  fa.max_dist = a.l_dmax;
  fa.view_cos_limit = 0.5f;
  fa.in_view = x.l_inview;
  fa.proj_x = x.l_px;
  fa.proj_y = x.l_py;
  fa.proj_xr = x.l_pxr;
  fa.level = x.l_level;
  fa.view_cos = x.l_vcos;
  fa.n_arr = a.l_count;
  fa.pitch = a.lp;
  fa.pose_stride = pstride;
  const float log_scale = log_scale_of(t->scale_factor);
  launch_in_frustum(t->consts, log_scale, fa, ts, S);
  LocalArgs ml{};
  ml.kps_un = C.kps_un;
  ml.desc = C.desc;
  ml.uright = C.uright;
  ml.cur_nobs = a.cur_nobs;
  ml.in_view = x.l_inview;
  ml.proj_x = x.l_px;
  ml.proj_y = x.l_py;
  ml.proj_xr = x.l_pxr;
  ml.level = x.l_level;
  ml.view_cos = x.l_vcos;
  ml.mp_desc = a.l_ldesc_pts;
  ml.mp_nobs = nullptr;        // every local map point is observed
  // RGB-D 3, stereo 1; 5 within mnLastRelocFrameId + 2 (Tracking.cc:1801-1809)
  ml.th = t->lm_step < 2 ? 5.0f : (t->stereo ? 1.0f : 3.0f);
  ml.nnratio = 0.8f;
  ml.match = const_cast<int*>(a.lm_match);
  ml.nmatches = field(offsetof(StreamState, lm_nlocal));
  ml.scratch = x.l_scratch;
  ml.n_arr = C.n;
  ml.nmp_arr = a.l_count;
  ml.kp_pitch = K;
  ml.mp_pitch = a.lp;
  ml.nm_stride = pstride;
  HIP_CHECK(hipEventRecord(ev[32], ts));
  launch_match_local(t->consts, ml, ts, S);
  HIP_CHECK(hipEventRecord(ev[33], ts));
  if (t->lines) {
    launch_line_in_frustum_batched(dTcw, pstride, a.ll_count, a.llp, a.ll_xyz, x.ll_valid, S, ts);
    LineListArgs l3{};
    l3.Tcw = dTcw;
    l3.cur_kl_un = C.kl_un;
    l3.cur_desc = C.ldesc;
    l3.cur_nobs = a.cur_nobs_l;
    l3.valid = x.ll_valid;
    l3.ml_xyz6 = a.ll_xyz;
    l3.ml_desc = a.ll_desc;
    l3.proj_kl = x.ll_proj;
    l3.proj_src = x.ll_src;
    l3.match = const_cast<int*>(a.llm_match);
    l3.nmatches = field(offsetof(StreamState, lm_nllocal));
    l3.wiped = field(offsetof(StreamState, lm_wiped));
    l3.ncur_arr = C.nl;
    l3.nml_arr = a.ll_count;
    l3.cur_pitch = kLineKeep;
    l3.ml_pitch = a.llp;
    l3.pose_stride = pstride;
    l3.nm_stride = pstride;
    launch_line_match_list(t->consts, l3, ts, S);
  }
  launch_map_assemble(a, S, ts);
  PoseLaunch p2 = pm;
  p2.ninliers = field(offsetof(StreamState, lm_ninl));
  p2.gate_lm = 1;
  HIP_CHECK(hipEventRecord(ev[34], ts));
  launch_pose(t->consts, p2, S, ts);
  HIP_CHECK(hipEventRecord(ev[35], ts));
  HIP_CHECK(hipEventRecord(ev[26], ts));
  // ---- decision, keyframe insertion, ProcessNewKeyFrame, relative pose ----
  launch_map_finish(t->consts, a, S, ts);
  t->lm_step++;
  return ORBPL_OK;
}

// One TrackWithMotionModel step for every stream: RGB-D (d_depth) or stereo
// (d_right, ORBPL_TRACK_STEREO trackers).
static int tracker_step(orbpl_tracker* t, const uint8_t* d_gray, const float* d_depth,
                        const uint8_t* d_right) {
  if (t->refkf && !t->voc)
    return arg_fail("ORBPL_TRACK_REFKF tracker: orbpl_tracker_set_vocabulary first");
  HIP_CHECK(hipSetDevice(t->device));
  const int ci = t->ring_pos % 3, li = (t->ring_pos + 2) % 3;
  FrameBufs& C = t->fb[ci];
  FrameBufs& L = t->fb[li];
  const int S = t->S, K = t->kp_cap;
  hipStream_t s = t->stream, ts = t->pipelined ? t->tstream : t->stream;
  const int pstride = (int)(sizeof(StreamState) / sizeof(float));
  char* st0 = reinterpret_cast<char*>(t->d_state);
  float* dTcw = reinterpret_cast<float*>(st0 + offsetof(StreamState, Tcw));
  float* dTlast = reinterpret_cast<float*>(st0 + offsetof(StreamState, Tlast));
  int* dNm = reinterpret_cast<int*>(st0 + offsetof(StreamState, nmatches));
  int* dNin = reinterpret_cast<int*>(st0 + offsetof(StreamState, ninliers));
  hipEvent_t* ev = &t->ring[(size_t)(t->ring_pos % orbpl_tracker::kRing) * orbpl_tracker::kEv];
  // ---- extraction stream: wait until tracking of step t-1 released fb[ci]
  if (t->free_pending[ci]) HIP_CHECK(hipStreamWaitEvent(s, t->ev_free[ci], 0));
  if (t->stereo) {
    // ---- right stream: ORB on the right images (Frame.cc:88-91). Ordered
    // after the previous step's stereo matching, which read r_kps and the
    // right pyramid on `s`.
    HIP_CHECK(hipEventRecord(t->ev_rin, s));
    HIP_CHECK(hipStreamWaitEvent(t->rstream, t->ev_rin, 0));
    HIP_CHECK(hipEventRecord(ev[15], t->rstream));
    int rrc = orbx_run(t->exr, d_right, S, t->W, (long long)t->W * t->H,
                       reinterpret_cast<orbpl_keypoint_dev*>(t->r_kps), t->r_desc, K, t->r_n);
    if (rrc) return rrc;
    HIP_CHECK(hipEventRecord(ev[16], t->rstream));
  }
  if (t->lines && t->stereo) {
    // ---- right line stream: LineExtractor on the right images (P17), after
    // the previous step's k_stereo_lines has read the right KeyLines
    HIP_CHECK(hipEventRecord(t->ev_rlin, s));
    HIP_CHECK(hipStreamWaitEvent(t->rlstream, t->ev_rlin, 0));
    HIP_CHECK(hipStreamWaitEvent(t->rlstream, t->ev_sl_done, 0));
    HIP_CHECK(hipEventRecord(ev[23], t->rlstream));
    LineOut ro{};
    ro.kl = t->r_kl;
    ro.desc = t->r_ldesc;
    ro.coef = t->r_lcoef;
    ro.n = t->r_nl;
    int lrc = lsdx_run(t->lxr, d_right, S, t->W, (int64_t)t->W * t->H, &ro, t->rlstream, nullptr);
    if (lrc) return lrc;
    HIP_CHECK(hipEventRecord(ev[24], t->rlstream));
  }
  LineTrackArgs la{};
  if (t->lines) {
    // ---- line stream: LineExtractor + UndistortKeyLines + line depths
    HIP_CHECK(hipEventRecord(t->ev_in, s));
    LineOut lo{};
    lo.kl = C.kl;
    lo.desc = C.ldesc;
    lo.coef = C.lcoef;
    lo.n = C.nl;
    if (t->lsplit) {
      // first half on lstream_a (its stage events are the step's LSD
      // timings), the second on lstream_b once the first half is sorted
      const int S1 = t->lsplit, S2 = S - S1;
      const int64_t fp = (int64_t)t->W * t->H;
      HIP_CHECK(hipStreamWaitEvent(t->lstream_a, t->ev_in, 0));
      HIP_CHECK(hipEventRecord(ev[11], t->lstream_a));
      int lrc = lsdx_run(t->lx, d_gray, S1, t->W, fp, &lo, t->lstream_a, ev[12], &ev[18]);
      if (lrc) return lrc;
      HIP_CHECK(hipEventRecord(t->ev_la_done, t->lstream_a));
      // the second half starts once the first half is sorted (ev_stage[1]);
      // ORBPL_LSD_STAGGER=0 / 2: at the step start / after its seed loop (A/B)
      static const char* stg = getenv("ORBPL_LSD_STAGGER");
      const int stagger = stg ? atoi(stg) : 1;
      HIP_CHECK(hipStreamWaitEvent(t->lstream_b, stagger == 0 ? t->ev_in : ev[stagger == 2 ? 20 : 19], 0));
      LineOut lo2 = lo;
      lo2.kl = C.kl + (size_t)S1 * kLineKeep;
      lo2.desc = C.ldesc + (size_t)S1 * kLineKeep * 32;
      lo2.coef = C.lcoef + (size_t)S1 * kLineKeep * 3;
      lo2.n = C.nl + S1;
      lrc = lsdx_run(t->lx2, d_gray + (size_t)S1 * fp, S2, t->W, fp, &lo2, t->lstream_b, nullptr);
      if (lrc) return lrc;
      HIP_CHECK(hipEventRecord(t->ev_lb_done, t->lstream_b));
      HIP_CHECK(hipStreamWaitEvent(t->lstream, t->ev_la_done, 0));
      HIP_CHECK(hipStreamWaitEvent(t->lstream, t->ev_lb_done, 0));
    } else {
      HIP_CHECK(hipStreamWaitEvent(t->lstream, t->ev_in, 0));
      HIP_CHECK(hipEventRecord(ev[11], t->lstream));
      int lrc = lsdx_run(t->lx, d_gray, S, t->W, (int64_t)t->W * t->H, &lo, t->lstream, ev[12],
                         &ev[18]);
      if (lrc) return lrc;
    }
    la.nl = C.nl;
    la.kl = C.kl;
    la.kl_un = C.kl_un;
    la.depth = d_depth;
    la.depth_pitch = (long long)t->W * t->H;
    la.dstart = C.dstart;
    la.dend = C.dend;
    la.lmatch = C.lmatch;
    la.loutlier = C.loutlier;
    la.desc = C.ldesc;
    la.last_nl = L.nl;
    la.last_kl_un = L.kl_un;
    la.last_has_ml = L.has_ml;
    la.last_loutlier = L.loutlier;
    la.last_ml_xyz = L.ml_xyz;
    la.last_desc = L.ldesc;
    launch_line_prepare(t->consts, la, S, t->lstream);
    if (t->stereo) {
      // end-point depths from the right image's lines (P17)
      HIP_CHECK(hipStreamWaitEvent(t->lstream, ev[24], 0));
      HIP_CHECK(hipEventRecord(ev[25], t->lstream));
      StereoLineArgs sa{C.nl, C.kl_un, C.ldesc, t->r_nl, t->r_kl, t->r_ldesc, C.dstart, C.dend};
      launch_stereo_lines(t->consts, sa, S, t->lstream);
      HIP_CHECK(hipEventRecord(t->ev_sl_done, t->lstream));
    }
    HIP_CHECK(hipEventRecord(ev[13], t->lstream));
  }
  int rc;
  if (t->osplit) {
    // first half on `s` (its stage events are the step's extraction
    // timings), the second on stream2 after the first half's pyramid
    const int S1 = t->osplit, S2 = S - S1;
    const long long fp = (long long)t->W * t->H;
    rc = orbx_run(t->ex, d_gray, S1, t->W, fp, reinterpret_cast<orbpl_keypoint_dev*>(C.kps),
                  C.desc, K, C.n, ev, ev + 36);
    if (rc) return rc;
    HIP_CHECK(hipStreamWaitEvent(t->stream2, ev[1], 0));
    rc = orbx_run(t->ex2, d_gray + (size_t)S1 * fp, S2, t->W, fp,
                  reinterpret_cast<orbpl_keypoint_dev*>(C.kps + (size_t)S1 * K),
                  C.desc + (size_t)S1 * K * 32, K, C.n + S1, nullptr);
    if (rc) return rc;
    HIP_CHECK(hipEventRecord(t->ev_ob_done, t->stream2));
    HIP_CHECK(hipStreamWaitEvent(s, t->ev_ob_done, 0));
  } else {
    rc = orbx_run(t->ex, d_gray, S, t->W, (long long)t->W * t->H,
                  reinterpret_cast<orbpl_keypoint_dev*>(C.kps), C.desc, K, C.n, ev, ev + 36);
    if (rc) return rc;
  }
  // The frame glue and KeyFrame::ComputeBoW read only this step's frame
  // buffers (and the depth input), so a pipelined RGB-D tracker can run them
  // at the head of the tracking stream (ORBPL_GLUE_ON_TRACK=1): the next
  // step's extraction on `s` then follows this step's orientation launch
  // directly. Measured 1-3 % slower at 2048 streams (the tracking chain
  // becomes the longer one; profiles/r06/ab/glue_on_track_ab.txt), so off by
  // default. Stereo keeps them on `s` regardless: ComputeStereoMatches reads
  // the extractors' device pyramids, which the next extraction overwrites.
  hipStream_t gs = s;
  if (t->glue_on_ts && ts != s && !t->stereo) {
    gs = ts;
    HIP_CHECK(hipEventRecord(ev[orbpl_tracker::kEvXdone], s));
    HIP_CHECK(hipStreamWaitEvent(ts, ev[orbpl_tracker::kEvXdone], 0));
  }
  HIP_CHECK(hipEventRecord(ev[orbpl_tracker::kEvGlue], gs));
  launch_frame_prepare(t->consts, C.kps, C.n, K, t->stereo ? nullptr : d_depth,
                       (long long)t->W * t->H, C.kps_un, C.depth, C.uright, C.gcell, S, gs);
  if (t->stereo) {
    // ComputeStereoMatches (Frame.cc:886-1063) for the whole batch
    HIP_CHECK(hipStreamWaitEvent(s, ev[16], 0));
    HIP_CHECK(hipEventRecord(ev[17], s));
    const uint8_t *pl = nullptr, *pr = nullptr;
    const OrbGeom *gl = nullptr, *gr = nullptr;
    hipStream_t sl, sr;
    int prc = orbx_device_pyramid(t->ex, 0, &pl, &gl, &sl);
    if (!prc) prc = orbx_device_pyramid(t->exr, 0, &pr, &gr, &sr);
    if (prc) return prc;
    StereoArgs a{};
    a.n_arr = C.n;
    a.nr_arr = t->r_n;
    a.kp_pitch = K;
    a.pyr_pitch = (long long)gl->pyr_bytes;
    a.kl = C.kps;
    a.dl = C.desc;
    a.kr = t->r_kps;
    a.dr = t->r_desc;
    a.pyrL = pl;
    a.pyrR = pr;
    stereo_set_levels(a, *gl);
    a.mb = t->consts.mb;
    a.mbf = t->consts.bf;
    a.uright = C.uright;
    a.depth = C.depth;
    a.sad = t->st_sad;
    a.entries = t->st_entries;
    a.entry_cap = t->st_entry_cap;
    a.err = t->d_err;
    launch_stereo(a, S, s);
  }
  HIP_CHECK(hipEventRecord(ev[27], gs));
  if (t->voc) {
    // every tracked frame is a keyframe (P18): KeyFrame::ComputeBoW
    // (KeyFrame.cc:67, Frame.cc:730) after the glue
    rc = orbv_transform_batch_device(t->voc, C.desc, K, C.n, S, K, t->voc_levelsup, C.feat_node,
                                     C.feat_word, C.feat_weight, C.bow_words, C.bow_vals, C.bow_n,
                                     K, t->d_bow_err, (void*)gs);
    if (rc) return rc;
  }
  HIP_CHECK(hipEventRecord(ev[6], gs));
  // ---- tracking stream
  HIP_CHECK(hipStreamWaitEvent(ts, ev[6], 0));
  if (t->lines) HIP_CHECK(hipStreamWaitEvent(ts, ev[13], 0));
  HIP_CHECK(hipEventRecord(ev[7], ts));
  if (t->map) {
    const int mrc = map_track(t, C, L, la, ev, ts);
    if (mrc) return mrc;
  } else {
  launch_predict(t->d_state, S, ts);
  MatchLaunch m{};
  m.cur_kps_un = C.kps_un;
  m.cur_desc = C.desc;
  m.cur_uright = C.uright;
  m.cur_gcell = C.gcell;
  m.cur_n = C.n;
  m.last_kps_un = L.kps_un;
  m.last_has_mp = L.has_mp;
  m.last_outlier = L.outlier;
  m.last_xyz = L.mp_xyz;
  m.last_desc = L.desc;
  m.last_nobs = L.nobs;
  m.last_n = L.n;
  m.kp_pitch = K;
  m.Tcw = dTcw;
  m.Tlw = dTlast;
  m.pose_stride = pstride;
  m.match = C.match;
  m.nmatches = dNm;
  m.nm_stride = pstride;
  m.th = t->stereo ? 7.0f : 15.0f;   // Tracking.cc:1238-1241
  m.mono = 0;
  m.check_ori = 1;       // ORBmatcher(0.9, true) (Tracking.cc:1216)
  m.retry = 1;
  m.active = t->d_state;
  launch_match_last(t->consts, m, S, ts);
  HIP_CHECK(hipEventRecord(ev[8], ts));
  if (t->lines) launch_line_match(t->consts, la, t->d_state, S, ts);
  HIP_CHECK(hipEventRecord(ev[14], ts));
  PoseLaunch p{};
  p.kps_un = C.kps_un;
  p.uright = C.uright;
  p.match = C.match;
  p.has_mp = nullptr;
  p.mp_xyz = L.mp_xyz;
  p.n = C.n;
  p.kp_pitch = K;
  p.nl = 0;
  p.Tcw = dTcw;
  p.pose_stride = pstride;
  p.outlier = C.outlier;
  p.line_outlier = nullptr;
  p.ninliers = dNin;
  p.nm_stride = pstride;
  p.active = t->d_state;
  p.edges = t->d_edges;
  if (t->lines) {
    p.t_kl_un = C.kl_un;
    p.t_lmatch = C.lmatch;
    p.t_ml_xyz = L.ml_xyz;
    p.t_nl = C.nl;
    p.t_loutlier = C.loutlier;
    p.lpitch = kLineKeep;
  }
  p.fixed_line_jac = t->fixed_line_jac;
  HIP_CHECK(hipEventRecord(ev[28], ts));
  launch_pose(t->consts, p, S, ts);
  HIP_CHECK(hipEventRecord(ev[29], ts));
  HIP_CHECK(hipEventRecord(ev[30], ts));   // k_pose of TrackReferenceKeyFrame (0 without)
  bool refkf_pose = false;
  if (t->refkf) {
    // ---- TrackReferenceKeyFrame where the motion model did not run or
    // failed (Tracking.cc:324-338, 942-1032; P22) ----
    TrkArgs ta{};
    ta.st = t->d_state;
    ta.kp_pitch = K;
    ta.lines = t->lines;
    ta.n = C.n;
    ta.match = C.match;
    ta.outlier = C.outlier;
    ta.nl = C.nl;
    ta.lmatch = C.lmatch;
    ta.loutlier = C.loutlier;
    ta.kps_un = C.kps_un;
    ta.desc = C.desc;
    ta.feat_node = C.feat_node;
    ta.last_n = L.n;
    ta.last_nl = L.nl;
    ta.last_kps_un = L.kps_un;
    ta.last_desc = L.desc;
    ta.last_has_mp = L.has_mp;
    ta.last_feat_node = L.feat_node;
    ta.lcur = t->trk_lcur;
    ta.cur_nobs_l = t->trk_nobs;
    ta.tlm = t->trk_lm;
    ta.nml = t->trk_nml;
    launch_trk_prep(ta, S, ts);
    launch_trk_bow(ta, S, ts);
    if (t->lines) {
      // LineMatcher(0.7, true).SearchByProjection(mCurrentFrame, mpReferenceKF)
      char* stb = reinterpret_cast<char*>(t->d_state);
      LineListArgs lr{};
      lr.Tcw = dTcw;
      lr.cur_kl_un = C.kl_un;
      lr.cur_desc = C.ldesc;
      lr.cur_nobs = t->trk_nobs;
      lr.valid = L.has_ml;      // mvpMapLines[i] != NULL
      lr.ml_xyz6 = L.ml_xyz;
      lr.ml_desc = L.ldesc;
      lr.proj_kl = t->trk_proj;
      lr.proj_src = t->trk_src;
      lr.match = t->trk_lm;
      lr.nmatches = reinterpret_cast<int*>(stb + offsetof(StreamState, trk_nlm));
      lr.wiped = reinterpret_cast<int*>(stb + offsetof(StreamState, trk_wiped));
      lr.refkf = 1;
      lr.ncur_arr = C.nl;
      lr.nml_arr = t->trk_nml;
      lr.cur_pitch = kLineKeep;
      lr.ml_pitch = kLineKeep;
      lr.pose_stride = pstride;
      lr.nm_stride = pstride;
      launch_line_match_list(t->consts, lr, ts, S);
    }
    launch_trk_merge(ta, S, ts);
    PoseLaunch pt = p;
    pt.gate_lm = 2;
    HIP_CHECK(hipEventRecord(ev[30], ts));
    launch_pose(t->consts, pt, S, ts);
    HIP_CHECK(hipEventRecord(ev[31], ts));
    refkf_pose = true;
  }
  if (!refkf_pose) HIP_CHECK(hipEventRecord(ev[31], ts));
  HIP_CHECK(hipEventRecord(ev[9], ts));
  // TrackLocalMap's k_match_local / k_pose brackets (0 without it)
  HIP_CHECK(hipEventRecord(ev[32], ts));
  HIP_CHECK(hipEventRecord(ev[34], ts));
  LocalMapArgs lm{};
  if (t->local_map) {
    // ---- TrackLocalMap (Tracking.cc:1332-1420), defined local map P18 ----
    const int K4 = orbpl_tracker::kLmK, fid = t->lm_step;
    lm.st = t->d_state;
    lm.kp_pitch = K;
    lm.lines = t->lines;
    lm.n = C.n;
    lm.match = C.match;
    lm.outlier = C.outlier;
    lm.nl = C.nl;
    lm.lmatch = C.lmatch;
    lm.loutlier = C.loutlier;
    lm.kps_un = C.kps_un;
    lm.desc = C.desc;
    lm.ldesc = C.ldesc;
    lm.has_mp = C.has_mp;
    lm.mp_xyz = C.mp_xyz;
    lm.has_ml = C.has_ml;
    lm.ml_xyz = C.ml_xyz;
    lm.last_xyz = L.mp_xyz;
    lm.last_lxyz = L.ml_xyz;
    lm.K = K4;
    lm.nslots = std::min(fid, K4);
    lm.head = ((fid - 1) % K4 + K4) % K4;
    lm.push_slot = fid % K4;
    lm.r_xyz = t->kr_xyz; lm.r_nrm = t->kr_nrm; lm.r_dmin = t->kr_dmin; lm.r_dmax = t->kr_dmax;
    lm.r_has = t->kr_has; lm.r_desc = t->kr_desc; lm.r_n = t->kr_n;
    lm.rl_xyz = t->rl_xyz; lm.rl_has = t->rl_has; lm.rl_desc = t->rl_desc; lm.rl_n = t->rl_n;
    lm.lp = t->lp;
    lm.llp = t->llp;
    lm.l_xyz = t->l_xyz; lm.l_nrm = t->l_nrm; lm.l_dmin = t->l_dmin; lm.l_dmax = t->l_dmax;
    lm.l_desc = t->l_desc; lm.l_n = t->l_n;
    lm.ll_xyz = t->ll_xyz; lm.ll_desc = t->ll_desc; lm.ll_n = t->ll_n;
    lm.cur_nobs = t->cur_nobs;
    lm.cur_nobs_l = t->cur_nobs_l;
    lm.lm_match = t->lm_match;
    lm.llm_match = t->llm_match;
    lm.match2 = t->match2; lm.xyz2 = t->xyz2; lm.lmatch2 = t->lmatch2; lm.lxyz2 = t->lxyz2;
    lm.outlier2 = t->outlier2; lm.loutlier2 = t->loutlier2;
    launch_lm_gather(lm, S, ts);
    // SearchLocalPoints: IsInFrustum(pMP, 0.5), ORBmatcher(0.8).SearchByProjection
    InFrustumArgs fa{};
    fa.Tcw = dTcw;
    fa.xyz = t->l_xyz;
    fa.normal = t->l_nrm;
    fa.min_dist = t->l_dmin;
    fa.max_dist = t->l_dmax;
    fa.view_cos_limit = 0.5f;
    fa.in_view = t->l_inview;
    fa.proj_x = t->l_px;
    fa.proj_y = t->l_py;
    fa.proj_xr = t->l_pxr;
    fa.level = t->l_level;
    fa.view_cos = t->l_vcos;
    fa.n_arr = t->l_n;
    fa.pitch = t->lp;
    fa.pose_stride = pstride;
    const float log_scale = log_scale_of(t->scale_factor);
    launch_in_frustum(t->consts, log_scale, fa, ts, S);
    char* stb = reinterpret_cast<char*>(t->d_state);
    LocalArgs ma{};
    ma.kps_un = C.kps_un;
    ma.desc = C.desc;
    ma.uright = C.uright;
    ma.cur_nobs = t->cur_nobs;
    ma.in_view = t->l_inview;
    ma.proj_x = t->l_px;
    ma.proj_y = t->l_py;
    ma.proj_xr = t->l_pxr;
    ma.level = t->l_level;
    ma.view_cos = t->l_vcos;
    ma.mp_desc = t->l_desc;
    ma.mp_nobs = nullptr;
    ma.th = fid < 2 ? 5.0f : (t->stereo ? 1.0f : 3.0f);
    ma.nnratio = 0.8f;
    ma.match = t->lm_match;
    ma.nmatches = reinterpret_cast<int*>(stb + offsetof(StreamState, lm_nlocal));
    ma.scratch = t->l_scratch;
    ma.n_arr = C.n;
    ma.nmp_arr = t->l_n;
    ma.kp_pitch = K;
    ma.mp_pitch = t->lp;
    ma.nm_stride = pstride;
    HIP_CHECK(hipEventRecord(ev[32], ts));
    launch_match_local(t->consts, ma, ts, S);
    HIP_CHECK(hipEventRecord(ev[33], ts));
    if (t->lines) {
      // SearchLocalLines: IsInFrustum(pML, 0.5), LineMatcher(0.8) local-map overload
      launch_line_in_frustum_batched(dTcw, pstride, t->ll_n, t->llp, t->ll_xyz, t->ll_valid, S, ts);
      LineListArgs la3{};
      la3.Tcw = dTcw;
      la3.cur_kl_un = C.kl_un;
      la3.cur_desc = C.ldesc;
      la3.cur_nobs = t->cur_nobs_l;
      la3.valid = t->ll_valid;
      la3.ml_xyz6 = t->ll_xyz;
      la3.ml_desc = t->ll_desc;
      la3.proj_kl = t->ll_proj;
      la3.proj_src = t->ll_src;
      la3.match = t->llm_match;
      la3.nmatches = reinterpret_cast<int*>(stb + offsetof(StreamState, lm_nllocal));
      la3.wiped = reinterpret_cast<int*>(stb + offsetof(StreamState, lm_wiped));
      la3.ncur_arr = C.nl;
      la3.nml_arr = t->ll_n;
      la3.cur_pitch = kLineKeep;
      la3.ml_pitch = t->llp;
      la3.pose_stride = pstride;
      la3.nm_stride = pstride;
      launch_line_match_list(t->consts, la3, ts, S);
    }
    launch_lm_assemble(lm, S, ts);
    // PoseOptimizationWithLines over every match of the frame
    PoseLaunch p2 = p;
    p2.match = t->match2;
    p2.mp_xyz = t->xyz2;
    p2.outlier = t->outlier2;
    p2.ninliers = reinterpret_cast<int*>(stb + offsetof(StreamState, lm_ninl));
    if (t->lines) {
      p2.t_lmatch = t->lmatch2;
      p2.t_ml_xyz = t->lxyz2;
      p2.t_loutlier = t->loutlier2;
    }
    p2.gate_lm = 1;
    HIP_CHECK(hipEventRecord(ev[34], ts));
    launch_pose(t->consts, p2, S, ts);
    HIP_CHECK(hipEventRecord(ev[35], ts));
    launch_lm_count(lm, fid, S, ts);
  }
  if (!t->local_map) {
    HIP_CHECK(hipEventRecord(ev[33], ts));
    HIP_CHECK(hipEventRecord(ev[35], ts));
  }
  HIP_CHECK(hipEventRecord(ev[26], ts));
  LineFinish lf{};
  if (t->lines) {
    lf.nl = C.nl;
    lf.lmatch = C.lmatch;
    lf.loutlier = C.loutlier;
    lf.dstart = C.dstart;
    lf.dend = C.dend;
    lf.kl_un = C.kl_un;
    lf.has_ml = C.has_ml;
    lf.ml_xyz = C.ml_xyz;
  }
  launch_finish(t->consts, t->d_state, C.n, K, C.kps_un, C.depth, C.match, C.outlier, C.has_mp,
                C.mp_xyz, C.nobs, lf, S, ts, t->local_map);
  if (t->local_map) {
    launch_lm_push(t->consts, lm, S, ts);   // the frame joins the local map
    t->lm_step++;
  }
  }   // !t->map
  HIP_CHECK(hipEventRecord(ev[10], ts));
  if (t->hist_count < t->hist_cap) {
    const size_t k = (size_t)t->hist_count++ * S;
    HIP_CHECK(hipMemcpyAsync(t->d_hist_state + k, t->d_state, sizeof(StreamState) * S,
                             hipMemcpyDeviceToDevice, ts));
    HIP_CHECK(hipMemcpyAsync(t->d_hist_n + k, C.n, 4 * (size_t)S, hipMemcpyDeviceToDevice, ts));
    if (t->lines)
      HIP_CHECK(hipMemcpyAsync(t->d_hist_nl + k, C.nl, 4 * (size_t)S, hipMemcpyDeviceToDevice, ts));
  }
  HIP_CHECK(hipEventRecord(t->ev_free[li], ts));
  t->free_pending[li] = true;
  HIP_CHECK(hipGetLastError());
  t->ring_pos++;
  t->ring_count = std::min(t->ring_count + 1, (int)orbpl_tracker::kRing);
  return ORBPL_OK;
}

extern "C" {

int orbpl_tracker_step(orbpl_tracker* t, const uint8_t* d_gray, const float* d_depth) {
  if (!t || !d_gray || !d_depth) return arg_fail("NULL argument");
  if (t->stereo) return arg_fail("stereo tracker: use orbpl_tracker_step_stereo");
  return tracker_step(t, d_gray, d_depth, nullptr);
}

int orbpl_tracker_step_host(orbpl_tracker* t, const uint8_t* h_gray, const uint16_t* h_depth,
                            float depth_map_factor) {
  if (!t || !h_gray || !h_depth) return arg_fail("NULL argument");
  if (t->stereo) return arg_fail("stereo tracker: orbpl_tracker_step_host takes RGB-D frames");
  if (!(depth_map_factor > 0.f)) return arg_fail("depth_map_factor must be > 0");
  HIP_CHECK(hipSetDevice(t->device));
  const size_t npx = (size_t)t->S * t->W * t->H;
  if (!t->cstream) {
    // everything into locals first: a failed allocation leaves the tracker
    // as it was (no half-initialised slots behind a non-null copy stream)
    std::vector<void*> got;
    auto fail = [&](hipError_t e, int line) {
      for (void* p : got) (void)hipFree(p);
      return hip_fail(e, "ingress slot allocation", line);
    };
    uint8_t* g[orbpl_tracker::kIn];
    uint16_t* d16[orbpl_tracker::kIn];
    float* df[orbpl_tracker::kIn];
    for (int k = 0; k < orbpl_tracker::kIn; k++) {
      void* p = nullptr;
      hipError_t e = hipMalloc(&p, npx);
      if (e != hipSuccess) return fail(e, __LINE__);
      got.push_back(p);
      g[k] = (uint8_t*)p;
      if ((e = hipMalloc(&p, npx * 2)) != hipSuccess) return fail(e, __LINE__);
      got.push_back(p);
      d16[k] = (uint16_t*)p;
      if ((e = hipMalloc(&p, npx * 4)) != hipSuccess) return fail(e, __LINE__);
      got.push_back(p);
      df[k] = (float*)p;
    }
    hipEvent_t evs[3 * orbpl_tracker::kIn] = {};
    hipStream_t cs = nullptr;
    hipError_t e = hipSuccess;
    for (int i = 0; i < 3 * orbpl_tracker::kIn && e == hipSuccess; i++)
      e = hipEventCreateWithFlags(&evs[i], hipEventDisableTiming);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&cs, hipStreamNonBlocking);
    if (e != hipSuccess) {
      for (hipEvent_t x : evs)
        if (x) (void)hipEventDestroy(x);
      return fail(e, __LINE__);
    }
    for (int k = 0; k < orbpl_tracker::kIn; k++) {
      t->in_gray[k] = g[k];
      t->in_d16[k] = d16[k];
      t->in_depth[k] = df[k];
      t->in_copied[k] = evs[3 * k];
      t->in_done_s[k] = evs[3 * k + 1];
      t->in_done_l[k] = evs[3 * k + 2];
    }
    t->allocs.insert(t->allocs.end(), got.begin(), got.end());
    t->cstream = cs;
  }
  const int k = t->in_pos % orbpl_tracker::kIn;
  // the slot's previous frames must have been read (extraction + line stream)
  if (t->in_used[k]) {
    HIP_CHECK(hipStreamWaitEvent(t->cstream, t->in_done_s[k], 0));
    if (t->lines) HIP_CHECK(hipStreamWaitEvent(t->cstream, t->in_done_l[k], 0));
  }
  HIP_CHECK(hipMemcpyAsync(t->in_gray[k], h_gray, npx, hipMemcpyHostToDevice, t->cstream));
  HIP_CHECK(hipMemcpyAsync(t->in_d16[k], h_depth, npx * 2, hipMemcpyHostToDevice, t->cstream));
  HIP_CHECK(hipEventRecord(t->in_copied[k], t->cstream));
  HIP_CHECK(hipStreamWaitEvent(t->stream, t->in_copied[k], 0));
  // mDepthMapFactor = 1.0f / DepthMapFactor (Tracking.cc:142-146)
  launch_depth_u16(t->in_d16[k], t->in_depth[k], (long long)npx, 1.0f / depth_map_factor,
                   t->stream);
  const int rc = tracker_step(t, t->in_gray[k], t->in_depth[k], nullptr);
  if (rc) return rc;
  // the depth slot is read by the frame glue, on the tracking stream when the
  // glue runs there (which follows the extraction stream's reads of the slot)
  HIP_CHECK(hipEventRecord(t->in_done_s[k], t->glue_on_ts && t->pipelined ? t->tstream : t->stream));
  if (t->lines) HIP_CHECK(hipEventRecord(t->in_done_l[k], t->lstream));
  t->in_used[k] = true;
  t->in_pos++;
  return ORBPL_OK;
}

int orbpl_tracker_step_stereo(orbpl_tracker* t, const uint8_t* d_left, const uint8_t* d_right) {
  if (!t || !d_left || !d_right) return arg_fail("NULL argument");
  if (!t->stereo) return arg_fail("tracker created without ORBPL_TRACK_STEREO");
  return tracker_step(t, d_left, nullptr, d_right);
}

int orbpl_tracker_launch_frames(const orbpl_tracker* t, int* orb_frames, int* lsd_frames) {
  if (!t) return arg_fail("NULL tracker");
  if (orb_frames) *orb_frames = t->osplit ? t->osplit : t->S;
  if (lsd_frames) *lsd_frames = !t->lines ? 0 : (t->lsplit ? t->lsplit : t->S);
  return ORBPL_OK;
}

int orbpl_tracker_set_pipelined(orbpl_tracker* t, int on) {
  if (!t) return arg_fail("NULL tracker");
  HIP_CHECK(hipSetDevice(t->device));
  HIP_CHECK(hipStreamSynchronize(t->stream));
  HIP_CHECK(hipStreamSynchronize(t->tstream));
  t->pipelined = on ? 1 : 0;
  return ORBPL_OK;
}

int orbpl_tracker_synchronize(orbpl_tracker* t) {
  if (!t) return arg_fail("NULL tracker");
  HIP_CHECK(hipSetDevice(t->device));
  if (t->cstream) HIP_CHECK(hipStreamSynchronize(t->cstream));
  HIP_CHECK(hipStreamSynchronize(t->tstream));
  if (t->lines) {
    HIP_CHECK(hipStreamSynchronize(t->lstream));
    int rc = t->lsplit ? lsdx_check(t->lx, t->lsplit) : lsdx_check(t->lx, t->S);
    if (!rc && t->lsplit) rc = lsdx_check(t->lx2, t->S - t->lsplit);
    if (rc) return rc;
  }
  if (t->stereo) {
    int rc = orbx_synchronize(t->exr);
    if (rc) return rc;
    if (t->lxr) {
      HIP_CHECK(hipStreamSynchronize(t->rlstream));
      rc = lsdx_check(t->lxr, t->S);
      if (rc) return rc;
    }
    HIP_CHECK(hipStreamSynchronize(t->stream));
    int err = 0;
    HIP_CHECK(hipMemcpy(&err, t->d_err, 4, hipMemcpyDeviceToHost));
    if (err) {
      // reported once: clear the flag so that later steps start clean
      HIP_CHECK(hipMemset(t->d_err, 0, 4));
      return (arg_fail("stereo row band capacity exceeded"), ORBPL_ERR_OVERFLOW);
    }
  }
  if (t->ex2) {
    const int rc = orbx_synchronize(t->ex2);
    if (rc) return rc;
  }
  return orbx_synchronize(t->ex);
}

int orbpl_tracker_get_state(orbpl_tracker* t, float* Tcw, int* nkps, int* nmatches, int* ninliers,
                            int* nmatches_map) {
  if (!t) return arg_fail("NULL tracker");
  HIP_CHECK(hipSetDevice(t->device));
  HIP_CHECK(hipStreamSynchronize(t->stream));
  HIP_CHECK(hipStreamSynchronize(t->tstream));
  if (t->lines) HIP_CHECK(hipStreamSynchronize(t->lstream));
  std::vector<StreamState> st(t->S);
  HIP_CHECK(hipMemcpy(st.data(), t->d_state, sizeof(StreamState) * t->S, hipMemcpyDeviceToHost));
  std::vector<int> n(t->S);
  // the frame just tracked
  HIP_CHECK(hipMemcpy(n.data(), t->fb[(t->ring_pos + 2) % 3].n, 4 * t->S, hipMemcpyDeviceToHost));
  for (int s = 0; s < t->S; s++) {
    if (Tcw) memcpy(Tcw + 16 * s, st[s].Tlast, 64);
    if (nkps) nkps[s] = n[s];
    if (nmatches) nmatches[s] = st[s].nmatches;
    if (ninliers) ninliers[s] = st[s].ninliers;
    if (nmatches_map) nmatches_map[s] = st[s].nmatches_map;
  }
  return ORBPL_OK;
}

int orbpl_tracker_timing_counts(int* counts5) {
  if (!counts5) return arg_fail("NULL argument");
  counts5[0] = kTimingStages;
  counts5[1] = kLineTimingStages;
  counts5[2] = kLsdTimingStages;
  counts5[3] = kStereoTimingStages;
  counts5[4] = kKernelTimingStages;
  return ORBPL_OK;
}

int orbpl_tracker_kernel_timings(orbpl_tracker* t, int max_steps, float* ms, int* n_steps) {
  if (!t || !ms || !n_steps) return arg_fail("NULL argument");
  HIP_CHECK(hipSetDevice(t->device));
  HIP_CHECK(hipStreamSynchronize(t->stream));
  HIP_CHECK(hipStreamSynchronize(t->tstream));
  // every k_pose launch of the step (TrackWithMotionModel, TrackReferenceKeyFrame,
  // TrackLocalMap) and TrackLocalMap's k_match_local, each bracketed alone
  static const int kPair[kKernelTimingStages][2] = {{28, 29}, {30, 31}, {34, 35}, {32, 33}};
  const int n = std::min(max_steps, t->ring_count);
  for (int k = 0; k < n; k++) {
    const int step = t->ring_pos - n + k;
    hipEvent_t* ev = &t->ring[(size_t)(step % orbpl_tracker::kRing) * orbpl_tracker::kEv];
    for (int i = 0; i < kKernelTimingStages; i++)
      HIP_CHECK(hipEventElapsedTime(&ms[k * kKernelTimingStages + i], ev[kPair[i][0]], ev[kPair[i][1]]));
  }
  *n_steps = n;
  return ORBPL_OK;
}

int orbpl_tracker_timings(orbpl_tracker* t, int max_steps, float* ms, int* n_steps) {
  if (!t || !ms || !n_steps) return arg_fail("NULL argument");
  HIP_CHECK(hipSetDevice(t->device));
  HIP_CHECK(hipStreamSynchronize(t->stream));
  HIP_CHECK(hipStreamSynchronize(t->tstream));
  // stage intervals: 5 extraction stages, glue (extraction stream), then
  // match (incl. prediction), pose, finish (tracking stream)
  // (+ TrackLocalMap: gather, frustum, local matching, second pose, count)
  // (+ KeyFrame::ComputeBoW with a vocabulary; 0 without)
  // (FAST, octree, orientation + descriptors, stages 2-4: the summed kernel
  // time of their level-group launches on the extractor's FAST stream, which
  // overlap the pyramid's later levels under the level pipeline)
  static const int kPair[kTimingStages][2] = {{0, 1}, {1, 2}, {36, 37}, {3, 4}, {4, 5},
                                              {orbpl_tracker::kEvGlue, 27},
                                              {7, 8}, {14, 9}, {26, 10}, {9, 26}, {27, 6}};
  const int n = std::min(max_steps, t->ring_count);
  for (int k = 0; k < n; k++) {
    const int step = t->ring_pos - n + k;
    hipEvent_t* ev = &t->ring[(size_t)(step % orbpl_tracker::kRing) * orbpl_tracker::kEv];
    for (int i = 0; i < kTimingStages; i++)
      HIP_CHECK(hipEventElapsedTime(&ms[k * kTimingStages + i], ev[kPair[i][0]], ev[kPair[i][1]]));
    // FAST (2), octree (3), orientation + descriptors (4): summed launch brackets
    for (int kind = 0; kind < 3; kind++) {
      float sum = 0.f;
      for (int gi = 0; gi < kFastGroups; gi++) {
        float m = 0.f;
        const int e = 36 + 2 * (kind * kFastGroups + gi);
        HIP_CHECK(hipEventElapsedTime(&m, ev[e], ev[e + 1]));
        sum += m;
      }
      ms[k * kTimingStages + 2 + kind] = sum;
    }
  }
  *n_steps = n;
  return ORBPL_OK;
}

int orbpl_tracker_line_timings(orbpl_tracker* t, int max_steps, float* ms, int* n_steps) {
  if (!t || !ms || !n_steps) return arg_fail("NULL argument");
  if (!t->lines) return arg_fail("tracker created without ORBPL_TRACK_LINES");
  HIP_CHECK(hipSetDevice(t->device));
  HIP_CHECK(hipStreamSynchronize(t->stream));
  HIP_CHECK(hipStreamSynchronize(t->tstream));
  HIP_CHECK(hipStreamSynchronize(t->lstream));
  // LSD (line stream), KeyLines + LBD + UndistortKeyLines (line stream),
  // LineMatcher::SearchByProjection (tracking stream)
  static const int kPair[kLineTimingStages][2] = {{11, 12}, {12, 13}, {8, 14}};
  const int n = std::min(max_steps, t->ring_count);
  for (int k = 0; k < n; k++) {
    const int step = t->ring_pos - n + k;
    hipEvent_t* ev = &t->ring[(size_t)(step % orbpl_tracker::kRing) * orbpl_tracker::kEv];
    for (int i = 0; i < kLineTimingStages; i++)
      HIP_CHECK(hipEventElapsedTime(&ms[k * kLineTimingStages + i], ev[kPair[i][0]], ev[kPair[i][1]]));
  }
  *n_steps = n;
  return ORBPL_OK;
}

int orbpl_tracker_set_history(orbpl_tracker* t, int max_steps) {
  if (!t || max_steps < 0) return arg_fail("bad argument");
  HIP_CHECK(hipSetDevice(t->device));
  HIP_CHECK(hipStreamSynchronize(t->stream));
  HIP_CHECK(hipStreamSynchronize(t->tstream));
  for (void* p : {(void*)t->d_hist_state, (void*)t->d_hist_n, (void*)t->d_hist_nl})
    if (p) {
      t->allocs.erase(std::remove(t->allocs.begin(), t->allocs.end(), p), t->allocs.end());
      HIP_CHECK(hipFree(p));
    }
  t->d_hist_state = nullptr;
  t->d_hist_n = t->d_hist_nl = nullptr;
  t->hist_cap = t->hist_count = 0;
  if (max_steps == 0) return ORBPL_OK;
  const size_t n = (size_t)max_steps * t->S;
  int rc = tr_alloc(t, (void**)&t->d_hist_state, n * sizeof(StreamState));
  if (!rc) rc = tr_alloc(t, (void**)&t->d_hist_n, n * 4);
  if (!rc) rc = tr_alloc(t, (void**)&t->d_hist_nl, n * 4);
  if (rc) return rc;
  t->hist_cap = max_steps;
  return ORBPL_OK;
}

int orbpl_tracker_get_history(orbpl_tracker* t, int stream, int max_steps, float* Tcw,
                              int* counts12, int* n_steps) {
  if (!t || !n_steps || stream < 0 || stream >= t->S || max_steps < 0) return arg_fail("bad argument");
  HIP_CHECK(hipSetDevice(t->device));
  HIP_CHECK(hipStreamSynchronize(t->tstream));
  const int n = std::min(max_steps, t->hist_count);
  *n_steps = n;
  for (int k = 0; k < n; k++) {
    const size_t o = (size_t)k * t->S + stream;
    StreamState st;
    int nk = 0, nl = 0;
    HIP_CHECK(hipMemcpy(&st, t->d_hist_state + o, sizeof(st), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemcpy(&nk, t->d_hist_n + o, 4, hipMemcpyDeviceToHost));
    if (t->lines) HIP_CHECK(hipMemcpy(&nl, t->d_hist_nl + o, 4, hipMemcpyDeviceToHost));
    if (Tcw) memcpy(Tcw + 16 * k, st.Tlast, 64);
    if (counts12) {
      int* c = counts12 + 12 * k;
      c[0] = nk; c[1] = st.nmatches; c[2] = st.ninliers; c[3] = st.nmatches_map; c[4] = st.ok;
      c[5] = nl; c[6] = t->lines ? st.nlmatches : 0; c[7] = t->lines ? st.nlmatches_map : 0;
      const bool lm = (t->local_map || t->map) && st.lm_active;
      c[8] = lm ? st.lm_nlocal : 0; c[9] = lm ? st.lm_inl : 0;
      c[10] = lm && t->lines ? st.lm_nllocal : 0; c[11] = lm && t->lines ? st.lm_linl : 0;
    }
  }
  return ORBPL_OK;
}

int orbpl_tracker_get_map_history(orbpl_tracker* t, int stream, int max_steps, int* counts24,
                                  int* n_steps) {
  if (!t || !n_steps || !counts24 || stream < 0 || stream >= t->S || max_steps < 0)
    return arg_fail("bad argument");
  if (!t->map) return arg_fail("tracker created without ORBPL_TRACK_MAP");
  std::vector<int> c12((size_t)std::max(max_steps, 1) * 12);
  int rc = orbpl_tracker_get_history(t, stream, max_steps, nullptr, c12.data(), n_steps);
  if (rc) return rc;
  for (int k = 0; k < *n_steps; k++) {
    StreamState st;
    HIP_CHECK(hipMemcpy(&st, t->d_hist_state + (size_t)k * t->S + stream, sizeof(st),
                        hipMemcpyDeviceToHost));
    int* c = counts24 + 24 * k;
    for (int q = 0; q < 12; q++) c[q] = c12[(size_t)k * 12 + q];
    for (int q = 0; q < kMapOut; q++) c[12 + q] = st.map_out[q];
  }
  return ORBPL_OK;
}

// one stream's map (host copies; tests and inspection): keyframes with their
// parent and covisibility order, map points, map lines
static int map_stream_state(orbpl_tracker* t, int stream, MapState* ms) {
  if (!t || stream < 0 || stream >= t->S) return arg_fail("bad argument");
  if (!t->map) return arg_fail("tracker created without ORBPL_TRACK_MAP");
  HIP_CHECK(hipSetDevice(t->device));
  HIP_CHECK(hipStreamSynchronize(t->tstream));
  HIP_CHECK(hipStreamSynchronize(t->stream));
  HIP_CHECK(hipMemcpy(ms, t->ma.ms + stream, sizeof(MapState), hipMemcpyDeviceToHost));
  return ORBPL_OK;
}

int orbpl_tracker_get_map_keyframes(orbpl_tracker* t, int stream, int* parent, int* ord, int cap,
                                    int* nord, int* n_kf) {
  MapState ms;
  int rc = map_stream_state(t, stream, &ms);
  if (rc) return rc;
  if (!n_kf || cap < 0) return arg_fail("bad argument");
  const int n = ms.n_kf, F = t->map_kfc;
  *n_kf = n;
  const size_t kb = (size_t)stream * F;
  std::vector<int> par(F), no(F);
  std::vector<uint8_t> o((size_t)F * F);
  HIP_CHECK(hipMemcpy(par.data(), t->ma.kf_parent + kb, 4 * (size_t)F, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(no.data(), t->ma.kf_nord + kb, 4 * (size_t)F, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(o.data(), t->ma.kf_ord + kb * F, (size_t)F * F, hipMemcpyDeviceToHost));
  for (int k = 0; k < n; k++) {
    if (parent) parent[k] = par[k];
    if (nord) nord[k] = no[k];
    if (ord)
      for (int j = 0; j < cap; j++) ord[(size_t)k * cap + j] = j < no[k] && j < F ? o[(size_t)k * F + j] : -1;
  }
  return ORBPL_OK;
}

int orbpl_tracker_get_map_points(orbpl_tracker* t, int stream, int cap, int* nobs, uint8_t* desc,
                                 float* xyz, float* normal, float* dist2, int* n_mp) {
  MapState ms;
  int rc = map_stream_state(t, stream, &ms);
  if (rc) return rc;
  if (!n_mp || cap < 0) return arg_fail("bad argument");
  *n_mp = ms.n_mp;
  const int n = std::min(ms.n_mp, cap);
  const size_t g = (size_t)stream * t->ma.mpc;
  std::vector<float> f4((size_t)n * 4 + 1);
  if (nobs && n) HIP_CHECK(hipMemcpy(nobs, t->ma.mp_nobs + g, 4 * (size_t)n, hipMemcpyDeviceToHost));
  if (desc && n) HIP_CHECK(hipMemcpy(desc, t->ma.mp_desc + g * 32, 32 * (size_t)n, hipMemcpyDeviceToHost));
  if (xyz && n) {
    HIP_CHECK(hipMemcpy(f4.data(), t->ma.mp_pos + g, 16 * (size_t)n, hipMemcpyDeviceToHost));
    for (int p = 0; p < n; p++)
      for (int q = 0; q < 3; q++) xyz[3 * p + q] = f4[4 * p + q];
  }
  if (normal && n) {
    HIP_CHECK(hipMemcpy(f4.data(), t->ma.mp_nrm + g, 16 * (size_t)n, hipMemcpyDeviceToHost));
    for (int p = 0; p < n; p++)
      for (int q = 0; q < 3; q++) normal[3 * p + q] = f4[4 * p + q];
  }
  if (dist2 && n) HIP_CHECK(hipMemcpy(dist2, t->ma.mp_dist + g, 8 * (size_t)n, hipMemcpyDeviceToHost));
  return ORBPL_OK;
}

int orbpl_tracker_get_map_lines(orbpl_tracker* t, int stream, int cap, int* nobs, uint8_t* desc,
                                float* pos6, int* n_ml) {
  MapState ms;
  int rc = map_stream_state(t, stream, &ms);
  if (rc) return rc;
  if (!n_ml || cap < 0) return arg_fail("bad argument");
  *n_ml = ms.n_ml;
  const int n = std::min(ms.n_ml, cap);
  const size_t g = (size_t)stream * t->ma.mlc;
  if (nobs && n) HIP_CHECK(hipMemcpy(nobs, t->ma.ml_nobs + g, 4 * (size_t)n, hipMemcpyDeviceToHost));
  if (desc && n) HIP_CHECK(hipMemcpy(desc, t->ma.ml_desc + g * 32, 32 * (size_t)n, hipMemcpyDeviceToHost));
  if (pos6 && n) HIP_CHECK(hipMemcpy(pos6, t->ma.ml_pos + g * 6, 24 * (size_t)n, hipMemcpyDeviceToHost));
  return ORBPL_OK;
}

int orbpl_tracker_get_map_errors(orbpl_tracker* t, int* err) {
  if (!t || !err) return arg_fail("NULL argument");
  if (!t->map) return arg_fail("tracker created without ORBPL_TRACK_MAP");
  HIP_CHECK(hipSetDevice(t->device));
  HIP_CHECK(hipStreamSynchronize(t->tstream));
  HIP_CHECK(hipStreamSynchronize(t->stream));
  std::vector<MapState> ms(t->S);
  HIP_CHECK(hipMemcpy(ms.data(), t->ma.ms, sizeof(MapState) * t->S, hipMemcpyDeviceToHost));
  for (int s = 0; s < t->S; s++) err[s] = ms[s].err;
  return ORBPL_OK;
}

int orbpl_tracker_lsd_timings(orbpl_tracker* t, int max_steps, float* ms, int* n_steps) {
  if (!t || !ms || !n_steps) return arg_fail("NULL argument");
  if (!t->lines) return arg_fail("tracker created without ORBPL_TRACK_LINES");
  HIP_CHECK(hipSetDevice(t->device));
  HIP_CHECK(hipStreamSynchronize(t->lstream));
  // line stream: blur+resize+grad, sort, seed loop, validate, KeyLines,
  // blur5+Sobel+LBD, UndistortKeyLines + line depths
  static const int kPair[kLsdTimingStages][2] = {{11, 18}, {18, 19}, {19, 20}, {20, 12},
                                                 {12, 21}, {21, 22}, {22, 13}};
  const int n = std::min(max_steps, t->ring_count);
  for (int k = 0; k < n; k++) {
    const int step = t->ring_pos - n + k;
    hipEvent_t* ev = &t->ring[(size_t)(step % orbpl_tracker::kRing) * orbpl_tracker::kEv];
    for (int i = 0; i < kLsdTimingStages; i++)
      HIP_CHECK(hipEventElapsedTime(&ms[k * kLsdTimingStages + i], ev[kPair[i][0]], ev[kPair[i][1]]));
  }
  *n_steps = n;
  return ORBPL_OK;
}

int orbpl_tracker_stereo_timings(orbpl_tracker* t, int max_steps, float* ms, int* n_steps) {
  if (!t || !ms || !n_steps) return arg_fail("NULL argument");
  if (!t->stereo) return arg_fail("tracker created without ORBPL_TRACK_STEREO");
  HIP_CHECK(hipSetDevice(t->device));
  HIP_CHECK(hipStreamSynchronize(t->stream));
  HIP_CHECK(hipStreamSynchronize(t->tstream));
  HIP_CHECK(hipStreamSynchronize(t->rstream));
  // right ORB extraction (right stream), ComputeStereoMatches (extraction
  // stream); with lines: right LineExtractor (right line stream),
  // k_stereo_lines (line stream); 0 without lines
  static const int kPair[kStereoTimingStages][2] = {{15, 16}, {17, 27}, {23, 24}, {25, 13}};
  if (t->rlstream) HIP_CHECK(hipStreamSynchronize(t->rlstream));
  if (t->lstream) HIP_CHECK(hipStreamSynchronize(t->lstream));
  const int n = std::min(max_steps, t->ring_count);
  for (int k = 0; k < n; k++) {
    const int step = t->ring_pos - n + k;
    hipEvent_t* ev = &t->ring[(size_t)(step % orbpl_tracker::kRing) * orbpl_tracker::kEv];
    for (int i = 0; i < kStereoTimingStages; i++) {
      float* o = &ms[k * kStereoTimingStages + i];
      *o = 0.0f;
      if (i < 2 || t->lines) HIP_CHECK(hipEventElapsedTime(o, ev[kPair[i][0]], ev[kPair[i][1]]));
    }
  }
  *n_steps = n;
  return ORBPL_OK;
}

// Debug (ORBPL_POSE_PROFILE): stream 0's PoseOptimization phase times of the
// last step, ns: edges, linearize+reduce, solve+exp, trial errors+reduce,
// classify; then LM iterations and trials (counts).
int orbpl_tracker_debug_pose_profile(orbpl_tracker* t, long long* out7) {  // 8 values
  if (!t || !out7) return arg_fail("NULL argument");
  HIP_CHECK(hipSetDevice(t->device));
  HIP_CHECK(hipDeviceSynchronize());
  long long p[8];
  if (read_pose_profile(p)) return arg_fail("pose profile unavailable");
  for (int k = 0; k < 5; k++) out7[k] = p[k] * 10;
  out7[5] = p[5];
  out7[6] = p[6];
  out7[7] = p[7] * 10;
  return ORBPL_OK;
}

// Debug (ORBPL_MATCH_PROFILE): stream 0's SearchByProjection(last frame)
// phase times of the last step, ns: grid, candidates, ordered claims,
// rotation check, output.
int orbpl_tracker_debug_match_profile(orbpl_tracker* t, long long* out5) {
  if (!t || !out5) return arg_fail("NULL argument");
  HIP_CHECK(hipSetDevice(t->device));
  HIP_CHECK(hipDeviceSynchronize());
  long long p[8];
  if (read_match_profile(p)) return arg_fail("match profile unavailable");
  for (int k = 0; k < 5; k++) out5[k] = p[k] * 10;
  return ORBPL_OK;
}

int orbpl_tracker_timings_reset(orbpl_tracker* t) {
  if (!t) return arg_fail("NULL tracker");
  t->ring_count = 0;
  return ORBPL_OK;
}

int orbpl_tracker_stage_ms(orbpl_tracker* t, float* ms5) {
  if (!t || !ms5) return arg_fail("NULL argument");
  if (t->ring_count == 0) return arg_fail("no step recorded yet");
  float m[kTimingStages];
  int n = 0;
  int rc = orbpl_tracker_timings(t, 1, m, &n);
  if (rc) return rc;
  ms5[0] = m[0] + m[1] + m[2] + m[3] + m[4];
  for (int i = 0; i < 4; i++) ms5[1 + i] = m[5 + i];
  ms5[1] += m[10];  // glue: + KeyFrame::ComputeBoW
  ms5[3] += m[9];   // pose: both PoseOptimizations (+ the local map search)
  return ORBPL_OK;
}

int orbpl_tracker_kp_capacity(const orbpl_tracker* t) { return t ? t->kp_cap : 0; }

int orbpl_tracker_get_frame(orbpl_tracker* t, int stream, orbpl_keypoint* kps_un, uint8_t* desc,
                            int32_t* match, uint8_t* outlier, int* n) {
  if (!t || stream < 0 || stream >= t->S) return arg_fail("bad argument");
  HIP_CHECK(hipSetDevice(t->device));
  HIP_CHECK(hipStreamSynchronize(t->stream));
  HIP_CHECK(hipStreamSynchronize(t->tstream));
  const FrameBufs& F = t->fb[(t->ring_pos + 2) % 3];
  const size_t K = t->kp_cap, o = (size_t)stream * K;
  int cnt = 0;
  HIP_CHECK(hipMemcpy(&cnt, F.n + stream, 4, hipMemcpyDeviceToHost));
  if (n) *n = cnt;
  if (kps_un) HIP_CHECK(hipMemcpy(kps_un, F.kps_un + o, K * sizeof(KeyPointD), hipMemcpyDeviceToHost));
  if (desc) HIP_CHECK(hipMemcpy(desc, F.desc + o * 32, K * 32, hipMemcpyDeviceToHost));
  if (match) HIP_CHECK(hipMemcpy(match, F.match + o, K * 4, hipMemcpyDeviceToHost));
  if (outlier) HIP_CHECK(hipMemcpy(outlier, F.outlier + o, K, hipMemcpyDeviceToHost));
  return ORBPL_OK;
}

int orbpl_tracker_get_status(orbpl_tracker* t, int* ok, int* nlines, int* line_matches,
                             int* line_nmatches_map) {
  if (!t) return arg_fail("NULL tracker");
  HIP_CHECK(hipSetDevice(t->device));
  HIP_CHECK(hipStreamSynchronize(t->stream));
  HIP_CHECK(hipStreamSynchronize(t->tstream));
  if (t->lines) HIP_CHECK(hipStreamSynchronize(t->lstream));
  std::vector<StreamState> st(t->S);
  HIP_CHECK(hipMemcpy(st.data(), t->d_state, sizeof(StreamState) * t->S, hipMemcpyDeviceToHost));
  std::vector<int> nl(t->S, 0);
  if (t->lines)
    HIP_CHECK(hipMemcpy(nl.data(), t->fb[(t->ring_pos + 2) % 3].nl, 4 * t->S, hipMemcpyDeviceToHost));
  for (int s = 0; s < t->S; s++) {
    if (ok) ok[s] = st[s].ok;
    if (nlines) nlines[s] = nl[s];
    if (line_matches) line_matches[s] = t->lines ? st[s].nlmatches : 0;
    if (line_nmatches_map) line_nmatches_map[s] = t->lines ? st[s].nlmatches_map : 0;
  }
  return ORBPL_OK;
}

int orbpl_tracker_set_vocabulary(orbpl_tracker* t, orbv_vocab* voc, int levelsup) {
  if (!t) return arg_fail("NULL tracker");
  HIP_CHECK(hipSetDevice(t->device));
  HIP_CHECK(hipStreamSynchronize(t->stream));
  HIP_CHECK(hipStreamSynchronize(t->tstream));
  if (!voc) {
    t->voc = nullptr;
    return ORBPL_OK;
  }
  if (t->kp_cap > 4096) return arg_fail("orbpl_tracker_set_vocabulary: > 4096 keypoints per frame");
  const int rc = orbv_upload(voc, t->device);
  if (rc) return rc;
  if (!t->d_bow_err) {
    const size_t SK = (size_t)t->S * t->kp_cap;
    auto alloc = [&](void** p, size_t bytes) -> int {
      HIP_CHECK(hipMalloc(p, bytes));
      t->allocs.push_back(*p);
      return ORBPL_OK;
    };
    for (FrameBufs& f : t->fb) {
      if (alloc((void**)&f.feat_node, SK * 4) || alloc((void**)&f.feat_word, SK * 4) ||
          alloc((void**)&f.feat_weight, SK * 8) || alloc((void**)&f.bow_words, SK * 4) ||
          alloc((void**)&f.bow_vals, SK * 8) || alloc((void**)&f.bow_n, (size_t)t->S * 4))
        return ORBPL_ERR_HIP;
      HIP_CHECK(hipMemset(f.bow_n, 0, (size_t)t->S * 4));
    }
    if (alloc((void**)&t->d_bow_err, 4)) return ORBPL_ERR_HIP;
    HIP_CHECK(hipMemset(t->d_bow_err, 0, 4));
  }
  t->voc = voc;
  t->voc_levelsup = levelsup;
  return ORBPL_OK;
}

int orbpl_tracker_get_bow(orbpl_tracker* t, int stream, uint32_t* bow_words, double* bow_vals,
                          int* bow_n, int32_t* feat_node, int* n) {
  if (!t || stream < 0 || stream >= t->S) return arg_fail("bad argument");
  if (!t->d_bow_err) return arg_fail("orbpl_tracker_get_bow: no vocabulary set");
  HIP_CHECK(hipSetDevice(t->device));
  HIP_CHECK(hipStreamSynchronize(t->stream));
  HIP_CHECK(hipStreamSynchronize(t->tstream));
  const FrameBufs& F = t->fb[(t->ring_pos + 2) % 3];
  const size_t K = t->kp_cap, o = (size_t)stream * K;
  int cnt = 0, bn = 0, err = 0;
  HIP_CHECK(hipMemcpy(&cnt, F.n + stream, 4, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(&bn, F.bow_n + stream, 4, hipMemcpyDeviceToHost));
  HIP_CHECK(hipMemcpy(&err, t->d_bow_err, 4, hipMemcpyDeviceToHost));
  if (err) {
    HIP_CHECK(hipMemset(t->d_bow_err, 0, 4));
    return arg_fail("BoW transform: feature capacity exceeded");
  }
  if (n) *n = cnt;
  if (bow_n) *bow_n = bn;
  if (bow_words && bn) HIP_CHECK(hipMemcpy(bow_words, F.bow_words + o, 4 * (size_t)bn, hipMemcpyDeviceToHost));
  if (bow_vals && bn) HIP_CHECK(hipMemcpy(bow_vals, F.bow_vals + o, 8 * (size_t)bn, hipMemcpyDeviceToHost));
  if (feat_node && cnt) HIP_CHECK(hipMemcpy(feat_node, F.feat_node + o, 4 * (size_t)cnt, hipMemcpyDeviceToHost));
  return ORBPL_OK;
}

int orbpl_tracker_get_trk(orbpl_tracker* t, int* trk) {
  if (!t || !trk) return arg_fail("NULL argument");
  HIP_CHECK(hipSetDevice(t->device));
  HIP_CHECK(hipStreamSynchronize(t->stream));
  HIP_CHECK(hipStreamSynchronize(t->tstream));
  std::vector<StreamState> st(t->S);
  HIP_CHECK(hipMemcpy(st.data(), t->d_state, sizeof(StreamState) * t->S, hipMemcpyDeviceToHost));
  for (int s = 0; s < t->S; s++) trk[s] = t->refkf ? st[s].trk : 0;
  return ORBPL_OK;
}

int orbpl_tracker_get_local_stats(orbpl_tracker* t, int* local_matches, int* local_inliers,
                                  int* local_line_matches, int* local_line_inliers) {
  if (!t) return arg_fail("NULL tracker");
  HIP_CHECK(hipSetDevice(t->device));
  HIP_CHECK(hipStreamSynchronize(t->tstream));
  HIP_CHECK(hipStreamSynchronize(t->stream));
  std::vector<StreamState> st(t->S);
  HIP_CHECK(hipMemcpy(st.data(), t->d_state, sizeof(StreamState) * t->S, hipMemcpyDeviceToHost));
  for (int s = 0; s < t->S; s++) {
    const bool lm = (t->local_map || t->map) && st[s].lm_active;
    if (local_matches) local_matches[s] = lm ? st[s].lm_nlocal : 0;
    if (local_inliers) local_inliers[s] = lm ? st[s].lm_inl : 0;
    if (local_line_matches) local_line_matches[s] = lm && t->lines ? st[s].lm_nllocal : 0;
    if (local_line_inliers) local_line_inliers[s] = lm && t->lines ? st[s].lm_linl : 0;
  }
  return ORBPL_OK;
}

int orbpl_tracker_get_lines(orbpl_tracker* t, int stream, orbpl_keyline* kl_un, uint8_t* desc,
                            int32_t* lmatch, uint8_t* loutlier, int* n) {
  if (!t || stream < 0 || stream >= t->S) return arg_fail("bad argument");
  if (!t->lines) return arg_fail("tracker created without ORBPL_TRACK_LINES");
  HIP_CHECK(hipSetDevice(t->device));
  HIP_CHECK(hipStreamSynchronize(t->stream));
  HIP_CHECK(hipStreamSynchronize(t->tstream));
  HIP_CHECK(hipStreamSynchronize(t->lstream));
  const FrameBufs& F = t->fb[(t->ring_pos + 2) % 3];
  const size_t K = kLineKeep, o = (size_t)stream * K;
  int cnt = 0;
  HIP_CHECK(hipMemcpy(&cnt, F.nl + stream, 4, hipMemcpyDeviceToHost));
  if (n) *n = cnt;
  if (kl_un) HIP_CHECK(hipMemcpy(kl_un, F.kl_un + o, K * sizeof(orbpl_keyline), hipMemcpyDeviceToHost));
  if (desc) HIP_CHECK(hipMemcpy(desc, F.ldesc + o * 32, K * 32, hipMemcpyDeviceToHost));
  if (lmatch) HIP_CHECK(hipMemcpy(lmatch, F.lmatch + o, K * 4, hipMemcpyDeviceToHost));
  if (loutlier) HIP_CHECK(hipMemcpy(loutlier, F.loutlier + o, K, hipMemcpyDeviceToHost));
  return ORBPL_OK;
}

}  // extern "C"
