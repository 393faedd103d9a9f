// C-ABI of the tracking half's single-call host-pointer entry points (drop-in
// for Frame / ORBmatcher / LineMatcher / Optimizer calls): refuse bad
// arguments, stage the host arrays on the device (host_stage.h), launch on the
// null stream, copy the results back. Plus the frame constants they share with
// the batched tracker (track_runtime.cpp) and the relocaliser (reloc.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>

#include "../../include/orbpl.h"
#include "host_stage.h"
#include "orb_kernels.h"
#include "orbpl_runtime.h"
#include "track_kernels.h"
#include "lsd_kernels.h"
#include "lsd_math.h"
#include "reloc_kernels.h"

using namespace orbpl;

// ComputeImageBounds uses the same undistortion code as the device kernel
// (host-compiled, same IEEE double sequence).
int orbpl::make_consts(const orbpl_camera* cam, const float* scale, const float* inv_sigma2,
                       int nlevels, TrackConsts* out) {
  if (!cam) return arg_fail("NULL camera");
  if (nlevels < 1 || nlevels > kMaxLevelsT) return arg_fail("nlevels out of range");
  TrackConsts c{};
  c.fx = cam->fx; c.fy = cam->fy; c.cx = cam->cx; c.cy = cam->cy;
  c.k1 = cam->k1; c.k2 = cam->k2; c.p1 = cam->p1; c.p2 = cam->p2; c.k3 = cam->k3;
  c.bf = cam->bf;
  c.mb = cam->bf / cam->fx;
  c.th_depth = cam->th_depth;
  c.invfx = 1.0f / cam->fx;
  c.invfy = 1.0f / cam->fy;
  c.width = cam->width;
  c.height = cam->height;
  if (cam->k1 != 0.0f) {
    float ux[4], uy[4];
    const float px[4] = {0.0f, (float)cam->width, 0.0f, (float)cam->width};
    const float py[4] = {0.0f, 0.0f, (float)cam->height, (float)cam->height};
    for (int i = 0; i < 4; i++) undistort_point_d(c, px[i], py[i], &ux[i], &uy[i]);
    c.minX = std::min(ux[0], ux[2]);
    c.maxX = std::max(ux[1], ux[3]);
    c.minY = std::min(uy[0], uy[1]);
    c.maxY = std::max(uy[2], uy[3]);
  } else {
    c.minX = 0.0f; c.maxX = (float)cam->width; c.minY = 0.0f; c.maxY = (float)cam->height;
  }
  c.gridInvW = static_cast<float>(kGridCols) / static_cast<float>(c.maxX - c.minX);
  c.gridInvH = static_cast<float>(kGridRows) / static_cast<float>(c.maxY - c.minY);
  c.nlevels = nlevels;
  for (int l = 0; l < nlevels; l++) {
    c.scale[l] = scale ? scale[l] : 1.0f;
    c.inv_sigma2[l] = inv_sigma2 ? inv_sigma2[l] : 1.0f;
  }
  *out = c;
  return ORBPL_OK;
}

float orbpl::log_scale_of(float scale_factor) { return (float)lsdm::log_((double)scale_factor); }

float orbpl::log_scale_of(const float* scale_factors, int nlevels) {
  return nlevels > 1 ? log_scale_of(scale_factors[1]) : 1.0f;
}

namespace {

hipStream_t scratch_stream() { return nullptr; }  // host-pointer APIs use the null stream

// orbpl_keypoint and the kernels' KeyPointD differ only in name
const KeyPointD* kpd(const orbpl_keypoint* k) { return reinterpret_cast<const KeyPointD*>(k); }
KeyPointD* kpd(orbpl_keypoint* k) { return reinterpret_cast<KeyPointD*>(k); }
static_assert(sizeof(KeyPointD) == sizeof(orbpl_keypoint), "keypoint layouts differ");

}  // namespace

extern "C" {

int orbpl_frame_prepare(const orbpl_camera* cam, const orbpl_keypoint* kps, int n,
                        const float* depth, orbpl_keypoint* kps_un, float* depth_out,
                        float* uright_out, int32_t* grid_cell, float* bounds) {
  if (!cam || n < 0 || (n > 0 && (!kps || !kps_un || !depth_out || !uright_out || !grid_cell)))
    return arg_fail("bad argument");
  TrackConsts c;
  int rc = make_consts(cam, nullptr, nullptr, 1, &c);
  if (rc) return rc;
  if (bounds) { bounds[0] = c.minX; bounds[1] = c.maxX; bounds[2] = c.minY; bounds[3] = c.maxY; }
  if (n == 0) return ORBPL_OK;
  HostStage st;
  const size_t img = (size_t)cam->width * cam->height;
  const KeyPointD* d_kps = st.in(kpd(kps), n, n);
  const int* d_n = st.in_value(n);
  const float* d_depth = st.in_opt(depth, img, img);
  KeyPointD* d_kps_un = st.out<KeyPointD>(n);
  float* d_depth_out = st.out<float>(n);
  float* d_uright = st.out<float>(n);
  int* d_gcell = st.out<int>(n);
  if (st.rc()) return st.rc();
  launch_frame_prepare(c, d_kps, d_n, n, d_depth, 0, d_kps_un, d_depth_out, d_uright, d_gcell, 1,
                       scratch_stream());
  st.launched();
  st.back(kpd(kps_un), d_kps_un, n);
  st.back(depth_out, d_depth_out, n);
  st.back(uright_out, d_uright, n);
  st.back(grid_cell, d_gcell, n);
  return st.rc();
}

int orbm_search_by_projection_last(const orbpl_camera* cam, const float* scale_factors, int nlevels,
                                   const orbpl_match_current* cur, const orbpl_match_last* last,
                                   float th, int mono, int check_orientation, int32_t* match,
                                   int* nmatches) {
  if (!cam || !scale_factors || !cur || !last || !match || !nmatches) return arg_fail("NULL argument");
  const int n = cur->n, nl = last->n;
  if (n < 0 || nl < 0 || n > kMatchMaxKp || nl > kMatchMaxKp)
    return arg_fail("keypoint count exceeds the matcher capacity (2048)");
  TrackConsts c;
  int rc = make_consts(cam, scale_factors, nullptr, nlevels, &c);
  if (rc) return rc;
  if (!cur->Tcw || !last->Tcw || (n > 0 && (!cur->kps_un || !cur->desc || !cur->uright)) ||
      (nl > 0 && (!last->kps_un || !last->has_mp || !last->outlier || !last->mp_xyz ||
                  !last->mp_desc || !last->mp_nobs)))
    return arg_fail("NULL frame arrays");
  // the kernel reads scale[] at a last-frame octave and keeps the current
  // octaves as int8 for the level window
  for (int i = 0; i < n; i++)
    if (cur->kps_un[i].octave < 0 || cur->kps_un[i].octave >= nlevels)
      return arg_fail("keypoint octave outside the pyramid");
  for (int i = 0; i < nl; i++)
    if (last->kps_un[i].octave < 0 || last->kps_un[i].octave >= nlevels)
      return arg_fail("keypoint octave outside the pyramid");
  const int P = std::max(1, std::max(n, nl));
  float T[32];   // the current pose, then the last frame's
  memcpy(T, cur->Tcw, 64);
  memcpy(T + 16, last->Tcw, 64);
  HostStage st;
  MatchLaunch m{};
  m.cur_kps_un = st.in(kpd(cur->kps_un), n, P);
  m.cur_desc = st.in(cur->desc, 32 * n, 32 * P);
  m.cur_uright = st.in(cur->uright, n, P);
  m.cur_gcell = nullptr;  // computed on device from kps_un (PosInGrid)
  m.cur_n = st.in_value(n);
  m.last_kps_un = st.in(kpd(last->kps_un), nl, P);
  m.last_has_mp = st.in(last->has_mp, nl, P);
  m.last_outlier = st.in(last->outlier, nl, P);
  m.last_xyz = st.in(last->mp_xyz, 3 * nl, 3 * P);
  m.last_desc = st.in(last->mp_desc, 32 * nl, 32 * P);
  m.last_nobs = st.in(last->mp_nobs, nl, P);
  m.last_n = st.in_value(nl);
  m.kp_pitch = P;
  m.Tcw = st.in(T, 32, 32);
  m.Tlw = m.Tcw + 16;
  m.pose_stride = 32;
  m.match = st.out<int>(P);
  m.nmatches = st.out<int>(1);
  m.nm_stride = 1;
  m.th = th;
  m.mono = mono;
  m.check_ori = check_orientation;
  m.retry = 0;
  m.active = nullptr;
  if (st.rc()) return st.rc();
  launch_match_last(c, m, 1, scratch_stream());
  st.launched();
  st.back(match, m.match, n);
  st.back(nmatches, m.nmatches, 1);
  return st.rc();
}

int orbpl_pose_optimization(const orbpl_camera* cam, const orbpl_pose_problem* P, float* Tcw,
                            uint8_t* outlier, uint8_t* line_outlier, int* n_inliers) {
  return orbpl_pose_optimization_ex(cam, P, 0, Tcw, outlier, line_outlier, n_inliers);
}

int orbpl_pose_optimization_ex(const orbpl_camera* cam, const orbpl_pose_problem* P, int flags,
                               float* Tcw, uint8_t* outlier, uint8_t* line_outlier,
                               int* n_inliers) {
  if (!cam || !P || !Tcw || !n_inliers) return arg_fail("NULL argument");
  if (flags & ~ORBPL_POSE_FIXED_LINE_JAC) return arg_fail("unknown pose flag");
  const int n = P->n, nl = P->nl;
  if (n < 0 || nl < 0 || n + nl > kPoseMaxEdges) return arg_fail("too many edges (max 2304)");
  if (n > 0 && (!P->kps_un || !P->uright || !P->has_mp || !P->mp_xyz || !outlier))
    return arg_fail("NULL point arrays");
  if (nl > 0 && (!P->kl_obs || !P->kl_octave || !P->has_ml || !P->ml_xyz || !line_outlier))
    return arg_fail("NULL line arrays");
  TrackConsts c;
  int rc = make_consts(cam, nullptr, P->inv_sigma2, P->nlevels, &c);
  if (rc) return rc;
  const int Pn = std::max(1, n), Pl = std::max(1, nl);
  HostStage st;
  PoseLaunch p{};
  p.kps_un = st.in(kpd(P->kps_un), n, Pn);
  p.uright = st.in(P->uright, n, Pn);
  p.match = nullptr;
  p.has_mp = st.in(P->has_mp, n, Pn);
  p.mp_xyz = st.in(P->mp_xyz, 3 * n, 3 * Pn);
  p.n = st.in_value(n);
  p.kp_pitch = Pn;
  p.kl_obs = st.in(P->kl_obs, 4 * nl, 4 * Pl);
  p.kl_octave = st.in(P->kl_octave, nl, Pl);
  p.has_ml = st.in(P->has_ml, nl, Pl);
  p.ml_xyz = st.in(P->ml_xyz, 6 * nl, 6 * Pl);
  p.nl = nl;
  p.Tcw = st.in(Tcw, 16, 16);
  p.pose_stride = 16;
  p.outlier = st.in(outlier, n, Pn);
  p.line_outlier = st.in(line_outlier, nl, Pl);
  p.ninliers = st.out<int>(1);
  p.nm_stride = 1;
  p.active = nullptr;
  // PoseEdge is the kernels' own type: sized in bytes
  p.edges = reinterpret_cast<PoseEdge*>(st.out<char>(kPoseMaxEdges * pose_edge_bytes()));
  p.fixed_line_jac = (flags & ORBPL_POSE_FIXED_LINE_JAC) ? 1 : 0;
  if (st.rc()) return st.rc();
  launch_pose(c, p, 1, scratch_stream());
  st.launched();
  st.back(Tcw, p.Tcw, 16);
  st.back(outlier, p.outlier, n);
  st.back(line_outlier, p.line_outlier, nl);
  st.back(n_inliers, p.ninliers, 1);
  return st.rc();
}

int orbpl_frame_is_in_frustum(const orbpl_camera* cam, float scale_factor, int nlevels,
                              const float* Tcw, int n, const float* xyz, const float* normal,
                              const float* min_dist, const float* max_dist, float view_cos_limit,
                              uint8_t* in_view, float* proj_x, float* proj_y, float* proj_xr,
                              int32_t* level, float* view_cos) {
  if (!cam || !Tcw || n < 0 || nlevels < 1 || nlevels > kMaxLevelsT) return arg_fail("bad argument");
  if (n > 0 && (!xyz || !normal || !min_dist || !max_dist || !in_view || !proj_x || !proj_y ||
                !proj_xr || !level || !view_cos))
    return arg_fail("NULL map point arrays");
  TrackConsts c;
  int rc = make_consts(cam, nullptr, nullptr, nlevels, &c);
  if (rc) return rc;
  if (n == 0) return ORBPL_OK;
  const size_t N = n;
  HostStage st;
  InFrustumArgs a{n,
                  st.in(Tcw, 16, 16),
                  st.in(xyz, 3 * N, 3 * N),
                  st.in(normal, 3 * N, 3 * N),
                  st.in(min_dist, N, N),
                  st.in(max_dist, N, N),
                  view_cos_limit,
                  st.out<uint8_t>(N),
                  st.out<float>(N),
                  st.out<float>(N),
                  st.out<float>(N),
                  st.out<int>(N),
                  st.out<float>(N)};
  if (st.rc()) return st.rc();
  launch_in_frustum(c, log_scale_of(scale_factor), a, scratch_stream());
  st.launched();
  st.back(in_view, a.in_view, n);
  st.back(proj_x, a.proj_x, n);
  st.back(proj_y, a.proj_y, n);
  st.back(proj_xr, a.proj_xr, n);
  st.back(level, a.level, n);
  st.back(view_cos, a.view_cos, n);
  return st.rc();
}

int orbm_search_by_projection_local(const orbpl_camera* cam, const float* scale_factors,
                                    int nlevels, const orbpl_match_current* cur, int nmp,
                                    const uint8_t* in_view, const float* proj_x,
                                    const float* proj_y, const float* proj_xr,
                                    const int32_t* level, const float* view_cos,
                                    const uint8_t* mp_desc, const int32_t* mp_nobs,
                                    const int32_t* cur_nobs, float th, float nnratio,
                                    int32_t* match, int* nmatches) {
  if (!cam || !scale_factors || !cur || !nmatches || nmp < 0) return arg_fail("bad argument");
  const int n = cur->n;
  if (n < 0 || n > kMatchMaxKp) return arg_fail("keypoint count exceeds the matcher capacity (2048)");
  if (n > 0 && (!cur->kps_un || !cur->desc || !cur->uright || !match)) return arg_fail("NULL frame arrays");
  if (nmp > 0 && (!in_view || !proj_x || !proj_y || !proj_xr || !level || !view_cos || !mp_desc ||
                  !mp_nobs))
    return arg_fail("NULL map point arrays");
  for (int i = 0; i < nmp; i++)
    if (in_view[i] && (level[i] < 0 || level[i] >= nlevels)) return arg_fail("level out of range");
  TrackConsts c;
  int rc = make_consts(cam, scale_factors, nullptr, nlevels, &c);
  if (rc) return rc;
  // the kernel sorts the keypoints into per-octave buckets
  for (int i = 0; i < n; i++)
    if (cur->kps_un[i].octave < 0 || cur->kps_un[i].octave >= nlevels)
      return arg_fail("keypoint octave outside the pyramid");
  const int P = std::max(1, n), M = std::max(1, nmp);
  HostStage st;
  LocalArgs a{};
  a.kps_un = st.in(kpd(cur->kps_un), n, P);
  a.desc = st.in(cur->desc, 32 * n, 32 * P);
  a.uright = st.in(cur->uright, n, P);
  a.n = n;
  a.cur_nobs = st.in_opt(cur_nobs, n, P);
  a.nmp = nmp;
  a.in_view = st.in(in_view, nmp, M);
  a.proj_x = st.in(proj_x, nmp, M);
  a.proj_y = st.in(proj_y, nmp, M);
  a.proj_xr = st.in(proj_xr, nmp, M);
  a.level = st.in(level, nmp, M);
  a.view_cos = st.in(view_cos, nmp, M);
  a.mp_desc = st.in(mp_desc, 32 * nmp, 32 * M);
  a.mp_nobs = st.in(mp_nobs, nmp, M);
  a.th = th;
  a.nnratio = nnratio;
  a.match = st.out<int>(P);
  a.nmatches = st.out<int>(1);
  a.scratch = st.out<int4>(M);
  if (st.rc()) return st.rc();
  launch_match_local(c, a, scratch_stream());
  st.launched();
  st.back(match, a.match, n);
  st.back(nmatches, a.nmatches, 1);
  return st.rc();
}

int orbpl_line_frame_prepare(const orbpl_camera* cam, const orbpl_keyline* kl, int n,
                             const float* depth, orbpl_keyline* kl_un, float* dstart, float* dend,
                             float* ur_start, float* ur_end) {
  if (!cam || n < 0 || (n > 0 && (!kl || !kl_un || !dstart || !dend || !ur_start || !ur_end)))
    return arg_fail("bad argument");
  if (n > kLineKeep) return arg_fail("more key lines than LineExtractor keeps (80)");
  TrackConsts c;
  int rc = make_consts(cam, nullptr, nullptr, 1, &c);
  if (rc) return rc;
  if (n == 0) return ORBPL_OK;
  HostStage st;
  const size_t img = (size_t)cam->width * cam->height;
  LineTrackArgs a{};
  a.nl = st.in_value(n);
  a.kl = st.in(kl, n, kLineKeep);
  a.kl_un = st.out<orbpl_keyline>(kLineKeep);
  a.depth = st.in_opt(depth, img, img);
  a.depth_pitch = 0;
  a.dstart = st.out<float>(kLineKeep);
  a.dend = st.out<float>(kLineKeep);
  a.ur_start = st.out<float>(kLineKeep);
  a.ur_end = st.out<float>(kLineKeep);
  a.lmatch = st.out<int>(kLineKeep);
  a.loutlier = st.out<uint8_t>(kLineKeep);
  if (st.rc()) return st.rc();
  launch_line_prepare(c, a, 1, scratch_stream());
  st.launched();
  st.back(kl_un, a.kl_un, n);
  st.back(dstart, a.dstart, n);
  st.back(dend, a.dend, n);
  st.back(ur_start, a.ur_start, n);
  st.back(ur_end, a.ur_end, n);
  return st.rc();
}

int orbl_search_by_projection_last(const orbpl_camera* cam, const float* Tcw, int ncur,
                                   const orbpl_keyline* cur_kl_un, const uint8_t* cur_desc,
                                   int nlast, const orbpl_keyline* last_kl_un,
                                   const uint8_t* has_ml, const uint8_t* last_outlier,
                                   const float* ml_xyz6, const uint8_t* last_desc, int32_t* match,
                                   int* nmatches) {
  if (!cam || !Tcw || !nmatches || ncur < 0 || nlast < 0) return arg_fail("bad argument");
  if (ncur > kLineKeep || nlast > kLineKeep)
    return arg_fail("more key lines than LineExtractor keeps (80)");
  if ((ncur > 0 && (!cur_kl_un || !cur_desc || !match)) ||
      (nlast > 0 && (!last_kl_un || !has_ml || !last_outlier || !ml_xyz6 || !last_desc)))
    return arg_fail("NULL line arrays");
  TrackConsts c;
  int rc = make_consts(cam, nullptr, nullptr, 1, &c);
  if (rc) return rc;
  const int L = kLineKeep;
  StreamState ss{};
  memcpy(ss.Tcw, Tcw, 64);
  ss.has_last = 1;
  HostStage st;
  StreamState* d_ss = st.in_value(ss);
  LineTrackArgs a{};
  a.nl = st.in_value(ncur);
  a.kl_un = st.in(cur_kl_un, ncur, L);
  a.desc = st.in(cur_desc, 32 * ncur, 32 * L);
  a.lmatch = st.out<int>(L);
  a.last_nl = st.in_value(nlast);
  a.last_kl_un = st.in(last_kl_un, nlast, L);
  a.last_has_ml = st.in(has_ml, nlast, L);
  a.last_loutlier = st.in(last_outlier, nlast, L);
  a.last_ml_xyz = st.in(ml_xyz6, 6 * nlast, 6 * L);
  a.last_desc = st.in(last_desc, 32 * nlast, 32 * L);
  if (st.rc()) return st.rc();
  launch_line_match(c, a, d_ss, 1, scratch_stream());
  st.launched();
  st.back(match, a.lmatch, ncur);
  st.back(&ss, d_ss, 1);
  if (st.rc()) return st.rc();
  *nmatches = ss.nlmatches;
  return ORBPL_OK;
}

int orbm_search_by_bow(int nkf, const int32_t* kf_node, const uint8_t* kf_valid,
                       const uint8_t* kf_desc, const float* kf_angle, int nf, const int32_t* f_node,
                       const uint8_t* f_desc, const float* f_angle, float nnratio, int check_ori,
                       int32_t* match, int* nmatches) {
  if (nkf < 0 || nf < 0 || !nmatches) return arg_fail("bad argument");
  if (nkf > 2048 || nf > 2048) return arg_fail("more than 2048 features");
  if ((nkf > 0 && (!kf_node || !kf_valid || !kf_desc || !kf_angle)) ||
      (nf > 0 && (!f_node || !f_desc || !f_angle || !match)))
    return arg_fail("NULL feature arrays");
  for (int i = 0; i < nkf; i++)
    if (kf_node[i] >= (1 << 21) - 1) return arg_fail("vocabulary node id >= 2^21 - 1");
  for (int i = 0; i < nf; i++)
    if (f_node[i] >= (1 << 21) - 1) return arg_fail("vocabulary node id >= 2^21 - 1");
  const int K = std::max(1, nkf), F = std::max(1, nf);
  HostStage st;
  BowArgs a{nkf,
            st.in(kf_node, nkf, K),
            st.in(kf_valid, nkf, K),
            st.in(kf_desc, 32 * nkf, 32 * K),
            st.in(kf_angle, nkf, K),
            nf,
            st.in(f_node, nf, F),
            st.in(f_desc, 32 * nf, 32 * F),
            st.in(f_angle, nf, F),
            nnratio,
            check_ori,
            st.out<int>(F),
            st.out<int>(1)};
  if (st.rc()) return st.rc();
  launch_match_bow(a, scratch_stream());
  st.launched();
  st.back(match, a.match, nf);
  st.back(nmatches, a.nmatches, 1);
  return st.rc();
}

int orbm_search_by_projection_kf_batch_device(const orbpl_camera* cam, const float* scale_factors,
                                              int nlevels, const orbm_kf_device_batch* b,
                                              int batch, float th, int orb_dist, int check_ori,
                                              void* stream) {
  if (!cam || !scale_factors || !b || batch < 0) return arg_fail("bad argument");
  if (b->kp_pitch < 1 || b->kf_pitch < 1 || b->kp_pitch > kMatchMaxKp || b->kf_pitch > kMatchMaxKp)
    return arg_fail("pitch outside [1, 2048] (the matcher capacity)");
  if (!b->d_cur_n || !b->d_Tcw || !b->d_cur_kps_un || !b->d_cur_desc || !b->d_cur_has_mp ||
      !b->d_kf_n || !b->d_kf_angle || !b->d_kf_valid || !b->d_kf_found || !b->d_mp_xyz ||
      !b->d_mp_min_dist || !b->d_mp_max_dist || !b->d_mp_desc || !b->d_match || !b->d_nmatches)
    return arg_fail("NULL device array");
  TrackConsts c;
  int rc = make_consts(cam, scale_factors, nullptr, nlevels, &c);
  if (rc) return rc;
  if (batch == 0) return ORBPL_OK;
  MatchKfArgs a{};
  a.cur_kps_un = kpd(b->d_cur_kps_un);
  a.cur_desc = b->d_cur_desc;
  a.cur_has_mp = b->d_cur_has_mp;
  a.cur_n = b->d_cur_n;
  a.kp_pitch = b->kp_pitch;
  a.kf_angle = b->d_kf_angle;
  a.kf_valid = b->d_kf_valid;
  a.kf_found = b->d_kf_found;
  a.mp_xyz = b->d_mp_xyz;
  a.mp_min_dist = b->d_mp_min_dist;
  a.mp_max_dist = b->d_mp_max_dist;
  a.mp_desc = b->d_mp_desc;
  a.kf_n = b->d_kf_n;
  a.kf_pitch = b->kf_pitch;
  a.Tcw = b->d_Tcw;
  a.pose_stride = 16;
  a.match = b->d_match;
  a.nmatches = b->d_nmatches;
  a.nm_stride = 1;
  a.th = th;
  a.orb_dist = orb_dist;
  a.check_ori = check_ori;
  a.log_scale = log_scale_of(scale_factors, nlevels);
  launch_match_kf(c, a, batch, (hipStream_t)stream);
  HIP_CHECK(hipGetLastError());
  return ORBPL_OK;
}

int orbm_search_by_projection_kf(const orbpl_camera* cam, const float* scale_factors, int nlevels,
                                 const orbpl_match_current* cur, const uint8_t* cur_has_mp,
                                 int nkf, const float* kf_angle, const uint8_t* kf_valid,
                                 const uint8_t* kf_found, const float* mp_xyz,
                                 const float* mp_min_dist, const float* mp_max_dist,
                                 const uint8_t* mp_desc, float th, int orb_dist, int check_ori,
                                 int32_t* match, int* nmatches) {
  if (!cam || !scale_factors || !cur || !nmatches) return arg_fail("NULL argument");
  const int n = cur->n;
  if (n < 0 || nkf < 0 || n > kMatchMaxKp || nkf > kMatchMaxKp)
    return arg_fail("keypoint count exceeds the matcher capacity (2048)");
  if (!cur->Tcw || (n > 0 && (!cur->kps_un || !cur->desc || !cur_has_mp || !match)) ||
      (nkf > 0 && (!kf_angle || !kf_valid || !kf_found || !mp_xyz || !mp_min_dist ||
                   !mp_max_dist || !mp_desc)))
    return arg_fail("NULL feature arrays");
  const int N = std::max(1, n), K = std::max(1, nkf);
  HostStage st;
  orbm_kf_device_batch b{};
  b.kp_pitch = N;
  b.d_cur_n = st.in_value(n);
  b.d_Tcw = st.in(cur->Tcw, 16, 16);
  b.d_cur_kps_un = st.in(cur->kps_un, n, N);
  b.d_cur_desc = st.in(cur->desc, 32 * n, 32 * N);
  b.d_cur_has_mp = st.in(cur_has_mp, n, N);
  b.kf_pitch = K;
  b.d_kf_n = st.in_value(nkf);
  b.d_kf_angle = st.in(kf_angle, nkf, K);
  b.d_kf_valid = st.in(kf_valid, nkf, K);
  b.d_kf_found = st.in(kf_found, nkf, K);
  b.d_mp_xyz = st.in(mp_xyz, 3 * nkf, 3 * K);
  b.d_mp_min_dist = st.in(mp_min_dist, nkf, K);
  b.d_mp_max_dist = st.in(mp_max_dist, nkf, K);
  b.d_mp_desc = st.in(mp_desc, 32 * nkf, 32 * K);
  b.d_match = st.out<int32_t>(N);
  b.d_nmatches = st.out<int32_t>(1);
  if (st.rc()) return st.rc();
  // the device form refuses the rest (nlevels), launches and checks the launch
  int rc = orbm_search_by_projection_kf_batch_device(cam, scale_factors, nlevels, &b, 1, th,
                                                     orb_dist, check_ori, scratch_stream());
  if (rc) return rc;
  st.back(match, b.d_match, n);
  st.back(nmatches, b.d_nmatches, 1);
  return st.rc();
}

int orbpl_stereo_matches(const orbpl_camera* cam, orbx_ctx* left, orbx_ctx* right, int frame,
                         const orbpl_keypoint* kl, const uint8_t* dl, int n,
                         const orbpl_keypoint* kr, const uint8_t* dr, int nr, float* uright,
                         float* depth) {
  if (!cam || !left || !right || n < 0 || nr < 0) return arg_fail("bad argument");
  if (n > 4096 || nr > 4096) return arg_fail("more than 4096 keypoints");
  if ((n > 0 && (!kl || !dl || !uright || !depth)) || (nr > 0 && (!kr || !dr)))
    return arg_fail("NULL keypoint arrays");
  const uint8_t *pl = nullptr, *pr = nullptr;
  const OrbGeom *gl = nullptr, *gr = nullptr;
  hipStream_t sl, sr;
  int rc = orbx_device_pyramid(left, frame, &pl, &gl, &sl);
  if (rc) return rc;
  rc = orbx_device_pyramid(right, frame, &pr, &gr, &sr);
  if (rc) return rc;
  if (gl->nlevels != gr->nlevels || gl->W != gr->W || gl->H != gr->H)
    return arg_fail("left and right extractors differ");
  if (gl->H > 1024) return arg_fail("image taller than 1024 rows");
  if (n == 0) return ORBPL_OK;
  for (int i = 0; i < n; i++)
    if (kl[i].octave < 0 || kl[i].octave >= gl->nlevels)
      return arg_fail("keypoint octave outside the pyramid");
  // the row-band scratch holds exactly the entries of these right keypoints:
  // rows floor(y - 2s) .. ceil(y + 2s) inside the image, as k_stereo counts them
  long long entries = 0;
  for (int i = 0; i < nr; i++) {
    if (kr[i].octave < 0 || kr[i].octave >= gl->nlevels)
      return arg_fail("keypoint octave outside the pyramid");
    const float r = 2.0f * gl->lv[kr[i].octave].scale;
    const float hi = ceilf(kr[i].y + r), lo = floorf(kr[i].y - r);
    if (!(hi >= 0.0f) || !(lo <= (float)(gl->H - 1))) continue;   // no row (or not a number)
    const int maxr = hi > (float)(gl->H - 1) ? gl->H - 1 : (int)hi;
    const int minr = lo < 0.0f ? 0 : (int)lo;
    entries += maxr - minr + 1;
  }
  HIP_CHECK(hipStreamSynchronize(sl));
  HIP_CHECK(hipStreamSynchronize(sr));
  const int R = std::max(1, nr), cap = (int)std::max(1LL, entries);
  HostStage st;
  StereoArgs a{};
  a.n = n;
  a.kl = st.in(kpd(kl), n, n);
  a.dl = st.in(dl, 32 * n, 32 * n);
  a.nr = nr;
  a.kr = st.in(kpd(kr), nr, R);
  a.dr = st.in(dr, 32 * nr, 32 * R);
  a.pyrL = pl;
  a.pyrR = pr;
  stereo_set_levels(a, *gl);
  a.mb = cam->bf / cam->fx;
  a.mbf = cam->bf;
  a.uright = st.out<float>(n);
  a.depth = st.out<float>(n);
  a.sad = st.out<int>(n);
  a.entries = st.out<uint16_t>(cap);
  a.entry_cap = cap;
  a.err = st.zeros<int>(1);
  if (st.rc()) return st.rc();
  launch_stereo(a, 1, scratch_stream());
  st.launched();
  int err = 0;
  st.back(&err, a.err, 1);
  if (st.rc()) return st.rc();
  if (err) return (arg_fail("stereo row band capacity exceeded"), ORBPL_ERR_OVERFLOW);
  st.back(uright, a.uright, n);
  st.back(depth, a.depth, n);
  return st.rc();
}

int orbl_frame_is_in_frustum(const float* Tcw, int n, const float* xyz6, uint8_t* in_view) {
  if (!Tcw || n < 0 || (n > 0 && (!xyz6 || !in_view))) return arg_fail("bad argument");
  if (n == 0) return ORBPL_OK;
  const size_t N = n;
  HostStage st;
  const float* d_T = st.in(Tcw, 16, 16);
  const float* d_xyz = st.in(xyz6, 6 * N, 6 * N);
  uint8_t* d_view = st.out<uint8_t>(N);
  if (st.rc()) return st.rc();
  launch_line_in_frustum(d_T, n, d_xyz, d_view, scratch_stream());
  st.launched();
  st.back(in_view, d_view, n);
  return st.rc();
}

int orbl_search_by_projection_list(const orbpl_camera* cam, const float* Tcw, int ncur,
                                   const orbpl_keyline* cur_kl_un, const uint8_t* cur_desc,
                                   const int32_t* cur_nobs, int nml, const uint8_t* valid,
                                   const float* ml_xyz6, const uint8_t* ml_desc, int32_t* match,
                                   int* nmatches, int* wiped) {
  if (!cam || !Tcw || !nmatches || ncur < 0 || nml < 0) return arg_fail("bad argument");
  if (ncur > kLineKeep) return arg_fail("more key lines than LineExtractor keeps (80)");
  if ((ncur > 0 && (!cur_kl_un || !cur_desc || !match)) ||
      (nml > 0 && (!valid || !ml_xyz6 || !ml_desc)))
    return arg_fail("NULL line arrays");
  TrackConsts c;
  int rc = make_consts(cam, nullptr, nullptr, 1, &c);
  if (rc) return rc;
  const int L = kLineKeep, M = std::max(1, nml);
  HostStage st;
  LineListArgs a{};
  a.Tcw = st.in(Tcw, 16, 16);
  a.ncur = ncur;
  a.cur_kl_un = st.in(cur_kl_un, ncur, L);
  a.cur_desc = st.in(cur_desc, 32 * ncur, 32 * L);
  a.cur_nobs = st.in_opt(cur_nobs, ncur, L);
  a.nml = nml;
  a.valid = st.in(valid, nml, M);
  a.ml_xyz6 = st.in(ml_xyz6, 6 * nml, 6 * M);
  a.ml_desc = st.in(ml_desc, 32 * nml, 32 * M);
  a.proj_kl = st.out<orbpl_keyline>(M);
  a.proj_src = st.out<int>(M);
  a.match = st.out<int>(L);
  a.nmatches = st.out<int>(1);
  a.wiped = st.out<int>(1);
  if (st.rc()) return st.rc();
  launch_line_match_list(c, a, scratch_stream());
  st.launched();
  st.back(match, a.match, ncur);
  st.back(nmatches, a.nmatches, 1);
  if (wiped) st.back(wiped, a.wiped, 1);
  return st.rc();
}

int orbl_search_by_projection_pairs(const orbpl_camera* cam, const float* Tcw, int mode, int ncur,
                                    const orbpl_keyline* cur_kl_un, const uint8_t* cur_desc,
                                    const int32_t* cur_nobs, int nml, const uint8_t* valid,
                                    const orbpl_keyline* base_kl, const float* ml_xyz6,
                                    const uint8_t* ml_desc, const int32_t* ml_nobs,
                                    orbpl_keyline* proj_kl, int32_t* proj_src, int* nproj,
                                    int32_t* pairs, int pair_cap, int* npairs, int32_t* match,
                                    int* nmatches, int* wiped) {
  if (!cam || !Tcw || !nmatches || !nproj || !npairs || !wiped || ncur < 0 || nml < 0 ||
      pair_cap < 0 || (mode != 0 && mode != 1))
    return arg_fail("bad argument");
  if (ncur > kLineKeep) return arg_fail("more key lines than LineExtractor keeps (80)");
  if ((ncur > 0 && (!cur_kl_un || !cur_desc || !match)) ||
      (nml > 0 && (!valid || !ml_xyz6 || !ml_desc || !proj_kl || !proj_src)) ||
      (pair_cap > 0 && !pairs))
    return arg_fail("NULL line arrays");
  TrackConsts c;
  int rc = make_consts(cam, nullptr, nullptr, 1, &c);
  if (rc) return rc;
  const size_t L = kLineKeep, M = std::max(1, nml), words = (size_t)(nml + 31) / 32;
  HostStage st;
  LinePairArgs a{};
  a.Tcw = st.in(Tcw, 16, 16);
  a.mode = mode;
  a.ncur = ncur;
  a.cur_kl_un = st.in(cur_kl_un, ncur, L);
  a.cur_desc = st.in(cur_desc, 32 * ncur, 32 * L);
  a.cur_nobs = st.in_opt(cur_nobs, ncur, L);
  a.nml = nml;
  a.valid = st.in(valid, nml, M);
  a.base_kl = st.in_opt(base_kl, nml, M);
  a.ml_xyz6 = st.in(ml_xyz6, 6 * nml, 6 * M);
  a.ml_desc = st.in(ml_desc, 32 * nml, 32 * M);
  a.ml_nobs = st.in_opt(ml_nobs, nml, M);
  a.proj_kl = st.out<orbpl_keyline>(M);
  a.proj_src = st.out<int>(M);
  a.nproj = st.out<int>(1);
  a.okbits = st.out<unsigned>(std::max<size_t>(1, L * words));
  a.pairs = st.out<int>(2 * std::max<size_t>(1, pair_cap));
  a.pair_cap = pair_cap;
  a.npairs = st.out<int>(1);
  a.match = st.out<int>(L);
  a.nmatches = st.out<int>(1);
  a.wiped = st.out<int>(1);
  if (st.rc()) return st.rc();
  launch_line_pairs(c, a, scratch_stream());
  st.launched();
  int np = 0, npr = 0;
  st.back(&np, a.nproj, 1);
  st.back(&npr, a.npairs, 1);
  st.back(proj_kl, a.proj_kl, np);
  st.back(proj_src, a.proj_src, np);
  st.back(pairs, a.pairs, 2 * (size_t)std::max(0, std::min(npr, pair_cap)));
  st.back(match, a.match, ncur);
  st.back(nmatches, a.nmatches, 1);
  st.back(wiped, a.wiped, 1);
  if (st.rc()) return st.rc();
  *nproj = np;
  *npairs = npr;
  return ORBPL_OK;
}

int orbl_match_bf_knn(int nq, const uint8_t* qdesc, int nt, const uint8_t* tdesc, int32_t* out,
                      int* nmatches) {
  if (nq < 0 || nt < 0 || !nmatches) return arg_fail("bad argument");
  if (nq > 256) return arg_fail("more than 256 query descriptors");
  if ((nq > 0 && !qdesc) || (nt > 0 && (!tdesc || !out))) return arg_fail("NULL descriptor arrays");
  const int Q = std::max(1, nq), T = std::max(1, nt);
  HostStage st;
  const uint8_t* d_q = st.in(qdesc, 32 * nq, 32 * Q);
  const uint8_t* d_t = st.in(tdesc, 32 * nt, 32 * T);
  int* d_out = st.out<int>(T);
  int* d_n = st.out<int>(1);
  if (st.rc()) return st.rc();
  launch_line_bf_knn(nq, d_q, nt, d_t, d_out, d_n, scratch_stream());
  st.launched();
  st.back(out, d_out, nt);
  st.back(nmatches, d_n, 1);
  return st.rc();
}

int orbl_stereo_line_depths(const orbpl_camera* cam, const orbpl_keyline* kl, const uint8_t* desc,
                            int nl, const orbpl_keyline* kr, const uint8_t* desc_r, int nr,
                            float* dstart, float* dend) {
  if (!cam || nl < 0 || nr < 0) return arg_fail("bad argument");
  if (nl > kLineKeep || nr > kLineKeep)
    return arg_fail("more key lines than LineExtractor keeps (80)");
  if ((nl > 0 && (!kl || !desc || !dstart || !dend)) || (nr > 0 && (!kr || !desc_r)))
    return arg_fail("NULL line arrays");
  TrackConsts c;
  int rc = make_consts(cam, nullptr, nullptr, 1, &c);
  if (rc) return rc;
  if (nl == 0) return ORBPL_OK;
  const int L = kLineKeep;
  HostStage st;
  StereoLineArgs a{};
  a.nl = st.in_value(nl);
  a.kl = st.in(kl, nl, L);
  a.desc = st.in(desc, 32 * nl, 32 * L);
  a.nr = st.in_value(nr);
  a.kr = st.in(kr, nr, L);
  a.desc_r = st.in(desc_r, 32 * nr, 32 * L);
  a.dstart = st.out<float>(L);
  a.dend = st.out<float>(L);
  if (st.rc()) return st.rc();
  launch_stereo_lines(c, a, 1, scratch_stream());
  st.launched();
  st.back(dstart, a.dstart, nl);
  st.back(dend, a.dend, nl);
  return st.rc();
}

}  // extern "C"
