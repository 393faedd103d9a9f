// Stand-alone check of the host side of orblm_search_in_neighbors / orbm_fuse
// (make fuse_check, host code under AddressSanitizer + UBSan): the map
// validation, the flattening of the maps into the staged pools and the failure
// path of a machine without a device, where the first hipMalloc fails after the
// pools were packed. With a device present the refusals are still checked.
// The library's reporters and the camera constants (track_host.cpp) are
// replaced by stand-ins: they are not what is under test.
#include <cstring>
#include <vector>

#include "search_neighbors.hip"
#include "check_common.h"

int orbpl::make_consts(const orbpl_camera* cam, const float* scale, const float* inv_sigma2,
                       int nlevels, TrackConsts* out) {
  TrackConsts c{};
  c.fx = cam->fx; c.fy = cam->fy; c.cx = cam->cx; c.cy = cam->cy; c.bf = cam->bf;
  c.maxX = (float)cam->width;
  c.maxY = (float)cam->height;
  c.gridInvW = kGridCols / c.maxX;
  c.gridInvH = kGridRows / c.maxY;
  c.nlevels = nlevels;
  for (int l = 0; l < nlevels; l++) {
    c.scale[l] = scale[l];
    c.inv_sigma2[l] = inv_sigma2[l];
  }
  *out = c;
  return ORBPL_OK;
}
float orbpl::log_scale_of(const float*, int) { return 0.18232156f; }

namespace {

const orbpl_camera kCam = {517.f, 516.f, 318.f, 255.f, 0, 0, 0, 0, 0, 40.f, 3.f, 640, 480};
const float kScale[8] = {1, 1.2f, 1.44f, 1.728f, 2.0736f, 2.48832f, 2.985984f, 3.5831808f};
const float kSigma2[8] = {1, 1.44f, 2.0736f, 2.985984f, 4.2998f, 6.1917f, 8.9161f, 12.8392f};

int sin_call(TinyMap& t, int cur = 0, int nlevels = 8) {
  orblm_sin_problem p{};
  p.map = t.m;
  p.cur = cur;
  return orblm_search_in_neighbors(&kCam, kScale, kSigma2, nlevels, &p, 1);
}

}  // namespace

int main() {
  // the map of two keyframes
#define REFUSED(edit, text)                      \
  do {                                           \
    TinyMap t(2);                                \
    edit;                                        \
    EXPECT(sin_call(t) == ORBPL_ERR_ARG);        \
    EXPECT(g_msg == text);                       \
  } while (0)
  REFUSED(t.mp[1][2] = 0, "map point twice in one keyframe");
  REFUSED(t.kf[1].id = t.kf[0].id, "two keyframes of a map with one id");
  REFUSED(t.kp[0][2].octave = 8, "keypoint octave outside [0, nlevels)");
  REFUSED(t.mp[0][1] = 2, "slot index outside [-1, M)");
  REFUSED(t.mp[0][1] = -2, "slot index outside [-1, M)");
  REFUSED(t.ref[1] = 0, "good map point whose ref_kf does not observe it");
  REFUSED(t.ref[1] = 77, "good map point whose ref_kf does not observe it");
  REFUSED(t.kf_ord[0][0] = 2, "ordered entry outside the table or naming its own keyframe");
  REFUSED(t.kf_ord[1][0] = 1, "ordered entry outside the table or naming its own keyframe");
  REFUSED(t.m.nkf = 65, "map with no keyframe or more than 64");
  REFUSED(t.m.M = 64 * 2048 + 1, "map points outside [0, 64 * 2048]");
  REFUSED(t.m.obs = nullptr, "NULL map point arrays");
  REFUSED(t.kf[0].n = 2049, "keyframe with more than 2048 features");
  REFUSED(t.kf[0].mp = nullptr, "NULL keyframe arrays");
  REFUSED(t.kf[0].Tcw = nullptr, "NULL keyframe pose");
  {
    TinyMap t(2);
    EXPECT(sin_call(t, 2) == ORBPL_ERR_ARG && g_msg == "current keyframe outside the table");
    EXPECT(sin_call(t, 0, 17) == ORBPL_ERR_ARG && g_msg == "nlevels outside [1, 16]");
    orblm_sin_problem two[2] = {};
    two[0].map = two[1].map = t.m;
    EXPECT(orblm_search_in_neighbors(&kCam, kScale, kSigma2, 8, two, 2) == ORBPL_ERR_ARG);
    EXPECT(g_msg == "a keyframe or point array belongs to two problems");
    int nf = 0;
    int32_t lst[3] = {0, -1, 2}, bi[3], bd[3], rs[3];
    EXPECT(orbm_fuse(&kCam, kScale, kSigma2, 8, &t.m, 0, lst, 3, 3.0f, &nf, bi, bd, rs) == ORBPL_ERR_ARG);
    EXPECT(g_msg == "list entry outside [-1, M)");
    EXPECT(orbm_fuse(&kCam, kScale, kSigma2, 8, &t.m, 2, lst, 2, 3.0f, &nf, bi, bd, rs) == ORBPL_ERR_ARG);
    EXPECT(orbm_fuse(&kCam, kScale, kSigma2, 8, &t.m, 0, nullptr, 2, 3.0f, &nf, bi, bd, rs) == ORBPL_ERR_ARG);
  }
  // a valid map: packed into the pools, then staged
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) {
    printf("a device is present: the refusals hold, the staging failure path was not run\n");
    return 0;
  }
  {
    TinyMap t(2);
    const TinyMap before(2);
    EXPECT(sin_call(t) == ORBPL_ERR_HIP);
    EXPECT(!memcmp(t.mp, before.mp, sizeof(t.mp)) && !memcmp(t.bad, before.bad, sizeof(t.bad)));
    int nf = -1;
    int32_t lst[2] = {1, -1}, bi[2], bd[2], rs[2];
    EXPECT(orbm_fuse(&kCam, kScale, kSigma2, 8, &t.m, 0, lst, 2, 3.0f, &nf, bi, bd, rs) == ORBPL_ERR_HIP);
    EXPECT(nf == -1);
    EXPECT(orblm_search_in_neighbors(&kCam, kScale, kSigma2, 8, nullptr, 0) == ORBPL_OK);
  }
  printf("search_neighbors_check: ok\n");
  return 0;
}
