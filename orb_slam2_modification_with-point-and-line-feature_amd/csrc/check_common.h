// What the stand-alone host checks share (fuse_check, cull_check, pool_check):
// stand-ins for the library's reporters, EXPECT and the hand-built map.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>

#include "orbpl_runtime.h"

static std::string g_msg;   // the last message reported

int orbpl::hip_fail(hipError_t e, const char* what, int) {
  g_msg = std::string(what) + ": " + hipGetErrorString(e);
  return ORBPL_ERR_HIP;
}
int orbpl::arg_fail(const char* msg) {
  g_msg = msg;
  return ORBPL_ERR_ARG;
}

#define EXPECT(cond)                                                          \
  do {                                                                        \
    if (!(cond)) {                                                            \
      printf("FAILED line %d: %s (last: %s)\n", __LINE__, #cond, g_msg.c_str()); \
      return 1;                                                               \
    }                                                                         \
  } while (0)

// three keyframes (ids 0, 5, 9) of three features, two points: point 0 in all
// three, point 1 in the second, the third keyframe without an ordered list;
// TinyMap(2) is the map of the first two
struct TinyMap {
  float T[3][16] = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1},
                    {1, 0, 0, -0.2f, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1},
                    {1, 0, 0, -0.4f, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}};
  orbpl_keypoint kp[3][3] = {};
  float ur[3][3] = {{300, -1, 100}, {290, 50, -1}, {280, -1, -1}};
  uint8_t kdesc[3][3 * 32] = {};
  int32_t mp[3][3] = {{0, -1, -1}, {0, 1, -1}, {0, -1, -1}};
  int32_t kf_ord[2][3] = {{1, -1, -1}, {0, -1, -1}};
  orblm_map_keyframe kf[3];
  float xyz[6] = {0, 0, 4, 0.5f, 0, 5}, normal[6] = {0, 0, 1, 0, 0, 1};
  float mind[2] = {1, 1}, maxd[2] = {10, 10};
  uint8_t desc[64] = {}, bad[2] = {0, 0};
  int32_t ref[2] = {0, 1}, vis[2] = {3, 4}, found[2] = {2, 2}, rep[2], nobs[2], src[4];
  int16_t obs[128];
  orblm_map m;

  explicit TinyMap(int nkf = 3) {
    for (int k = 0; k < 3; k++) {
      for (int i = 0; i < 3; i++) kp[k][i].x = 320.f + 10 * i, kp[k][i].y = 240.f;
      kf[k] = {k == 0 ? 0 : 4 * k + 1, T[k], 3, kp[k], ur[k], kdesc[k], mp[k], k < 2 ? kf_ord[k] : nullptr};
    }
    m = {nkf, kf, 2, xyz, normal, mind, maxd, desc, ref, bad, vis, found, rep, nobs, obs, src};
  }
};
