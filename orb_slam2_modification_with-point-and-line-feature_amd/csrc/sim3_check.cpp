// Stand-alone check of the host side of the Sim3 solver (make sim3_check, host
// code under AddressSanitizer + UBSan): the parameter table, orbsim3_setup and
// its refusals, the validation of orbsim3_iterate, its packing into the staged
// pools and the failure path of a machine without a device, where the first
// hipMalloc fails after the pools were packed. With a device present the
// refusals are still checked. orbpnp_iterate (pnp.hip) and orbkf_detect_reloc
// (kfdb.hip) get the same failure-path block. The library's reporters are
// check_common.h's stand-ins: they are not what is under test.
#include <cstring>
#include <vector>

#include "sim3.hip"
#include "pnp.hip"
#include "kfdb.hip"
#include "check_common.h"

namespace {

// keyframe 1 of six features, keyframe 2 of four: feature 0 matched to 2,
// 1 unmatched, 2 matched to a point keyframe 2 does not observe, 3 without a
// point of its own, 4 matched to a bad point, 5 matched to 0
struct TinyPair {
  int32_t matched12[6] = {2, -1, -2, 1, 3, 0};
  uint8_t valid1[6] = {1, 1, 1, 0, 1, 1};
  float xyz1[18] = {0, 0, 4, 1, 0, 5, 0, 1, 6, 1, 1, 4, -1, 0, 5, 0.5f, -0.5f, 3};
  int32_t octave1[6] = {0, 1, 2, 3, 4, 7};
  uint8_t valid2[4] = {1, 1, 1, 0};
  float xyz2[12] = {0.5f, -0.5f, 3, 1, 1, 4, 0, 0, 4, -1, 0, 5};
  int32_t octave2[4] = {1, 0, 3, 2};
  float T1[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  float T2[16] = {1, 0, 0, -0.25f, 0, 1, 0, 0, 0, 0, 1, 0.5f, 0, 0, 0, 1};
  int32_t n = -1, ind[6], me1[6], me2[6];
  float X1[18], X2[18], i1[12], i2[12];
  orbsim3_pair pair() {
    return {6, matched12, valid1, xyz1, octave1, 4, valid2, xyz2, octave2, T1, T2,
            500.f, 500.f, 320.f, 240.f, &n, ind, X1, X2, i1, i2, me1, me2};
  }
};

// one solver over four correspondences
struct TinyProblem {
  float X1[12] = {0, 0, 4, 1, 0, 5, 0, 1, 6, 1, 1, 4}, X2[12] = {0, 0, 4, 1, 0, 5, 0, 1, 6, 1, 1, 4};
  float i1[8] = {320, 240, 420, 240, 320, 323, 445, 365}, i2[8] = {320, 240, 420, 240, 320, 323, 445, 365};
  int32_t m1[4] = {9, 9, 9, 9}, m2[4] = {9, 9, 9, 9};
  int32_t draws[15] = {};
  int32_t it = 0, best = 0, res = 7, nm = 7, ni = 7, dc = 7;
  uint8_t bm[4] = {}, inl[4] = {9, 9, 9, 9};
  float bT[16] = {}, bR[9] = {}, bt[3] = {}, bs = 0, T[16];
  orbsim3_problem problem() {
    return {500.f, 500.f, 320.f, 240.f, 4, X1, X2, i1, i2, m1, m2, 3, 5, 0, 15, draws,
            &it, &best, bm, bT, bR, bt, &bs, T, &res, &nm, &ni, inl, &dc};
  }
};

}  // namespace

int main() {
  // SetRansacParameters (:114-138) with 0.99 / 20 / 300
  int32_t its = 0;
  EXPECT(orbsim3_ransac_parameters(25, 0.99, 20, 300, &its) == ORBPL_OK && its == 7);
  EXPECT(orbsim3_ransac_parameters(100, 0.99, 20, 300, &its) == ORBPL_OK && its == 300);
  EXPECT(orbsim3_ransac_parameters(20, 0.99, 20, 300, &its) == ORBPL_OK && its == 1);
  EXPECT(orbsim3_ransac_parameters(0, 0.99, 20, 300, &its) == ORBPL_OK && its == 1);
  EXPECT(orbsim3_ransac_parameters(-1, 0.99, 20, 300, &its) == ORBPL_ERR_ARG);
  EXPECT(orbsim3_ransac_parameters(5, 0.99, 20, 300, nullptr) == ORBPL_ERR_ARG);

  const float sigma2[8] = {1.0f, 1.44f, 2.0736f, 2.985984f, 4.299817f, 6.1917367f, 8.916101f,
                           12.839185f};
  {
    TinyPair t;
    orbsim3_pair p = t.pair();
    EXPECT(orbsim3_setup(&p, 1, sigma2, 8) == ORBPL_OK);
    EXPECT(t.n == 2 && t.ind[0] == 0 && t.ind[1] == 5);
    EXPECT(t.me1[0] == 9 && t.me2[0] == 27 && t.me1[1] == 118 && t.me2[1] == 13);
    EXPECT(t.X1[2] == 4.f && t.X2[0] == -0.25f && t.X2[2] == 4.5f && t.i1[0] == 320.f);
    EXPECT(orbsim3_setup(nullptr, 0, sigma2, 8) == ORBPL_OK);
  }
#define SETUP_REFUSED(edit, text)                              \
  do {                                                         \
    TinyPair t;                                                \
    orbsim3_pair p = t.pair();                                 \
    edit;                                                      \
    EXPECT(orbsim3_setup(&p, 1, sigma2, 8) == ORBPL_ERR_ARG);  \
    EXPECT(g_msg == text);                                     \
  } while (0)
  SETUP_REFUSED(p.n1 = 2049, "keyframe with more than 2048 features");
  SETUP_REFUSED(p.n2 = 2049, "keyframe with more than 2048 features");
  SETUP_REFUSED(t.matched12[1] = 4, "matched12 entry outside [-2, n2)");
  SETUP_REFUSED(t.matched12[1] = -3, "matched12 entry outside [-2, n2)");
  SETUP_REFUSED(t.octave1[1] = 8, "keypoint octave outside [0, nlevels)");
  SETUP_REFUSED(t.octave2[3] = -1, "keypoint octave outside [0, nlevels)");
  SETUP_REFUSED(p.Tcw2 = nullptr, "NULL pose or count");
  SETUP_REFUSED(p.valid1 = nullptr, "NULL keyframe 1 or output arrays");
  SETUP_REFUSED(p.max_error2 = nullptr, "NULL keyframe 1 or output arrays");
  SETUP_REFUSED(p.xyz2 = nullptr, "NULL keyframe 2 arrays");
  {
    TinyPair t;
    orbsim3_pair p = t.pair();
    EXPECT(orbsim3_setup(&p, 1, sigma2, 17) == ORBPL_ERR_ARG && g_msg == "nlevels outside [1, 16]");
    EXPECT(orbsim3_setup(&p, 1, nullptr, 8) == ORBPL_ERR_ARG && g_msg == "NULL level_sigma2");
    orbsim3_setup_device_batch b{};
    EXPECT(orbsim3_setup_batch_device(&b, 1, nullptr) == ORBPL_ERR_ARG && g_msg == "NULL device array");
    EXPECT(orbsim3_setup_batch_device(&b, 0, nullptr) == ORBPL_OK);
    orbsim3_device_batch d{};
    EXPECT(orbsim3_iterate_batch_device(&d, 1, 5, nullptr) == ORBPL_ERR_ARG && g_msg == "NULL device array");
    EXPECT(orbsim3_iterate_batch_device(nullptr, 1, 5, nullptr) == ORBPL_ERR_ARG);
  }
#define ITER_REFUSED(edit, nit, text)                       \
  do {                                                      \
    TinyProblem t;                                          \
    orbsim3_problem p = t.problem();                        \
    edit;                                                   \
    EXPECT(orbsim3_iterate(&p, 1, nit) == ORBPL_ERR_ARG);   \
    EXPECT(g_msg == text);                                  \
  } while (0)
  ITER_REFUSED(p.n = 2049, 5, "more than 2048 correspondences");
  ITER_REFUSED(p.min_inliers = 2, 5, "min_inliers below the minimal set of 3");
  ITER_REFUSED(p.best_s = nullptr, 5, "NULL state or output");
  ITER_REFUSED(p.P2im2 = nullptr, 5, "NULL correspondence arrays");
  ITER_REFUSED(t.it = -1, 5, "negative iteration count");
  ITER_REFUSED(p.max_its = 400, 321, "more hypotheses in one call than ORBSIM3_MAX_ITERATIONS");
  ITER_REFUSED(p.n_draws = 14, 5, "fewer draws than 3 per hypothesis");
  ITER_REFUSED(p.draws = nullptr, 5, "fewer draws than 3 per hypothesis");
  EXPECT(orbsim3_iterate(nullptr, 0, 5) == ORBPL_OK);

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) {
    printf("a device is present: the refusals hold, the staging failure path was not run\n");
    return 0;
  }
  {
    // valid problems, one of them exhausted (needs no draws): packed, then the
    // staging fails and nothing of the caller's is written
    TinyProblem t, u;
    u.it = 5;
    orbsim3_problem two[2] = {t.problem(), u.problem()};
    two[1].n_draws = 0;
    two[1].draws = nullptr;
    EXPECT(orbsim3_iterate(two, 2, 5) == ORBPL_ERR_HIP);
    EXPECT(t.it == 0 && t.res == 7 && t.nm == 7 && t.ni == 7 && t.dc == 7 && t.inl[0] == 9);
    EXPECT(u.it == 5 && u.res == 7 && u.bs == 0);
  }
  {
    // the same for orbpnp_iterate: an empty problem and one of five points
    float p2[10] = {}, p3[15] = {}, me[5] = {}, bT[2][16] = {}, T[2][16];
    int32_t draws[8] = {}, it[2] = {0, 0}, bi[2] = {0, 0}, out[8] = {7, 7, 7, 7, 7, 7, 7, 7};
    uint8_t bm[5] = {}, inl[5] = {9, 9, 9, 9, 9};
    T[0][0] = T[1][0] = 7.f;
    orbpnp_problem two[2] = {
        {500, 500, 320, 240, 0, nullptr, nullptr, nullptr, 4, 10, nullptr, 0, nullptr, &it[0], &bi[0],
         nullptr, bT[0], T[0], &out[0], &out[1], &out[2], nullptr, &out[3]},
        {500, 500, 320, 240, 5, p2, nullptr, p3, 4, 2, me, 8, draws, &it[1], &bi[1], bm, bT[1], T[1],
         &out[4], &out[5], &out[6], inl, &out[7]}};
    EXPECT(orbpnp_iterate(two, 2, 2) == ORBPL_ERR_HIP);
    for (int i = 0; i < 8; i++) EXPECT(out[i] == 7);
    EXPECT(it[0] == 0 && it[1] == 0 && bi[1] == 0 && T[0][0] == 7.f && T[1][0] == 7.f && inl[0] == 9);
  }
  {
    // and for orbkf_detect_reloc: an empty database and one of two keyframes
    const int32_t off[3] = {0, 1, 4};
    int32_t covis[20], cand[2][64], nc[2] = {7, 7}, cw[2] = {7, 7};
    const uint32_t words[4] = {5, 2, 6, 9}, qw[2] = {2, 9};
    const double vals[4] = {0.5, 0.25, 0.125, 0.0625}, qv[2] = {0.75, 0.375};
    float rs[2] = {1.5f, 2.5f};
    for (int i = 0; i < 20; i++) covis[i] = -1;
    cand[0][0] = cand[1][0] = 7;
    orbkf_problem two[2] = {
        {0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, cand[0], &nc[0], nullptr},
        {2, off, words, vals, covis, rs, 2, qw, qv, cand[1], &nc[1], cw}};
    EXPECT(orbkf_detect_reloc(two, 2, 0) == ORBPL_ERR_HIP);
    EXPECT(nc[0] == 7 && nc[1] == 7 && cw[0] == 7 && cand[0][0] == 7 && cand[1][0] == 7 && rs[0] == 1.5f &&
           rs[1] == 2.5f);
  }
  printf("sim3_check: ok\n");
  return 0;
}
