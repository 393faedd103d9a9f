// Stand-alone check of Rows (host_stage.h) and the pack structs of host_rows.h
// (make rows_check, host code under AddressSanitizer + UBSan, no device call).
// Every struct is built from two hand-built problems of different shape, one of
// them empty: each column row against the values written out here (the input
// where a problem fills it, the pad elsewhere), then the unpack of hand-filled
// out columns into the callers' arrays, whose entries past n are guards.
#include <cstring>
#include <vector>

#include "host_rows.h"
#include "check_common.h"

using namespace orbpl;

// row r of c: its first n elements are src's, the rest the pad
template <class T>
static bool row_is(const Rows<T>& c, size_t r, const T* src, size_t n, T pad = T()) {
  if (r >= c.rows || n > c.row || c.h.size() != c.rows * c.row) return false;
  for (size_t i = 0; i < c.row; i++)
    if (memcmp(&c.h[r * c.row + i], i < n ? &src[i] : &pad, sizeof(T))) return false;
  return true;
}
template <class T>
static bool is(const Rows<T>& c, std::initializer_list<typename std::vector<T>::value_type> want) {
  return c.h == std::vector<T>(want);
}
// every element of a column becomes base + its index
template <class T>
static void count_up(Rows<T>& c, int base) {
  for (size_t i = 0; i < c.h.size(); i++) c.h[i] = (T)(base + (int)i);
}

static int check_rows() {
  const int32_t v[3] = {7, 8, 9};
  Rows<int32_t> c(2, 3, -1);
  EXPECT(c.rows == 2 && c.row == 3 && c.d == nullptr && is(c, {-1, -1, -1, -1, -1, -1}));
  c.put(0, nullptr, 0);
  c.put(1, v, 3);                                  // n == row
  EXPECT(is(c, {-1, -1, -1, 7, 8, 9}));
  c.put(0, v + 1, 1);                              // the pad survives past n
  EXPECT(is(c, {8, -1, -1, 7, 8, 9}));
  c.at(0, 2) = 5;
  EXPECT(c.at(1) == 7 && is(c, {8, -1, 5, 7, 8, 9}));
  int32_t dst[4] = {1, 2, 3, 4};
  c.take(0, nullptr, 0);
  c.take(0, dst, 1);
  EXPECT(dst[0] == 8 && dst[1] == 2);
  c.take(1, dst, 3);
  EXPECT(dst[0] == 7 && dst[1] == 8 && dst[2] == 9 && dst[3] == 4);
  Rows<uint8_t> e(0, 4), one(3, 1, 1);
  EXPECT(e.h.empty() && is(one, {1, 1, 1}));
  e.put(0, nullptr, 0);
  return 0;
}

static int check_pnp() {
  // A: n = 0 (below min_inliers, no draws); B: n = 5, two hypotheses' draws
  float p2[10], p3[15], me[5], bTA[16], bTB[16], TA[16] = {}, TB[16] = {};
  for (int i = 0; i < 15; i++) p3[i] = 100.f + i;
  for (int i = 0; i < 10; i++) p2[i] = 200.f + i;
  for (int i = 0; i < 5; i++) me[i] = 300.f + i;
  for (int i = 0; i < 16; i++) bTA[i] = 1.f + i, bTB[i] = 20.f + i;
  const int32_t draws[8] = {11, 12, 13, 14, 15, 16, 17, 18};
  int32_t itA = 3, biA = 4, itB = 1, biB = 2, out[8] = {-9, -9, -9, -9, -9, -9, -9, -9};
  uint8_t bm[6] = {1, 0, 1, 0, 1, 77}, inl[6] = {9, 9, 9, 9, 9, 77};
  orbpnp_problem P[2] = {
      {500, 501, 320, 240, 0, nullptr, nullptr, nullptr, 4, 10, nullptr, 0, nullptr, &itA, &biA, nullptr,
       bTA, TA, &out[0], &out[1], &out[2], nullptr, &out[3]},
      {600, 601, 321, 241, 5, p2, nullptr, p3, 4, 10, me, 8, draws, &itB, &biB, bm, bTB, TB, &out[4],
       &out[5], &out[6], inl, &out[7]}};
  PnpRows R(P, 2, 5, 8, {0, 8});
  const float camA[4] = {500, 501, 320, 240}, camB[4] = {600, 601, 321, 241};
  EXPECT(is(R.n, {0, 5}) && is(R.min_inliers, {4, 4}) && is(R.max_its, {10, 10}));
  EXPECT(is(R.iterations, {3, 1}) && is(R.best_inliers, {4, 2}));
  EXPECT(row_is(R.cam, 0, camA, 4) && row_is(R.cam, 1, camB, 4));
  EXPECT(row_is(R.best_Tcw, 0, bTA, 16) && row_is(R.best_Tcw, 1, bTB, 16));
  EXPECT(row_is(R.draws, 0, draws, 0) && row_is(R.draws, 1, draws, 8));
  EXPECT(row_is(R.p2d, 0, p2, 0) && row_is(R.p2d, 1, p2, 10) && row_is(R.p3d, 0, p3, 0) &&
         row_is(R.p3d, 1, p3, 15));
  EXPECT(row_is(R.max_error, 0, me, 0) && row_is(R.max_error, 1, me, 5));
  EXPECT(row_is(R.best_mask, 0, bm, 0) && row_is(R.best_mask, 1, bm, 5));
  EXPECT(R.Tcw.h.size() == 32 && R.inliers.h.size() == 10 && R.result.h.size() == 2 &&
         R.no_more.h.size() == 2 && R.n_inliers.h.size() == 2 && R.draws_consumed.h.size() == 2);
  count_up(R.iterations, 30), count_up(R.best_inliers, 40), count_up(R.result, 50);
  count_up(R.no_more, 60), count_up(R.n_inliers, 70), count_up(R.draws_consumed, 80);
  count_up(R.Tcw, 100), count_up(R.best_Tcw, 200), count_up(R.inliers, 2), count_up(R.best_mask, 20);
  R.unpack();
  EXPECT(itA == 30 && biA == 40 && itB == 31 && biB == 41);
  EXPECT(out[0] == 50 && out[1] == 60 && out[2] == 70 && out[3] == 80);
  EXPECT(out[4] == 51 && out[5] == 61 && out[6] == 71 && out[7] == 81);
  EXPECT(TA[0] == 100 && TA[15] == 115 && TB[0] == 116 && TB[15] == 131);
  EXPECT(bTA[0] == 1 && bTA[15] == 16);                       // n < min_inliers: the state stays
  EXPECT(bTB[0] == 216 && bTB[15] == 231);
  EXPECT(inl[0] == 7 && inl[4] == 11 && inl[5] == 77 && bm[0] == 25 && bm[4] == 29 && bm[5] == 77);
  return 0;
}

static int check_sim3() {
  float X1[15], X2[15], i1[10], i2[10];
  int32_t m1[5], m2[5];
  for (int i = 0; i < 15; i++) X1[i] = 100.f + i, X2[i] = 150.f + i;
  for (int i = 0; i < 10; i++) i1[i] = 200.f + i, i2[i] = 250.f + i;
  for (int i = 0; i < 5; i++) m1[i] = 300 + i, m2[i] = 350 + i;
  const int32_t draws[6] = {11, 12, 13, 14, 15, 16};
  float bT[2][16], bR[2][9], bt[2][3], bs[2] = {0.5f, 0.25f}, T[2][16] = {};
  for (int s = 0; s < 2; s++) {
    for (int i = 0; i < 16; i++) bT[s][i] = 1.f + 20 * s + i;
    for (int i = 0; i < 9; i++) bR[s][i] = 2.f + 20 * s + i;
    for (int i = 0; i < 3; i++) bt[s][i] = 3.f + 20 * s + i;
  }
  int32_t it[2] = {3, 1}, bi[2] = {4, 2}, out[8] = {-9, -9, -9, -9, -9, -9, -9, -9};
  uint8_t bm[6] = {1, 0, 1, 0, 1, 77}, inl[6] = {9, 9, 9, 9, 9, 77};
  orbsim3_problem P[2] = {
      {500, 501, 320, 240, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 3, 10, 0, 0, nullptr,
       &it[0], &bi[0], nullptr, bT[0], bR[0], bt[0], &bs[0], T[0], &out[0], &out[1], &out[2], nullptr,
       &out[3]},
      {600, 601, 321, 241, 5, X1, X2, i1, i2, m1, m2, 3, 10, 7, 6, draws, &it[1], &bi[1], bm, bT[1],
       bR[1], bt[1], &bs[1], T[1], &out[4], &out[5], &out[6], inl, &out[7]}};
  Sim3Rows R(P, 2, 5, 6, {0, 6});
  const float camA[4] = {500, 501, 320, 240}, camB[4] = {600, 601, 321, 241};
  EXPECT(is(R.n, {0, 5}) && is(R.min_inliers, {3, 3}) && is(R.max_its, {10, 10}) && is(R.fix_scale, {0, 1}));
  EXPECT(is(R.iterations, {3, 1}) && is(R.best_inliers, {4, 2}) && is(R.best_s, {0.5f, 0.25f}));
  EXPECT(row_is(R.cam, 0, camA, 4) && row_is(R.cam, 1, camB, 4));
  for (size_t s = 0; s < 2; s++)
    EXPECT(row_is(R.best_T12, s, bT[s], 16) && row_is(R.best_R, s, bR[s], 9) && row_is(R.best_t, s, bt[s], 3));
  EXPECT(row_is(R.draws, 0, draws, 0) && row_is(R.draws, 1, draws, 6));
  EXPECT(row_is(R.X3Dc1, 0, X1, 0) && row_is(R.X3Dc1, 1, X1, 15) && row_is(R.X3Dc2, 0, X2, 0) &&
         row_is(R.X3Dc2, 1, X2, 15));
  EXPECT(row_is(R.P1im1, 0, i1, 0) && row_is(R.P1im1, 1, i1, 10) && row_is(R.P2im2, 0, i2, 0) &&
         row_is(R.P2im2, 1, i2, 10));
  EXPECT(row_is(R.max_error1, 0, m1, 0) && row_is(R.max_error1, 1, m1, 5) &&
         row_is(R.max_error2, 0, m2, 0) && row_is(R.max_error2, 1, m2, 5));
  EXPECT(row_is(R.best_mask, 0, bm, 0) && row_is(R.best_mask, 1, bm, 5));
  EXPECT(R.T12.h.size() == 32 && R.inliers.h.size() == 10 && R.result.h.size() == 2);
  count_up(R.iterations, 30), count_up(R.best_inliers, 40), count_up(R.result, 50);
  count_up(R.no_more, 60), count_up(R.n_inliers, 70), count_up(R.draws_consumed, 80);
  count_up(R.T12, 100), count_up(R.best_T12, 200), count_up(R.best_R, 300), count_up(R.best_t, 400);
  count_up(R.best_s, 500), count_up(R.inliers, 2), count_up(R.best_mask, 20);
  R.unpack();
  EXPECT(out[0] == 50 && out[1] == 60 && out[2] == 70 && out[3] == 80);
  EXPECT(out[4] == 51 && out[5] == 61 && out[6] == 71 && out[7] == 81);
  EXPECT(T[0][0] == 100 && T[0][15] == 115 && T[1][0] == 116 && T[1][15] == 131);
  // n < min_inliers: the whole state stays
  EXPECT(it[0] == 3 && bi[0] == 4 && bs[0] == 0.5f && bT[0][0] == 1 && bR[0][8] == 10 && bt[0][2] == 5);
  EXPECT(it[1] == 31 && bi[1] == 41 && bs[1] == 501 && bT[1][0] == 216 && bT[1][15] == 231);
  EXPECT(bR[1][0] == 309 && bR[1][8] == 317 && bt[1][0] == 403 && bt[1][2] == 405);
  EXPECT(inl[0] == 7 && inl[4] == 11 && inl[5] == 77 && bm[0] == 25 && bm[4] == 29 && bm[5] == 77);
  return 0;
}

static int check_search_by_sim3() {
  // (n1, n2) = (2, 0) and (1, 3): pitches 2 and 3
  orbpl_keypoint kp[3] = {};
  uint8_t desc[96], mpd[96], valid[3] = {1, 0, 1};
  float xyz[9], mind[3] = {1, 2, 3}, maxd[3] = {4, 5, 6}, T1[16], T2[16];
  for (int i = 0; i < 3; i++) kp[i].x = 10.f + i, kp[i].octave = i;
  for (int i = 0; i < 96; i++) desc[i] = (uint8_t)(i + 1), mpd[i] = (uint8_t)(200 - i);
  for (int i = 0; i < 9; i++) xyz[i] = 0.5f + i;
  for (int i = 0; i < 16; i++) T1[i] = 1.f + i, T2[i] = 30.f + i;
  const float R12[9] = {1, 2, 3, 4, 5, 6, 7, 8, 9}, t12[3] = {-1, -2, -3};
  int32_t mA[3] = {1, -2, 77}, mB[2] = {0, 77}, nf[2] = {-9, -9};
  int32_t v1A[3] = {9, 9, 77}, r1A[3] = {9, 9, 77}, v1B[2] = {9, 77}, r1B[2] = {9, 77};
  int32_t v2B[4] = {9, 9, 9, 77}, r2B[4] = {9, 9, 9, 77};
  const orbm_sim3_keyframe two = {2, kp, desc, valid, xyz, mind, maxd, mpd, T1};
  const orbm_sim3_keyframe none = {0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, T2};
  const orbm_sim3_keyframe one = {1, kp + 2, desc + 64, valid + 2, xyz + 6, mind + 2, maxd + 2, mpd + 64, T2};
  const orbm_sim3_keyframe three = {3, kp, desc, valid, xyz, mind, maxd, mpd, T1};
  orbm_sim3_pair P[2] = {{two, none, 2.f, R12, t12, mA, &nf[0], v1A, nullptr, r1A, nullptr},
                         {one, three, 3.f, R12, t12, mB, &nf[1], v1B, v2B, r1B, r2B}};
  SbsRows R(P, 2, 2, 3);
  EXPECT(is(R.k1.n, {2, 1}) && is(R.k2.n, {0, 3}) && is(R.s12, {2.f, 3.f}));
  EXPECT(is(R.matched12, {1, -2, 0, -1}));                    // padded with -1
  EXPECT(row_is(R.R12, 0, R12, 9) && row_is(R.R12, 1, R12, 9) && row_is(R.t12, 0, t12, 3) &&
         row_is(R.t12, 1, t12, 3));
  EXPECT(row_is(R.k1.Tcw, 0, T1, 16) && row_is(R.k1.Tcw, 1, T2, 16) && row_is(R.k2.Tcw, 0, T2, 16) &&
         row_is(R.k2.Tcw, 1, T1, 16));
  EXPECT(row_is(R.k1.kps_un, 0, kp, 2) && row_is(R.k1.kps_un, 1, kp + 2, 1) &&
         row_is(R.k2.kps_un, 0, kp, 0) && row_is(R.k2.kps_un, 1, kp, 3));
  EXPECT(row_is(R.k1.desc, 0, desc, 64) && row_is(R.k1.desc, 1, desc + 64, 32) &&
         row_is(R.k2.desc, 0, desc, 0) && row_is(R.k2.desc, 1, desc, 96));
  EXPECT(row_is(R.k1.mp_desc, 0, mpd, 64) && row_is(R.k1.mp_desc, 1, mpd + 64, 32) &&
         row_is(R.k2.mp_desc, 0, mpd, 0) && row_is(R.k2.mp_desc, 1, mpd, 96));
  EXPECT(row_is(R.k1.valid, 0, valid, 2) && row_is(R.k1.valid, 1, valid + 2, 1) &&
         row_is(R.k2.valid, 0, valid, 0) && row_is(R.k2.valid, 1, valid, 3));
  EXPECT(row_is(R.k1.xyz, 0, xyz, 6) && row_is(R.k1.xyz, 1, xyz + 6, 3) && row_is(R.k2.xyz, 0, xyz, 0) &&
         row_is(R.k2.xyz, 1, xyz, 9));
  EXPECT(row_is(R.k1.min_dist, 0, mind, 2) && row_is(R.k1.min_dist, 1, mind + 2, 1) &&
         row_is(R.k2.min_dist, 0, mind, 0) && row_is(R.k2.min_dist, 1, mind, 3));
  EXPECT(row_is(R.k1.max_dist, 0, maxd, 2) && row_is(R.k1.max_dist, 1, maxd + 2, 1) &&
         row_is(R.k2.max_dist, 0, maxd, 0) && row_is(R.k2.max_dist, 1, maxd, 3));
  EXPECT(R.k1.vn_match.h.size() == 4 && R.k1.reason.h.size() == 4 && R.k2.vn_match.h.size() == 6 &&
         R.k2.reason.h.size() == 6 && R.n_found.h.size() == 2);
  count_up(R.n_found, 40), count_up(R.matched12, 50), count_up(R.k1.vn_match, 60);
  count_up(R.k1.reason, 70), count_up(R.k2.vn_match, 80), count_up(R.k2.reason, 90);
  R.unpack();
  EXPECT(nf[0] == 40 && nf[1] == 41);
  EXPECT(mA[0] == 50 && mA[1] == 51 && mA[2] == 77 && mB[0] == 52 && mB[1] == 77);
  EXPECT(v1A[0] == 60 && v1A[1] == 61 && v1A[2] == 77 && v1B[0] == 62 && v1B[1] == 77);
  EXPECT(r1A[0] == 70 && r1A[1] == 71 && r1A[2] == 77 && r1B[0] == 72 && r1B[1] == 77);
  EXPECT(v2B[0] == 83 && v2B[2] == 85 && v2B[3] == 77 && r2B[0] == 93 && r2B[2] == 95 && r2B[3] == 77);
  return 0;
}

// the database of the second problem: two keyframes, BowVectors of 1 and 3 entries
struct TinyDb {
  int32_t off[3] = {0, 1, 4}, covis[20];
  uint32_t words[4] = {5, 2, 6, 9}, qw[2] = {2, 9};
  double vals[4] = {0.5, 0.25, 0.125, 0.0625}, qv[2] = {0.75, 0.375};
  float rs[3] = {1.5f, 2.5f, 77.f};
  TinyDb() {
    for (int i = 0; i < 20; i++) covis[i] = i % 3 - 1;
  }
};

template <class Prob>
static int check_db_columns(const KfdbRows<Prob>& D, const TinyDb& t) {
  EXPECT(is(D.nkf, {0, 2}) && is(D.q_n, {0, 2}));
  EXPECT(row_is(D.kf_off, 0, t.off, 0) && row_is(D.kf_off, 1, t.off, 3) && D.kf_off.row == 65);
  EXPECT(row_is(D.kf_words, 0, t.words, 0) && row_is(D.kf_words, 1, t.words, 4));
  EXPECT(row_is(D.kf_vals, 0, t.vals, 0) && row_is(D.kf_vals, 1, t.vals, 4));
  EXPECT(row_is(D.covis, 0, t.covis, 0, -1) && row_is(D.covis, 1, t.covis, 20, -1) && D.covis.row == 640);
  EXPECT(row_is(D.reloc_score, 0, t.rs, 0) && row_is(D.reloc_score, 1, t.rs, 2) && D.reloc_score.row == 64);
  EXPECT(row_is(D.q_words, 0, t.qw, 0) && row_is(D.q_words, 1, t.qw, 2));
  EXPECT(row_is(D.q_vals, 0, t.qv, 0) && row_is(D.q_vals, 1, t.qv, 2));
  return 0;
}

static int check_kfdb() {
  TinyDb t;
  int32_t candA[64], candB[64], nc[2] = {-9, -9}, cw[3] = {-9, -9, 77};
  for (int i = 0; i < 64; i++) candA[i] = candB[i] = 77;
  orbkf_problem P[2] = {
      {0, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr, candA, &nc[0], nullptr},
      {2, t.off, t.words, t.vals, t.covis, t.rs, 2, t.qw, t.qv, candB, &nc[1], cw}};
  size_t entp = 1, qp = 1;
  EXPECT(!kfdb_refusal(P[0], "x", &entp, &qp) && entp == 1 && qp == 1);
  EXPECT(!kfdb_refusal(P[1], "x", &entp, &qp) && entp == 4 && qp == 2);
  orbkf_problem bad = P[1];
  bad.nkf = 65;
  EXPECT(std::string(kfdb_refusal(bad, "x", &entp, &qp)) == "more than 64 keyframes in a database");
  bad = P[1], bad.q_vals = nullptr;
  EXPECT(std::string(kfdb_refusal(bad, "x", &entp, &qp)) == "NULL query BowVector");
  bad = P[1], bad.covis = nullptr;
  EXPECT(std::string(kfdb_refusal(bad, "x", &entp, &qp)) == "NULL keyframe arrays");
  bad = P[1], bad.kf_words = nullptr;
  EXPECT(std::string(kfdb_refusal(bad, "x", &entp, &qp)) == "NULL keyframe BowVectors");
  t.off[0] = 1;
  EXPECT(std::string(kfdb_refusal(P[1], "the caller's words", &entp, &qp)) == "the caller's words");
  t.off[0] = 0, t.off[1] = 5;
  EXPECT(std::string(kfdb_refusal(P[1], "x", &entp, &qp)) ==
         "a keyframe's BowVector has a negative length or more than 4096 entries");
  t.off[1] = 1;
  EXPECT(entp == 4 && qp == 2);

  KfdbCallRows R(P, 2, entp, qp);
  if (check_db_columns(R.db, t)) return 1;
  EXPECT(R.cand.h.size() == 128 && R.ncand.h.size() == 2 && R.common_words.h.size() == 128);
  count_up(R.cand, 100), count_up(R.common_words, 300), count_up(R.db.reloc_score, 500);
  R.ncand.at(0) = 0, R.ncand.at(1) = 2;
  R.unpack();
  EXPECT(nc[0] == 0 && nc[1] == 2 && candA[0] == 77 && candB[0] == 164 && candB[1] == 165 && candB[2] == 77);
  EXPECT(cw[0] == 364 && cw[1] == 365 && cw[2] == 77);       // asked for by the second problem only
  EXPECT(t.rs[0] == 564 && t.rs[1] == 565 && t.rs[2] == 77);
  return 0;
}

static int check_reloc() {
  // A: no keyframe, no keypoint, no stream. B: the database above, keyframe
  // features (0, 2), a frame of 3 keypoints, two streams. kp_pitch 4, draw_pitch 2
  TinyDb t;
  const int32_t foff[3] = {0, 0, 2}, fnode[2] = {31, 32}, node[3] = {41, 42, 43}, draws[4] = {1, 2, 3, 4};
  const float ang[2] = {0.5f, 1.5f}, xyz[6] = {1, 2, 3, 4, 5, 6}, mn[2] = {7, 8}, mx[2] = {9, 10};
  const float ur[3] = {11, -1, 13};
  uint8_t kdesc[64], mdesc[64], desc[96];
  const uint8_t kval[2] = {1, 0};
  for (int i = 0; i < 64; i++) kdesc[i] = (uint8_t)(i + 1), mdesc[i] = (uint8_t)(100 + i);
  for (int i = 0; i < 96; i++) desc[i] = (uint8_t)(150 + i);
  orbpl_keypoint kp[3] = {};
  for (int i = 0; i < 3; i++) kp[i].x = 20.f + i;
  int32_t match[4] = {9, 9, 9, 77}, recA[64 * ORBRL_REC_INTS], recB[64 * ORBRL_REC_INTS + 1];
  uint8_t outl[4] = {9, 9, 9, 77};
  recB[64 * ORBRL_REC_INTS] = 77;
  orbrl_problem P[2] = {};
  P[0].records = recA;
  P[1].nkf = 2, P[1].kf_off = t.off, P[1].kf_words = t.words, P[1].kf_vals = t.vals;
  P[1].covis = t.covis, P[1].reloc_score = t.rs, P[1].kf_feat_off = foff, P[1].kf_angle = ang;
  P[1].kf_feat_node = fnode, P[1].kf_desc = kdesc, P[1].kf_valid = kval, P[1].mp_xyz = xyz;
  P[1].mp_min_dist = mn, P[1].mp_max_dist = mx, P[1].mp_desc = mdesc, P[1].n = 3, P[1].kps_un = kp;
  P[1].uright = ur, P[1].desc = desc, P[1].feat_node = node, P[1].nq_words = 2, P[1].q_words = t.qw;
  P[1].q_vals = t.qv, P[1].n_draw_streams = 2, P[1].draws = draws, P[1].mp_kf_feature = match;
  P[1].outlier = outl, P[1].records = recB;
  size_t entp = 1, qp = 1;
  EXPECT(!kfdb_refusal(P[0], "x", &entp, &qp) && !kfdb_refusal(P[1], "x", &entp, &qp) && entp == 4 && qp == 2);
  RelocRows R(P, 2, 4, 2, entp, qp, 2);
  if (check_db_columns(R.db, t)) return 1;
  EXPECT(R.S == 2 && is(R.kf_first, {0, 0}) && is(R.kf_n, {0, 2}) && is(R.n, {0, 3}) && is(R.n_streams, {0, 2}));
  EXPECT(row_is(R.kf_angle, 0, ang, 0) && row_is(R.kf_angle, 1, ang, 2));
  EXPECT(row_is(R.kf_feat_node, 0, fnode, 0, -1) && row_is(R.kf_feat_node, 1, fnode, 2, -1));
  EXPECT(row_is(R.kf_desc, 0, kdesc, 0) && row_is(R.kf_desc, 1, kdesc, 64) && R.kf_desc.row == 128);
  EXPECT(row_is(R.kf_valid, 0, kval, 0) && row_is(R.kf_valid, 1, kval, 2));
  EXPECT(row_is(R.mp_xyz, 0, xyz, 0) && row_is(R.mp_xyz, 1, xyz, 6) && R.mp_xyz.row == 12);
  EXPECT(row_is(R.mp_min_dist, 0, mn, 0) && row_is(R.mp_min_dist, 1, mn, 2));
  EXPECT(row_is(R.mp_max_dist, 0, mx, 0) && row_is(R.mp_max_dist, 1, mx, 2));
  EXPECT(row_is(R.mp_desc, 0, mdesc, 0) && row_is(R.mp_desc, 1, mdesc, 64));
  EXPECT(row_is(R.kps_un, 0, kp, 0) && row_is(R.kps_un, 1, kp, 3) && R.kps_un.row == 4);
  EXPECT(row_is(R.uright, 0, ur, 0, -1.0f) && row_is(R.uright, 1, ur, 3, -1.0f));
  EXPECT(row_is(R.desc, 0, desc, 0) && row_is(R.desc, 1, desc, 96) && R.desc.row == 128);
  EXPECT(row_is(R.feat_node, 0, node, 0, -1) && row_is(R.feat_node, 1, node, 3, -1));
  EXPECT(row_is(R.draws, 0, draws, 0) && row_is(R.draws, 1, draws, 4) && R.draws.row == 4);
  EXPECT(R.scalars.rows == 6 && R.scalars.row == 2 && R.cand.h.size() == 128 && R.Tcw.h.size() == 32 &&
         R.mp_kf_feature.h.size() == 8 && R.outlier.h.size() == 8 &&
         R.records.h.size() == 2 * 64 * ORBRL_REC_INTS);
  count_up(R.scalars, 10), count_up(R.cand, 100), count_up(R.Tcw, 300), count_up(R.mp_kf_feature, 40);
  count_up(R.outlier, 50), count_up(R.records, 1000), count_up(R.db.reloc_score, 500);
  R.ncand.at(0) = 0, R.ncand.at(1) = 2;
  EXPECT(!R.unpack());
  EXPECT(P[0].ok == 10 && P[1].ok == 11 && P[0].status == 12 && P[1].status == 13 && P[1].winner == 15 &&
         P[1].rounds == 17 && P[1].n_good == 19 && P[0].n_candidates == 20 && P[1].n_candidates == 21);
  EXPECT(P[0].ncand == 0 && P[0].cand[0] == -1 && P[0].cand[63] == -1);
  EXPECT(P[1].ncand == 2 && P[1].cand[0] == 164 && P[1].cand[1] == 165 && P[1].cand[2] == -1 &&
         P[1].cand[63] == -1);
  EXPECT(P[0].Tcw[0] == 300 && P[1].Tcw[0] == 316 && P[1].Tcw[15] == 331);
  EXPECT(match[0] == 44 && match[2] == 46 && match[3] == 77 && outl[0] == 54 && outl[2] == 56 && outl[3] == 77);
  EXPECT(recA[0] == 1000 && recB[0] == 1000 + 64 * ORBRL_REC_INTS && recB[64 * ORBRL_REC_INTS] == 77);
  EXPECT(t.rs[0] == 564 && t.rs[1] == 565 && t.rs[2] == 77);
  R.scalars.at(RelocRows::kStatus, 0) = ORBRL_DRAW_EXHAUSTED;
  EXPECT(R.unpack() && P[0].status == ORBRL_DRAW_EXHAUSTED && P[1].status == 13);
  return 0;
}

static int check_triangulation() {
  // A: no neighbour, an empty current keyframe. B: cur of (2 features, 1 line),
  // neighbours of (3, 0) and (1, 2): pitches 3 and 2
  float T[16];
  for (int i = 0; i < 16; i++) T[i] = 1.f + i;
  orbpl_keypoint kp[3] = {}, ku[3] = {};
  orbpl_keyline kl[2] = {};
  for (int i = 0; i < 3; i++) kp[i].x = 10.f + i, ku[i].x = 20.f + i;
  kl[0].startPointX = 5.f, kl[1].startPointX = 6.f;
  const float ur[3] = {30, -1, 32}, dep[3] = {2, -1, 3}, mpx[9] = {1, 2, 3, 4, 5, 6, 7, 8, 9};
  const int32_t node[3] = {7, 8, 9};
  const uint8_t has[3] = {1, 0, 1};
  uint8_t desc[96], ld[64];
  for (int i = 0; i < 96; i++) desc[i] = (uint8_t)(i + 1);
  for (int i = 0; i < 64; i++) ld[i] = (uint8_t)(100 + i);
  const double lc[6] = {0.5, 1.5, 2.5, 3.5, 4.5, 5.5};
  auto kf = [&](int id, int n, int nl) {
    return orblm_keyframe{id, T, n, kp, ku, ur, dep, desc, node, has, mpx, nl, kl, ld, lc};
  };
  const orblm_keyframe neigh[2] = {kf(5, 3, 0), kf(6, 1, 2)};
  orblm_point_record pts[3];
  orblm_line_record lns[11];
  memset(pts, 0x77, sizeof(pts));
  memset(lns, 0x77, sizeof(lns));
  int32_t prec[3] = {9, 9, 77}, lrec[2] = {9, 77};
  orblm_problem P[2] = {};
  P[0].cur = orblm_keyframe{3, T, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                            0, nullptr, nullptr, nullptr};
  P[1].cur = kf(4, 2, 1);
  P[1].n_neigh = 2, P[1].neigh = neigh, P[1].points = pts, P[1].kf1_point_record = prec;
  P[1].lines = lns, P[1].kf1_line_record = lrec;
  LmRows R;
  R.add_problem(&P[0].cur, nullptr, 0);
  R.add_problem(&P[1].cur, neigh, 2);
  EXPECT(R.kfs.size() == 4 && R.pitch == 3 && R.lpitch == 2);
  EXPECT(R.cur == std::vector<int32_t>({0, 1}));
  EXPECT(R.neigh == std::vector<int32_t>({-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 2, 3, -1, -1, -1, -1, -1, -1, -1, -1}));
  R.pack();
  const size_t n[4] = {0, 2, 3, 1}, nl[4] = {0, 1, 0, 2};
  EXPECT(is(R.id, {3, 4, 5, 6}) && is(R.n, {0, 2, 3, 1}) && is(R.nl, {0, 1, 0, 2}));
  for (size_t k = 0; k < 4; k++) {
    EXPECT(row_is(R.Tcw, k, T, 16) && row_is(R.kps, k, kp, n[k]) && row_is(R.kps_un, k, ku, n[k]));
    EXPECT(row_is(R.uright, k, ur, n[k], -1.0f) && row_is(R.depth, k, dep, n[k], -1.0f));
    EXPECT(row_is(R.desc, k, desc, 32 * n[k]) && row_is(R.feat_node, k, node, n[k], -1));
    EXPECT(row_is(R.has_mp, k, has, n[k], (uint8_t)1) && row_is(R.mp_xyz, k, mpx, 3 * n[k]));
    EXPECT(row_is(R.klines, k, kl, nl[k]) && row_is(R.ldesc, k, ld, 32 * nl[k]) && row_is(R.lcoef, k, lc, 3 * nl[k]));
  }
  EXPECT(R.desc.row == 96 && R.mp_xyz.row == 9 && R.ldesc.row == 64 && R.lcoef.row == 6);
  EXPECT(R.points.rows == 2 && R.points.row == 3 && R.lines.row == 20 && R.point_record.row == 3 &&
         R.line_record.row == 2 && R.pairs.row == 10 && R.line_pairs.row == 10 && R.n_points.h.size() == 2 &&
         R.n_lines.h.size() == 2);
  // a call that reads the lines only packs no point column
  LmRows L;
  L.reads = kReadLines;
  L.add_problem(&P[1].cur, neigh, 1);
  L.pack();
  EXPECT(L.pitch == 1 && L.lpitch == 1 && is(L.n, {0, 0}) && is(L.nl, {1, 0}) && is(L.feat_node, {-1, -1}) &&
         is(L.has_mp, {1, 1}));

  R.n_points.at(0) = 0, R.n_points.at(1) = 1, R.n_lines.at(0) = 0, R.n_lines.at(1) = 3;
  count_up(R.pairs, 100), count_up(R.line_pairs, 200), count_up(R.point_record, 300), count_up(R.line_record, 400);
  for (size_t i = 0; i < R.points.h.size(); i++) R.points.h[i].idx1 = 500 + (int)i;
  for (size_t i = 0; i < R.lines.h.size(); i++) R.lines.h[i].idx1 = 600 + (int)i;
  R.unpack(P);
  EXPECT(P[0].n_points == 0 && P[0].n_lines == 0 && P[1].n_points == 1 && P[1].n_lines == 3);
  EXPECT(P[0].pairs[0] == 100 && P[0].pairs[9] == 109 && P[1].pairs[0] == 110 && P[1].pairs[9] == 119);
  EXPECT(P[0].line_pairs[0] == 200 && P[1].line_pairs[9] == 219);
  EXPECT(prec[0] == 303 && prec[1] == 304 && prec[2] == 77 && lrec[0] == 402 && lrec[1] == 77);
  EXPECT(pts[0].idx1 == 503 && pts[1].idx1 == 0x77777777);    // the first n_points records
  EXPECT(lns[0].idx1 == 620 && lns[2].idx1 == 622 && lns[3].idx1 == 0x77777777);
  return 0;
}

int main() {
  if (check_rows() || check_pnp() || check_sim3() || check_search_by_sim3() || check_kfdb() ||
      check_reloc() || check_triangulation())
    return 1;
  printf("host_rows_check: ok\n");
  return 0;
}
