// The host side of the batched host-pointer entry points (map_pool.h's
// counterpart for the calls without an orblm_map): one struct per call that
// holds the call's pitched columns as Rows (host_stage.h). Host code, no HIP
// call: an entry point validates, builds the struct from its problems and the
// pitches it found (which fills the in columns), stages the columns through
// its HostStage, launches, copies the out columns back and unpacks. A row's
// length is stated once, where the column is built. What no problem fills is
// padding: matched12, covis, feat_node -1, uright and depth -1.0f, has_mp 1,
// every other column 0. Pitches are the call's widest count, at least 1.
#pragma once
#include <algorithm>
#include <vector>

#include "host_stage.h"
#include "reloc_kernels.h"

namespace orbpl {

typedef Rows<int32_t> RowsI;
typedef Rows<float> RowsF;
typedef Rows<uint8_t> RowsB;

// ---- orbpnp_iterate: nd[p] = the draws problem p can consume in this call ----
struct PnpRows {
  const orbpnp_problem* P;
  size_t S, ptp, drp;
  RowsI n{S, 1}, min_inliers{S, 1}, max_its{S, 1}, draws{S, drp}, iterations{S, 1}, best_inliers{S, 1};
  RowsF cam{S, 4}, p2d{S, ptp * 2}, p3d{S, ptp * 3}, max_error{S, ptp}, best_Tcw{S, 16};
  RowsB best_mask{S, ptp};
  // out
  RowsI result{S, 1}, no_more{S, 1}, n_inliers{S, 1}, draws_consumed{S, 1};
  RowsF Tcw{S, 16};
  RowsB inliers{S, ptp};

  PnpRows(const orbpnp_problem* P_, size_t S_, size_t ptp_, size_t drp_, const std::vector<size_t>& nd)
      : P(P_), S(S_), ptp(ptp_), drp(drp_) {
    for (size_t p = 0; p < S; p++) {
      const orbpnp_problem& r = P[p];
      const size_t m = r.n;
      const float c[4] = {r.fx, r.fy, r.cx, r.cy};
      n.at(p) = r.n;
      min_inliers.at(p) = r.min_inliers;
      max_its.at(p) = r.max_its;
      iterations.at(p) = *r.iterations;
      best_inliers.at(p) = *r.best_inliers;
      cam.put(p, c, 4);
      best_Tcw.put(p, r.best_Tcw, 16);
      draws.put(p, r.draws, nd[p]);
      p2d.put(p, r.p2d, 2 * m);
      p3d.put(p, r.p3d, 3 * m);
      max_error.put(p, r.max_error, m);
      best_mask.put(p, r.best_mask, m);
    }
  }
  void unpack() {
    for (size_t p = 0; p < S; p++) {
      const orbpnp_problem& r = P[p];
      *r.iterations = iterations.at(p);
      *r.best_inliers = best_inliers.at(p);
      *r.result = result.at(p);
      *r.no_more = no_more.at(p);
      *r.n_inliers = n_inliers.at(p);
      *r.draws_consumed = draws_consumed.at(p);
      Tcw.take(p, r.Tcw, 16);
      inliers.take(p, r.inliers, r.n);
      if (r.n < r.min_inliers) continue;  // the early return leaves the state as it was
      best_Tcw.take(p, r.best_Tcw, 16);
      best_mask.take(p, r.best_mask, r.n);
    }
  }
};

// ---- orbsim3_iterate ----
struct Sim3Rows {
  const orbsim3_problem* P;
  size_t S, ptp, drp;
  RowsI n{S, 1}, min_inliers{S, 1}, max_its{S, 1}, fix_scale{S, 1}, draws{S, drp}, iterations{S, 1},
      best_inliers{S, 1}, max_error1{S, ptp}, max_error2{S, ptp};
  RowsF cam{S, 4}, X3Dc1{S, ptp * 3}, X3Dc2{S, ptp * 3}, P1im1{S, ptp * 2}, P2im2{S, ptp * 2},
      best_T12{S, 16}, best_R{S, 9}, best_t{S, 3}, best_s{S, 1};
  RowsB best_mask{S, ptp};
  // out
  RowsI result{S, 1}, no_more{S, 1}, n_inliers{S, 1}, draws_consumed{S, 1};
  RowsF T12{S, 16};
  RowsB inliers{S, ptp};

  Sim3Rows(const orbsim3_problem* P_, size_t S_, size_t ptp_, size_t drp_, const std::vector<size_t>& nd)
      : P(P_), S(S_), ptp(ptp_), drp(drp_) {
    for (size_t p = 0; p < S; p++) {
      const orbsim3_problem& r = P[p];
      const size_t m = r.n;
      const float c[4] = {r.fx, r.fy, r.cx, r.cy};
      n.at(p) = r.n;
      min_inliers.at(p) = r.min_inliers;
      max_its.at(p) = r.max_its;
      fix_scale.at(p) = r.fix_scale != 0;
      iterations.at(p) = *r.iterations;
      best_inliers.at(p) = *r.best_inliers;
      best_s.at(p) = *r.best_s;
      cam.put(p, c, 4);
      best_T12.put(p, r.best_T12, 16);
      best_R.put(p, r.best_R, 9);
      best_t.put(p, r.best_t, 3);
      draws.put(p, r.draws, nd[p]);
      X3Dc1.put(p, r.X3Dc1, 3 * m);
      X3Dc2.put(p, r.X3Dc2, 3 * m);
      P1im1.put(p, r.P1im1, 2 * m);
      P2im2.put(p, r.P2im2, 2 * m);
      max_error1.put(p, r.max_error1, m);
      max_error2.put(p, r.max_error2, m);
      best_mask.put(p, r.best_mask, m);
    }
  }
  void unpack() {
    for (size_t p = 0; p < S; p++) {
      const orbsim3_problem& r = P[p];
      *r.result = result.at(p);
      *r.no_more = no_more.at(p);
      *r.n_inliers = n_inliers.at(p);
      *r.draws_consumed = draws_consumed.at(p);
      T12.take(p, r.T12, 16);
      inliers.take(p, r.inliers, r.n);
      if (r.n < r.min_inliers) continue;  // the early return leaves the state as it was
      *r.iterations = iterations.at(p);
      *r.best_inliers = best_inliers.at(p);
      *r.best_s = best_s.at(p);
      best_T12.take(p, r.best_T12, 16);
      best_R.take(p, r.best_R, 9);
      best_t.take(p, r.best_t, 3);
      best_mask.take(p, r.best_mask, r.n);
    }
  }
};

// ---- orbm_search_by_sim3 ----
struct SbsRows {
  struct Side {
    size_t S, pitch;
    RowsI n{S, 1};
    Rows<orbpl_keypoint> kps_un{S, pitch};
    RowsB desc{S, pitch * 32}, valid{S, pitch}, mp_desc{S, pitch * 32};
    RowsF xyz{S, pitch * 3}, min_dist{S, pitch}, max_dist{S, pitch}, Tcw{S, 16};
    RowsI vn_match{S, pitch}, reason{S, pitch};   // out
    void put(size_t p, const orbm_sim3_keyframe& k) {
      const size_t m = k.n;
      n.at(p) = k.n;
      Tcw.put(p, k.Tcw, 16);
      kps_un.put(p, k.kps_un, m);
      desc.put(p, k.desc, 32 * m);
      valid.put(p, k.valid, m);
      mp_desc.put(p, k.mp_desc, 32 * m);
      xyz.put(p, k.xyz, 3 * m);
      min_dist.put(p, k.min_dist, m);
      max_dist.put(p, k.max_dist, m);
    }
  };
  const orbm_sim3_pair* P;
  size_t S;
  Side k1, k2;
  RowsF s12{S, 1}, R12{S, 9}, t12{S, 3};
  RowsI matched12{S, k1.pitch, -1}, n_found{S, 1};

  SbsRows(const orbm_sim3_pair* P_, size_t S_, size_t p1, size_t p2)
      : P(P_), S(S_), k1{S_, p1}, k2{S_, p2} {
    for (size_t p = 0; p < S; p++) {
      const orbm_sim3_pair& r = P[p];
      k1.put(p, r.kf1);
      k2.put(p, r.kf2);
      s12.at(p) = r.s12;
      R12.put(p, r.R12, 9);
      t12.put(p, r.t12, 3);
      matched12.put(p, r.matched12, r.kf1.n);
    }
  }
  void unpack() {
    for (size_t p = 0; p < S; p++) {
      const orbm_sim3_pair& r = P[p];
      *r.n_found = n_found.at(p);
      matched12.take(p, r.matched12, r.kf1.n);
      k1.vn_match.take(p, r.vn_match1, r.kf1.n);
      k1.reason.take(p, r.reason1, r.kf1.n);
      k2.vn_match.take(p, r.vn_match2, r.kf2.n);
      k2.reason.take(p, r.reason2, r.kf2.n);
    }
  }
};

// ---- the keyframe database of orbkf_problem and orbrl_problem (the same field
// names): its refusals and its columns ----

// the refusal of r's database and query, or nullptr; entp and qp grow to r's
// entry and query counts. off0: the caller's words for kf_off[0] != 0
template <class Prob>
const char* kfdb_refusal(const Prob& r, const char* off0, size_t* entp, size_t* qp) {
  if (r.nkf < 0 || r.nkf > kKfdbMaxKf) return "more than 64 keyframes in a database";
  if (r.nq_words < 0 || r.nq_words > kKfdbMaxWords)
    return "more than 4096 entries in the query's BowVector";
  if (r.nq_words > 0 && (!r.q_words || !r.q_vals)) return "NULL query BowVector";
  *qp = std::max(*qp, (size_t)r.nq_words);
  if (r.nkf == 0) return nullptr;
  if (!r.kf_off || !r.covis || !r.reloc_score) return "NULL keyframe arrays";
  if (r.kf_off[0] != 0) return off0;
  for (int k = 0; k < r.nkf; k++) {
    const int len = r.kf_off[k + 1] - r.kf_off[k];
    if (len < 0 || len > kKfdbMaxWords)
      return "a keyframe's BowVector has a negative length or more than 4096 entries";
  }
  if (r.kf_off[r.nkf] > 0 && (!r.kf_words || !r.kf_vals)) return "NULL keyframe BowVectors";
  *entp = std::max(*entp, (size_t)r.kf_off[r.nkf]);
  return nullptr;
}

template <class Prob>
struct KfdbRows {
  const Prob* P;
  size_t Q, entp, qp;
  RowsI nkf{Q, 1}, kf_off{Q, kKfdbMaxKf + 1}, covis{Q, kKfdbMaxKf * kKfdbCovis, -1}, q_n{Q, 1};
  Rows<uint32_t> kf_words{Q, entp}, q_words{Q, qp};
  Rows<double> kf_vals{Q, entp}, q_vals{Q, qp};
  RowsF reloc_score{Q, kKfdbMaxKf};   // in/out

  KfdbRows(const Prob* P_, size_t Q_, size_t entp_, size_t qp_) : P(P_), Q(Q_), entp(entp_), qp(qp_) {
    for (size_t p = 0; p < Q; p++) {
      const Prob& r = P[p];
      const size_t K = r.nkf, ne = K ? r.kf_off[K] : 0;
      nkf.at(p) = r.nkf;
      q_n.at(p) = r.nq_words;
      q_words.put(p, r.q_words, r.nq_words);
      q_vals.put(p, r.q_vals, r.nq_words);
      kf_off.put(p, r.kf_off, K ? K + 1 : 0);
      kf_words.put(p, r.kf_words, ne);
      kf_vals.put(p, r.kf_vals, ne);
      covis.put(p, r.covis, K * kKfdbCovis);
      reloc_score.put(p, r.reloc_score, K);
    }
  }
  void unpack_scores() {
    for (size_t p = 0; p < Q; p++) reloc_score.take(p, P[p].reloc_score, P[p].nkf);
  }
};

// ---- orbkf_detect_reloc ----
struct KfdbCallRows {
  KfdbRows<orbkf_problem> db;
  RowsI cand{db.Q, kKfdbMaxKf}, ncand{db.Q, 1}, common_words{db.Q, kKfdbMaxKf};   // out

  KfdbCallRows(const orbkf_problem* P, size_t Q, size_t entp, size_t qp) : db(P, Q, entp, qp) {}
  void unpack() {
    db.unpack_scores();
    for (size_t p = 0; p < db.Q; p++) {
      const orbkf_problem& r = db.P[p];
      *r.ncand = ncand.at(p);
      cand.take(p, r.cand, ncand.at(p));
      if (r.common_words) common_words.take(p, r.common_words, r.nkf);
    }
  }
};

// ---- orbrl_relocalize: the database, the keyframe features in one slot per
// keyframe of the call (kf_first[p] = problem p's first), the frames, the draw
// streams; P = the handle's kp_pitch, DP its draw_pitch, sp the widest stream count ----
struct RelocRows {
  enum { kOk, kStatus, kWinner, kRounds, kNGood, kNCandidates, kScalars };
  orbrl_problem* probs;
  size_t NP, P, DP, sp, S = slots(probs, NP);
  KfdbRows<orbrl_problem> db;
  // per slot
  RowsI kf_n{S, 1}, kf_feat_node{S, P, -1};
  RowsF kf_angle{S, P}, mp_xyz{S, P * 3}, mp_min_dist{S, P}, mp_max_dist{S, P};
  RowsB kf_desc{S, P * 32}, kf_valid{S, P}, mp_desc{S, P * 32};
  // per problem
  RowsI kf_first{NP, 1}, n{NP, 1}, feat_node{NP, P, -1}, draws{NP, sp * DP}, n_streams{NP, 1};
  RowsF uright{NP, P, -1.0f};
  RowsB desc{NP, P * 32};
  Rows<orbpl_keypoint> kps_un{NP, P};
  // out: scalars holds one row per output of kOk .. kNCandidates, NP long
  RowsI scalars{kScalars, NP}, cand{NP, kKfdbMaxKf}, ncand{NP, 1}, mp_kf_feature{NP, P},
      records{NP, kKfdbMaxKf * ORBRL_REC_INTS};
  RowsF Tcw{NP, 16};
  RowsB outlier{NP, P};

  static size_t slots(const orbrl_problem* probs, size_t NP) {
    size_t s = 0;
    for (size_t p = 0; p < NP; p++) s += probs[p].nkf;
    return std::max<size_t>(1, s);
  }
  RelocRows(orbrl_problem* probs_, size_t NP_, size_t P_, size_t DP_, size_t entp, size_t qp, size_t sp_)
      : probs(probs_), NP(NP_), P(P_), DP(DP_), sp(sp_), db(probs_, NP_, entp, qp) {
    size_t first = 0;
    for (size_t p = 0; p < NP; p++) {
      const orbrl_problem& r = probs[p];
      const size_t m = r.n;
      kf_first.at(p) = (int32_t)first;
      n.at(p) = r.n;
      n_streams.at(p) = r.n_draw_streams;
      kps_un.put(p, r.kps_un, m);
      uright.put(p, r.uright, m);
      desc.put(p, r.desc, m * 32);
      feat_node.put(p, r.feat_node, m);
      draws.put(p, r.draws, (size_t)r.n_draw_streams * DP);
      for (int k = 0; k < r.nkf; k++) {
        const size_t b = r.kf_feat_off[k], nf = r.kf_feat_off[k + 1] - b, s = first + k;
        kf_n.at(s) = (int32_t)nf;
        if (!nf) continue;   // the feature arrays may be NULL
        kf_angle.put(s, r.kf_angle + b, nf);
        kf_feat_node.put(s, r.kf_feat_node + b, nf);
        kf_desc.put(s, r.kf_desc + b * 32, nf * 32);
        kf_valid.put(s, r.kf_valid + b, nf);
        mp_xyz.put(s, r.mp_xyz + b * 3, nf * 3);
        mp_min_dist.put(s, r.mp_min_dist + b, nf);
        mp_max_dist.put(s, r.mp_max_dist + b, nf);
        mp_desc.put(s, r.mp_desc + b * 32, nf * 32);
      }
      first += r.nkf;
    }
  }
  bool unpack() {
    db.unpack_scores();
    bool exhausted = false;
    for (size_t p = 0; p < NP; p++) {
      orbrl_problem& r = probs[p];
      r.ok = scalars.at(kOk, p);
      r.status = scalars.at(kStatus, p);
      r.winner = scalars.at(kWinner, p);
      r.rounds = scalars.at(kRounds, p);
      r.n_good = scalars.at(kNGood, p);
      r.n_candidates = scalars.at(kNCandidates, p);
      r.ncand = ncand.at(p);
      std::fill(r.cand, r.cand + kKfdbMaxKf, -1);
      cand.take(p, r.cand, r.ncand);
      Tcw.take(p, r.Tcw, 16);
      mp_kf_feature.take(p, r.mp_kf_feature, r.n);
      outlier.take(p, r.outlier, r.n);
      records.take(p, r.records, records.row);
      exhausted |= r.status == ORBRL_DRAW_EXHAUSTED;
    }
    return exhausted;
  }
};

// ---- orblm_create_new_map_features and the two SearchForTriangulation calls:
// every keyframe of every problem in one pool, a problem's current keyframe
// first; cur / neigh are indices into it ----
enum { kReadPoints = 1, kReadLines = 2, kReadMapPoints = 4 };   // what of a keyframe a call reads

struct LmRows {
  enum { NB = ORBLM_MAX_NEIGHBOURS };
  std::vector<const orblm_keyframe*> kfs;
  std::vector<int32_t> cur, neigh;
  int pitch = 1, lpitch = 1, reads = kReadPoints | kReadLines | kReadMapPoints;
  RowsI id, n, nl, feat_node;
  RowsF Tcw, uright, depth, mp_xyz;
  Rows<orbpl_keypoint> kps, kps_un;
  RowsB desc, has_mp, ldesc;
  Rows<orbpl_keyline> klines;
  Rows<double> lcoef;
  // out, per problem
  Rows<orblm_point_record> points;
  Rows<orblm_line_record> lines;
  RowsI n_points, point_record, pairs, n_lines, line_record, line_pairs;

  void add_keyframe(const orblm_keyframe* k) {
    kfs.push_back(k);
    if (reads & kReadPoints) pitch = std::max(pitch, k->n);
    if (reads & kReadLines) lpitch = std::max(lpitch, k->nl);
  }
  void add_problem(const orblm_keyframe* c, const orblm_keyframe* nb, int nn) {
    cur.push_back((int32_t)kfs.size());
    add_keyframe(c);
    for (int k = 0; k < NB; k++) {
      neigh.push_back(k < nn ? (int32_t)kfs.size() : -1);
      if (k < nn) add_keyframe(nb + k);
    }
  }
  // after every add_problem: the columns, filled from the keyframes
  void pack() {
    const size_t K = kfs.size(), P = (size_t)pitch, LP = (size_t)lpitch, N = cur.size();
    id = RowsI(K, 1), n = RowsI(K, 1), nl = RowsI(K, 1), feat_node = RowsI(K, P, -1);
    Tcw = RowsF(K, 16), uright = RowsF(K, P, -1.0f), depth = RowsF(K, P, -1.0f), mp_xyz = RowsF(K, P * 3);
    kps = Rows<orbpl_keypoint>(K, P), kps_un = Rows<orbpl_keypoint>(K, P);
    desc = RowsB(K, P * 32), has_mp = RowsB(K, P, 1), ldesc = RowsB(K, LP * 32);
    klines = Rows<orbpl_keyline>(K, LP), lcoef = Rows<double>(K, LP * 3);
    points = Rows<orblm_point_record>(N, P), lines = Rows<orblm_line_record>(N, NB * LP);
    n_points = RowsI(N, 1), point_record = RowsI(N, P), pairs = RowsI(N, NB);
    n_lines = RowsI(N, 1), line_record = RowsI(N, LP), line_pairs = RowsI(N, NB);
    for (size_t k = 0; k < K; k++) {
      const orblm_keyframe& f = *kfs[k];
      const size_t m = (reads & kReadPoints) ? f.n : 0, ml = (reads & kReadLines) ? f.nl : 0;
      id.at(k) = f.id;
      Tcw.put(k, f.Tcw, 16);
      n.at(k) = (int32_t)m;
      kps.put(k, f.kps, m);
      kps_un.put(k, f.kps_un, m);
      uright.put(k, f.uright, m);
      depth.put(k, f.depth, m);
      desc.put(k, f.desc, m * 32);
      feat_node.put(k, f.feat_node, m);
      has_mp.put(k, f.has_mp, m);
      if (reads & kReadMapPoints) mp_xyz.put(k, f.mp_xyz, m * 3);
      nl.at(k) = (int32_t)ml;
      klines.put(k, f.klines, ml);
      ldesc.put(k, f.ldesc, ml * 32);
      lcoef.put(k, f.lcoef, ml * 3);
    }
  }
  // the out columns to problems[0 .. cur.size())
  void unpack(orblm_problem* problems) {
    for (size_t p = 0; p < cur.size(); p++) {
      orblm_problem& r = problems[p];
      r.n_points = n_points.at(p);
      r.n_lines = n_lines.at(p);
      pairs.take(p, r.pairs, NB);
      line_pairs.take(p, r.line_pairs, NB);
      if (r.cur.n > 0) {
        point_record.take(p, r.kf1_point_record, r.cur.n);
        points.take(p, r.points, r.n_points);
      }
      if (r.cur.nl > 0) {
        line_record.take(p, r.kf1_line_record, r.cur.nl);
        lines.take(p, r.lines, r.n_lines);
      }
    }
  }
};

}  // namespace orbpl
