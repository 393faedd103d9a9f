// The host side of the LocalMapping calls' map (orblm_map): the
// maps of one host call flattened into the pooled arrays that map_rows.h reads
// on the device. Host code over std::vector, no HIP call: an entry point adds
// its maps, packs the columns its kernel reads, stages them through its own
// HostStage, copies the device's columns back into the same vectors and unpacks
// the ones the call writes. The layout, stated here and nowhere else:
//   - problem p is the row prob[5 p ..] = (kf0, nkf, mp0, nmp, last): its
//     keyframes are the pool's [kf0, kf0 + nkf), its points [mp0, mp0 + nmp);
//     `last` is the call's own (a current keyframe, or its id);
//   - a per-feature column has `pitch` entries per keyframe (the widest n of the
//     call, at least 1), `ordered` 64; a per-point column has max(nmp, 1) rows;
//   - what no map fills is padding: mp -1, uright -1.0f, ordered -1, bad 1,
//     every other column 0.
#pragma once
#include <string.h>

#include <algorithm>
#include <vector>

#include "map_rows.h"

namespace orbpl {

struct MapPool {
  enum : uint32_t {
    // per keyframe
    kId = 1u << 0, kN = 1u << 1, kTcw = 1u << 2, kKpsUn = 1u << 3, kUright = 1u << 4,
    kKfDesc = 1u << 5, kMp = 1u << 6, kOrdered = 1u << 7,
    // per point, in/out
    kXyz = 1u << 8, kNormal = 1u << 9, kMinDist = 1u << 10, kMaxDist = 1u << 11, kDesc = 1u << 12,
    kRefKf = 1u << 13, kBad = 1u << 14, kNVisible = 1u << 15, kNFound = 1u << 16,
    // per point, out: pack only sizes them for the copy back (a call of its own
    // after the launch keeps that off the path to the launch)
    kReplacedBy = 1u << 17, kNObs = 1u << 18, kObs = 1u << 19, kDescSrc = 1u << 20,
    kOut = kReplacedBy | kNObs | kObs | kDescSrc, kIn = (1u << 17) - 1,
  };

  std::vector<const orblm_map*> maps;
  std::vector<int32_t> prob;
  std::vector<const void*> owned;   // the arrays the call writes: add names the slot arrays, the entry the rest
  int nkf = 0, nmp = 0, pitch = 1;
  std::vector<int32_t> id, n, mp, ordered, ref_kf, n_visible, n_found, replaced_by, n_obs, desc_src;
  std::vector<float> Tcw, uright, xyz, normal, min_dist, max_dist;
  std::vector<orbpl_keypoint> kps_un;
  std::vector<uint8_t> kf_desc, desc, bad;
  std::vector<int16_t> obs;

  void add(const orblm_map& m, int last) {
    maps.push_back(&m);
    prob.insert(prob.end(), {nkf, m.nkf, nmp, m.M, last});
    nkf += m.nkf;
    nmp += m.M;
    for (int k = 0; k < m.nkf; k++) {
      pitch = std::max(pitch, m.kf[k].n);
      if (m.kf[k].n) owned.push_back(m.kf[k].mp);
    }
  }
  // true if one array is owned twice: what a call writes belongs to one problem
  bool shares_an_array() {
    std::sort(owned.begin(), owned.end());
    return std::adjacent_find(owned.begin(), owned.end()) != owned.end();
  }
  size_t kf0(int p) const { return (size_t)prob[5 * p]; }
  size_t mp0(int p) const { return (size_t)prob[5 * p + 2]; }
  size_t K() const { return (size_t)nkf; }
  size_t P() const { return (size_t)pitch; }
  size_t M() const { return (size_t)std::max(nmp, 1); }   // no array of the pools is empty

  // after every add: the columns of `cols`, padded; no other vector is touched
  void pack(uint32_t cols) {
    const size_t K = this->K(), P = this->P();
    if (cols & kId) id.assign(K, 0);
    if (cols & kN) n.assign(K, 0);
    if (cols & kTcw) Tcw.assign(K * 16, 0.0f);
    if (cols & kKpsUn) kps_un.assign(K * P, orbpl_keypoint());
    if (cols & kUright) uright.assign(K * P, -1.0f);
    if (cols & kKfDesc) kf_desc.assign(K * P * 32, 0);
    if (cols & kMp) mp.assign(K * P, -1);
    if (cols & kOrdered) ordered.assign(K * kMapKF, -1);
    size_t g = 0;
    for (const orblm_map* m : maps)
      for (int k = 0; k < m->nkf; k++, g++) {
        const orblm_map_keyframe& f = m->kf[k];
        const size_t nf = (size_t)f.n;
        if (cols & kId) id[g] = f.id;
        if (cols & kN) n[g] = f.n;
        if (cols & kTcw) memcpy(&Tcw[g * 16], f.Tcw, 64);
        if ((cols & kKpsUn) && nf) memcpy(&kps_un[g * P], f.kps_un, nf * sizeof(orbpl_keypoint));
        if ((cols & kUright) && nf) memcpy(&uright[g * P], f.uright, nf * 4);
        if ((cols & kKfDesc) && nf) memcpy(&kf_desc[g * P * 32], f.desc, nf * 32);
        if ((cols & kMp) && nf) memcpy(&mp[g * P], f.mp, nf * 4);
        if ((cols & kOrdered) && f.ordered)
          for (int x = 0; x < kMapKF && f.ordered[x] >= 0; x++) ordered[g * kMapKF + x] = f.ordered[x];
      }
    points(cols, false);
  }

  // the columns of `cols` (packed, then overwritten with the device's) back to
  // the maps: the first n entries of a keyframe's row, the first M of a map
  void unpack(uint32_t cols) {
    size_t g = 0;
    for (const orblm_map* m : maps)
      for (int k = 0; k < m->nkf; k++, g++)
        if ((cols & kMp) && m->kf[k].n) memcpy(m->kf[k].mp, &mp[g * P()], (size_t)m->kf[k].n * 4);
    points(cols, true);
  }

 private:
  // a per-point column of w elements: sized, padded and (an in column) filled
  // from the maps, or (back) a map's first M rows copied back to it
  template <class T>
  void point(bool on, bool back, std::vector<T>& v, size_t w, T* orblm_map::*a, bool in = true, T pad = T()) {
    if (!on) return;
    if (!back) v.assign(M() * w, pad);
    size_t q = 0;
    for (const orblm_map* m : maps) {
      const size_t bytes = (size_t)m->M * w * sizeof(T);
      if (back && bytes) memcpy(m->*a, &v[q * w], bytes);
      if (!back && in && bytes) memcpy(&v[q * w], m->*a, bytes);
      q += (size_t)m->M;
    }
  }
  void points(uint32_t cols, bool back) {
    typedef orblm_map Q;
    point(cols & kXyz, back, xyz, 3, &Q::xyz);
    point(cols & kNormal, back, normal, 3, &Q::normal);
    point(cols & kMinDist, back, min_dist, 1, &Q::min_dist);
    point(cols & kMaxDist, back, max_dist, 1, &Q::max_dist);
    point(cols & kDesc, back, desc, 32, &Q::desc);
    point(cols & kRefKf, back, ref_kf, 1, &Q::ref_kf);
    point(cols & kBad, back, bad, 1, &Q::bad, true, (uint8_t)1);
    point(cols & kNVisible, back, n_visible, 1, &Q::n_visible);
    point(cols & kNFound, back, n_found, 1, &Q::n_found);
    point(cols & kReplacedBy, back, replaced_by, 1, &Q::replaced_by, false);
    point(cols & kNObs, back, n_obs, 1, &Q::n_obs, false);
    point(cols & kObs, back, obs, kMapKF, &Q::obs, false);
    point(cols & kDescSrc, back, desc_src, 2, &Q::desc_src, false);
  }
};

}  // namespace orbpl
