"""Sequential restatement of Tracking::Relocalization (src/Tracking.cc:2049-2269)
under the project's pins P30-P32, one statement after the other as
the C++ reads. It composes the restatements and oracles of its parts:

  _reloc_ref.detect_reloc               DetectRelocalizationCandidates
  oracle.search_by_bow(nnratio=0.75)    ORBmatcher(0.75, true).SearchByBoW
  _pnp_ref.PnPsolver                    PnPsolver, SetRansacParameters, iterate
  oracle.pose_optimization              Optimizer::PoseOptimization
  _reloc_ref.search_by_projection_kf    ORBmatcher(0.9, true).SearchByProjection

It knows nothing of the library's parallel schedule: candidates are visited
one after the other inside the reference's while loop, and the frame's
mvpMapPoints / mvbOutlier / mTcw are the single shared members of
mCurrentFrame. What the pins add:
  P30  candidate c draws from its own stream draws[c] at its own cursor
  P31  a candidate whose next iterate(5) may need more draws than its stream
       has left ends the call with status DRAW_EXHAUSTED
  P32  on failure the outputs are cleared; a map point is named by the
       keyframe feature that holds it; outlier[] is reported where a map
       point is assigned
Besides the outputs it returns a branch trace and the solvers' margins."""
import numpy as np

import _pnp_ref
from _pkg import load_oracle
from _reloc_ref import RefFrame, detect_reloc, search_by_projection_kf

OK, NO_CANDIDATES, FAILED, DRAW_EXHAUSTED = 0, 1, 2, 3
REC = ("bow_matches", "discarded", "calls", "iterations", "draws_used", "result", "no_more",
       "n_inliers", "g1", "nadd1", "g2", "nadd2", "g3")
RELOC_PARAMS = (0.99, 10, 300, 4, 0.5, 5.991)


def _new_record():
    r = dict.fromkeys(REC, 0)
    r.update(g1=-1, nadd1=-1, g2=-1, nadd2=-1, g3=-1)
    return r


def relocalize(P, cfg, bounds, scale, sigma2, skip=()):
    """P: the problem (see orbpl.Relocalizer); cfg: the camera settings dict;
    bounds = (minX, maxX, minY, maxY); scale / sigma2 = mvScaleFactors /
    mvLevelSigma2. skip: candidate positions to treat as discarded from the
    start (a test's way to ask what a later candidate would have done).
    Returns the outputs of orbpl.Relocalizer.relocalize_batch plus ``trace``
    (set of branch names) and ``margins`` (one _pnp_ref.Margins per solver)."""
    O = load_oracle()
    cam = O.camera(cfg)
    cam4 = (cfg["fx"], cfg["fy"], cfg["cx"], cfg["cy"])
    F = P["frame"]
    kps = F["kps_un"]
    N = len(kps)
    sigma2 = np.asarray(sigma2, np.float32)
    inv_sigma2 = (np.float32(1.0) / sigma2).astype(np.float32)
    draws = np.asarray(P["draws"], np.int32)
    draws = draws.reshape(-1, draws.shape[-1]) if draws.size else np.zeros((0, 0), np.int32)
    trace, margins = set(), []

    # Step 2: the candidates
    cand, _, score, _ = detect_reloc(P["kf_bows"], P.get("covis", []), P["reloc_score"],
                                     F["bow_words"], F["bow_vals"])
    out = dict(ok=False, status=NO_CANDIDATES, winner=-1, rounds=0,
               Tcw=np.zeros((4, 4), np.float32), n_good=0, n_candidates=0,
               cand=np.array(cand, np.int32), mp_kf_feature=np.full(N, -1, np.int32),
               outlier=np.zeros(N, np.uint8), records=[], reloc_score=score, trace=trace,
               margins=margins)
    if not cand:
        trace.add("no_candidates")
        return out
    nKFs = len(cand)
    recs = [_new_record() for _ in range(nKFs)]
    out["records"] = recs

    # Step 3: SearchByBoW and a solver per candidate
    vvpMapPointMatches = [None] * nKFs
    vpPnPsolvers = [None] * nKFs
    vKeyPointIndices = [None] * nKFs
    vbDiscarded = [False] * nKFs
    cursor = [0] * nKFs
    nCandidates = 0
    for i in range(nKFs):
        kf = P["kfs"][cand[i]]
        m, nmatches = O.search_by_bow(kf["feat_node"], kf["valid"], kf["desc"], kf["angle"],
                                      F["feat_node"], F["desc"], kps["angle"], nnratio=0.75,
                                      check_ori=True)
        recs[i]["bow_matches"] = nmatches
        if nmatches < 15 or i in skip:
            vbDiscarded[i] = True
            recs[i]["discarded"] = 1
            continue
        vvpMapPointMatches[i] = m
        idx = np.flatnonzero(m >= 0)                        # mvKeyPointIndices
        xy = np.stack([kps["x"][idx], kps["y"][idx]], axis=1)
        s = _pnp_ref.PnPsolver(cam4, xy, sigma2[kps["octave"][idx]],
                               np.asarray(kf["mp_xyz"], np.float32)[m[idx]])
        s.SetRansacParameters(*RELOC_PARAMS)
        vpPnPsolvers[i] = s
        vKeyPointIndices[i] = idx
        margins.append(s.margins)
        nCandidates += 1
    if nCandidates == 0:
        trace.add("all_under_15")

    # mCurrentFrame's members
    mvpMapPoints = np.full(N, -1, np.int32)
    mvbOutlier = np.zeros(N, np.uint8)
    mTcw = np.zeros((4, 4), np.float32)

    def pose_optimization(kf):
        nonlocal mTcw, mvbOutlier
        has = mvpMapPoints >= 0
        xyz = np.zeros((N, 3), np.float32)
        xyz[has] = np.asarray(kf["mp_xyz"], np.float32)[mvpMapPoints[has]]
        prob = dict(kps_un=kps, uright=F["uright"], has_mp=has.astype(np.uint8), mp_xyz=xyz,
                    inv_sigma2=inv_sigma2)
        mTcw, mvbOutlier, _, n = O.pose_optimization(cam, prob, mTcw, mvbOutlier)
        return n

    def search_by_projection(kf, sFound, th, orb_dist):
        frame = RefFrame(cfg, bounds, scale, mTcw, kps, F["desc"])
        found = np.zeros(len(kf["angle"]), np.uint8)
        found[list(sFound)] = 1
        m, n = search_by_projection_kf(frame, mvpMapPoints >= 0, kf["angle"], kf["valid"], found,
                                       kf["mp_xyz"], kf["mp_min_dist"], kf["mp_max_dist"],
                                       kf["mp_desc"], th, orb_dist, True)
        mvpMapPoints[m >= 0] = m[m >= 0]
        return n

    # Step 4
    bMatch = False
    status = FAILED
    winner = -1
    nGood = 0
    rounds = 0
    failed_before = False
    while nCandidates > 0 and not bMatch and status != DRAW_EXHAUSTED:
        rounds += 1
        for i in range(nKFs):
            if vbDiscarded[i]:
                continue
            pSolver = vpPnPsolvers[i]
            kf = P["kfs"][cand[i]]
            rec = recs[i]
            # P31
            stream = draws[i] if i < len(draws) else np.zeros(0, np.int32)
            if 4 * max(pSolver.max_its - pSolver.iterations, 5) > len(stream) - cursor[i]:
                status = DRAW_EXHAUSTED
                trace.add("draw_exhausted")
                break
            o = pSolver.iterate(5, stream[cursor[i]:])
            cursor[i] += o["draws_consumed"]
            rec.update(calls=rec["calls"] + 1, iterations=pSolver.iterations,
                       draws_used=cursor[i], result=o["result"], no_more=int(o["no_more"]),
                       n_inliers=o["n_inliers"], g1=-1, nadd1=-1, g2=-1, nadd2=-1, g3=-1)
            if o["no_more"]:
                vbDiscarded[i] = True
                rec["discarded"] = 1
                nCandidates -= 1
                trace.add("exhaust_with_pose" if o["result"] else "exhaust_without_pose")
            if not o["result"]:
                failed_before = True
                continue
            mTcw = o["Tcw"].copy()
            sFound = set()
            mvpMapPoints[:] = -1
            idx = vKeyPointIndices[i]
            for j in range(len(idx)):                       # vbInliers, by keypoint
                if o["inliers"][j]:
                    mvpMapPoints[idx[j]] = vvpMapPointMatches[i][idx[j]]
                    sFound.add(int(vvpMapPointMatches[i][idx[j]]))
            nGood = pose_optimization(kf)
            rec["g1"] = nGood
            if nGood < 10:
                trace.add("ngood_lt10")
                failed_before = True
                continue
            mvpMapPoints[mvbOutlier != 0] = -1
            if nGood < 50:
                nadditional = search_by_projection(kf, sFound, 10, 100)
                rec["nadd1"] = nadditional
                if nadditional + nGood >= 50:
                    nGood = pose_optimization(kf)
                    rec["g2"] = nGood
                    if nGood >= 50:
                        trace.add("first_search_success")
                    if 30 < nGood < 50:
                        trace.add("second_search_entry")
                        sFound = set(int(v) for v in mvpMapPoints[mvpMapPoints >= 0])
                        nadditional = search_by_projection(kf, sFound, 3, 64)
                        rec["nadd2"] = nadditional
                        if nGood + nadditional >= 50:
                            nGood = pose_optimization(kf)
                            rec["g3"] = nGood
                            mvpMapPoints[mvbOutlier != 0] = -1
                            if nGood >= 50:
                                trace.add("second_search_success")
            else:
                trace.add("direct")
            if nGood >= 50:
                bMatch = True
                winner = i
                break
            failed_before = True
    out.update(rounds=rounds, n_candidates=nCandidates, status=status)
    if bMatch:
        if rounds >= 2:
            trace.add("win_round_ge2")
        if failed_before:
            trace.add("fail_then_later_wins" if any(
                recs[j]["calls"] > 0 for j in range(winner)) else "fail_then_same_wins")
        has = mvpMapPoints >= 0
        out.update(ok=True, status=OK, winner=int(cand[winner]), Tcw=mTcw.copy(), n_good=nGood,
                   mp_kf_feature=mvpMapPoints.copy(),
                   outlier=np.where(has, mvbOutlier, 0).astype(np.uint8))
    elif status == FAILED:
        trace.add("failed")
    return out
