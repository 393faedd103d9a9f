"""GPU: the batched Tracking::Relocalization (orbrl_relocalize; csrc/reloc.hip,
k_reloc_bow in csrc/match_local.hip) against the sequential restatement
tests/_relocalize_ref.py on every problem of tests/_relocalize_problems.py.
ok, status, winner, rounds, cand, the assignments, the outlier flags, n_good,
nCandidates, mRelocScore and every candidate record are equal; the pose agrees
within 1e-4 absolute (the project's pose bound; each test prints the
difference it measured). A batch gives every problem byte for byte what it
gives alone."""
import numpy as np
import pytest

import _relocalize_problems as RP

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-4
PROBLEMS = RP.problems()
_HANDLES = {}


def _relocalizer(orbpl, kp_pitch, draw_pitch, max_problems=32, cfg=RP.CFG):
    key = (kp_pitch, draw_pitch, cfg["k1"])
    if key not in _HANDLES:
        _HANDLES[key] = orbpl.Relocalizer(orbpl.make_camera(cfg), RP.SCALE, RP.SIGMA2,
                                          max_problems=max_problems, kp_pitch=kp_pitch,
                                          draw_pitch=draw_pitch)
    return _HANDLES[key]


def _run(orbpl, rl, problems):
    """relocalize_batch; a batch with a problem that runs out of draws raises,
    with the results attached (P31)"""
    try:
        return rl.relocalize_batch(problems), False
    except orbpl.OrbplError as e:
        assert "-5" in str(e), e
        return e.results, True


def _same(got, want, what):
    for k in ("ok", "status", "winner", "rounds", "n_good", "n_candidates"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert np.array_equal(got["cand"], want["cand"]), what
    assert got["records"] == want["records"], (what, got["records"], want["records"])
    assert np.array_equal(got["mp_kf_feature"], want["mp_kf_feature"]), what
    assert np.array_equal(got["outlier"], want["outlier"]), what
    assert got["reloc_score"].tobytes() == want["reloc_score"].tobytes(), what
    d = float(np.abs(got["Tcw"].astype(np.float64) - want["Tcw"]).max())
    assert d <= POSE_TOL, (what, d)
    return d


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_problem_equals_restatement(orbpl, name):
    P = PROBLEMS[name]
    want = RP.ref_run(name)
    rl = _relocalizer(orbpl, P["kp_pitch"], P["draw_pitch"], cfg=P["cfg"])
    (got,), raised = _run(orbpl, rl, [P])
    d = _same(got, want, name)
    assert raised == (want["status"] == 3), name
    if not got["ok"]:          # P32: cleared
        assert not got["Tcw"].any() and (got["mp_kf_feature"] == -1).all()
        assert not got["outlier"].any() and got["n_good"] == 0
    print(f"{name}: status {got['status']} rounds {got['rounds']} pose diff {d:.3g}")


def _bytes(r):
    return (r["ok"], r["status"], r["winner"], r["rounds"], r["n_good"], r["n_candidates"],
            r["cand"].tobytes(), r["Tcw"].tobytes(), r["mp_kf_feature"].tobytes(),
            r["outlier"].tobytes(), repr(r["records"]), r["reloc_score"].tobytes())


@pytest.mark.parametrize("draw_pitch,camera", [(1280, "synthetic"), (160, "synthetic"),
                                               (1280, "image")])
def test_batch_equals_alone(orbpl, draw_pitch, camera):
    """All problems in one shuffled batch at the 2048 pitch give each problem
    byte for byte what it gives alone. A handle has one camera and one draw
    pitch, so "all" is: every problem whose streams hold 1280 draws (all but
    second_entry, whose streams are 160 long) - once through the synthetic
    camera's handle without the image-derived problem, once through the image
    problem's camera with it (the synthetic problems then see a camera they
    were not made for: equality with themselves alone is what is checked, not
    the restatement) - and every problem with its streams cut to 160 draws."""
    cfg = PROBLEMS["image"]["cfg"] if camera == "image" else RP.CFG
    names = sorted(n for n in PROBLEMS
                   if (camera == "image" or PROBLEMS[n]["cfg"] is RP.CFG) and
                   (draw_pitch == 160 or PROBLEMS[n]["draw_pitch"] == 1280))
    assert ("image" in names) == (camera == "image")
    ps = [dict(PROBLEMS[n], draws=PROBLEMS[n]["draws"][:, :draw_pitch].copy()) for n in names]
    rl = _relocalizer(orbpl, 2048, draw_pitch, cfg=cfg)
    alone = [_run(orbpl, rl, [p])[0][0] for p in ps]
    order = np.random.default_rng(5).permutation(len(ps))
    got, _ = _run(orbpl, rl, [ps[i] for i in order])
    for j, i in enumerate(order):
        assert _bytes(got[j]) == _bytes(alone[i]), names[i]
    if camera == "synthetic":
        assert len({r["status"] for r in alone}) >= 3, "the batch mixes outcomes"
        assert len({len(r["cand"]) for r in alone}) >= 4, "and candidate counts 0, 1, 2, 4"
    else:
        assert alone[names.index("image")]["ok"]


def test_pitch_1024_equals_2048(orbpl):
    P = PROBLEMS["first_search"]
    a = _run(orbpl, _relocalizer(orbpl, 1024, 1280), [P])[0][0]
    b = _run(orbpl, _relocalizer(orbpl, 2048, 1280), [P])[0][0]
    assert _bytes(a) == _bytes(b)


def test_draw_exhaustion_is_reported(orbpl):
    """P31: ORBPL_ERR_OVERFLOW, status DRAW_EXHAUSTED, cleared outputs, and
    the other problem of the batch is unaffected"""
    rl = _relocalizer(orbpl, 1024, 160)
    direct = dict(PROBLEMS["direct"], draws=PROBLEMS["direct"]["draws"][:, :160].copy())
    with pytest.raises(orbpl.OrbplError) as ei:
        rl.relocalize_batch([PROBLEMS["second_entry"], direct])
    res = ei.value.results
    assert res[0]["status"] == orbpl.RL_DRAW_EXHAUSTED and not res[0]["ok"]
    assert not res[0]["Tcw"].any() and (res[0]["mp_kf_feature"] == -1).all()
    assert res[1]["ok"] and res[1]["n_good"] == 80


def test_argument_errors(orbpl):
    cam = orbpl.make_camera(RP.CFG)
    for kw in (dict(kp_pitch=1000), dict(draw_pitch=1282), dict(draw_pitch=16),
               dict(draw_pitch=1284), dict(max_problems=0)):
        with pytest.raises(orbpl.OrbplError):
            orbpl.Relocalizer(cam, RP.SCALE, RP.SIGMA2, **kw)
    rl = _relocalizer(orbpl, 1024, 1280)
    P = PROBLEMS["direct"]
    with pytest.raises(orbpl.OrbplError):
        rl.relocalize_batch([P], scoring=1)                       # only L1
    with pytest.raises(orbpl.OrbplError):
        rl.relocalize_batch([P] * 33)                             # max_problems
    many = dict(P, kf_bows=P["kf_bows"] * 65, kfs=P["kfs"] * 65, covis=[[]] * 65,
                reloc_score=np.zeros(65, np.float32))
    with pytest.raises(orbpl.OrbplError):
        rl.relocalize_batch([many])                               # 64 keyframes
    words = np.arange(5000, dtype=np.uint32)
    wide_bow = dict(P, frame=dict(P["frame"], bow_words=words, bow_vals=np.full(5000, 2e-4)))
    with pytest.raises(orbpl.OrbplError):
        rl.relocalize_batch([wide_bow])                           # 4096 words
    with pytest.raises(orbpl.OrbplError):
        rl.relocalize_batch([PROBLEMS["wide"]])                   # 1090 keypoints at pitch 1024
    assert rl.relocalize_batch([]) == []


def test_parameter_table(orbpl):
    import _pnp_ref
    mn, mx = orbpl.reloc_ransac_table()
    for n in range(orbpl.RL_TABLE_N + 1):
        want = _pnp_ref.ransac_parameters(n, 0.99, 10, 300, 4, 0.5, 5.991)
        assert (int(mn[n]), int(mx[n])) == want[:2], n


def test_device_entry_equals_host_entry(orbpl):
    """three problems packed into pitched device arrays by the test itself"""
    names = ["first_search", "fail_then_win", "round2"]
    ps = [PROBLEMS[n] for n in names]
    rl = _relocalizer(orbpl, 1024, 1280)
    want = rl.relocalize_batch(ps)
    NP, P, K, DP, SP = len(ps), 1024, 64, 1280, 2
    i32, f32, u8 = np.int32, np.float32, np.uint8
    nslots = sum(len(p["kfs"]) for p in ps)
    entp = max(sum(len(w) for w, _ in p["kf_bows"]) for p in ps)
    qp = max(len(p["frame"]["bow_words"]) for p in ps)
    h = dict(nkf=np.zeros(NP, i32), off=np.zeros((NP, K + 1), i32), kw=np.zeros((NP, entp), np.uint32),
             kv=np.zeros((NP, entp)), cov=np.full((NP, K, 10), -1, i32), rs=np.zeros((NP, K), f32),
             qn=np.zeros(NP, i32), qw=np.zeros((NP, qp), np.uint32), qv=np.zeros((NP, qp)),
             first=np.zeros(NP, i32), kfn=np.zeros(nslots, i32), kang=np.zeros((nslots, P), f32),
             knode=np.full((nslots, P), -1, i32), kdesc=np.zeros((nslots, P, 32), u8),
             kval=np.zeros((nslots, P), u8), xyz=np.zeros((nslots, P, 3), f32),
             mn=np.zeros((nslots, P), f32), mx=np.zeros((nslots, P), f32),
             mdesc=np.zeros((nslots, P, 32), u8), n=np.zeros(NP, i32),
             kps=np.zeros((NP, P), orbpl.KP_DTYPE), ur=np.full((NP, P), -1, f32),
             desc=np.zeros((NP, P, 32), u8), fnode=np.full((NP, P), -1, i32),
             draws=np.zeros((NP, SP, DP), i32), ns=np.zeros(NP, i32))
    slot = 0
    for p, pr in enumerate(ps):
        F = pr["frame"]
        n = len(F["kps_un"])
        h["nkf"][p], h["first"][p], h["n"][p] = len(pr["kfs"]), slot, n
        e = 0
        for k, ((w, v), kf) in enumerate(zip(pr["kf_bows"], pr["kfs"])):
            h["kw"][p, e:e + len(w)], h["kv"][p, e:e + len(w)] = w, v
            e += len(w)
            h["off"][p, k + 1] = e
            m = len(kf["angle"])
            h["kfn"][slot] = m
            for dst, src in (("kang", "angle"), ("knode", "feat_node"), ("kdesc", "desc"),
                             ("kval", "valid"), ("xyz", "mp_xyz"), ("mn", "mp_min_dist"),
                             ("mx", "mp_max_dist"), ("mdesc", "mp_desc")):
                h[dst][slot, :m] = kf[src]
            slot += 1
        h["qn"][p] = len(F["bow_words"])
        h["qw"][p, :h["qn"][p]], h["qv"][p, :h["qn"][p]] = F["bow_words"], F["bow_vals"]
        h["kps"][p, :n], h["ur"][p, :n] = F["kps_un"], F["uright"]
        h["desc"][p, :n], h["fnode"][p, :n] = F["desc"], F["feat_node"]
        h["ns"][p] = len(pr["draws"])
        h["draws"][p, :len(pr["draws"])] = pr["draws"]
    d = {k: orbpl.DeviceBuffer.from_array(np.ascontiguousarray(v)) for k, v in h.items()}
    out = dict(cand=(i32, (NP, K)), ncand=(i32, NP), ok=(i32, NP), status=(i32, NP),
               winner=(i32, NP), rounds=(i32, NP), n_good=(i32, NP), n_cands=(i32, NP),
               Tcw=(f32, (NP, 4, 4)), match=(i32, (NP, P)), outl=(u8, (NP, P)),
               rec=(i32, (NP, K, len(orbpl.RL_REC))))
    o = {k: orbpl.DeviceBuffer.from_array(np.zeros(s, t)) for k, (t, s) in out.items()}
    b = orbpl.RelocDeviceBatch(
        d["nkf"].ptr, d["off"].ptr, d["kw"].ptr, d["kv"].ptr, entp, d["cov"].ptr, d["rs"].ptr,
        d["qn"].ptr, d["qw"].ptr, d["qv"].ptr, qp, d["first"].ptr, d["kfn"].ptr, d["kang"].ptr,
        d["knode"].ptr, d["kdesc"].ptr, d["kval"].ptr, d["xyz"].ptr, d["mn"].ptr, d["mx"].ptr,
        d["mdesc"].ptr, d["n"].ptr, d["kps"].ptr, d["ur"].ptr, d["desc"].ptr, d["fnode"].ptr,
        d["draws"].ptr, d["ns"].ptr, SP, o["cand"].ptr, o["ncand"].ptr, o["ok"].ptr,
        o["status"].ptr, o["winner"].ptr, o["rounds"].ptr, o["n_good"].ptr, o["n_cands"].ptr,
        o["Tcw"].ptr, o["match"].ptr, o["outl"].ptr, o["rec"].ptr)
    rl.relocalize_batch_device(b, NP)
    g = {k: o[k].download(t, s) for k, (t, s) in out.items()}
    rs = d["rs"].download(f32, (NP, K))
    for p, w in enumerate(want):
        n, nc = int(h["n"][p]), int(g["ncand"][p])
        assert (bool(g["ok"][p]), g["status"][p], g["winner"][p], g["rounds"][p], g["n_good"][p],
                g["n_cands"][p]) == (w["ok"], w["status"], w["winner"], w["rounds"], w["n_good"],
                                     w["n_candidates"]), names[p]
        assert np.array_equal(g["cand"][p, :nc], w["cand"])
        assert g["Tcw"][p].tobytes() == w["Tcw"].tobytes()
        assert np.array_equal(g["match"][p, :n], w["mp_kf_feature"])
        assert np.array_equal(g["outl"][p, :n], w["outlier"])
        assert [dict(zip(orbpl.RL_REC, (int(v) for v in g["rec"][p, c]))) for c in range(nc)] == \
            w["records"]
        assert rs[p, :len(w["reloc_score"])].tobytes() == w["reloc_score"].tobytes()


def test_relocalize_with_vocabulary_and_rand(orbpl):
    """Relocalizer.relocalize on the image-derived problem: ComputeBoW through
    the vocabulary, the streams from the C library's rand() under srand(k),
    draw_pitch values per candidate in candidate order (P30)"""
    import _relocalize_ref as R
    P = PROBLEMS["image"]
    ncand = len(RP.ref_run("image")["cand"])
    orbpl.pnp_srand(9)
    draws = np.zeros((ncand, 1280), np.int32)
    for c in range(ncand):
        draws[c] = orbpl._pnp_take_rand(1280)
        del orbpl._pnp_rand_queue[:1280]
    nxt = int(orbpl._pnp_take_rand(1)[0])
    want = R.relocalize(dict(P, draws=draws), P["cfg"], P["bounds"], RP.SCALE, RP.SIGMA2)
    voc = orbpl.ORBVocabulary(RP.image_vocabulary())
    bare = dict(P, frame={k: P["frame"][k] for k in ("kps_un", "uright", "desc")})
    del bare["draws"]
    orbpl.pnp_srand(9)
    rl = _relocalizer(orbpl, 1024, 1280, cfg=P["cfg"])
    got = rl.relocalize(voc, bare, RP.IMAGE_LEVELSUP)
    _same(got, want, "image under srand(9)")
    assert int(orbpl._pnp_take_rand(1)[0]) == nxt      # unconsumed values were dropped
