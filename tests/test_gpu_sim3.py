"""GPU: the batched Sim3 solver (orbsim3_iterate, orbsim3_iterate_batch_device,
orbsim3_setup_batch_device; csrc/sim3.hip) against the sequential restatement
tests/_sim3_ref.py on the admissible problems of tests/_sim3_problems.py.
result, no_more, n_inliers, the inlier mask, draws_consumed and the integer
state are equal; T12 and the best R / t / s agree within 1e-4 absolute (the
project's pose bound; the aim is bit equality and each test prints the
difference it measured). An entry that is not a number must be one on both
sides."""
import copy

import numpy as np
import pytest

import _sim3_ref as ref
from _sim3_problems import (SIGMA2, TRUNCATED_POINT, big_problems, collinear_points,
                            exactly_min_inliers, identical_points, make_problem, problems,
                            pure_translation, ref_run, ref_solver, truncated_threshold)

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-4
PROBLEMS = problems()


def _corr(p):
    if "_corr" not in p:
        p["_corr"] = ref.setup(p["pair"], SIGMA2)
    return p["_corr"]


def _kernel_problem(orbpl, p, state=None, offset=0, draws=None, max_its=None):
    c = _corr(p)
    mx = orbpl.sim3_ransac_parameters(c["n"], 0.99, p["min_inliers"], 300)
    return dict(cam=p["pair"]["cam"], corr=c, min_inliers=p["min_inliers"],
                max_its=mx if max_its is None else max_its, fix_scale=p["fix_scale"],
                draws=p["draws"][offset:] if draws is None else draws, state=state)


def _diff(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, what
    assert np.array_equal(np.isnan(a), np.isnan(b)), (what, "not-a-number entries differ")
    ok = ~np.isnan(a)
    return float(np.abs(a[ok] - b[ok]).max()) if ok.any() else 0.0


def _same(got, want, want_state, what):
    """Returns the largest pose difference."""
    for k in ("result", "no_more", "n_inliers", "draws_consumed"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert np.array_equal(got["inliers"], want["inliers"]), what
    st = got["state"]
    assert st["iterations"] == want_state["iterations"], what
    assert st["best_inliers"] == want_state["best_inliers"], what
    assert np.array_equal(st["best_mask"].astype(bool), want_state["best_mask"]), what
    d = max(_diff(got["T12"], want["T12"], what),
            _diff(st["best_T12"], want_state["best_T12"], what),
            _diff(st["best_R"].reshape(9), want_state["best_R"], what),
            _diff(st["best_t"], want_state["best_t"], what),
            _diff(st["best_s"], want_state["best_s"], what))
    assert d <= POSE_TOL, (what, d)
    return d


def _drive(orbpl, p, what):
    """iterate(5) until a Sim3 or bNoMore, then one more call on the final
    state, kernel and restatement side by side"""
    r = ref_run(p)
    state, worst = None, 0.0
    for off, o, st in r["calls"]:
        got = orbpl.sim3_iterate_batch([_kernel_problem(orbpl, p, state, off)], 5)[0]
        worst = max(worst, _same(got, o, st, what))
        state = got["state"]
    s = copy.deepcopy(r["solver"])
    off = r["calls"][-1][0] + r["calls"][-1][1]["draws_consumed"]
    o = s.iterate(5, p["draws"][off:])
    got = orbpl.sim3_iterate_batch([_kernel_problem(orbpl, p, state, off)], 5)[0]
    worst = max(worst, _same(got, o, s.state(), what + " (later call)"))
    print(f"{what}: calls {len(r['calls'])} + 1, result {r['calls'][-1][1]['result']}, "
          f"max |pose difference| {worst:g}")
    return r


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_driven_problem_equals_restatement(orbpl, name):
    _drive(orbpl, PROBLEMS[name], name)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_driven_problem_at_the_point_cap(orbpl, k):
    p = big_problems()[k]
    r = _drive(orbpl, p, p["name"])
    assert r["calls"][-1][1]["result"] == 1


@pytest.mark.parametrize("name", ["N100_o60_free_s121", "N257_o154_fix_s124",
                                  "N25_o15_fix_s112"])
def test_find_is_one_call_of_up_to_300(orbpl, name):
    p = PROBLEMS[name]
    s = ref_solver(p)
    o = s.find(p["draws"])
    got = orbpl.sim3_iterate_batch([_kernel_problem(orbpl, p)], s.max_its)[0]
    d = _same(got, o, s.state(), name)
    print(f"find {name}: result {o['result']}, hypotheses {o['draws_consumed'] // 3}, "
          f"max |pose difference| {d:g}")


def test_solver_class_draws_from_rand(orbpl):
    """Sim3Solver over the C library's rand(): the same draws given explicitly
    reproduce it, and the getters return the best state"""
    p = PROBLEMS["N100_o30_free_s132"]
    orbpl.pnp_srand(11)
    draws = orbpl._pnp_take_rand(3 * 300).copy()
    orbpl.pnp_srand(11)
    a = orbpl.Sim3Solver(p["pair"], SIGMA2, p["fix_scale"])
    a.SetRansacParameters(0.99, p["min_inliers"], 300)
    b = orbpl.Sim3Solver(p["pair"], SIGMA2, p["fix_scale"])
    b.SetRansacParameters(0.99, p["min_inliers"], 300)
    s = ref_solver(p)
    off = 0
    for _ in range(60):
        Ta, nma, vba, na = a.iterate(5)
        Tb, nmb, vbb, nb = b.iterate(5, draws[off:])
        o = s.iterate(5, draws[off:])
        off += o["draws_consumed"]
        assert (Ta is None) == (Tb is None) == (o["result"] == 0)
        assert nma == nmb == o["no_more"] and na == nb == o["n_inliers"]
        assert np.array_equal(vba, vbb) and vba.sum() == na
        assert np.array_equal(np.flatnonzero(vba), s.c["indices1"][o["inliers"]])
        if Ta is not None or nma:
            break
    assert Ta is not None and np.array_equal(Ta, Tb)
    assert _diff(a.GetEstimatedRotation().reshape(9), s.best_R, "R") <= POSE_TOL
    assert _diff(a.GetEstimatedTranslation(), s.best_t, "t") <= POSE_TOL
    assert _diff(a.GetEstimatedScale(), s.best_s, "s") <= POSE_TOL
    T, vb, n = orbpl.Sim3Solver(p["pair"], SIGMA2, p["fix_scale"]).find(draws)
    assert T is not None and n == vb.sum()


def test_too_few_and_no_points_end_at_once(orbpl):
    for N in (0, 2, 5):
        p = make_problem(N, seed=9, extras=False, min_inliers=6, name=f"few{N}")
        got = orbpl.sim3_iterate_batch([_kernel_problem(orbpl, p)], 5)[0]
        assert got["no_more"] and got["result"] == 0 and got["draws_consumed"] == 0
        assert got["n_inliers"] == 0 and got["state"]["iterations"] == 0
        assert not got["T12"].any() and not got["inliers"].any()
        _same(got, ref_solver(p).iterate(5, p["draws"]), ref_solver(p).state(), p["name"])


def test_exactly_min_inliers_runs_to_exhaustion(orbpl):
    p = exactly_min_inliers()
    r = _drive(orbpl, p, p["name"])
    s = r["solver"]
    assert all(o["result"] == 0 for _, o, _ in r["calls"]) and r["calls"][-1][1]["no_more"]
    assert s.best_inliers == 6 and s.iterations == s.max_its
    # the next call consumes nothing and needs no draw
    got = orbpl.sim3_iterate_batch(
        [_kernel_problem(orbpl, p, r["calls"][-1][2], draws=np.zeros(0, np.int32))], 5)[0]
    assert got["draws_consumed"] == 0 and got["no_more"] and got["result"] == 0
    assert got["state"]["iterations"] == s.max_its and got["state"]["best_inliers"] == 6


@pytest.mark.parametrize("make", [pure_translation, identical_points, collinear_points])
def test_degenerate_samples(orbpl, make):
    """pure translation in exact floats and three identical points give a T12
    that is not a number: 0 inliers, stored as the best by >=. Every loop of the
    kernel is bounded."""
    p = make()
    s = ref_solver(p)
    o = s.iterate(1, p["draws"])
    got = orbpl.sim3_iterate_batch([_kernel_problem(orbpl, p)], 1)[0]
    _same(got, o, s.state(), p["name"] + " first hypothesis")
    if make is not collinear_points:
        st = got["state"]
        assert st["best_inliers"] == 0 and st["iterations"] == 1
        assert np.isnan(st["best_T12"][:3]).all() and not st["best_mask"].any()
    _drive(orbpl, p, p["name"])


def test_truncated_threshold(orbpl):
    """an error between floor(9.21 sigma2) and 9.21 sigma2 is an outlier"""
    p = truncated_threshold()
    r = _drive(orbpl, p, p["name"])
    o = r["calls"][0][1]
    got = orbpl.sim3_iterate_batch([_kernel_problem(orbpl, p)], 5)[0]
    assert got["result"] == 1 and got["n_inliers"] == 8 == o["n_inliers"]
    assert not got["inliers"][TRUNCATED_POINT] and got["inliers"].sum() == 8


def test_a_later_tie_replaces_the_best(orbpl):
    p = make_problem(10, noise=0.0, seed=31, extras=False, min_inliers=10, name="tie")
    s = ref_solver(p)
    s.max_its = 4
    o = s.iterate(2, p["draws"])
    got = orbpl.sim3_iterate_batch([_kernel_problem(orbpl, p, max_its=4)], 2)[0]
    _same(got, o, s.state(), "tie, two hypotheses")
    first = got["state"]["best_T12"].copy()
    o = s.iterate(1, p["draws"][6:])
    got = orbpl.sim3_iterate_batch([_kernel_problem(orbpl, p, got["state"], 6, max_its=4)], 1)[0]
    _same(got, o, s.state(), "tie, third hypothesis")
    assert got["state"]["best_inliers"] == 10 and not np.array_equal(first, got["state"]["best_T12"])


def _mixed(count):
    names = sorted(PROBLEMS)
    return [PROBLEMS[names[(5 * k) % len(names)]] for k in range(count)]


@pytest.mark.parametrize("count", [1, 3, 70])
def test_batches_of_mixed_sizes_host_and_device(orbpl, count):
    """the host entry over the host setup, and Sim3DeviceProblems with the
    setup kernel: equal to the restatement and to each other byte for byte"""
    ps = _mixed(count)
    refs = [ref_run(p)["calls"][0] for p in ps]
    host_corr = orbpl.sim3_setup([p["pair"] for p in ps], SIGMA2)
    host = orbpl.sim3_iterate_batch([dict(_kernel_problem(orbpl, p), corr=c)
                                     for p, c in zip(ps, host_corr)], 5)
    dev = orbpl.Sim3DeviceProblems([dict(p["pair"], fix_scale=p["fix_scale"], draws=p["draws"],
                                         min_inliers=p["min_inliers"]) for p in ps], SIGMA2)
    dev.setup()
    dev.iterate(5)
    devo = dev.download()
    worst = 0.0
    for p, (off, o, st), h, d, hc in zip(ps, refs, host, devo, host_corr):
        worst = max(worst, _same(h, o, st, p["name"] + " host"),
                    _same(d, o, st, p["name"] + " device"))
        assert d["corr"]["n"] == hc["n"]
        for k in hc:
            if k != "n":
                assert d["corr"][k].tobytes() == hc[k].tobytes(), (p["name"], k)
        for k in ("T12",):
            assert h[k].tobytes() == d[k].tobytes(), (p["name"], k)
        for k in ("best_T12", "best_R", "best_t", "best_mask"):
            assert np.asarray(h["state"][k]).tobytes() == np.asarray(d["state"][k]).tobytes(), \
                (p["name"], k)
        assert np.float32(h["state"]["best_s"]).tobytes() == np.float32(d["state"]["best_s"]).tobytes()
    print(f"batch of {count}: max |pose difference| {worst:g}")


def test_over_the_caps_is_an_argument_error(orbpl):
    p = PROBLEMS["N25_o15_fix_s112"]
    draws = np.zeros(3 * 400, np.int32)
    kp = _kernel_problem(orbpl, p, draws=draws, max_its=400)
    with pytest.raises(orbpl.OrbplError, match="failed with -1"):
        orbpl.sim3_iterate_batch([kp], orbpl.SIM3_MAX_ITERATIONS + 1)
    got = orbpl.sim3_iterate_batch([kp], orbpl.SIM3_MAX_ITERATIONS)[0]   # at the cap
    assert got["draws_consumed"] <= 3 * orbpl.SIM3_MAX_ITERATIONS
    with pytest.raises(orbpl.OrbplError, match="failed with -1"):        # one draw short
        orbpl.sim3_iterate_batch([dict(kp, draws=draws[:14])], 5)
    assert orbpl.sim3_iterate_batch([dict(kp, draws=draws[:15])], 5)[0]["draws_consumed"] == 15
    with pytest.raises(orbpl.OrbplError, match="failed with -1"):
        orbpl.sim3_iterate_batch([dict(kp, min_inliers=2)], 5)
    orbpl.sim3_iterate_batch([dict(kp, min_inliers=3)], 5)
    # 2049 correspondences
    big = _corr(big_problems()[0])
    over = {k: (np.concatenate([v, v[:1]]) if k != "n" else 2049) for k, v in big.items()}
    q = dict(cam=p["pair"]["cam"], corr=over, min_inliers=20, max_its=5, fix_scale=False,
             draws=draws)
    with pytest.raises(orbpl.OrbplError, match="failed with -1"):
        orbpl.sim3_iterate_batch([q], 5)
    assert orbpl.sim3_iterate_batch([dict(q, corr=big)], 5)[0]["draws_consumed"] > 0
    # 2049 features in a keyframe
    pair = big_problems()[0]["pair"]
    grown = dict(pair, matched12=np.append(pair["matched12"], -1).astype(np.int32),
                 valid1=np.append(pair["valid1"], 1).astype(np.uint8),
                 xyz1=np.concatenate([pair["xyz1"], pair["xyz1"][:1]]),
                 octave1=np.append(pair["octave1"], 0).astype(np.int32))
    with pytest.raises(orbpl.OrbplError, match="failed with -1"):
        orbpl.sim3_setup([grown], SIGMA2)
    assert orbpl.sim3_setup([pair], SIGMA2)[0]["n"] == 2048
