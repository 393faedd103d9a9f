"""GPU: the batched PnP solver (orbpnp_iterate, orbpnp_iterate_batch_device;
csrc/pnp.hip) against the sequential restatement tests/_pnp_ref.py on the
admissible problems of tests/_pnp_problems.py. result, no_more, n_inliers, the
inlier mask, draws_consumed and the returned state are equal; poses agree
within 1e-4 absolute (the project's pose bound; the aim is bit equality and
each test prints the difference it measured)."""
import copy

import numpy as np
import pytest

from _pnp_problems import DEFAULTS, big_problem, make_problem, problems, ref_run

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-4
PROBLEMS = problems()


def _kernel_problem(orbpl, p, state=None, offset=0, draws=None, params=DEFAULTS):
    mn, mx, _, me = orbpl.pnp_ransac_parameters(len(p["p2d"]), *params, sigma2=p["sigma2"])
    return dict(cam=p["cam"], p2d=p["p2d"], p3d=p["p3d"], max_error=me, min_inliers=mn,
                max_its=mx, draws=p["draws"][offset:] if draws is None else draws, state=state)


def _same(got, want, want_state, what):
    """Returns the largest pose difference."""
    for k in ("result", "no_more", "n_inliers", "draws_consumed"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert np.array_equal(got["inliers"], want["inliers"]), what
    st = got["state"]
    assert st["iterations"] == want_state["iterations"], what
    assert st["best_inliers"] == want_state["best_inliers"], what
    assert np.array_equal(st["best_mask"].astype(bool), want_state["best_mask"]), what
    d = max(float(np.abs(got["Tcw"].astype(np.float64) - want["Tcw"]).max()),
            float(np.abs(st["best_Tcw"].astype(np.float64) - want_state["best_Tcw"]).max()))
    assert d <= POSE_TOL, (what, d)
    return d


def _drive(orbpl, p, what):
    """iterate(5) until a pose or bNoMore, then one more call on the final
    state, kernel and restatement side by side"""
    r = ref_run(p)
    state, worst = None, 0.0
    for off, o, st in r["calls"]:
        got = orbpl.pnp_iterate_batch([_kernel_problem(orbpl, p, state, off)], 5)[0]
        worst = max(worst, _same(got, o, st, what))
        state = got["state"]
    s = copy.deepcopy(r["solver"])
    off = r["calls"][-1][0] + r["calls"][-1][1]["draws_consumed"]
    o = s.iterate(5, p["draws"][off:])
    got = orbpl.pnp_iterate_batch([_kernel_problem(orbpl, p, state, off)], 5)[0]
    worst = max(worst, _same(got, o, s.state(), what + " (later call)"))
    print(f"{what}: calls {len(r['calls'])} + 1, result {r['calls'][-1][1]['result']}, "
          f"max |Tcw difference| {worst:g}")
    return r


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_driven_problem_equals_restatement(orbpl, name):
    _drive(orbpl, PROBLEMS[name], name)


def test_too_few_and_no_points_end_at_once(orbpl):
    for p in (PROBLEMS["N8_o0_s1"], make_problem(0, seed=1)):
        got = orbpl.pnp_iterate_batch([_kernel_problem(orbpl, p)], 5)[0]
        assert got["no_more"] and got["result"] == 0 and got["draws_consumed"] == 0
        assert got["n_inliers"] == 0 and got["state"]["iterations"] == 0
        assert not got["Tcw"].any() and not got["inliers"].any()


def test_refine_at_the_point_cap(orbpl):
    """N = 2048, all inliers: Refine() over ORBPNP_MAX_POINTS correspondences"""
    p = big_problem()
    r = _drive(orbpl, p, p["name"])
    o = r["calls"][-1][1]
    assert o["result"] == 1 and o["n_inliers"] == 2048
    assert np.abs(o["Tcw"].astype(np.float64) - p["Tcw"]).max() < 1e-3


def test_identical_world_points_end(orbpl):
    """no pose exists; every loop of the kernel is bounded"""
    p = PROBLEMS["identical_N20"]
    got = orbpl.pnp_iterate_batch([_kernel_problem(orbpl, p)], 5)[0]
    assert got["no_more"] and got["result"] == 0 and got["n_inliers"] == 0
    assert got["draws_consumed"] == 4 * 35


def _mixed(count):
    names = sorted(PROBLEMS)
    return [PROBLEMS[names[(3 * k) % len(names)]] for k in range(count)]


@pytest.mark.parametrize("count", [1, 3, 70])
def test_batches_of_mixed_sizes_host_and_device(orbpl, count):
    ps = _mixed(count)
    refs = [ref_run(p)["calls"][0] for p in ps]
    kp = [_kernel_problem(orbpl, p) for p in ps]
    host = orbpl.pnp_iterate_batch(kp, 5)
    dev = orbpl.PnpDeviceProblems(kp)
    dev.iterate(5)
    devo = dev.download()
    worst = 0.0
    for p, (off, o, st), h, d in zip(ps, refs, host, devo):
        worst = max(worst, _same(h, o, st, p["name"] + " host"),
                    _same(d, o, st, p["name"] + " device"))
        assert np.array_equal(h["Tcw"], d["Tcw"])
    print(f"batch of {count}: max |Tcw difference| {worst:g}")


def test_over_the_caps_is_an_argument_error(orbpl):
    p = PROBLEMS["N15_o0_s3"]
    draws = np.zeros(4 * 400, np.int32)
    with pytest.raises(orbpl.OrbplError, match="failed with -1"):
        orbpl.pnp_iterate_batch([_kernel_problem(orbpl, p, draws=draws)],
                                orbpl.PNP_MAX_ITERATIONS + 1)
    # exactly at the cap is accepted
    got = orbpl.pnp_iterate_batch([_kernel_problem(orbpl, p, draws=draws)],
                                  orbpl.PNP_MAX_ITERATIONS)[0]
    assert got["draws_consumed"] % 4 == 0 and got["draws_consumed"] > 0
    with pytest.raises(orbpl.OrbplError, match="failed with -1"):     # too few draws
        orbpl.pnp_iterate_batch([_kernel_problem(orbpl, p, draws=draws[:8])], 5)
    kp = _kernel_problem(orbpl, p)
    kp["min_inliers"] = 3                                             # below minSet = 4
    with pytest.raises(orbpl.OrbplError, match="failed with -1"):
        orbpl.pnp_iterate_batch([kp], 5)
    big = make_problem(orbpl.PNP_MAX_POINTS + 1, seed=2)
    with pytest.raises(orbpl.OrbplError, match="failed with -1"):
        orbpl.pnp_iterate_batch([_kernel_problem(orbpl, big)], 5)
