"""CPU: the sequential restatement of Tracking::Relocalization
(tests/_relocalize_ref.py) on the synthetic problems of
tests/_relocalize_problems.py: every branch of the function is reached, the
planted answers come out, the solvers' margins are clean, and the
SetRansacParameters table the library uploads equals the restatement's."""
import numpy as np
import pytest

import _pnp_ref
import _relocalize_problems as RP
import _relocalize_ref as R

PROBLEMS = RP.problems()


def test_every_branch_is_reached():
    reached = set()
    for name, P in PROBLEMS.items():
        trace = RP.ref_run(name)["trace"]
        for b in P["expect"]["branches"]:
            assert b in trace, (name, b, sorted(trace))
        reached |= trace
    for b in RP.REQUIRED_BRANCHES:
        assert b in reached, b


def test_two_candidates_would_both_win():
    """the lower index is taken; with it out of the way the other one wins"""
    P = PROBLEMS["two_win"]
    r = RP.ref_run("two_win")
    assert r["ok"] and r["winner"] == r["cand"][0] == 0 and r["records"][1]["calls"] == 0
    r2 = R.relocalize(P, RP.CFG, RP.BOUNDS, RP.SCALE, RP.SIGMA2, skip=(0,))
    assert r2["ok"] and r2["winner"] == r2["cand"][1] == 1 and r2["n_good"] == 55


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_planted_answers(name):
    P, r = PROBLEMS[name], RP.ref_run(name)
    e = P["expect"]
    assert r["ok"] == e["ok"], name
    if r["ok"]:
        assert r["status"] == R.OK and r["winner"] == e["winner"]
        if "n_good" in e:      # noise-free: exactly the planted inliers
            assert r["n_good"] == e["n_good"]
            assert int((r["mp_kf_feature"] >= 0).sum()) == e["n_good"] and not r["outlier"].any()
        d = np.abs(r["Tcw"].astype(np.float64) - P["Tcw_true"]).max()
        assert d < (1e-3 if "n_good" in e else 5e-2), (name, d)
    else:                      # P32: cleared
        assert r["status"] != R.OK and r["winner"] == -1 and r["n_good"] == 0
        assert not r["Tcw"].any() and (r["mp_kf_feature"] == -1).all() and not r["outlier"].any()
    assert len(r["records"]) == len(r["cand"])


def test_margins_are_clean():
    for name in PROBLEMS:
        for m in RP.ref_run(name)["margins"]:
            assert not m.count_fragile, name


def test_round_and_stage_bookkeeping():
    r = RP.ref_run("round2")["records"][0]
    assert RP.ref_run("round2")["rounds"] >= 2 and r["calls"] == RP.ref_run("round2")["rounds"]
    r = RP.ref_run("second_entry")
    assert r["status"] == R.DRAW_EXHAUSTED and 30 < r["records"][0]["g2"] < 50
    assert r["records"][0]["nadd2"] == 0 and r["records"][0]["g3"] == -1
    r = RP.ref_run("exhaust")
    assert [x["result"] for x in r["records"]] == [0, 2] and r["n_candidates"] == 0
    assert all(x["no_more"] and x["discarded"] for x in r["records"])
    r = RP.ref_run("ngood_lt10")
    assert 0 <= r["records"][0]["g1"] < 10 and not r["records"][0]["discarded"]
    r = RP.ref_run("no_stream")     # the second candidate has no stream (P30 / P31)
    assert r["status"] == R.DRAW_EXHAUSTED and r["records"][1]["calls"] == 0


def test_parameter_table_matches_the_library_formula():
    """the table's generator (orbpnp_ransac_parameters, host only) against the
    restatement for every N"""
    from _pkg import load_pkg
    orbpl = load_pkg()
    mn, mx = orbpl.reloc_ransac_table()
    assert len(mn) == 2049
    for n in range(2049):
        want = _pnp_ref.ransac_parameters(n, *R.RELOC_PARAMS)
        assert (int(mn[n]), int(mx[n])) == want[:2], n


def test_package_record_layout_and_status_codes_match_the_restatement():
    from _pkg import load_pkg
    orbpl = load_pkg()
    assert tuple(orbpl.RL_REC) == tuple(R.REC)
    assert (orbpl.RL_OK, orbpl.RL_NO_CANDIDATES, orbpl.RL_FAILED, orbpl.RL_DRAW_EXHAUSTED) == \
        (R.OK, R.NO_CANDIDATES, R.FAILED, R.DRAW_EXHAUSTED)
