"""The restatement of SearchInNeighbors / Fuse (tests/_fuse_ref.py) on its own,
without a GPU: every branch is reached over the problem set, no decision of a
problem hangs on the last bits, the map stays consistent, and against the scene
the call removes duplicates and creates none."""
import numpy as np
import pytest

import _fuse_problems as fp

FRAGILE = 1e-6   # relative margin below which a decision is taken to hang on rounding

# branches the problem set must reach (stats keys of _fuse_ref)
REQUIRED = ("null", "bad", "in_kf", "behind", "out_of_image", "distance", "view", "empty_window",
            "gate_level", "gate_chi_stereo", "gate_chi_mono", "no_match_over_th_low",
            "no_match_none_passed", "added", "replaced", "replaces", "replace_equal_counts",
            "replace_handover", "replace_conflict", "tie_first_wins", "duplicate_target",
            "second_neighbour_skipped", "candidate_dedup", "connections_below_threshold",
            "connections_empty")
# branches no consistent map reaches, with the reason
UNREACHED = (
    ("bad_slot", "Replace empties every slot of the point it marks bad and the problems start from "
                 "maps without a bad point in a slot, so Fuse never finds a bad point under a keypoint "
                 "(test_gpu_fuse.py runs Fuse alone on a map that holds one at entry)"),
    ("candidate_bad", "for the same reason no target slot holds a bad point when the backward list "
                      "is collected"),
)


def test_every_branch_is_reached():
    total = {}
    for name in fp.NAMES:
        for k, v in fp.ref_run(name)[2].items():
            total[k] = total.get(k, 0) + v
    missing = [k for k in REQUIRED if not total.get(k)]
    assert not missing, missing
    assert not [k for k, _ in UNREACHED if total.get(k)]


def test_problem_shapes():
    sizes = {n: [len(k["uright"]) for k in fp.problem(n)["map"]["kfs"]] for n in fp.NAMES}
    assert {sizes[n][0] for n in ("n0", "n1", "n65", "n300", "n2048")} == {0, 1, 65, 300, 2048}
    assert len(sizes["kf64"]) == 64 and len(sizes["n2048"]) == 12
    res = fp.ref_run("kf64")[1]
    assert len(res["targets"]) > len(set(res["targets"].tolist()))      # duplicates kept
    firsts = {n: len(fp.problem(n)["map"]["kfs"][fp.problem(n)["cur"]]["ordered"]) for n in fp.NAMES}
    assert {0, 1, 3, 10} <= set(firsts.values())
    p = fp.problem("cur_empty")
    assert (p["map"]["kfs"][p["cur"]]["mp"] < 0).all()
    p = fp.problem("target_empty")
    t = fp.ref_run("target_empty")[1]["targets"]
    assert any((p["map"]["kfs"][k]["mp"] < 0).all() for k in t)
    ur = [k["uright"] for k in fp.problem("mono_mixed")["map"]["kfs"]]
    assert any((u < 0).all() for u in ur) and any((u < 0).any() and (u >= 0).any() for u in ur)


@pytest.mark.parametrize("name", fp.NAMES)
def test_no_decision_hangs_on_the_last_bits(name):
    margins = fp.ref_run(name)[3]
    assert not margins or min(margins) >= FRAGILE, min(margins)


@pytest.mark.parametrize("name", fp.NAMES)
def test_map_invariants(name):
    p, (_, r, _, _) = fp.problem(name), fp.ref_run(name)
    m = p["map"]
    M, K = len(r["bad"]), len(m["kfs"])
    # slots and observation tables agree in both directions
    for k in range(K):
        for i, q in enumerate(r["mp"][k]):
            if q >= 0:
                assert r["obs"][q, k] == i and not r["bad"][q]      # no bad point sits in a slot
    for q in range(M):
        for k in range(64):
            if r["obs"][q, k] >= 0:
                assert k < K and r["mp"][k][r["obs"][q, k]] == q
    # n_obs is the 2 / 1 sum over observers
    for q in range(M):
        want = sum(2 if m["kfs"][k]["uright"][r["obs"][q, k]] >= 0 else 1
                   for k in range(K) if r["obs"][q, k] >= 0)
        assert r["n_obs"][q] == want
    for q in range(M):
        if r["bad"][q]:
            e, hops = q, 0
            while r["replaced_by"][e] >= 0:
                e, hops = r["replaced_by"][e], hops + 1
                assert hops <= M
            assert not r["bad"][e] and hops > 0                     # the chain ends at a good point
        else:
            assert r["obs"][q, r["ref_kf"][q]] >= 0                 # ref_kf observes its point
    # every point was good at entry: what the survivors hold is what all held
    good = r["bad"] == 0
    assert r["n_found"][good].sum() == m["n_found"].sum()
    assert r["n_visible"][good].sum() == m["n_visible"].sum()


def _owners(p, slots, bad, kfs):
    own = {}
    for k in kfs:
        for q in slots[k]:
            if q >= 0 and not bad[q] and p["corner"][q] >= 0:
                own.setdefault(int(p["corner"][q]), set()).add(int(q))
    return own


def duplicate_share(name):
    """(share of corners owned by more than one good point over the current
    keyframe and its targets before, after; points per corner before, after)"""
    p, r = fp.problem(name), fp.ref_run(name)[1]
    kfs = sorted(set(r["targets"].tolist()) | {p["cur"]})
    before = _owners(p, [k["mp"] for k in p["map"]["kfs"]], p["map"]["bad"], kfs)
    after = _owners(p, r["mp"], r["bad"], kfs)
    share = lambda o: sum(len(v) > 1 for v in o.values()) / max(1, len(o))
    return share(before), share(after), before, after


def test_duplicates_fall_against_the_scene():
    """Noise-free problem n300_clean, 8 keyframes of 300 keypoints: 48.7 % of the
    corners seen in the target neighbourhood are owned by more than one good map
    point before the call, 18.7 % after it."""
    s0, s1, before, after = duplicate_share("n300_clean")
    print(f"corners with more than one good point: {100 * s0:.1f} % before, {100 * s1:.1f} % after")
    assert sum(map(len, after.values())) < sum(map(len, before.values()))
    assert s1 < s0
    for c, pts in after.items():
        assert len(pts) <= len(before.get(c, ())), c            # none created
        assert pts <= before[c]
