"""The sequential restatement of KeyFrameCulling and MapPointCulling /
MapLineCulling (tests/_cull_ref.py) on the hand-built maps against values
written out by hand, its branch coverage over all problems, the refusals of
the host entries (before any device call: they hold on a machine with or
without a GPU) and the stand-alone sanitizer check of the host code."""
import copy
import ctypes as C
import os
import shutil
import subprocess
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

import _cull_problems as cp
import _cull_ref as ref
from _pkg import load_pkg

A = {a: i for i, a in enumerate(ref.ACTIONS)}
RC = {r: i for i, r in enumerate(ref.REASONS)}


def _ordered(res, k):
    return [int(x) for x in res["ordered"][k] if x >= 0]


# name -> (list, action, nMPs, nRedundant, culled set, parents after, bad points after)
HAND = {
    "nkf1": ([], [], [], [], [], [-1], []),
    "nkf2": ([1], ["kept"], [3], [0], [], [-1, 0], []),
    "t10_9": ([3], ["kept"], [10], [9], [], [-1, 0, 0, 0, 0], []),
    "t10_10": ([3], ["culled"], [10], [10], [3], [-1, 0, 0, 0, 0], []),
    "t20_18": ([3], ["kept"], [20], [18], [], [-1, 0, 0, 0, 0], []),
    "t20_19": ([3], ["culled"], [20], [19], [3], [-1, 0, 0, 0, 0], [19]),
    "nmps0": ([3], ["kept"], [0], [0], [], [-1, 0, 0, 0, 0], []),
    "gates": ([3], ["kept"], [6], [3], [], [-1, 0, 0, 0, 0], []),
    "first": ([3], ["first"], [0], [0], [], [3, 3, 3, -1, 3], []),
    "not_erase": ([3], ["deferred"], [10], [10], [], [-1, 0, 0, 0, 0], []),
    "order_ab": ([2, 3], ["culled", "kept"], [10, 10], [10, 0], [2], [-1, 0, 0, 0, 0], []),
    "order_ba": ([3, 2], ["culled", "kept"], [10, 10], [10, 0], [3], [-1, 0, 0, 0, 0], []),
    "goes_bad": ([3], ["culled"], [30], [28], [3], [1, -1, 1, 1, 1], [28, 29]),
    "tree_chain": ([1], ["culled"], [10], [10], [1], [-1, 0, 0, 2, 0, 0], []),
    "tree_tie": ([1], ["culled"], [10], [10], [1], [-1, 0, 3, 0, 0], []),
    "asym": ([3], ["culled"], [10], [10], [3], [-1, 0, 0, 0, 0], []),
    "bad_entry": ([2, 4, 0, 1], ["culled", "culled", "first", "kept"], [10, 5, 0, 10], [10, 5, 0, 0],
                  [2, 3, 4], [-1, 0, 0, 0, -1, 0], [10]),
}


def test_every_hand_map_is_listed():
    assert set(HAND) == set(cp.HAND)
    for name in cp.HAND:
        kfs = cp.problem(name)["map"]["kfs"]
        assert len(kfs) <= 6 and all(len(k["mp"]) <= 40 for k in kfs), name


@pytest.mark.parametrize("name", cp.HAND)
def test_hand_maps_against_hand_values(name):
    res, _ = cp.ref_run(name)
    lst, action, nmps, nred, culled, parent, bad = HAND[name]
    assert res["list"].tolist() == lst
    assert res["action"].tolist() == [A[a] for a in action]
    assert res["n_mps"].tolist() == nmps and res["n_redundant"].tolist() == nred
    assert np.flatnonzero(res["kf_bad"]).tolist() == culled
    assert res["parent"].tolist() == parent
    assert np.flatnonzero(res["bad"]).tolist() == bad
    before = int(np.sum(cp.problem(name)["map"]["bad"]))
    assert res["n_points_bad"] == len(bad) - before


def test_hand_details():
    """what a cull leaves behind, beyond the sets above"""
    res, _ = cp.ref_run("not_erase")
    assert res["to_be_erased"].tolist() == [0, 0, 0, 1, 0]
    assert np.array_equal(res["conn_w"], cp.problem("not_erase")["conn_w"]) and _ordered(res, 4) == [3]
    # t20_19: point 19 sat in K and A: A's slot is cleared, K's own slot keeps naming it
    res, _ = cp.ref_run("t20_19")
    assert res["mp"][0][19] == -1 and res["mp"][3][19] == 19 and res["n_obs"][19] == 2
    assert res["n_obs"][:19].tolist() == [6] * 19 and not res["conn_w"][3].any() and not res["conn_w"][:, 3].any()
    assert _ordered(res, 3) == [] and _ordered(res, 4) == [] and 3 not in _ordered(res, 0)
    assert np.all(res["obs"][:, 3] == -1) and res["Tcp"][3][15] == 1 and not res["Tcp"][[0, 1, 2, 4]].any()
    # goes_bad: the reference keyframe goes to B (index 1, id 0), not to A (index 0, id 8)
    res, _ = cp.ref_run("goes_bad")
    assert res["ref_kf"].tolist() == [1] * 28 + [0, -1]
    assert res["n_obs"].tolist() == [6] * 28 + [2, 0]
    assert res["mp"][0][28] == -1 and res["mp"][3].tolist() == list(range(30))
    # order dependence: the survivor's points kept three observers
    for name, gone, stays in (("order_ab", 2, 3), ("order_ba", 3, 2)):
        res, _ = cp.ref_run(name)
        assert res["kf_bad"][gone] == 1 and res["kf_bad"][stays] == 0 and res["n_obs"].tolist() == [6] * 10
    # tree_chain: C2 (index 3) was not in K's row: its row and list stay; C3 never listed K
    res, _ = cp.ref_run("tree_chain")
    assert res["conn_w"][3].tolist() == [0, 10, 0, 0, 0, 0] and _ordered(res, 3) == [1, 2]
    assert _ordered(res, 0) == [3, 2] and _ordered(res, 2) == [3, 0] and _ordered(res, 5) == []
    # tree_tie: equal weights come out id descending
    res, _ = cp.ref_run("tree_tie")
    assert _ordered(res, 2) == [3, 0] and _ordered(res, 3) == [0]
    # asym: A keeps naming K, B's >= 15 subset becomes its whole row, C loses its only connection
    res, _ = cp.ref_run("asym")
    assert _ordered(res, 0) == [3] and _ordered(res, 1) == [0, 2] and _ordered(res, 2) == []
    assert res["conn_w"][1].tolist() == [30, 0, 5, 0, 0]
    # bad_entry: nothing moves but Kd's parent and Kb's mTcp
    p = cp.problem("bad_entry")
    res, _ = cp.ref_run("bad_entry")
    assert all(np.array_equal(a["mp"], b) for a, b in zip(p["map"]["kfs"], res["mp"]))
    assert np.array_equal(res["conn_w"], p["conn_w"]) and res["n_obs"].tolist() == [6] * 10 + [0]
    assert res["Tcp"][2].any() and not res["Tcp"][4].any()


def test_tcp_is_the_relative_pose():
    p = cp.problem("t10_10")
    res, _ = cp.ref_run("t10_10")
    T = [np.asarray(k["Tcw"], np.float64).reshape(4, 4) for k in p["map"]["kfs"]]
    want = T[3] @ np.linalg.inv(T[0])
    assert np.abs(res["Tcp"][3].reshape(4, 4) - want).max() < 1e-6


def test_every_branch_is_taken():
    stats = Counter()
    for name in cp.NAMES:
        stats += cp.ref_run(name)[1]
    assert not [b for b in ref.BRANCHES if stats[b] == 0]
    assert not set(stats) - set(ref.BRANCHES)
    actions = Counter(a for name in cp.NAMES for a in cp.ref_run(name)[0]["action"].tolist())
    assert all(actions[i] > 0 for i in range(len(ref.ACTIONS)))
    stats = Counter()
    for name in cp.RC_NAMES:
        stats += cp.recent_ref_run(name)[1]
    assert not [b for b in ref.RECENT_BRANCHES if stats[b] == 0]
    assert not set(stats) - set(ref.RECENT_BRANCHES)


def test_scenes_cull_some_and_keep_some():
    for name in ("k64", "s8", "s12"):
        act = cp.ref_run(name)[0]["action"].tolist()
        assert A["culled"] in act and A["kept"] in act, name
    res, _ = cp.ref_run("k64")
    assert len(res["list"]) == 63 and res["action"].tolist().count(A["culled"]) > 3
    kfs = cp.problem("n2048")["map"]["kfs"]
    assert len(kfs) == 5 and all(len(k["mp"]) == 2048 for k in kfs)
    assert len(cp.recent_problem("rc_2048")["recent"]) == 2048


def test_recent_hand_lists_against_hand_values():
    res, _ = cp.recent_ref_run("rc_hand")
    # point 0 bad; 1: 1/5 < 0.25; 2: 1/4, age 0; 3: 0/0, age 3; 4: 2/0, age 2, 3 observations;
    # 5: age 2, 4 observations; 6: age 3; 7: age 2, 8 observations
    want = ["was_bad", "found_ratio", "stays", "aged_out", "few_observations", "stays", "aged_out", "stays"]
    assert res["reason"].tolist() == [RC[r] for r in want]
    assert res["recent"].tolist() == [2, 5, 7]
    assert np.flatnonzero(res["bad"]).tolist() == [0, 1, 4]
    assert res["n_obs"].tolist() == [8, 8, 8, 8, 3, 4, 8, 8]
    assert [int(r[1]) for r in res["mp"][:4]] == [-1] * 4 and res["mp"][0][4] == -1 and res["mp"][3][4] == -1
    assert res["mp"][0][0] == 0                        # bad at entry: its slots stay
    # lines, list [4, 3, 2, 1, 0]: 4 age 1; 3 first_kf -1, 4 observations; 2 first_kf -1, 3 observations;
    # 1 0/3; 0 bad
    want = ["stays", "aged_out", "few_observations", "found_ratio", "was_bad"]
    assert res["line_reason"].tolist() == [RC[r] for r in want]
    assert res["recent_lines"].tolist() == [4] and res["line_bad"].tolist() == [1, 1, 1, 0, 0, 1]
    assert [r.tolist() for r in res["ml"]] == [[0, -1, -1], [-1, -1, 3], [4, 5], [5, -1], []]
    res, _ = cp.recent_ref_run("rc_empty")
    assert len(res["recent"]) == len(res["reason"]) == len(res["recent_lines"]) == 0
    assert not res["bad"].any()


# ---------------------------------------------------------------------------
# the host entries' refusals
# ---------------------------------------------------------------------------
orbpl = load_pkg()
CAM = orbpl.Camera(cp.CAM["fx"], cp.CAM["fy"], cp.CAM["cx"], cp.CAM["cy"], 0.0, 0.0, 0.0, 0.0, 0.0,
                   cp.CAM["bf"], float(cp.TH_DEPTH), 640, 480)


needs_lib = pytest.mark.skipif(not orbpl.LIB_PATH.exists(), reason="liborbpl.so is not built")


def _culler():
    return orbpl.MapCuller(CAM, cp.SCALE, cp.SIGMA2)


def _refused(call, text):
    with pytest.raises(orbpl.OrbplError) as e:
        call()
    assert text in str(e.value), str(e.value)


def _kfc(edit):
    p = copy.deepcopy(cp.problem("tree_chain"))
    edit(p)
    return lambda: _culler().keyframes([p])


def _set(key, idx, val):
    def edit(p):
        p[key][idx] = val
    return edit


def _slot_twice(p):
    p["map"]["kfs"][0]["mp"][1] = 0


KFC_CASES = [
    (_slot_twice, "map point twice in one keyframe"),
    (lambda p: p.update(cur=6), "current keyframe outside the table"),
    (lambda p: p["conn_w"].__setitem__((2, 3), -1), "negative covisibility weight"),
    (lambda p: p["conn_w"].__setitem__((2, 2), 1), "non-zero diagonal of conn_w"),
    (_set("ordered", 2, [6]), "ordered entry outside the table or naming its own keyframe"),
    (_set("ordered", 2, [2]), "ordered entry outside the table or naming its own keyframe"),
    (_set("ordered", 2, [1, 0, 1]), "ordered list names a keyframe twice"),
    (_set("parent", 2, 6), "parent outside the table or naming its own keyframe"),
    (_set("parent", 2, 2), "parent outside the table or naming its own keyframe"),
    (_set("parent", 2, -1), "good keyframe with id != 0 and no parent"),
]


@needs_lib
@pytest.mark.parametrize("edit,text", KFC_CASES, ids=[str(i) for i in range(len(KFC_CASES))])
def test_keyframe_culling_refusals(edit, text):
    _refused(_kfc(edit), text)


@needs_lib
def test_keyframe_culling_null_and_shared_arrays():
    keep = []
    p = cp.problem("tree_chain")
    P = (orbpl.LmKfcProblem * 2)()
    P[0].map, kfs, _ = orbpl._sin_map_struct(p["map"], keep)
    P[0].cur = p["cur"]
    g = orbpl._kfc_graph_arrays(p, kfs)
    dptr = (C.c_void_p * len(kfs))(*[d.ctypes.data for d in g["depth"]])
    P[0].depth = C.cast(dptr, C.c_void_p)
    names = ("conn_w", "ordered", "parent", "not_erase", "kf_bad", "to_be_erased", "Tcp")
    for name in names:
        setattr(P[0], name, g[name].ctypes.data)
    L = orbpl.lib()
    for name in names + ("depth",):
        saved = getattr(P[0], name)
        setattr(P[0], name, None)
        assert L.orblm_keyframe_culling(C.byref(CAM), 8, P, 1) == orbpl.ORBPL_ERR_ARG
        assert L.orbpl_last_error().decode() == "NULL graph arrays"
        setattr(P[0], name, saved)
    C.memmove(C.byref(P[1]), C.byref(P[0]), C.sizeof(orbpl.LmKfcProblem))
    assert L.orblm_keyframe_culling(C.byref(CAM), 8, P, 2) == orbpl.ORBPL_ERR_ARG
    assert L.orbpl_last_error().decode() == "a keyframe, point or graph array belongs to two problems"
    assert L.orblm_keyframe_culling(C.byref(CAM), 17, P, 1) == orbpl.ORBPL_ERR_ARG
    assert L.orbpl_last_error().decode() == "nlevels outside [1, 16]"


def _rc(edit):
    p = copy.deepcopy(cp.recent_problem("rc_hand"))
    edit(p)
    return lambda: _culler().recent([p])


RC_CASES = [
    (lambda p: p.update(recent=np.int32([0, 1, 0])), "recent entry repeats"),
    (lambda p: p.update(recent=np.int32([8])), "recent entry outside [0, M)"),
    (lambda p: p.update(recent_lines=np.int32([2, 2])), "recent line entry repeats"),
    (lambda p: p.update(recent_lines=np.int32([6])), "recent line entry outside [0, L)"),
    (lambda p: p["lines"]["ml"].__setitem__(0, np.int32([6])), "line slot outside [-1, L)"),
    (lambda p: p["lines"]["ml"].__setitem__(0, np.full(257, -1, np.int32)), "keyframe with more than 256 lines"),
    (lambda p: p["map"]["kfs"][0]["mp"].__setitem__(1, 0), "map point twice in one keyframe"),
]


@needs_lib
@pytest.mark.parametrize("edit,text", RC_CASES, ids=[str(i) for i in range(len(RC_CASES))])
def test_cull_recent_refusals(edit, text):
    _refused(_rc(edit), text)


def test_cull_check_builds_and_runs():
    """the validation, the flattening into the staged pools and the no-device
    failure path of both calls, as a program of its own under the host sanitizers"""
    if shutil.which("make") is None or shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) is None:
        pytest.skip("no make or no hipcc (the Makefile's HIPCC)")
    csrc = Path(orbpl.__file__).resolve().parent / "csrc"
    subprocess.run(["make", "-C", str(csrc), "cull_check"], check=True, capture_output=True)
    out = subprocess.run([str(csrc.parent / "keyframe_culling_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "keyframe_culling_check: ok" in out.stdout or "a device is present" in out.stdout
