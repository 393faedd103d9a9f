"""orblm_search_in_neighbors and orbm_fuse refuse a bad argument before they
touch the device: every case comes back as ORBPL_ERR_ARG with the given
orbpl_last_error() text, on a machine with or without a GPU (the pattern of
test_host_refusals.py)."""
import copy
import ctypes as C

import numpy as np
import pytest

import _fuse_problems as fp
from _pkg import load_pkg

orbpl = load_pkg()
CAM = orbpl.Camera(fp.CAM["fx"], fp.CAM["fy"], fp.CAM["cx"], fp.CAM["cy"], 0.0, 0.0, 0.0, 0.0, 0.0,
                   fp.CAM["bf"], 3.0, fp.W, fp.H)


def _map():
    p = fp.problem("hand_conflict")
    m = copy.deepcopy(p["map"])
    return m, p["cur"]


def _sin(m, cur, nlevels=fp.NLEVELS, null=None):
    """the raw call on a map dict; null: a field of the C structure to clear"""
    keep = []
    P = (orbpl.LmSinProblem * 1)()
    P[0].map, _, _ = orbpl._sin_map_struct(m, keep)
    P[0].cur = cur
    if null:
        setattr(P[0].map, null, None)
    scale, sigma2 = fp.SCALE.copy(), fp.SIGMA2.copy()
    rc = orbpl.lib().orblm_search_in_neighbors(C.byref(CAM), scale.ctypes.data, sigma2.ctypes.data,
                                               nlevels, P, 1)
    return rc, orbpl.lib().orbpl_last_error().decode()


def _edit(fn):
    m, cur = _map()
    fn(m)
    return m, cur


def _twice(m):
    m["kfs"][2]["mp"][1] = 0              # point 0 already sits in keyframe 2's slot 0


def _dup_id(m):
    m["kfs"][1]["id"] = m["kfs"][0]["id"]


def _octave(m):
    m["kfs"][1]["kps_un"]["octave"][0] = fp.NLEVELS


def _slot(m):
    m["kfs"][0]["mp"][0] = 3              # M = 3


def _ref(m):
    m["ref_kf"][0] = 3                    # keyframe 3 does not observe point 0


def _ordered(m):
    m["kfs"][0]["ordered"] = [4]


def _self(m):
    m["kfs"][0]["ordered"] = [0]


CASES = [
    (_twice, "map point twice in one keyframe"),
    (_dup_id, "two keyframes of a map with one id"),
    (_octave, "keypoint octave outside [0, nlevels)"),
    (_slot, "slot index outside [-1, M)"),
    (_ref, "good map point whose ref_kf does not observe it"),
    (_ordered, "ordered entry outside the table or naming its own keyframe"),
    (_self, "ordered entry outside the table or naming its own keyframe"),
]


@pytest.mark.parametrize("edit,text", CASES, ids=[c[0].__name__ for c in CASES])
def test_inconsistent_maps_are_refused(edit, text):
    rc, msg = _sin(*_edit(edit))
    assert rc == orbpl.ORBPL_ERR_ARG and msg == text


@pytest.mark.parametrize("field", ["kf", "xyz", "normal", "min_dist", "max_dist", "desc", "ref_kf", "bad",
                                   "n_visible", "n_found", "replaced_by", "n_obs", "obs", "desc_src"])
def test_null_arrays_are_refused(field):
    rc, msg = _sin(*_map(), null=field)
    assert rc == orbpl.ORBPL_ERR_ARG
    assert msg == ("NULL keyframe table" if field == "kf" else "NULL map point arrays")


def test_counts_are_refused():
    m, cur = _map()
    assert _sin(m, 4) == (orbpl.ORBPL_ERR_ARG, "current keyframe outside the table")
    assert _sin(m, cur, nlevels=17) == (orbpl.ORBPL_ERR_ARG, "nlevels outside [1, 16]")
    big = dict(m, kfs=[m["kfs"][i % 4] for i in range(65)])
    assert _sin(big, 0) == (orbpl.ORBPL_ERR_ARG, "map with no keyframe or more than 64")
    assert _sin(dict(m, kfs=[]), 0) == (orbpl.ORBPL_ERR_ARG, "map with no keyframe or more than 64")
    k = dict(m["kfs"][0])
    n = 2049
    k.update(kps_un=np.zeros(n, fp.KP_DTYPE), uright=np.zeros(n, np.float32),
             desc=np.zeros((n, 32), np.uint8), mp=np.full(n, -1, np.int32))
    assert _sin(dict(m, kfs=[k] + m["kfs"][1:]), 0) == (orbpl.ORBPL_ERR_ARG,
                                                        "keyframe with more than 2048 features")


def test_a_shared_array_is_refused():
    m, cur = _map()
    keep = []
    P = (orbpl.LmSinProblem * 2)()
    P[0].map, _, _ = orbpl._sin_map_struct(m, keep)
    P[1].map = P[0].map                      # both problems would write the same arrays
    P[0].cur = P[1].cur = cur
    rc = orbpl.lib().orblm_search_in_neighbors(C.byref(CAM), fp.SCALE.ctypes.data, fp.SIGMA2.ctypes.data,
                                               fp.NLEVELS, P, 2)
    assert rc == orbpl.ORBPL_ERR_ARG
    assert orbpl.lib().orbpl_last_error().decode() == "a keyframe or point array belongs to two problems"


def test_fuse_refusals():
    m, cur = _map()
    keep = []
    s, _, _ = orbpl._sin_map_struct(m, keep)
    out = np.zeros(4, np.int32)
    nf = C.c_int(0)

    def call(kf, lst, smap=s):
        a = np.array(lst, np.int32)
        rc = orbpl.lib().orbm_fuse(C.byref(CAM), fp.SCALE.ctypes.data, fp.SIGMA2.ctypes.data, fp.NLEVELS,
                                   C.byref(smap), kf, a.ctypes.data, len(a), 3.0, C.byref(nf),
                                   out.ctypes.data, out.ctypes.data, out.ctypes.data)
        return rc, orbpl.lib().orbpl_last_error().decode()

    assert call(4, [0]) == (orbpl.ORBPL_ERR_ARG, "keyframe outside the table")
    assert call(0, [3]) == (orbpl.ORBPL_ERR_ARG, "list entry outside [-1, M)")
    assert call(0, [-2]) == (orbpl.ORBPL_ERR_ARG, "list entry outside [-1, M)")
    bad, _ = _edit(_twice)
    s2, _, _ = orbpl._sin_map_struct(bad, keep)
    assert call(0, [0], s2) == (orbpl.ORBPL_ERR_ARG, "map point twice in one keyframe")
