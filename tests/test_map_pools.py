"""The package's shared map packer (orbpl.MapPools, the layout csrc/map_pool.h
states) on the CPU: the host arrays of SinDeviceProblems and KfcDeviceProblems
for two problems of different shape, with device=None (no device buffer, no
library call). Problem table, K / M / pitch, every keyframe's row and every
problem's point range equal to the inputs, everything else the padding value."""
import numpy as np

import _cull_problems as cp
import _fuse_problems as fp
from _pkg import load_pkg

orbpl = load_pkg()
PAD = dict(uright=-1, mp=-1, ordered=-1, bad=1)
KF_KEY = dict(id="id", T="Tcw", kps_un="kps_un", uright="uright", kdesc="desc", mp="mp")
PER_FEATURE = ("kps_un", "uright", "kdesc", "mp")


def check_pools(pools, probs):
    """every map column of pools.host: the inputs where a map fills it, padding elsewhere"""
    maps = [p["map"] for p in probs]
    nkf, npt = [len(m["kfs"]) for m in maps], [len(m["bad"]) for m in maps]
    widest = [max(len(k["uright"]) for k in m["kfs"]) for m in maps]
    assert nkf[0] != nkf[1] and widest[0] != widest[1]            # the two shapes differ
    assert pools.prob.tolist() == [[0, nkf[0], 0, npt[0], probs[0]["cur"]],
                                   [nkf[0], nkf[1], npt[0], npt[1], probs[1]["cur"]]]
    assert (pools.K, pools.M, pools.pitch) == (sum(nkf), sum(npt), max(widest))
    h = pools.host
    seen = {c: np.zeros(h[c].shape, bool) for c in h}            # what a map filled
    g = q = 0
    for m in maps:
        for k in m["kfs"]:
            n = len(k["uright"])
            assert h["n"][g] == n
            seen["n"][g] = True
            for c, key in KF_KEY.items():
                if c not in h:
                    continue
                if c in PER_FEATURE:
                    want = np.asarray(k[key]).reshape((n,) + h[c].shape[2:])
                    assert h[c][g, :n].tobytes() == want.astype(h[c].dtype).tobytes(), c
                    seen[c][g, :n] = True
                else:
                    assert np.array_equal(h[c][g], np.asarray(k[key]).reshape(h[c].shape[1:])), c
                    seen[c][g] = True
            g += 1
        M = len(m["bad"])
        for c in pools._PT_COLS:
            assert np.array_equal(h[c][q:q + M], np.asarray(m[c]).reshape((M,) + h[c].shape[1:])), c
            seen[c][q:q + M] = True
        q += M
    for c in KF_KEY.keys() | set(pools._PT_COLS) | {"n"}:
        if c in h:
            rest = h[c][~seen[c]]
            assert rest.tobytes() == np.full(rest.shape, PAD.get(c, 0), h[c].dtype).tobytes(), c
    return seen


def test_search_in_neighbors_pools_on_the_host():
    probs = [dict(map=fp.problem(n)["map"], cur=fp.problem(n)["cur"]) for n in ("n65", "hand_conflict")]
    pools = orbpl.SinDeviceProblems(None, probs, device=None)
    assert not hasattr(pools, "bufs") and not hasattr(pools, "batch")
    check_pools(pools, probs)
    assert set(pools.host) == set(pools._KF_COLS + pools._PT_COLS)
    assert pools.list_pitch == max(pools.pitch, max(len(p["map"]["bad"]) for p in probs))
    g = 0
    for p in probs:                                              # ordered: the list, then -1
        for k in p["map"]["kfs"]:
            o = list(k["ordered"])
            assert pools.host["ordered"][g].tolist() == o + [-1] * (64 - len(o))
            g += 1


def test_keyframe_culling_pools_on_the_host():
    probs = [cp.problem("tree_chain"), cp.problem("nkf1")]
    pools = orbpl.KfcDeviceProblems(None, probs, device=None)
    assert not hasattr(pools, "bufs")
    seen = check_pools(pools, probs)
    h = pools.host
    assert "kdesc" not in h and "xyz" not in h and "n_found" not in h     # columns the call does not read
    assert h["depth"].shape == h["uright"].shape
    assert np.all(h["depth"][~seen["uright"]] == -1)
    g = 0
    for p in probs:
        K = len(p["map"]["kfs"])
        for j in range(K):
            n = len(p["map"]["kfs"][j]["uright"])
            assert np.array_equal(h["depth"][g, :n], np.asarray(p["depth"][j], np.float32))
            assert h["conn_w"][g, :K].tolist() == np.asarray(p["conn_w"]).reshape(K, K)[j].tolist()
            assert not h["conn_w"][g, K:].any()
            assert h["parent"][g] == p["parent"][j] and h["kf_bad"][g] == p["kf_bad"][j]
            g += 1
