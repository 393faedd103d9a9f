"""GPU: the batched ORBmatcher::SearchBySim3 (orbm_search_by_sim3,
orbm_search_by_sim3_batch_device; csrc/search_by_sim3.hip) against the
sequential restatement in tests/_sim3_ref.py. The reason codes, vnMatch1 /
vnMatch2, the updated matched12 and nFound are equal, through the host entry
and through the device entry. The branch-by-branch pairs also state what the
reference does with them."""
import numpy as np
import pytest

import _sim3_ref as ref
from _sim3_problems import SCALE, TH, hand_cases, kernel_camera, ref_camera, scene

pytestmark = pytest.mark.gpu

CASES = hand_cases()
KEYS = ("n_found", "matched12", "vn_match1", "vn_match2", "reason1", "reason2")
_REF = {}


def _want(name, pair):
    if name not in _REF:
        _REF[name] = ref.search_by_sim3(ref_camera(), pair["kf1"], pair["kf2"], pair["matched12"],
                                        pair["s12"], pair["R12"], pair["t12"], TH)
    return _REF[name]


def _same(got, want, what):
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])


def _both_entries(orbpl, pairs):
    cam = kernel_camera(orbpl)
    host = orbpl.search_by_sim3_batch(cam, SCALE, pairs, TH)
    dev = orbpl.Sim3MatchDeviceProblems(pairs)
    dev.run(cam, SCALE, TH)
    return host, dev.download()


@pytest.mark.parametrize("name", sorted(CASES))
def test_branch(orbpl, name):
    pair, d, reason, vn, found = CASES[name]
    want = _want(name, pair)
    assert want["reason%d" % d][0] == reason and want["vn_match%d" % d][0] == vn
    assert want["n_found"] == found
    if found:
        assert want["matched12"][0] == 0     # feature 0 of both keyframes
    else:
        assert np.array_equal(want["matched12"], pair["matched12"])
    host, dev = _both_entries(orbpl, [pair])
    _same(host[0], want, name + " host")
    _same(dev[0], want, name + " device")


def test_matcher_class_updates_in_place(orbpl):
    pair, d, reason, vn, found = CASES["mutual_dir1"]
    m = pair["matched12"].copy()
    n = orbpl.ORBmatcher().SearchBySim3(kernel_camera(orbpl), SCALE, pair["kf1"], pair["kf2"], m,
                                        pair["s12"], pair["R12"], pair["t12"], TH)
    assert n == 1 and list(m) == [0]


@pytest.mark.parametrize("n,seed", [(500, 1), (2048, 2)])
def test_seeded_scene(orbpl, n, seed):
    s = scene(n, seed)
    want = _want(s["name"], s)
    host, dev = _both_entries(orbpl, [s])
    _same(host[0], want, s["name"] + " host")
    _same(dev[0], want, s["name"] + " device")
    print(f"{s['name']}: nFound {want['n_found']}, reasons 1->2 "
          f"{np.bincount(want['reason1'], minlength=8)}, 2->1 "
          f"{np.bincount(want['reason2'], minlength=8)}")
    assert want["n_found"] > 0.1 * n


def _mixed(count):
    sizes = [(37, 41), (1, 1), (300, 120), (64, 65), (257, 256), (8, 200), (0, 5), (5, 0)]
    hand = [CASES[k][0] for k in sorted(CASES)]
    out = []
    for k in range(count):
        if k % 3 == 2:
            out.append((f"hand{k}", hand[(7 * k) % len(hand)]))
        else:
            a, b = sizes[k % len(sizes)]
            s = scene(a, 100 + k % 16, b)
            out.append((s["name"], s))
    return out


@pytest.mark.parametrize("count", [1, 3, 40])
def test_batches_of_mixed_sizes_host_and_device(orbpl, count):
    named = _mixed(count)
    host, dev = _both_entries(orbpl, [p for _, p in named])
    for (name, p), h, d in zip(named, host, dev):
        want = _want(name if not name.startswith("hand") else name + "_batch", p)
        _same(h, want, name + " host")
        _same(d, want, name + " device")


def test_over_the_cap_is_an_argument_error(orbpl):
    s = scene(2048, 2)
    k = s["kf1"]
    grown = {key: (np.concatenate([v, v[:1]]) if key != "Tcw" else v) for key, v in k.items()}
    cam = kernel_camera(orbpl)
    with pytest.raises(orbpl.OrbplError, match="failed with -1"):
        orbpl.search_by_sim3_batch(cam, SCALE, [dict(s, kf1=grown,
                                                     matched12=np.append(s["matched12"], -1))], TH)
    with pytest.raises(orbpl.OrbplError, match="failed with -1"):
        orbpl.search_by_sim3_batch(cam, SCALE, [dict(s, kf2=grown)], TH)
    with pytest.raises(orbpl.OrbplError, match="failed with -1"):
        orbpl.search_by_sim3_batch(cam, SCALE, [dict(s, matched12=np.full(2048, -3, np.int32))], TH)
