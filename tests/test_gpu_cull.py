"""orblm_keyframe_culling, its device-pool form and orblm_cull_recent on the GPU
against the sequential restatement (tests/_cull_ref.py): every integer output
equal (slots, obs, n_obs, bad, ref_kf, conn_w, ordered, parent, kf_bad,
to_be_erased, the result struct, the remaining lists and the reason codes),
mTcp within the project's pose bound 1e-4 absolute (the aim is 0: both sides
accumulate in double and round once; each test prints the largest difference
it met)."""
import numpy as np
import pytest

import _cull_problems as cp
from _pkg import load_pkg

pytestmark = pytest.mark.gpu
orbpl = load_pkg()

TOL = 1e-4
KFC_FIELDS = ("obs", "n_obs", "bad", "ref_kf", "conn_w", "ordered", "parent", "kf_bad", "to_be_erased",
              "list", "n_mps", "n_redundant", "action", "n_points_bad")
RC_FIELDS = ("obs", "n_obs", "bad", "recent", "reason", "line_bad", "recent_lines", "line_reason")
SMALL = cp.HAND


@pytest.fixture(scope="module")
def culler():
    cam = orbpl.Camera(cp.CAM["fx"], cp.CAM["fy"], cp.CAM["cx"], cp.CAM["cy"], 0.0, 0.0, 0.0, 0.0, 0.0,
                       cp.CAM["bf"], float(cp.TH_DEPTH), 640, 480)
    return orbpl.MapCuller(cam, cp.SCALE, cp.SIGMA2)


def compare(got, want, what=""):
    """the integer outputs equal; returns the largest mTcp difference"""
    for k in range(len(want["mp"])):
        assert np.array_equal(got["mp"][k], want["mp"][k]), (what, "mp", k)
    for f in KFC_FIELDS:
        assert np.array_equal(np.asarray(got[f]), np.asarray(want[f])), (what, f)
    worst = float(np.abs(np.asarray(got["Tcp"], np.float64) - np.asarray(want["Tcp"], np.float64)).max())
    assert worst <= TOL, (what, worst)
    return worst


def compare_recent(got, want, what=""):
    for f in ("mp", "ml"):
        assert len(got[f]) == len(want[f])
        for k in range(len(want[f])):
            assert np.array_equal(got[f][k], want[f][k]), (what, f, k)
    for f in RC_FIELDS:
        assert np.array_equal(np.asarray(got[f]), np.asarray(want[f])), (what, f)


@pytest.mark.parametrize("name", cp.NAMES)
def test_each_problem_alone(culler, name):
    got = culler.keyframes([cp.problem(name)])[0]
    worst = compare(got, cp.ref_run(name)[0], what=name)
    print(f"{name}: largest mTcp difference {worst:.3g}")


@pytest.mark.parametrize("count", [1, 3, 70])
def test_mixed_batches(culler, count):
    names = [("s8", "tree_chain", "goes_bad")[i % 3] for i in range(count)] if count <= 3 else \
        [SMALL[i % len(SMALL)] for i in range(count)]
    got = culler.keyframes([cp.problem(n) for n in names])
    worst = max(compare(g, cp.ref_run(n)[0], what=n) for g, n in zip(got, names))
    print(f"batch of {count}: largest mTcp difference {worst:.3g}")


def test_device_pools_bit_equal_to_host_entry(culler):
    names = ["tree_chain", "nkf1", "s8", "goes_bad", "bad_entry", "k64", "nmps0"]
    probs = [cp.problem(n) for n in names]
    host = culler.keyframes(probs)
    pools = orbpl.KfcDeviceProblems(culler, probs)
    culler.keyframes_device(pools)
    dev = pools.download()
    for n, h, d in zip(names, host, dev):
        compare(d, cp.ref_run(n)[0], what=n)
        for k in range(len(h["mp"])):
            assert np.array_equal(h["mp"][k], d["mp"][k])
        for f in KFC_FIELDS + ("Tcp",):
            assert np.asarray(h[f]).tobytes() == np.asarray(d[f]).tobytes(), (n, f)   # floats bit for bit
    pools.upload()                                             # a second run from the same inputs
    pools.run()
    for h, d in zip(host, pools.download()):
        assert np.asarray(h["Tcp"]).tobytes() == np.asarray(d["Tcp"]).tobytes()
        assert np.array_equal(h["obs"], d["obs"]) and np.array_equal(h["parent"], d["parent"])


def test_list_order_matters(culler):
    """two keyframes that are each redundant only through the other: the first
    in the list is culled, the second then is not; reversed, it is the other"""
    ab, ba = culler.keyframes([cp.problem("order_ab"), cp.problem("order_ba")])
    compare(ab, cp.ref_run("order_ab")[0], "order_ab")
    compare(ba, cp.ref_run("order_ba")[0], "order_ba")
    assert ab["kf_bad"].tolist() == [0, 0, 1, 0, 0] and ba["kf_bad"].tolist() == [0, 0, 0, 1, 0]
    assert ab["action"].tolist() == ba["action"].tolist() == [orbpl.KFC_ACTIONS.index("culled"),
                                                              orbpl.KFC_ACTIONS.index("kept")]


def test_a_second_call_sees_the_culled_keyframes_as_gone(culler):
    """the result of a call is a valid input: the culled keyframes are bad at
    entry, their slots give no observations, and the restatement agrees"""
    import _cull_ref as ref
    p = cp.problem("s12")
    got = culler.keyframes([p])[0]
    m = dict(p["map"], kfs=[dict(k, mp=got["mp"][i]) for i, k in enumerate(p["map"]["kfs"])],
             ref_kf=np.where(got["ref_kf"] < 0, 0, got["ref_kf"]), bad=got["bad"])
    p2 = dict(p, map=m, conn_w=got["conn_w"], ordered=[[int(x) for x in r if x >= 0] for r in got["ordered"]],
              parent=got["parent"], kf_bad=got["kf_bad"], Tcp=got["Tcp"])
    again = culler.keyframes([p2])[0]
    compare(again, ref.keyframe_culling(p2, cp.TH_DEPTH)[0], "s12 again")
    assert np.all(again["obs"][:, np.flatnonzero(got["kf_bad"])] == -1)


@pytest.mark.parametrize("name", cp.RC_NAMES)
def test_recent_on_every_problem(culler, name):
    got = culler.recent([cp.recent_problem(name)])[0]
    compare_recent(got, cp.recent_ref_run(name)[0], what=name)


def test_recent_batch(culler):
    names = [cp.RC_NAMES[i % len(cp.RC_NAMES)] for i in range(30)]
    got = culler.recent([cp.recent_problem(n) for n in names])
    for g, n in zip(got, names):
        compare_recent(g, cp.recent_ref_run(n)[0], what=n)
