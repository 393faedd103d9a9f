"""orblm_search_in_neighbors, its device-pool form and orbm_fuse on the GPU
against the sequential restatement (tests/_fuse_ref.py): every integer output
and all 32 descriptor bytes equal, normal / min_dist / max_dist within 1e-4
absolute (the aim is 0; each test prints the largest difference it met)."""
import numpy as np
import pytest

import _fuse_problems as fp
import _fuse_ref as ref
from _pkg import load_pkg

pytestmark = pytest.mark.gpu
orbpl = load_pkg()

TOL = 1e-4
INT_FIELDS = ("bad", "replaced_by", "n_obs", "obs", "desc_src", "desc", "n_visible", "n_found",
              "ref_kf", "targets", "n_fused", "n_candidates", "conn_w", "n_ordered", "ordered",
              "ordered_w", "add_conn")
FLOAT_FIELDS = ("normal", "min_dist", "max_dist", "xyz")


@pytest.fixture(scope="module")
def fuser():
    cam = orbpl.Camera(fp.CAM["fx"], fp.CAM["fy"], fp.CAM["cx"], fp.CAM["cy"], 0.0, 0.0, 0.0, 0.0, 0.0,
                       fp.CAM["bf"], 3.0, fp.W, fp.H)
    return orbpl.NeighborFuser(cam, fp.SCALE, fp.SIGMA2)


def _prob(name):
    p = fp.problem(name)
    return dict(map=p["map"], cur=p["cur"])


def compare(got, want, fields=INT_FIELDS, what=""):
    """the integer outputs equal; returns the largest float difference"""
    for k in range(len(want["mp"])):
        assert np.array_equal(got["mp"][k], want["mp"][k]), (what, "mp", k)
    for f in fields:
        if f in want:
            assert np.array_equal(np.asarray(got[f]), np.asarray(want[f])), (what, f)
    worst = 0.0
    for f in FLOAT_FIELDS:
        a, b = np.asarray(got[f], np.float64), np.asarray(want[f], np.float64)
        if a.size:
            worst = max(worst, float(np.abs(a - b).max()))
    assert worst <= TOL, (what, worst)
    return worst


@pytest.mark.parametrize("name", fp.NAMES)
def test_each_problem_alone(fuser, name):
    got = fuser.search_in_neighbors([_prob(name)])[0]
    worst = compare(got, fp.ref_run(name)[1], what=name)
    print(f"{name}: largest float difference {worst:.3g}")


@pytest.mark.parametrize("count", [1, 3, 70])
def test_mixed_batches(fuser, count):
    names = [("n300", "hand_conflict", "n65")[i % 3] for i in range(count)] if count <= 3 else \
        [fp.SMALL[i % len(fp.SMALL)] for i in range(count)]
    got = fuser.search_in_neighbors([_prob(n) for n in names])
    worst = max(compare(g, fp.ref_run(n)[1], what=n) for g, n in zip(got, names))
    print(f"batch of {count}: largest float difference {worst:.3g}")


def test_device_pools_bit_equal_to_host_entry(fuser):
    names = ["n65", "hand_tie", "n300", "n0", "mono_mixed", "kf64"]
    probs = [_prob(n) for n in names]
    host = fuser.search_in_neighbors(probs)
    pools = orbpl.SinDeviceProblems(fuser, probs)
    pools.run()
    dev = pools.download()
    for n, h, d in zip(names, host, dev):
        compare(d, fp.ref_run(n)[1], what=n)
        for k in range(len(h["mp"])):
            assert np.array_equal(h["mp"][k], d["mp"][k])
        for f in INT_FIELDS + FLOAT_FIELDS:
            a, b = np.asarray(h[f]), np.asarray(d[f])
            assert a.tobytes() == b.tobytes(), (n, f)          # floats bit for bit
    pools.upload()                                             # a second run from the same inputs
    pools.run()
    for h, d in zip(host, pools.download()):
        assert np.asarray(h["normal"]).tobytes() == np.asarray(d["normal"]).tobytes()
        assert np.array_equal(h["obs"], d["obs"])


FUSE_CASES = [("n65", "cur_into_first_target"), ("n300", "cur_into_first_target"),
              ("n300", "target_into_cur"), ("hand_tie", "cur_into_first_target"),
              ("hand_conflict", "cur_into_first_target"), ("hand_gates", "cur_into_first_target"),
              ("mono_mixed", "repeats_and_nulls"), ("n2048", "target_into_cur"), ("tiny", "long_list")]


def tiny_problem():
    """the smallest map: two keyframes of three features, two points; point 0 in
    both keyframes, point 1 in the second only, where the first sees its corner"""
    rng = np.random.default_rng(8)
    X0, X1 = np.array([0.1, 0.05, 4.0]), np.array([-0.3, 0.1, 5.0])
    d0, d1 = (rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(2))

    def feat(centre, X, d):
        pu, pv, pz = fp._px(centre, X)
        return (pu, pv, 0, pu - fp.CAM["bf"] / pz, d)

    ca, cb = [0, 0, 0], [0.2, 0, 0]
    a = fp._hand_kf(3, ca, [feat(ca, X0, d0), feat(ca, X1, fp._flip(rng, d1, 5)),
                            (50.0, 60.0, 0, -1.0, fp._flip(rng, d0, 120))])
    b = fp._hand_kf(8, cb, [feat(cb, X0, fp._flip(rng, d0, 4)), feat(cb, X1, d1),
                            (90.0, 60.0, 0, -1.0, fp._flip(rng, d1, 120))])
    a["mp"][:], b["mp"][:] = [0, -1, -1], [0, 1, -1]
    a["ordered"], b["ordered"] = [1], [0]
    return fp._finish([a, b], [dict(xyz=X0, ref_kf=0), dict(xyz=X1, ref_kf=1)], 1, [0, 1])


@pytest.mark.parametrize("name,case", FUSE_CASES)
def test_fuse_alone(fuser, name, case):
    p = tiny_problem() if name == "tiny" else fp.problem(name)
    m, cur = p["map"], p["cur"]
    first = m["kfs"][cur]["ordered"][0]
    if case == "long_list":   # longer than M and the widest keyframe: the list alone sets list_pitch
        kf, lst = first, [0, -1, 1, -1, 0]
        assert len(lst) > max(len(m["bad"]), max(len(k["uright"]) for k in m["kfs"]))
    elif case == "cur_into_first_target":
        kf, lst = first, [int(x) for x in m["kfs"][cur]["mp"]]
    elif case == "target_into_cur":
        kf, lst = cur, [int(x) for x in m["kfs"][first]["mp"] if x >= 0]
    else:   # every point of the map twice over, nulls between
        kf = first
        lst = [q for x in range(len(m["bad"])) for q in (x, -1)] * 2
    rmap = ref.Map(fp.camera(), m)
    trace = []
    nf = ref.fuse(fp.camera(), rmap.kfs[kf], [None if x < 0 else rmap.points[x] for x in lst],
                  3.0, trace=trace)
    got_nf, got = fuser.fuse(m, kf, lst)
    assert got_nf == nf
    want = np.array(trace, np.int64).reshape(-1, 3)
    assert np.array_equal(got["reason"], want[:, 0]), [ref.REASONS[r] for r in got["reason"][:20]]
    assert np.array_equal(got["best_idx"], want[:, 1])
    assert np.array_equal(got["best_dist"], want[:, 2])
    worst = compare(got, rmap.state(), what=f"{name}/{case}")
    print(f"{name}/{case}: nFused {nf}, largest float difference {worst:.3g}")


def test_target_order_matters(fuser):
    """the same targets in two orders give different maps, each equal to the
    restatement's for that order"""
    p = fp.problem("n300")
    m, cur = p["map"], p["cur"]
    outs = []
    for rev in (False, True):
        kfs = [dict(k) for k in m["kfs"]]
        o = list(kfs[cur]["ordered"])
        kfs[cur]["ordered"] = o[::-1] if rev else o
        mm = dict(m, kfs=kfs)
        got = fuser.search_in_neighbors([dict(map=mm, cur=cur)])[0]
        compare(got, ref.search_in_neighbors(fp.camera(), mm, cur)[1], what=f"reversed={rev}")
        outs.append(got)
    a, b = outs
    assert not np.array_equal(a["targets"], b["targets"])
    assert not (np.array_equal(a["obs"], b["obs"]) and np.array_equal(a["bad"], b["bad"]))


def test_fuse_counts_a_bad_point_under_the_keypoint(fuser):
    """a map that holds a bad point in a slot at entry (Replace never leaves one):
    Fuse counts the keypoint in nFused and changes nothing"""
    p = fp.problem("hand_conflict")
    m = dict(p["map"], bad=p["map"]["bad"].copy())
    m["bad"][1] = 1                              # B, the point under the target's keypoint
    lst = [int(x) for x in m["kfs"][p["cur"]]["mp"]]
    rmap = ref.Map(fp.camera(), m)
    trace = []
    nf = ref.fuse(fp.camera(), rmap.kfs[1], [rmap.points[x] for x in lst], 3.0, trace=trace)
    got_nf, got = fuser.fuse(m, 1, lst)
    assert nf == got_nf == 1
    assert trace[0][0] == ref.REASONS.index("bad_slot")
    assert np.array_equal(got["reason"], [t[0] for t in trace])
    assert np.array_equal(got["best_idx"], [t[1] for t in trace])
    compare(got, rmap.state(), what="bad_slot")
    for k, kf in enumerate(m["kfs"]):
        assert np.array_equal(got["mp"][k], kf["mp"])
