"""GPU: LocalMapping::CreateNewMapPoints + CreateNewMapLines as one batched call
(orblm_create_new_map_features*, orbm_search_for_triangulation,
orbl_search_for_triangulation; csrc/local_mapping.hip) against the sequential restatement
tests/_localmap_ref.py on the problems of tests/_localmap_problems.py.

Bit-equal: the pairs per neighbour, the point and line records (neighbour,
idx1, idx2, desc_from, order, count) and KF1's slot arrays; the host and the device entry
are bit-equal to each other, floats included. Positions, normals and distances
agree with the restatement within 1e-4 absolute (the project's pose bound; the
aim is 0 and each test prints the difference it measured)."""
import numpy as np
import pytest

import _localmap_ref as ref
from _localmap_problems import SCALE, SIGMA2, CAM, as_dict, kernel_problem, problems, ref_run

pytestmark = pytest.mark.gpu

TOL = 1e-4
PROBLEMS = problems()
NAMES = list(PROBLEMS)
SMALL = [n for n in NAMES if n != "n2048"]


@pytest.fixture(scope="module")
def mapper(orbpl):
    cam = orbpl.Camera(CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], 0, 0, 0, 0, 0, CAM["bf"], 3.0,
                       640, 480)
    return orbpl.LocalMapper(cam, SCALE, SIGMA2)


def _same(got, name):
    """Returns the largest float difference."""
    want = ref_run(name)
    assert list(got["pairs"]) == want["pairs"], (name, list(got["pairs"]), want["pairs"])
    recs = want["records"]
    pts = got["points"]
    assert len(pts) == len(recs), (name, len(pts), len(recs))
    ints = [(int(r["neighbour"]), int(r["idx1"]), int(r["idx2"]), int(r["desc_from"])) for r in pts]
    assert ints == [tuple(r[:4]) for r in recs], name
    assert np.array_equal(got["kf1_point_record"], want["kf1_point_record"]), name
    d = 0.0
    for r, w in zip(pts, recs):
        d = max(d, float(np.abs(r["xyz"].astype(np.float64) - w[4]).max()),
                float(np.abs(r["normal"].astype(np.float64) - w[5]).max()),
                abs(float(r["min_dist"]) - float(w[6])), abs(float(r["max_dist"]) - float(w[7])))
    assert list(got["line_pairs"]) == want["line_pairs"], (name, list(got["line_pairs"]),
                                                            want["line_pairs"])
    lns, lrecs = got["lines"], want["lines"]
    assert len(lns) == len(lrecs), (name, len(lns), len(lrecs))
    ints = [(int(r["neighbour"]), int(r["idx1"]), int(r["idx2"]), int(r["desc_from"])) for r in lns]
    assert ints == [tuple(r[:4]) for r in lrecs], name
    assert np.array_equal(got["kf1_line_record"], want["kf1_line_record"]), name
    for r, w in zip(lns, lrecs):
        d = max(d, float(np.abs(r["xyz6"].astype(np.float64) - w[4]).max()))
    assert d <= TOL, (name, d)
    return d


def _bit_equal(a, b, what):
    assert a["points"].tobytes() == b["points"].tobytes(), what
    assert np.array_equal(a["kf1_point_record"], b["kf1_point_record"]), what
    assert np.array_equal(a["pairs"], b["pairs"]), what
    assert a["lines"].tobytes() == b["lines"].tobytes(), what
    assert np.array_equal(a["kf1_line_record"], b["kf1_line_record"]), what
    assert np.array_equal(a["line_pairs"], b["line_pairs"]), what


@pytest.mark.parametrize("name", NAMES)
def test_each_problem_alone(mapper, name):
    got = mapper.create_new_map_features([kernel_problem(PROBLEMS[name])])[0]
    d = _same(got, name)
    print(f"{name}: {len(got['points'])} points, {len(got['lines'])} lines, largest difference {d:.3g}")


@pytest.mark.parametrize("names", [["n300"], ["n2048", "n0", "forward"],
                                   [SMALL[i % len(SMALL)] for i in range(70)]],
                         ids=["1", "3", "70"])
def test_mixed_batches(mapper, names):
    got = mapper.create_new_map_features([kernel_problem(PROBLEMS[n]) for n in names])
    d = max(_same(g, n) for g, n in zip(got, names))
    print(f"batch of {len(names)}: largest difference {d:.3g}")


def test_order_of_neighbours_matters(mapper):
    """the same neighbours in reverse order give other records: a point created
    with one neighbour occupies KF1's feature for the next"""
    a, b = mapper.create_new_map_features([kernel_problem(PROBLEMS[n]) for n in ("n300", "n300_rev")])
    fwd = sorted((int(r["neighbour"]), int(r["idx1"]), int(r["idx2"])) for r in a["points"])
    rev = sorted((9 - int(r["neighbour"]), int(r["idx1"]), int(r["idx2"])) for r in b["points"])
    assert fwd != rev


def test_device_entry_equals_host_entry(orbpl, mapper):
    probs = [kernel_problem(PROBLEMS[n]) for n in NAMES]
    host = mapper.create_new_map_features(probs)
    dev = orbpl.LmDeviceProblems(mapper, probs)
    dev.run()
    got = dev.download()
    d = 0.0
    for g, h, n in zip(got, host, NAMES):
        _bit_equal(g, h, n)
        d = max(d, _same(g, n))
    print(f"device entry, {len(NAMES)} problems: largest difference {d:.3g}")


@pytest.mark.parametrize("only_stereo", [False, True])
@pytest.mark.parametrize("check_ori", [False, True])
@pytest.mark.parametrize("name,nb", [("n300", 2), ("bignode", 0), ("forward", 0), ("n1", 0)])
def test_search_for_triangulation(mapper, name, nb, only_stereo, check_ori):
    p = PROBLEMS[name]
    kf1, kf2 = p.cur, p.neigh[nb]
    F12 = ref.compute_f12(p.cam, kf1, kf2)
    want = ref.search_for_triangulation(p.cam, kf1, kf2, F12, None, only_stereo, check_ori)
    pairs, gF = mapper.search_for_triangulation(as_dict(kf1), as_dict(kf2), only_stereo, check_ori)
    assert gF.tobytes() == F12.tobytes(), (name, gF, F12)
    assert [tuple(int(x) for x in r) for r in pairs] == want, name
    print(f"{name}/{nb} only_stereo={only_stereo} check_ori={check_ori}: {len(want)} pairs")


@pytest.mark.parametrize("name,nb", [("n300", 1), ("forward", 0), ("forward", 1), ("n65", 0),
                                     ("n65", 2), ("n1", 0), ("mixed", 1)])
def test_line_search_for_triangulation(orbpl, name, nb):
    """NL = 256 / 80 / 2 / 1 / 0 on either side"""
    p = PROBLEMS[name]
    want = ref.line_search_for_triangulation(p.cur.ldesc, p.neigh[nb].ldesc)
    pairs = orbpl.line_search_for_triangulation(p.cur.ldesc, p.neigh[nb].ldesc)
    assert [tuple(int(x) for x in r) for r in pairs] == want, name
    print(f"{name}/{nb}: {p.cur.nl} x {p.neigh[nb].nl} lines, {len(want)} pairs")


def test_matchers_by_hand(orbpl, mapper):
    """the caller's F12 is the one used; lineDescriptorMAD on the hand-made case
    of test_localmap_ref.test_line_matcher_medians"""
    p = PROBLEMS["forward"]
    kf1, kf2 = p.cur, p.neigh[1]
    F12 = ref.compute_f12(p.cam, kf1, kf2)
    want = ref.search_for_triangulation(p.cam, kf1, kf2, F12)
    pairs, used = mapper.search_for_triangulation(as_dict(kf1), as_dict(kf2), F12=F12)
    assert used.tobytes() == F12.tobytes() and [tuple(int(x) for x in r) for r in pairs] == want
    other = ref.search_for_triangulation(p.cam, kf1, kf2, F12.T.copy())
    pairs, used = mapper.search_for_triangulation(as_dict(kf1), as_dict(kf2), F12=F12.T.copy())
    assert [tuple(int(x) for x in r) for r in pairs] == other and other != want

    def row(k):
        return np.packbits(np.arange(256) < k)
    t = np.stack([row(0), row(100)])
    q = np.stack([row(a) for a in (50, 45, 40, 35, 30)])
    got = orbpl.line_search_for_triangulation(q, t)
    assert [tuple(int(x) for x in r) for r in got] == [(1, 0), (2, 0), (3, 0), (4, 0)]


def test_over_the_cap_is_an_error(orbpl, mapper):
    p = kernel_problem(PROBLEMS["n65"])
    big = dict(p["cur"])
    for k in ("kps", "kps_un", "uright", "depth", "desc", "feat_node", "has_mp", "mp_xyz"):
        big[k] = np.concatenate([p["cur"][k]] * 32)[:2049]
    with pytest.raises(orbpl.OrbplError):
        mapper.create_new_map_features([dict(cur=big, neigh=p["neigh"])])
    with pytest.raises(orbpl.OrbplError):
        mapper.create_new_map_features([dict(cur=p["cur"], neigh=[p["neigh"][0]] * 11)])
    with pytest.raises(orbpl.OrbplError):
        mapper.search_for_triangulation(big, p["neigh"][0])
    many = dict(p["cur"], ldesc=np.zeros((257, 32), np.uint8), lcoef=np.zeros((257, 3)),
                klines=np.zeros(257, orbpl.KEYLINE_DTYPE))
    with pytest.raises(orbpl.OrbplError):
        mapper.create_new_map_features([dict(cur=many, neigh=p["neigh"])])
    with pytest.raises(orbpl.OrbplError):
        orbpl.line_search_for_triangulation(np.zeros((257, 32), np.uint8), np.zeros((3, 32), np.uint8))
