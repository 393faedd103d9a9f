"""CPU tests of Frame::ComputeStereoMatches branch by branch: the sequential
restatement tests/_stereo_ref.py against the oracle, bit for bit, on the
hand-made cases and the shifted pairs of tests/_stereo_cases.py; every reason
code reached by a case made for it; the non-vacuity of the shifted pairs."""
import numpy as np
import pytest

import _stereo_cases as SC
import _stereo_ref as R

ALL_DIRECTED = SC.DIRECTED + SC.LARGE


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_same(c, res, ur, d):
    bad = np.nonzero((_u32(res.uright) != _u32(ur)) | (_u32(res.depth) != _u32(d)))[0]
    assert len(bad) == 0, (c.name, bad[:5], [R.NAMES[x] for x in res.reason[bad[:5]]])


@pytest.mark.parametrize("fn", ALL_DIRECTED, ids=lambda f: f.__name__[5:])
def test_restatement_equals_oracle_on_directed_case(oracle, fn):
    c = SC.directed(fn)
    res = SC.run_ref(oracle, c)
    ur, d = SC.run_oracle(oracle, c)
    _assert_same(c, res, ur, d)
    # unmatched means -1 in both outputs, matched means a positive depth
    kept = (res.reason == R.ACCEPTED) | (res.reason == R.ACCEPTED_CLAMPED)
    assert np.all(d[kept] > 0) and np.all(ur[~kept] == -1) and np.all(d[~kept] == -1)


@pytest.mark.parametrize("fn", ALL_DIRECTED, ids=lambda f: f.__name__[5:])
def test_directed_case_lands_where_it_was_aimed(oracle, fn):
    """Each named edge takes the branch it was made for: the reason code
    before the median cut (`stage`), after it (`reason`), and the traced
    values (chosen right index, Hamming distance, window centres, smallest
    SAD and its position, deltaR, disparity)."""
    c = SC.directed(fn)
    res = SC.run_ref(oracle, c)
    assert c.stage or c.reason or c.trace
    for i, want in c.stage.items():
        assert res.stage[i] == want, (c.name, i, R.NAMES[want], R.NAMES[res.stage[i]])
    for i, want in c.reason.items():
        assert res.reason[i] == want, (c.name, i, R.NAMES[want], R.NAMES[res.reason[i]])
    for i, vals in c.trace.items():
        for k, v in vals.items():
            assert k in res.trace.get(i, {}), (c.name, i, k, R.NAMES[res.stage[i]])
            got = res.trace[i][k]
            if isinstance(v, np.float32):
                assert np.float32(got).view(np.uint32) == v.view(np.uint32), (c.name, i, k, got, v)
            else:
                assert got == v, (c.name, i, k, got, v)


def test_reason_codes_are_all_reached(oracle):
    """The union over the directed cases holds every reason code an input can
    reach. DELTA_RANGE and DELTA_NAN cannot be reached (the argument stands at
    _stereo_ref.UNREACHABLE; test_parabola_stays_within_half checks it), so
    they must not appear either."""
    seen = set()
    for fn in ALL_DIRECTED:
        res = SC.run_ref(oracle, SC.directed(fn))
        seen |= set(res.stage.tolist()) | set(res.reason.tolist())
    assert seen == set(range(len(R.NAMES))) - R.UNREACHABLE, sorted(R.NAMES[x] for x in seen)


def test_parabola_stays_within_half():
    """deltaR at the first smallest SAD of a curve: d1 > d2 and d3 >= d2, all
    integers up to 121 * 510. Over the extremes of that domain the quotient is
    finite and within [-1/2, 1/2], so the reference's range test and a
    not-a-number deltaR are dead branches; the restatement's `parabola` still
    answers them as the reference would if they were fed."""
    top = 121 * 510
    steps = [0, 1, 2, 3, 255, 510, 4095, 4096, top - 1, top]
    for d2 in (0, 1, 20, 4095, top - 1):
        for p in steps[1:]:
            for q in steps:
                if d2 + p > top or d2 + q > top:
                    continue
                delta = R.parabola(d2 + p, d2, d2 + q)
                assert delta is not None and np.isfinite(delta), (d2, p, q)
                assert -0.5 <= delta <= 0.5, (d2, p, q, delta)
                assert (delta == 0.5) == (q == 0), (d2, p, q, delta)
    # what the dead branches would do
    assert R.parabola(5, 5, 5) != R.parabola(5, 5, 5)      # 0 / 0: not a number, not refused
    assert R.parabola(5, 9, 5) == 0 and R.parabola(0, 5, 9) is None


def test_named_values_of_the_directed_cases(oracle):
    """Values the cases state in words, taken from the oracle's output."""
    c = SC.directed(SC.case_disparity_window)
    ur, d = SC.run_oracle(oracle, c)
    res = SC.run_ref(oracle, c)
    clamped = np.nonzero(res.stage == R.ACCEPTED_CLAMPED)[0]
    assert len(clamped) == 2
    for i in clamped:
        # disparity 0 becomes 0.01f; uRight goes through (double)uL - 0.01
        assert d[i] == np.float32(c.bf) / np.float32(0.01)
        assert ur[i] == np.float32(float(c.kl["x"][i]) - 0.01)
    assert any(c.kl["x"][i] != np.round(c.kl["x"][i]) for i in clamped)
    c = SC.directed(SC.case_capacity_4096)
    assert len(c.kl) == 4096 and len(c.kr) == 4096
    c = SC.directed(SC.case_rows_1024)
    assert c.h == 1024
    c = SC.directed(SC.case_scratch_top_level)
    rows = [len(b) for b in R.row_bands([1, 2, 4, 8], c.h, c.kr)]
    assert set(c.kr["octave"]) == {3} and sum(rows) == 33 * len(c.kr) > 20 * len(c.kr)
    assert (SC.run_oracle(oracle, c)[1] > 0).sum() >= 6


SHIFTED = [(g, s) for s in SC.SHIFT_SIZES for g in SC.SHIFT_GEOMS]


@pytest.mark.parametrize("g,s", SHIFTED, ids=[SC.shifted_id(g, s) for g, s in SHIFTED])
def test_restatement_equals_oracle_on_shifted_pair(oracle, g, s):
    """Oracle keypoints of a textured image and its shifted copy, 1 to 16
    levels. Non-vacuity: at least 30 % of the left keypoints get a depth, on
    at least two levels where the pyramid has two, and the depth is bf / d for
    the disparity d the rows were moved by."""
    c = SC.shifted_case(g[0], g[1], s[0], s[1])
    res = SC.run_ref(oracle, c)
    ur, d = SC.run_oracle(oracle, c)
    _assert_same(c, res, ur, d)
    m = d > 0
    assert m.sum() >= 0.3 * len(c.kl), (m.sum(), len(c.kl))
    per_level = np.bincount(c.kl["octave"][m], minlength=g[0])
    assert (per_level > 0).sum() >= min(2, g[0]), per_level
    _, _, disp = SC.shifted_pair(*s)
    want = disp[np.clip(c.kl["y"][m].astype(int), 0, c.h - 1)]
    near = np.abs((c.kl["x"][m] - ur[m]) - want) < 1.0
    assert near.mean() > 0.95
    assert np.allclose(d[m][near], c.bf / want[near], rtol=0.3)
    assert np.array_equal(_u32(d[m]), _u32(np.float32(c.bf) / (c.kl["x"][m] - ur[m])))


def test_case_geometries_are_accepted(orbpl):
    """Every frame size and pyramid the stereo cases use is one the extractor
    accepts (host geometry, no device call); the 1024-row frame has 1024
    rows on level 0."""
    geoms = {(SC.orb_of(c), c.w, c.h) for c in (SC.directed(fn) for fn in ALL_DIRECTED)}
    geoms |= {((500, g[1], g[0], 20, 7), s[0], s[1]) for g, s in SHIFTED}
    geoms.add(((300, 1.2, 8, 20, 7), 72, 1025))
    for orb, w, h in sorted(geoms):
        d = orbpl.describe(*orb, width=w, height=h)
        assert d["width"][0] == w and d["height"][0] == h and len(d["width"]) == orb[2]
