"""The sequential restatement of the per-frame line code (tests/_line_ref.py)
against the C++ oracle, bit for bit, on every hand-built case and crowd of
tests/_line_cases.py, and the witness that the cases reach what they were
built for: every projection, clipping, LineMatching, LineOverLap and stereo
code, the values worked out by hand, both outcomes of every retry rule, and
that each wrong variant of the restatement changes the outputs of a named case.
No GPU."""
import functools

import numpy as np
import pytest

import _line_cases as LC
import _line_ref as R


@functools.lru_cache(maxsize=None)
def _ref(kind, k, entry=None):
    return LC.run_ref(LC.all_problems(kind)[k], entry)


def _params(kinds=LC.KINDS):
    return [pytest.param(kind, k, en, id=f"{kind}-{LC.all_problems(kind)[k].name}" + (f"-{en}" if en else ""))
            for kind in kinds for k, en in LC.runs(kind)]


def _search(name):
    for k, P in enumerate(LC.all_problems("search")):
        if P.name == name:
            return k, P
    raise KeyError(name)


def test_case_names_are_unique():
    for kind in LC.KINDS:
        names = [P.name for P in LC.all_problems(kind)]
        assert len(set(names)) == len(names), kind


@pytest.mark.parametrize("kind,k,entry", _params())
def test_oracle_equals_restatement(oracle, kind, k, entry):
    """match arrays, counts, wiped, the projected KeyLines' bytes (with them the angle
    float(atan2(double, double)) of DESIGN.md P12 against math.atan2), proj_src, pairs and
    depths"""
    P = LC.all_problems(kind)[k]
    want, _ = _ref(kind, k, entry)
    got = LC.run_oracle(oracle, P, entry)
    assert LC.differences(want, got) == [], (P, entry)


# --------------------------------------------------------------------------
# the searches
# --------------------------------------------------------------------------
def _hand_cases():
    return [pytest.param(k, id=P.name) for k, P in enumerate(LC.all_problems("search"))
            if not P.name.startswith("crowd")]


@pytest.mark.parametrize("k", _hand_cases())
def test_search_case_reaches_what_it_was_built_for(k):
    P = LC.all_problems("search")[k]
    e = P.expect
    for en in P.entries:
        out, tr = _ref("search", k, en)
        for i, code in e["codes"].items():
            assert tr["codes"][i] == code, (P, en, i, tr["codes"][i], code)
        if en in e["match"]:
            assert out["match"].tolist() == e["match"][en], (P, en, out["match"].tolist())
        if en in e["nm"]:
            assert out["nm"] == e["nm"][en], (P, en, out["nm"])
        if en in e["retry"]:
            assert tr["retry"]["retried"] == e["retry"][en], (P, en, tr["retry"])
            if en != "last":
                assert out["wiped"] == e["retry"][en]
        if "pairs" in out:
            # every passing pair counts and is listed, in loop order (j, then i)
            assert out["npairs"] == out["nm"] == sum(len(p) for p in tr["passing"][-1])
            assert out["pairs"].tolist() == [[i, j] for j, p in enumerate(tr["passing"][-1])
                                             for i in p][:len(out["pairs"])]
    en = "list" if "list" in P.entries else P.entries[0]
    out, tr = _ref("search", k, en)
    src = tr["proj_src"].tolist()
    for i, seg in e["proj"].items():
        kl = tr["proj_kl"][src.index(i)]
        got = tuple(float(kl[f]) for f in ("startPointX", "startPointY", "endPointX", "endPointY"))
        assert got == tuple(float(np.float32(v)) for v in seg), (P, i, got, seg)
    pg, cg = R.geoms(tr["proj_kl"]), R.geoms(P.cur_kl)
    D = R.hamming_table(P.ml_desc, P.cur_desc)
    for (npass, i, j), want in e["reasons"].items():
        assert npass < len(tr["reasons"]), (P, "the retry did not run")
        got = tr["reasons"][npass][j][src.index(i)]
        if isinstance(want, tuple):
            got = R.line_matching(pg[src.index(i)], cg[j], int(D[i, j]), (R.OFF0, R.OFF1)[npass],
                                  want_exit=True)[1]
            if not isinstance(got, tuple):
                got = (got, None)
        assert got == want, (P, npass, i, j, got, want)


def test_hand_computed_projection_values():
    """the case's own arithmetic, spelled out for four map lines"""
    k, P = _search("projection")
    tr = _ref("search", k, "list")[1]
    src = tr["proj_src"].tolist()

    def kl(name):
        return tr["proj_kl"][src.index(P.names[name])]
    # left border: p0 = -100, q0 = -50, u_min = 0.5: start = (-50 + 50, 100 + 50)
    a = kl("left")
    assert (a["startPointX"], a["startPointY"], a["endPointX"], a["endPointY"]) == (0, 150, 50, 200)
    assert a["lineLength"] == np.float32(np.sqrt(5000.0)) and a["numOfPixels"] == 51
    assert a["pt_x"] == 25 and a["pt_y"] == 175 and a["size"] == 2500
    assert a["response"] == np.float32(np.float32(np.sqrt(5000.0)) / np.float32(640))
    # u * (e - s) = +-1.5 rounds away from zero
    assert kl("half_up")["startPointY"] == 102 and kl("half_down")["startPointY"] == 101
    # x = 640 is kept by LiangBarsky; cv::LineIterator clips it to column 639
    r = kl("right")
    assert r["endPointX"] == 640 and r["numOfPixels"] == 40
    # a start point behind the camera: the crossing is in metres, not pixels
    s = kl("start_behind")
    assert (s["startPointX"], s["startPointY"]) == (np.float32(0.015625), np.float32(0.0078125))
    assert tr["codes"][P.names["horizontal"]] == "IN_FRONT/LB_HORIZONTAL_REJECT"
    assert tr["codes"][P.names["vertical_start_at_minY"]] == "IN_FRONT/LB_VERTICAL_REJECT"


ALL_CODES = set(R.LB_CODES + R.BRANCH_CODES + R.MATCH_REASONS + R.OVERLAP_EXITS)


@pytest.mark.parametrize("entry", LC.ENTRIES)
def test_every_code_is_reached_or_argued_unreachable(entry):
    seen = set()
    for k, P in enumerate(LC.all_problems("search")):
        if entry not in P.entries or P.name.startswith("crowd"):
            continue
        tr = _ref("search", k, entry)[1]
        for c in tr["codes"]:
            seen |= set(c.split("/"))
        for reasons in tr["reasons"]:
            for row in reasons:
                seen |= set(row)
        for (npass, i, j), want in P.expect["reasons"].items():
            if isinstance(want, tuple) and npass < len(tr["reasons"]):
                seen.add(want[1])     # asserted by test_search_case_reaches_what_it_was_built_for
    unreachable = set(R.UNREACHABLE[entry])
    assert not (seen & unreachable)
    assert seen | unreachable == ALL_CODES, ALL_CODES - seen - unreachable


# the case whose outputs each wrong variant changes
CAUGHT_BY = {
    "first_wins": "several_pass",
    "textbook_clip": "projection",
    "retry_le": "retry_10_2",
    "wrap_angle": "thresholds_strict",
    "count_unique": "several_pass",
    "nan_rejects": "nan_fields",
}


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_each_wrong_variant_is_caught_by_a_named_case(variant):
    k, P = _search(CAUGHT_BY[variant])
    caught = []
    for en in P.entries:
        wrong, _ = LC.run_ref(P, en, frozenset([variant]))
        if LC.differences(_ref("search", k, en)[0], wrong):
            caught.append(en)
    # retry_le changes the last-frame / list rule alone (mode 1 has <= as written)
    assert caught == (["last", "list"] if variant == "retry_le" else list(P.entries)), caught


def test_retry_rules_differ_at_the_equalities():
    for name, nl, k in (("retry_10_1", 10, 1), ("retry_10_2", 10, 2), ("retry_10_3", 10, 3),
                        ("retry_5_1", 5, 1), ("retry_15_3", 15, 3)):
        idx, P = _search(name)
        got = {en: _ref("search", idx, en)[1]["retry"] for en in P.entries}
        for en in ("last", "list", "pairs0"):
            assert got[en]["retried"] == (k / nl < 0.2) and got[en]["first_pass"] == k
        assert got["pairs1"]["retried"] == (k <= 0.2 * nl)
        assert (got["pairs1"]["lhs"], got["pairs1"]["rhs"]) == (float(k), 0.2 * nl)
    # mode 1 alone retries at 2 / 10, 1 / 5 and 3 / 15
    for name in ("retry_10_2", "retry_5_1", "retry_15_3"):
        idx, P = _search(name)
        assert [_ref("search", idx, en)[1]["retry"]["retried"] for en in LC.ENTRIES] == \
            [False, False, False, True]
    # mode 0's retry stops on a map line with observations: fewer pairs than its first pass
    idx, P = _search("retry_fewer")
    for en in LC.ENTRIES:
        out, tr = _ref("search", idx, en)
        assert tr["retry"]["first_pass"] == 3 and tr["retry"]["retried"]
        assert (out["nm"] < 3) == (en == "pairs0")
    assert _ref("search", idx, "pairs0")[1]["skipped_claimed"] == [(1, 1, 0), (1, 2, 0), (1, 3, 0)]
    idx, P = _search("retry_nl0")
    lhs = _ref("search", idx, "last")[1]["retry"]["lhs"]
    assert lhs != lhs                                        # 0 / 0


def test_list_without_claims_equals_last_frame(oracle):
    """the list overload with valid = has & !outlier and no claims is the last-frame one"""
    for name in ("projection", "corner_touch", "distorted_tum1", "distorted_negative_bounds"):
        k, P = _search(name)
        m, n, tr = R.search_last(P.cam, P.Tcw, P.cur_kl, P.cur_desc, P.base_kl, P.has_ml, P.outlier,
                                 P.xyz6, P.ml_desc)
        m2, n2, w2, tr2 = R.search_list(P.cam, P.Tcw, P.cur_kl, P.cur_desc, None, P.valid, P.xyz6,
                                        P.ml_desc)
        assert np.array_equal(m, m2) and n == n2 and tr["retry"] == tr2["retry"]
        om, on, _ = oracle.line_search_by_projection_list(oracle.camera(P.cam), P.Tcw, P.cur_kl,
                                                          P.cur_desc, None, P.valid, P.xyz6, P.ml_desc)
        assert np.array_equal(om, m) and on == n


def test_mode0_and_mode1_project_alike():
    """apart from the fields of base_kl that UpdateKeyLineData leaves alone"""
    for k, P in enumerate(LC.all_problems("search")):
        if P.name.startswith("crowd"):
            continue
        a = np.frombuffer(_ref("search", k, "pairs0")[0]["proj_kl"], R.KL).copy()
        b = np.frombuffer(_ref("search", k, "pairs1")[0]["proj_kl"], R.KL).copy()
        assert len(a) == len(b)
        if len(a):
            src = _ref("search", k, "pairs0")[0]["proj_src"]
            assert np.array_equal(a["class_id"], 100 + src) and np.all(a["octave"] == 1)
            assert np.all(b["class_id"] == 0) and np.all(b["octave"] == 0)
            a["class_id"], a["octave"] = 0, 0
        assert a.tobytes() == b.tobytes(), P


def test_search_crowd_conditions():
    """on the restatement alone, per crowd and per entry it runs through: every LineMatching
    reason on >= 5 % of the tested pairs (pooled over the passes that ran: a crowd that
    retries passes next to nothing in its first pass), >= 20 % of the current lines with
    >= 2 passing projected lines, every projection code; across the seeds both retry
    outcomes per entry, and first-pass skips of claimed current lines"""
    retried, skipped = {en: set() for en in LC.ENTRIES}, 0
    for k, P in enumerate(LC.all_problems("search")):
        if not P.name.startswith("crowd"):
            continue
        assert 60 <= len(P.cur_kl) <= 80 and 80 <= len(P.valid) <= 600, P
        for en in P.entries:
            out, tr = _ref("search", k, en)
            flat = [r for reasons in tr["reasons"] for row in reasons for r in row]
            for reason in R.MATCH_REASONS:
                assert flat.count(reason) * 20 >= len(flat), (P, en, reason, flat.count(reason),
                                                              len(flat))
            multi = sum(1 for p in tr["passing"][-1] if len(p) >= 2)
            assert multi * 5 >= len(P.cur_kl), (P, en, multi)
            codes = set(tr["codes"])
            assert {"INVALID", "BOTH_BEHIND", "NO_BRANCH", "START_BEHIND/LB_OK", "END_BEHIND/LB_OK",
                    "IN_FRONT/LB_OK", "IN_FRONT/LB_OUTSIDE", "IN_FRONT/LB_VERTICAL_REJECT",
                    "IN_FRONT/LB_HORIZONTAL_REJECT"} <= codes, (P, en, codes)
            skipped += len(tr["skipped_claimed"])
            retried[en].add(tr["retry"]["retried"])
    for en in LC.ENTRIES:
        assert retried[en] == {False, True}, (en, retried)
    assert skipped >= 100


# --------------------------------------------------------------------------
# match_bf_knn, line_in_frustum, line_frame_prepare, stereo_line_depths
# --------------------------------------------------------------------------
def _f32_equal(got, want):
    return np.asarray(got, np.float32).tobytes() == np.asarray(want, np.float32).tobytes()


@pytest.mark.parametrize("kind", ["bf", "frustum", "prepare"])
def test_known_answers(kind):
    n = 0
    for k, P in enumerate(LC.all_problems(kind)):
        out, _ = _ref(kind, k)
        for name, want in P.expect.items():
            n += 1
            if isinstance(want, bytes):
                assert out[name] == want, (P, name)
            elif out[name].dtype == np.float32 if isinstance(out[name], np.ndarray) else False:
                assert _f32_equal(out[name], want), (P, name, out[name], want)
            else:
                assert np.array_equal(out[name], want), (P, name, out[name], want)
    assert n >= 3


def test_bf_knn_traces():
    P = {p.name: k for k, p in enumerate(LC.all_problems("bf"))}
    tr = _ref("bf", P["tie_lower_index"])[1]
    assert tr[0][:4] == (1, 2, 5, 5) and tr[1][:4] == (3, 4, 7, 7)      # ties: the lower index first
    assert _ref("bf", P["tie_first_of_three"])[1][0][:2] == (0, 1)
    b, s, db, ds, ratio, ok = _ref("bf", P["best0_second0"])[1][0]
    assert (db, ds, ok) == (0, 0, False) and ratio != ratio
    assert _ref("bf", P["ratio_30_40"])[1][0][4] == 0.75 and _ref("bf", P["ratio_29_40"])[1][0][4] < 0.75
    big = _ref("bf", P["nq256_nt300"])
    assert 20 < big[0]["nm"] < 256
    assert len(set(big[0]["out"].tolist()) - {-1}) < big[0]["nm"]           # some were overwritten


def test_frustum_negative_zero():
    P = {p.name: k for k, p in enumerate(LC.all_problems("frustum"))}
    z = _ref("frustum", P["negative_zero"])[1]
    assert z[0, 0] == 0 and np.signbit(z[0, 0]) and z[1, 0] < 0
    z = _ref("frustum", P["accumulation_order"])[1]
    assert z[0, 0] == np.float32(-2.0 ** -30)


def test_prepare_distorted_uright():
    """ur = x_un - bf / depth on the undistorted x, the depth read at the distorted point"""
    P = {p.name: k for k, p in enumerate(LC.all_problems("prepare"))}
    prob = LC.all_problems("prepare")[P["distorted_80"]]
    out = _ref("prepare", P["distorted_80"])[0]
    ku = np.frombuffer(out["kl_un"], R.KL)
    assert np.all(ku["startPointX"] != prob.kl["startPointX"])
    ramp = prob.depth.reshape(-1)
    for i in (0, 40, 79):
        d = ramp[int(prob.kl["startPointY"][i]) * 640 + int(prob.kl["startPointX"][i])]
        assert out["dstart"][i] == d
        assert out["ur_start"][i] == np.float32(ku["startPointX"][i] - np.float32(40.0) / d)
    same = _ref("prepare", P["k1_zero_k2_nonzero"])[0]
    assert same["kl_un"] == prob.kl[:7].tobytes()


@pytest.mark.parametrize("k", range(len(LC.all_problems("stereo"))))
def test_stereo_case_reaches_what_it_was_built_for(k):
    P = LC.all_problems("stereo")[k]
    out, tr = _ref("stereo", k)
    for (i, j), want in P.expect["reasons"].items():
        got = tr[i] if j is None else tr[i][j]
        assert got == want, (P, i, j, got, want)
    for name in ("dstart", "dend"):
        for i, v in P.expect[name].items():
            assert out[name][i] == np.float32(v), (P, name, i, out[name][i])


def test_every_stereo_reason_is_reached_and_crowds_mix_them():
    seen = set()
    for k, P in enumerate(LC.all_problems("stereo")):
        out, tr = _ref("stereo", k)
        flat = [r for t in tr for r in ([t] if isinstance(t, str) else t)]
        if not P.name.startswith("crowd"):
            seen |= set(flat)
            continue
        scanned = [r for t in tr if not isinstance(t, str) for r in t]
        # every reason of the scan at least 30 times among the ~5500 (left, right) pairs, flat
        # left lines, and left lines whose holder is displaced by a better right line
        for reason in R.STEREO_REASONS[1:]:
            assert scanned.count(reason) >= 30, (P, reason, scanned.count(reason))
        assert sum(1 for t in tr if t == R.LEFT_FLAT) >= 8
        assert sum(1 for t in tr if not isinstance(t, str) and t.count(R.TAKEN) >= 2) >= 16
    assert seen | set(R.UNREACHABLE["stereo"]) == set(R.STEREO_REASONS)
