"""The sequential restatement of the three per-frame point matchers
(tests/_match_ref.py) against the C++ oracle and against the values worked out
by hand in tests/_match_cases.py, and the witness that the cases and crowds
reach what they were built for: every reason code, the re-scan of the top-4
scheme, claims across 64-point chunks, overwritten non-claimers and both
outcomes of the rotation cut. No GPU."""
import functools

import numpy as np
import pytest

import _match_cases as MC
import _match_ref as M

KINDS = ("last", "local", "bow")


@functools.lru_cache(maxsize=None)
def _problems(kind):
    return tuple(MC.all_problems(kind))


@functools.lru_cache(maxsize=None)
def _ref(kind, k):
    return MC.run_ref(_problems(kind)[k])


def _ids(kind):
    return [p.name for p in MC.all_problems(kind)]


def _params():
    return [pytest.param(kind, k, id=f"{kind}-{name}") for kind in KINDS
            for k, name in enumerate(_ids(kind))]


def test_case_names_are_unique():
    for kind in KINDS:
        names = _ids(kind)
        assert len(set(names)) == len(names), kind


@pytest.mark.parametrize("kind,k", _params())
def test_oracle_equals_restatement(oracle, kind, k):
    P = _problems(kind)[k]
    match, nm, _, _ = _ref(kind, k)
    om, on = MC.run_oracle(oracle, P)
    assert on == nm, P
    bad = np.flatnonzero(om != match)
    assert bad.size == 0, (P, int(bad[0]), int(om[bad[0]]), int(match[bad[0]]))


@pytest.mark.parametrize("kind,k", _params())
def test_case_reaches_what_it_was_built_for(kind, k):
    P = _problems(kind)[k]
    match, nm, rec, info = _ref(kind, k)
    for i, want in P.expect.items():
        for field, value in want.items():
            assert rec[i][field] == value, (P, i, field, rec[i][field], value)
        if want["reason"] in (M.ACCEPTED, M.ACCEPTED_OVERWRITES, M.ROT_CUT):
            assert rec[i]["kp"] >= 0
    npad = getattr(P, "npad", 0)
    if npad:
        # the padding lies in no window, and some point takes the highest index
        for r in rec:
            assert all(j >= npad for j in r.get("window", ())), P
        assert len(match) in (1025, 2048) and any(r["kp"] == len(match) - 1 for r in rec)
    # match / nmatches against the records: a keypoint's entry is its last
    # writer unless some writer's bin was cut
    writers = {}
    for i, r in enumerate(rec):
        if r["kp"] >= 0:
            writers.setdefault(r["kp"], []).append(i)
    for j, ws in writers.items():
        cut = any(rec[i]["reason"] == M.ROT_CUT for i in ws)
        assert match[j] == (-1 if cut else ws[-1])
    assert nm == sum(1 for r in rec if r["reason"] in (M.ACCEPTED, M.ACCEPTED_OVERWRITES))


@pytest.mark.parametrize("kind", KINDS)
def test_every_reason_code_is_reached_or_argued_unreachable(kind):
    seen = set()
    for k, P in enumerate(_problems(kind)):
        seen |= {r["reason"] for r in _ref(kind, k)[2]}
    assert None not in seen
    unreachable = set(M.UNREACHABLE[kind])
    assert not (seen & unreachable), seen & unreachable
    assert seen | unreachable == set(M.REASONS), set(M.REASONS) - seen - unreachable


@pytest.mark.parametrize("kind", KINDS)
def test_replay_topk_equals_the_loop_and_rescans(kind):
    rescans = 0
    for k, P in enumerate(_problems(kind)):
        match, nm, _, _ = _ref(kind, k)
        tm, tn, n_rescans = MC.run_topk(P)
        assert tn == nm and np.array_equal(tm, match), P
        rescans += n_rescans
        if P.name.startswith("exhaustion"):
            assert n_rescans > 0, P
    assert rescans > 0


@pytest.mark.parametrize("kind", KINDS)
def test_a_scheme_without_the_rescan_is_caught(kind):
    """non-vacuity of the GPU comparison: the top-4 scheme without its re-scan
    gives other matches on the exhaustion case and on some crowd"""
    caught = set()
    for k, P in enumerate(_problems(kind)):
        if P.name == "exhaustion" or P.name.startswith("crowd") or P.name == "runs":
            match, nm, _, _ = _ref(kind, k)
            tm, tn, _, _ = MC.run_ref(P, scheme="topk_without_rescan")
            if tn != nm or not np.array_equal(tm, match):
                caught.add(P.name[:5])
    assert "crowd" in caught and caught & {"exhau", "runs"}, caught


@pytest.mark.parametrize("kind", KINDS)
def test_crowds_force_the_replay(kind):
    """across a matcher's crowds: >= 20 points that skipped at least four
    claimed candidates and had more (the re-scan), at >= 3 different chunk
    positions i // 64 (the chunks of wave 0's replay in the two projection
    kernels; the BoW kernel walks a node with one lane and has no chunks, the
    position only says that the points are spread over the keyframe); >= 10 %
    of the accepts overwrite a non-claimer (bow: every match claims, see
    UNREACHABLE); rotation bins both cut and kept"""
    names = _ids(kind)
    deep, chunks, accepts, overwrites, cut, kept = 0, set(), 0, 0, 0, 0
    for k, name in enumerate(names):
        if not name.startswith("crowd"):
            continue
        _, _, rec, info = _ref(kind, k)
        for i, r in enumerate(rec):
            if r["skipped"] >= 4 and r["ncand"] > 4:
                deep += 1
                chunks.add(i // 64)
            if r["reason"] in (M.ACCEPTED, M.ACCEPTED_OVERWRITES, M.ROT_CUT):
                accepts += 1
                overwrites += r["overwrote"]
            cut += r["reason"] == M.ROT_CUT
        if "keep" in info:
            kept += sum(1 for b in info["keep"] if b >= 0)
    assert deep >= 20, deep
    assert len(chunks) >= 3, chunks
    if kind != "bow":
        assert overwrites * 10 >= accepts, (overwrites, accepts)
    if kind != "local":
        assert cut > 0 and kept > 0, (cut, kept)


def test_keyframe_crowds_force_the_replay():
    """SearchByProjection(CurrentFrame, pKF), from the trace of
    _reloc_ref.search_by_projection_kf: the same conditions as above, but for
    the overwrites (every match of this function holds its keypoint)"""
    deep, chunks, cut, kept = 0, set(), 0, 0
    for P in MC.crowds()["kf"]:
        match, nm, _, trace = MC.run_ref(P)
        for i, (ncand, skipped, taken) in trace["points"].items():
            if skipped >= 4 and ncand > 4:
                deep += 1
                chunks.add(i // 64)
        keep = [b for b in trace["keep"] if b >= 0]
        kept += len(keep)
        cut += sum(n for b, n in enumerate(trace["hist"]) if b not in keep)
        assert nm == sum(1 for _, _, taken in trace["points"].values() if taken >= 0) - \
            sum(n for b, n in enumerate(trace["hist"]) if b not in keep)
    assert deep >= 20, deep
    assert len(chunks) >= 3, chunks
    assert cut > 0 and kept > 0, (cut, kept)


def test_hand_worked_last_frame_site():
    """one site by hand: keypoints at distances 0 / 1 / 2 from three points
    with one descriptor; the second point does not claim"""
    b = MC.LastBuilder("hand", check_ori=False)
    c = b.new_code()
    ks = [b.kp(100.0 + q, 100.0, 0, MC.flip(c, q)) for q in range(3)]
    b.mp(100.0, 100.0, c, nobs=1)
    b.mp(100.0, 100.0, c, nobs=0)
    b.mp(100.0, 100.0, c, nobs=1)
    match, nm, rec, _ = MC.run_ref(b.done())
    # point 0 takes k0 and claims it; point 1 takes k1 without a claim; point 2 overwrites k1
    assert match.tolist() == [0, 2, -1] and nm == 3 and ks == [0, 1, 2]
    assert [r["reason"] for r in rec] == [M.ACCEPTED, M.ACCEPTED, M.ACCEPTED_OVERWRITES]
    assert [(r["ncand"], r["skipped"]) for r in rec] == [(3, 0), (3, 1), (3, 1)]
