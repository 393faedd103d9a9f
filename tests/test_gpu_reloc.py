"""GPU parity of the two relocalisation pieces against the sequential numpy
reference (tests/_reloc_ref.py, itself pinned by tests/test_reloc_ref.py):
KeyFrameDatabase::DetectRelocalizationCandidates (orbkf_detect_reloc) and
ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist)
(orbm_search_by_projection_kf). Everything is compared bit for bit:
candidates in order, their count, mnRelocWords, the mRelocScore bytes, the
match vector and the return value."""

import numpy as np
import pytest

import _reloc_ref as R
from _reloc_problems import (KP, conflict_problem, level_edge_problem, random_db_batch,
                             sequence_problem, unit_bow, wide_pitch_problem)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ database
def _run_db(orbpl, problems):
    out = orbpl.detect_reloc_batch(problems)
    for pr, o in zip(problems, out):
        cand, words, score, _ = R.detect_reloc(pr["kf_bows"], pr["covis"], pr["reloc_score"],
                                               pr["q_words"], pr["q_vals"])
        assert o["cand"].tolist() == cand
        assert o["common_words"].tolist() == words
        assert o["reloc_score"].tobytes() == score.tobytes()
    return out


def _pr(kf_bows, covis, q, score=None):
    return dict(kf_bows=kf_bows, covis=covis, q_words=q[0], q_vals=q[1],
                reloc_score=np.zeros(len(kf_bows), np.float32) if score is None else score)


def test_db_no_shared_word(orbpl):
    out = _run_db(orbpl, [_pr([unit_bow([1, 2, 3]), unit_bow([7, 9])], [[1], [0]],
                              unit_bow([4, 5, 6, 100]))])
    assert len(out[0]["cand"]) == 0


def test_db_single_keyframe(orbpl):
    out = _run_db(orbpl, [_pr([unit_bow([3, 8, 20, 41])], [[]], unit_bow([8, 41, 77]))])
    assert out[0]["cand"].tolist() == [0]


def test_db_order_follows_first_shared_word(orbpl):
    # keyframe 2 shares the query's smallest word, keyframe 0 its largest: the
    # list (and with singleton groups the result) runs 2, 1, 0
    q = unit_bow([10, 20, 30, 40, 50, 60])
    kf = [unit_bow([50, 60, 70]), unit_bow([20, 30, 71]), unit_bow([10, 40, 72])]
    out = _run_db(orbpl, [_pr(kf, [[], [], []], q)])
    assert out[0]["cand"].tolist() == [2, 1, 0]


def test_db_group_best_is_neighbour_and_dedup(orbpl):
    # keyframe 1 matches the query best; the groups of 0 and 2 both name it
    q = unit_bow(list(range(0, 40, 2)))
    kf = [unit_bow(list(range(0, 34, 2)) + [101, 103]),
          unit_bow(list(range(0, 40, 2))),
          unit_bow(list(range(4, 40, 2)) + [105])]
    pr = _pr(kf, [[1, 2], [0], [1, 0]], q)
    cand, _, _, info = R.detect_reloc(pr["kf_bows"], pr["covis"], pr["reloc_score"], *q)
    assert cand == [1] and info["dedup_removed"] >= 1
    _run_db(orbpl, [pr])


def test_db_stale_score_of_unscored_neighbour(orbpl):
    db = orbpl.KeyFrameDatabase()
    kf = [unit_bow(list(range(0, 30))), unit_bow(list(range(20, 50))), unit_bow(list(range(45, 60)))]
    for w, v in kf:
        db.add(w, v)
    covis = [[1], [0, 2], [1]]
    for k, c in enumerate(covis):
        db.set_covisibles(k, c)
    score = np.zeros(3, np.float32)
    # query 1 scores keyframe 1; query 2 matches keyframe 0 and shares a few
    # words with keyframe 1, which stays under the threshold: its score from
    # query 1 enters keyframe 0's group
    for q in (unit_bow(list(range(20, 50))), unit_bow(list(range(0, 24)))):
        cand, words, after, info = R.detect_reloc(kf, covis, score, *q)
        got = db.DetectRelocalizationCandidates(*q)
        assert got == cand
        assert [db.last_common_words[k] for k in range(3)] == words
        assert np.array([db.reloc_score(k) for k in range(3)], np.float32).tobytes() == \
            after.tobytes()
        score = after
    assert 1 not in info["scored"] and words[1] > 0 and score[1] > 0
    # and it changed the outcome's arithmetic: without the kept score the group sum differs
    fresh = R.detect_reloc(kf, covis, np.zeros(3, np.float32), *q)
    assert fresh[2][1] == 0 and score[1] != 0


def test_db_summation_order(orbpl):
    rng = np.random.default_rng(5)
    words = np.arange(0, 400)
    mag = 10.0 ** rng.uniform(-12, 0, size=400)
    # a double sum's order shows in the float only next to a float rounding
    # boundary, so two keyframes are built to sit on one: word 0 contributes
    # -2 (1 + 2^-24), the float midpoint above 1, and every other term is below
    # half an ulp of that double. Added after it, in word order, each is lost
    # and the score is the tie (rounds to 1.0f); added before it they carry it
    # over the boundary.
    mid = 1.0 + 2.0 ** -24
    mag[0] = mid
    q = (words.astype(np.uint32), mag)
    kf = [(words.astype(np.uint32), 10.0 ** rng.uniform(-12, 0, size=400)) for _ in range(4)]
    for _ in range(2):
        v = 10.0 ** rng.uniform(-18, -16.4, size=400)
        v[0] = mid
        kf.append((words.astype(np.uint32), v))
    pr = _pr(kf, [[] for _ in kf], q)
    fwd = R.detect_reloc(pr["kf_bows"], pr["covis"], pr["reloc_score"], *q)[2]
    rev = R.detect_reloc(pr["kf_bows"], pr["covis"], pr["reloc_score"], *q, reverse_sum=True)[2]
    # the case proves the order only if the order shows in the float
    assert (fwd != rev).any()
    _run_db(orbpl, [pr])


def test_db_random_batch_of_200(orbpl):
    problems = random_db_batch()
    nonempty = two = dedup = 0
    for pr in problems:
        cand, _, _, info = R.detect_reloc(pr["kf_bows"], pr["covis"], pr["reloc_score"],
                                          pr["q_words"], pr["q_vals"])
        nonempty += len(cand) > 0
        two += len(cand) >= 2
        dedup += info["dedup_removed"] > 0
    assert len(problems) == 200 and nonempty >= 150 and two >= 50 and dedup >= 20, \
        (nonempty, two, dedup)
    _run_db(orbpl, problems)


def test_db_capacity(orbpl):
    rng = np.random.default_rng(9)
    qw = np.sort(rng.choice(20000, 4096, replace=False)).astype(np.uint32)
    q = (qw, rng.random(4096) / 2048)
    kf = []
    for k in range(64):
        w = np.sort(np.concatenate([rng.choice(qw, 300 + 5 * k, replace=False),
                                    20000 + rng.choice(5000, 100, replace=False)]))
        kf.append((w.astype(np.uint32), rng.random(len(w)) / len(w)))
    covis = [list(rng.choice(64, 10, replace=False)) for _ in range(64)]
    _run_db(orbpl, [_pr(kf, covis, q)])
    with pytest.raises(orbpl.OrbplError, match="-1"):
        orbpl.detect_reloc_batch([_pr(kf + [kf[0]], covis + [[]], q)])
    with pytest.raises(orbpl.OrbplError, match="-1"):
        orbpl.detect_reloc_batch([_pr(kf[:2], covis[:2], q)], scoring=1)


# ---------------------------------------------------------------- projection
def _run_proj(orbpl, P, th, orb_dist, check_ori):
    F = R.RefFrame(P["cam_cfg"], P["bounds"], P["scale"], P["cur"]["Tcw"], P["cur"]["kps_un"],
                   P["cur"]["desc"])
    kf = P["kf"]
    ref_m, ref_n = R.search_by_projection_kf(F, P["cur_has_mp"], kf["angle"], kf["valid"],
                                             kf["found"], kf["mp_xyz"], kf["mp_min_dist"],
                                             kf["mp_max_dist"], kf["mp_desc"], th, orb_dist,
                                             check_ori)
    m, n = orbpl.ORBmatcher(0.75, check_ori).SearchByProjectionKeyFrame(
        orbpl.make_camera(P["cam_cfg"]), P["scale"], P["cur"], P["cur_has_mp"], kf, th, orb_dist)
    assert n == ref_n
    assert m.tobytes() == ref_m.tobytes()
    return ref_m, ref_n


@pytest.mark.parametrize("check_ori", [True, False])
@pytest.mark.parametrize("th,orb_dist", [(10, 100), (3, 64)])
def test_proj_sequence(orbpl, th, orb_dist, check_ori):
    P = sequence_problem()
    _, n = _run_proj(orbpl, P, th, orb_dist, check_ori)
    if (th, orb_dist) == (10, 100):
        assert n >= 30      # an all -1 output cannot pass


@pytest.mark.parametrize("check_ori", [True, False])
def test_proj_conflict_128_points_40_keypoints(orbpl, check_ori):
    P = conflict_problem()
    m, n = _run_proj(orbpl, P, 10, 100, check_ori)
    if not check_ori:
        # the first points take the keypoints one by one, best first
        assert n == P["expect_claims"] and sorted(m[m >= 0].tolist()) == list(range(n))


@pytest.mark.parametrize("check_ori", [True, False])
def test_proj_conflict_wide_pitch(orbpl, check_ori):
    """more than 1024 keypoints: the 2048-keypoint build of the matcher, whose
    matches all lie behind the padding"""
    P = wide_pitch_problem()
    assert len(P["cur"]["kps_un"]) == 1090 and len(P["kf"]["angle"]) == 128
    m, n = _run_proj(orbpl, P, 10, 100, check_ori)
    assert (np.flatnonzero(m >= 0) >= 1024).all()
    if check_ori:
        assert n >= 1
    else:
        assert n == P["expect_claims"]


def test_proj_level_edges(orbpl):
    P = level_edge_problem()
    m, n = _run_proj(orbpl, P, 10, 100, False)
    assert n >= 4
    # even points predict level 0, odd ones nlevels - 1: levels [-1, 1] / [6, 8]
    octave = P["cur"]["kps_un"]["octave"]
    for i in np.flatnonzero(m >= 0):
        assert octave[i] in ((0, 1) if m[i] % 2 == 0 else (6, 7))
    assert {int(k) % 2 for k in m[m >= 0]} == {0, 1}


def test_proj_empty_and_capacity(orbpl):
    P = dict(conflict_problem())
    kf, cur = P["kf"], P["cur"]
    none = {k: v[:0] for k, v in kf.items()}
    Q = dict(P, kf=none)
    m, n = _run_proj(orbpl, Q, 10, 100, True)
    assert n == 0 and (m == -1).all()
    Q = dict(P, cur=dict(Tcw=cur["Tcw"], kps_un=cur["kps_un"][:0], desc=cur["desc"][:0]),
             cur_has_mp=P["cur_has_mp"][:0])
    m, n = _run_proj(orbpl, Q, 10, 100, True)
    assert n == 0 and len(m) == 0
    Q = dict(P, kf=dict(kf, found=np.ones_like(kf["found"])))
    m, n = _run_proj(orbpl, Q, 10, 100, True)
    assert n == 0 and (m == -1).all()
    big = dict(Tcw=cur["Tcw"], kps_un=np.zeros(2049, KP), desc=np.zeros((2049, 32), np.uint8))
    with pytest.raises(orbpl.OrbplError, match="-1"):
        orbpl.ORBmatcher(0.75, True).SearchByProjectionKeyFrame(
            orbpl.make_camera(P["cam_cfg"]), P["scale"], big, np.zeros(2049, np.uint8), kf, 10, 100)
