"""Known answers, worked by hand, for the numpy reference of the two
relocalisation functions (tests/_reloc_ref.py), so that the reference the GPU
tests compare against is not merely consistent with itself. No GPU."""
import numpy as np

import _reloc_ref as R

KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
               ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


def test_three_keyframe_database_by_hand():
    # every value is a binary fraction, so the hand arithmetic is exact
    q = ([1, 2, 5], [0.5, 0.25, 0.25])
    kf = [([2, 5], [0.25, 0.5]),          # word 2: 0 - .25 - .25, word 5: .25 - .25 - .5 -> 0.5
          ([1, 5, 8], [0.5, 0.25, 0.25]),  # word 1: 0 - .5 - .5, word 5: 0 - .25 - .25 -> 0.75
          ([2, 9], [0.125, 0.875])]        # one common word: under the threshold, not scored
    covis = [[1], [2], []]
    # query words ascending, inverted lists in add() order: word 1 -> kf1,
    # word 2 -> kf0, kf2; max common words 2 -> threshold int(1.6) = 1
    cand, words, score, info = R.detect_reloc(kf, covis, [0, 0, 0], *q)
    assert info["sharing"] == [1, 0, 2]
    assert words == [2, 2, 1]
    assert info["scored"] == [1, 0]
    assert score.tolist() == [0.5, 0.75, 0.0]
    # groups: kf1 + kf2 (shares a word, never scored: 0) = 0.75, best kf1;
    # kf0 + kf1 = 1.25, best kf1. Retain > 0.9375: only the second group
    assert cand == [1]
    # the same with a score kf2 kept from an earlier query: kf1's group is
    # 0.75 + 2 = 2.75 with best kf2; retain > 2.0625 drops kf0's group
    cand, _, score, _ = R.detect_reloc(kf, covis, [0, 0, 2.0], *q)
    assert cand == [2]
    assert score.tolist() == [0.5, 0.75, 2.0]
    # kf1 + kf0 = 1.25 and kf0 + kf1 = 1.25 both pass and both name kf1: one entry
    cand, _, _, info = R.detect_reloc(kf, [[1], [0], []], [0, 0, 0], *q)
    assert cand == [1] and info["dedup_removed"] == 1


def _db_with_counts(counts, nq):
    """keyframe k shares its first counts[k] words with a query of nq words"""
    q = (list(range(nq)), [1.0 / nq] * nq)
    kf = []
    for k, c in enumerate(counts):
        w = list(range(c)) + [1000 + k]
        kf.append((w, [1.0 / len(w)] * len(w)))
    return kf, q


def test_min_common_words_boundary():
    # max 5: int(5 * 0.8f) = 4, so 4 common words are out and 5 are in
    kf, q = _db_with_counts([5, 4, 5], 5)
    _, words, _, info = R.detect_reloc(kf, [[], [], []], [0, 0, 0], *q)
    assert words == [5, 4, 5] and info["scored"] == [0, 2]
    # max 10: the float product 10 * 0.8f rounds to 8.0f: 8 out, 9 in
    kf, q = _db_with_counts([10, 8, 9], 10)
    _, words, _, info = R.detect_reloc(kf, [[], [], []], [0, 0, 0], *q)
    assert words == [10, 8, 9] and info["scored"] == [0, 2]


def test_l1_score_order_and_lower_bound():
    # skipping runs on either side (the lower_bound branches)
    s = R.l1_score([1, 4, 9], [0.5, 0.25, 0.25], [2, 3, 4, 5, 9], [0.25, 0.25, 0.25, 0.125, 0.125])
    # word 4: 0 - .25 - .25; word 9: .125 - .25 - .125 -> -(-0.75) / 2
    assert s == 0.375


def test_projection_two_points_compete_for_one_keypoint():
    cam = dict(fx=500.0, fy=500.0, cx=320.0, cy=240.0)
    kps = np.zeros(2, KP)
    kps["x"], kps["y"], kps["octave"] = [320.0, 100.0], [240.0, 100.0], [0, 0]
    desc = np.zeros((2, 32), np.uint8)
    desc[1] = 0xFF
    F = R.RefFrame(cam, (0, 640, 0, 480), [1.0, 1.2, 1.44], np.eye(4), kps, desc)
    # both points project onto (320, 240) +- 1 px at depth 2; level 0 for
    # mfMaxDistance = 2 (ratio 1 -> log 0)
    xyz = np.array([[0.0, 0, 2], [0.004, 0, 2]], np.float32)
    mp_desc = np.zeros((2, 32), np.uint8)
    mp_desc[0, 0] = 0x07          # distance 3 to keypoint 0
    args = dict(cur_has_mp=[0, 0], kf_angle=[10.0, 10.0], kf_valid=[1, 1], kf_found=[0, 0],
                mp_xyz=xyz, mp_min_dist=[1.0, 1.0], mp_max_dist=[2.0, 2.0], mp_desc=mp_desc,
                th=10, orb_dist=100)
    # point 0 comes first and takes the keypoint although point 1 is closer;
    # point 1 then finds it held and has no other candidate within range
    m, n = R.search_by_projection_kf(F, check_ori=False, **args)
    assert m.tolist() == [0, -1] and n == 1
    m, n = R.search_by_projection_kf(F, check_ori=True, **args)
    assert m.tolist() == [0, -1] and n == 1
    # point 0 already found: point 1 gets it
    args["kf_found"] = [1, 0]
    m, n = R.search_by_projection_kf(F, check_ori=False, **args)
    assert m.tolist() == [1, -1] and n == 1
    # the keypoint held on entry: nobody gets it
    args["cur_has_mp"] = [1, 0]
    m, n = R.search_by_projection_kf(F, check_ori=False, **args)
    assert m.tolist() == [-1, -1] and n == 0
    # ORBdist below the distance
    args.update(cur_has_mp=[0, 0], kf_found=[0, 1], orb_dist=2)
    m, n = R.search_by_projection_kf(F, check_ori=False, **args)
    assert m.tolist() == [-1, -1] and n == 0
