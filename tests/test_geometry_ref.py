"""CPU tests of the extractor geometries that test_gpu_geometry.py runs on the
device: the host geometry (orbx_describe / lsdx_describe, no device call)
against the oracle's, the configurations that are refused, and the
non-vacuity of the inputs (the oracle's level populations per ORB case and
its segment counts per line-detector size)."""
import ctypes as C

import numpy as np
import pytest

import _geometry_cases as G


@pytest.mark.parametrize("c", G.ORB_CASES, ids=G.orb_case_id)
def test_describe_matches_oracle_level_table(c, orbpl, oracle):
    d = orbpl.describe(*G.orb_params(c), width=c.w, height=c.h)
    lw, lh, nf, sc, _ = oracle.level_sizes(oracle.params(*G.orb_params(c)), c.w, c.h)
    assert np.array_equal(d["width"], lw)
    assert np.array_equal(d["height"], lh)
    assert np.array_equal(d["nfeatures"], nf)
    assert np.array_equal(d["scale"].view(np.uint32), sc.view(np.uint32))
    assert d["width"][0] == c.w and d["height"][0] == c.h
    assert min(d["width"].min(), d["height"].min()) >= 20
    assert d["max_keypoints"] >= int(nf.sum())


def _describe_rc(orbpl, nfeatures, scale, levels, w, h):
    """(return code, message) of orbx_describe without raising."""
    p = orbpl.OrbParams(nfeatures, scale, levels, 20, 7)
    n = max(1, levels)
    lw, lh, nf = (np.zeros(n, np.int32) for _ in range(3))
    sc = np.zeros(n, np.float32)
    mk = C.c_int(0)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    rc = orbpl.lib().orbx_describe(C.byref(p), w, h, ptr(lw), ptr(lh), ptr(nf), ptr(sc),
                                   C.byref(mk))
    return rc, orbpl.lib().orbpl_last_error().decode(errors="replace")


REFUSALS = [
    ("nlevels_17", (500, 1.2, 17, 321, 243), "nlevels out of range"),
    ("scale_1", (500, 1.0, 8, 321, 243), "scale_factor must be > 1"),
    ("top_level_under_20px", (50, 1.2, 6, 60, 44), "smaller than 20 px"),
    ("over_1024_cells", (2000, 1.2, 8, 1920, 1080), "more than 1024 FAST cells"),
    ("level_budget_over_octree_list", (4704, 1.2, 8, 641, 479), "octree list capacity"),
]


@pytest.mark.parametrize("name,args,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_geometries(name, args, msg, orbpl):
    rc, text = _describe_rc(orbpl, *args)
    assert rc == orbpl.ORBPL_ERR_ARG
    assert msg in text, text


def test_refusals_have_distinct_messages(orbpl):
    texts = [_describe_rc(orbpl, *r[1])[1] for r in REFUSALS]
    texts.append(_describe_rc(orbpl, 500, SCALE_FIRST_REFUSED, 2, 321, 243)[1])
    assert len(set(texts)) == len(texts), texts


# The resize walk reads the source bytes of 4 adjacent output columns from 3
# dwords (12 bytes from a 4-byte-aligned start): the columns' source span,
# 3 * ratio + 2 bytes plus up to 3 bytes of misalignment, fits for every level
# ratio up to 2 and, depending on the widths, a little above. Stepping the
# scale factor by 0.25 from 2.0 on a 321x243 frame with 2 levels, the first
# refused value and the one before it:
SCALE_LAST_ACCEPTED = 2.25
SCALE_FIRST_REFUSED = 2.5


def test_smallest_refused_scale_factor(orbpl):
    sf, last_ok = 2.0, None
    while sf <= 6.0:
        rc, text = _describe_rc(orbpl, 500, sf, 2, 321, 243)
        if rc != orbpl.ORBPL_OK:
            break
        last_ok = sf
        sf += 0.25
    assert rc == orbpl.ORBPL_ERR_ARG
    assert "scale factor too large for the resize walk" in text
    assert (last_ok, sf) == (SCALE_LAST_ACCEPTED, SCALE_FIRST_REFUSED)
    # every scale factor the GPU cases use is on the accepted side
    assert max(c.scale for c in G.ORB_CASES) <= SCALE_LAST_ACCEPTED


@pytest.mark.parametrize("c", G.ORB_CASES, ids=G.orb_case_id)
def test_orb_cases_are_not_vacuous(c, oracle, synth):
    """The oracle's keypoints per level follow the populated / empty pattern
    each case was chosen for."""
    img = synth.textured_image(c.w, c.h, seed=G.ORB_SEED)
    p = oracle.params(*G.orb_params(c))
    kps, desc, cnt = oracle.extract(p, img, cap=2 * c.nfeatures + 1024)
    G.check_level_population(c, cnt)
    assert len(kps) == int(cnt.sum())
    # levels without a FAST cell (a side below 59 px) hold no keypoint
    lw, lh, _, _, _ = oracle.level_sizes(p, c.w, c.h)
    for l in range(c.levels):
        if min(lw[l], lh[l]) < 59:
            assert cnt[l] == 0, l


def test_orb_cases_cover_the_intended_geometries(orbpl):
    """The properties the cases are named for, from the host geometry."""
    by = {G.orb_case_id(c): orbpl.describe(*G.orb_params(c), width=c.w, height=c.h)
          for c in G.ORB_CASES}
    top20 = by["72x72_n200_s1.2_l8_t20-7"]
    assert top20["width"][-1] == 20 and top20["height"][-1] == 20
    nocell = by["60x44_n50_s1.2_l4_t20-7"]
    assert nocell["height"].max() < 59
    assert by["641x479_n1000_s1.2_l8_t20-7"]["width"][0] % 16 != 0
    assert by["322x241_n500_s1.2_l8_t20-7"]["width"][0] % 4 == 2
    # nfeatures = 1: every level's list capacity is 4 * nIni, not nfeat + 3
    one = by["321x243_n1_s1.2_l8_t20-7"]
    assert one["nfeatures"].sum() == 1 and one["max_keypoints"] >= 4 * 8
    assert by["321x243_n500_s1.05_l16_t20-7"]["width"].size == 16
    # level 0's list (nfeat + 3) is exactly the octree's capacity
    assert by["641x479_n4703_s1.2_l8_t20-7"]["nfeatures"][0] + 3 == 1024


def test_full_octree_list_case_fills_level_0(oracle, synth):
    """The largest-budget case is only a test of a full list if the image
    supplies the features: the oracle reaches the budget on level 0."""
    c = next(c for c in G.ORB_CASES if c.nfeatures == 4703)
    img = synth.textured_image(c.w, c.h, seed=G.ORB_SEED)
    _, _, cnt = oracle.extract(oracle.params(*G.orb_params(c)), img, cap=2 * c.nfeatures)
    assert 1021 <= cnt[0] <= 1024, cnt


@pytest.mark.parametrize("s", G.LSD_SIZES, ids=G.lsd_size_id)
def test_lsd_geometry_matches_oracle(s, orbpl, oracle):
    w, h = s[0], s[1]
    d = orbpl.lsd_describe(w, h)
    sw, sh, min_reg = oracle.lsd_geometry(w, h)
    assert (d["sw"], d["sh"], d["min_reg_size"]) == (sw, sh, min_reg)
    assert min_reg >= 1 and sw < w and sh < h


def test_lsd_size_limits(orbpl):
    for w, h in ((15, 16), (16, 15), (4097, 16), (16, 4097)):
        with pytest.raises(orbpl.OrbplError):
            orbpl.lsd_describe(w, h)
    assert orbpl.lsd_describe(16, 16)["sw"] == 13


@pytest.mark.parametrize("s", G.LSD_SIZES, ids=G.lsd_size_id)
def test_lsd_inputs_are_not_vacuous(s, oracle, synth):
    """The oracle's segment count on each line-detector input: at least the
    stated minimum, or exactly none on the zero-segment frames."""
    w, h, source, fewest = s
    n = len(oracle.lsd_detect(G.lsd_image(synth, w, h, source)))
    if fewest == 0:
        assert n == 0
    else:
        assert n >= fewest, n


def test_polygon_image_is_seeded():
    a = G.polygon_image(97, 67, 3)
    assert a.shape == (67, 97) and a.dtype == np.uint8
    assert np.array_equal(a, G.polygon_image(97, 67, 3))
    assert not np.array_equal(a, G.polygon_image(97, 67, 4))
