"""Extractor geometries off the 640x480 / 1.2 / 8-level default, shared by
test_geometry_ref.py (CPU: geometry tables, refusals, non-vacuity of the
inputs) and test_gpu_geometry.py (GPU: stage parity against the oracle)."""
from collections import namedtuple

import numpy as np

OrbCase = namedtuple("OrbCase", "w h nfeatures scale levels ini_th min_th populated")


def _case(w, h, nf, sf, nl, ini, mn, populated):
    return OrbCase(w, h, nf, sf, nl, ini, mn,
                   None if populated is None else frozenset(populated))


# `populated`: the levels on which the oracle finds keypoints in
# synth.textured_image(w, h, seed=7); every other level must stay empty
ORB_CASES = [
    _case(641, 479, 1000, 1.2, 8, 20, 7, range(8)),     # odd width and height
    _case(322, 241, 500, 1.2, 8, 20, 7, range(8)),      # w = 2 mod 4
    _case(125, 93, 300, 1.2, 8, 20, 7, range(3)),       # levels 3..7 without FAST cells
    _case(72, 72, 200, 1.2, 8, 20, 7, range(1)),        # top level 20 px wide
    _case(60, 44, 50, 1.2, 4, 20, 7, ()),               # no level has a cell
    _case(240, 320, 500, 1.2, 8, 20, 7, range(8)),      # portrait: nIni pinned to 1
    _case(120, 400, 500, 1.2, 8, 20, 7, range(4)),      # tall strip
    _case(400, 120, 500, 1.2, 8, 20, 7, range(4)),      # wide strip: nIni = 3
    _case(321, 243, 500, 2.0, 4, 20, 7, range(2)),      # widest resize span
    _case(321, 243, 500, 1.5, 5, 20, 7, range(4)),
    _case(321, 243, 500, 1.1, 12, 20, 7, range(12)),
    _case(321, 243, 500, 1.05, 16, 20, 7, range(16)),   # kMaxLevels
    _case(321, 243, 500, 1.2, 1, 20, 7, range(1)),      # one level, no resize
    _case(321, 243, 1, 1.2, 8, 20, 7, None),            # kp_cap = 4 * nIni
    _case(321, 243, 3000, 1.2, 8, 20, 7, range(8)),     # budget above supply
    _case(321, 243, 500, 1.2, 8, 7, 7, range(8)),       # iniTh == minTh
    _case(321, 243, 500, 1.2, 8, 100, 100, range(2)),   # nearly every cell empty
    # the largest budget orbx_create accepts at this size: level 0 holds 1021
    # features, its list capacity is the octree's 1024 (4704 is refused)
    _case(641, 479, 4703, 1.2, 8, 20, 7, range(8)),
]


def orb_case_id(c):
    return f"{c.w}x{c.h}_n{c.nfeatures}_s{c.scale}_l{c.levels}_t{c.ini_th}-{c.min_th}"


def orb_params(c):
    return (c.nfeatures, c.scale, c.levels, c.ini_th, c.min_th)


ORB_SEED = 7


def check_level_population(c, level_counts):
    """The oracle's keypoints per level follow the case's populated / empty
    pattern (exact counts are not pinned: they move with the image source)."""
    cnt = [int(x) for x in level_counts]
    assert len(cnt) == c.levels
    if c.populated is None:     # nfeatures = 1: some keypoints, levels not pinned
        assert sum(cnt) > 0, cnt
        return
    for l, n in enumerate(cnt):
        if l in c.populated:
            assert n > 0, (l, cnt)
        else:
            assert n == 0, (l, cnt)


# --- line detector sizes -----------------------------------------------------
# (w, h, image source, fewest segments the oracle must find; 0 = exactly none)
LSD_SIZES = [
    (641, 479, "textured", 100),
    (322, 241, "textured", 10),
    (161, 123, "polygons", 10),
    (240, 320, "polygons", 10),
    (500, 40, "polygons", 10),
    (40, 500, "polygons", 10),
    (97, 67, "polygons", 1),
    (33, 21, "textured", 0),
    (16, 16, "textured", 0),
    # the polygons still leave a few segments on the two smallest frames
    (33, 21, "polygons", 1),
    (16, 16, "polygons", 1),
]
LSD_SEED = 7
# both seed loops (speculative and wave-serial) run at these sizes
LSD_BOTH_LOOPS = {(97, 67), (33, 21), (16, 16), (641, 479)}


def lsd_size_id(s):
    return f"{s[0]}x{s[1]}_{s[2]}"


def polygon_image(w, h, seed):
    """Seeded filled convex polygons (3 to 6 corners on an ellipse, flat grey
    levels at least 40 apart from the background) with +-2 grey levels of
    noise: long straight edges at any frame size, which the textured image
    lacks on small frames."""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 96.0)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    n = max(6, (w * h) // 2500)
    for k in range(n):
        cx, cy = rng.uniform(0, w), rng.uniform(0, h)
        rx = rng.uniform(0.15, 0.45) * max(w, 24)
        ry = rng.uniform(0.15, 0.45) * max(h, 24)
        ang = np.sort(rng.uniform(0, 2 * np.pi, int(rng.integers(3, 7))))
        px, py = cx + rx * np.cos(ang), cy + ry * np.sin(ang)
        inside = np.ones((h, w), bool)
        for i in range(len(ang)):
            x0, y0 = px[i], py[i]
            x1, y1 = px[(i + 1) % len(ang)], py[(i + 1) % len(ang)]
            inside &= (x1 - x0) * (yy - y0) - (y1 - y0) * (xx - x0) >= 0
        level = (30, 160, 220, 60, 190, 250)[k % 6]
        img[inside] = level
    img += rng.integers(-2, 3, (h, w))
    return np.clip(img, 0, 255).astype(np.uint8)


def lsd_image(synth, w, h, source):
    if source == "polygons":
        return polygon_image(w, h, LSD_SEED)
    return synth.textured_image(w, h, seed=LSD_SEED)
