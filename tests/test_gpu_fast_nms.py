"""FAST non-maximum suppression in k_fast_cells: the sparse pass at iniThFAST
over the pixels the walk recorded, and the dense pass at minThFAST of a cell
that has no corner at iniThFAST. Bit-exact against the CPU oracle on an image
built to reach every branch; the image is checked to do so with a numpy
restatement of the FAST score on level 0."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 320, 240
PP = (500, 1.2, 8, 20, 7)
# the 16-pixel Bresenham ring of cv::FAST, in arc order
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3),
        (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]


def _kp_equal(a, b):
    if len(a) != len(b):
        return False
    return all(np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32))
               for f in ("x", "y", "size", "angle", "response")) and \
        np.array_equal(a["octave"], b["octave"]) and np.array_equal(a["class_id"], b["class_id"])


def _scaled(img, k):
    return np.clip(np.rint(128.0 + k * (img.astype(np.float32) - 128.0)), 0, 255).astype(np.uint8)


def _branch_image(synth, seed=42, width=W):
    """Vertical quarters: full contrast | weak corners only, with a flat patch
    that carries a 2-pixel-wide bar (mirror-symmetric: its scores come in equal
    pairs) | uniform noise | a pixel-doubled texture (tied scores)."""
    rng = np.random.default_rng(seed)
    base = synth.textured_image(width, H, seed=seed)
    q = width // 4
    img = base.copy()
    img[:, q:2 * q] = _scaled(base[:, q:2 * q], 0.12)
    img[:, 2 * q:3 * q] = rng.integers(0, 256, (H, q), dtype=np.uint8)
    half = synth.textured_image(width // 2, H // 2, seed=seed + 100)
    rep = np.repeat(np.repeat(half, 2, axis=0), 2, axis=1)
    img[:, 3 * q:] = _scaled(rep[:, :width - 3 * q], 0.45)
    # flat patch and bar inside level 0's cell (row 2, column 3) of a 320-wide
    # frame, next to weak texture of the same cell
    img[92:120, 121:139] = 128
    img[100:112, 129:131] = 230
    return np.ascontiguousarray(img)


def _fast_score(img):
    """m = max(A, -B, 0) per pixel (cv::FAST's cornerScore<16> + 1 where the
    pixel is a corner): A / B = max / min over the 16 9-arcs of the min / max
    of v - ring. Zero on the 3-pixel frame."""
    v = img.astype(np.int16)
    h, w = v.shape
    c = v[3:h - 3, 3:w - 3]
    d = np.stack([c - v[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in RING])
    d2 = np.concatenate([d, d[:8]])
    lo = np.stack([d2[k:k + 9].min(axis=0) for k in range(16)]).max(axis=0)
    hi = np.stack([d2[k:k + 9].max(axis=0) for k in range(16)]).min(axis=0)
    m = np.zeros((h, w), np.int16)
    m[3:h - 3, 3:w - 3] = np.maximum(np.maximum(lo, -hi), 0)
    return m


def _level0_cells(w, h):
    """Detection regions (x0, y0, x1, y1) of the level-0 FAST cells: border 16,
    30-pixel nominal cells, a 3-pixel frame inside each cell window."""
    min_b, max_bx, max_by = 16, w - 16, h - 16
    ncols, nrows = (max_bx - min_b) // 30, (max_by - min_b) // 30
    wc, hc = -(-(max_bx - min_b) // ncols), -(-(max_by - min_b) // nrows)
    cells = []
    for i in range(nrows):
        y0 = min_b + i * hc
        for j in range(ncols):
            x0 = min_b + j * wc
            if y0 >= max_by - 3 or x0 >= max_bx - 6:
                continue
            x1, y1 = min(x0 + wc + 6, max_bx), min(y0 + hc + 6, max_by)
            cells.append((x0 + 3, y0 + 3, x1 - 3, y1 - 3))
    return cells


def _strict_max(mc):
    """mc > each of its 8 neighbours, with zeros outside the region"""
    p = np.pad(mc, 1)
    hh, ww = mc.shape
    nb = [p[1 + dy:1 + dy + hh, 1 + dx:1 + dx + ww]
          for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)]
    return mc > np.stack(nb).max(axis=0)


def _assert_branches(img):
    m = _fast_score(img)
    dense = fallback = tied_cell = tie = False
    for x0, y0, x1, y1 in _level0_cells(img.shape[1], img.shape[0]):
        mc = m[y0:y1, x0:x1]
        if mc.size == 0:
            continue
        lmax = _strict_max(mc)
        n21 = int((mc >= 21).sum())
        max21, max8 = bool((lmax & (mc >= 21)).any()), bool((lmax & (mc >= 8)).any())
        dense |= n21 > 64
        fallback |= n21 == 0 and max8
        tied_cell |= n21 > 0 and not max21 and max8
        p = np.pad(mc, 1)
        hh, ww = mc.shape
        for dx, dy in ((1, 0), (0, 1), (1, 1), (-1, 1)):
            tie |= bool(((mc >= 21) & (mc == p[1 + dy:1 + dy + hh, 1 + dx:1 + dx + ww])).any())
    assert dense, "no cell with more than 64 pixels at iniThFAST"
    assert fallback, "no cell that falls back without a pixel at iniThFAST"
    assert tied_cell, "no cell with pixels at iniThFAST, none a strict maximum, and a corner at 8"
    assert tie, "no tied neighbour pair at iniThFAST"


@functools.lru_cache(maxsize=None)
def _image(synth):
    img = _branch_image(synth)
    img.setflags(write=False)
    return img


def _check_against_oracle(orbpl, oracle, img, pp):
    h, w = img.shape
    nf, sf, nl, ini, mn = pp
    ex = orbpl.ORBextractor(nf, sf, nl, ini, mn, width=w, height=h)
    kps, desc = ex(img)
    p = oracle.params(*pp)
    gc = ex.candidates()
    oc = oracle.candidates(p, img)
    for l in range(nl):
        assert np.array_equal(gc[l], oc[l]), f"FAST candidates level {l} differ"
    okps, odesc, _ = oracle.extract(p, img)
    assert len(okps) > 0
    assert _kp_equal(kps, okps)
    assert np.array_equal(desc, odesc)


def test_branch_image_matches_oracle(orbpl, oracle, synth):
    img = _image(synth)
    _assert_branches(img)
    _check_against_oracle(orbpl, oracle, img, PP)


def test_high_thresholds_fall_back(orbpl, oracle, synth):
    """(60, 7): most cells have no corner at iniThFAST and take the dense pass"""
    _check_against_oracle(orbpl, oracle, _image(synth), (500, 1.2, 8, 60, 7))


def test_batch_odd_detection_width(orbpl, oracle, synth):
    """Two different frames in one batch, 322 wide: level 0's cells are 33
    pixels wide, so the last column pair of a row has no right pixel."""
    w = 322
    cells = _level0_cells(w, H)
    assert (cells[0][2] - cells[0][0]) % 2 == 1
    imgs = np.stack([_branch_image(synth, 42, w), _branch_image(synth, 43, w)])
    ex1 = orbpl.ORBextractor(*PP, width=w, height=H)
    singles = [ex1(imgs[i]) for i in range(2)]
    for i in range(2):
        okps, odesc, _ = oracle.extract(oracle.params(*PP), imgs[i])
        assert _kp_equal(singles[i][0], okps) and np.array_equal(singles[i][1], odesc)
    exb = orbpl.ORBextractor(*PP, width=w, height=H, max_batch=2)
    cap = exb.max_keypoints
    d_img = orbpl.DeviceBuffer.from_array(imgs)
    d_kps = orbpl.DeviceBuffer(2 * cap * 28)
    d_desc = orbpl.DeviceBuffer(2 * cap * 32)
    d_n = orbpl.DeviceBuffer(2 * 4)
    exb.extract_batch_device(d_img.ptr, 2, w, w * H, d_kps.ptr, d_desc.ptr, cap, d_n.ptr)
    exb.synchronize()
    n = d_n.download(np.int32, 2)
    kraw = d_kps.download(orbpl.KP_DTYPE, (2, cap))
    dd = d_desc.download(np.uint8, (2, cap, 32))
    for i in range(2):
        assert _kp_equal(kraw[i, :n[i]], singles[i][0])
        assert np.array_equal(dd[i, :n[i]], singles[i][1])


def test_one_wave_octree_override(orbpl, oracle, synth, monkeypatch):
    """ORBPL_OCT_WAVE_FROM=0 at creation: every level's octree runs as one-wave
    workgroups (off by default); keypoints and descriptors stay bit-exact."""
    monkeypatch.setenv("ORBPL_OCT_WAVE_FROM", "0")
    img = _image(synth)
    ex = orbpl.ORBextractor(*PP, width=W, height=H)
    kps, desc = ex(img)
    okps, odesc, _ = oracle.extract(oracle.params(*PP), img)
    assert _kp_equal(kps, okps)
    assert np.array_equal(desc, odesc)
