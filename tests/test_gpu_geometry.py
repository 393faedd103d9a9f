"""GPU parity of the ORB extractor and the LSD / LineExtractor kernels against
the CPU oracle at geometries off the 640x480 / 1.2 / 8-level default: odd and
tiny sizes, portrait and strip frames, 1 to 16 levels, scale factors 1.05 to
2.0, levels without FAST cells, unaligned sources and row bands at odd sizes.
Bit-exact, stage by stage."""
import numpy as np
import pytest

import _geometry_cases as G

pytestmark = pytest.mark.gpu


def _extractor(orbpl, pp, w, h, batch=1):
    nf, sf, nl, ini, mn = pp
    return orbpl.ORBextractor(nf, sf, nl, ini, mn, width=w, height=h, max_batch=batch)


def _kp_diff(a, b):
    """Name of the first keypoint field whose bit patterns differ, or None."""
    if len(a) != len(b):
        return f"count {len(a)} != {len(b)}"
    for f in ("x", "y", "size", "angle", "response"):
        if not np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)):
            return f
    for f in ("octave", "class_id"):
        if not np.array_equal(a[f], b[f]):
            return f
    return None


def _where(g, o):
    """First differing (row, column) and the number of differing bytes."""
    if g.shape != o.shape:
        return f"shape {g.shape} != {o.shape}"
    d = np.argwhere(g != o)
    return f"{len(d)} bytes, first at row {d[0][0]} column {d[0][1]}" if len(d) else "equal"


@pytest.mark.parametrize("c", G.ORB_CASES, ids=G.orb_case_id)
def test_orb_stage_parity(c, orbpl, oracle, synth):
    pp = G.orb_params(c)
    img = synth.textured_image(c.w, c.h, seed=G.ORB_SEED)
    p = oracle.params(*pp)
    okps, odesc, ocnt = oracle.extract(p, img, cap=2 * c.nfeatures + 1024)
    G.check_level_population(c, ocnt)
    ex = _extractor(orbpl, pp, c.w, c.h)      # a refusal here fails the test
    kps, desc = ex(img)
    opyr = oracle.pyramid(p, img)
    oblur = oracle.pyramid(p, img, blurred=True)
    for l in range(c.levels):
        g = ex.pyramid_level(l, padded=True)
        assert np.array_equal(g, opyr[l]), f"pyramid level {l}: {_where(g, opyr[l])}"
    for l in range(c.levels):
        gb = ex.pyramid_level(l, blurred=True)
        ob = oblur[l][19:-19, 19:-19]
        assert np.array_equal(gb, ob), f"blur level {l}: {_where(gb, ob)}"
    gc = ex.candidates()
    oc = oracle.candidates(p, img)
    for l in range(c.levels):
        assert np.array_equal(gc[l].view(np.uint32), oc[l].view(np.uint32)), \
            f"FAST candidates level {l}: gpu {len(gc[l])} oracle {len(oc[l])}"
    gcnt = np.bincount(kps["octave"], minlength=c.levels)
    assert gcnt.tolist() == [int(x) for x in ocnt], "keypoints per level"
    assert _kp_diff(kps, okps) is None, _kp_diff(kps, okps)
    if len(okps) == 0:
        assert desc is None
    else:
        assert np.array_equal(desc, odesc), \
            f"{int((desc != odesc).any(axis=1).sum())} descriptor rows differ"


# --- unaligned sources ---------------------------------------------------------
ROI_W, ROI_H, ROI_PITCH = 641, 479, 761
ROI_PP = (1000, 1.2, 8, 20, 7)


def _roi_parent(synth, seed):
    big = synth.textured_image(ROI_PITCH, 560, seed=seed)
    return big, big[51:51 + ROI_H, 41:41 + ROI_W]


def test_orb_unaligned_host_roi(orbpl, oracle, synth):
    """A cv::Mat ROI with an odd column offset and an odd row pitch through
    the host entry: the same bytes as its contiguous copy and as the oracle."""
    big, roi = _roi_parent(synth, 40)
    assert roi.shape == (ROI_H, ROI_W) and roi.strides == (ROI_PITCH, 1)
    assert not roi.flags["C_CONTIGUOUS"]
    assert (roi.ctypes.data - big.ctypes.data) % ROI_PITCH == 41
    ex = _extractor(orbpl, ROI_PP, ROI_W, ROI_H)
    kv, dv = ex(roi)
    pyr_v = [ex.pyramid_level(l, padded=True) for l in range(8)]
    kc, dc = ex(np.ascontiguousarray(roi))
    okps, odesc, _ = oracle.extract(oracle.params(*ROI_PP), np.ascontiguousarray(roi))
    for l in range(8):
        assert np.array_equal(pyr_v[l], ex.pyramid_level(l, padded=True)), f"pyramid level {l}"
    assert len(okps) > 500
    assert _kp_diff(kv, kc) is None and np.array_equal(dv, dc)
    assert _kp_diff(kv, okps) is None and np.array_equal(dv, odesc)


def _batch_device(orbpl, exb, d_ptr, B, stride, frame_pitch):
    cap = exb.max_keypoints
    d_kps = orbpl.DeviceBuffer(B * cap * 28)
    d_desc = orbpl.DeviceBuffer(B * cap * 32)
    d_n = orbpl.DeviceBuffer(B * 4)
    d_n.zero()
    exb.extract_batch_device(d_ptr, B, stride, frame_pitch, d_kps.ptr, d_desc.ptr, cap, d_n.ptr)
    exb.synchronize()
    n = d_n.download(np.int32, B)
    kraw = d_kps.download(orbpl.KP_DTYPE, (B, cap))
    dd = d_desc.download(np.uint8, (B, cap, 32))
    return [(kraw[i, :n[i]], dd[i, :n[i]]) for i in range(B)]


def test_orb_unaligned_device_batch(orbpl, synth):
    """extract_batch_device on a device pointer at an odd address, an odd row
    pitch (761) and a frame pitch that is no multiple of 16: three different
    frames, each equal to its single-frame extraction."""
    B = 3
    frame_pitch = ROI_PITCH * ROI_H + 6
    assert frame_pitch % 16 != 0 and frame_pitch % 2 == 1   # frames at odd and even addresses
    frames = [synth.textured_image(ROI_W, ROI_H, seed=41 + i) for i in range(B)]
    host = np.zeros(1 + B * frame_pitch + ROI_PITCH, np.uint8)
    for i, fr in enumerate(frames):
        rows = np.lib.stride_tricks.as_strided(host[1 + i * frame_pitch:], (ROI_H, ROI_W),
                                               (ROI_PITCH, 1))
        rows[:] = fr
    # the last byte read is 1 + (B - 1) frame_pitch + (H - 1) pitch + W - 1 < host.size
    assert 1 + (B - 1) * frame_pitch + (ROI_H - 1) * ROI_PITCH + ROI_W <= host.size
    d_img = orbpl.DeviceBuffer.from_array(host)
    ex1 = _extractor(orbpl, ROI_PP, ROI_W, ROI_H)
    singles, pyramids = [], []
    for fr in frames:
        singles.append(ex1(fr))
        pyramids.append([ex1.pyramid_level(l, padded=True) for l in range(8)])
    exb = _extractor(orbpl, ROI_PP, ROI_W, ROI_H, batch=B)
    out = _batch_device(orbpl, exb, d_img.ptr + 1, B, ROI_PITCH, frame_pitch)
    for i in range(B):
        for l in range(8):
            assert np.array_equal(exb.pyramid_level(l, padded=True, frame=i), pyramids[i][l]), \
                (i, l, "pyramid")
        assert len(singles[i][0]) > 500
        assert _kp_diff(out[i][0], singles[i][0]) is None, (i, _kp_diff(out[i][0], singles[i][0]))
        assert np.array_equal(out[i][1], singles[i][1]), i


# --- batch and row bands at odd sizes --------------------------------------------
BAND_CASES = [c for c in G.ORB_CASES if (c.w, c.h) in ((641, 479), (125, 93), (72, 72))]


@pytest.mark.parametrize("bands", ["1", "8"], ids=["bands_1", "bands_8"])
@pytest.mark.parametrize("c", BAND_CASES, ids=G.orb_case_id)
def test_orb_batch_row_bands(c, bands, orbpl, oracle, synth, monkeypatch):
    """A batch of 4 through extract_batch_device with the pyramid's row bands
    per frame forced to 1 and to 8 (ORBPL_PYR_BANDS, read at create; 8 is
    also what a batch this small gets by default): band edges fall on the
    levels without FAST cells and on the 20 px level. Byte for byte the
    single-frame extraction and the oracle."""
    monkeypatch.setenv("ORBPL_PYR_BANDS", bands)
    B = 4
    pp = G.orb_params(c)
    imgs = np.stack([synth.textured_image(c.w, c.h, seed=G.ORB_SEED + i) for i in range(B)])
    exb = _extractor(orbpl, pp, c.w, c.h, batch=B)
    d_img = orbpl.DeviceBuffer.from_array(imgs)
    out = _batch_device(orbpl, exb, d_img.ptr, B, c.w, c.w * c.h)
    monkeypatch.delenv("ORBPL_PYR_BANDS", raising=False)
    ex1 = _extractor(orbpl, pp, c.w, c.h)
    p = oracle.params(*pp)
    for i in range(B):
        kp, de = ex1(imgs[i])
        okps, odesc, _ = oracle.extract(p, imgs[i])
        assert len(okps) > 0 and _kp_diff(kp, okps) is None
        for l in range(c.levels):
            assert np.array_equal(exb.pyramid_level(l, padded=True, frame=i),
                                  ex1.pyramid_level(l, padded=True)), (i, l, "pyramid")
            assert np.array_equal(exb.pyramid_level(l, blurred=True, frame=i),
                                  ex1.pyramid_level(l, blurred=True)), (i, l, "blur")
        assert _kp_diff(out[i][0], kp) is None, (i, _kp_diff(out[i][0], kp))
        assert np.array_equal(out[i][1], de), i


PIPE_CASES = [c for c in G.ORB_CASES
              if (c.w, c.h, c.scale, c.levels, c.nfeatures, c.ini_th) in (
                  (125, 93, 1.2, 8, 300, 20), (321, 243, 2.0, 4, 500, 20),
                  (321, 243, 1.05, 16, 500, 20), (321, 243, 1.2, 1, 500, 20))]


@pytest.mark.parametrize("c", PIPE_CASES, ids=G.orb_case_id)
def test_orb_level_pipeline_geometries(c, orbpl, synth, monkeypatch):
    """The level pipeline (ORBPL_LEVEL_PIPE=1, a batch of 64: one pyramid, FAST
    and octree launch per level group) where its default groups [0,1) [1,2)
    [2,3) [3,n) meet levels without FAST cells, 4, 16 and a single level:
    every frame equals its single-frame extraction."""
    B, U = 64, 4
    pp = G.orb_params(c)
    uniq = [synth.textured_image(c.w, c.h, seed=G.ORB_SEED + i) for i in range(U)]
    monkeypatch.setenv("ORBPL_LEVEL_PIPE", "0")
    ex1 = _extractor(orbpl, pp, c.w, c.h)
    singles = [ex1(u) for u in uniq]
    monkeypatch.setenv("ORBPL_LEVEL_PIPE", "1")
    exb = _extractor(orbpl, pp, c.w, c.h, batch=B)
    d_img = orbpl.DeviceBuffer.from_array(np.stack([uniq[i % U] for i in range(B)]))
    for rep in range(2):   # the second batch reuses the group events and streams
        out = _batch_device(orbpl, exb, d_img.ptr, B, c.w, c.w * c.h)
        for i in range(B):
            kp, de = singles[i % U]
            assert len(kp) > 0
            assert _kp_diff(out[i][0], kp) is None, (rep, i, _kp_diff(out[i][0], kp))
            assert np.array_equal(out[i][1], de), (rep, i)


# --- LSD and LineExtractor sizes -------------------------------------------------
def _check_lsd_stages(det, oracle, img):
    scaled, deg, order = det.stages(0)
    s_o, ang_o, ord_o = oracle.lsd_stages(img)
    assert np.array_equal(scaled, s_o), f"scaled image: {_where(scaled, s_o)}"
    notdef = ang_o == -1024.0
    assert np.array_equal(deg < 0, notdef), "undefined angles"
    a = deg.astype(np.float64) * (np.pi / 180)
    assert np.array_equal(a[~notdef], ang_o[~notdef]), "angles"
    # the ordered list up to its last defined pixel is the reference's
    # std::sort order; the tail holds only undefined pixels (same elements)
    defined = ~notdef[ord_o >> 16, ord_o & 0xFFFF]
    last = int(np.nonzero(defined)[0].max()) + 1 if defined.any() else 0
    assert np.array_equal(order[:last], ord_o[:last]), "pixel order"
    assert np.array_equal(np.sort(order), np.sort(ord_o)), "pixel order elements"


def _cmp_keylines(kl, desc, coef, kl_o, desc_o, coef_o):
    assert len(kl) == len(kl_o), (len(kl), len(kl_o))
    assert len(kl.dtype.names) == 17
    for name in kl.dtype.names:
        assert np.array_equal(kl[name].view(np.uint32), kl_o[name].view(np.uint32)), name
    assert np.array_equal(desc, desc_o), "LBD rows"
    assert np.array_equal(coef.view(np.uint64), coef_o.view(np.uint64)), "coefficients"


@pytest.mark.parametrize("s", G.LSD_SIZES, ids=G.lsd_size_id)
def test_lsd_and_line_extract_sizes(s, orbpl, oracle, synth):
    """Scaled image, angles, pixel order, segments, the 17 KeyLine fields, LBD
    rows and coefficients at each size; both seed loops where listed. A frame
    without segments gives none, with no capacity or overflow code (detect
    and ExtractLineSegment raise on either)."""
    w, h, source, fewest = s
    img = G.lsd_image(synth, w, h, source)
    Lo = oracle.lsd_detect(img)
    assert len(Lo) == 0 if fewest == 0 else len(Lo) >= fewest
    ex = orbpl.LineExtractor(w, h)
    loops = (False, True) if (w, h) in G.LSD_BOTH_LOOPS else (False,)
    for serial in loops:
        ex.set_serial_grow(serial)
        L = ex.detect(img)
        _check_lsd_stages(ex, oracle, img)
        assert len(L) == len(Lo), (serial, len(L), len(Lo))
        assert np.array_equal(L.view(np.uint32), Lo.view(np.uint32)), (serial, "segments")
        kl, desc, coef = ex.ExtractLineSegment(img)
        kl_o, desc_o, coef_o, nd = oracle.line_extract(img)
        assert nd == len(Lo) and len(kl_o) == min(nd, 80)
        _cmp_keylines(kl, desc, coef, kl_o, desc_o, coef_o)


FALLBACK_SIZES = [s for s in G.LSD_SIZES
                  if (s[0], s[1], s[2]) in ((641, 479, "textured"), (97, 67, "polygons"),
                                            (16, 16, "polygons"))]


@pytest.mark.parametrize("s", FALLBACK_SIZES, ids=G.lsd_size_id)
def test_lsd_unfused_paths_sizes(s, orbpl, oracle, synth, monkeypatch):
    """The three-kernel LSD front (ORBPL_LSD_PREP=0 at create) and the
    separate 5x5 blur and Sobel kernels of the LBD (ORBPL_BLUR_SOBEL=0), the
    paths a geometry falls back to, at an odd, a small and the minimum size."""
    monkeypatch.setenv("ORBPL_LSD_PREP", "0")
    monkeypatch.setenv("ORBPL_BLUR_SOBEL", "0")
    w, h, source, fewest = s
    img = G.lsd_image(synth, w, h, source)
    ex = orbpl.LineExtractor(w, h)
    L = ex.detect(img)
    _check_lsd_stages(ex, oracle, img)
    Lo = oracle.lsd_detect(img)
    assert len(Lo) >= fewest > 0
    assert np.array_equal(L.view(np.uint32), Lo.view(np.uint32)), "segments"
    kl_o, desc_o, coef_o, nd = oracle.line_extract(img)
    _cmp_keylines(*ex.ExtractLineSegment(img), kl_o, desc_o, coef_o)


def test_line_extract_unaligned_device_batch(orbpl, oracle):
    """extract_batch_device of the line extractor on a device pointer at an
    odd address with an odd row pitch and an odd frame pitch, at an odd size:
    three different frames, each equal to the oracle."""
    w, h, pitch, B = 161, 123, 171, 3
    frame_pitch = pitch * h + 6
    assert frame_pitch % 2 == 1
    frames = [G.polygon_image(w, h, G.LSD_SEED + i) for i in range(B)]
    host = np.zeros(1 + B * frame_pitch + pitch, np.uint8)
    for i, fr in enumerate(frames):
        rows = np.lib.stride_tricks.as_strided(host[1 + i * frame_pitch:], (h, w), (pitch, 1))
        rows[:] = fr
    assert 1 + (B - 1) * frame_pitch + (h - 1) * pitch + w <= host.size
    d_img = orbpl.DeviceBuffer.from_array(host)
    ex = orbpl.LineExtractor(w, h, max_batch=B)
    ex.extract_batch_device(d_img.ptr + 1, B, stride=pitch, frame_pitch=frame_pitch)
    ex.synchronize()
    for i, fr in enumerate(frames):
        Lo = oracle.lsd_detect(fr)
        assert len(Lo) >= 10
        assert np.array_equal(ex.lines(i).view(np.uint32), Lo.view(np.uint32)), i
        kl_o, desc_o, coef_o, nd = oracle.line_extract(fr)
        _cmp_keylines(*ex.keylines(i), kl_o, desc_o, coef_o)


WIDE_PITCH = 65536 + 41    # a row pitch that does not fit 16 bits


def _wide_pitch_buffer(orbpl, frame):
    h, w = frame.shape
    host = np.zeros((h - 1) * WIDE_PITCH + w, np.uint8)
    np.lib.stride_tricks.as_strided(host, (h, w), (WIDE_PITCH, 1))[:] = frame
    return orbpl.DeviceBuffer.from_array(host)


def test_line_extract_row_pitch_above_16_bits(orbpl, oracle):
    """A frame inside a device image whose row pitch is above 65535 bytes (a
    narrow ROI of a very wide buffer): the entry takes any stride >= width,
    and the result must not depend on it."""
    w, h = 97, 67
    fr = G.polygon_image(w, h, G.LSD_SEED)
    d_img = _wide_pitch_buffer(orbpl, fr)
    ex = orbpl.LineExtractor(w, h)
    ex.extract_batch_device(d_img.ptr, 1, stride=WIDE_PITCH, frame_pitch=0)
    ex.synchronize()
    _check_lsd_stages(ex, oracle, fr)
    Lo = oracle.lsd_detect(fr)
    assert len(Lo) >= 1
    assert np.array_equal(ex.lines(0).view(np.uint32), Lo.view(np.uint32))
    kl_o, desc_o, coef_o, nd = oracle.line_extract(fr)
    _cmp_keylines(*ex.keylines(0), kl_o, desc_o, coef_o)


def test_orb_row_pitch_above_16_bits(orbpl, oracle, synth):
    c = next(c for c in G.ORB_CASES if (c.w, c.h) == (125, 93))
    img = synth.textured_image(c.w, c.h, seed=G.ORB_SEED)
    d_img = _wide_pitch_buffer(orbpl, img)
    exb = _extractor(orbpl, G.orb_params(c), c.w, c.h)
    (kps, desc), = _batch_device(orbpl, exb, d_img.ptr, 1, WIDE_PITCH, 0)
    okps, odesc, _ = oracle.extract(oracle.params(*G.orb_params(c)), img)
    assert len(okps) > 0 and _kp_diff(kps, okps) is None, _kp_diff(kps, okps)
    assert np.array_equal(desc, odesc)


def test_line_extract_unaligned_roi(orbpl, oracle, synth):
    """ExtractLineSegment on a view with an odd column offset and an odd row
    pitch equals its contiguous copy and the oracle."""
    big, roi = _roi_parent(synth, 40)
    ex = orbpl.LineExtractor(ROI_W, ROI_H)
    out_v = ex.ExtractLineSegment(roi)
    out_c = ex.ExtractLineSegment(np.ascontiguousarray(roi))
    kl_o, desc_o, coef_o, nd = oracle.line_extract(np.ascontiguousarray(roi))
    assert nd > 80
    _cmp_keylines(*out_v, *out_c)
    _cmp_keylines(*out_v, kl_o, desc_o, coef_o)
