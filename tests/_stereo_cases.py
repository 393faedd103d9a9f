"""Hand-made inputs for Frame::ComputeStereoMatches, shared by
test_stereo_ref.py (CPU: restatement against oracle, reason codes) and
test_gpu_stereo.py (GPU: orbpl.stereo_matches against the oracle).

Directed cases: a tiny frame whose level 0 is the source image, hand-placed
keypoints, descriptors at chosen Hamming distances and image strips with a
chosen SAD curve. A case names, per left keypoint, the reason code
(_stereo_ref) the keypoint was made for, before the median cut (`stage`) or
after it (`reason`), and values of the restatement's trace (`trace`).

Shifted pairs: a textured image and the same image moved by an integer
disparity per row band plus noise, keypoints from the oracle's extractor, at
pyramids off the 1.2 / 8-level default."""
import functools
from collections import namedtuple

import numpy as np

import _stereo_ref as R
from _pkg import load_oracle, load_pkg

Case = namedtuple("Case", "name w h levels factor fx bf left right kl dl kr dr stage reason trace")

W0, H0 = 125, 93          # _geometry_cases: levels 3..7 of 1.2 / 8 hold no FAST cell


def cfg_of(c):
    """Camera settings of a case (what synth / oracle.camera / make_camera read)."""
    return dict(fx=c.fx, fy=c.fx, cx=c.w / 2.0, cy=c.h / 2.0, k1=0.0, k2=0.0, p1=0.0, p2=0.0,
                k3=0.0, width=c.w, height=c.h, bf=c.bf, thdepth=35.0, depth_factor=1.0)


def orb_of(c):
    return (300, c.factor, c.levels, 20, 7)


def code(i):
    """256-bit codeword i (1..255) of the Hadamard code: any two differ in
    exactly 128 bits, so a foreign right keypoint is never under TH_HIGH."""
    assert 1 <= i <= 255
    j = np.arange(256)
    bits = np.array([bin(i & int(x)).count("1") & 1 for x in j], np.uint8)
    return np.packbits(bits)


def flip(desc, nbits, start=0):
    """desc with bits start .. start + nbits - 1 inverted: Hamming distance nbits."""
    bits = np.unpackbits(desc)
    bits[start:start + nbits] ^= 1
    return np.packbits(bits)


# the default SAD curve: smallest at incR = 0, symmetric (deltaR = 0)
V_CURVE = (500, 400, 300, 200, 100, 20, 100, 200, 300, 400, 500)


def v_curve(best):
    return tuple(best + 80 * abs(k - 5) for k in range(11))


class Builder:
    """Left image flat (every centred left window is zero), right image zero
    with painted strips: the SAD at shift k is the sum of the painted pixels
    under the window, which `curve` solves for a wanted list of 11 SADs."""

    def __init__(self, name, w=W0, h=H0, levels=8, factor=1.2, fx=32.0, bf=8.0):
        self.name, self.w, self.h, self.levels, self.factor = name, w, h, levels, factor
        self.fx, self.bf = fx, bf          # maxD = bf / (bf / fx) = fx for powers of two
        self.left = np.full((h, w), 128, np.uint8)
        self.right = np.zeros((h, w), np.uint8)
        self.kl, self.dl, self.kr, self.dr = [], [], [], []
        self.stage, self.reason, self.trace = {}, {}, {}
        self._code = 0
        self._slot = 0

    def new_code(self):
        self._code += 1
        return code(self._code)

    def slot(self):
        """Centre (cuR, cv) of the next free 21 x 11 strip of the right image."""
        per_row = (self.w - 3) // 22
        i, j = self._slot % per_row, self._slot // per_row
        self._slot += 1
        cu, cv = 11 + 22 * i, 6 + 12 * j
        assert cv + 5 < self.h, "no strip left"
        return cu, cv

    def L(self, x, y, octave=0, desc=None, stage=None, reason=None, **trace):
        self.kl.append((x, y, octave))
        self.dl.append(self.new_code() if desc is None else desc)
        i = len(self.kl) - 1
        if stage is not None:
            self.stage[i] = stage
        if reason is not None:
            self.reason[i] = reason
        if trace:
            self.trace[i] = trace
        return i

    def Rk(self, x, y, octave=0, desc=None):
        self.kr.append((x, y, octave))
        self.dr.append(np.full(32, 0xFF, np.uint8) if desc is None else desc)
        return len(self.kr) - 1

    def curve(self, cu, cv, sads):
        """Paint the right strip centred (cu, cv) so that the SAD of a flat
        left window against the window centred cu - 5 + k is sads[k]."""
        assert len(sads) == 11
        # column sums A[0..20] with sum(A[k .. k + 10]) == sads[k]: A[k + 11] = A[k] +
        # sads[k + 1] - sads[k]; A[k] starts at the drop it has to pay for, A[10] takes the rest
        A = [max(0, sads[k] - sads[k + 1]) for k in range(10)]
        A.append(sads[0] - sum(A))
        for k in range(10):
            A.append(A[k] + sads[k + 1] - sads[k])
        rows = [cv + d for d in (-5, -4, -3, -2, -1, 1, 2, 3, 4, 5)]   # the centre row stays 0
        for j, a in enumerate(A):
            assert 0 <= a <= 255 * len(rows), (sads, A)
            for r in rows:
                v = min(255, a)
                self.right[r, cu - 10 + j] = v
                a -= v

    def pair(self, d=8.0, sads=V_CURVE, dist=0, stage=R.ACCEPTED, reason=None, **trace):
        """A left keypoint, its right keypoint d pixels to the left at Hamming
        distance `dist`, on a strip of their own with the given SAD curve."""
        cu, cv = self.slot()
        c = self.new_code()
        if sads is not None:
            self.curve(cu, cv, sads)
        iR = self.Rk(float(cu), float(cv), 0, flip(c, dist))
        iL = self.L(float(cu) + d, float(cv), 0, c, stage, reason, **trace)
        return iL, iR

    def done(self):
        O = load_oracle()
        def kps(lst):
            k = np.zeros(len(lst), O.KP_DTYPE)
            for i, (x, y, o) in enumerate(lst):
                k["x"][i], k["y"][i], k["octave"][i] = x, y, o
                k["size"][i], k["angle"][i], k["response"][i] = 31.0, 0.0, 20.0
            return k
        def desc(lst):
            return np.ascontiguousarray(np.stack(lst) if lst else np.zeros((0, 32)), np.uint8)
        return Case(self.name, self.w, self.h, self.levels, self.factor, self.fx, self.bf,
                    self.left, self.right, kps(self.kl), desc(self.dl), kps(self.kr), desc(self.dr),
                    self.stage, self.reason, self.trace)


def up(x):
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


def down(x):
    return float(np.nextafter(np.float32(x), np.float32(-np.inf)))


# ---------------------------------------------------------------------------
def case_row_bands():
    """Row-band membership: radius 2 * scale[octave], floor / ceil of the band
    ends, the first and last image row, (int)vL of a negative vL."""
    b = Builder("row_bands")
    # right keypoint, then probes (vL, in band?) with the same codeword, 4 px of disparity
    def probe(xr, yr, octave, probes, level=None):
        c = b.new_code()
        iR = b.Rk(xr, yr, octave, c)
        for vL, inside, *st in probes:
            if inside:
                b.L(xr + 4.0, vL, octave if level is None else level, c, st[0] if st else None,
                    best_idx=iR)
            else:
                b.L(xr + 4.0, vL, octave if level is None else level, c, st[0])
        return iR
    # y = 0: rows -2 .. 2, cut to 0 .. 2; vL = -0.5 truncates to row 0 and rounds to -1
    probe(20.0, 0.0, 0, [(0.0, True, R.WINDOW_OUTSIDE), (2.0, True), (2.9, True),
                         (-0.5, True, R.WINDOW_OUTSIDE), (-0.99, True, R.WINDOW_OUTSIDE),
                         (-1.0, False, R.ROW_OUTSIDE)])
    # y = 0.4: floor(-1.6) .. ceil(2.4) = -2 .. 3
    probe(50.0, 0.4, 0, [(3.5, True), (4.0, False, R.EMPTY_BAND)])
    # y = H - 1: rows 90 .. 94, cut to 90 .. 92
    probe(20.0, 92.0, 0, [(92.0, True, R.WINDOW_OUTSIDE), (92.99, True, R.WINDOW_OUTSIDE),
                          (90.0, True, R.WINDOW_OUTSIDE), (93.0, False, R.ROW_OUTSIDE)])
    # y = 91.7: floor(89.7) .. ceil(93.7) = 89 .. 94
    probe(50.0, 91.7, 0, [(89.0, True), (88.99, False, R.EMPTY_BAND)])
    # y = 40.5: floor(38.5) .. ceil(42.5) = 38 .. 43, seen from its first and last row
    probe(20.0, 40.5, 0, [(38.0, True), (43.99, True), (37.99, False, R.EMPTY_BAND),
                          (44.0, False, R.EMPTY_BAND)])
    # octave 3: radius 2 * 1.728 = 3.456: floor(56.544) .. ceil(63.456) = 56 .. 64
    probe(60.0, 60.0, 3, [(56.0, True), (64.9, True), (55.99, False, R.EMPTY_BAND),
                          (65.0, False, R.EMPTY_BAND)])
    # octave 7: radius 2 * 3.583 = 7.166: floor(12.83) .. ceil(27.17) = 12 .. 28
    probe(90.0, 20.0, 7, [(12.0, True), (28.5, True), (11.9, False, R.EMPTY_BAND),
                          (29.0, False, R.EMPTY_BAND)], level=6)
    return b.done()


def case_octave_gate():
    """Right octaves levelL - 2, - 1, + 1, + 2: the two outer ones are passed
    over although they are the closest descriptors."""
    b = Builder("octave_gate")
    c = b.new_code()
    b.Rk(56.0, 30.0, 0, c)                       # levelL - 2, distance 0
    b.Rk(56.0, 30.0, 4, flip(c, 1))              # levelL + 2, distance 1
    b.Rk(56.0, 30.0, 1, flip(c, 20))             # levelL - 1
    best = b.Rk(56.0, 30.0, 3, flip(c, 10))      # levelL + 1: chosen
    b.L(60.0, 30.0, 2, c, best_idx=best, best_dist=10)
    c = b.new_code()
    b.Rk(56.0, 60.0, 0, c)
    b.Rk(56.0, 60.0, 4, c)
    b.L(60.0, 60.0, 2, c, R.NO_CANDIDATE)        # a band with entries, none admitted
    c = b.new_code()
    lo = b.Rk(56.0, 80.0, 0, flip(c, 5))
    b.Rk(56.0, 80.0, 1, flip(c, 5))
    b.L(60.0, 80.0, 0, c, best_idx=lo, best_dist=5)     # levelL = 0: octaves 0 and 1 only
    b.L(60.0, 80.0, 7, c, R.NO_CANDIDATE)               # levelL = 7: octaves 6 and 7 only
    return b.done()


def case_disparity_window():
    """uR exactly minU and maxU and one float step beyond; a disparity of
    exactly 0 (clamped), one float step of uL below maxD (the largest float
    below maxD is case_disparity_below_max's), exactly maxD, negative.
    fx = 16: maxD = 16."""
    b = Builder("disparity_window", fx=16.0, bf=8.0)
    # one strip per keypoint, painted where its right keypoint rounds to
    rows = [6 + 12 * j for j in range(7)]
    def at_row(j, uL, uR, stage, sads=V_CURVE, **trace):
        cv = rows[j]
        c = b.new_code()
        b.curve(int(R.std_round(uR)), cv, sads)
        b.Rk(uR, float(cv), 0, c)
        return b.L(uL, float(cv), 0, c, stage, **trace)
    at_row(0, 48.0, 32.0, R.DISPARITY_MAX, disparity=np.float32(16.0))      # uR == minU, d == maxD
    at_row(0, 100.0, down(84.0), R.NO_CANDIDATE)                             # one step below minU
    at_row(1, down(32.0), 16.0, R.ACCEPTED, disparity=np.float32(32.0) - np.float32(16.0)
           - np.float32(2.0 ** -19))                                        # one step of uL below
    at_row(1, 90.0, 90.0, R.ACCEPTED_CLAMPED, disparity=np.float32(0.0))     # uR == maxU, d == 0
    at_row(2, 40.0, up(40.0), R.NO_CANDIDATE)                                # one step above maxU
    # the SAD minimum 3 columns right of a right keypoint 1 px away: d = -2
    at_row(2, 91.0, 90.0, R.DISPARITY_NEGATIVE, sads=tuple(20 + 80 * abs(k - 8) for k in range(11)),
           inc=3, disparity=np.float32(-2.0))
    # maxU < 0: a left keypoint left of the image
    c = b.new_code()
    b.Rk(-3.0, float(rows[3]), 0, c)
    b.L(-0.5, float(rows[3]), 0, c, R.MAXU_NEGATIVE)
    # a clamped match whose uL is not an integer (deltaR = 200 / 800 puts bestuR on uL):
    # bestuR goes through (double)uL - 0.01
    at_row(4, 40.25, 40.25, R.ACCEPTED_CLAMPED, delta=np.float32(0.25),
           sads=(620, 520, 420, 370, 320, 20, 120, 200, 300, 400, 500))
    at_row(4, 90.0, 82.0, R.ACCEPTED)
    at_row(5, 40.0, 32.0, R.ACCEPTED)
    return b.done()


def case_disparity_below_max():
    """fx one float step above 16, so that maxD = bf / (bf / fx) is 16 + 2^-19:
    a disparity of 16 is the largest float below maxD and is accepted, a
    disparity of 16 + 2^-19 is exactly maxD and is not."""
    b = Builder("disparity_below_max", fx=up(16.0), bf=8.0)
    for j, (uL, uR, stage, d) in enumerate([(48.0, 32.0, R.ACCEPTED, 16.0),
                                            (up(26.0), 10.0, R.DISPARITY_MAX, up(16.0)),
                                            (70.0, 62.0, R.ACCEPTED, 8.0)]):
        cv = 6 + 12 * j
        c = b.new_code()
        b.curve(int(uR), cv, V_CURVE)
        b.Rk(uR, float(cv), 0, c)
        b.L(uL, float(cv), 0, c, stage, disparity=np.float32(d))
    return b.done()


def case_descriptor():
    """bestDist 74 kept, 75 dropped, 99 chosen and then dropped; equal
    distances: the lower right index wins."""
    b = Builder("descriptor")
    b.pair(dist=74, best_dist=74)
    b.pair(dist=75, stage=R.NO_CANDIDATE)
    b.pair(dist=99, stage=R.NO_CANDIDATE)
    b.pair(dist=100, stage=R.NO_CANDIDATE)
    b.pair(dist=0, best_dist=0)
    # two right keypoints at distance 30 (different bits), the later one nearer in x
    cu, cv = b.slot()
    c = b.new_code()
    b.curve(cu, cv, V_CURVE)
    first = b.Rk(float(cu), float(cv), 0, flip(c, 30))
    b.Rk(float(cu) + 2.0, float(cv) + 1.0, 0, flip(c, 30, 100))
    b.L(float(cu) + 8.0, float(cv), 0, c, R.ACCEPTED, best_idx=first, best_dist=30)
    # a closer descriptor later in the list replaces an earlier one
    cu, cv = b.slot()
    c = b.new_code()
    b.curve(cu, cv, V_CURVE)
    b.Rk(float(cu) + 2.0, float(cv) + 1.0, 0, flip(c, 31))
    best = b.Rk(float(cu), float(cv), 0, flip(c, 30))
    b.L(float(cu) + 8.0, float(cv), 0, c, R.ACCEPTED, best_idx=best, best_dist=30)
    return b.done()


def case_tie_order_256():
    """Ties between right indices 255 / 256 and 257 / 300: the kernel enters
    index >= 256 from a thread's second stride, in whatever order the waves
    reach their atomics (case_tie_order_bands forces the inverted order). 320
    right keypoints share the deciding rows."""
    b = Builder("tie_order_256")
    ca, cb = b.new_code(), b.new_code()
    (cu_a, cv_a), (cu_b, cv_b) = b.slot(), b.slot()
    b.curve(cu_a, cv_a, V_CURVE)
    b.curve(cu_b, cv_b, V_CURVE)
    want = {}
    for i in range(320):
        if i == 255:
            want["a"] = b.Rk(float(cu_a), float(cv_a), 0, flip(ca, 30))
        elif i == 256:
            b.Rk(float(cu_a) + 3.0, float(cv_a), 0, flip(ca, 30, 64))
        elif i == 257:
            want["b"] = b.Rk(float(cu_b), float(cv_b), 0, flip(cb, 30))
        elif i == 300:
            b.Rk(float(cu_b) + 3.0, float(cv_b), 0, flip(cb, 30, 64))
        else:
            # fillers right of every left keypoint, in the deciding rows' bands
            b.Rk(100.0 + (i % 20), float(cv_a) + (i % 3) - 1, i % 2)
    b.L(float(cu_a) + 8.0, float(cv_a), 0, ca, R.ACCEPTED, best_idx=want["a"])
    b.L(float(cu_b) + 8.0, float(cv_b), 0, cb, R.ACCEPTED, best_idx=want["b"])
    return b.done()


def case_tie_order_bands():
    """Equal distances where the lower right index enters the deciding row
    last: it sits on octave 2 of a 2.0-factor pyramid (17 rows, the deciding
    row the last of them), the higher index on octave 0 (5 rows, the deciding
    row the first). Lanes of one wave walk their bands in step, so the
    kernel's row list receives the higher index first and only its in-row
    sort restores vRowIndices' order. Textured pair, 16 px of disparity: the
    lower index is the true match, the higher one lies 24 px further left."""
    load_pkg()
    import orbpl.synth as synth
    b = Builder("tie_order_bands", w=321, h=243, levels=4, factor=2.0, fx=64.0, bf=16.0)
    img = synth.textured_image(321 + 16, 243, seed=5)
    rng = np.random.default_rng(6)
    b.left = np.ascontiguousarray(img[:, :321])
    noisy = img[:, 16:].astype(np.int32) + rng.integers(-3, 4, (243, 321))
    b.right = np.clip(noisy, 0, 255).astype(np.uint8)
    for i, (uL, yd) in enumerate([(120.0, 60.0), (160.0, 100.0), (200.0, 140.0), (240.0, 180.0),
                                  (140.0, 200.0), (180.0, 40.0)]):
        c = b.new_code()
        lo = b.Rk(uL - 16.0, yd - 8.0, 2, flip(c, 30))          # rows yd - 16 .. yd
        b.Rk(uL - 40.0, yd + 2.0, 0, flip(c, 30, 64))           # rows yd .. yd + 4
        b.L(uL, yd, 1, c, best_idx=lo, best_dist=30)
    return b.done()


def case_endu():
    """scaleduR0 + 11 == width - 1 (kept) and == width (dropped) on level 0
    (125 wide) and on level 1 (104 wide); iniu < 0. Both images flat there:
    a kept keypoint finds eleven SADs of 0 and leaves at incR = -L."""
    b = Builder("endu")
    def at(uR, y, level, stage, **trace):
        c = b.new_code()
        b.Rk(uR, y, level, c)
        b.L(uR, y, level, c, stage, **trace)
    at(113.0, 20.0, 0, R.SAD_MIN_FIRST, cuR=113)
    at(114.0, 40.0, 0, R.INIU_ENDU)
    at(110.4, 60.0, 1, R.SAD_MIN_FIRST, cuR=92)     # 110.4 / 1.2 = 92
    at(111.6, 80.0, 1, R.INIU_ENDU)                 # 111.6 / 1.2 = 93
    c = b.new_code()
    b.Rk(-1.0, 30.0, 0, c)                          # scaleduR0 = -1: iniu = -1
    b.L(3.0, 30.0, 0, c, R.INIU_ENDU)
    c = b.new_code()
    b.Rk(-0.4, 50.0, 0, c)                          # rounds to -0: iniu = 0 passes, the window not
    b.L(12.0, 50.0, 0, c, R.WINDOW_OUTSIDE, cuR=0)
    return b.done()


def case_window_skip():
    """The pinned skip: cuR in 0 .. 9, cuL within 5 of either side, cvL within
    5 of top and bottom; the first position inside on each side."""
    b = Builder("window_skip")
    def at(uL, uR, y, stage, **trace):
        c = b.new_code()
        b.Rk(uR, y, 0, c)
        b.L(uL, y, 0, c, stage, **trace)
    for k in range(10):
        at(k + 12.0, float(k), 10.0 + 8 * (k % 10), R.WINDOW_OUTSIDE, cuR=k)
    at(22.0, 10.0, 90.0 - 5.0, R.SAD_MIN_FIRST, cuR=10)       # cuR = 10, cvL = H - 6: inside
    at(4.0, 2.0, 46.0, R.WINDOW_OUTSIDE, cuL=4)
    at(120.0, 100.0, 30.0, R.WINDOW_OUTSIDE, cuL=120)
    at(119.0, 100.0, 40.0, R.SAD_MIN_FIRST, cuL=119)
    at(60.0, 50.0, 4.0, R.WINDOW_OUTSIDE, cvL=4)
    at(60.0, 50.0, 5.0, R.SAD_MIN_FIRST, cvL=5)
    at(60.0, 50.0, 87.4, R.SAD_MIN_FIRST, cvL=87)
    at(60.0, 50.0, 87.5, R.WINDOW_OUTSIDE, cvL=88)            # round half away from zero
    return b.done()


def _curve_min_at(k, best=20):
    return tuple(best + 70 * abs(j - k) for j in range(11))


def case_sad_curve():
    """Where the smallest SAD sits and what the parabola makes of it. deltaR
    lies in (-1/2, 1/2] (see _stereo_ref.UNREACHABLE): + 1/2 exactly with two
    equal neighbouring minima, towards - 1/2 with d1 = d2 + 1 and a steep d3."""
    b = Builder("sad_curve")
    b.pair(sads=_curve_min_at(0), stage=R.SAD_MIN_FIRST, inc=-5)
    b.pair(sads=_curve_min_at(10), stage=R.SAD_MIN_LAST, inc=5)
    b.pair(sads=_curve_min_at(1), inc=-4, delta=np.float32(0))
    b.pair(sads=_curve_min_at(9), inc=4, delta=np.float32(0))
    b.pair(sads=_curve_min_at(5), inc=0, delta=np.float32(0))
    # two equal minima at k = 3 and k = 7: the first wins
    b.pair(sads=(1000, 800, 600, 500, 600, 700, 600, 500, 600, 700, 800), inc=-2, best_sad=500)
    # every SAD equal: the first wins, which is incR = -L
    b.pair(sads=(40,) * 11, stage=R.SAD_MIN_FIRST, inc=-5)
    # equal minima side by side: d3 == d2, deltaR = p / 2p = + 1/2 exactly
    b.pair(sads=(400, 300, 200, 100, 20, 20, 100, 200, 300, 400, 500), inc=-1,
           delta=np.float32(0.5))
    # d1 = d2 + 1, d3 = d2 + 2000: deltaR = -1999 / 4002
    b.pair(sads=(600, 400, 200, 100, 21, 20, 2020, 2100, 2200, 2300, 2400), inc=0,
           delta=np.float32(-1999.0) / np.float32(4002.0))
    # asymmetric neighbours: deltaR = (100 - 40) / (2 * (100 + 40 - 40)) = 0.3
    b.pair(sads=(500, 400, 300, 200, 100, 20, 40, 200, 300, 400, 500), inc=0,
           delta=np.float32(60.0) / np.float32(200.0))
    return b.done()


def _median_case(name, sads, cut):
    b = Builder(name)
    for s in sads:
        b.pair(sads=v_curve(s), reason=R.MEDIAN_CUT if s in cut else R.ACCEPTED, best_sad=s)
    return b.done()


def case_median_one():
    """One accepted match: it is its own median and stays."""
    return _median_case("median_one", [20], ())


def case_median_odd():
    """Five matches, median 10 (index 2): 21 == 2.1 * 10 is cut by the strict
    '<' (1.5f * 1.4f * 10 rounds to 21 exactly), 20 stays."""
    return _median_case("median_odd", [21, 5, 10, 20, 10], (21,))


def case_median_even():
    """Eight matches, median = element 4 of the sorted list (5, 10, 10, 10, 10,
    20, 21, 50), equal SADs on both sides of it; 21 and 50 are cut, 20 stays."""
    return _median_case("median_even", [50, 10, 21, 10, 10, 10, 20, 5], (50, 21))


def case_median_zero():
    """The same noise-free image on both sides, the right one moved by 3 px:
    every match has SAD 0, the median is 0 and 0 < 0 fails, so every match is
    removed."""
    b = Builder("median_zero")
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (b.h, b.w + 3)).astype(np.uint8)
    b.left = np.ascontiguousarray(img[:, :b.w])
    b.right = np.ascontiguousarray(img[:, 3:])
    for _ in range(6):
        cu, cv = b.slot()
        c = b.new_code()
        b.Rk(float(cu), float(cv), 0, c)
        b.L(float(cu) + 3.0, float(cv), 0, c, R.ACCEPTED, R.MEDIAN_CUT, best_sad=0, inc=0)
    return b.done()


def case_capacity_4096():
    """n = nr = 4096 (the capacity of the kernel's packed sort key): deciding
    keypoints at indices 0, 255, 256 and 4095, ties across the whole index
    range, replicated ordinary pairs in between, and one window of black
    against white whose SAD (58650) needs 16 of the key's 20 SAD bits."""
    b = Builder("capacity_4096")
    N = 4096
    # four deciding strips and eight ordinary ones
    ca, cb, cc = b.new_code(), b.new_code(), b.new_code()
    sa, sb, sc = b.slot(), b.slot(), b.slot()
    for s in (sa, sb):
        b.curve(s[0], s[1], V_CURVE)
    # black against white: left window 0 with a 255 centre; right strip 255 with the
    # eleven possible centres 0. incR = 0: 110 * 510 + 10 * 255 = 58650, 255 more per step
    cu, cv = sc
    b.left[cv - 5:cv + 6, cu + 2 - 5:cu + 2 + 6] = 0
    b.left[cv, cu + 2] = 255
    b.right[cv - 5:cv + 6, cu - 10:cu + 11] = 255
    b.right[cv, cu - 5:cu + 6] = 0
    base = []
    for j in range(8):
        s = b.slot()
        c = b.new_code()
        b.curve(s[0], s[1], v_curve(20 + 3 * j))
        base.append((s, c))
    rights, lefts = {}, {}
    # right 0 and right 4095 tie for left 0; right 255 and right 256 tie for left 255
    rights[0] = (float(sa[0]), float(sa[1]), 0, flip(ca, 30))
    rights[4095] = (float(sa[0]) + 3.0, float(sa[1]), 0, flip(ca, 30, 64))
    rights[255] = (float(sb[0]), float(sb[1]), 0, flip(cb, 30))
    rights[256] = (float(sb[0]) + 3.0, float(sb[1]), 0, flip(cb, 30, 64))
    rights[2048] = (float(sc[0]), float(sc[1]), 0, cc)
    lefts[0] = (float(sa[0]) + 8.0, float(sa[1]), 0, ca)
    lefts[255] = (float(sb[0]) + 8.0, float(sb[1]), 0, cb)
    lefts[256] = (float(sb[0]) + 9.0, float(sb[1]), 0, cb)
    lefts[4095] = (float(sc[0]) + 2.0, float(sc[1]), 0, cc)
    for i in range(N):
        (s, c) = base[i % 8]
        if i in rights:
            b.Rk(*rights[i])
        elif i % 32 < 8:
            b.Rk(float(s[0]), float(s[1]), 0, c)            # a replica of pair i % 8
        else:
            b.Rk(110.0 + i % 7, float(i % H0), i % 3)       # right of every left keypoint
        if i in lefts:
            x, y, o, d = lefts[i]
            b.L(x, y, o, d)
        elif i % 32 < 8:
            b.L(float(s[0]) + 8.0, float(s[1]), 0, c)
        else:
            b.L(float(s[0]) + 8.0, float(s[1]) + 0.25, 1, c)   # level 1 on the resized strip
    b.trace = {0: dict(best_idx=0), 255: dict(best_idx=255), 256: dict(best_idx=255),
               4095: dict(best_idx=2048, best_sad=58650, inc=0)}
    b.stage = {0: R.ACCEPTED, 255: R.ACCEPTED, 256: R.ACCEPTED, 4095: R.ACCEPTED}
    b.reason = {4095: R.MEDIAN_CUT, 0: R.ACCEPTED}
    return b.done()


def case_rows_1024():
    """A 1024-row frame, the most the kernel's row table holds: right
    keypoints whose bands end on row 0 and on row 1023, left keypoints on both,
    and ordinary pairs next to them."""
    b = Builder("rows_1024", w=72, h=1024)
    def at(uR, y, vL, stage, **trace):
        c = b.new_code()
        iR = b.Rk(uR, y, 0, c)
        b.L(uR + 4.0, vL, 0, c, stage, best_idx=iR, **trace)
    at(30.0, 1023.0, 1023.0, R.WINDOW_OUTSIDE)
    at(30.0, 1023.0, 1023.9, R.WINDOW_OUTSIDE)
    at(30.0, 1021.0, 1023.0, R.WINDOW_OUTSIDE)      # band 1019 .. 1023
    at(30.0, 1016.0, 1018.0, R.SAD_MIN_FIRST)       # cvL = 1018 = H - 6: inside
    at(30.0, 0.0, 0.0, R.WINDOW_OUTSIDE)
    at(30.0, 3.0, 5.0, R.SAD_MIN_FIRST)
    c = b.new_code()
    b.Rk(30.0, 1020.9, 0, c)                        # band 1018 .. 1023
    b.L(34.0, 1017.9, 0, c, R.NO_CANDIDATE)         # row 1017: only the band of y = 1016
    # ordinary pairs far down the frame
    b._slot = 3 * 40
    for s in (20, 24, 30):
        b.pair(sads=v_curve(s), best_sad=s)
    return b.done()


def case_scratch_top_level():
    """Right keypoints only on the top level of a 2.0-factor, 4-level pyramid
    (scale 8: each enters 33 rows, against the 20 per keypoint the host entry
    point used to reserve). Textured pair, 16 px of disparity: 2 px on level 3
    (41 x 31), where the windows lie."""
    load_pkg()
    import orbpl.synth as synth
    b = Builder("scratch_top_level", w=321, h=243, levels=4, factor=2.0, fx=64.0, bf=16.0)
    img = synth.textured_image(321 + 16, 243, seed=5)
    rng = np.random.default_rng(5)
    b.left = np.ascontiguousarray(img[:, :321])
    noisy = img[:, 16:].astype(np.int32) + rng.integers(-3, 4, (243, 321))
    b.right = np.clip(noisy, 0, 255).astype(np.uint8)
    for i, (cx, cy) in enumerate([(12, 6), (16, 9), (20, 12), (24, 15), (27, 18), (14, 22),
                                  (18, 24), (22, 7), (26, 10), (11, 14), (15, 17), (19, 20)]):
        c = b.new_code()
        iR = b.Rk(8.0 * cx, 8.0 * cy, 3, flip(c, i))
        b.L(8.0 * cx + 16.0, 8.0 * cy, 3 if i % 3 else 2, c, best_idx=iR, best_dist=i)
    return b.done()


DIRECTED = [case_row_bands, case_octave_gate, case_disparity_window,
            case_disparity_below_max, case_descriptor,
            case_tie_order_256, case_tie_order_bands, case_endu, case_window_skip, case_sad_curve, case_median_one,
            case_median_odd, case_median_even, case_median_zero, case_scratch_top_level]
LARGE = [case_capacity_4096, case_rows_1024]


@functools.lru_cache(maxsize=None)
def directed(fn):
    return fn()


# ---------------------------------------------------------------------------
# shifted pairs off the default pyramid: (levels, factor) x (w, h)
SHIFT_GEOMS = [(1, 1.2), (2, 1.2), (4, 2.0), (5, 1.5), (12, 1.1), (16, 1.05)]
SHIFT_SIZES = [(321, 243), (240, 320)]      # _geometry_cases: landscape, portrait
SHIFT_DISP = (4, 9, 14, 6)                  # px, one per quarter of the rows
SHIFT_FX, SHIFT_BF = 32.0, 8.0              # maxD = 32


def shifted_id(g, s):
    return f"{s[0]}x{s[1]}_l{g[0]}_s{g[1]}"


@functools.lru_cache(maxsize=None)
def shifted_pair(w, h):
    """Left: a textured image. Right: each quarter of its rows moved left by
    SHIFT_DISP px (so a point at column u is seen at u - d), both with their
    own +-3 grey levels of noise, or every SAD would be 0 and the median cut
    would remove every match."""
    load_pkg()
    import orbpl.synth as synth
    pad = max(SHIFT_DISP)
    img = synth.textured_image(w + pad, h, seed=7).astype(np.int32)
    rng = np.random.default_rng(7)
    left = img[:, :w] + rng.integers(-3, 4, (h, w))
    right = np.empty((h, w), np.int32)
    for q, d in enumerate(SHIFT_DISP):
        r0, r1 = q * h // 4, (q + 1) * h // 4
        right[r0:r1] = img[r0:r1, d:d + w]
    right += rng.integers(-3, 4, (h, w))
    disp = np.repeat(SHIFT_DISP, [(q + 1) * h // 4 - q * h // 4 for q in range(4)])
    return (np.clip(left, 0, 255).astype(np.uint8), np.clip(right, 0, 255).astype(np.uint8), disp)


@functools.lru_cache(maxsize=None)
def shifted_case(levels, factor, w, h):
    """The pair with the oracle extractor's keypoints of both images."""
    O = load_oracle()
    left, right, _ = shifted_pair(w, h)
    p = O.params(500, factor, levels, 20, 7)
    kl, dl, _ = O.extract(p, left)
    kr, dr, _ = O.extract(p, right)
    return Case(shifted_id((levels, factor), (w, h)), w, h, levels, factor, SHIFT_FX, SHIFT_BF,
                left, right, kl, dl, kr, dr, {}, {}, {})


def content_pyramid(O, c, img):
    """The oracle's pyramid of img as content-only levels (its levels carry a
    19 px border)."""
    p = O.params(*orb_of(c))
    return [np.ascontiguousarray(lv[19:-19, 19:-19]) for lv in O.pyramid(p, img)]


def run_ref(O, c):
    p = O.params(*orb_of(c))
    _, _, _, sc, isc = O.level_sizes(p, c.w, c.h)
    return R.compute_stereo_matches(c.bf, c.fx, sc, isc, content_pyramid(O, c, c.left),
                                    content_pyramid(O, c, c.right), c.kl, c.dl, c.kr, c.dr)


def run_oracle(O, c):
    return O.stereo_matches(O.camera(cfg_of(c)), O.params(*orb_of(c)), c.left, c.right, c.kl, c.dl,
                            c.kr, c.dr)
