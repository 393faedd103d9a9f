"""The DBoW2 transform on the GPU (k_bow_words / k_bow_vector) branch by
branch: ORBVocabulary.transform against the oracle and against the sequential
restatement tests/_bow_ref.py, bit for bit, on the hand-built vocabularies of
tests/_bow_cases.py (sibling numberings, fan-out 1 to 20, Hamming ties and
extremes, unbalanced trees, leaf flags and stop words, BowVector assembly at
0 to 4096 features, every scoring x weighting pair on order-sensitive
weights, the empty vocabulary, the largest accepted vocabulary), and the
batch call: several frames in one launch, unequal pitches, an explicit
stream, and a frame longer than max_n."""
import ctypes as C

import numpy as np
import pytest

import _bow_cases as BC

pytestmark = pytest.mark.gpu

RUNS, RUN_IDS = BC.case_runs(BC.small_cases())
_VOCS = {}


def _vocs(orbpl, oracle, arrays):
    """One device vocabulary and one oracle vocabulary per `arrays` object."""
    if id(arrays) not in _VOCS:
        _VOCS[id(arrays)] = (orbpl.ORBVocabulary(arrays=arrays), oracle.Vocabulary(arrays=arrays),
                             arrays)
    return _VOCS[id(arrays)][:2]


def _check(orbpl, oracle, case, levelsup):
    g, o = _vocs(orbpl, oracle, case.arrays)
    ref = BC.reference(case, levelsup)
    name = f"{case.name} levelsup {levelsup}"
    gw, gv, gn = g.transform(case.feats, levelsup=levelsup)
    msg = BC.mismatch(name + " (device against restatement)", case.arrays, ref, gw, gv, gn)
    assert msg is None, msg
    ow, ov, on, _, _ = o.transform(case.feats, levelsup=levelsup)
    assert np.array_equal(gn, on), name
    assert np.array_equal(gw, ow) and np.array_equal(gv.view(np.uint64), ov.view(np.uint64)), name


@pytest.mark.parametrize("case,levelsup", RUNS, ids=RUN_IDS)
def test_transform_equals_oracle_and_restatement(orbpl, oracle, case, levelsup):
    _check(orbpl, oracle, case, levelsup)


def test_transform_at_the_word_limit(orbpl, oracle):
    """2^20 - 1 words, 4096 features: feature 4095 in the last word has the
    largest sort key a frame can produce and stays in the BowVector; 16
    children per node at real size."""
    case = BC.limit_case()
    ref = BC.reference(case, case.levelsups[0])
    case.aim(ref, case.levelsups[0])
    g = orbpl.ORBVocabulary(arrays=case.arrays)
    gw, gv, gn = g.transform(case.feats, levelsup=case.levelsups[0])
    msg = BC.mismatch(case.name, case.arrays, ref, gw, gv, gn)
    assert msg is None, msg
    assert gw[-1] == BC.MAX_WORDS - 1 and gn[BC.MAX_FEAT - 1] > 0


# --------------------------------------------------------------------------
# the batch call
# --------------------------------------------------------------------------
class _Stream:
    """A stream of the HIP runtime the library runs on."""

    def __init__(self):
        path = None
        with open("/proc/self/maps") as maps:
            for line in maps:
                if "libamdhip64" in line:
                    path = line.split()[-1]
                    break
        assert path, "the HIP runtime is not loaded"
        self.hip = C.CDLL(path)
        self.hip.hipStreamSynchronize.argtypes = [C.c_void_p]
        self.hip.hipStreamDestroy.argtypes = [C.c_void_p]
        h = C.c_void_p()
        assert self.hip.hipStreamCreate(C.byref(h)) == 0
        self.handle = h.value

    def synchronize(self):
        assert self.hip.hipStreamSynchronize(self.handle) == 0

    def destroy(self):
        assert self.hip.hipStreamDestroy(self.handle) == 0


PATTERN_WORD, PATTERN_NODE = 7, 0x5A5A5A5A


def _run_batch(orbpl, g, frames, max_n, levelsup, desc_pitch, out_pitch, stream=None):
    """One orbv_transform_batch_device call. The per-feature outputs are
    pre-filled: word 7 / weight 1 / node 0x5A5A5A5A, so a slot that is read
    without having been written adds to the BowVector, and a slot that is
    written without reason shows."""
    g.upload()
    F = len(frames)
    desc = np.zeros((F, desc_pitch, 32), np.uint8)
    n = np.zeros(F, np.int32)
    for f, d in enumerate(frames):
        desc[f, :len(d)] = d
        n[f] = len(d)
    dd = orbpl.DeviceBuffer.from_array(desc)
    dn = orbpl.DeviceBuffer.from_array(n)
    FP = F * out_pitch
    out = dict(pitch=out_pitch,
               feat_node=orbpl.DeviceBuffer.from_array(np.full(FP, PATTERN_NODE, np.int32)),
               feat_word=orbpl.DeviceBuffer.from_array(np.full(FP, PATTERN_WORD, np.int32)),
               feat_weight=orbpl.DeviceBuffer.from_array(np.ones(FP, np.float64)),
               bow_words=orbpl.DeviceBuffer.from_array(np.full(FP, 0xFFFFFFFF, np.uint32)),
               bow_vals=orbpl.DeviceBuffer.from_array(np.full(FP, -1.0, np.float64)),
               bow_n=orbpl.DeviceBuffer.from_array(np.full(F, -1, np.int32)),
               err=orbpl.DeviceBuffer(4))
    out["err"].zero()
    orbpl.lib().orbpl_device_synchronize(0)
    g.transform_batch_device(dd.ptr, desc_pitch, dn.ptr, F, max_n, levelsup, out,
                             stream=None if stream is None else stream.handle)
    if stream is not None:
        stream.synchronize()
    orbpl.lib().orbpl_device_synchronize(0)
    res = dict(node=out["feat_node"].download(np.int32, (F, out_pitch)),
               words=out["bow_words"].download(np.uint32, (F, out_pitch)),
               vals=out["bow_vals"].download(np.float64, (F, out_pitch)),
               bow_n=out["bow_n"].download(np.int32, F),
               err=int(out["err"].download(np.int32, 1)[0]))
    for b in list(out.values()) + [dd, dn]:
        if hasattr(b, "free"):
            b.free()
    return res


def _check_frame(name, arrays, ref, res, f, n):
    k = int(res["bow_n"][f])
    assert 0 <= k <= n, (name, f, k)
    msg = BC.mismatch(f"{name} frame {f}", arrays, ref, res["words"][f, :k], res["vals"][f, :k],
                      res["node"][f, :n])
    assert msg is None, msg
    assert np.all(res["node"][f, n:] == PATTERN_NODE), (name, f)      # nothing past the frame


def test_batch_assembly_cases(orbpl, oracle):
    """Every BowVector assembly case as one frame of one launch."""
    cases = BC.assembly_cases()
    g, _ = _vocs(orbpl, oracle, cases[0].arrays)
    res = _run_batch(orbpl, g, [c.feats for c in cases], BC.MAX_FEAT, 1, BC.MAX_FEAT, BC.MAX_FEAT)
    assert res["err"] == 0
    for f, c in enumerate(cases):
        _check_frame(c.name, c.arrays, BC.reference(c, 1), res, f, len(c.feats))


@pytest.mark.parametrize("levelsup", [0, 2])
def test_batch_frames_pitches_and_stream(orbpl, oracle, levelsup):
    """Frames of 0 to 512 features in one launch on a stream of the caller's;
    the descriptor pitch and the output pitch differ and both exceed max_n."""
    import _bow_ref as R
    arrays, _ = BC.assembly_vocabulary()
    g, o = _vocs(orbpl, oracle, arrays)
    frames = BC.batch_frames()
    max_n = max(len(d) for d in frames)
    assert max_n == 512 and min(len(d) for d in frames) == 0
    s = _Stream()
    res = _run_batch(orbpl, g, frames, max_n, levelsup, max_n + 7, max_n + 32, stream=s)
    s.destroy()
    assert res["err"] == 0
    for f, d in enumerate(frames):
        ref = R.transform(arrays, d, levelsup, tree=BC.tree_of(arrays))
        _check_frame("batch", arrays, ref, res, f, len(d))
        ow, ov, on, _, _ = o.transform(d, levelsup=levelsup)
        assert np.array_equal(ref.bow_words, ow) and np.array_equal(ref.feat_node, on)
        assert np.array_equal(ref.bow_vals.view(np.uint64), ov.view(np.uint64))


def test_batch_empty_vocabulary(orbpl, oracle):
    """The root-only vocabulary and the one without words, through the batch
    call: bow_n is 0 and every node is -1."""
    for case in BC.empty_cases():
        g, _ = _vocs(orbpl, oracle, case.arrays)
        frames = [case.feats, case.feats[:2], case.feats[:0]]
        res = _run_batch(orbpl, g, frames, 8, 0, 8, 8)
        assert res["err"] == 0 and res["bow_n"].tolist() == [0, 0, 0], case.name
        for f, d in enumerate(frames):
            assert np.all(res["node"][f, :len(d)] == -1), (case.name, f)


def test_batch_frame_longer_than_max_n(orbpl, oracle):
    """max_n = 300 and a frame of 400 features (below the 512 sort slots):
    the frame is cut to its first 300 features and err is 2; the slots 300 to
    399, which k_bow_words did not write, still hold the pre-filled word and
    weight and must not reach the BowVector. The frames beside it are whole."""
    import _bow_ref as R
    arrays, _ = BC.assembly_vocabulary()
    g, _ = _vocs(orbpl, oracle, arrays)
    long = BC.overflow_frame()
    other = BC.batch_frames()[0]
    assert len(long) == 400 and len(other) == 300
    res = _run_batch(orbpl, g, [other, long, other[:17]], 300, 1, 416, 448)
    assert res["err"] == 2
    tree = BC.tree_of(arrays)
    for f, d in enumerate([other, long[:300], other[:17]]):
        _check_frame("longer_than_max_n", arrays, R.transform(arrays, d, 1, tree=tree), res, f, len(d))
    full = R.transform(arrays, long, 1, tree=tree)
    assert len(full.bow_words) == res["bow_n"][1] + 1      # the 100 cut features were one more word
