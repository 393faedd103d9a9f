"""The per-frame line kernels (k_line_prepare, k_line_match, k_line_match_list,
k_line_pairs, k_line_bf_knn, k_line_in_frustum, k_stereo_lines) against the
sequential restatement of tests/_line_ref.py, bit for bit, on every hand-built
case and crowd of tests/_line_cases.py. The projection, threshold, assignment
and retry cases run through the last-frame, list and both harness entries
alike, so k_line_match's own copy of the projection is held to the cases that
hold project_map_line. A failure names the outputs that differ and, for a
search, the first differing current line with the restatement's reasons for it."""
import functools

import numpy as np
import pytest

import _line_cases as LC

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _expected(kind, k, entry):
    return LC.run_ref(LC.all_problems(kind)[k], entry)


def _params(kind):
    return [pytest.param(k, en, id=LC.all_problems(kind)[k].name + (f"-{en}" if en else ""))
            for k, en in LC.runs(kind)]


def _check(orbpl, kind, k, entry=None):
    P = LC.all_problems(kind)[k]
    want, trace = _expected(kind, k, entry)
    got = LC.run_gpu(orbpl, P, entry)
    bad = LC.differences(want, got)
    if not bad:
        return
    note = ""
    if kind == "search" and "match" in bad and want["match"].shape == got["match"].shape:
        j = int(np.flatnonzero(want["match"] != got["match"])[0])
        note = (f": current line {j} holds {int(got['match'][j])}, expected {int(want['match'][j])}; "
                f"passing projected lines per pass {[p[j] for p in trace['passing']]}, "
                f"retry {trace['retry']}")
    elif kind == "search":
        note = f": nm {got['nm']} / {want['nm']}, retry {trace['retry']}"
    else:
        w, g = want[bad[0]], got[bad[0]]
        if isinstance(w, bytes):
            w, g = np.frombuffer(w, LC.KL), np.frombuffer(g, LC.KL)
        if isinstance(w, np.ndarray) and w.shape == np.shape(g):
            i = next(i for i in range(len(w)) if w[i].tobytes() != np.asarray(g)[i].tobytes())
            note = f": {bad[0]}[{i}] is {g[i]}, expected {w[i]}"
    pytest.fail(f"{P} {entry or ''}: {bad} differ{note}")


@pytest.mark.parametrize("k,entry", _params("search"))
def test_search_by_projection(orbpl, k, entry):
    """orbl_search_by_projection_last / _list / _pairs (modes 0 and 1): match, count, wiped,
    the projected KeyLines' bytes, their map-line indices and the pairs, with sentinels around
    every capacity-bound output of the harness entries"""
    _check(orbpl, "search", k, entry)


@pytest.mark.parametrize("k,entry", _params("bf"))
def test_match_bf_knn(orbpl, k, entry):
    _check(orbpl, "bf", k)


@pytest.mark.parametrize("k,entry", _params("frustum"))
def test_line_in_frustum(orbpl, k, entry):
    _check(orbpl, "frustum", k)


@pytest.mark.parametrize("k,entry", _params("prepare"))
def test_line_frame_prepare(orbpl, k, entry):
    _check(orbpl, "prepare", k)


@pytest.mark.parametrize("k,entry", _params("stereo"))
def test_stereo_line_depths(orbpl, k, entry):
    _check(orbpl, "stereo", k)
