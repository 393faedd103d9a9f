"""The four per-frame point matchers on the GPU (k_match_last, k_match_local,
match_bow_body through k_match_bow, k_match_kf) against the sequential
restatement, on every hand-built case and crowd of tests/_match_cases.py, the
last-frame set at each workgroup width of k_match_last and the local set at
each of k_match_local. A failure names the first differing keypoint, the map
points the two sides put there and the restatement's reason for them."""
import functools

import numpy as np
import pytest

import _match_cases as MC

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _problems(kind):
    return tuple(MC.all_problems(kind))


@functools.lru_cache(maxsize=None)
def _expected(kind, k):
    return MC.run_ref(_problems(kind)[k])


def _params(kind):
    return [pytest.param(k, id=p.name) for k, p in enumerate(MC.all_problems(kind))]


def _check(orbpl, kind, k, note=""):
    P = _problems(kind)[k]
    match, nm, rec, _ = _expected(kind, k)
    gm, gn = MC.run_gpu(orbpl, P)
    assert gm.shape == match.shape, (P, note)
    bad = np.flatnonzero(gm != match)
    if bad.size:
        j = int(bad[0])
        why = {}
        if rec is not None:
            for i in {int(gm[j]), int(match[j])} - {-1}:
                if 0 <= i < len(rec):
                    why[i] = (rec[i]["reason"], rec[i]["kp"], rec[i]["best"], rec[i]["second"],
                              rec[i]["ncand"], rec[i]["skipped"])
        pytest.fail(f"{P} {note}: keypoint {j} holds {int(gm[j])}, expected {int(match[j])} "
                    f"({bad.size} keypoints differ; reason, kp, best, second, ncand, skipped "
                    f"of the points involved: {why})")
    assert gn == nm, (P, note, gn, nm)


@pytest.fixture
def width(monkeypatch):
    """the matchers read their workgroup width from the environment per launch"""
    def set_width(var, nt):
        monkeypatch.setenv(var, str(nt))
    return set_width


@pytest.mark.parametrize("nt", [128, 256, 512, 1024])
@pytest.mark.parametrize("k", _params("last"))
def test_search_by_projection_last_frame(orbpl, width, k, nt):
    width("ORBPL_MATCH_NT", nt)
    _check(orbpl, "last", k, f"ORBPL_MATCH_NT={nt}")


@pytest.mark.parametrize("nt", [256, 512, 1024])
@pytest.mark.parametrize("k", _params("local"))
def test_search_by_projection_local_map(orbpl, width, k, nt):
    width("ORBPL_LOCAL_NT", nt)
    _check(orbpl, "local", k, f"ORBPL_LOCAL_NT={nt}")


@pytest.mark.parametrize("k", _params("bow"))
def test_search_by_bow(orbpl, k):
    _check(orbpl, "bow", k)


@pytest.mark.parametrize("k", _params("kf"))
def test_search_by_projection_keyframe(orbpl, k):
    _check(orbpl, "kf", k)
