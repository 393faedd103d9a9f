"""bench.py's plain run and its side outputs: the rendered-loop cache that
`--prepare` writes (CPU), the `--dump-outputs` writer (CPU), and one plain
run on the GPU: only the headline leg, `--steps` timed steps, `ms_per_step`,
and the last step's outputs as float .npy files."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def test_render_loop_cache_round_trip(tmp_path, monkeypatch):
    """A stored loop is read back bit for bit; a loop nobody stored is
    rendered and leaves no file; the file name follows the arguments."""
    import bench
    monkeypatch.setattr(bench, "LOOP_CACHE", tmp_path / "cache")
    g0, d0 = bench.render_loop(2, seed=3, workers=2)
    assert not (tmp_path / "cache").exists()
    g1, d1 = bench.render_loop(2, seed=3, workers=2, store=True)
    f = bench.loop_cache_file(2, 3, "TUM1", False, 1)
    assert f.exists() and [p.name for p in f.parent.iterdir()] == [f.name]
    assert f != bench.loop_cache_file(2, 4, "TUM1", False, 1)
    assert f != bench.loop_cache_file(2, 3, "TUM3", False, 1)
    monkeypatch.setattr(bench, "_render", None)      # a cached loop renders nothing
    g2, d2 = bench.render_loop(2, seed=3, workers=2)
    for a, b, c in ((g0, g1, g2), (d0, d1, d2)):
        assert a.dtype == b.dtype == c.dtype and a.tobytes() == b.tobytes() == c.tobytes()
    assert g2.shape == (2, 480, 640) and g2.dtype == np.uint8 and d2.dtype == np.float32


def test_write_outputs_float_arrays_within_the_limit(tmp_path, monkeypatch):
    import bench
    arrays = {"Tcw": np.arange(32, dtype=np.float32).reshape(2, 16),
              "counts": np.ones((2, 12), np.float64)}
    bench.write_outputs(tmp_path / "o", arrays)
    bench.write_outputs(tmp_path / "o", arrays, rank=1)
    assert sorted(p.name for p in (tmp_path / "o").iterdir()) == [
        "Tcw.npy", "Tcw_rank1.npy", "counts.npy", "counts_rank1.npy"]
    assert np.array_equal(np.load(tmp_path / "o" / "Tcw.npy"), arrays["Tcw"])
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 100)
    with pytest.raises(SystemExit):
        bench.write_outputs(tmp_path / "p", arrays)
    with pytest.raises(AssertionError):
        bench.write_outputs(tmp_path / "q", {"n": np.zeros(3, np.int32)})


def test_detail_file_never_costs_the_result_line(tmp_path, monkeypatch, capsys):
    """A plain run without --detail writes no side file; --full defaults to the
    temporary directory, never the repository; a place that cannot be written
    gives None and a note on stderr instead of an exception."""
    import argparse
    import tempfile
    import bench
    out = {"value": 1.0}
    assert bench.write_detail(argparse.Namespace(detail=None, full=False), out) is None
    monkeypatch.setattr(tempfile, "tempdir", str(tmp_path))
    name = bench.write_detail(argparse.Namespace(detail=None, full=True), out)
    assert name == str(tmp_path / "bench_detail.json") and json.loads(Path(name).read_text()) == out
    given = tmp_path / "sub" / "d.json"
    assert bench.write_detail(argparse.Namespace(detail=str(given), full=False), out) == str(given)
    assert json.loads(given.read_text()) == out
    (tmp_path / "file").write_text("not a directory")
    blocked = tmp_path / "file" / "d.json"
    assert bench.write_detail(argparse.Namespace(detail=str(blocked), full=True), out) is None
    assert "not written" in capsys.readouterr().err


@pytest.mark.gpu
def test_plain_run_times_the_headline_only_and_dumps_outputs(tmp_path):
    S, steps = 16, 3
    dump = tmp_path / "out"
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--streams", str(S),
           "--steps", str(steps), "--warmup", "1", "--loop", "8", "--vocab-levels", "4",
           "--dump-outputs", str(dump),
           "--detail", str(tmp_path / "detail.json")]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=str(ROOT))
    assert out.returncode == 0, out.stderr[-3000:]
    c = json.loads([x for x in out.stdout.splitlines() if x.startswith("{")][-1])
    assert c["steps"] == steps and c["unit"] == "frames/s" and c["dtype"] == "u8"
    assert c["higher_is_better"] is True and c["value"] > 0 and c["ms_per_step"] > 0
    # value = frames / elapsed and ms_per_step = elapsed / steps: the same clock
    assert abs(c["value"] * c["ms_per_step"] * 1e-3 - S) < 1e-2 * S
    # nothing beside the headline leg ran
    assert c["cpu_baseline"] is None and c["parity"]["headline_pass"] is None
    assert not {"secondary", "stereo", "rig", "ingress"} & set(c["summary"])
    r = json.loads((tmp_path / "detail.json").read_text())
    assert not {"sweep", "trk_load", "ingress", "secondary"} & set(r)
    assert "isolated" not in r["roofline"]
    arr = {p.stem: np.load(p) for p in dump.iterdir()}
    assert {"Tcw", "counts", "sampled_streams", "keypoints", "descriptors", "matches"} == set(arr)
    assert all(a.dtype in (np.float32, np.float64) for a in arr.values())
    assert sum(a.nbytes for a in arr.values()) <= 64 << 20
    assert arr["Tcw"].shape == (S, 16) and arr["Tcw"].dtype == np.float32
    assert np.isfinite(arr["Tcw"]).all()
    assert arr["counts"].shape == (S, 12) and arr["counts"].dtype == np.float64
    assert np.isin(arr["counts"][:, 4], (0, 1)).all()                 # ok
    assert (arr["counts"][:, 0] > 0).all()                            # nkeypoints
    assert np.array_equal(arr["sampled_streams"], np.arange(S))       # S <= DUMP_STREAMS: all
    n = len(arr["keypoints"])
    assert arr["keypoints"].shape == (n, 8) and arr["descriptors"].shape == (n, 32)
    assert arr["matches"].shape == (n, 3)
    per_stream = np.bincount(arr["keypoints"][:, 0].astype(int), minlength=S)
    assert len(per_stream) == S and (per_stream > 0).all()            # rows tagged by stream
    assert 0 <= arr["descriptors"].min() and arr["descriptors"].max() <= 255
    assert arr["descriptors"].max() > 0 and np.array_equal(arr["descriptors"],
                                                           np.rint(arr["descriptors"]))
