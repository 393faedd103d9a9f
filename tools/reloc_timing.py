#!/usr/bin/env python3
"""First timings of the two relocalisation kernels (no threshold: nothing to
compare against yet). hipEvents around each launch on the null stream, one
warm-up launch, the median of 20, everything in one process:

  k_kfdb_reloc  DetectRelocalizationCandidates at nq = 1, 256, 2048 problems of
                32 keyframes and ~600 words per BowVector
  k_match_kf    SearchByProjection(Frame, KeyFrame, sAlreadyFound, 10, 100) at
                batch 1 and 256 with 1000 keypoints on both sides

Device-resident inputs (orbkf_detect_reloc_batch_device,
orbm_search_by_projection_kf_batch_device). Writes profiles/r07/reloc_timing.txt
(or the path given as the first argument) with the commit (the second argument,
where the tree is not a git checkout) and the box.
"""
import ctypes as C
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
from _pkg import load_pkg  # noqa: E402

REPS = 20


class Events:
    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so")
        self.a, self.b = C.c_void_p(), C.c_void_p()
        for e in (self.a, self.b):
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def time(self, launch):
        """ms of one launch on the null stream"""
        assert self.hip.hipEventRecord(self.a, None) == 0
        launch()
        assert self.hip.hipEventRecord(self.b, None) == 0
        assert self.hip.hipEventSynchronize(self.b) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
        return ms.value

    def median(self, launch):
        self.time(launch)                       # warm-up
        return float(np.median([self.time(launch) for _ in range(REPS)]))


def db_batch(pkg, nq, nkf=32, nwords=600, seed=1):
    rng = np.random.default_rng(seed)
    K, ent = pkg.KFDB_MAX_KEYFRAMES, nkf * nwords
    base = []
    for _ in range(min(nq, 16)):                # 16 distinct problems, repeated
        place = rng.choice(100000, nwords + 100, replace=False)
        views = [np.sort(rng.choice(place, nwords, replace=False)) for _ in range(nkf + 1)]
        vals = [rng.random(nwords) / nwords for _ in range(nkf + 1)]
        cov = np.full((K, 10), -1, np.int32)
        for k in range(nkf):
            cov[k] = rng.choice(nkf, 10, replace=False)
        base.append((views, vals, cov))
    off = np.zeros((nq, K + 1), np.int32)
    off[:, :nkf + 1] = np.arange(nkf + 1) * nwords
    kw = np.zeros((nq, ent), np.uint32)
    kv = np.zeros((nq, ent), np.float64)
    qw = np.zeros((nq, nwords), np.uint32)
    qv = np.zeros((nq, nwords), np.float64)
    cov = np.zeros((nq, K, 10), np.int32)
    for p in range(nq):
        views, vals, c = base[p % len(base)]
        kw[p] = np.concatenate(views[:nkf])
        kv[p] = np.concatenate(vals[:nkf])
        qw[p], qv[p], cov[p] = views[nkf], vals[nkf], c
    D = pkg.DeviceBuffer.from_array
    bufs = dict(nkf=D(np.full(nq, nkf, np.int32)), off=D(off), kw=D(kw), kv=D(kv), cov=D(cov),
                rs=D(np.zeros((nq, K), np.float32)), qn=D(np.full(nq, nwords, np.int32)),
                qw=D(qw), qv=D(qv), cand=D(np.zeros((nq, K), np.int32)),
                nc=D(np.zeros(nq, np.int32)), cw=D(np.zeros((nq, K), np.int32)))
    b = pkg.KfdbDeviceBatch(bufs["nkf"].ptr, bufs["off"].ptr, bufs["kw"].ptr, bufs["kv"].ptr, ent,
                            bufs["cov"].ptr, bufs["rs"].ptr, bufs["qn"].ptr, bufs["qw"].ptr,
                            bufs["qv"].ptr, nwords, bufs["cand"].ptr, bufs["nc"].ptr,
                            bufs["cw"].ptr)
    return b, bufs


def match_batch(pkg, batch, n=1000, seed=2):
    rng = np.random.default_rng(seed)
    fx = fy = 520.0
    cx, cy = 320.0, 240.0
    scale = (1.2 ** np.arange(8)).astype(np.float32)
    kps = np.zeros((batch, n), pkg.KP_DTYPE)
    desc = rng.integers(0, 256, (batch, n, 32), dtype=np.uint8)
    kps["x"] = rng.uniform(20, 620, (batch, n))
    kps["y"] = rng.uniform(20, 460, (batch, n))
    kps["octave"] = rng.integers(0, 8, (batch, n))
    kps["angle"] = rng.uniform(0, 360, (batch, n))
    # the keyframe's points: the keypoints unprojected at a depth of 2 to 5 m,
    # moved by a pixel or two, descriptors a few bits away
    z = rng.uniform(2, 5, (batch, n))
    u = kps["x"] + rng.normal(0, 1.5, (batch, n))
    v = kps["y"] + rng.normal(0, 1.5, (batch, n))
    xyz = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], -1).astype(np.float32)
    dist = np.linalg.norm(xyz, axis=-1)
    dmax = (dist * scale[kps["octave"]]).astype(np.float32)
    mpd = desc ^ (rng.random((batch, n, 32)) < 0.02).astype(np.uint8)
    Tcw = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (batch, 1))
    D = pkg.DeviceBuffer.from_array
    bufs = dict(cn=D(np.full(batch, n, np.int32)), T=D(Tcw), kps=D(kps), desc=D(desc),
                held=D((rng.random((batch, n)) < 0.1).astype(np.uint8)),
                kn=D(np.full(batch, n, np.int32)), ang=D(kps["angle"].astype(np.float32)),
                valid=D(np.ones((batch, n), np.uint8)),
                found=D((rng.random((batch, n)) < 0.1).astype(np.uint8)), xyz=D(xyz),
                dmin=D((dmax / scale[-1]).astype(np.float32)), dmax=D(dmax), mpd=D(mpd),
                match=D(np.zeros((batch, n), np.int32)), nm=D(np.zeros(batch, np.int32)))
    b = pkg.MatchKfDeviceBatch(n, bufs["cn"].ptr, bufs["T"].ptr, bufs["kps"].ptr, bufs["desc"].ptr,
                               bufs["held"].ptr, n, bufs["kn"].ptr, bufs["ang"].ptr,
                               bufs["valid"].ptr, bufs["found"].ptr, bufs["xyz"].ptr,
                               bufs["dmin"].ptr, bufs["dmax"].ptr, bufs["mpd"].ptr,
                               bufs["match"].ptr, bufs["nm"].ptr)
    cam = pkg.Camera(fx, fy, cx, cy, 0, 0, 0, 0, 0, 40.0, 3.0, 640, 480)
    return b, bufs, cam, scale


def box():
    out = []
    try:
        info = subprocess.run(["rocminfo"], capture_output=True, text=True).stdout
        names = [ln.split(":", 1)[1].strip() for ln in info.splitlines()
                 if ln.strip().startswith("Name:")]
        gpus = [n for n in names if n.startswith("gfx")]
        out.append("devices: " + ", ".join(f"{gpus.count(g)} x {g}" for g in sorted(set(gpus))))
    except OSError:
        pass
    for ln in Path("/proc/cpuinfo").read_text().splitlines():
        if ln.startswith("model name"):
            out.append("cpu: " + ln.split(":", 1)[1].strip())
            break
    return out


def commit():
    try:
        h = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"],
                           capture_output=True, text=True).stdout.strip()
        dirty = subprocess.run(["git", "-C", str(ROOT), "status", "--porcelain"],
                               capture_output=True, text=True).stdout.strip()
        return (h or "unknown") + (" + working tree changes" if dirty else "")
    except OSError:
        return "unknown"


def main():
    out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles/r07/reloc_timing.txt"
    pkg = load_pkg()
    L = pkg.lib()
    ev = Events()
    lines = ["Relocalisation kernels, first measurements (tools/reloc_timing.py): hipEvents on the "
             f"null stream, 1 warm-up launch, median of {REPS}, one process.",
             "commit: " + (sys.argv[2] if len(sys.argv) > 2 else commit())] + box() + [""]
    lines.append("k_kfdb_reloc (DetectRelocalizationCandidates), 32 keyframes, 600 words per vector")
    for nq in (1, 256, 2048):
        b, bufs = db_batch(pkg, nq)
        ms = ev.median(lambda: pkg.check(L.orbkf_detect_reloc_batch_device(C.byref(b), nq, 0, None)))
        nc = bufs["nc"].download(np.int32, (nq,))
        lines.append(f"  nq {nq:5d}: {ms:8.4f} ms per launch, {1e3 * ms / nq:9.3f} us per problem "
                     f"(candidates per problem: mean {nc.mean():.1f})")
    lines += ["", "k_match_kf (SearchByProjection(Frame, KeyFrame, sAlreadyFound, 10, 100), "
              "orientation check on), 1000 keypoints, 1000 keyframe points"]
    for batch in (1, 256):
        b, bufs, cam, scale = match_batch(pkg, batch)
        ms = ev.median(lambda: pkg.check(L.orbm_search_by_projection_kf_batch_device(
            C.byref(cam), scale.ctypes.data_as(C.c_void_p), len(scale), C.byref(b), batch, 10.0,
            100, 1, None)))
        nm = bufs["nm"].download(np.int32, (batch,))
        lines.append(f"  batch {batch:4d}: {ms:8.4f} ms per launch, {1e3 * ms / batch:9.3f} us per "
                     f"problem (matches per problem: mean {nm.mean():.0f})")
    text = "\n".join(lines) + "\n"
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(text)
    print(text)


if __name__ == "__main__":
    main()
