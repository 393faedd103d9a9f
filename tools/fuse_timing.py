#!/usr/bin/env python3
"""First timings of the batched SearchInNeighbors call (no threshold: nothing of
this kind existed before). k_search_in_neighbors on one map of 11 keyframes x
1000 keypoints, one of 11 x 2048, and a batch of 64 maps of 11 x 1000
(tests/_fuse_problems.py scenes, 10 first neighbours; 8 distinct maps, each
problem with its own copy in the pools), device-resident inputs
(orblm_search_in_neighbors_batch_device). The call mutates its map, so every
timed launch starts from freshly uploaded inputs; hipEvents around the launch
alone on the null stream, one warm-up launch, the median of 10. One more launch
with in-kernel stamps (orblm_debug_search_in_neighbors_phases) splits the time
of a workgroup into the Fuse calls' search phases and their commit phases.

Every case runs in a child process of its own under a time limit; the first one
that fails or runs out of time ends the run. Writes
profiles/r09/fuse_timing.txt (or the path given as the first argument) with the
commit (the second argument, where the tree is not a git checkout) and the box.
"""
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))
from _pkg import load_pkg  # noqa: E402

REPS = 10
CASES = {"1x1000": (1, 1000), "1x2048": (1, 2048), "64x1000": (64, 1000)}
LIMIT_S = 240
DISTINCT = 8
KEYFRAMES = 11


def one_case(name):
    import warnings
    warnings.simplefilter("ignore")
    import _fuse_problems as FP
    from reloc_timing import Events
    pkg = load_pkg()
    ns, nkp = CASES[name]
    cam = pkg.Camera(FP.CAM["fx"], FP.CAM["fy"], FP.CAM["cx"], FP.CAM["cy"], 0, 0, 0, 0, 0,
                     FP.CAM["bf"], 3.0, FP.W, FP.H)
    fuser = pkg.NeighborFuser(cam, FP.SCALE, FP.SIGMA2)
    base = [FP.scene(400 + k, KEYFRAMES, nkp, corners_per=1.2) for k in range(min(ns, DISTINCT))]
    probs = [dict(map=base[i % len(base)]["map"], cur=base[i % len(base)]["cur"]) for i in range(ns)]
    dev = pkg.SinDeviceProblems(fuser, probs)
    ev = Events()

    def timed():
        dev.upload()
        return ev.time(dev.run)

    timed()                                     # warm-up
    ms = float(np.median([timed() for _ in range(REPS)]))
    out = dev.download()
    dev.upload()
    ph = dev.run_phases().mean(axis=0)
    nt = np.mean([len(o["targets"]) for o in out])
    nf = np.mean([o["n_fused"].sum() for o in out])
    pts = np.mean([len(o["bad"]) for o in out])
    print(f"  {name:8s}: {ms:9.4f} ms per launch, {1e3 * ms / ns:10.2f} us per problem "
          f"({pts:.0f} map points, {nt:.0f} targets, {nf:.0f} fused per problem); a workgroup: "
          f"{ph[2]:.0f} us, of which search phases {ph[0]:.0f} us, commit phases {ph[1]:.0f} us "
          f"(commit / search = {ph[1] / max(ph[0], 1e-9):.2f})")


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--case":
        one_case(sys.argv[2])
        return
    from reloc_timing import box, commit
    out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles/r09/fuse_timing.txt"
    lines = ["SearchInNeighbors kernel, first measurements (tools/fuse_timing.py): hipEvents on the null "
             f"stream, inputs uploaded before every launch, 1 warm-up launch, median of {REPS}, one process "
             "per case; phase times from in-kernel stamps of one more launch.",
             "commit: " + (sys.argv[2] if len(sys.argv) > 2 else commit())] + box() + [""]
    lines.append(f"k_search_in_neighbors, {KEYFRAMES} keyframes, 10 first neighbours, one 256-thread "
                 "workgroup per problem (problems x keypoints per keyframe)")
    for name in CASES:
        try:
            r = subprocess.run([sys.executable, __file__, "--case", name], capture_output=True,
                               text=True, timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            lines.append(f"  {name}: no result within {LIMIT_S} s; stopped here")
            break
        if r.returncode != 0:
            lines.append(f"  {name}: failed with exit status {r.returncode}; stopped here")
            sys.stderr.write(r.stdout + r.stderr)
            break
        lines.append(r.stdout.rstrip("\n"))
    text = "\n".join(lines) + "\n"
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(text)
    print(text)


if __name__ == "__main__":
    main()
