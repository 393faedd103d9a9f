#!/usr/bin/env python3
"""First timings of the batched KeyFrameCulling call (no threshold: nothing of
this kind existed before). k_keyframe_culling on one map of 11 keyframes x 2048
features, one of 11 x 1000, and a batch of 64 maps of 11 x 1000
(tests/_cull_problems.py scenes, a 10-entry list; 8 distinct maps, each problem
with its own copy in the pools), device-resident inputs
(orblm_keyframe_culling_batch_device). The call mutates its map, so every timed
launch starts from freshly uploaded inputs; hipEvents around the launch alone
on the null stream, one warm-up launch, the median of 10.

Every case runs in a child process of its own under a time limit; the first one
that fails or runs out of time ends the run. Writes
profiles/r10/cull_timing.txt (or the path given as the first argument) with the
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
CASES = {"1x2048": (1, 2048), "1x1000": (1, 1000), "64x1000": (64, 1000)}
LIMIT_S = 240
DISTINCT = 8
KEYFRAMES = 11


def one_case(name):
    import warnings
    warnings.simplefilter("ignore")
    import _cull_problems as CP
    from reloc_timing import Events
    pkg = load_pkg()
    ns, nkp = CASES[name]
    cam = pkg.Camera(CP.CAM["fx"], CP.CAM["fy"], CP.CAM["cx"], CP.CAM["cy"], 0, 0, 0, 0, 0,
                     CP.CAM["bf"], float(CP.TH_DEPTH), 640, 480)
    culler = pkg.MapCuller(cam, CP.SCALE, CP.SIGMA2)
    base = [CP.scene(500 + k, KEYFRAMES, nkp, pool=1.3) for k in range(min(ns, DISTINCT))]
    probs = [base[i % len(base)] for i in range(ns)]
    dev = pkg.KfcDeviceProblems(culler, probs)
    ev = Events()

    def timed():
        dev.upload()
        return ev.time(dev.run)

    timed()                                     # warm-up
    ms = float(np.median([timed() for _ in range(REPS)]))
    out = dev.download()
    act = np.concatenate([o["action"] for o in out])
    pts = np.mean([len(o["bad"]) for o in out])
    print(f"  {name:8s}: {ms:9.4f} ms per launch, {1e3 * ms / ns:10.2f} us per problem "
          f"({pts:.0f} map points, {len(act) / ns:.1f} list entries, "
          f"{np.sum(act == pkg.KFC_ACTIONS.index('culled')) / ns:.1f} culled, "
          f"{np.mean([o['n_points_bad'] for o in out]):.1f} points set bad per problem)")


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--case":
        one_case(sys.argv[2])
        return
    from reloc_timing import box, commit
    out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles/r10/cull_timing.txt"
    lines = ["KeyFrameCulling kernel, first measurements (tools/cull_timing.py): hipEvents on the null "
             f"stream, inputs uploaded before every launch, 1 warm-up launch, median of {REPS}, one process "
             "per case.",
             "commit: " + (sys.argv[2] if len(sys.argv) > 2 else commit())] + box() + [""]
    lines.append(f"k_keyframe_culling, {KEYFRAMES} keyframes, one 256-thread workgroup per problem "
                 "(problems x features per keyframe)")
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
