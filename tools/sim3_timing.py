#!/usr/bin/env python3
"""First timings of the loop-closing kernels (no threshold: nothing to compare
against yet), device-resident inputs, hipEvents around each launch on the null
stream, one warm-up launch, the median of 10.

k_sim3_iterate at 1 / 64 / 1024 solvers of N = 100 correspondences (TUM1
intrinsics, 50 % outliers, ComputeSim3's RANSAC parameters 0.99 / 20 / 300, so
mRansacMaxIts = 300), as iterate(5) and as find() (one call of up to 300
hypotheses, all computed in phase A). The solver state is zeroed before every
launch, outside the timed region, so each launch is a first call.

k_search_by_sim3 at 1 / 64 pairs of 1000 features per keyframe (seeded scenes
of tests/_sim3_problems.py, th = 7.5); matched12, which the launch updates, is
restored before every launch, outside the timed region.

Every case runs in a child process of its own under a time limit; the first
one that fails or runs out of time ends the run. Writes
profiles/r11/sim3_timing.txt (or the path given as the first argument) with the
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
LIMIT_S = 120
CASES = [("iterate5", 1), ("iterate5", 64), ("iterate5", 1024), ("find", 1), ("find", 64),
         ("find", 1024), ("match", 1), ("match", 64)]
STATE = ("iterations", "best_inliers", "best_mask", "best_T12", "best_R", "best_t", "best_s")


def solver_case(kind, ns):
    from _sim3_problems import SIGMA2, make_problem
    from reloc_timing import Events
    pkg = load_pkg()
    base = [make_problem(100, 0.5, seed=500 + k, extras=False) for k in range(min(ns, 16))]
    pairs = [dict(base[s % len(base)]["pair"], fix_scale=bool(s % 2),
                  draws=base[s % len(base)]["draws"], min_inliers=20) for s in range(ns)]
    dev = pkg.Sim3DeviceProblems(pairs, SIGMA2, 0.99, 20, 300)
    dev.setup()
    n_it = 5 if kind == "iterate5" else 300
    ev = Events()

    def timed():
        for k in STATE:
            dev.bufs[k].zero()
        return ev.time(lambda: dev.iterate(n_it))

    timed()                                     # warm-up
    ms = float(np.median([timed() for _ in range(REPS)]))
    out = dev.download()
    walked = np.mean([o["draws_consumed"] / 3 for o in out])
    found = np.mean([o["result"] == 1 for o in out])
    print(f"  {kind:8s} solvers {ns:5d}: {ms:9.4f} ms per launch, {1e3 * ms / ns:10.3f} us per "
          f"solver ({n_it} hypotheses computed, {walked:.1f} walked on average, Sim3 found in "
          f"{100 * found:.0f} %)")


def match_case(ns):
    from _sim3_problems import SCALE, TH, kernel_camera, scene
    from reloc_timing import Events
    pkg = load_pkg()
    base = [scene(1000, 700 + k) for k in range(min(ns, 8))]
    dev = pkg.Sim3MatchDeviceProblems([base[s % len(base)] for s in range(ns)])
    cam = kernel_camera(pkg)
    ev = Events()

    def timed():
        dev.bufs["matched12"].upload(dev.host_matched12)
        return ev.time(lambda: dev.run(cam, SCALE, TH))

    timed()                                     # warm-up
    ms = float(np.median([timed() for _ in range(REPS)]))
    out = dev.download()
    print(f"  match    pairs   {ns:5d}: {ms:9.4f} ms per launch, {1e3 * ms / ns:10.3f} us per "
          f"pair (1000 features per keyframe, nFound {np.mean([o['n_found'] for o in out]):.0f} "
          "on average)")


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--case":
        kind, ns = sys.argv[2], int(sys.argv[3])
        match_case(ns) if kind == "match" else solver_case(kind, ns)
        return
    from reloc_timing import box, commit
    out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles/r11/sim3_timing.txt"
    lines = ["Sim3 solver and SearchBySim3 kernels, first measurements (tools/sim3_timing.py): "
             f"hipEvents on the null stream, 1 warm-up launch, median of {REPS}, one process per "
             "case.", "commit: " + (sys.argv[2] if len(sys.argv) > 2 else commit())] + box() + [""]
    lines.append("k_sim3_iterate: N = 100, 50 % outliers, min_inliers 20, mRansacMaxIts 300; "
                 "k_search_by_sim3: 1000 features per keyframe, th 7.5")
    for kind, ns in CASES:
        try:
            r = subprocess.run([sys.executable, __file__, "--case", kind, str(ns)],
                               capture_output=True, text=True, timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            lines.append(f"  {kind} {ns}: no result within {LIMIT_S} s; stopped here")
            break
        if r.returncode != 0:
            lines.append(f"  {kind} {ns}: failed with exit status {r.returncode}; stopped here")
            sys.stderr.write(r.stdout + r.stderr)
            break
        lines.append(r.stdout.rstrip("\n"))
    text = "\n".join(lines) + "\n"
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(text)
    print(text)


if __name__ == "__main__":
    main()
