#!/usr/bin/env python3
"""First timings of the PnP solver kernel (no threshold: nothing to compare
against yet). k_pnp_iterate at 1 / 64 / 1024 solvers of N = 100 correspondences
(TUM1 intrinsics, 50 % outliers, Relocalization's RANSAC parameters: 35
hypotheses per first call), device-resident inputs
(orbpnp_iterate_batch_device). hipEvents around each launch on the null stream,
one warm-up launch, the median of 10; the solver state is zeroed before every
launch, outside the timed region, so each launch is a first iterate(5): all 35
hypotheses are computed, the walk stops at the first Refine() that succeeds.

Every batch size runs in a child process of its own under a time limit; the
first one that fails or runs out of time ends the run. Writes
profiles/r07/pnp_timing.txt (or the path given as the first argument) with the
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
SIZES = (1, 64, 1024)
LIMIT_S = 120
PARAMS = (0.99, 10, 300, 4, 0.5, 5.991)


def one_size(ns):
    from _pnp_problems import make_problem
    from reloc_timing import Events
    pkg = load_pkg()
    base = []
    for k in range(min(ns, 16)):                # 16 distinct problems, repeated
        p = make_problem(100, 0.5, seed=100 + k)
        mn, mx, _, me = pkg.pnp_ransac_parameters(100, *PARAMS, sigma2=p["sigma2"])
        base.append(dict(cam=p["cam"], p2d=p["p2d"], p3d=p["p3d"], max_error=me, min_inliers=mn,
                         max_its=mx, draws=p["draws"]))
    dev = pkg.PnpDeviceProblems([base[s % len(base)] for s in range(ns)], draw_pitch=4 * 35)
    ev = Events()

    def timed():
        for k in ("iterations", "best_inliers", "best_mask", "best_Tcw"):
            dev.bufs[k].zero()
        return ev.time(lambda: dev.iterate(5))

    timed()                                     # warm-up
    ms = float(np.median([timed() for _ in range(REPS)]))
    out = dev.download()
    walked = np.mean([o["draws_consumed"] / 4 for o in out])
    found = np.mean([o["result"] == 1 for o in out])
    print(f"  solvers {ns:5d}: {ms:9.4f} ms per launch, {1e3 * ms / ns:10.3f} us per solver "
          f"(35 hypotheses computed, {walked:.1f} walked on average, pose found in "
          f"{100 * found:.0f} %)")


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--size":
        one_size(int(sys.argv[2]))
        return
    from reloc_timing import box, commit
    out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles/r07/pnp_timing.txt"
    lines = ["PnP solver kernel, first measurements (tools/pnp_timing.py): hipEvents on the null "
             f"stream, 1 warm-up launch, median of {REPS}, one process per batch size.",
             "commit: " + (sys.argv[2] if len(sys.argv) > 2 else commit())] + box() + [""]
    lines.append("k_pnp_iterate (PnPsolver::iterate(5), first call), N = 100, 50 % outliers, "
                 "min_inliers 50, 35 hypotheses")
    for ns in SIZES:
        try:
            r = subprocess.run([sys.executable, __file__, "--size", str(ns)], capture_output=True,
                               text=True, timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            lines.append(f"  solvers {ns:5d}: no result within {LIMIT_S} s; stopped here")
            break
        if r.returncode != 0:
            lines.append(f"  solvers {ns:5d}: failed with exit status {r.returncode}; stopped here")
            sys.stderr.write(r.stdout + r.stderr)
            break
        lines.append(r.stdout.rstrip("\n"))
    text = "\n".join(lines) + "\n"
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(text)
    print(text)


if __name__ == "__main__":
    main()
