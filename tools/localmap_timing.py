#!/usr/bin/env python3
"""First timings of the batched CreateNewMapPoints + CreateNewMapLines call (no
threshold: nothing of this kind existed before). k_create_new_map_features at
1 / 64 / 2048 problems of 1000 keypoints, 80 lines and 10 neighbours per
keyframe (tests/_localmap_problems.py scenes, every neighbour past the baseline
test), device-resident inputs (orblm_create_new_map_features_batch_device: 8
distinct problems in one keyframe pool, repeated). hipEvents around each launch
on the null stream, one warm-up launch, the median of 20.

Every batch size runs in a child process of its own under a time limit; the
first one that fails or runs out of time ends the run. Writes
profiles/r08/localmap_timing.txt (or the path given as the first argument) with
the commit (the second argument, where the tree is not a git checkout) and the
box.
"""
import subprocess
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))
from _pkg import load_pkg  # noqa: E402

REPS = 20
SIZES = (1, 64, 2048)
LIMIT_S = 240
DISTINCT = 8
STEPS = [1.5, 2.0, 3.0, 1.2, 6.0, 2.2, 12.0, 1.8, 4.0, 8.0]      # multiples of mb, all > 1


def one_size(ns):
    import warnings
    warnings.simplefilter("ignore")
    import _localmap_problems as LP
    from reloc_timing import Events
    pkg = load_pkg()
    cam = pkg.Camera(LP.CAM["fx"], LP.CAM["fy"], LP.CAM["cx"], LP.CAM["cy"], 0, 0, 0, 0, 0,
                     LP.CAM["bf"], 3.0, 640, 480)
    mapper = pkg.LocalMapper(cam, LP.SCALE, LP.SIGMA2)
    nd = min(ns, DISTINCT)
    probs = []
    for k in range(nd):
        sc = LP.Scene(300 + k, 1000, [1000] * 10, steps=STEPS, nl_cur=80)
        probs.append(dict(cur=LP.as_dict(sc.cur), neigh=[LP.as_dict(x) for x in sc.neigh]))
    dev = pkg.LmDeviceProblems(mapper, probs, repeat=max(1, ns // nd))
    assert dev.ns == ns
    ev = Events()
    ev.time(dev.run)                            # warm-up
    ms = float(np.median([ev.time(dev.run) for _ in range(REPS)]))
    out = dev.download()
    pts = np.mean([len(o["points"]) for o in out])
    lns = np.mean([len(o["lines"]) for o in out])
    prs = np.mean([np.maximum(o["pairs"], 0).sum() for o in out])
    print(f"  problems {ns:5d}: {ms:9.4f} ms per launch, {1e3 * ms / ns:10.2f} us per problem "
          f"({prs:.0f} point pairs, {pts:.0f} points and {lns:.0f} lines created per problem)")


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--size":
        one_size(int(sys.argv[2]))
        return
    from reloc_timing import box, commit
    out_path = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles/r08/localmap_timing.txt"
    lines = ["CreateNewMapPoints + CreateNewMapLines kernel, first measurements "
             f"(tools/localmap_timing.py): hipEvents on the null stream, 1 warm-up launch, median of "
             f"{REPS}, one process per batch size.",
             "commit: " + (sys.argv[2] if len(sys.argv) > 2 else commit())] + box() + [""]
    lines.append("k_create_new_map_features, 1000 keypoints, 80 lines, 10 neighbours, one 256-thread "
                 "workgroup per problem")
    for ns in SIZES:
        try:
            r = subprocess.run([sys.executable, __file__, "--size", str(ns)], capture_output=True,
                               text=True, timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            lines.append(f"  problems {ns:5d}: no result within {LIMIT_S} s; stopped here")
            break
        if r.returncode != 0:
            lines.append(f"  problems {ns:5d}: failed with exit status {r.returncode}; stopped here")
            sys.stderr.write(r.stdout + r.stderr)
            break
        lines.append(r.stdout.rstrip("\n"))
    text = "\n".join(lines) + "\n"
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(text)
    print(text)


if __name__ == "__main__":
    main()
