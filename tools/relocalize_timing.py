#!/usr/bin/env python3
"""First timings of the batched Tracking::Relocalization call (no threshold:
nothing has been timed before). orbrl_relocalize (host entry point: packing,
upload, every round, download) at 1 / 64 / 1024 problems, the problems of
tests/_relocalize_problems.py that use 1280 draws at the 1024 pitch, repeated.
Beside them, for one problem, the same relocalisation driven from Python
through the entry points that existed before the call (detect_reloc_batch,
ORBmatcher.SearchByBoW, PnPsolver.iterate, pose_optimization,
ORBmatcher.SearchByProjectionKeyFrame), one candidate after another: the only
way to relocalise without it. hipEvents around each call on the null stream,
one warm-up, the median of 10.

Every batch size runs in a child process of its own under a time limit; the
first one that fails or runs out of time ends the run. Writes
profiles/r09/relocalize_timing.txt (or the path given as the first argument)
with the commit (the second argument, where the tree is not a git checkout)
and the box."""
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
LIMIT_S = 240
NAMES = ("first_search", "direct", "fail_then_win", "round2", "exhaust", "ngood_lt10", "two_win",
         "many_rounds")


def composed(pkg, cam, P, RP):
    """Tracking.cc:2049-2269 over the separate entry points, sequentially"""
    F = P["frame"]
    kps, N = F["kps_un"], len(F["kps_un"])
    inv_sigma2 = (np.float32(1.0) / RP.SIGMA2).astype(np.float32)
    cand = pkg.detect_reloc_batch([dict(kf_bows=P["kf_bows"], covis=P["covis"],
                                        reloc_score=P["reloc_score"], q_words=F["bow_words"],
                                        q_vals=F["bow_vals"])])[0]["cand"]
    m075, m09 = pkg.ORBmatcher(0.75, True), pkg.ORBmatcher(0.9, True)
    solvers, matches, cursor = {}, {}, {}
    for i, k in enumerate(cand):
        kf = P["kfs"][k]
        m, nm = m075.SearchByBoW(kf["feat_node"], kf["valid"], kf["desc"], kf["angle"],
                                 F["feat_node"], F["desc"], kps["angle"])
        if nm < 15:
            continue
        xyz = np.zeros((N, 3), np.float32)
        xyz[m >= 0] = kf["mp_xyz"][m[m >= 0]]
        s = pkg.PnPsolver(cam, np.stack([kps["x"], kps["y"]], 1), RP.SIGMA2[kps["octave"]], xyz,
                          m >= 0)
        s.SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991)
        solvers[i], matches[i], cursor[i] = s, m, 0
    mvp = np.full(N, -1, np.int32)
    outl = np.zeros(N, np.uint8)

    def pose(kf, T):
        nonlocal outl
        xyz = np.zeros((N, 3), np.float32)
        xyz[mvp >= 0] = kf["mp_xyz"][mvp[mvp >= 0]]
        T, outl, _, n = pkg.pose_optimization(cam, dict(kps_un=kps, uright=F["uright"],
                                                        has_mp=(mvp >= 0).astype(np.uint8),
                                                        mp_xyz=xyz, inv_sigma2=inv_sigma2), T, outl)
        return T, n

    def search(kf, T, found, th, dist):
        fm = np.zeros(len(kf["angle"]), np.uint8)
        fm[list(found)] = 1
        m, n = m09.SearchByProjectionKeyFrame(
            cam, RP.SCALE, dict(Tcw=T, kps_un=kps, desc=F["desc"]), (mvp >= 0).astype(np.uint8),
            dict(angle=kf["angle"], valid=kf["valid"], found=fm, mp_xyz=kf["mp_xyz"],
                 mp_min_dist=kf["mp_min_dist"], mp_max_dist=kf["mp_max_dist"],
                 mp_desc=kf["mp_desc"]), th, dist)
        mvp[m >= 0] = m[m >= 0]
        return n

    while solvers:
        for i in sorted(solvers):
            s, kf = solvers[i], P["kfs"][cand[i]]
            need = 4 * max(s.max_its - s.state["iterations"], 5)
            if need > P["draws"].shape[1] - cursor[i]:
                return False
            T, no_more, vb, _ = s.iterate(5, P["draws"][i, cursor[i]:cursor[i] + need])
            cursor[i] += s.last["draws_consumed"]
            if no_more:
                del solvers[i]
            if T is None:
                continue
            mvp[:] = np.where(vb, matches[i], -1)
            found = set(int(v) for v in mvp[mvp >= 0])
            T, g = pose(kf, T)
            if g < 10:
                continue
            mvp[outl != 0] = -1
            if g < 50:
                nadd = search(kf, T, found, 10, 100)
                if nadd + g >= 50:
                    T, g = pose(kf, T)
                    if 30 < g < 50:
                        found = set(int(v) for v in mvp[mvp >= 0])
                        nadd = search(kf, T, found, 3, 64)
                        if g + nadd >= 50:
                            T, g = pose(kf, T)
                            mvp[outl != 0] = -1
            if g >= 50:
                return True
    return False


def one_size(ns):
    import _relocalize_problems as RP
    from reloc_timing import Events
    pkg = load_pkg()
    cam = pkg.make_camera(RP.CFG)
    base = [RP.problems()[n] for n in NAMES]
    ps = [base[k % len(base)] for k in range(ns)]
    rl = pkg.Relocalizer(cam, RP.SCALE, RP.SIGMA2, max_problems=ns, kp_pitch=1024)
    ev = Events()
    res = []

    def call():
        res[:] = rl.relocalize_batch(ps)

    ev.time(call)                               # warm-up
    ms = float(np.median([ev.time(call) for _ in range(REPS)]))
    rounds = max(r["rounds"] for r in res)
    print(f"  problems {ns:5d}: {ms:10.3f} ms per call, {ms / ns:9.4f} ms per problem "
          f"({sum(r['ok'] for r in res)} relocalised, {rounds} rounds, "
          f"{sum(len(r['cand']) for r in res)} candidates)")
    if ns == 1:
        ok = []
        ev.time(lambda: ok.append(composed(pkg, cam, ps[0], RP)))
        cms = float(np.median([ev.time(lambda: ok.append(composed(pkg, cam, ps[0], RP)))
                               for _ in range(REPS)]))
        assert all(o == res[0]["ok"] for o in ok)
        print(f"  the same problem over the separate entry points, from Python: {cms:10.3f} ms "
              f"({cms / ms:.2f} x the call)")


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--size":
        one_size(int(sys.argv[2]))
        return
    from reloc_timing import box, commit
    out_path = (Path(sys.argv[1]) if len(sys.argv) > 1
                else ROOT / "profiles/r09/relocalize_timing.txt")
    lines = ["Batched Tracking::Relocalization, first measurements (tools/relocalize_timing.py): "
             f"hipEvents on the null stream around the host entry point, 1 warm-up call, median of "
             f"{REPS}, one process per batch size.",
             "commit: " + (sys.argv[2] if len(sys.argv) > 2 else commit())] + box() + [""]
    lines.append("orbrl_relocalize, kp_pitch 1024, draw_pitch 1280, problems " + ", ".join(NAMES) +
                 " repeated")
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
