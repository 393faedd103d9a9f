"""KeyFrameCulling and MapPointCulling / MapLineCulling problems (no images): the
culling calls read slots, octaves, the sign of uright, depths and the graph, so
the maps carry placeholder geometry. Hand-built maps of 1 to 6 keyframes and at
most 40 features pin one branch each (see the builders' docstrings); the seeded
scenes draw every keyframe's points from a shared pool, so that most keyframes
are redundant at entry and stop being so as the list is worked off."""
import functools

import numpy as np

import _cull_ref as ref
from _fuse_problems import KP_DTYPE, NLEVELS, SCALE, SIGMA2

CAM = dict(fx=517.306408, fy=516.469215, cx=318.643040, cy=255.313989, bf=40.0)
TH_DEPTH = np.float32(CAM["bf"] * 40.0 / CAM["fx"])   # mThDepth = mbf * ThDepth / fx
NAN = float("nan")


def _pose(k):
    rng = np.random.default_rng(1000 + k)
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    ang = rng.uniform(-0.2, 0.2)
    S = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(ang) * S + (1 - np.cos(ang)) * (S @ S)
    T[:3, 3] = rng.normal(size=3)
    return T.astype(np.float32)


def _row_order(w, ids, k):
    """UpdateBestCovisibles of row k: weight descending, id descending"""
    nb = [j for j in range(len(ids)) if j != k and w[k][j] > 0]
    nb.sort(key=lambda j: (-w[k][j], -ids[j]))
    return nb


def build(ids, feats, cur, weights=None, ordered=None, parent=None, not_erase=(), kf_bad=(), ref=None,
          bad_points=()):
    """a problem from feats[k] = [(point or -1, octave, stereo, depth)] per keyframe.
    Defaults: weights = shared points (symmetric, bad keyframes none), ordered =
    every row in full, parent = the keyframe with the lowest id (itself: none),
    ref_kf = a point's first observer in table order. weights / ordered / parent /
    ref are dicts of overrides."""
    K = len(ids)
    M = 1 + max([f[0] for fs in feats for f in fs] + [-1])
    kfs, depth = [], []
    for k, fs in enumerate(feats):
        n = len(fs)
        kp = np.zeros(n, KP_DTYPE)
        kp["x"], kp["y"] = 100.0 + np.arange(n), 100.0 + k
        kp["octave"] = [f[1] for f in fs]
        ur = np.array([kp["x"][i] - 10.0 if f[2] else -1.0 for i, f in enumerate(fs)], np.float32).reshape(n)
        kfs.append(dict(id=int(ids[k]), Tcw=_pose(k), kps_un=kp, uright=ur, desc=np.zeros((n, 32), np.uint8),
                        mp=np.array([f[0] for f in fs], np.int32).reshape(n), ordered=[]))
        depth.append(np.array([f[3] for f in fs], np.float32).reshape(n))
    kb = np.zeros(K, np.uint8)
    kb[list(kf_bad)] = 1
    seen = [[k for k in range(K) if not kb[k] and p in kfs[k]["mp"]] for p in range(M)]
    w = np.zeros((K, K), np.int32)
    for ks in seen:
        for a in ks:
            for b in ks:
                w[a, b] += a != b
    for (a, b), v in (weights or {}).items():
        w[a, b] = v
    root = int(np.argmin(ids))
    par = np.array([-1 if k == root else root for k in range(K)], np.int32)
    for k, v in (parent or {}).items():
        par[k] = v
    order = [_row_order(w, ids, k) for k in range(K)]
    for k, v in (ordered or {}).items():
        order[k] = list(v)
    bad = np.zeros(M, np.uint8)
    bad[list(bad_points)] = 1
    ref_kf = np.array([s[0] if s else 0 for s in seen], np.int32).reshape(M)
    for p, v in (ref or {}).items():
        ref_kf[p] = v
    ne = np.zeros(K, np.uint8)
    ne[list(not_erase)] = 1
    m = dict(kfs=kfs, xyz=np.tile(np.float32([0, 0, 4]), (M, 1)), normal=np.tile(np.float32([0, 0, 1]), (M, 1)),
             min_dist=np.ones(M, np.float32), max_dist=np.full(M, 10, np.float32),
             desc=np.zeros((M, 32), np.uint8), ref_kf=ref_kf, bad=bad, n_visible=np.full(M, 3, np.int32),
             n_found=np.full(M, 2, np.int32))
    return dict(map=m, cur=cur, depth=depth, conn_w=w, ordered=order, parent=par, not_erase=ne, kf_bad=kb)


def R(p, octave=0, depth=1.0, stereo=True):
    return (p, octave, stereo, depth)


def thresh(nmps, nred, **kw):
    """A(id 0), B, C, K(id 5), cur(id 9, no features, list = [K]): K holds nmps
    counted points, the first nred of them also in A, B and C (redundant), the
    rest in A only (Observations() = 4, one other observer)."""
    allp, red = [R(p) for p in range(nmps)], [R(p) for p in range(nred)]
    return build([0, 3, 4, 5, 9], [allp, red, red, allp, []], 4, weights={(4, 3): 20, (3, 4): 20},
                 ordered={4: [3]}, **kw)


def gates():
    """K = keyframe 3 (list = [K]); per slot of K:
    0 depth == th_depth: counted, redundant      1 just above th_depth: skipped
    2 negative depth: skipped                    3 NaN depth: counted, redundant
    4 Observations() == 3 (K stereo, A mono)     5 Observations() == 4 (K, A stereo)
    6 K at octave 2, A B C at 3: redundant       7 K at 2, A B at 3, C at 4: not
    8 no point                                   -> nMPs 6, redundant 3, kept"""
    above = float(np.nextafter(TH_DEPTH, np.float32(10)))
    K = [R(0, depth=float(TH_DEPTH)), R(1, depth=above), R(2, depth=-0.5), R(3, depth=NAN), R(4), R(5),
         R(6, 2), R(7, 2), R(-1)]
    A = [R(0), R(1), R(2), R(3), R(4, stereo=False), R(5), R(6, 3), R(7, 3)]
    B = [R(0), R(1), R(2), R(3), R(6, 3), R(7, 3)]
    C = [R(0), R(1), R(2), R(3), R(6, 3), R(7, 4)]
    return build([0, 3, 4, 5, 9], [A, B, C, K, []], 4, weights={(4, 3): 20, (3, 4): 20}, ordered={4: [3]})


def first():
    """a fully redundant keyframe with mnId == 0 in the list: skipped"""
    red = [R(p) for p in range(10)]
    return build([8, 3, 4, 0, 9], [red, red, red, red, []], 4, weights={(4, 3): 20, (3, 4): 20},
                 ordered={4: [3]})


def order_pair(reverse):
    """K1 (index 2) and K2 (index 3) are each redundant only through the other:
    ten points in A, B, K1, K2. The first in the list is culled, the second then is not."""
    red = [R(p) for p in range(10)]
    lst = [3, 2] if reverse else [2, 3]
    return build([0, 3, 5, 6, 9], [red, red, red, red, []], 4,
                 weights={(4, 2): 20, (4, 3): 20, (2, 4): 20, (3, 4): 20}, ordered={4: lst})


def goes_bad():
    """K = index 3 (ids: A 8, B 0, C 4): 28 redundant points whose ref_kf is K (handed
    to B, the lowest id left, not the first in the table), point 28 in K and A
    only (stereo both: 4 -> 2 observations, goes bad, A's slot cleared, K's own
    slot kept), point 29 in K alone (mono: ref_kf -1, bad). 28 > 0.9 * 30: culled."""
    red = [R(p) for p in range(28)]
    return build([8, 0, 4, 5, 9], [red + [R(28)], red, red, red + [R(28), R(29, stereo=False)], []], 4,
                 weights={(4, 3): 20, (3, 4): 20}, ordered={4: [3]}, ref={p: 3 for p in range(30)})


def tree_chain():
    """P(0) K(5) C1(11) C2(12) C3(13) cur(30); C1, C2, C3 are K's children. C1 sees P
    and attaches to it; C2's list names C1 (no weight: GetWeight 0) and attaches
    once C1 is a candidate; C3 sees nobody and falls to P. K's row lists C3 (which
    does not list K: nothing erased there) but not C2 (whose row and list stay)."""
    red = [R(p) for p in range(10)]
    w = {(a, b): 0 for a in range(6) for b in range(6)}
    w.update({(1, 0): 10, (1, 2): 10, (1, 5): 20, (1, 4): 7, (0, 1): 10, (0, 2): 10, (0, 3): 10,
              (2, 1): 10, (2, 0): 10, (2, 3): 10, (3, 1): 10, (5, 1): 20})
    return build([0, 5, 11, 12, 13, 30], [red, red, red, red, [], []], 5, weights=w,
                 ordered={0: [1, 2, 3], 1: [5, 0, 2], 2: [1, 0, 3], 3: [1, 2], 4: [], 5: [1]},
                 parent={1: 0, 2: 1, 3: 1, 4: 1, 5: 0})


def tree_tie():
    """P(0) K(5) C2(12) C1(11) cur(30), the children out of id order in the table:
    C1 and C2 both reach P at weight 20, C1 (lower id) goes first; C2 then finds
    C1 and P at 20 and takes the first of its list, C1."""
    red = [R(p) for p in range(10)]
    w = {(a, b): 0 for a in range(5) for b in range(5)}
    w.update({(1, 0): 10, (1, 2): 10, (1, 3): 10, (1, 4): 20, (4, 1): 20, (0, 1): 10,
              (3, 1): 10, (3, 0): 20, (2, 1): 10, (2, 3): 20, (2, 0): 20})
    return build([0, 5, 12, 11, 30], [red, red, red, red, []], 4, weights=w,
                 ordered={0: [1], 1: [4, 0, 2, 3], 2: [3, 0, 1], 3: [0, 1], 4: [1]},
                 parent={1: 0, 2: 1, 3: 1, 4: 0})


def asym():
    """thresh(10, 10) with rows that disagree: A's list names K but its row does
    not (A keeps K), B's list is its >= 15 subset [A, K] of the row {A 30, K 20,
    C 5} and becomes [A, C], C's only connection is K"""
    p = thresh(10, 10)
    p["conn_w"] = _w(5, {(3, 0): 10, (3, 1): 10, (3, 2): 10, (3, 4): 20, (4, 3): 20, (1, 3): 20, (1, 0): 30,
                         (1, 2): 5, (2, 3): 10})
    p["ordered"] = [[3], [0, 3], [3], [4, 1, 0, 2], [3]]
    return p


def _w(K, d):
    w = np.zeros((K, K), np.int32)
    for (a, b), v in d.items():
        w[a, b] = v
    return w


def bad_entry():
    """A(0) B(3) Kb(5) Kd(6) Ko(7) cur(9). Kb and Ko are bad at entry and sit in the
    list: their slots still name ten points that A, B and cur observe (and a bad
    point), their rows are empty. Both are processed as written and culled again:
    nothing changes but mTcp (Ko has no parent: not even that). Kd, bad too, is
    Kb's child: skipped in the loop, then handed to Kb's parent."""
    red = [R(p) for p in range(10)]
    return build([0, 3, 5, 6, 7, 9], [red, red, red + [R(10)], [], red[:5], red], 5,
                 ordered={5: [2, 4, 0, 1]}, parent={2: 0, 3: 2, 4: -1}, kf_bad=[2, 3, 4], bad_points=[10])


def nkf1():
    return build([0], [[R(0), R(1, stereo=False)]], 0)


def nkf2():
    """cur(0) and K(5): three points in both, one other observer each: kept"""
    three = [R(p) for p in range(3)]
    return build([0, 5], [three, three], 0)


def scene(seed, K, N, pool=1.5, full_list=False, jitter=2):
    """K keyframes of N features: a keyframe's points are N draws (less a tenth
    of empty slots) from a pool of pool * N, so a point has about K / pool
    observers. Non-current rows keep only their stronger weights and their lists
    only the strongest (UpdateConnections' >= 15 rule, scaled to the scene)."""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(K) * 3
    cur = int(np.argmax(ids))
    npool = max(1, int(N * pool))
    base = rng.integers(0, 5, npool)
    feats = []
    for k in range(K):
        n_pts = min(npool, N - N // 10)
        pts = list(rng.choice(npool, n_pts, replace=False)) + [-1] * (N - n_pts)
        rng.shuffle(pts)
        fs = []
        for p in pts:
            d = rng.uniform(0.4, float(TH_DEPTH) * 1.25)
            if rng.random() < 0.03:
                d = -1.0
            fs.append((int(p), int(np.clip(base[p] + rng.integers(-1, jitter), 0, NLEVELS - 1)) if p >= 0 else 0,
                       rng.random() < 0.85, d))
        feats.append(fs)
    used = sorted({f[0] for fs in feats for f in fs if f[0] >= 0})
    dense = {p: i for i, p in enumerate(used)}
    feats = [[(dense.get(f[0], -1),) + f[1:] for f in fs] for fs in feats]
    M = len(used)
    prob = build(list(ids), feats, cur, bad_points=list(rng.choice(M, max(1, M // 50), replace=False)) if M else ())
    w = prob["conn_w"]
    pos = w[w > 0]
    lo, hi = (np.percentile(pos, 30), np.percentile(pos, 60)) if len(pos) else (0, 0)
    order = []
    for k in range(K):
        if k == cur:
            if full_list:
                w[k, :] += 1
                w[k, k] = 0
        else:
            w[k, w[k] < lo] = 0
        keep = w.copy()
        if k != cur:
            keep[k, keep[k] < hi] = 0
        order.append(_row_order(keep, ids, k))
    by_id = np.argsort(ids)
    par = np.full(K, -1, np.int32)
    for r in range(1, K):
        k, older = int(by_id[r]), by_id[:r]
        par[k] = int(older[np.argmax([w[k, j] for j in older])])
    ref_kf = prob["map"]["ref_kf"]
    sets = [set(f[0] for f in fs) for fs in feats]
    for p in range(M):
        obs = [k for k in range(K) if p in sets[k]]
        ref_kf[p] = obs[int(rng.integers(len(obs)))]
    prob.update(ordered=order, parent=par, not_erase=(rng.random(K) < 0.1).astype(np.uint8))
    return prob


_BUILDERS = {
    "nkf1": nkf1,
    "nkf2": nkf2,
    "t10_9": lambda: thresh(10, 9),
    "t10_10": lambda: thresh(10, 10),
    "t20_18": lambda: thresh(20, 18),
    "t20_19": lambda: thresh(20, 19),
    "nmps0": lambda: thresh(0, 0),
    "gates": gates,
    "first": first,
    "not_erase": lambda: thresh(10, 10, not_erase=[3]),
    "order_ab": lambda: order_pair(False),
    "order_ba": lambda: order_pair(True),
    "goes_bad": goes_bad,
    "tree_chain": tree_chain,
    "tree_tie": tree_tie,
    "asym": asym,
    "bad_entry": bad_entry,
    "k64": lambda: scene(31, 64, 32, pool=8.0, full_list=True),
    "n2048": lambda: scene(32, 5, 2048, pool=1.0, jitter=1),
    "s8": lambda: scene(33, 8, 300, pool=1.1),
    "s12": lambda: scene(34, 12, 300, pool=1.3, jitter=3),
}
NAMES = tuple(_BUILDERS)
HAND = NAMES[:NAMES.index("k64")]


@functools.lru_cache(maxsize=None)
def problem(name):
    return _BUILDERS[name]()


@functools.lru_cache(maxsize=None)
def ref_run(name):
    """(result, stats) of the restatement, computed once"""
    return ref.keyframe_culling(problem(name), TH_DEPTH)


def _lines(rng, K, cur_id, L, per_kf):
    ml = []
    for _ in range(K):
        n = int(rng.integers(0, per_kf + 1)) if L else 0
        row = rng.choice(L, min(n, L), replace=False) if L else np.zeros(0, np.int64)
        ml.append(np.where(rng.random(len(row)) < 0.2, -1, row).astype(np.int32))
    first = cur_id - rng.integers(0, 5, L)
    first[rng.random(L) < 0.1] = -1
    return dict(ml=ml, bad=(rng.random(L) < 0.1).astype(np.uint8), n_visible=rng.integers(0, 6, L).astype(np.int32),
                n_found=rng.integers(0, 4, L).astype(np.int32), first_kf=first.astype(np.int32),
                n_obs=rng.integers(1, 7, L).astype(np.int32))


def rc_hand():
    """the `gates` map (Observations(): point 4 has 3, point 5 has 4, the rest of
    0-7 have 8), cur_id 9; the expected reasons are written out in test_cull_ref.py"""
    p = gates()
    m = dict(p["map"])
    #                     0  1  2  3  4  5  6  7
    m["bad"] = np.uint8([1, 0, 0, 0, 0, 0, 0, 0])
    m["n_found"] = np.int32([2, 1, 1, 0, 2, 2, 2, 2])
    m["n_visible"] = np.int32([3, 5, 4, 0, 0, 3, 3, 3])
    first_kf = np.int32([9, 9, 9, 6, 7, 7, 6, 7])
    lines = dict(ml=[np.int32([0, 1, 2]), np.int32([1, -1, 3]), np.int32([4, 5]), np.int32([5, 2]),
                     np.zeros(0, np.int32)],
                 bad=np.uint8([1, 0, 0, 0, 0, 1]), n_visible=np.int32([3, 3, 3, 3, 3, 3]),
                 n_found=np.int32([2, 0, 2, 2, 2, 2]), first_kf=np.int32([9, 9, -1, -1, 8, 0]),
                 n_obs=np.int32([5, 5, 3, 4, 1, 1]))
    return dict(map=m, cur_id=9, first_kf=first_kf, recent=np.int32([0, 1, 2, 3, 4, 5, 6, 7]), lines=lines,
                recent_lines=np.int32([4, 3, 2, 1, 0]))


def rc_empty():
    """empty lists and a line table with L = 0"""
    p = thresh(10, 9)
    K = len(p["map"]["kfs"])
    return dict(map=p["map"], cur_id=9, first_kf=np.full(10, 9, np.int32), recent=np.zeros(0, np.int32),
                lines=_lines(np.random.default_rng(0), K, 9, 0, 0), recent_lines=np.zeros(0, np.int32))


def rc_seeded(name, n_recent=None):
    """the culling problem's map with seeded counters, ages, lists and lines"""
    p = problem(name)
    rng = np.random.default_rng(sum(map(ord, name)))
    m = dict(p["map"])
    M, K = len(m["bad"]), len(m["kfs"])
    cur_id = int(m["kfs"][p["cur"]]["id"])
    m["n_visible"] = rng.integers(0, 6, M).astype(np.int32)
    m["n_found"] = rng.integers(0, 4, M).astype(np.int32)
    n = min(M, (M + 1) // 2 if n_recent is None else n_recent)
    L = K * 6
    return dict(map=m, cur_id=cur_id, kf_bad=p["kf_bad"], first_kf=(cur_id - rng.integers(0, 5, M)).astype(np.int32),
                recent=rng.permutation(M)[:n].astype(np.int32), lines=_lines(rng, K, cur_id, L, 10),
                recent_lines=rng.permutation(L)[:L // 2].astype(np.int32))


RC_NAMES = ("rc_hand", "rc_empty", "rc_2048") + NAMES


@functools.lru_cache(maxsize=None)
def recent_problem(name):
    if name == "rc_hand":
        return rc_hand()
    if name == "rc_empty":
        return rc_empty()
    if name == "rc_2048":
        return rc_seeded("n2048", 2048)
    return rc_seeded(name)


@functools.lru_cache(maxsize=None)
def recent_ref_run(name):
    return ref.cull_recent(recent_problem(name))
