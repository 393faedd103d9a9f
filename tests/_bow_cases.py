"""Hand-built vocabularies and features for the DBoW2 transform, shared by
test_bow_ref.py (CPU: oracle against the restatement tests/_bow_ref.py) and
test_gpu_bow_cases.py (GPU: k_bow_words / k_bow_vector against both).

A case is (name, arrays, features, levelsups) plus `aim`: facts the case was
built for, checked on the restatement's result so that a case cannot quietly
stop reaching its branch. Everything is seeded; nothing is trained or
rendered. Vocabularies are shared between cases as one `arrays` object, so a
test can keep one loaded vocabulary per object."""
import functools
from collections import namedtuple

import numpy as np

import _bow_ref as R

Case = namedtuple("Case", "name arrays feats levelsups aim")

MAX_FEAT = 4096            # features per frame the transform accepts
MAX_WORDS = (1 << 20) - 1  # words the library accepts (DESIGN.md, f3 limits)


def make_arrays(parent, leaf, desc, weight, k, L, scoring=0, weighting=0):
    return dict(parent=np.asarray(parent, np.int32), leaf=np.asarray(leaf, np.uint8),
                desc=np.ascontiguousarray(desc, np.uint8).reshape(-1, 32),
                weight=np.asarray(weight, np.float64), k=k, L=L, scoring=scoring,
                weighting=weighting)


def with_kind(arrays, scoring, weighting, **more):
    a = dict(arrays)
    a.update(scoring=scoring, weighting=weighting, **more)
    return a


def hadamard(i, nbits=256):
    """Codeword i (1 <= i < nbits) of the Hadamard code as bytes: any two
    differ in exactly nbits / 2 bits and each has nbits / 2 bits set."""
    assert 1 <= i < nbits
    bits = np.array([bin(i & j).count("1") & 1 for j in range(nbits)], np.uint8)
    return np.packbits(bits)


def with_bits(nbits, start=0, base=None):
    """`base` (default zeros) with bits start .. start + nbits - 1 inverted."""
    bits = np.zeros(256, np.uint8) if base is None else np.unpackbits(np.asarray(base, np.uint8))
    bits[start:start + nbits] ^= 1
    return np.packbits(bits)


class Builder:
    """A tree grown node by node; `finish` flags the childless nodes that
    were not given a flag by hand."""

    def __init__(self):
        self.parent, self.leaf, self.desc, self.weight = [-1], [0], [np.zeros(32, np.uint8)], [0.0]

    def add(self, parent, desc, weight=1.0, leaf=None):
        assert 0 <= parent < len(self.parent)
        self.parent.append(parent)
        self.leaf.append(leaf)
        self.desc.append(np.asarray(desc, np.uint8))
        self.weight.append(weight)
        return len(self.parent) - 1

    def finish(self, k, L, scoring=0, weighting=0):
        has_child = set(self.parent[1:])
        leaf = [(0 if i in has_child else 1) if f is None else f for i, f in enumerate(self.leaf)]
        return make_arrays(self.parent, leaf, np.stack(self.desc), self.weight, k, L, scoring,
                           weighting)


def word_of(arrays, node):
    leaf = np.asarray(arrays["leaf"]).astype(bool).copy()
    leaf[0] = False
    return int(np.cumsum(leaf)[node] - 1) if leaf[node] else 0


# --------------------------------------------------------------------------
# 1. sibling order: one random tree numbered three ways
# --------------------------------------------------------------------------
def _random_tree(seed):
    """Mixed fan-out, depth up to 4, children lists in a canonical order.
    Weights are multiples of 1/4, so that every sum is exact and the three
    numberings give the same values whatever the word order."""
    rng = np.random.default_rng(seed)
    kids = {0: []}
    depth = {0: 0}
    frontier, nxt = [0], 1
    while frontier:
        p = frontier.pop(0)
        if depth[p] == 4:
            continue
        fan = 5 if p == 0 else int(rng.choice([0, 0, 1, 2, 3, 7, 12]))
        if nxt + fan > 260:
            fan = 0
        for _ in range(fan):
            kids[p].append(nxt)
            kids[nxt] = []
            depth[nxt] = depth[p] + 1
            frontier.append(nxt)
            nxt += 1
    n = nxt
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    weight = rng.choice([0.0, 0.25, 0.5, 1.0, 1.5, 2.0], n)
    return kids, desc, weight


def _numbering(kids, how, seed):
    """canonical ids in the order they are numbered: order[new] = canonical.
    Siblings keep their relative order in every numbering (ties break the
    same way); in "interleaved" other nodes' children come between them."""
    if how == "bfs":
        order, q = [], [0]
        while q:
            p = q.pop(0)
            order.append(p)
            q.extend(kids[p])
        return order
    if how == "dfs":
        order, st = [], [0]
        while st:
            p = st.pop()
            order.append(p)
            st.extend(reversed(kids[p]))
        return order
    rng = np.random.default_rng(seed)
    order, nxt = [0], {0: 0}
    open_parents = [0] if kids[0] else []
    while open_parents:
        p = open_parents[int(rng.integers(len(open_parents)))]
        c = kids[p][nxt[p]]
        nxt[p] += 1
        if nxt[p] == len(kids[p]):
            open_parents.remove(p)
        order.append(c)
        if kids[c]:
            nxt[c] = 0
            open_parents.append(c)
    return order


@functools.lru_cache(None)
def sibling_order_cases():
    """-> [(case, order)] with order[new id] = canonical id."""
    kids, desc, weight = _random_tree(101)
    par = {c: p for p, cs in kids.items() for c in cs}
    rng = np.random.default_rng(102)
    n = len(desc)
    src = rng.integers(1, n, 300)
    feats = desc[src].copy()
    for i in range(len(feats)):          # a few flipped bits: near a node, not on it
        for b in rng.integers(0, 256, int(rng.integers(0, 40))):
            feats[i, b >> 3] ^= 1 << (b & 7)
    feats[::7] = rng.integers(0, 256, (len(feats[::7]), 32), dtype=np.uint8)
    out = []
    for how in ("bfs", "dfs", "interleaved"):
        order = _numbering(kids, how, 103)
        new = {c: i for i, c in enumerate(order)}
        parent = [-1] + [new[par[c]] for c in order[1:]]
        assert all(p < i for i, p in enumerate(parent))
        leaf = [0] + [0 if kids[c] else 1 for c in order[1:]]
        a = make_arrays(parent, leaf, desc[order], weight[order], 12, 4)
        out.append((Case(f"siblings_{how}", a, feats, (0, 1, 2, 4), None), order))
    # the interleaved numbering really separates siblings
    p = np.asarray(out[2][0].arrays["parent"])[1:]
    assert np.any(np.diff(p) < 0)
    return out


# --------------------------------------------------------------------------
# 2. fan-out across the kBowBatch = 10 boundary
# --------------------------------------------------------------------------
FANOUTS = (1, 2, 9, 10, 11, 19, 20)


@functools.lru_cache(None)
def fanout_cases():
    rng = np.random.default_rng(201)
    b = Builder()
    top = [b.add(0, hadamard(1 + j), weight=0.5 + 0.125 * j) for j in range(20)]
    groups = {}
    def near(code):
        """40 random bit positions of `code` flipped (repeats cancel): within
        40 of its parent, at least 88 from every other level-1 node."""
        bits = np.unpackbits(code)
        for p in rng.integers(0, 256, 40):
            bits[p] ^= 1
        return np.packbits(bits)

    for j, fan in enumerate(FANOUTS):
        groups[fan] = [b.add(top[j], near(b.desc[top[j]]), weight=float(rng.uniform(0.5, 2.0)))
                       for _ in range(fan)]
    a20 = b.finish(20, 2)
    leaves = [i for i in range(1, len(a20["parent"])) if a20["leaf"][i]]
    feats = a20["desc"][leaves].copy()
    noisy = feats.copy()
    noisy[:, 31] ^= 0x81
    feats = np.concatenate([feats, noisy])
    want = np.array([word_of(a20, x) for x in leaves] * 2)

    def aim(res, levelsup):
        assert np.array_equal(res.feat_word, want)       # every child of every node is reached
        assert {len(p) for p in res.paths} == {1, 2}

    small = with_kind(a20, 0, 0, k=9)       # header k below the largest fan-out: not checked
    return [Case("fanout_k20", a20, feats, (0, 1, 2), aim),
            Case("fanout_header_k9", small, feats, (0, 1), aim)]


# --------------------------------------------------------------------------
# 3. ties and distance extremes
# --------------------------------------------------------------------------
def _selector(g):
    """Byte 24 + g set: features and the nodes of group g share it, so the
    walk enters group g with distance 0 against 16 for any other group."""
    d = np.zeros(32, np.uint8)
    d[24 + g] = 0xFF
    return d


@functools.lru_cache(None)
def tie_cases():
    b = Builder()
    groups = [b.add(0, _selector(g), weight=0.0) for g in range(6)]
    feats, want = [], []

    def child(g, nbits, start):
        d = with_bits(nbits, start)
        d[24 + g] = 0xFF
        return d

    # groups 0-2: 20 children at distance 40, two of them at 17
    for g, (i, j) in enumerate([(3, 12), (9, 10), (0, 19)]):
        ids = [b.add(groups[g], child(g, 17 if q in (i, j) else 40, q), weight=1.0 + q)
               for q in range(20)]
        feats.append(_selector(g))
        want.append(ids[i])
    # group 3: all 20 children equal
    ids = [b.add(groups[3], child(3, 9, 5), weight=1.0 + q) for q in range(20)]
    feats.append(_selector(3))
    want.append(ids[0])
    # group 4: duplicate children in pairs (60, 60, 58, 58, ...), the nearest
    # pair at positions (12, 13), then one far child
    ids = [b.add(groups[4], child(4, 60 - 2 * (q // 2) if q < 14 else 90, 3), weight=1.0 + q)
           for q in range(15)]
    feats.append(_selector(4))
    want.append(ids[12])
    # group 5: distances 0 and 256
    ones = np.full(32, 0xFF, np.uint8)
    f5 = _selector(5)
    far = ones ^ f5                   # the complement of the feature: distance 256
    i_far = b.add(groups[5], far, weight=3.0)
    i_far2 = b.add(groups[5], far, weight=4.0)
    i_hit = b.add(groups[5], f5, weight=5.0)
    feats.append(f5)
    want.append(i_hit)               # 256, 256, 0
    a = b.finish(20, 2)
    # a vocabulary whose every node is at distance 256: the first child wins
    b2 = Builder()
    b2.add(0, ones, weight=1.0)
    b2.add(0, ones, weight=2.0)
    a2 = b2.finish(2, 1)
    assert i_far < i_far2 < i_hit
    feats = np.stack(feats)
    want = np.array(want)

    def aim(res, levelsup):
        assert [p[-1] for p in res.paths] == want.tolist()

    def aim2(res, levelsup):
        assert [p[-1] for p in res.paths] == [1, 1, 1]

    return [Case("ties", a, feats, (0, 1), aim),
            Case("all_256", a2, np.zeros((3, 32), np.uint8), (0,), aim2)]


@functools.lru_cache(None)
def one_bit_case():
    """16 nodes R_g (Hadamard codewords), each with the children R_g ^ one bit
    of byte 2g, R_g ^ one bit of byte 2g + 1, and R_g itself. The feature R_g
    belongs to the third; a distance that misses byte 2g or 2g + 1 (or its
    word) sees a tie at 0 and takes an earlier child."""
    b = Builder()
    feats, want = [], []
    for g in range(16):
        r = hadamard(3 + 5 * g)
        top = b.add(0, r, weight=0.0)
        kids = []
        for byte in (2 * g, 2 * g + 1):
            d = r.copy()
            d[byte] ^= 1 << (byte % 8)
            kids.append(b.add(top, d, weight=1.0 + byte))
        kids.append(b.add(top, r, weight=40.0 + g))
        for q in range(3):
            feats.append(b.desc[kids[q]])
            want.append(kids[q])
    a = b.finish(16, 2)
    want = np.array(want)

    def aim(res, levelsup):
        assert [p[-1] for p in res.paths] == want.tolist()

    return Case("one_bit_per_byte", a, np.stack(feats), (0, 1), aim)


# --------------------------------------------------------------------------
# 4. unbalanced trees (P20)
# --------------------------------------------------------------------------
@functools.lru_cache(None)
def unbalanced_case(L):
    """A comb: at every level one leaf A_d and one inner node B_d (both
    leaves at level L). Level d owns bytes 3(d-1) .. 3d-1: set in B_d, clear
    in A_d. The feature for depth d has the regions of levels 1 .. d-1 set."""
    b = Builder()
    node, a_of = 0, {}
    for d in range(1, L + 1):
        region = np.zeros(32, np.uint8)
        region[3 * (d - 1):3 * d] = 0xFF
        a_of[d] = b.add(node, np.zeros(32, np.uint8), weight=1.0 + 0.5 * d)
        node = b.add(node, region, weight=0.25 if d == L else 0.0)
    a_of[L + 1] = node                 # the B leaf at level L
    feats = np.zeros((L + 1, 32), np.uint8)
    for d in range(1, L + 2):
        feats[d - 1, :3 * (d - 1)] = 0xFF
    a = b.finish(2, L)
    depth = list(range(1, L + 1)) + [L]

    def aim(res, levelsup):
        assert [len(p) for p in res.paths] == depth
        assert [p[-1] for p in res.paths] == [a_of[d] for d in range(1, L + 2)]
        lvl = L - levelsup
        for i, p in enumerate(res.paths):
            want = 0 if lvl <= 0 else (p[lvl - 1] if lvl <= len(p) else p[-1])
            assert res.feat_node[i] == want
        # the leaf lies above, at and below level L - levelsup within one frame
        if 1 < lvl < L:
            assert min(depth) < lvl < max(depth)

    return Case(f"unbalanced_L{L}", a, feats, tuple(range(0, L + 2)), aim)


# --------------------------------------------------------------------------
# 5. leaf flags and stop words
# --------------------------------------------------------------------------
@functools.lru_cache(None)
def flag_cases():
    b = Builder()
    n1 = b.add(0, hadamard(1), weight=1.0, leaf=1)             # word 0
    n2 = b.add(0, hadamard(2), weight=0.5, leaf=0)             # childless, no flag: word 0 too
    n3 = b.add(0, hadamard(3), weight=9.0, leaf=1)             # word 1, but has children
    n4 = b.add(0, hadamard(4), weight=0.0, leaf=1)             # word 2, stopped
    n5 = b.add(0, hadamard(5), weight=-1.0, leaf=1)            # word 3, stopped
    n6 = b.add(n3, with_bits(20, 0, hadamard(3)), weight=2.0, leaf=1)      # word 4
    n7 = b.add(n3, with_bits(30, 100, hadamard(3)), weight=0.75, leaf=1)   # word 5
    tf = b.finish(5, 2, scoring=0, weighting=0)
    idf = with_kind(tf, 5, 2)           # addIfNotExist: word 0 keeps its first feature's weight
    order = [n2, n1, n4, n7, n5, n1, n2, n6, n3, n4]
    feats = np.stack([b.desc[x] for x in order])
    final = [n2, n1, n4, n7, n5, n1, n2, n6, n6, n4]       # n3 is walked through (20 < 30)
    words = [0, 0, 2, 5, 3, 0, 0, 4, 4, 2]

    def aim(res, levelsup):
        assert [p[-1] for p in res.paths] == final
        assert res.feat_word.tolist() == words
        assert res.bow_words.tolist() == [0, 4, 5]          # word 1 is never produced
        assert (res.feat_node < 0).tolist() == [x in (n4, n5) for x in final]

    def aim_idf(res, levelsup):
        aim(res, levelsup)
        assert res.bow_vals.tolist() == [0.5, 2.0, 0.75]    # not 1.0: n2 came first

    stopped = np.stack([b.desc[x] for x in (n4, n5, n5, n4, n4)])

    def aim_stopped(res, levelsup):
        assert len(res.bow_words) == 0 and np.all(res.feat_node == -1)

    return [Case("flags_tf", tf, feats, (0, 1, 2), aim),
            Case("flags_idf", idf, feats, (0, 1), aim_idf),
            Case("flags_all_stopped", tf, stopped, (0, 1), aim_stopped)]


# --------------------------------------------------------------------------
# 6. BowVector assembly
# --------------------------------------------------------------------------
ASSEMBLY_N = (0, 1, 2, 255, 256, 257, 1000, 4095, 4096)


@functools.lru_cache(None)
def assembly_vocabulary():
    """Complete tree, k = 16, L = 3: 4096 words (one per feature of a full
    frame), 4369 nodes in breadth-first order. Level l owns bytes 8(l-1) ..
    8l-1, child j of a node holds codeword j of the 64-bit Hadamard code
    there, so the leaf's own descriptor walks to it with distance 0 against
    32. Every 7th word is stopped."""
    rng = np.random.default_rng(601)
    codes = np.stack([hadamard(1 + j, 64) for j in range(16)])       # 16 x 8 bytes
    parent, desc = [-1], [np.zeros(32, np.uint8)]
    level = [0]
    for l in range(1, 4):
        nxt = []
        for p in level:
            for j in range(16):
                d = desc[p].copy()
                d[8 * (l - 1):8 * l] = codes[j]
                parent.append(p)
                desc.append(d)
                nxt.append(len(parent) - 1)
        level = nxt
    n = len(parent)
    leaf = np.zeros(n, np.uint8)
    leaf[level] = 1
    weight = np.zeros(n)
    weight[level] = rng.uniform(0.05, 3.0, len(level))
    weight[level[3::7]] = 0.0
    a = make_arrays(parent, leaf, np.stack(desc), weight, 16, 3)
    return a, np.array(level)


def _assembly_feats(kind, n, seed):
    a, leaves = assembly_vocabulary()
    rng = np.random.default_rng(seed)
    live = leaves[a["weight"][leaves] > 0]
    dead = leaves[a["weight"][leaves] <= 0]
    if kind == "one_word":
        pick = np.full(n, live[len(live) // 3])
    elif kind == "own_word":
        pick = rng.permutation(leaves)[:n]
    else:
        # runs of one word in the sorted keys, their lengths around the span a
        # thread owns (per = np / 256 sorted positions), a wave of spans
        # (64 * per) and one position; shuffled over the frame
        np2 = 1
        while np2 < n:
            np2 <<= 1
        per = max(1, np2 // 256)
        lens = [per - 1, per, per + 1, 1, 2 * per + 1, 1, 1, 3, 64 * per - 2 * per - 9, 5, 63, 64, 65,
                2, 1, 64 * per + 1, 7]
        words = np.sort(rng.permutation(live)[:512])
        pick, q = [], 0
        while len(pick) < n:
            m = max(1, lens[q % len(lens)] if q < 3 * len(lens) else int(rng.integers(1, 2 * per + 3)))
            pick += [words[q % len(words)]] * m
            q += 1
        pick = rng.permutation(np.array(pick[:n]))
    pick = np.array(pick, np.int64)
    if n > 2:
        pick[2::5] = dead[rng.integers(0, len(dead), len(pick[2::5]))]   # stopped, interleaved
    return a["desc"][pick].copy() if n else np.zeros((0, 32), np.uint8)


@functools.lru_cache(None)
def assembly_cases():
    a, _ = assembly_vocabulary()
    out = []
    for kind in ("one_word", "own_word", "runs"):
        for n in ASSEMBLY_N:
            feats = _assembly_feats(kind, n, 610 + n)

            def aim(res, levelsup, kind=kind, n=n):
                kept = res.feat_node >= 0
                if n > 2:
                    assert 0 < (~kept).sum() < n
                if kind == "one_word":
                    assert len(res.bow_words) == min(n, 1)
                if kind == "own_word":
                    assert len(res.bow_words) == kept.sum()
                if kind == "runs" and n >= 1000:
                    runs = np.bincount(res.feat_word[kept])
                    assert runs.max() > 128 and len(res.bow_words) > 20

            out.append(Case(f"assembly_{kind}_{n}", a, feats, (1,), aim))
    return out


# --------------------------------------------------------------------------
# 7. every scoring x weighting pair, on weights that tell sums apart
# --------------------------------------------------------------------------
def _flat_vocabulary(weights, L=1):
    """One level of len(weights) words, word j = Hadamard codeword j + 1."""
    b = Builder()
    for j, w in enumerate(weights):
        b.add(0, hadamard(1 + j), weight=w)
    return b


@functools.lru_cache(None)
def sum_order_inputs():
    """-> {"a": (arrays, feats), "b": ..., "c": ...} with scoring / weighting 0.
    (a) word 2 is hit by ten features of weight 0.1: ten additions give
        0.9999999999999999, 10 * 0.1 gives 1.0;
    (b) 16 words whose weights spread over twelve orders of magnitude: the
        L1 norm added in word order, last to first and pairwise differ;
    (c) weights whose squares need more than 53 bits, so that a fused
        multiply-add keeps what `x * x` rounds away before the add.
    The other weights are random; their seeds are the first for which the
    difference survives the normalisation under every scoring / weighting
    kind, which test_bow_ref asserts against each alternative sum."""
    wa = list(np.random.default_rng(700).uniform(0.2, 2.0, 4))
    wa[2] = 0.1
    ba = _flat_vocabulary(wa)
    hit = [2, 0, 2, 2, 1, 2, 2, 3, 2, 2, 2, 1, 2, 2]
    assert hit.count(2) == 10
    a = (ba.finish(4, 1), np.stack([ba.desc[1 + j] for j in hit]))
    bb = _flat_vocabulary(list(10.0 ** np.random.default_rng(700).uniform(-6, 6, 16)))
    order = (5, 0, 15, 3, 1, 2, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14)
    b = (bb.finish(16, 1), np.stack([bb.desc[1 + j] for j in order]))
    rng = np.random.default_rng(701)
    bc = _flat_vocabulary(list(rng.uniform(0.5, 2.0, 12)))
    c = (bc.finish(12, 1), np.stack([bc.desc[1 + j] for j in rng.permutation(12)]))
    return dict(a=a, b=b, c=c)


PAIRS = [(s, w) for s in range(6) for w in range(4)]


@functools.lru_cache(None)
def pair_cases():
    out = []
    for tag, (arrays, feats) in sum_order_inputs().items():
        for s, w in PAIRS:
            out.append(Case(f"pairs_{tag}_s{s}_w{w}", with_kind(arrays, s, w), feats, (0,), None))
    return out


# --------------------------------------------------------------------------
# 8. the empty vocabulary
# --------------------------------------------------------------------------
@functools.lru_cache(None)
def empty_cases():
    root = make_arrays([-1], [0], np.zeros((1, 32), np.uint8), [0.0], 10, 5)
    # nodes, but no leaf flag anywhere: no words, empty() as well
    b = Builder()
    for j in range(3):
        b.add(0, hadamard(1 + j), weight=1.0, leaf=0)
    wordless = b.finish(3, 1)
    feats = np.stack([hadamard(1 + j) for j in range(5)])

    def aim(res, levelsup):
        assert len(res.bow_words) == 0 and np.all(res.feat_node == -1)

    none = np.zeros((0, 32), np.uint8)
    return [Case("empty_root_only", root, feats, (0, 4), aim),
            Case("empty_root_only_no_features", root, none, (4,), aim),
            Case("empty_no_words", wordless, feats, (0, 1), aim)]


# --------------------------------------------------------------------------
# 9. the batch call
# --------------------------------------------------------------------------
@functools.lru_cache(None)
def batch_frames():
    """Frames of different length for one launch on the assembly vocabulary."""
    return [_assembly_feats("runs", 300, 901), np.zeros((0, 32), np.uint8),
            _assembly_feats("own_word", 37, 902), _assembly_feats("one_word", 511, 903),
            _assembly_feats("own_word", 1, 904), _assembly_feats("runs", 512, 905),
            np.zeros((0, 32), np.uint8)]


@functools.lru_cache(None)
def overflow_frame():
    """400 features for a call with max_n = 300 (cap 512): the last 100 must
    not be seen. They all belong to one live word the first 300 never hit."""
    a, leaves = assembly_vocabulary()
    live = leaves[a["weight"][leaves] > 0]
    f = _assembly_feats("own_word", 400, 906)
    f[300:] = a["desc"][live[-1]]
    assert not np.any(np.all(f[:300] == f[300], axis=1))
    return f


# --------------------------------------------------------------------------
# 10. limits
# --------------------------------------------------------------------------
def complete_tree_16_5():
    """parent / leaf of the complete k = 16, L = 5 tree in breadth-first
    order: 1,118,481 nodes, 2^20 leaves."""
    n = (16 ** 6 - 1) // 15
    parent = (np.arange(n, dtype=np.int64) - 1) // 16
    parent[0] = -1
    leaf = np.zeros(n, np.uint8)
    leaf[n - 16 ** 5:] = 1
    return parent.astype(np.int32), leaf


@functools.lru_cache(None)
def limit_case():
    """The largest vocabulary the library accepts: the complete k = 16, L = 5
    tree with its first leaf left without a flag, 2^20 - 1 words. Child j of
    every node holds Hadamard codeword j + 1, except on the path of last
    children, which holds D = all ones; the leaf before the last holds E.
    Feature 4095 = D walks to the last word, 2^20 - 2, whose sort key is the
    largest a frame can produce. The other features take a handful of
    descriptors: codewords (codeword 1 walks to the unflagged first leaf and
    folds into word 0), H, the descriptor of the second leaf, which is the
    flagged word 0, and G, between D and E, which walks to word 2^20 - 3."""
    parent, leaf = complete_tree_16_5()
    n = len(parent)
    first_leaf = n - 16 ** 5
    leaf[first_leaf] = 0
    codes = np.stack([hadamard(1 + j) for j in range(16)])
    desc = codes[(np.arange(n) - 1) % 16]
    desc[0] = 0
    D = np.full(32, 0xFF, np.uint8)
    last = [(16 ** (l + 1) - 1) // 15 - 1 for l in range(1, 6)]
    assert last[-1] == n - 1
    desc[last] = D
    E = with_bits(120, 0, D)
    desc[n - 2] = E
    G = with_bits(100, 0, D)
    H = with_bits(10, 0, codes[0])     # the second leaf: the flagged word 0
    desc[first_leaf + 1] = H
    rng = np.random.default_rng(1001)
    weight = np.zeros(n)
    weight[first_leaf:] = rng.uniform(0.1, 2.0, n - first_leaf)
    a = make_arrays(parent, leaf, desc, weight, 16, 5)
    pool = [codes[0], codes[3], G, codes[9], H]
    feats = np.stack([pool[i % len(pool)] for i in range(MAX_FEAT)])
    feats[MAX_FEAT - 1] = D

    def aim(res, levelsup):
        assert res.feat_word[MAX_FEAT - 1] == MAX_WORDS - 1 == (1 << 20) - 2
        assert res.paths[MAX_FEAT - 1] == last
        assert (res.feat_word == MAX_WORDS - 1).sum() == 1
        assert res.feat_word[2] == MAX_WORDS - 2 and res.paths[0][-1] == first_leaf
        assert res.bow_words.tolist()[-2:] == [MAX_WORDS - 2, MAX_WORDS - 1]
        assert res.bow_words[0] == 0 and len(res.bow_words) >= 4

    return Case("limit_max_words", a, feats, (4,), aim)


_TREES, _REFS = {}, {}


def tree_of(arrays):
    """One restatement tree per `arrays` object."""
    if id(arrays) not in _TREES:
        _TREES[id(arrays)] = (R.Tree(arrays), arrays)
    return _TREES[id(arrays)][0]


def reference(case, levelsup):
    """The restatement's result of a case, computed once per process."""
    key = (case.name, levelsup)
    if key not in _REFS:
        _REFS[key] = R.transform(case.arrays, case.feats, levelsup, tree=tree_of(case.arrays))
    return _REFS[key]


def first_divergence(arrays, path, node):
    """The first level at which the chain root -> `node` leaves `path`."""
    chain, parent = [], arrays["parent"]
    while node > 0:
        chain.append(int(node))
        node = int(parent[node])
    chain.reverse()
    for level, (a, b) in enumerate(zip(chain, path), 1):
        if a != b:
            return level
    return min(len(chain), len(path)) + 1


def mismatch(name, arrays, ref, words, vals, node, word=None, weight=None):
    """None if (words, vals, node[, word, weight]) equal the restatement's
    result bit for bit, else a message that names the case, the first
    differing feature and the level at which its walk left the
    restatement's path."""
    node = np.asarray(node)
    if len(node) != len(ref.feat_node):
        return f"{name}: {len(node)} feature nodes, expected {len(ref.feat_node)}"
    bad = np.nonzero(node != ref.feat_node)[0]
    if word is not None and any(len(p) for p in ref.paths):
        bad = np.union1d(bad, np.nonzero((np.asarray(word) != ref.feat_word) |
                                         (np.asarray(weight).view(np.uint64) !=
                                          ref.feat_weight.view(np.uint64)))[0])
    if len(bad):
        i = int(bad[0])
        path = ref.paths[i]
        level = (first_divergence(arrays, path, int(node[i]))
                 if 0 <= node[i] < len(arrays["parent"]) else "none (no node of the tree)")
        return (f"{name}: feature {i}: node {int(node[i])}, expected {int(ref.feat_node[i])}; "
                f"restatement path {path} (word {int(ref.feat_word[i])}, weight "
                f"{float(ref.feat_weight[i])!r}); first differing level {level}"
                + ("" if word is None else f"; word {int(word[i])}, weight {float(weight[i])!r}"))
    words, vals = np.asarray(words), np.asarray(vals, np.float64)
    if not np.array_equal(words, ref.bow_words):
        extra = sorted(set(words.tolist()) ^ set(ref.bow_words.tolist()))[:5]
        feat = [int(np.nonzero(ref.feat_word == w)[0][0]) for w in extra if np.any(ref.feat_word == w)]
        return (f"{name}: BowVector words differ ({len(words)} against {len(ref.bow_words)}), "
                f"first {extra}, features {feat}")
    diff = np.nonzero(vals.view(np.uint64) != ref.bow_vals.view(np.uint64))[0]
    if len(diff):
        q = int(diff[0])
        return (f"{name}: BowVector value of word {int(words[q])} is {float(vals[q])!r}, expected "
                f"{float(ref.bow_vals[q])!r} ({len(diff)} of {len(vals)} values differ)")
    return None


def small_cases():
    """Every case but the limit case."""
    out = [c for c, _ in sibling_order_cases()]
    out += fanout_cases() + tie_cases() + [one_bit_case()]
    out += [unbalanced_case(3), unbalanced_case(10)]
    out += flag_cases() + assembly_cases() + pair_cases() + empty_cases()
    return out


def case_runs(cases):
    """(case, levelsup) pairs with readable ids."""
    runs = [(c, ls) for c in cases for ls in c.levelsups]
    return runs, [f"{c.name}-up{ls}" for c, ls in runs]
