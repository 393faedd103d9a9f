"""Sequential restatement of DBoW2's ORB vocabulary transform in plain
Python / numpy, independent of oracle/ and of the package:

  TemplatedVocabulary::transform(features, BowVector, FeatureVector, levelsup)
      Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1194
  TemplatedVocabulary::transform(feature, word_id, weight, nid, levelsup)
      TemplatedVocabulary.h:1217-1259
  TemplatedVocabulary::empty()  (m_words.empty())       TemplatedVocabulary.h:1009
  FORB::distance                                         FORB.cpp:81-101
  BowVector::addWeight / addIfNotExist / normalize       BowVector.cpp:34-84

The tree is given as the flat node arrays of ORBVocabulary.to_arrays() (node 0
= root, parent[i] < i, word ids follow the leaf flags in node order, a node
without the flag keeps Node()'s word id 0). Children are visited in id order
with a strict `<`, so the first child of minimal distance wins. Every sum is
taken with Python floats, one `+=` at a time, in the reference's order: a
word's weights in feature order, the norm in word order, `x * x` rounded
before it is added.

Pinned where the reference leaves a value indeterminate: a
walk that ends in a leaf above level L - levelsup reports that leaf as the
feature's node.

`transform` also returns, per feature, the node visited at every level, so a
failing comparison can name the level at which a walk diverged."""
import math
from collections import namedtuple

import numpy as np

Result = namedtuple("Result", "bow_words bow_vals feat_node feat_word feat_weight paths")

NORM_NONE, NORM_L1, NORM_L2 = 0, 1, 2
TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3


def must_normalize(scoring):
    """ScoringObject.h: L1_NORM, CHI_SQUARE, KL, BHATTACHARYYA normalise with
    L1, L2_NORM with L2, DOT_PRODUCT does not."""
    return {0: NORM_L1, 1: NORM_L2, 2: NORM_L1, 3: NORM_L1, 4: NORM_L1, 5: NORM_NONE}[int(scoring)]


def distance(a, b):
    """FORB::distance of two 32-byte descriptors: eight 32-bit words, each
    counted with the reference's parallel bit count."""
    pa = np.frombuffer(bytes(bytearray(a)), "<u4")
    pb = np.frombuffer(bytes(bytearray(b)), "<u4")
    dist = 0
    for i in range(8):
        v = int(pa[i]) ^ int(pb[i])
        v = v - ((v >> 1) & 0x55555555)
        v = (v & 0x33333333) + ((v >> 2) & 0x33333333)
        dist += ((((v + (v >> 4)) & 0xF0F0F0F) * 0x1010101) & 0xFFFFFFFF) >> 24
    return dist


def distances(f8, rows8):
    """`distance` of one descriptor (8 u32) to several (m x 8 u32) at once:
    the same bit count on numpy words; test_bow_ref holds it to `distance`."""
    v = rows8 ^ f8
    v = v - ((v >> np.uint32(1)) & np.uint32(0x55555555))
    v = (v & np.uint32(0x33333333)) + ((v >> np.uint32(2)) & np.uint32(0x33333333))
    v = (((v + (v >> np.uint32(4))) & np.uint32(0xF0F0F0F)) * np.uint32(0x1010101)) >> np.uint32(24)
    return v.sum(axis=1, dtype=np.int64).tolist()


class Tree:
    """The node arrays as the reference holds them: children per node in id
    order, the word id of every node, the number of words."""

    def __init__(self, arrays):
        parent = np.asarray(arrays["parent"], np.int64)
        n = len(parent)
        assert n >= 1
        ids = np.arange(1, n)
        assert np.all((parent[1:] >= 0) & (parent[1:] < ids)), "a node's parent must precede it"
        self.child = (np.argsort(parent[1:], kind="stable") + 1).astype(np.int64)
        counts = np.bincount(parent[1:], minlength=n) if n > 1 else np.zeros(1, np.int64)
        self.child_start = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        leaf = np.asarray(arrays["leaf"]).astype(bool).copy()
        leaf[0] = False                       # the root is no line of the file
        self.word = np.where(leaf, np.cumsum(leaf) - 1, 0).astype(np.int64)
        self.n_words = int(leaf.sum())
        self.weight = np.asarray(arrays["weight"], np.float64)
        self.desc8 = np.ascontiguousarray(arrays["desc"], np.uint8).reshape(n, 32).view("<u4")
        self.L = int(arrays["L"])
        self.scoring, self.weighting = int(arrays["scoring"]), int(arrays["weighting"])
        self.n_nodes = n

    def children(self, node):
        return self.child[self.child_start[node]:self.child_start[node + 1]]

    def walk(self, f8):
        """The node chosen at level 1, 2, ... down to a node without children."""
        path, node = [], 0
        while True:
            ch = self.children(node)
            d = distances(f8, self.desc8[ch])
            best, best_d = int(ch[0]), d[0]
            for q in range(1, len(ch)):
                if d[q] < best_d:
                    best_d = d[q]
                    best = int(ch[q])
            node = best
            path.append(node)
            if self.child_start[node] == self.child_start[node + 1]:   # isLeaf()
                return path


def seq_sum(values):
    s = 0.0
    for x in values:
        s += x
    return s


def seq_sum_squares(values):
    s = 0.0
    for x in values:
        sq = x * x          # rounded on its own (no fused multiply-add)
        s += sq
    return s


def assemble(feat_word, feat_weight, scoring, weighting, run_sum=seq_sum, l1_sum=seq_sum,
             l2_sum=seq_sum_squares):
    """The BowVector of per-feature (word, weight): addWeight / addIfNotExist
    of every feature that is not stopped, the TF division, normalize. The three
    sums can be replaced to show that a case tells summation orders apart."""
    tf = weighting in (TF_IDF, TF)
    order, runs = [], {}
    for wid, w in zip(feat_word, feat_weight):
        w = float(w)
        if not w > 0:
            continue
        wid = int(wid)
        if wid not in runs:
            runs[wid] = [w]
            order.append(wid)
        elif tf:
            runs[wid].append(w)          # addWeight; addIfNotExist keeps the first
    words = sorted(order)
    vals = [run_sum(runs[wid]) if len(runs[wid]) > 1 else runs[wid][0] for wid in words]
    norm_kind = must_normalize(scoring)
    if tf and vals and norm_kind == NORM_NONE:
        nd = float(len(vals))
        vals = [x / nd for x in vals]
    if norm_kind != NORM_NONE:
        if norm_kind == NORM_L1:
            norm = l1_sum([abs(x) for x in vals])
        else:
            norm = math.sqrt(l2_sum(vals))
        if norm > 0.0:
            vals = [x / norm for x in vals]
    return np.array(words, np.uint32), np.array(vals, np.float64)


def transform(arrays, features, levelsup, tree=None):
    t = tree if tree is not None else Tree(arrays)
    feats = np.ascontiguousarray(features, np.uint8).reshape(-1, 32)
    n = len(feats)
    feat_node = np.full(n, -1, np.int32)
    feat_word = np.zeros(n, np.int32)
    feat_weight = np.zeros(n, np.float64)
    if t.n_words == 0:                        # empty(): nothing is added
        return Result(np.zeros(0, np.uint32), np.zeros(0, np.float64), feat_node, feat_word,
                      feat_weight, [[] for _ in range(n)])
    nid_level = t.L - levelsup
    f8 = feats.view("<u4")
    cache, paths = {}, []
    for i in range(n):
        key = feats[i].tobytes()
        path = cache.get(key)
        if path is None:
            path = cache[key] = t.walk(f8[i])
        paths.append(path)
        final = path[-1]
        if nid_level <= 0:
            nid = 0
        elif nid_level <= len(path):
            nid = path[nid_level - 1]
        else:
            nid = final                       # P20
        feat_word[i] = t.word[final]
        feat_weight[i] = t.weight[final]
        if feat_weight[i] > 0:
            feat_node[i] = nid
    words, vals = assemble(feat_word, feat_weight, t.scoring, t.weighting)
    return Result(words, vals, feat_node, feat_word, feat_weight, paths)
