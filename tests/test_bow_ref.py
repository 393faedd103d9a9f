"""CPU tests of the DBoW2 transform branch by branch: the oracle's
TemplatedVocabulary::transform against the sequential restatement
tests/_bow_ref.py, bit for bit, on the hand-built vocabularies of
tests/_bow_cases.py; every case checked to reach the branch it was built for;
the summation-order cases shown to tell the orders apart; the vocabularies
the library refuses; and the text loader against the oracle's on rewritten
files."""
from fractions import Fraction

import numpy as np
import pytest

import _bow_cases as BC
import _bow_ref as R

RUNS, RUN_IDS = BC.case_runs(BC.small_cases())
_ORACLES = {}


def _oracle_voc(oracle, arrays):
    if id(arrays) not in _ORACLES:
        _ORACLES[id(arrays)] = (oracle.Vocabulary(arrays=arrays), arrays)
    return _ORACLES[id(arrays)][0]


def _check(oracle, case, levelsup):
    ref = BC.reference(case, levelsup)
    if case.aim:
        case.aim(ref, levelsup)
    ow, ov, on, owd, owt = _oracle_voc(oracle, case.arrays).transform(case.feats, levelsup=levelsup)
    msg = BC.mismatch(f"{case.name} levelsup {levelsup}", case.arrays, ref, ow, ov, on, owd, owt)
    assert msg is None, msg


@pytest.mark.parametrize("case,levelsup", RUNS, ids=RUN_IDS)
def test_oracle_equals_restatement(oracle, case, levelsup):
    _check(oracle, case, levelsup)


def test_oracle_equals_restatement_at_the_word_limit(orbpl, oracle):
    """2^20 - 1 words: accepted by the library (host only), and the oracle
    walks feature 4095 to the last word as the restatement does."""
    case = BC.limit_case()
    v = orbpl.ORBVocabulary(arrays=case.arrays)
    assert v.n_words == BC.MAX_WORDS and v.n_nodes == (16 ** 6 - 1) // 15
    _check(oracle, case, case.levelsups[0])


def test_vector_distance_is_the_scalar_distance():
    rng = np.random.default_rng(5)
    rows = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    rows[0] = 0
    rows[1] = 0xFF
    rows[2] = rows[3]
    for f in (rows[0], rows[1], rows[3], rows[7]):
        want = [R.distance(f, r) for r in rows]
        assert R.distances(f.view("<u4"), rows.view("<u4")) == want
        assert want == [int(np.unpackbits(f ^ r).sum()) for r in rows]
    assert R.distance(rows[0], rows[1]) == 256 and R.distance(rows[2], rows[3]) == 0


def test_numberings_agree_after_mapping_back():
    """Breadth-first, depth-first and interleaved numberings of one tree give
    the same FeatureVector nodes and the same BowVector once node and word ids
    are mapped back to the canonical tree."""
    results = []
    for case, order in BC.sibling_order_cases():
        order = np.asarray(order)
        leaf_nodes = np.nonzero(case.arrays["leaf"])[0]          # word id -> node id
        for ls in case.levelsups:
            ref = BC.reference(case, ls)
            node = np.where(ref.feat_node >= 0, order[np.maximum(ref.feat_node, 0)], -1)
            bow = {int(order[leaf_nodes[w]]): float(v).hex()
                   for w, v in zip(ref.bow_words, ref.bow_vals)}
            final = [int(order[p[-1]]) for p in ref.paths]
            results.append((case.name, ls, node.tolist(), bow, final))
    per_ls = len(results) // 3
    for q in range(per_ls):
        a, b, c = results[q], results[per_ls + q], results[2 * per_ls + q]
        assert a[1] == b[1] == c[1]
        assert a[2:] == b[2:], (a[0], b[0], a[1])
        assert a[2:] == c[2:], (a[0], c[0], a[1])
        assert len(a[3]) > 30 and len(set(a[4])) > 50


def _bits(vals):
    return np.asarray(vals, np.float64).view(np.uint64)


def _ref_parts(tag, scoring, weighting):
    arrays, feats = BC.sum_order_inputs()[tag]
    ref = R.transform(BC.with_kind(arrays, scoring, weighting), feats, 0)
    return ref


def test_repeated_weight_is_not_count_times_weight():
    """(a): ten additions of 0.1 are not 10 * 0.1, and the BowVector shows it
    under every scoring with TF-IDF and TF."""
    assert R.seq_sum([0.1] * 10) != 10 * 0.1
    for scoring in range(6):
        for weighting in (R.TF_IDF, R.TF):
            ref = _ref_parts("a", scoring, weighting)
            assert (ref.feat_word == 2).sum() == 10
            _, alt = R.assemble(ref.feat_word, ref.feat_weight, scoring, weighting,
                                run_sum=lambda ws: len(ws) * ws[0])
            assert np.any(_bits(alt) != _bits(ref.bow_vals)), (scoring, weighting)


def _pairwise(v):
    return v[0] if len(v) == 1 else _pairwise(v[:len(v) // 2]) + _pairwise(v[len(v) // 2:])


def test_l1_norm_order_is_visible():
    """(b): the L1 norm summed in word order differs from the same sum taken
    from the last word to the first and from a pairwise sum, and so do the
    normalised values."""
    for scoring in (0, 2, 3, 4):
        for weighting in range(4):
            ref = _ref_parts("b", scoring, weighting)
            assert len(ref.bow_words) == 16
            for other in (lambda v: R.seq_sum(v[::-1]), _pairwise):
                _, alt = R.assemble(ref.feat_word, ref.feat_weight, scoring, weighting, l1_sum=other)
                assert np.any(_bits(alt) != _bits(ref.bow_vals)), (scoring, weighting)


def _fma_sum_squares(values):
    """acc = fma(x, x, acc): the exact x * x + acc rounded once."""
    acc = 0.0
    for x in values:
        acc = float(Fraction(x) * Fraction(x) + Fraction(acc))
    return acc


def test_l2_norm_tells_fused_from_unfused():
    """(c): x * x rounded and then added differs from a fused multiply-add,
    in the norm and in the normalised values."""
    for weighting in range(4):
        ref = _ref_parts("c", 1, weighting)
        vals = [float(x) for x in R.assemble(ref.feat_word, ref.feat_weight, 5, 2)[1]]
        assert len(vals) == 12
        assert R.seq_sum_squares(vals) != _fma_sum_squares(vals)
        _, alt = R.assemble(ref.feat_word, ref.feat_weight, 1, weighting, l2_sum=_fma_sum_squares)
        assert np.any(_bits(alt) != _bits(ref.bow_vals)), weighting
        _, rev = R.assemble(ref.feat_word, ref.feat_weight, 1, weighting,
                            l2_sum=lambda v: R.seq_sum_squares(v[::-1]))
        assert np.any(_bits(rev) != _bits(ref.bow_vals)), weighting


def test_refused_vocabularies(orbpl):
    """Host only: 2^20 words (one more than accepted), 2^21 - 1 nodes, a
    parent at or after its child."""
    parent, leaf = BC.complete_tree_16_5()
    n = len(parent)
    assert int(leaf.sum()) == BC.MAX_WORDS + 1 == 1 << 20

    def build(parent, leaf):
        m = len(parent)
        return orbpl.ORBVocabulary(arrays=BC.make_arrays(parent, leaf, np.zeros((m, 32), np.uint8),
                                                         np.ones(m), 16, 5))
    with pytest.raises(orbpl.OrbplError, match="words"):
        build(parent, leaf)
    leaf[n - 1] = 0
    assert build(parent, leaf).n_words == BC.MAX_WORDS
    m = (1 << 21) - 1
    star = np.zeros(m, np.int32)
    star[0] = -1
    with pytest.raises(orbpl.OrbplError, match="nodes"):
        build(star, np.zeros(m, np.uint8))
    assert build(star[:m - 1], np.zeros(m - 1, np.uint8)).n_nodes == m - 1
    for bad in ([-1, 0, 2, 1], [-1, 0, 3, 1], [-1, 1], [-1, -1]):
        with pytest.raises(orbpl.OrbplError, match="parent"):
            build(np.array(bad, np.int32), np.ones(len(bad), np.uint8))


def _rewrites():
    from _vocab import tiny_vocabulary_text
    txt = tiny_vocabulary_text()
    lines = txt.split("\n")

    def cut(line, ntok):
        return " ".join(line.split()[:ntok])
    short_desc = list(lines)
    short_desc[4] = cut(lines[4], 2 + 10)          # parent, flag, 10 of 32 descriptor tokens
    no_weight = list(lines)
    no_weight[6] = cut(lines[6], 2 + 32)           # everything but the weight
    blank = lines[:3] + [""] + lines[3:5] + ["  \t "] + lines[5:]
    return {"crlf": txt.replace("\n", "\r\n"), "tabs": txt.replace(" ", "\t"),
            "space_runs": txt.replace(" ", "    "), "blank_line": "\n".join(blank),
            "short_descriptor": "\n".join(short_desc), "no_weight": "\n".join(no_weight)}


@pytest.mark.parametrize("how", ["crlf", "tabs", "space_runs", "blank_line", "short_descriptor",
                                 "no_weight"])
def test_loader_equals_oracle_on_rewritten_file(orbpl, oracle, tmp_path, how):
    from _vocab import tiny_features
    p = tmp_path / f"{how}.txt"
    p.write_bytes(_rewrites()[how].encode())
    g = orbpl.ORBVocabulary(p)
    o = oracle.Vocabulary(p)
    ga, on = g.to_arrays(), o.nodes()
    assert (g.k, g.L, g.scoring, g.weighting) == (o.k, o.L, o.scoring, o.weighting) == (2, 2, 0, 0)
    assert (g.n_nodes, g.n_words) == (o.n_nodes, o.n_words) == (7, 4)
    for k in ("parent", "leaf", "desc", "weight"):
        assert np.array_equal(ga[k], on[k]), k
    if how == "short_descriptor":
        assert ga["desc"][4, :10].tolist() == [240] + [0] * 9 and ga["weight"][4] == 0
    if how == "no_weight":
        assert ga["weight"][6] == 0 and ga["desc"][6, 31] == 255
    # the restatement on the loaded arrays equals the oracle on the loaded file
    ref = R.transform(ga, tiny_features(), 1)
    ow, ov, onode, _, _ = o.transform(tiny_features(), levelsup=1)
    assert BC.mismatch(how, ga, ref, ow, ov, onode) is None
