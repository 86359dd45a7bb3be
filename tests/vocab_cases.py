"""Directed vocabulary cases (numpy only): hand-written DBoW2 text vocabularies and descriptor
sets that hit the decisions of k_transform (csrc/orbx_vocab.hip) and of the host assembly of
the BowVector / FeatureVector on purpose, and BowVector sets for k_bow_score.

A vocabulary case: name, constructs, text (the file's contents, with its own line ends), desc
(n x 32 uint8), levelsups.  Node ids are line numbers (the root is 0); word ids count the
lines with isLeaf > 0 in file order.  A descriptor is given as the set of its 1-bits, so every
Hamming distance in a case can be read off."""
import numpy as np

ZERO = frozenset()
ALL = frozenset(range(256))


def desc(bits):
    d = np.zeros(256, np.uint8)
    d[list(bits)] = 1
    return np.packbits(d)   # bit 0 is the top bit of byte 0: only distances matter


def rand_desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def line(parent, leaf, d, weight):
    return f"{parent} {leaf} " + " ".join(str(int(x)) for x in d) + f" {weight!r}"


def text(k, L, scoring, weighting, nodes, eol="\n", blanks=()):
    """nodes: (parent, isLeaf, descriptor bytes, weight) in file order; `blanks`: node indices
    (1-based ids) after which a blank line follows."""
    out = [f"{k} {L} {scoring} {weighting}"]
    for i, nd in enumerate(nodes, 1):
        out.append(line(*nd))
        if i in blanks:
            out.append("   " if i % 2 else "")
    return eol.join(out) + eol


def case(name, constructs, txt, descs, levelsups=(0,)):
    d = np.ascontiguousarray(np.asarray(descs, np.uint8).reshape(-1, 32))
    return dict(name=name, constructs=tuple(constructs), text=txt, desc=d,
                levelsups=tuple(levelsups))


CONSTRUCTS = (
    "tie_children_0_1", "tie_children_0_last", "tie_children_last_two", "tie_all_children",
    "tie_different_bits", "distance_0_and_256", "byte_sensitivity",
    "leaf_depths_1_2_L", "childless_nonleaf", "one_child", "k1", "k20", "children_not_contiguous",
    "blank_lines_crlf", "levelsup_sweep",
    "stop_word_third", "all_stop_words", "scoring_weighting_pairs",
    "sizes_0_1_255_256_257",
)


def _tie_cases():
    out = []
    rng = np.random.default_rng(11)
    a = rand_desc(rng, 1)[0]
    others = rand_desc(rng, 4)
    k = 4
    for name, same in (("tie_children_0_1", (0, 1)), ("tie_children_0_last", (0, k - 1)),
                       ("tie_children_last_two", (k - 2, k - 1)),
                       ("tie_all_children", tuple(range(k)))):
        nodes = [(0, 1, a if c in same else others[c], 1.0 + c) for c in range(k)]
        # the tied descriptor itself, one bit off it, and the other children's descriptors
        near = a.copy()
        near[17] ^= 0x10
        out.append(case(name, [name], text(k, 1, 0, 0, nodes), [a, near] + list(others)))
    # distance 1 through bit 0 and through bit 200, 2 through {0, 200} against {5, 77}
    nodes = [(0, 1, desc({0}), 1.0), (0, 1, desc({200}), 2.0), (0, 1, desc({5, 77}), 3.0)]
    qs = [desc(ZERO), desc({0, 200}), desc({5}), desc({200, 77})]
    out.append(case("tie_different_bits", ["tie_different_bits"], text(3, 1, 0, 0, nodes), qs))
    # the complement first: 256 against 0, then 256 alone (k = 1)
    f = rand_desc(rng, 1)[0]
    nodes = [(0, 1, ~f, 1.0), (0, 1, f, 2.0)]
    out.append(case("distance_0_and_256", ["distance_0_and_256"], text(2, 1, 0, 0, nodes),
                    [f, ~f, desc(ZERO), desc(ALL)]))
    # per byte b: child 2b' has 0x0F there, child 2b'+1 has 0xF0; the descriptor with 0xF0 in
    # byte b is at distance 0 from the odd child and 8 from every other one.  With byte b (or
    # its dword) dropped from the distance the even child ties at 0 and wins.
    for g in range(4):
        nodes, qs = [], []
        for b in range(8 * g, 8 * g + 8):
            lo, hi = np.zeros(32, np.uint8), np.zeros(32, np.uint8)
            lo[b], hi[b] = 0x0F, 0xF0
            nodes += [(0, 1, lo, 1.0), (0, 1, hi, 1.0)]
            qs.append(hi)
        out.append(case(f"bytes_{8 * g}_{8 * g + 7}", ["byte_sensitivity"],
                        text(16, 1, 0, 0, nodes), qs))
    return out


def ragged_nodes():
    """L = 3.  Root children in file order: 1 (leaf, depth 1), 2, 3.
        2: children 4 (leaf, depth 2), 6 (inner), 8 (childless, isLeaf 0); 3: one child 5.
        6: children 7, 9 (leaves, depth 3).  Children of 2 and of 6 are not contiguous."""
    B = lambda *b: desc(set(b))
    up, mid, down = set(range(0, 64)), set(range(64, 128)), set(range(128, 192))
    return [
        (0, 1, desc(up), 1.5),                    # 1: word 0, leaf at depth 1
        (0, 0, desc(mid), 0.0),                   # 2
        (0, 0, desc(down), 0.0),                  # 3: one child
        (2, 1, desc(mid | {200}), 2.5),           # 4: word 1, leaf at depth 2
        (3, 1, B(7), 0.75),                       # 5: word 2, the only child of 3
        (2, 0, desc(mid | {201}), 0.0),           # 6
        (6, 1, desc(mid | {201, 210}), 3.5),      # 7: word 3, depth 3
        (2, 0, desc(mid | {202}), 4.5),           # 8: childless with isLeaf 0 (word_id 0)
        (6, 1, desc(mid | {201, 211}), 0.5),      # 9: word 4, depth 3
    ]


def ragged_descs():
    up, mid, down = set(range(0, 64)), set(range(64, 128)), set(range(128, 192))
    return [desc(up), desc(up | {3}), desc(mid | {200}), desc(mid | {201, 210}),
            desc(mid | {201, 211}), desc(mid | {201}), desc(mid | {202}), desc(down),
            desc(ALL), desc(ZERO), desc(mid), desc(mid | {201, 210, 211})]


def _ragged_cases():
    L = 3
    sweep = (-1, 0, 1, L - 1, L, L + 3)
    nodes = ragged_nodes()
    out = [case("ragged", ["leaf_depths_1_2_L", "childless_nonleaf", "one_child",
                           "children_not_contiguous", "levelsup_sweep"],
                text(3, L, 0, 0, nodes), ragged_descs(), sweep),
           case("ragged_crlf_blank", ["blank_lines_crlf"],
                text(3, L, 0, 0, nodes, eol="\r\n", blanks=(2, 5, 9)), ragged_descs(), sweep)]
    rng = np.random.default_rng(12)
    d = rand_desc(rng, 3)
    chain = [(0, 0, d[0], 0.0), (1, 0, d[1], 0.0), (2, 1, d[2], 2.0)]
    out.append(case("k1_chain", ["k1"], text(1, 3, 0, 0, chain), rand_desc(rng, 5), sweep))
    leaves = rand_desc(rng, 20)
    nodes = [(0, 1, leaves[c], 1.0 + c / 4.0) for c in range(20)]
    qs = np.concatenate([leaves[::3], rand_desc(rng, 40)])
    out.append(case("k20", ["k20"], text(20, 1, 0, 0, nodes), qs, (0, 1)))
    return out


def _weight_cases():
    out = []
    rng = np.random.default_rng(13)
    leaves = rand_desc(rng, 3)
    near = lambda c, n: np.array([leaves[c] ^ np.eye(32, dtype=np.uint8)[i % 32] for i in range(n)])
    # 30 descriptors, 10 of them reach the stop word (weight 0) of leaf 1
    d = np.concatenate([near(0, 12), near(1, 10), near(2, 8)])
    nodes = [(0, 1, leaves[0], 1.25), (0, 1, leaves[1], 0.0), (0, 1, leaves[2], 0.5)]
    out.append(case("stop_word_third", ["stop_word_third"], text(3, 1, 0, 0, nodes), d))
    nodes = [(0, 1, leaves[0], 0.0), (0, 1, leaves[1], -1.0), (0, 1, leaves[2], 0.0)]
    for sc in (0, 1, 5):
        out.append(case(f"all_stop_words_sc{sc}", ["all_stop_words"],
                        text(3, 1, sc, 0, nodes), d))
    # every (scoring, weighting) pair on a two-level tree with repeated words
    inner = rand_desc(rng, 2)
    lv = rand_desc(rng, 4)
    nodes = [(0, 0, inner[0], 0.0), (0, 0, inner[1], 0.0), (1, 1, lv[0], 0.3), (1, 1, lv[1], 1.7),
             (2, 1, lv[2], 0.0), (2, 1, lv[3], 2.9)]
    d = np.concatenate([rand_desc(rng, 24), lv, lv[:2]])
    for sc in range(6):
        for wt in range(4):
            out.append(case(f"pair_sc{sc}_wt{wt}", ["scoring_weighting_pairs"],
                            text(2, 2, sc, wt, nodes), d, (0, 1)))
    return out


def _size_cases():
    rng = np.random.default_rng(14)
    nodes = [(0, 0, x, 0.0) for x in rand_desc(rng, 4)]
    nodes += [(1 + p, 1, x, 0.5 + i / 8.0) for p in range(4)
              for i, x in enumerate(rand_desc(rng, 4))]
    txt = text(4, 2, 0, 0, nodes)
    return [case(f"size_{n}", ["sizes_0_1_255_256_257"], txt, rand_desc(rng, n), (1,))
            for n in (0, 1, 255, 256, 257)]


def all_cases():
    cases = _tie_cases() + _ragged_cases() + _weight_cases() + _size_cases()
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return cases


CASES = all_cases()

HEADER_ONLY = "10 6 0 0\n"
# node 2 names itself as parent; node 2 names a later node
BAD_PARENT = [text(2, 2, 0, 0, [(0, 0, desc(ZERO), 0.0), (2, 1, desc(ALL), 1.0)]),
              text(2, 2, 0, 0, [(0, 0, desc(ZERO), 0.0), (3, 1, desc(ALL), 1.0),
                                (1, 1, desc({1}), 1.0)])]


# ---- k_bow_score ------------------------------------------------------------------------------
def bow_score_sets():
    """(name, query BowVector, keyframe BowVectors): nq = 0, 1 / 3 / 4 / 5 keyframes (the
    4-keyframes-per-workgroup tail), keyframes of 0, 64 and 65 words, the order-dependent sum
    (one term of -(2^53 + 2^29), then 70 of -1: the score is a float32 tie only in ascending
    order)."""
    rng = np.random.default_rng(15)

    def rb(n, lo=0, hi=400):
        w = np.sort(rng.choice(np.arange(lo, hi), n, replace=False)).astype(np.uint32)
        return w, rng.random(n) / max(n, 1)

    q = rb(120)
    sets = [("nq0", (np.zeros(0, np.uint32), np.zeros(0)), [rb(10), rb(0), rb(70)])]
    for nkf in (1, 3, 4, 5):
        sets.append((f"nkf{nkf}", q, [rb(int(n)) for n in rng.integers(1, 150, nkf)]))
    sets.append(("words_0_64_65", q, [rb(0), rb(64), rb(65), (q[0][:64].copy(), q[1][:64] * 0.5),
                                      (q[0][:65].copy(), q[1][:65] * 2.0)]))
    big = 2.0**52 + 2.0**28
    w = np.arange(5000, 5071, dtype=np.uint32)
    v = np.array([big] + [0.5] * 70)
    sets.append(("order_dependent_sum", (w, v), [(w, v), (w[::-1][::-1][1:], v[1:]), (w[:1], v[:1])]))
    return sets
