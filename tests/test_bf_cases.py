"""CPU: the directed brute-force top-2 cases (tests/bf_cases.py) before any kernel sees them.

For every case: the plain reference gives exactly the outcome the case states (so a noise row
that undercut a planted distance fails here), the oracle (oracle_bf_top2, the best / second
loop of src/ORBmatcher.cc:232-256) equals the reference, whole and on shard_range shards folded
by distributed.merge_top2, and the structural model of the kernels equals the reference.  The
census then shows that the table is neither thin nor padded: every model variant (one flipped
decision of the kernels) changes some case's outcome, every construct a case claims occurs in
it, and every case is the only holder of some construct.
"""
import numpy as np
import pytest

import bf_cases as bc
from bf_cases import MFMA, VALU, where
from my_orb_slam2_amd.distributed import merge_top2, shard_range

CASES = {c.name: c for c in bc.cases()}
NAMES = list(CASES)
_REF = {}


def ref_of(name):
    """The reference's result per case, computed once and never modified."""
    if name not in _REF:
        c = CASES[name]
        r = bc.reference_top2(c.q, c.db)
        for a in r:
            a.setflags(write=False)
        _REF[name] = r
    return _REF[name]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- every case ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_reference_gives_the_stated_outcome(name):
    c, r = CASES[name], ref_of(name)
    assert c.expect, "a case states at least one query's outcome"
    for i, want in c.expect.items():
        got = (int(r[0][i]), int(r[1][i]), int(r[2][i]))
        assert got == want, f"{name}: query {i}: reference {got}, the case states {want}"


def test_reference_slabs_agree():
    """The slab join of the reference itself: one row per slab and 7 rows per slab against a
    single slab, on the case with the most ties."""
    c = CASES["ties_c256"]
    whole = bc.top2_of_distances(c.dist())
    for rows in (1, 7, 255):
        assert same(bc.reference_top2(c.q, c.db, slab_rows=rows), whole)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_reference(oracle_mod, name):
    import oracle.matcher as om
    c, r = CASES[name], ref_of(name)
    got = om.bf_top2(c.q, c.db)
    for g, w, what in zip(got, r, ("best_idx", "best_dist", "second_dist")):
        np.testing.assert_array_equal(g, w, err_msg=f"{name}: {what}")
    for world in (3, 8):
        parts = [om.bf_top2(c.q, c.db, *shard_range(c.ndb, k, world)) for k in range(world)]
        merged = merge_top2(parts)
        for g, w, what in zip(merged, r, ("best_idx", "best_dist", "second_dist")):
            np.testing.assert_array_equal(np.asarray(g), w, err_msg=f"{name}: world {world} {what}")


@pytest.mark.parametrize("name", NAMES)
def test_model_equals_reference(name):
    c = CASES[name]
    want = c.with_base(ref_of(name))
    for k in c.kernels:
        got = bc.model_top2(c.q, c.db, c.chunk_rows(), k, idx_base=c.idx_base, d=c.dist())
        for g, w, what in zip(got, want, ("best_idx", "best_dist", "second_dist")):
            np.testing.assert_array_equal(g, w, err_msg=f"{name}: {bc.KERNEL_NAMES[k]} {what}")


def test_regimes_cover_both_grid_forms():
    """xcd_block remaps a grid only when its workgroup count is a multiple of 8: the merge
    family runs both forms with either kernel."""
    for k in (MFMA, VALU):
        counts = {n: CASES[f"merge_{n}"].regime(k) for n in bc.MERGE_NCHUNKS}
        mult = {n for n, r in counts.items() if (r["query_blocks"] * r["nchunks"]) % 8 == 0}
        # k_bf_top2's grid x is nqpad / 256 = 4 here: every even chunk count is remapped
        assert mult == ({8, 16, 64, 72} if k == MFMA else {2, 8, 16, 64, 72})
    assert [CASES[f"merge_{n}"].regime(MFMA)["merge_slice"] for n in bc.MERGE_NCHUNKS] == \
        [1, 1, 1, 1, 2, 2, 3, 8, 8, 9, 9, 10]
    big = CASES["nq_2049"]
    assert big.regime(MFMA)["query_blocks"] == 3 and big.regime(VALU)["query_blocks"] == 12
    assert big.regime(MFMA)["nqpad"] == 3072


# ---- merge_top2, directed ----------------------------------------------------------------------

def _part(*rows):
    a = np.array(rows, np.int32)
    return a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy()


def test_merge_top2_directed():
    none = (-1, 256, 256)
    # query 0: a tie across shards, the earlier shard wins and the second equals the best
    # query 1: the first shard has nothing below 256
    # query 2: best from the later shard, second from the earlier
    # query 3: best and second both from the later shard
    # query 4: nothing anywhere
    a = _part((5, 10, 40), none, (7, 30, 31), (3, 50, 60), none)
    b = _part((105, 10, 12), (140, 20, 256), (150, 9, 90), (160, 7, 8), none)
    got = merge_top2([a, b])
    want = _part((5, 10, 10), (140, 20, 256), (150, 9, 30), (160, 7, 8), none)
    assert same([np.asarray(g) for g in got], want)
    # an empty shard (what a rank without rows reports) changes nothing, wherever it stands
    empty = _part(*[none] * 5)
    for parts in ([empty, a, b], [a, empty, b], [a, b, empty]):
        assert same([np.asarray(g) for g in merge_top2(parts)], want)
    # three shards: the tie's winner is the first of the three, not the last compared
    c = _part((205, 10, 11), none, none, (260, 7, 9), none)
    got = merge_top2([a, b, c])
    want3 = _part((5, 10, 10), (140, 20, 256), (150, 9, 30), (160, 7, 7), none)
    assert same([np.asarray(g) for g in got], want3)
    # one shard alone is returned as it is
    assert same([np.asarray(g) for g in merge_top2([a])], a)


def test_merge_top2_on_tensors():
    import torch
    a = _part((5, 10, 40), (-1, 256, 256))
    b = _part((105, 10, 12), (140, 20, 256))
    got = merge_top2([tuple(torch.from_numpy(x) for x in p) for p in (a, b)])
    assert same([g.numpy() for g in got], _part((5, 10, 10), (140, 20, 256)))


# ---- census ------------------------------------------------------------------------------------

# what a tie's / a split's name claims about its two rows (a = the best's position, b = the
# second's; bf_cases.where)
GEOMETRY = {
    "tie_even_odd_of_a_pair": lambda a, b: not a["tail"] and (a["block"], a["pair"]) ==
    (b["block"], b["pair"]) and a["chunk"] == b["chunk"] and (a["odd"], b["odd"]) == (0, 1),
    "tie_odd_even_pairs": lambda a, b: not b["tail"] and a["odd"] == 1 and b["odd"] == 0 and
    b["e"] == a["e"] + 1 and a["block"] == b["block"],
    "tie_3_4_halfwaves": lambda a, b: (a["e"], b["e"]) == (3, 4) and
    a["halfwave"] != b["halfwave"],
    "tie_7_8": lambda a, b: (a["e"], b["e"]) == (7, 8) and a["halfwave"] != b["halfwave"],
    "tie_31_32_blocks": lambda a, b: b["blk32"] == a["blk32"] + 1 and a["sb"] == b["sb"] and
    b["e"] == a["e"] + 1,
    "tie_127_128_superblocks": lambda a, b: b["sb"] == a["sb"] + 1 and b["e"] == a["e"] + 1,
    "tie_247_248_epilogue": lambda a, b: (a["e"], b["e"]) == (247, 248) and not b["tail"],
    "tie_chunk_to_chunk": lambda a, b: b["chunk"] == a["chunk"] + 1 and a["e"] == a["n"] - 1 and
    b["e"] == 0,
    "tie_4_8_halfwaves": lambda a, b: (a["e"] % 32, b["e"] % 32) == (4, 8) and
    a["blk32"] == b["blk32"] and a["halfwave"] != b["halfwave"],
    "tie_0_255_of_a_block": lambda a, b: (a["e"] % 256, b["e"] % 256) == (0, 255) and
    a["block"] == b["block"] and a["chunk"] == b["chunk"] and not b["tail"],
    "tie_block_to_block": lambda a, b: a["chunk"] == b["chunk"] and b["block"] == a["block"] + 1
    and not b["tail"] and b["e"] == a["e"] + 1,
    "tie_block_to_tail": lambda a, b: a["chunk"] == b["chunk"] and not a["tail"] and b["tail"] and
    b["e"] == a["e"] + 1,
    "tie_tail_to_tail": lambda a, b: a["chunk"] == b["chunk"] and a["tail"] and b["tail"] and
    b["e"] == b["n"] - 1,
    "split_halves_even_best": lambda a, b: not b["tail"] and a["block"] == b["block"] and
    (a["odd"], b["odd"]) == (0, 1),
    "split_halves_odd_best": lambda a, b: not a["tail"] and a["block"] == b["block"] and
    (a["odd"], b["odd"]) == (1, 0) and b["e"] < a["e"],
    "split_halfwaves_later_best": lambda a, b: a["blk32"] == b["blk32"] and
    a["halfwave"] != b["halfwave"] and b["e"] < a["e"],
    "split_superblocks_later_best": lambda a, b: a["chunk"] == b["chunk"] and a["sb"] > b["sb"],
    "split_chunks_later_best": lambda a, b: a["chunk"] > b["chunk"],
    "split_chunks_earlier_best": lambda a, b: a["chunk"] < b["chunk"],
    "split_blocks_earlier_best": lambda a, b: a["chunk"] == b["chunk"] and
    a["block"] < b["block"] and not b["tail"],
    "split_blocks_later_best": lambda a, b: a["chunk"] == b["chunk"] and
    a["block"] > b["block"] and not a["tail"],
    "split_block_tail_later_best": lambda a, b: a["chunk"] == b["chunk"] and a["tail"] and
    not b["tail"],
}
GEOMETRY["tie_chunk_to_chunk_512"] = GEOMETRY["tie_chunk_to_chunk"]


def _pair_check(name):
    table, pairs = (bc.TIES, "ties") if name in bc.TIES else (bc.SPLITS, "splits")
    chunk, r1, r2 = table[name]

    def check(c):
        return c.chunk_rows() == chunk and (r1, r2) in getattr(c, pairs)() and \
            GEOMETRY[name](where(c, r1), where(c, r2))
    return check


def _bests(c):
    return {e[0] for e in c.expect.values()}


def _swept(c, rows):
    s = c.splits()
    return {a for a, _ in s} >= set(rows) and {b for _, b in s} >= set(rows)


def _three_way(c, chunk, pred):
    for i, pl in c.near.items():
        d1 = c.expect[i][1]
        rows = sorted(r for r, d in pl if d == d1)
        if len(rows) >= 3 and c.expect[i][2] == d1 and c.chunk_rows() == chunk and \
                pred(d1, [where(c, r) for r in rows]):
            return True
    return False


def _row_at(c, dist_value, pred):
    """Some query with a usable outcome has a row at `dist_value` where pred(row) holds."""
    d = c.dist()
    for i, e in c.expect.items():
        if e[0] >= 0 and any(pred(int(r)) for r in np.nonzero(d[i] == dist_value)[0]):
            return True
    return False


def _best_in_last_superblock(c, blocks):
    for i, e in c.expect.items():
        if e[0] >= 0:
            w = where(c, e[0])
            if w["sb_blocks"] == blocks and w["sb"] == (-(-w["n"] // 32) - 1) // 4:
                return True
    return False


def _merge_family(c, n):
    last, s = n - 1, {(where(c, a)["chunk"], where(c, b)["chunk"]) for a, b in c.splits()}
    return c.regime(MFMA)["nchunks"] == n and c.chunk_rows() == 256 and c.ndb % 256 == 100 and \
        (last, 0) in s and (0, last) in s


def _tie_chunks(c, ca, cb):
    return any((where(c, a)["chunk"], where(c, b)["chunk"]) == (ca, cb) for a, b in c.ties())


CHECKS = {
    **{name: _pair_check(name) for name in list(bc.TIES) + list(bc.SPLITS)},
    "bit_pairing": lambda c: c.nq == 256 and c.ndb == 256 and
    (bc.POP[c.q].sum(axis=1) == 1).all() and (bc.POP[c.db].sum(axis=1) == 1).all() and
    sorted(_bests(c)) == list(range(256)) and (c.db != c.q).any(),
    "sweep_valu_first_block": lambda c: c.chunk_rows() == 512 and _swept(c, range(0, 256)),
    "sweep_valu_last_block": lambda c: c.chunk_rows() == c.ndb == 512 and
    _swept(c, range(256, 512)),
    "sweep_mfma_first_superblock": lambda c: c.chunk_rows() == 512 and _swept(c, range(0, 128)),
    "sweep_mfma_last_superblock": lambda c: c.chunk_rows() == c.ndb == 512 and
    _swept(c, range(384, 512)),
    # k_bf_top2's grid x is nqpad / 256 = 4: here the second block's queries are live
    "valu_second_query_block_live": lambda c: c.regime(VALU)["query_blocks"] == 4 and
    c.regime(MFMA)["query_blocks"] == 1 and c.nq == 512 and max(c.expect) == 511,
    "tie_three_way_duplicates_d0": lambda c: _three_way(
        c, 256, lambda d, w: d == 0 and len({x["chunk"] for x in w}) == 3),
    "tie_three_way_one_half": lambda c: _three_way(
        c, 256, lambda d, w: len({(x["chunk"], x["block"], x["odd"], x["sb"], x["halfwave"])
                                  for x in w}) == 1 and not w[0]["tail"]),
    "tie_three_way_blocks": lambda c: _three_way(
        c, 512, lambda d, w: {x["block"] for x in w} == {0, 1} and not w[-1]["tail"]),
    "tie_three_way_tail": lambda c: _three_way(
        c, 320, lambda d, w: w[0]["tail"] and w[1]["tail"] and w[2]["chunk"] == 1),
    **{f"ndb_{n}": (lambda n: lambda c: c.ndb == n and c.chunk is None and any(
        e[0] == n - 1 and e[2] > e[1] for e in c.expect.values()))(n) for n in bc.PARTIAL_ENDS},
    "ndb_0": lambda c: c.ndb == 0 and c.nq > 0 and set(c.expect.values()) == {(-1, 256, 256)},
    "complement_row0_of_chunk": lambda c: _row_at(c, 256, lambda r: r % c.chunk_rows() == 0 and
                                                  r > 0) and _row_at(c, 256, lambda r: r == 0),
    "complement_odd_row": lambda c: _row_at(c, 256, lambda r: r % 2 == 1),
    "all_256": lambda c: c.ndb > 256 and (c.dist()[0] == 256).all() and
    c.expect[0] == (-1, 256, 256),
    "one_255": lambda c: sorted(c.dist()[0])[:2] == [255, 256] and c.expect[0][0] % 2 == 1 and
    c.expect[0][0] > c.chunk_rows(),
    "d1_d255_one_half": lambda c: sorted(c.dist()[0])[:3] == [1, 255, 256] and
    (lambda a, b: a["block"] == b["block"] and a["odd"] == b["odd"] and
     abs(a["pair"] - b["pair"]) == 1)(*[where(c, r) for r, _ in c.near[0]]),
    **{f"chunk_{n}": (lambda n: lambda c: c.chunk == n and c.ndb > n)(n) for n in (512, 576, 1024)},
    "last_superblock_1_block": lambda c: _best_in_last_superblock(c, 1),
    "last_superblock_2_blocks": lambda c: _best_in_last_superblock(c, 2),
    "last_superblock_3_blocks": lambda c: _best_in_last_superblock(c, 3),
    **{f"nq_{n}": (lambda n: lambda c: c.nq == n and c.ndb == 600 and c.chunk == 256 and all(
        c.expect[i][0] == (i * 7919) % 600 for i in range(n)))(n) for n in bc.NQ_SWEEP},
    **{f"nchunks_{n}": (lambda n: lambda c: _merge_family(c, n) if n > 1 else
                        c.regime(MFMA)["nchunks"] == 1)(n) for n in bc.MERGE_NCHUNKS},
    **{f"merge_tie_slices_0_1_L{L}": (lambda L: lambda c: c.regime(MFMA)["merge_slice"] == L and
                                      _tie_chunks(c, L - 1, L))(L) for L in (1, 2, 3, 8, 9, 10)},
    **{f"merge_tie_partials_7_8_L{L}": (lambda L: lambda c: c.regime(MFMA)["merge_slice"] == L and
                                        _tie_chunks(c, 7, 8))(L) for L in (9, 10)},
    "row_field_limit": lambda c: c.chunk == bc.CHUNK_MAX and c.ndb == (1 << 23) + 192 and
    (c.chunk - 1, c.chunk) in c.ties() and c.ndb - 1 in _bests(c) and c.device_only,
    "idx_base_max": lambda c: c.idx_base + c.ndb == bc.INT_MAX - 1 and c.ndb - 1 in _bests(c),
    "none_not_offset": lambda c: c.idx_base > 0 and -1 in _bests(c),
}


def test_census_constructs():
    """Every construct a case claims occurs in it, every construct of the table is claimed,
    and every case is the only holder of at least one (removing a case uncovers something)."""
    holders = {}
    for c in bc.cases():
        assert c.constructs, f"{c.name} claims nothing"
        for con in c.constructs:
            assert con in CHECKS, f"{c.name}: construct {con} has no check"
            assert CHECKS[con](c), f"{c.name}: construct {con} does not occur"
            holders.setdefault(con, []).append(c.name)
    # merge cases tag their ties by L; not every L of the table exists (8 -> L = 1 has chunk 1)
    unclaimed = {k for k in CHECKS if k not in holders}
    assert not unclaimed, sorted(unclaimed)
    for c in bc.cases():
        assert any(len(holders[con]) == 1 for con in c.constructs), \
            f"{c.name} is redundant: {c.constructs}"


# the case (and kernel) each variant is expected to change at the least: the census fails if a
# variant stops being noticed there, and prints every case that notices it
NOTICED_BY = {
    "later_row_wins_in_block": ("ties_c256", VALU),
    "odd_half_first": ("ties_c256", VALU),
    "fold_drops_seconds": ("sweep_512", VALU),
    "signed_min_max": ("d1_d255", VALU),
    "dist256_becomes_best": ("all_256", MFMA),
    "mfma_tail_unmasked": ("ndb_33", MFMA),
    "mfma_fold_e0": ("sweep_512", MFMA),
    "mfma_no_halfwave_fold": ("ties_c256", MFMA),
    "bx_ignored": ("nq_1025", MFMA),
    "merge_le": ("ties_c256", VALU),
    "merge_slice_floor": ("merge_9", MFMA),
    "merge_batch_unmasked": ("merge_9", MFMA),
    "row_22_bits": ("row_limit", VALU),
    "base_added_to_none": ("idx_base_none", MFMA),
}


def test_census_variants():
    """Each variant flips one decision of the model; each must change the outcome of at least
    one case (a kernel that took the flipped decision would then differ from the oracle on that
    case on the GPU).  Prints which."""
    hits = {v: [] for v in bc.VARIANTS}
    for c in bc.cases():
        want = c.with_base(ref_of(c.name))
        for k in c.kernels:
            for v in c.variants:
                got = bc.model_top2(c.q, c.db, c.chunk_rows(), k, v, idx_base=c.idx_base,
                                    d=c.dist())
                if not same(got, want):
                    hits[v].append((c.name, k))
    for v in bc.VARIANTS:
        print(f"variant {v}: " + ", ".join(f"{n}/{bc.KERNEL_NAMES[k]}" for n, k in hits[v]))
    assert set(NOTICED_BY) == set(bc.VARIANTS)
    missing = [v for v in bc.VARIANTS if NOTICED_BY[v] not in hits[v]]
    assert not missing, {v: hits[v] for v in missing}
    # the kernel-specific variants leave the other kernel's outcomes alone
    for v in ("mfma_tail_unmasked", "mfma_fold_e0", "mfma_no_halfwave_fold"):
        assert all(k == MFMA for _, k in hits[v]), v
    assert all(k == VALU for _, k in hits["odd_half_first"])
