"""Directed brute-force Hamming top-2 cases for the kernels of orbx_bf.hip (k_bf_top2,
k_bf_mfma, k_bf_merge), a plain exact reference, and a structural model of the kernels.

The contract (include/orbx_match.h, orbx_hamming_bf_top2): best = the FIRST row at the least
distance below 256 (-1 if none), second = the second least of the multiset {256, 256} ∪
distances, so it equals the best on a tie.

  reference_top2   the contract, plainly: a byte-popcount table over q[:, None] ^ db[None] in
                   slabs of rows, the first argmin and the second least per slab, slabs joined
                   in row order.
  Case             q, db, chunk (None = automatic), kernels, idx_base, and per query of interest
                   the outcome its construction implies.  tests/test_bf_cases.py asserts that
                   the reference gives exactly that, so a noise row that undercuts a planted
                   distance fails the case's own construction on the CPU, not on the GPU.
  model_top2       the kernels' decomposition in numpy (not their instructions): chunks, packed
                   256-row blocks with two 16-bit halves (k_bf_top2) or 32-row blocks in 128-row
                   superblocks per half-wave (k_bf_mfma), 32-bit (distance << 23 | row) keys per
                   chunk, and the eight-slice merge in batches of 8.  With variant=None it
                   equals the reference; each VARIANTS entry flips one decision, and the census
                   shows that every flip changes some case's outcome, i.e. a kernel that took
                   the flipped decision would fail that case on the GPU.

Two ways to build a case.  Builder: noise rows and noise queries, and per query a list of
planted rows (the query with `dist` bits flipped, plant()); planted distances stay <= 40, a
256-bit noise row is 128 +- 8 from any query.  paired rows (where more queries than rows need a
stated outcome, or every row must be both a best and a second): rows r and p(r) differ in a
24-bit mask, a query is row r with d < 12 bits OF THAT MASK flipped, so it is d from r and
24 - d from p(r).  Constant backgrounds give closed forms where noise would not.
"""
import numpy as np

MFMA, VALU = 0, 1                    # ORBX_BF_MFMA, ORBX_BF_VALU
KERNEL_NAMES = {MFMA: "k_bf_mfma", VALU: "k_bf_top2"}
BLK = 256                            # rows per packed block of k_bf_top2
MFMA_Q = 1024                        # queries per k_bf_mfma workgroup (k_bf_top2: 256)
ROW_BITS = 23
CHUNK_MAX = (1 << ROW_BITS) - 64
INT_MAX = 2**31 - 1
AUTO_CHUNK_SMALL = 256               # bf_chunk_rows up to 2048 rows: the 256-row floor
PAIR_BITS = 24

POP = np.array([bin(i).count("1") for i in range(256)], np.uint16)

VARIANTS = (
    "later_row_wins_in_block",   # 16-bit keys order a tie by the LAST row of a block
    "odd_half_first",            # the halves meet by (distance, pair), the odd row first
    "fold_drops_seconds",        # only the 16-bit bests reach the chunk's 32-bit top-2
    "signed_min_max",            # 16-bit min / max compare as signed
    "dist256_becomes_best",      # a row at 256 replaces "none"
    "mfma_tail_unmasked",        # re-read rows past n of the last block count
    "mfma_fold_e0",              # superblock fold adds e0, not e0 - 32 j
    "mfma_no_halfwave_fold",     # lanes 0-31's rows only
    "bx_ignored",                # every query block computes the first block's queries
    "merge_le",                  # `e1 <= d1`: a later chunk takes a tie
    "merge_slice_floor",         # L = nchunks / 8 rounded down
    "merge_batch_unmasked",      # a batch's entries past c1 (re-reads of chunk c1 - 1) count
    "row_22_bits",               # the row field is 22 bits wide
    "base_added_to_none",        # idx_base is added to -1
)


# ---- reference ------------------------------------------------------------------------------

def distances(q, db, slab_bytes=1 << 26):
    """[nq, ndb] int32 Hamming distances by the byte-popcount table, in slabs of rows."""
    nq, ndb = len(q), len(db)
    out = np.empty((nq, ndb), np.int32)
    step = max(1, slab_bytes // (32 * max(nq, 1)))
    for s in range(0, ndb, step):
        out[:, s:s + step] = POP[q[:, None, :] ^ db[None, s:s + step, :]].sum(axis=2)
    return out


def top2_of_distances(d):
    """The contract on a distance matrix."""
    nq = d.shape[0]
    if d.shape[1] == 0:
        return (np.full(nq, -1, np.int32), np.full(nq, 256, np.int32), np.full(nq, 256, np.int32))
    ext = np.concatenate([d, np.full((nq, 2), 256, np.int32)], axis=1)
    two = np.partition(ext, 1, axis=1)[:, :2]
    b1, b2 = two[:, 0], two[:, 1]
    idx = np.where(b1 < 256, np.argmin(d, axis=1), -1)
    return idx.astype(np.int32), b1.astype(np.int32), b2.astype(np.int32)


def reference_top2(q, db, slab_rows=None):
    """Exact top-2 of every query over every row; slabs of rows keep the largest case's
    temporaries far below 1 GB.  Slabs are joined in row order: the earlier slab keeps a tie."""
    nq, ndb = len(q), len(db)
    step = slab_rows or max(1, (1 << 26) // (32 * max(nq, 1)))
    idx = np.full(nq, -1, np.int64)
    b1 = np.full(nq, 256, np.int32)
    b2 = np.full(nq, 256, np.int32)
    for s in range(0, ndb, step):
        d = POP[q[:, None, :] ^ db[None, s:s + step, :]].sum(axis=2).astype(np.int32)
        i, e1, e2 = top2_of_distances(d)
        four = np.sort(np.stack([b1, b2, e1, e2], axis=1), axis=1)
        idx = np.where(e1 < b1, i.astype(np.int64) + s, idx)
        b1, b2 = four[:, 0], four[:, 1]
    return idx.astype(np.int32), b1.astype(np.int32), b2.astype(np.int32)


# ---- builders -------------------------------------------------------------------------------

def flipped(desc, bits):
    out = desc.copy()
    for b in bits:
        out[int(b) // 8] ^= np.uint8(1 << (int(b) % 8))
    return out


def plant(db, q, i, row, dist, rng):
    """db[row] = q[i] with `dist` chosen bits flipped."""
    assert 0 <= dist <= 256 and 0 <= row < len(db)
    db[row] = flipped(q[i], rng.choice(256, dist, replace=False))


def from_plants(plants):
    """The outcome a query's (row, distance) list implies when no other row is nearer: the
    first row at the least distance, and the second least of {256, 256} ∪ distances."""
    ds = sorted([d for _, d in plants] + [256, 256])
    if ds[0] >= 256:
        return (-1, 256, 256)
    return (min(r for r, d in plants if d == ds[0]), ds[0], ds[1])


class Case:
    """One call: q (nq x 32), db (ndb x 32), chunk (None: automatic), the kernels it applies to,
    idx_base.  expect[i] = (best_idx, best_dist, second_dist) of query i, best_idx WITHOUT
    idx_base (-1 stays -1); near[i] = the (row, distance) pairs that decide query i (what the
    census reads a case's constructs from); constructs = the tags the census checks."""

    def __init__(self, name, q, db, chunk, expect, constructs, near=None, idx_base=0,
                 kernels=(MFMA, VALU), device_only=False, variants=VARIANTS):
        assert q.dtype == np.uint8 and db.dtype == np.uint8
        assert q.shape[1:] == (32,) and db.shape[1:] == (32,)
        self.name, self.q, self.db, self.chunk = name, q, db, chunk
        self.expect, self.constructs = dict(expect), tuple(constructs)
        self.near = dict(near or {})
        self.idx_base, self.kernels, self.device_only = idx_base, tuple(kernels), device_only
        self.variants = tuple(variants)      # the variants the census tries on this case
        self._d = None

    nq = property(lambda self: len(self.q))
    ndb = property(lambda self: len(self.db))

    def chunk_rows(self):
        """The chunk the call runs with.  An automatic chunk is the 256-row floor: the table
        keeps such cases at or below 2048 rows, where every CU count gives it."""
        if self.chunk is None:
            assert self.ndb <= 2048
            return AUTO_CHUNK_SMALL
        return self.chunk

    def regime(self, kernel):
        """What orbx_matcher_bf_launch_info must report for this case."""
        chunk = self.chunk_rows()
        nchunks = -(-self.ndb // chunk)
        nqpad = -(-self.nq // MFMA_Q) * MFMA_Q
        return dict(chunk=chunk, nchunks=nchunks, nqpad=nqpad,
                    query_blocks=nqpad // (MFMA_Q if kernel == MFMA else 256),
                    merge_slice=-(-nchunks // 8), partial_bytes=8 * nchunks * nqpad)

    def dist(self):
        if self._d is None:
            self._d = distances(self.q, self.db)
        return self._d

    def with_base(self, ref):
        """Result arrays with idx_base applied (what a device call must return)."""
        idx = np.where(ref[0] >= 0, ref[0].astype(np.int64) + self.idx_base, -1)
        return idx.astype(np.int32), ref[1], ref[2]

    # -- what the census reads --
    def ties(self):
        """(r1, r2): the first two rows of every query whose best and second tie."""
        out = set()
        for i, pl in self.near.items():
            _, d1, d2 = self.expect[i]
            rows = sorted(r for r, d in pl if d == d1)
            if d1 == d2 and len(rows) >= 2:
                out.add((rows[0], rows[1]))
        return out

    def splits(self):
        """(best row, second row) of every query with a unique best and a unique second."""
        out = set()
        for i, pl in self.near.items():
            _, d1, d2 = self.expect[i]
            r1 = [r for r, d in pl if d == d1]
            r2 = [r for r, d in pl if d == d2]
            if d1 < d2 and len(r1) == 1 and len(r2) == 1:
                out.add((r1[0], r2[0]))
        return out


class Builder:
    """A noise database and noise queries with planted near copies."""

    def __init__(self, name, ndb, chunk, seed):
        self.name, self.chunk = name, chunk
        self.rng = np.random.default_rng(seed)
        self.db = self.rng.integers(0, 256, (ndb, 32), dtype=np.uint8)
        self.qs, self.expect, self.near, self.used = [], {}, {}, set()

    def query(self, plants):
        """A new noise query with rows planted at the given (row, distance) pairs; a row serves
        one query only.  Returns the query's index."""
        i = len(self.qs)
        self.qs.append(self.rng.integers(0, 256, 32, dtype=np.uint8))
        for row, dist in plants:
            assert dist <= 40, "planted distances stay clear of the noise (128 +- 8)"
            assert row not in self.used, f"{self.name}: row {row} planted twice"
            self.used.add(row)
            plant(self.db, self.qs, i, row, dist, self.rng)
        self.expect[i] = from_plants(plants)
        self.near[i] = list(plants)
        return i

    def case(self, constructs, **kw):
        return Case(self.name, np.stack(self.qs), self.db, self.chunk, self.expect, constructs,
                    near=self.near, **kw)


def paired_rows(ndb, partner, rng):
    """Noise rows in pairs: db[partner(r)] = db[r] with the PAIR_BITS bits of mask[r] flipped
    (partner is an involution without fixed points)."""
    db = rng.integers(0, 256, (ndb, 32), dtype=np.uint8)
    mask = {}
    for r in range(ndb):
        p = partner(r)
        assert p != r and partner(p) == r and 0 <= p < ndb
        if r < p:
            mask[r] = mask[p] = rng.choice(256, PAIR_BITS, replace=False)
            db[p] = flipped(db[r], mask[r])
    return db, mask


def near_row(db, mask, r, d, rng):
    """A query d < 12 from row r and 24 - d from its partner."""
    assert 0 <= d < PAIR_BITS // 2
    return flipped(db[r], rng.choice(mask[r], d, replace=False))


# ---- positions (what the census reads a construct from) ---------------------------------------

def where(case, row):
    """Where global row `row` sits in each kernel's decomposition of this case."""
    chunk = case.chunk_rows()
    c, e = divmod(row, chunk)
    n = min(chunk, case.ndb - c * chunk)
    full = (n // BLK) * BLK
    return dict(chunk=c, e=e, n=n, tail=e >= full, block=e // BLK, pair=(e % BLK) // 2,
                odd=e & 1, blk32=e // 32, sb=e // 128, halfwave=(e >> 2) & 1,
                sb_blocks=min(4, -(-n // 32) - 4 * (e // 128)))


# ---- the cases ------------------------------------------------------------------------------

def _bit_pairing():
    """256 one-hot queries against 256 one-hot rows in a fixed permutation: best = the row
    with the query's bit at distance 0, every other row is at 2.  The only case that fails if
    the A and B MFMA fragments disagree on which bit element j of step s, half h is; it equally
    pins expand16 and the 16 * h shift (noise cannot: a permutation of the bits applied to
    queries and rows alike keeps every distance, one applied to one side only moves the 0)."""
    perm = (np.arange(256) * 37 + 11) % 256            # row r holds bit perm[r]
    eye = np.zeros((256, 32), np.uint8)
    for b in range(256):
        eye[b, b // 8] = 1 << (b % 8)
    inv = np.argsort(perm)
    expect = {i: (int(inv[i]), 0, 2) for i in range(256)}
    return Case("bit_pairing", eye.copy(), eye[perm].copy(), 256, expect, ["bit_pairing"])


def _sweep():
    """One 512-row chunk = two packed blocks = four superblocks.  Rows pair up, r with r ^ 2 in
    the first block (the same 16-bit half and, where r & 4 agrees, the same half-wave: both of a
    half's top-2 are needed) and r with r ^ 5 in the last (the other half, the other half-wave).
    Query k is near row k: every row is one query's unique best and its partner's query's
    unique second.  512 queries: a second query block for k_bf_top2."""
    rng = np.random.default_rng(102)
    db, mask = paired_rows(512, lambda r: r ^ 2 if r < 256 else r ^ 5, rng)
    q, expect, near = [], {}, {}
    for r in range(512):
        d = 1 + r % 9
        p = r ^ 2 if r < 256 else r ^ 5
        q.append(near_row(db, mask, r, d, rng))
        expect[r] = (r, d, PAIR_BITS - d)
        near[r] = [(r, d), (p, PAIR_BITS - d)]
    return Case("sweep_512", np.stack(q), db, 512, expect,
                ["sweep_valu_first_block", "sweep_valu_last_block", "sweep_mfma_first_superblock",
                 "sweep_mfma_last_superblock", "valu_second_query_block_live"], near=near)


# name -> (chunk, r1, r2): a tie (best at r1, second equal) between these global rows
TIES = {
    "tie_even_odd_of_a_pair": (256, 10, 11),
    "tie_odd_even_pairs": (256, 21, 22),
    "tie_3_4_halfwaves": (256, 3, 4),
    "tie_7_8": (256, 7, 8),
    "tie_31_32_blocks": (256, 31, 32),
    "tie_127_128_superblocks": (256, 127, 128),
    "tie_247_248_epilogue": (256, 247, 248),
    "tie_chunk_to_chunk": (256, 255, 256),
    "tie_4_8_halfwaves": (256, 260, 264),
    "tie_0_255_of_a_block": (256, 512, 767),
    "tie_block_to_block": (512, 255, 256),
    "tie_chunk_to_chunk_512": (512, 511, 512),
    "tie_block_to_tail": (320, 255, 256),
    "tie_tail_to_tail": (320, 300, 319),
}
# name -> (chunk, best row, second row): unique best, unique second greater
SPLITS = {
    "split_halves_even_best": (256, 40, 43),
    "split_halves_odd_best": (256, 51, 48),
    "split_halfwaves_later_best": (256, 68, 65),
    "split_superblocks_later_best": (256, 200, 100),
    "split_chunks_later_best": (256, 600, 150),
    "split_chunks_earlier_best": (256, 160, 610),
    "split_blocks_earlier_best": (512, 30, 290),
    "split_blocks_later_best": (512, 300, 40),
    "split_block_tail_later_best": (320, 310, 50),
}


def _ties(chunk, ndb, seed, extra=()):
    b = Builder(f"ties_c{chunk}", ndb, chunk, seed)
    cons = []
    for k, (name, (ch, r1, r2)) in enumerate(TIES.items()):
        if ch == chunk:
            b.query([(r1, 3 + k), (r2, 3 + k)])
            cons.append(name)
    for k, (name, (ch, r1, r2)) in enumerate(SPLITS.items()):
        if ch == chunk:
            b.query([(r1, 4 + k), (r2, 9 + k)])
            cons.append(name)
    for name, plants in extra:
        b.query(plants)
        cons.append(name)
    return b.case(cons)


def _tie_cases():
    return [
        # three chunks of 256; a three-way tie at distance 0 (exact duplicates) over three chunks
        # and one inside one 16-bit half of a packed block = one half-wave of a superblock
        # (rows 74, 82, 90 of the second chunk): only there does the order INSIDE a block's
        # 16-bit top-2 decide, both of a half's entries reach the 32-bit keys otherwise
        _ties(256, 768, 103, [("tie_three_way_duplicates_d0", [(230, 0), (420, 0), (700, 0)]),
                              ("tie_three_way_one_half", [(330, 4), (338, 4), (346, 4)])]),
        # two packed blocks per chunk, two chunks; a three-way tie over both blocks
        _ties(512, 1024, 104, [("tie_three_way_blocks", [(100, 6), (400, 6), (401, 6)])]),
        # one packed block and a 64-row tail per chunk; the last chunk is all tail (100 rows)
        _ties(320, 420, 105, [("tie_three_way_tail", [(257, 6), (258, 6), (400, 6)])]),
    ]


PARTIAL_ENDS = (1, 2, 5, 31, 33, 127, 129, 255, 257, 319)


def _partial_end(ndb):
    """The unique best at the last row, ndb - 1, the second strictly greater at row 0 (256 for
    one row); a second query the other way round.  k_bf_mfma's fetch re-reads row n - 1 for the
    rows past it: unmasked, the re-reads make the second equal the best."""
    b = Builder(f"ndb_{ndb}", ndb, None, 200 + ndb)
    if ndb == 1:
        b.query([(0, 5)])
    else:
        b.query([(ndb - 1, 5), (0, 9)])
        if ndb >= 5:
            b.query([(1, 4), (ndb - 2, 11)])
    return b.case([f"ndb_{ndb}"])


def _empty():
    q = np.random.default_rng(106).integers(0, 256, (3, 32), dtype=np.uint8)
    return Case("ndb_0", q, np.zeros((0, 32), np.uint8), None,
                {i: (-1, 256, 256) for i in range(3)}, ["ndb_0"])


def _extreme_cases():
    rng = np.random.default_rng(107)
    out = []
    # complements (distance 256) at row 0 of both chunks and at odd rows, among planted rows:
    # they must neither become the best nor disturb the keys next to them
    b = Builder("complements", 512, 256, 108)
    i0 = b.query([(100, 7), (300, 9)])
    i1 = b.query([(258, 6), (2, 8)])
    for i, rows in ((i0, (0, 256, 101)), (i1, (257, 3, 511))):
        for r in rows:
            b.db[r] = ~b.qs[i]
    out.append(b.case(["complement_row0_of_chunk", "complement_odd_row"]))
    # every row at 256 from query 0: (-1, 256, 256); query 1 = query 0 with one bit flipped is
    # 255 from every row: a tie at 255 everywhere, the first row wins
    q0 = rng.integers(0, 256, 32, dtype=np.uint8)
    q = np.stack([q0, flipped(q0, [0])])
    db = np.tile(~q0, (300, 1))
    out.append(Case("all_256", q, db, 256, {0: (-1, 256, 256), 1: (0, 255, 255)}, ["all_256"]))
    # one row at 255 (an odd row of the second chunk), the rest at 256
    db = np.tile(~q0, (300, 1))
    db[257] = flipped(db[257], [77])
    out.append(Case("one_255", q0[None].copy(), db, 256, {0: (257, 255, 256)}, ["one_255"],
                    near={0: [(257, 255)]}))
    # 255 and 1 in neighbouring pairs of one 16-bit half (rows 10 and 12), the rest at 256:
    # keys 255 << 7 | 5 = 32645 and 1 << 7 | 6 sit either side of the signed 16-bit range's end
    db = np.tile(~q0, (256, 1))
    db[10] = flipped(db[10], [5])
    db[12] = flipped(q0, [200])
    out.append(Case("d1_d255", q0[None].copy(), db, 256, {0: (12, 1, 255)}, ["d1_d255_one_half"],
                    near={0: [(10, 255), (12, 1)]}))
    return out


def _multi_block_cases():
    out = []
    # chunk 512, last chunk 160 rows: k_bf_mfma's last superblock has 1 block (k_bf_top2: all
    # tail); best / second over the two packed blocks are in ties_c512
    b = Builder("multi_512", 512 + 160, 512, 110)
    b.query([(512 + 130, 5), (512 + 3, 9)])        # best in the 1-block superblock
    b.query([(512 + 20, 5), (512 + 159, 5)])       # tie, second at the chunk's last row
    out.append(b.case(["chunk_512", "last_superblock_1_block"]))
    # chunk 576 = 2 packed blocks + 64 tail rows = 4 superblocks + 2 blocks; last chunk 224
    # rows = 1 superblock + 3 blocks
    b = Builder("multi_576", 576 + 224, 576, 111)
    b.query([(540, 5), (10, 9)])                    # best in the 2-block superblock / the tail
    b.query([(300, 4), (575, 8)])                   # best in block 1, second at the chunk's end
    b.query([(511, 6), (512, 6)])                   # tie block to tail, superblock 3 to 4
    b.query([(576 + 200, 5), (576 + 100, 9)])       # best in the 3-block superblock
    b.query([(576 + 127, 7), (576 + 223, 7)])       # tie into the 3-block superblock's end
    out.append(b.case(["chunk_576", "last_superblock_2_blocks", "last_superblock_3_blocks"]))
    # chunk 1024 = 4 packed blocks = 8 superblocks; two chunks
    b = Builder("multi_1024", 2048, 1024, 112)
    b.query([(800, 5), (20, 9)])                    # best in block 3, second in block 0
    b.query([(30, 5), (1000, 9)])                   # the reverse
    b.query([(511, 6), (768, 6)])                   # tie blocks 1 and 3
    b.query([(1023, 7), (1024, 7)])                 # tie chunk to chunk
    b.query([(1024 + 700, 3), (1024 + 300, 3), (600, 8)])
    out.append(b.case(["chunk_1024"]))
    return out


NQ_SWEEP = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049)
_geometry_rows = None


def _query_geometry(nq):
    """600 paired rows (r with r + 300 mod 600) in three chunks of 256; query i is near row
    (i * 7919) mod 600: any wrong query-to-output mapping (tile, wave, bx, the nqpad stride)
    shows as a wrong index."""
    global _geometry_rows
    if _geometry_rows is None:
        _geometry_rows = paired_rows(600, lambda r: (r + 300) % 600, np.random.default_rng(113))
    db, mask = _geometry_rows
    rng = np.random.default_rng(300 + nq)
    q, expect, near = [], {}, {}
    for i in range(nq):
        r, d = (i * 7919) % 600, 1 + i % 9
        q.append(near_row(db, mask, r, d, rng))
        expect[i] = (r, d, PAIR_BITS - d)
        near[i] = [(r, d), ((r + 300) % 600, PAIR_BITS - d)]
    return Case(f"nq_{nq}", np.stack(q), db, 256, expect, [f"nq_{nq}"], near=near)


MERGE_NCHUNKS = (1, 2, 7, 8, 9, 16, 17, 63, 64, 65, 72, 73)


def _merge_case(nchunks):
    """chunk = 256, a short last chunk (100 rows).  Best in the last chunk with the second in
    the first and the reverse; where they exist, ties across the slice boundary (chunks L - 1
    and L) and across partials 7 / 8 of slice 0 (two batches of 8)."""
    ndb = (nchunks - 1) * 256 + 100
    L = -(-nchunks // 8)
    b = Builder(f"merge_{nchunks}", ndb, 256, 400 + nchunks)
    cons = [f"nchunks_{nchunks}"]
    last = (nchunks - 1) * 256
    if nchunks == 1:
        b.query([(90, 5), (10, 9)])
        b.query([(20, 5), (99, 9)])
    else:
        b.query([(last + 90, 5), (10, 9)])
        b.query([(20, 5), (last + 99, 9)])
    if L < nchunks:
        b.query([((L - 1) * 256 + 200, 6), (L * 256 + 50, 6)])
        cons.append(f"merge_tie_slices_0_1_L{L}")
    if L >= 9:
        b.query([(7 * 256 + 33, 7), (8 * 256 + 44, 7)])
        cons.append(f"merge_tie_partials_7_8_L{L}")
    return b.case(cons)


def _row_limit():
    """The row field at its limit: chunk = 2^23 - 64, ndb = 2^23 + 192 (a second chunk of 256
    rows), device entry only (268 MB of rows).  Every row is one constant descriptor B; the
    queries are B with 80 bits flipped (disjoint bit ranges), so the background is at 80.
      query 0: rows chunk - 1 and chunk at 10: a tie, the earlier row (row field all ones but
               the low six bits) wins;
      query 1: the last row at 7, second = the background's 80;
      query 2: nothing below the background: (0, 80, 80)."""
    rng = np.random.default_rng(114)
    chunk, ndb = CHUNK_MAX, (1 << ROW_BITS) + 192
    B = rng.integers(0, 256, 32, dtype=np.uint8)
    q = np.stack([flipped(B, range(80 * i, 80 * i + 80)) for i in range(3)])
    db = np.tile(B, (ndb, 1))
    db[chunk - 1] = flipped(q[0], range(240, 250))
    db[chunk] = flipped(q[0], range(245, 255))
    db[ndb - 1] = flipped(q[1], range(240, 247))
    expect = {0: (chunk - 1, 10, 10), 1: (ndb - 1, 7, 80), 2: (0, 80, 80)}
    near = {0: [(chunk - 1, 10), (chunk, 10)], 1: [(ndb - 1, 7)]}
    return Case("row_limit", q, db, chunk, expect, ["row_field_limit"], near=near,
                device_only=True, variants=("row_22_bits",))


def _idx_base_cases():
    """idx_base = 2^31 - 2 - ndb, the largest the entry point takes: the last row's index is
    2^31 - 3, exact in int32."""
    ndb = 300
    b = Builder("idx_base_max", ndb, 256, 115)
    b.query([(ndb - 1, 5), (4, 9)])
    b.query([(0, 6), (ndb - 2, 6)])
    first = b.case(["idx_base_max"], idx_base=INT_MAX - 1 - ndb)
    # Every row is the complement of query 1, which therefore has no row below 256 and reports
    # -1, NOT idx_base - 1; query 0 = query 1 with 246 bits flipped is 10 from every row.
    rng = np.random.default_rng(116)
    q1 = rng.integers(0, 256, 32, dtype=np.uint8)
    q = np.stack([flipped(q1, range(246)), q1])
    second = Case("idx_base_none", q, np.tile(~q1, (ndb, 1)), 256,
                  {0: (0, 10, 10), 1: (-1, 256, 256)}, ["none_not_offset"],
                  idx_base=INT_MAX - 1 - ndb)
    return [first, second]


_CASES = None


def cases():
    """Every case, built once and shared (nothing may modify a case's arrays)."""
    global _CASES
    if _CASES is None:
        cs = [_bit_pairing(), _sweep()] + _tie_cases()
        cs += [_partial_end(n) for n in PARTIAL_ENDS] + [_empty()]
        cs += _extreme_cases() + _multi_block_cases()
        cs += [_query_geometry(n) for n in NQ_SWEEP]
        cs += [_merge_case(n) for n in MERGE_NCHUNKS]
        cs += [_row_limit()] + _idx_base_cases()
        assert len({c.name for c in cs}) == len(cs)
        for c in cs:
            c.q.setflags(write=False)
            c.db.setflags(write=False)
        _CASES = cs
    return _CASES


# ---- structural model -----------------------------------------------------------------------

def _least2_unique(cmp, key, none_cmp, none_key):
    """The two least of {none, none} ∪ keys along the last axis, ordered by cmp (16-bit values,
    distinct within a block by construction), returned as keys.  [..., n] -> [..., 2]."""
    x = (cmp.astype(np.int64) << 16) | key.astype(np.int64)
    nn = np.full(x.shape[:-1] + (2,), (int(none_cmp) << 16) | int(none_key), np.int64)
    x = np.concatenate([nn, x], axis=-1)
    return np.partition(x, 1, axis=-1)[..., :2] & 0xFFFF


def _least2_ordered(cmp, key, none):
    """The two least of {none, none} ∪ keys along the last axis by cmp; equal cmp: the one
    inserted first (nones first, then left to right) stays ahead, as a strict compare keeps
    it.  Returns keys [..., 2]."""
    nn = np.full(cmp.shape[:-1] + (2,), none, np.int64)
    cmp = np.concatenate([nn, cmp], axis=-1)
    key = np.concatenate([nn, key], axis=-1)
    o = np.argsort(cmp, axis=-1, kind="stable")[..., :2]
    return np.take_along_axis(key, o, axis=-1)


def _k16(d, m, variant):
    """16-bit (distance << 7 | m) keys and the value they are compared by."""
    key = (d << 7) + m
    cmp = (d << 7) + (127 - m) if variant == "later_row_wins_in_block" else key
    return key, _cmp16(cmp, variant)


def _cmp16(x, variant):
    return x ^ 0x8000 if variant == "signed_min_max" else x


def _valu_chunk(D, variant, shift, none32):
    """k_bf_top2 on one chunk's distances D [nq, n]: (b1, b2) 32-bit keys."""
    nq, n = D.shape
    nb = n // BLK
    cmps, keys = [], []
    if nb:
        # [nq, block, half (even / odd rows), pair]
        Dk = D[:, :nb * BLK].reshape(nq, nb, 128, 2).transpose(0, 1, 3, 2)
        key16, cmp16 = _k16(Dk, np.arange(128), variant)
        h_none = 0xFFFF if variant == "dist256_becomes_best" else 256 << 7
        h = _least2_unique(cmp16, key16, _cmp16(h_none, variant), h_none)   # [nq, nb, 2, 2]
        e0 = (np.arange(nb) * BLK)[None, :, None, None]
        odd = np.arange(2)[None, None, :, None]
        pair_row = e0 + 2 * (h & 127)
        full = ((h >> 7) << shift) | (pair_row + odd)
        if variant == "dist256_becomes_best":
            full = np.where(h == 0xFFFF, none32, full)
        cmp = full
        if variant == "odd_half_first":
            # the halves' keys meet as (distance, pair): the odd half goes in first and a
            # strict compare then keeps it ahead of the even row of the same pair
            cmp = ((h >> 7) << shift) | pair_row
            full, cmp = full[:, :, ::-1], cmp[:, :, ::-1]
        if variant == "fold_drops_seconds":
            full, cmp = full[..., :1], cmp[..., :1]
        keys.append(full.reshape(nq, -1))
        cmps.append(cmp.reshape(nq, -1))
    e = np.arange(nb * BLK, n)
    tail = (D[:, nb * BLK:] << shift) | e
    keys.append(tail)
    cmps.append(tail)
    b = _least2_ordered(np.concatenate(cmps, axis=1), np.concatenate(keys, axis=1), none32)
    return b[:, 0], b[:, 1]


def _mfma_chunk(D, variant, shift, none32):
    """k_bf_mfma on one chunk's distances D [nq, n]: (b1, b2) 32-bit keys."""
    nq, n = D.shape
    nblk = -(-n // 32)
    nsb = -(-nblk // 4)
    # rows past n of the last block are re-reads of row n - 1 (fetch clamps), masked to 0xFFFF
    # there; whole blocks past nblk never run
    Dp = np.concatenate([D, np.repeat(D[:, n - 1:n], nsb * 128 - n, axis=1)], axis=1)
    row = np.arange(nsb * 128)
    ok = row < (nblk * 32 if variant == "mfma_tail_unmasked" else n)
    m = row % 128
    key16, cmp16 = _k16(Dp, m, variant)
    key16 = np.where(ok, key16, 0xFFFF)
    cmp16 = np.where(ok, cmp16, _cmp16(0xFFFF, variant))
    esb = np.arange(nsb) * 128
    if variant == "mfma_fold_e0":
        esb = np.minimum(esb + 96, (nblk - 1) * 32)       # e0 of the superblock's last block
    halves = []
    for hw in range(2):                                    # accumulator rows with bit 2 == hw
        sel = ((m >> 2) & 1) == hw
        k = key16[:, sel].reshape(nq, nsb, 64)
        c = cmp16[:, sel].reshape(nq, nsb, 64)
        l = _least2_unique(c, k, _cmp16(0xFFFF, variant), 0xFFFF)          # [nq, nsb, 2]
        o = np.where(l == 0xFFFF, 0xFFFFFFFF, ((l >> 7) << shift) + esb[None, :, None] + (l & 127))
        if variant == "fold_drops_seconds":
            o = o[..., :1]
        o = o.reshape(nq, -1)
        halves.append(_least2_ordered(o, o, none32))
    if variant == "mfma_no_halfwave_fold":
        b = halves[0]
    else:
        both = np.concatenate(halves, axis=1)
        b = _least2_ordered(both, both, none32)
    return b[:, 0], b[:, 1]


def _merge(P1, P2, chunk, variant, shift, none32, idx_base):
    """k_bf_merge: P1, P2 [nchunks, nq] 32-bit keys -> (best_idx, best_dist, second_dist)."""
    nchunks, nq = P1.shape
    L = nchunks // 8 if variant == "merge_slice_floor" else -(-nchunks // 8)
    mask = (1 << shift) - 1

    def fold(st, e1, e2, erow):
        d1, d2, row = st
        d2 = np.minimum(np.maximum(d1, e1), np.minimum(d2, e2))
        take = e1 <= d1 if variant == "merge_le" else e1 < d1
        if variant == "dist256_becomes_best":
            take = take | ((row < 0) & (e1 <= 256))
        return np.where(take, e1, d1), d2, np.where(take, erow, row)

    def fresh():
        return (np.full(nq, 256, np.int64), np.full(nq, 256, np.int64), np.full(nq, -1, np.int64))

    slices = []
    for s in range(8):
        c0 = s * L
        c1 = min(nchunks, c0 + L)
        st = fresh()
        for cb in range(c0, c1, 8):
            for j in range(8):
                c = min(cb + j, c1 - 1)
                k1, k2 = P1[c], P2[c]
                if cb + j >= c1 and variant != "merge_batch_unmasked":
                    k1 = k2 = np.full(nq, none32, np.int64)
                st = fold(st, k1 >> shift, k2 >> shift, (cb + j) * chunk + (k1 & mask))
        slices.append(st)
    st = slices[0]
    for t in range(1, 8):
        st = fold(st, *slices[t])
    d1, d2, row = st
    if variant == "base_added_to_none":
        idx = idx_base + row
    else:
        idx = np.where(row < 0, -1, idx_base + row)
    return (idx.astype(np.int32), np.minimum(d1, 256).astype(np.int32),
            np.minimum(d2, 256).astype(np.int32))


def model_top2(q, db, chunk, kernel, variant=None, idx_base=0, d=None):
    """The kernels' decomposition on the distance matrix (d, else computed from q and db)."""
    assert variant is None or variant in VARIANTS
    D = (distances(q, db) if d is None else d).astype(np.int64)
    nq, ndb = D.shape
    if variant == "bx_ignored":
        D = D[np.arange(nq) % (MFMA_Q if kernel == MFMA else 256)]
    shift = 22 if variant == "row_22_bits" else ROW_BITS
    none32 = 0xFFFFFFFF if variant == "dist256_becomes_best" else 256 << shift
    nchunks = -(-ndb // chunk)
    P1 = np.empty((nchunks, nq), np.int64)
    P2 = np.empty((nchunks, nq), np.int64)
    one = _mfma_chunk if kernel == MFMA else _valu_chunk
    for c in range(nchunks):
        P1[c], P2[c] = one(D[:, c * chunk:(c + 1) * chunk], variant, shift, none32)
    return _merge(P1, P2, chunk, variant, shift, none32, idx_base)
