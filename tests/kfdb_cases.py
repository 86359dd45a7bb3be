"""Directed KeyFrameDatabase cases (numpy only): the pure-Python restatement of
src/KeyFrameDatabase.cc with a per-slot record of every query, and scripts that plant each
decision edge of the two detectors and each launch regime of csrc/orbx_kfdb.hip on purpose.

A case is a script of steps that runs identically on the restatement, the C++ oracle and the
GPU database:

    ("add", bow)  ("cov", slot, neighbours)  ("erase", slot)  ("clear",)
    ("reloc", bow)  ("loop", bow, connected, min_score)

and carries the names of the constructs it plants (CONSTRUCTS is the census the CPU test
requires).  Scores are planted exactly: query words weigh 1.0, a keyframe word weighs a
float32 value v in (2^-29, 1], so its term is |1 - v| - 1 - v = -2v without rounding; a word of
weight 0 counts as shared and adds nothing.  A one-word keyframe therefore scores exactly v.

The invariant: at every query, every covisible slot is < len(db) (the oracle and the
reference index keyframes unchecked).  `Script` asserts it.

The record of a query (PyKeyFrameDatabase.last), per slot:
    common  shared words by set intersection, for every alive slot, connected ones included
            (a scan of the database does not know about exclusion); 0 for erased slots
    score   float32 L1 score of every alive slot (-0.0 without a shared word, and for erased)
    first   query position of the smallest shared word, INT_MAX without one
    acc / best   accScore and pBestKF of the slots in lScoreAndMatch, -1 elsewhere
    state   the carried mRelocScore
    selected     lKFsSharingWords was not empty (acc / best belong to this query)

Float32 edges that exist and are planted: 0.75f * 0.8132702112197876f rounds up to
0.6099526882171631f, so a slot accumulating exactly that value is dropped although the double
product is smaller.  An edge that does not exist: for no maxCommonWords <= 8192 does
int(mx * 0.8f) in float32 differ from int(mx * 0.8) in double (checked exhaustively by
test_kfdb_directed.test_filter_float_remark), so no case pretends to separate them.  Likewise
`bestAccScore = minScore` cannot be told from `bestAccScore = 0`: L1 terms are <= 0, so scores
and accumulated scores are >= 0 and every listed slot accumulates at least its own score
>= minScore; the cases plant the equality (every accumulated score == minScore) only.
"""
import numpy as np

F32 = np.float32
INT_MAX = 2**31 - 1

VARIANTS = (
    "common_ge",          # common >= minC instead of common > minC
    "minscore_gt",        # si > minScore instead of si >= minScore
    "thr_double",         # 0.75 * best taken in double
    "acc_double",         # accScore accumulated in double
    "acc_ge",             # acc >= thr instead of acc > thr
    "best_ge",            # bestScore updated on >=
    "slot_order",         # output in slot order instead of (first shared query word, slot)
    "dedup_last",         # de-duplication keeping the last occurrence
    "loop_nb_no_excl",    # loop neighbours not checked for exclusion
    "loop_nb_no_minc",    # loop neighbours not checked for > minC
    "reloc_nb_current",   # reloc neighbours below the filter read the current score
    "state_not_carried",  # stored score never carried
    "k_unbounded",        # more than K neighbours used
    "erased_counted",     # erased neighbours counted
    "score_f32",          # score summed in float32
    "score_desc",         # score summed in descending word order
)


class PyKeyFrameDatabase:
    """Pure-Python restatement (test-only), statement by statement with the reference.
    `variant` (test-only) flips exactly one decision, see VARIANTS."""

    def __init__(self, covisibles=10, variant=None, record=False):
        assert variant is None or variant in VARIANTS, variant
        self.K = covisibles
        self.record = record or variant is not None   # the per-slot record costs a full scan
        self.variant = variant
        self.kfs = []            # dicts: words, values, ordered, state fields
        self.inv = {}            # word -> list of slots in add order
        self.qid = 1
        self.last = None

    def __len__(self):
        return len(self.kfs)

    def add(self, bow):
        w, v = bow
        s = len(self.kfs)
        self.kfs.append(dict(w=[int(x) for x in w], v=[float(x) for x in v], ordered=[],
                             lq=0, lw=0, ls=F32(0), rq=0, rw=0, rs=F32(0), erased=False))
        for x in w:
            self.inv.setdefault(int(x), []).append(s)
        return s

    def erase(self, s):
        self.kfs[s]["erased"] = True
        for x in self.kfs[s]["w"]:
            lst = self.inv[x]
            if s in lst:
                lst.remove(s)

    def clear(self):
        self.kfs, self.inv = [], {}

    def set_covisibles(self, s, nb):
        self.kfs[s]["ordered"] = [int(x) for x in nb]

    def _score(self, qw, qv, k):
        # L1Scoring::score (ScoringObject.cpp:23-67): merged walk in ascending word order
        pos = {w: i for i, w in enumerate(k["w"])}
        pairs = list(zip(qw, qv))
        if self.variant == "score_desc":
            pairs.reverse()
        acc = F32(0) if self.variant == "score_f32" else 0.0
        for w, vi in pairs:
            j = pos.get(int(w))
            if j is not None:
                wi = k["v"][j]
                t = abs(vi - wi) - abs(vi) - abs(wi)
                acc = F32(acc + F32(t)) if self.variant == "score_f32" else acc + t
        return F32(-float(acc) / 2.0)

    # ---- the record ----------------------------------------------------------------------
    def _scan(self, qw, qv):
        """common / score / first of every slot by set intersection; erased slots are counted
        in the *_raw copies only (what the `erased_counted` variant reads)."""
        if not self.record:
            return None
        n = len(self.kfs)
        qpos = {w: i for i, w in enumerate(qw)}
        common, first = np.zeros(n, np.int32), np.full(n, INT_MAX, np.int32)
        score = np.full(n, -0.0, np.float32)
        raw_common, raw_score = common.copy(), score.copy()
        for s, k in enumerate(self.kfs):
            shared = [w for w in k["w"] if w in qpos]
            raw_common[s] = len(shared)
            raw_score[s] = self._score(qw, qv, k)
            if not k["erased"]:
                common[s], score[s] = raw_common[s], raw_score[s]
                if shared:
                    first[s] = qpos[min(shared)]
        return common, score, first, raw_common, raw_score

    def _record(self, loop, conn, scan, accl_slots, accl, selected):
        if scan is None:
            return
        n = len(self.kfs)
        acc, best = np.full(n, -1.0, np.float32), np.full(n, -1, np.int32)
        for s, (a, bk) in zip(accl_slots, accl):
            acc[s], best[s] = a, bk
        self.last = dict(loop=loop, connected=set(conn), common=scan[0], score=scan[1],
                         first=scan[2], acc=acc, best=best, selected=selected,
                         state=np.array([k["rs"] for k in self.kfs], np.float32))

    def _retain(self, scored_slots, accl, best_acc):
        """minScoreToRetain, the retained list in lKFsSharingWords order, de-duplication."""
        v = self.variant
        thr = 0.75 * float(best_acc) if v == "thr_double" else F32(F32(0.75) * best_acc)
        order = range(len(accl))
        if v == "slot_order":
            order = sorted(order, key=lambda i: scored_slots[i])
        kept = [accl[i][1] for i in order
                if (float(accl[i][0]) >= thr if v == "acc_ge" else float(accl[i][0]) > thr)]
        if v == "dedup_last":
            return [bk for i, bk in enumerate(kept) if bk not in kept[i + 1:]]
        out, seen = [], set()
        for bk in kept:
            if bk not in seen:
                out.append(bk)
                seen.add(bk)
        return out

    def _accumulate(self, sc, s, value_of):
        """bestScore / accScore / pBestKF of listed slot s over its covisibles; value_of(n)
        is the neighbour's contribution or None if it is skipped."""
        v = self.variant
        best, acc, bk = sc, (float(sc) if v == "acc_double" else sc), s
        nbs = self.kfs[s]["ordered"]
        for n in (nbs if v == "k_unbounded" else nbs[:self.K]):
            x = value_of(n)
            if x is None:
                continue
            acc = acc + float(x) if v == "acc_double" else F32(acc + x)
            if (x >= best) if v == "best_ge" else (x > best):
                bk, best = n, x
        return F32(acc), bk

    def DetectRelocalizationCandidates(self, bow):
        qw, qv = [int(x) for x in bow[0]], [float(x) for x in bow[1]]
        v = self.variant
        qid, self.qid = self.qid, self.qid + 1
        scan = self._scan(qw, qv)
        if v == "state_not_carried":
            for k in self.kfs:
                k["rs"] = F32(0)
        sharing = []
        for w in qw:
            for s in self.inv.get(w, []):
                k = self.kfs[s]
                if k["rq"] != qid:
                    k["rw"] = 0
                    k["rq"] = qid
                    sharing.append(s)
                k["rw"] += 1
        if not sharing:
            self._record(False, (), scan, [], [], False)
            return []
        mx = max(self.kfs[s]["rw"] for s in sharing)
        minc = int(F32(mx) * F32(0.8))
        scored = []
        for s in sharing:
            k = self.kfs[s]
            if (k["rw"] >= minc) if v == "common_ge" else (k["rw"] > minc):
                k["rs"] = self._score(qw, qv, k)
                scored.append((k["rs"], s))

        def value_of(n):
            k2 = self.kfs[n]
            if k2["rq"] != qid:
                if v == "erased_counted" and k2["erased"] and scan[3][n] > 0:
                    return scan[4][n] if scan[3][n] > minc else k2["rs"]
                return None
            if v == "reloc_nb_current" and k2["rw"] <= minc:
                return scan[1][n]
            return k2["rs"]

        accl, best_acc = [], F32(0)
        for sc, s in scored:
            acc, bk = self._accumulate(sc, s, value_of)
            accl.append((acc, bk))
            if acc > best_acc:
                best_acc = acc
        slots = [s for _, s in scored]
        self._record(False, (), scan, slots, accl, True)
        if not scored:
            return []
        return self._retain(slots, accl, best_acc)

    def DetectLoopCandidates(self, bow, connected, min_score):
        qw, qv = [int(x) for x in bow[0]], [float(x) for x in bow[1]]
        conn = set(int(x) for x in connected)
        min_score = F32(min_score)
        v = self.variant
        qid, self.qid = self.qid, self.qid + 1
        scan = self._scan(qw, qv)
        sharing = []
        for w in qw:
            for s in self.inv.get(w, []):
                k = self.kfs[s]
                if k["lq"] != qid:
                    k["lw"] = 0
                    if s not in conn:
                        k["lq"] = qid
                        sharing.append(s)
                k["lw"] += 1
        if not sharing:
            self._record(True, conn, scan, [], [], False)
            return []
        mx = max(self.kfs[s]["lw"] for s in sharing)
        minc = int(F32(mx) * F32(0.8))
        scored = []
        for s in sharing:
            k = self.kfs[s]
            if (k["lw"] >= minc) if v == "common_ge" else (k["lw"] > minc):
                k["ls"] = self._score(qw, qv, k)
                if (k["ls"] > min_score) if v == "minscore_gt" else (k["ls"] >= min_score):
                    scored.append((k["ls"], s))

        def value_of(n):
            k2 = self.kfs[n]
            if v == "loop_nb_no_excl":
                return scan[1][n] if scan[0][n] > minc else None
            if v == "loop_nb_no_minc":
                return scan[1][n] if k2["lq"] == qid else None
            if v == "erased_counted" and k2["erased"] and n not in conn and scan[3][n] > minc:
                return scan[4][n]
            if k2["lq"] == qid and k2["lw"] > minc:
                return k2["ls"]
            return None

        accl, best_acc = [], min_score
        for sc, s in scored:
            acc, bk = self._accumulate(sc, s, value_of)
            accl.append((acc, bk))
            if acc > best_acc:
                best_acc = acc
        slots = [s for _, s in scored]
        self._record(True, conn, scan, slots, accl, True)
        if not scored:
            return []
        return self._retain(slots, accl, best_acc)


# ---- running a case on any database ------------------------------------------------------------
def run_case(db, case, read=None):
    """Runs the script on `db`; returns one (candidates, read(db)) pair per query."""
    out = []
    for st in case["steps"]:
        op = st[0]
        if op == "add":
            db.add(st[1])
        elif op == "cov":
            db.set_covisibles(st[1], st[2])
        elif op == "erase":
            db.erase(st[1])
        elif op == "clear":
            db.clear()
        elif op == "reloc":
            c = [int(x) for x in db.DetectRelocalizationCandidates(st[1])]
            out.append((c, read(db) if read else None))
        elif op == "loop":
            c = [int(x) for x in db.DetectLoopCandidates(st[1], st[2], st[3])]
            out.append((c, read(db) if read else None))
        else:
            raise ValueError(op)
    return out


def read_py(db):
    r = db.last
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in r.items()}


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def assert_oracle_record(py, o, where=""):
    """The oracle's read-back (OracleKeyFrameDatabase.debug_read) against the restatement's
    record.  The oracle knows words / first only of the keyframes it listed; a connected
    keyframe's counter is reset at every word there."""
    n = len(py["common"])
    conn = np.array([s in py["connected"] for s in range(n)], bool)
    listed = (py["common"] > 0) & ~conn
    assert o["loop"] == py["loop"] and o["selected"] == py["selected"], where
    np.testing.assert_array_equal(o["listed"][:n].astype(bool), listed, where)
    np.testing.assert_array_equal(o["words"][:n][listed], py["common"][listed], where)
    np.testing.assert_array_equal(o["first"][:n][listed], py["first"][listed], where)
    assert np.all(o["first"][:n][~listed] == INT_MAX), where
    np.testing.assert_array_equal(bits(o["score"][:n]), bits(py["score"]), where)
    np.testing.assert_array_equal(bits(o["reloc_score"][:n]), bits(py["state"]), where)
    scored = py["best"] >= 0   # in lScoreAndMatch: mRelocScore / mLoopScore is this query's
    np.testing.assert_array_equal(bits(o["query_score"][:n][scored]), bits(py["score"][scored]),
                                  where)
    np.testing.assert_array_equal(bits(o["acc"][:n]), bits(py["acc"]), where)
    np.testing.assert_array_equal(o["best"][:n], py["best"], where)


def same_record(a, b):
    """Two restatement records are equal (floats as bits)."""
    if a["selected"] != b["selected"]:
        return False
    for k in ("common", "first", "best"):
        if not np.array_equal(a[k], b[k]):
            return False
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in ("score", "acc", "state"))


# ---- building cases ----------------------------------------------------------------------------
def bow(words, vals):
    w = np.asarray(words, np.uint32)
    v = np.asarray(vals, np.float64)
    assert len(w) == len(v) and np.all(np.diff(w.astype(np.int64)) > 0)
    return w, v


def query(words):
    """A query BowVector: every word weighs 1.0."""
    words = list(words)
    return bow(words, [1.0] * len(words))


def kf(words, score, at=0):
    """A keyframe sharing `words`: the word at index `at` weighs `score` (a float32 value),
    the others 0, so its score against a `query` holding all its words is exactly `score`."""
    words = list(words)
    s = float(F32(score))
    assert s == float(score) and (s == 0.0 or 2.0**-29 < s <= 1.0)
    v = [0.0] * len(words)
    if words:
        v[at] = s
    return bow(words, v)


class Script:
    """Collects the steps of a case and asserts the invariant at every query."""

    def __init__(self, name, constructs, K=10, expect=None):
        self.name, self.constructs, self.K, self.expect = name, tuple(constructs), K, expect
        self.steps, self.n, self.cov = [], 0, {}

    def add(self, *bows):
        for b in bows:
            self.steps.append(("add", b))
            self.n += 1
        return self

    def cov_(self, s, nb):
        assert 0 <= s < self.n and all(x >= 0 for x in nb)
        self.steps.append(("cov", s, [int(x) for x in nb]))
        self.cov[s] = list(nb)
        return self

    def erase(self, s):
        assert 0 <= s < self.n
        self.steps.append(("erase", s))
        return self

    def clear(self):
        self.steps.append(("clear",))
        self.n, self.cov = 0, {}
        return self

    def _invariant(self):
        for s, nb in self.cov.items():
            assert all(x < self.n for x in nb), (self.name, s, nb, self.n)

    def reloc(self, q):
        self._invariant()
        self.steps.append(("reloc", q))
        return self

    def loop(self, q, connected, min_score):
        self._invariant()
        self.steps.append(("loop", q, [int(x) for x in connected], float(F32(min_score))))
        return self

    def done(self):
        nq = sum(1 for s in self.steps if s[0] in ("reloc", "loop"))
        assert self.expect is None or len(self.expect) == nq, self.name
        return dict(name=self.name, constructs=self.constructs, K=self.K, steps=self.steps,
                    expect=self.expect)


CONSTRUCTS = (
    "filter_mx1", "filter_mx4", "filter_mx5", "filter_mx6", "filter_mx10", "filter_loop",
    "min_score_equal_in", "min_score_below_out", "best_acc_starts_at_min_score",
    "retain_thr_rounds_up", "retain_one_above", "all_scores_zero",
    "acc_float32",
    "best_tie_keeps_self", "neighbour_is_self", "neighbour_twice",
    "order_first_word", "order_equal_first_slot",
    "dedup_first_wins",
    "excl_highest_common", "excl_neighbour_adds_nothing", "excl_unsorted_dups", "excl_all",
    "excl_beyond_db",
    "loop_nb_below_minc", "reloc_nb_stored", "state_zero_initially", "state_query_before_last",
    "state_zero_after_clear", "state_survives_growth",
    "row_exactly_K1", "row_exactly_K10", "row_exactly_K64", "row_over_K1", "row_over_K10",
    "row_over_K64", "erased_neighbour", "erased_best", "row_shortened", "stale_row_clear",
    "stale_row_late_add",
    "scan_sizes", "scan_first_chunk2", "scan_first_chunk3", "scan_lane0", "scan_lane63",
    "scan_order_dependent_sum", "scan_float32_sum", "slots_1", "slots_3", "slots_4", "slots_5",
    "slots_1023", "slots_1024", "slots_1025", "erased_between", "erase_after_upload",
)

Q5 = query(range(10, 15))
Q10 = query(range(10, 20))
Q1 = query([10])


def _filter_cases():
    out = []
    for mx, minc in ((1, 0), (4, 3), (5, 4), (6, 4), (10, 8)):
        assert int(F32(mx) * F32(0.8)) == minc
        q = query(range(10, 10 + mx))
        s = Script(f"filter_mx{mx}", [f"filter_mx{mx}"], expect=[[0, 2]])
        # slot 1 shares exactly minC words (none for mx = 1): out; slot 2 shares minC + 1: in
        s.add(kf(range(10, 10 + mx), 0.5),
              kf(list(range(10, 10 + minc)) or [900], 0.5),
              kf(range(10, 10 + minc + 1), 0.5))
        out.append(s.reloc(q).done())
    s = Script("filter_loop", ["filter_loop"], expect=[[0, 2]])
    s.add(kf(range(10, 16), 0.5), kf(range(10, 14), 0.5), kf(range(10, 15), 0.5))
    out.append(s.loop(query(range(10, 16)), [], 0.25).done())
    return out


def _min_score_cases():
    m = F32(0.3)
    below = np.nextafter(m, F32(0))
    s = Script("min_score", ["min_score_equal_in", "min_score_below_out",
                             "best_acc_starts_at_min_score"], expect=[[0], []])
    s.add(kf([10], m), kf([10], below))
    s.loop(Q1, [], m)
    # above every score: lScoreAndMatch empty
    s.loop(Q1, [], np.nextafter(m, F32(1)))
    return [s.done()]


def _retention_cases():
    best = F32(0.8132702112197876)
    thr = F32(F32(0.75) * best)
    assert float(thr) == 0.6099526882171631 and float(thr) > 0.75 * float(best)
    s = Script("retain_float32", ["retain_thr_rounds_up", "retain_one_above"], expect=[[0, 2]])
    s.add(kf([10], best), kf([10], thr), kf([10], np.nextafter(thr, F32(1))))
    z = Script("all_scores_zero", ["all_scores_zero"], expect=[[], []])
    z.add(kf([10], 0.0), kf([10], 0.0), kf([10], 0.0))
    z.reloc(Q1).loop(Q1, [], 0.0)
    return [s.reloc(Q1).done(), z.done()]


def _accumulation_cases():
    e = 2.0**-25
    assert F32(F32(F32(0.5) + F32(e)) + F32(e)) == F32(0.5) and F32(0.5 + e + e) != F32(0.5)
    s = Script("acc_float32", ["acc_float32"], expect=[[0], [0]])
    s.add(kf([10], 0.5), kf([10], e), kf([10], e)).cov_(0, [1, 2])
    # slots 1 and 2 accumulate 2^-25 + 0.5 = 0.5 with best 0: three entries, one candidate
    s.cov_(1, [0]).cov_(2, [0])
    s.reloc(Q1).loop(Q1, [], 0.0)
    t = Script("best_ties", ["best_tie_keeps_self", "neighbour_is_self", "neighbour_twice"],
               expect=[[0, 1, 3], [0, 1, 3]])
    # 0: neighbour 1 ties -> best stays 0.  1: its own neighbour -> acc 1.0, best 1.
    # 2: neighbour 3 twice -> acc 0.25 + 2 * 0.375 = 1.0, best 3
    t.add(kf([10], 0.5), kf([10], 0.5), kf([10], 0.25), kf([10], 0.375))
    t.cov_(0, [1]).cov_(1, [1]).cov_(2, [3, 3])
    t.reloc(Q1).loop(Q1, [], 0.0)
    return [s.done(), t.done()]


def _order_cases():
    s = Script("list_order", ["order_first_word", "order_equal_first_slot"],
               expect=[[1, 2, 0], [1, 2, 0]])
    s.add(kf(range(11, 15), 0.5), kf(range(10, 14), 0.5), kf(range(10, 14), 0.5))
    s.reloc(Q5).loop(Q5, [], 0.0)
    # list order 0 .. 3 (word 11), then 4, 5 (word 12): 4 and 5 (0.5 each) miss
    # 0.75 * 0.75, the four 0.25-slots carry them as best 4, 5, 4, 4: three entries name 4,
    # four are retained, two survive
    d = Script("dedup", ["dedup_first_wins"], expect=[[4, 5], [4, 5]])
    d.add(*[kf([11], 0.25)] * 4, kf([12], 0.5), kf([12], 0.5))
    d.cov_(0, [4]).cov_(1, [5]).cov_(2, [4]).cov_(3, [4])
    q = query([11, 12])
    d.reloc(q).loop(q, [], 0.0)
    return [s.done(), d.done()]


def _exclusion_cases():
    s = Script("loop_exclusion", ["excl_highest_common", "excl_neighbour_adds_nothing",
                                  "excl_unsorted_dups", "excl_all", "excl_beyond_db"],
               expect=[[1], [1], [], [0]])
    s.add(kf(range(10, 20), 0.5), kf(range(10, 15), 0.25), kf(range(10, 14), 0.25))
    s.cov_(1, [0, 2])
    s.loop(Q10, [0], 0.0)                       # mx is 5, not 10; neighbour 0 adds nothing
    s.loop(Q10, [7, 0, 0, 3, 0, 100000], 0.0)   # unsorted, duplicates, slots beyond the db
    s.loop(Q10, [2, 1, 0], 0.0)                 # every slot connected
    # exclusion is per query: without it mx is 10 and only slot 0 passes the filter
    s.loop(Q10, [], 0.0)
    return [s.done()]


def _neighbour_cases():
    out = []
    s = Script("loop_nb_below_minc", ["loop_nb_below_minc"], expect=[[0]])
    s.add(kf(range(10, 15), 0.25), kf(range(10, 14), 0.5)).cov_(0, [1])
    out.append(s.loop(Q5, [], 0.0).done())

    # slot 1 scores 0.25 against word 50 and shares word 14 (weight 0.125) with Q5, below the
    # filter there; slot 2 answers word 60 only.  Slot 0's row names slot 1.
    def base(s):
        s.add(kf(range(10, 15), 0.5), bow([14, 50], [0.125, 0.25]), kf([60], 0.5))
        return s.cov_(0, [1])
    s = base(Script("reloc_nb_stored", ["reloc_nb_stored"], expect=[[1], [0]]))
    out.append(s.reloc(query([50])).reloc(Q5).done())
    s = base(Script("state_zero_initially", ["state_zero_initially"], expect=[[0]]))
    out.append(s.reloc(Q5).done())
    s = base(Script("state_query_before_last", ["state_query_before_last"],
                    expect=[[1], [2], [0]]))
    out.append(s.reloc(query([50])).reloc(query([60])).reloc(Q5).done())
    s = base(Script("state_zero_after_clear", ["state_zero_after_clear"], expect=[[1], [0]]))
    s.reloc(query([50])).clear()
    out.append(base(s).reloc(Q5).done())
    s = base(Script("state_survives_growth", ["state_survives_growth"], expect=[[1], [0]]))
    s.reloc(query([50]))
    s.add(*[kf([70], 0.5)] * 1100)
    out.append(s.reloc(Q5).done())
    return out


def _row_cases():
    out = []
    for K in (1, 10, 64):
        for extra, tag in ((0, "exactly"), (3, "over")):
            s = Script(f"row_{tag}_K{K}", [f"row_{tag}_K{K}"], K=K)
            s.add(kf([10], 0.5), *[kf([10], 1.0 / 64)] * (K + extra))
            s.cov_(0, range(1, 1 + K + extra))
            out.append(s.reloc(Q1).loop(Q1, [], 0.0).done())
    s = Script("erased", ["erased_neighbour", "erased_best"], expect=[[2], [2]])
    # slot 1 would be the best keyframe of slot 0 (1.0); erased, slot 2 (0.75) is
    s.add(kf([10], 0.5), kf([10], 1.0), kf([10], 0.75)).cov_(0, [1, 2]).erase(1)
    out.append(s.reloc(Q1).loop(Q1, [], 0.0).done())
    # slot 0 accumulates 0.5 + 0.25 + 0.375 + 0.125, then 0.5 + 0.375
    s = Script("row_shortened", ["row_shortened"], expect=[[0], [0]])
    s.add(kf([10], 0.5), kf([10], 0.25), kf([10], 0.375), kf([10], 0.125)).cov_(0, [1, 2, 3])
    s.reloc(Q1).cov_(0, [2])
    out.append(s.reloc(Q1).done())

    # the stale-row scripts: a device row that outlives clear()
    a = bow(range(10, 15), [.25, .25, .2, .15, .15])
    b = bow(range(10, 15), [.2] * 5)
    qs = bow(range(10, 15), [.2] * 5)
    s = Script("stale_row_clear", ["stale_row_clear"], expect=[[1], [0, 1]])
    s.add(a, b).cov_(0, [1]).reloc(qs).clear().add(a, b)
    out.append(s.reloc(qs).done())
    s = Script("stale_row_late_add", ["stale_row_late_add"], expect=[[0], [0, 1], [0, 1, 2]])
    # slot 2 accumulates 0.25 + 1.0 before clear(); afterwards its row is empty
    s.add(kf([10], 1.0), kf([10], 0.875), kf([10], 0.8125)).cov_(2, [0]).cov_(1, [0]).cov_(0, [])
    s.reloc(Q1).clear().add(kf([10], 1.0), kf([10], 0.875)).reloc(Q1)
    s.add(kf([10], 0.8125))
    out.append(s.reloc(Q1).done())
    return out


def _scan_cases():
    out = []
    q = query(range(5000, 5200))
    wt = lambda j: (j % 7 + 1) / 1024.0
    s = Script("scan_sizes", ["scan_sizes"])
    for n in (0, 1, 63, 64, 65, 128, 129):
        s.add(bow(range(5000, 5000 + n), [wt(j) for j in range(n)]))
    out.append(s.reloc(q).loop(q, [6], 0.0).done())

    s = Script("scan_chunks", ["scan_first_chunk2", "scan_first_chunk3", "scan_lane0",
                               "scan_lane63"])
    s.add(bow(list(range(64)) + [5003], [0.5] * 65))              # first hit in chunk 2
    s.add(bow(list(range(128)) + [5005, 5006], [0.25] * 130))     # in chunk 3
    s.add(bow([5001] + list(range(6000, 6063)), [0.5] * 64))      # lane 0 only
    s.add(bow(list(range(63)) + [5002], [0.5] * 64))              # lane 63 only
    out.append(s.reloc(q).done())

    # ascending: -(2^53 + 2^29), then 70 times -1 is absorbed (ties to even): the score is the
    # tie 2^52 + 2^28 -> 2^52 in float32.  Any other order keeps part of the 70: rounds up.
    big = 2.0**52 + 2.0**28
    words = list(range(5000, 5071))
    vals = [big] + [0.5] * 70
    acc = 0.0
    for v in vals:
        acc += -2.0 * v
    assert F32(-acc / 2) == F32(2.0**52) and F32(-sum(-2.0 * v for v in vals[::-1]) / 2) != F32(2.0**52)
    s = Script("scan_order_dependent_sum", ["scan_order_dependent_sum"], expect=[[0]])
    s.add(bow(words, vals))
    out.append(s.reloc(bow(words, vals)).done())
    # 1 + 2^-24 + 2^-24 (halved): float32 summation loses both small terms
    s = Script("scan_float32_sum", ["scan_float32_sum"], expect=[[0]])
    s.add(bow([10, 11, 12], [0.5, 2.0**-25, 2.0**-25]))
    out.append(s.reloc(query([10, 11, 12])).done())

    for n in (1, 3, 4, 5, 1023, 1024, 1025):
        s = Script(f"slots_{n}", [f"slots_{n}"])
        s.add(*[kf([10], (i % 4 + 5) / 16.0) for i in range(n)])
        if n > 5:   # rows across the 1024-thread stride: the last slot gathers the first ones
            s.cov_(n - 1, [0, 1, 2, n - 2])
        out.append(s.reloc(Q1).loop(Q1, [n - 1], 0.4375).done())
    s = Script("erased_between", ["erased_between", "erase_after_upload"],
               expect=[[0, 2], [0, 2], [2], [2]])
    s.add(kf([10], 0.5), kf([10], 1.0), kf([10], 0.5)).erase(1)
    s.reloc(Q1).loop(Q1, [], 0.0)
    # erased once the database is on the device: only the alive flags travel
    s.erase(0)
    out.append(s.reloc(Q1).loop(Q1, [], 0.0).done())
    return out


def all_cases():
    cases = (_filter_cases() + _min_score_cases() + _retention_cases() + _accumulation_cases() +
             _order_cases() + _exclusion_cases() + _neighbour_cases() + _row_cases() +
             _scan_cases())
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return cases


CASES = all_cases()
