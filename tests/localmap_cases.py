"""Tracking::UpdateLocalMap (src/Tracking.cc:1288-1442) as orbx_update_local_map* runs it
(include/orbx_localmap.h): a numpy / Python restatement over the CSR snapshot, the directed case
builders, a seeded random generator, single-decision variants, and the binary files of
tests/native/localmap_ref.cpp.

A case is {"name", "S": the snapshot (the arrays of orbx_map_view and its counts), "F": one frame
(feat_mp, nfeat, outlier, cap_kf, cap_mp and the in/out local_kf, n_local_kf, ref_kf)}.
"""
from __future__ import annotations

import numpy as np

MAP_POINT_DTYPE = np.dtype([("pos", "<f4", 3), ("min_dist", "<f4"), ("normal", "<f4", 3),
                            ("max_dist", "<f4")])

KEPT, CAP_KF, CAP_MP, BAD_INDEX = 1, 1 << 8, 1 << 9, 1 << 10
REFUSED_ANY = 7 << 8
MAX_KF, MAX_FEAT = 131072, 32768
MAX_UNITS = 1 << 25
i32 = np.int32

VARIANTS = ["tie_by_slot", "max_ge", "parent_break_inner", "limit_ge_80", "eleven_neighbours",
            "bad_parent_skipped", "extension_over_added", "last_occurrence"]


# ---- the restatement -------------------------------------------------------------------------------

def _row(off, i, n_entries):
    """Row i of a CSR array, or None when its offsets decrease or leave the array."""
    b, e = int(off[i]), int(off[i + 1])
    if b < 0 or e < b or e > n_entries:
        return None
    return b, e


def update_local_map_np(S, F, variant=None):
    """One frame.  Returns {"info", "refused"} and, when not refused, "local_kf", "ref_kf",
    "n_local", "block" (the ids of the frame's block: the locals, then the extras), "skip" (per block
    entry), "mp_of_feat" and "nulled" (mvpMapPoints as ids after :1350).  A refusal stops at the
    checks the kernel stops at: after the setup, the vote, the first list, the extension, the rows'
    offsets, the rows' entries, the block's size."""
    n_kf, n_mp = S["n_kf"], S["n_mp"]
    flags = 0

    def refused(fl):
        return dict(info=fl, refused=True)

    nfeat = int(F["nfeat"])
    if nfeat < 0 or nfeat > len(F["feat_mp"]):
        flags |= BAD_INDEX
        nfeat = 0
    order = [int(r) for r in S["kf_order"]]
    if any(r < 0 or r >= n_kf for r in order) or len(set(order)) != n_kf:
        flags |= BAD_INDEX
    if flags:
        return refused(flags)
    if variant == "tie_by_slot":
        order = list(range(n_kf))
    inv = [0] * n_kf
    for s, r in enumerate(order):
        inv[r] = s
    kf_bad, mp_bad = S["kf_bad"], S["mp_bad"]

    # mvpMapPoints after the outliers are nulled (:955-975) and :1339-1351
    eff = []
    for i in range(nfeat):
        if F["outlier"] is not None and F["outlier"][i]:
            eff.append(-1)
            continue
        m = int(F["feat_mp"][i])
        if m < -1 or m >= n_mp:
            flags |= BAD_INDEX
            eff.append(-1)
            continue
        eff.append(-1 if m >= 0 and mp_bad[m] else m)
    votes = [0] * n_kf          # by rank: the iteration order of keyframeCounter
    voted = False
    for m in eff:
        if m < 0:
            continue
        r = _row(S["mp_obs_off"], m, S["n_obs"])
        if r is None:
            flags |= BAD_INDEX
            continue
        for k in range(*r):
            s = int(S["mp_obs"][k])
            if s < 0 or s >= n_kf:
                flags |= BAD_INDEX
                continue
            votes[order[s]] += 1
            voted = True
    if flags:
        return refused(flags)

    cap_kf, cap_mp = F["cap_kf"], F["cap_mp"]
    ref = int(F["ref_kf"])
    kept = not voted                                     # :1355
    if kept:
        n_in = int(F["n_local_kf"])
        if n_in < 0 or n_in > cap_kf:
            return refused(BAD_INDEX)
        lst = [int(s) for s in F["local_kf"][:n_in]]
        seen = set()
        for s in lst:
            if s < 0 or s >= n_kf or s in seen:
                flags |= BAD_INDEX
            seen.add(s)
        if flags:
            return refused(flags)
    else:
        lst, best = [], 0
        for r in range(n_kf):                            # :1366-1381
            if votes[r] == 0:
                continue
            s = inv[r]
            if kf_bad[s]:
                continue
            if votes[r] > best or (variant == "max_ge" and votes[r] >= best):
                best, ref = votes[r], s
            lst.append(s)
        if len(lst) > cap_kf:
            return refused(CAP_KF)
        listed = set(lst)
        nfirst = len(lst)
        full = False

        def push(s):
            nonlocal flags, full
            if len(lst) >= cap_kf:
                flags |= CAP_KF
                full = True
                return False
            lst.append(s)
            listed.add(s)
            return True

        i = 0
        while i < (len(lst) if variant == "extension_over_added" else nfirst) and not full:
            if len(lst) > 80 or (variant == "limit_ge_80" and len(lst) >= 80):     # :1388
                break
            kf = lst[i]
            i += 1
            r = _row(S["kf_cov_off"], kf, S["n_cov"])
            if r is None:
                flags |= BAD_INDEX
                r = (0, 0)
            take = None
            for k in range(r[0], min(r[1], r[0] + (11 if variant == "eleven_neighbours" else 10))):
                s = int(S["kf_cov"][k])
                if s < 0 or s >= n_kf:
                    flags |= BAD_INDEX
                elif take is None and not kf_bad[s] and s not in listed:
                    take = s
            if take is not None and not push(take):
                break
            r = _row(S["kf_child_off"], kf, S["n_child"])
            if r is None:
                flags |= BAD_INDEX
                r = (0, 0)
            take = None
            for k in range(*r):                          # the whole row is read
                s = int(S["kf_child"][k])
                if s < 0 or s >= n_kf:
                    flags |= BAD_INDEX
                elif take is None and not kf_bad[s] and s not in listed:
                    take = s
            if take is not None and not push(take):
                break
            p = int(S["kf_parent"][kf])
            if p < -1 or p >= n_kf:
                flags |= BAD_INDEX
            elif p >= 0 and p not in listed and not (variant == "bad_parent_skipped" and kf_bad[p]):
                push(p)
                if variant != "parent_break_inner":
                    break                                # :1431
        if flags:
            return refused(flags)

    # UpdateLocalPoints (:1299-1322)
    rows, units = [], (nfeat + 63) // 64
    for s in lst:
        r = _row(S["kf_mp_off"], s, S["n_kfmp"])
        if r is None:
            flags |= BAD_INDEX
            r = (0, 0)
        rows.append(r)
        units += (r[1] - r[0] + 63) // 64
    if units >= MAX_UNITS:
        flags |= BAD_INDEX
    if flags:
        return refused(flags)
    local, where = [], {}
    for r in rows:
        for k in range(*r):
            m = int(S["kf_mp"][k])
            if m < -1 or m >= n_mp:
                flags |= BAD_INDEX
                continue
            if m < 0 or mp_bad[m]:
                continue
            if variant == "last_occurrence":
                if m in where:
                    local.remove(m)
            elif m in where:
                continue
            where[m] = True
            local.append(m)
    if flags:
        return refused(flags)
    where = {m: k for k, m in enumerate(local)}
    n_local = len(local)
    block = list(local)
    for m in eff:                                        # the extras, once per id
        if m >= 0 and m not in where:
            where[m] = len(block)
            block.append(m)
    if len(block) > cap_mp:
        return refused(CAP_MP)
    mp_of_feat = [where[m] if m >= 0 else -1 for m in eff]
    skip = [0] * n_local + [1] * (len(block) - n_local)
    for k in mp_of_feat:
        if 0 <= k < n_local:
            skip[k] = 1                                  # :1261
    return dict(info=KEPT if kept else 0, refused=False, local_kf=lst, ref_kf=ref, n_local=n_local,
                block=block, skip=skip, mp_of_feat=mp_of_feat, nulled=eff)


def result_key(r):
    if r["refused"]:
        return ("refused", r["info"])
    return (r["info"], tuple(r["local_kf"]), r["ref_kf"], r["n_local"], tuple(r["block"]),
            tuple(r["skip"]), tuple(r["mp_of_feat"]))


def apply_result(r, S, F, out, f=0):
    """What the call leaves in `out` -- numpy arrays local_kf [B, cap_kf], n_local_kf [B], ref_kf [B],
    local_mp [B, cap_mp], n_local_mp [B, 2], mps [B, cap_mp], skip [B, cap_mp], mp_of_feat
    [B, feat_stride], info [B] -- for frame f, given what was in them."""
    out["info"][f] = r["info"]
    if r["refused"]:
        return
    if not r["info"] & KEPT:
        n = len(r["local_kf"])
        out["local_kf"][f, :n] = r["local_kf"]
        out["n_local_kf"][f] = n
        out["ref_kf"][f] = r["ref_kf"]
    nb = len(r["block"])
    out["n_local_mp"][f] = (r["n_local"], nb)
    out["local_mp"][f, :nb] = r["block"]
    out["local_mp"][f, nb:] = -1
    out["mps"][f, :nb] = S["mp_rec"][r["block"]] if nb else []
    out["mps"][f, nb:] = np.zeros((), MAP_POINT_DTYPE)
    out["skip"][f, :nb] = r["skip"]
    out["skip"][f, nb:] = 1
    out["mp_of_feat"][f, :len(r["mp_of_feat"])] = r["mp_of_feat"]
    out["mp_of_feat"][f, len(r["mp_of_feat"]):] = -1


# ---- snapshots and cases ------------------------------------------------------------------------------

def _csr(rows):
    off = np.zeros(len(rows) + 1, i32)
    for k, r in enumerate(rows):
        off[k + 1] = off[k] + len(r)
    flat = np.array([x for r in rows for x in r], i32)
    return off, flat


def records(n_mp, seed=0):
    rng = np.random.default_rng(1000 + seed)
    rec = np.zeros(n_mp, MAP_POINT_DTYPE)
    rec["pos"] = rng.uniform(-3, 3, (n_mp, 3)).astype(np.float32)
    rec["pos"][:, 2] += np.float32(6)
    nrm = rng.normal(size=(n_mp, 3))
    rec["normal"] = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    rec["min_dist"] = rng.uniform(0.5, 2, n_mp).astype(np.float32)
    rec["max_dist"] = rec["min_dist"] * np.float32(12)
    return rec


def snapshot(n_kf, kf_mp, *, n_mp=None, order=None, bad_kf=(), parent=None, cov=None, children=None,
             bad_mp=(), obs=None, temporal=(), rec=None):
    """kf_mp: per keyframe the MapPoint id (or -1) of each feature.  Defaults: the identity order,
    no parents, no neighbours, children derived from the parents, observations derived from kf_mp
    (`temporal` ids get an empty row; `obs` {id: slots} overrides rows)."""
    kf_mp = [list(r) for r in kf_mp]
    assert len(kf_mp) == n_kf
    if n_mp is None:
        n_mp = max([m for r in kf_mp for m in r] + [-1]) + 1
    order = list(range(n_kf)) if order is None else list(order)
    parent = [-1] * n_kf if parent is None else list(parent)
    cov = [[] for _ in range(n_kf)] if cov is None else [list(r) for r in cov]
    if children is None:
        children = [[c for c in range(n_kf) if parent[c] == k] for k in range(n_kf)]
    # std::set<KeyFrame*> iterates by pointer: ascending kf_order
    children = [sorted(r, key=lambda c: order[c]) for r in children]
    rows = [[] for _ in range(n_mp)]
    for k, r in enumerate(kf_mp):
        for m in r:
            if m >= 0 and k not in rows[m]:
                rows[m].append(k)
    for m in temporal:
        rows[m] = []
    for m, r in (obs or {}).items():
        rows[m] = list(r)
    S = dict(n_kf=n_kf, n_mp=n_mp, kf_order=np.array(order, i32),
             kf_bad=np.array([k in set(bad_kf) for k in range(n_kf)], np.uint8),
             kf_parent=np.array(parent, i32),
             mp_bad=np.array([m in set(bad_mp) for m in range(n_mp)], np.uint8),
             mp_rec=records(n_mp) if rec is None else rec)
    S["kf_cov_off"], S["kf_cov"] = _csr(cov)
    S["kf_child_off"], S["kf_child"] = _csr(children)
    S["kf_mp_off"], S["kf_mp"] = _csr(kf_mp)
    S["mp_obs_off"], S["mp_obs"] = _csr(rows)
    for n, a in (("n_cov", "kf_cov"), ("n_child", "kf_child"), ("n_kfmp", "kf_mp"),
                 ("n_obs", "mp_obs")):
        S[n] = len(S[a])
    return S


def frame(S, feat_mp, *, outlier=None, cap_kf=None, cap_mp=None, local_in=(), ref_in=-1, stride=None,
          nfeat=None):
    feat = np.array(list(feat_mp), i32)
    n = len(feat) if nfeat is None else nfeat
    stride = max(len(feat), 1) if stride is None else stride
    fm = np.full(stride, -1, i32)
    fm[:len(feat)] = feat
    ol = None
    if outlier is not None:
        ol = np.zeros(stride, np.uint8)
        ol[:len(outlier)] = outlier
    cap_kf = max(S["n_kf"], len(local_in), 1) if cap_kf is None else cap_kf
    cap_mp = max(S["n_mp"], 1) if cap_mp is None else cap_mp
    lk = np.full(max(cap_kf, len(local_in)), -7, i32)
    lk[:len(local_in)] = list(local_in)
    return dict(feat_mp=fm, nfeat=n, outlier=ol, cap_kf=cap_kf, cap_mp=cap_mp, local_kf=lk,
                n_local_kf=len(local_in), ref_kf=ref_in)


def chain(n_kf, per=3):
    """Keyframe k holds the MapPoints [k*per, (k+1)*per): a feature on MapPoint k*per + j is one
    vote for keyframe k."""
    return [[k * per + j for j in range(per)] for k in range(n_kf)]


def vote(counts, per=3):
    """Features that give keyframe k counts[k] votes in a chain() world."""
    return [k * per + j for k, c in enumerate(counts) for j in range(c)]


def directed_cases():
    C = []

    def add(name, S, F):
        C.append(dict(name=name, S=S, F=F))

    # -- the tie on the maximum, non-identity kf_order: ranks 1, 2, 0 hold slots 1, 2, 0
    S = snapshot(3, chain(3), order=[2, 0, 1])
    add("tie_on_max", S, frame(S, vote([2, 1, 2])))
    # -- bad keyframes in the vote
    S = snapshot(4, chain(4), bad_kf=[1], order=[3, 1, 0, 2])
    add("most_voted_bad", S, frame(S, vote([1, 3, 2, 1]), ref_in=3))
    S = snapshot(3, chain(3), bad_kf=[0, 2])
    add("all_voted_bad", S, frame(S, vote([2, 0, 1]), local_in=[1, 0], ref_in=1))
    # -- nobody votes: the list that came in, the points under the current mp_bad
    S = snapshot(4, chain(4), bad_mp=[7], n_mp=14, temporal=[12, 13])
    add("kept_all_none", S, frame(S, [-1] * 5, local_in=[2, 0], ref_in=2))
    add("kept_all_outliers", S, frame(S, vote([1, 1, 1, 1]), outlier=[1] * 4, local_in=[2, 0],
                                      ref_in=0))
    add("kept_temporal_only", S, frame(S, [12, -1, 13, 12], local_in=[3, 2, 1], ref_in=1))
    add("kept_empty_list", S, frame(S, [-1], local_in=[], ref_in=-1))
    S = snapshot(3, chain(3), bad_kf=[1])
    add("kept_bad_kf_listed", S, frame(S, [-1, -1], local_in=[1, 2], ref_in=1))
    # -- the parent's break leaves the outer loop
    cov6 = [[], [4], [3], [], [], []]
    S = snapshot(6, chain(6), cov=cov6)
    add("parent_missing", S, frame(S, vote([1, 1, 1])))
    S = snapshot(6, chain(6), cov=cov6, parent=[1, 2, -1, -1, -1, -1])
    add("parent_in_list", S, frame(S, vote([1, 1, 1])))
    S = snapshot(6, chain(6), cov=cov6, parent=[5, -1, -1, -1, -1, -1])
    add("parent_new_first", S, frame(S, vote([1, 2, 1])))
    S = snapshot(6, chain(6), cov=cov6, parent=[-1, 5, -1, -1, -1, -1])
    add("parent_new_middle", S, frame(S, vote([1, 1, 1])))
    S = snapshot(6, chain(6), cov=cov6, parent=[-1, -1, 5, -1, -1, -1])
    add("parent_new_last", S, frame(S, vote([1, 1, 1])))
    # -- the limit of 80: every first keyframe k has the unlisted neighbour nfirst + k
    for nfirst in (79, 80, 81, 130):
        S = snapshot(2 * nfirst, chain(2 * nfirst, 1),
                     cov=[[nfirst + k] for k in range(nfirst)] + [[]] * nfirst)
        add(f"limit_first_{nfirst}", S, frame(S, vote([1] * nfirst, 1)))
    # 78, then a neighbour and a child per keyframe: 80 at the second test, 82 at the third
    S = snapshot(3 * 78, chain(3 * 78, 1), cov=[[78 + k] for k in range(78)] + [[]] * 156,
                 children=[[156 + k] for k in range(78)] + [[]] * 156)
    add("limit_crossed_mid_loop", S, frame(S, vote([1] * 78, 1)))
    # -- neighbours: slots 1..9 are bad or listed, the eligible one is the 10th / the 11th
    kfm = chain(16)
    S = snapshot(16, kfm, bad_kf=[3, 4, 5, 6, 7, 8, 9], cov=[list(range(1, 10)) + [12, 13]] + [[]] * 15)
    add("neighbour_at_10", S, frame(S, vote([2, 1, 1])))
    S = snapshot(16, kfm, bad_kf=[3, 4, 5, 6, 7, 8, 9, 10],
                 cov=[list(range(1, 11)) + [12, 13]] + [[]] * 15)
    add("neighbour_at_11", S, frame(S, vote([2, 1, 1])))
    S = snapshot(8, chain(8), bad_kf=[3], cov=[[3, 1, 5, 6], [0, 5], [], [], [], [], [], []])
    add("neighbour_first_eligible_only", S, frame(S, vote([1, 1, 1])))
    S = snapshot(5, chain(5), cov=[[3], [], [0, 1], [], []])
    add("neighbour_short_and_empty_rows", S, frame(S, vote([1, 1, 1])))
    S = snapshot(4, chain(4), cov=[[1], [2], [3], []])
    add("neighbour_of_an_added_keyframe", S, frame(S, vote([1])))
    # -- children: std::set order is kf_order, bad ones skipped
    S = snapshot(6, chain(6), order=[0, 1, 5, 4, 3, 2], parent=[-1, -1, 0, 0, 0, 0])
    add("child_by_kf_order", S, frame(S, vote([1, 1])))
    S = snapshot(6, chain(6), order=[0, 1, 5, 4, 3, 2], parent=[-1, -1, 0, 0, 0, 0], bad_kf=[5, 4])
    add("child_bad_skipped", S, frame(S, vote([1, 1])))
    S = snapshot(4, chain(4), parent=[-1, 0, 0, -1])
    add("child_listed_skipped", S, frame(S, vote([1, 1])))
    # -- a bad parent is added and its points appear
    S = snapshot(3, chain(3), parent=[2, -1, -1], bad_kf=[2])
    add("bad_parent_added", S, frame(S, vote([1])))
    # -- points
    S = snapshot(3, [[0, 1, 2], [2, 3, 0], [4, 0, 1]])
    add("points_duplicates_across", S, frame(S, [0, 3, 4]))
    S = snapshot(2, [[0, 1, 0, 1, 2], [2, 2, 3]])
    add("points_twice_in_one_keyframe", S, frame(S, [1, 3]))
    S = snapshot(4, [[0, -1, 1, -1], [], [-1, -1], [2, 1, 3]], bad_mp=[1],
                 obs={0: [0, 1, 2, 3]})
    add("points_bad_none_and_empty_keyframe", S, frame(S, [0, -1, 3]))
    # -- the frame side
    S = snapshot(3, chain(3), bad_mp=[4])
    add("feature_on_bad_point", S, frame(S, [0, 4, 3, 4, -1]))
    # ids 9, 10 temporal; 6..8 seen by the bad keyframe 2 only; each extra once, in feature order
    S = snapshot(3, chain(3), n_mp=11, bad_kf=[2], temporal=[9, 10])
    add("extras_after_locals", S, frame(S, [10, 0, 7, 9, 10, 3, 7, 6, -1, 1]))
    add("extras_with_outliers", S, frame(S, [10, 0, 7, 9, 10, 3, 7, 6, -1, 1],
                                         outlier=[0, 0, 1, 0, 1, 1, 0, 0, 0, 0]))
    # -- wave boundaries
    S = snapshot(3, chain(3, 70), n_mp=220, temporal=range(210, 220))
    for n in (0, 1, 63, 64, 65):
        feats = ([5, 212, 80, 150] * 17)[:n]
        add(f"nfeat_{n}", S, frame(S, feats, local_in=[1], ref_in=1))
    for n in (1, 64, 65, 130):
        rng = np.random.default_rng(n)
        S = snapshot(n, chain(n, 2), order=rng.permutation(n))
        add(f"n_kf_{n}", S, frame(S, vote([1 + k % 2 for k in range(n)], 2), cap_kf=n))
    rng = np.random.default_rng(77)
    big = list(rng.integers(-1, 1500, 2000))
    S = snapshot(3, [big, list(rng.integers(-1, 1600, 777)), [1599, 3, 1599]], n_mp=1600,
                 bad_mp=list(rng.integers(0, 1600, 40)))
    add("keyframe_of_2000_features", S, frame(S, list(rng.integers(-1, 1600, 130))))
    # reversed order: the row is slots 70, 69, ... 1; the first 66 are bad, so the first eligible
    # child sits in the row's second chunk of 64
    S = snapshot(75, chain(75, 1), order=list(range(74, -1, -1)),
                 parent=[-1] + [0] * 70 + [-1] * 4, bad_kf=list(range(5, 71)))
    add("child_row_of_70", S, frame(S, vote([1], 1)))
    # -- capacities: the list is 3 + 2, the block 15 + 1
    S = snapshot(6, chain(6), cov=[[3], [4], []] + [[]] * 3, n_mp=19, temporal=[18])
    feats = vote([1, 1, 1]) + [18]
    add("cap_kf_exact", S, frame(S, feats, cap_kf=5))
    add("cap_kf_over_in_extension", S, frame(S, feats, cap_kf=4, local_in=[1], ref_in=1))
    add("cap_kf_over_in_first_list", S, frame(S, feats, cap_kf=2, local_in=[1], ref_in=1))
    add("cap_mp_exact", S, frame(S, feats, cap_mp=16))
    add("cap_mp_over", S, frame(S, feats, cap_mp=15, local_in=[1], ref_in=1))
    add("cap_mp_over_by_the_locals", S, frame(S, feats, cap_mp=14, local_in=[1], ref_in=1))
    return C


# ---- corrupt snapshots: one per array ---------------------------------------------------------------

def bad_index_cases():
    """Each: a copy of one healthy case with one entry of one array out of range.  The bad values
    are small, so in a snapshot carved out of one larger zero-filled tensor the address they would
    give still lies inside that tensor: a missing check shows as a wrong answer or a missing flag."""
    def base():
        S = snapshot(6, chain(6), order=[1, 0, 2, 3, 5, 4], cov=[[3], [4], [0]] + [[]] * 3,
                     parent=[-1, 0, 0, 1, -1, -1], n_mp=20, temporal=[18, 19])
        return S, frame(S, vote([2, 1, 1]) + [18], local_in=[1, 2], ref_in=1)

    out = []

    def add(name, edit_s=None, edit_f=None, feats=None):
        S, F = base()
        if feats is not None:
            F = frame(S, feats, local_in=[1, 2], ref_in=1)
        S = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in S.items()}
        if edit_s:
            edit_s(S)
        if edit_f:
            edit_f(F)
        out.append(dict(name="bad_" + name, S=S, F=F))

    def put(arr, idx, val):
        return lambda S: S[arr].__setitem__(idx, val)

    add("kf_order_range", put("kf_order", 2, 6))
    add("kf_order_negative", put("kf_order", 2, -1))
    add("kf_order_twice", put("kf_order", 2, 3))
    add("kf_parent", put("kf_parent", 0, 6))
    add("kf_parent_below", put("kf_parent", 1, -2))
    add("kf_cov_off_decreasing", put("kf_cov_off", 1, 3))
    add("kf_cov_off_past_end", put("kf_cov_off", 3, 9))
    add("kf_cov", put("kf_cov", 1, 6))
    add("kf_cov_negative", put("kf_cov", 0, -1))
    add("kf_child_off", put("kf_child_off", 1, -1))
    add("kf_child", put("kf_child", 0, 9))
    add("kf_mp_off", put("kf_mp_off", 2, 40))
    add("kf_mp", put("kf_mp", 4, 20))
    add("kf_mp_below", put("kf_mp", 7, -2))
    add("mp_obs_off", put("mp_obs_off", 4, 1))
    add("mp_obs", put("mp_obs", 0, 6))
    add("mp_obs_negative", put("mp_obs", 3, -3))
    add("feat_mp", feats=[0, 20, 3])
    add("feat_mp_below", feats=[0, -2, 3])
    add("nfeat_past_stride", edit_f=lambda F: F.__setitem__("nfeat", len(F["feat_mp"]) + 1))
    add("nfeat_negative", edit_f=lambda F: F.__setitem__("nfeat", -1))
    add("kept_list_slot", feats=[18, -1], edit_f=lambda F: F["local_kf"].__setitem__(1, 6))
    add("kept_list_twice", feats=[18, -1], edit_f=lambda F: F["local_kf"].__setitem__(1, 1))
    add("kept_list_count", feats=[18, -1], edit_f=lambda F: F.__setitem__("n_local_kf", 7))
    return out


# ---- random --------------------------------------------------------------------------------------------

def random_batch(seed, n_kf_max=200, n_mp_max=6000, b_max=8):
    """One snapshot and up to b_max frames of it."""
    rng = np.random.default_rng(seed)
    n_kf = int(rng.integers(1, n_kf_max + 1))
    n_mp = int(rng.integers(1, n_mp_max + 1))
    order = rng.permutation(n_kf)
    bad_kf = [k for k in range(n_kf) if rng.random() < 0.1]
    parent = [-1] + [int(rng.integers(0, k)) if rng.random() < 0.9 else -1 for k in range(1, n_kf)]
    cov = [list(rng.choice(n_kf, size=min(n_kf, int(rng.integers(0, 16))), replace=False))
           for _ in range(n_kf)]
    kf_mp = []
    for k in range(n_kf):
        n = int(rng.integers(0, 120))
        # neighbouring keyframes share points: ids around k's share of the map
        c = int(n_mp * k / n_kf)
        ids = (c + rng.integers(-n_mp // 8 - 1, n_mp // 8 + 2, n)) % n_mp
        ids[rng.random(n) < 0.25] = -1
        kf_mp.append([int(x) for x in ids])
    bad_mp = [m for m in range(n_mp) if rng.random() < 0.05]
    temporal = [m for m in range(n_mp) if rng.random() < 0.02]
    S = snapshot(n_kf, kf_mp, n_mp=n_mp, order=order, bad_kf=bad_kf, parent=parent, cov=cov,
                 bad_mp=bad_mp, temporal=temporal, rec=records(n_mp, seed))
    B = int(rng.integers(1, b_max + 1))
    stride = int(rng.integers(1, 600))
    frames = []
    for f in range(B):
        mode = f % 4
        # mode 3: a full frame that sees the whole map, so that most keyframes are voted
        nfeat = stride if mode == 3 else int(rng.integers(0, stride + 1))
        c = int(rng.integers(0, n_mp))
        spread = n_mp // 2 if mode == 3 else n_mp // 10
        feats = (c + rng.integers(-spread - 1, spread + 2, nfeat)) % n_mp
        feats[rng.random(nfeat) < 0.3] = -1
        if mode == 2:
            feats[:] = -1 if not temporal else rng.choice(temporal, nfeat)      # nobody votes
        ol = (rng.random(nfeat) < 0.2).astype(np.uint8) if mode == 1 else None
        n_in = int(rng.integers(0, min(n_kf, 20) + 1))
        frames.append(frame(S, feats, outlier=ol, stride=stride, cap_kf=n_kf + 3, cap_mp=n_mp,
                            local_in=list(rng.choice(n_kf, n_in, replace=False)),
                            ref_in=int(rng.integers(-1, n_kf))))
    return S, frames


def random_cases(seeds=range(1, 9)):
    out = []
    for seed in seeds:
        S, frames = random_batch(seed)
        out += [dict(name=f"random_{seed}_{f}", S=S, F=F) for f, F in enumerate(frames)]
    return out


def mixed_batch():
    """One snapshot, six frames of one call, each in another regime: a voted list with extension;
    nobody votes (kept); every feature an outlier (kept); refused for cap_mp; refused for a
    MapPoint id out of range; every voted keyframe bad (empty list, extras only)."""
    n_kf, per = 12, 5
    S = snapshot(n_kf, chain(n_kf, per), order=[3, 0, 1, 2, 7, 6, 5, 4, 11, 10, 9, 8],
                 parent=[-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10], cov=[[k + 1] for k in range(11)] + [[]],
                 bad_kf=[10, 11], n_mp=n_kf * per + 4, temporal=range(60, 64), bad_mp=[7, 33])
    kw = dict(stride=70, cap_kf=8, cap_mp=25)
    frames = [
        frame(S, vote([2, 3, 1], per) + [61, 7], local_in=[5], ref_in=5, **kw),
        frame(S, [60, -1, 63, 60], local_in=[6, 2, 4], ref_in=4, **kw),
        frame(S, vote([1, 1, 1, 1], per), outlier=[1] * 4, local_in=[1], ref_in=1, **kw),
        frame(S, vote([1, 0, 1, 0, 1, 0, 1], per), local_in=[2], ref_in=2, **kw),
        frame(S, [0, 5, 64, 1], local_in=[3], ref_in=3, **kw),
        frame(S, vote([0] * 10 + [2, 1], per) + [62], local_in=[0, 1], ref_in=0, **kw),
    ]
    return S, frames


_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = directed_cases() + random_cases()
    return _ALL


_REF = {}


def reference(c):
    if c["name"] not in _REF:
        _REF[c["name"]] = update_local_map_np(c["S"], c["F"])
    return _REF[c["name"]]


def case_named(name):
    return next(c for c in all_cases() + bad_index_cases() if c["name"] == name)


# ---- the files of tests/native/localmap_ref.cpp --------------------------------------------------------

MAGIC = 0x4c4d4150


def write_cases(path, cases):
    w = [np.array([MAGIC, len(cases)], i32)]
    for c in cases:
        S, F = c["S"], c["F"]
        n, has = F["nfeat"], F["outlier"] is not None
        w.append(np.array([S["n_kf"], S["n_mp"], S["n_cov"], S["n_child"], S["n_kfmp"], S["n_obs"],
                           n, has, F["n_local_kf"], F["ref_kf"]], i32))
        for k in ("kf_order", "kf_bad", "kf_parent", "kf_cov_off", "kf_cov", "kf_child_off",
                  "kf_child", "kf_mp_off", "kf_mp", "mp_bad", "mp_obs_off", "mp_obs"):
            w.append(S[k].astype(i32))
        w.append(F["feat_mp"][:n].astype(i32))
        if has:
            w.append(F["outlier"][:n].astype(i32))
        w.append(F["local_kf"][:F["n_local_kf"]].astype(i32))
    np.concatenate(w).tofile(path)


def read_results(path, cases):
    w = np.fromfile(path, i32)
    at, out = 0, []

    def take(n):
        nonlocal at
        v = w[at:at + n]
        at += n
        return [int(x) for x in v]

    for _ in cases:
        kept, = take(1)
        lst = take(take(1)[0])
        ref, = take(1)
        local = take(take(1)[0])
        nulled = take(take(1)[0])
        out.append(dict(kept=bool(kept), local_kf=lst, ref_kf=ref, local_mp=local, nulled=nulled))
    assert at == len(w)
    return out
