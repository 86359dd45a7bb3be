"""MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:346-392) and ComputeDistinctiveDescriptors
(:252-313) as orbx_refresh_map_points* runs them over the CSR snapshot (include/orbx_localmap.h):
the numpy restatement with its single-decision variants, the directed cases, the corrupt snapshots,
the random batches, and the files of tests/native/mprefresh_ref.cpp.

The float steps, as the kernel and the C++ restatement take them: normali = pos - Ow in float; its
norm in double; alpha = (float)(1.0 / s); normal = normali * alpha + normal with the product and the
sum rounded on their own; normal * (float)(1.0 / n) + 0.0f at the end (a copy for n == 1);
max_dist = (float)norm(pos - Ow_ref) * scale[level]; min_dist = max_dist / scale[nlevels - 1].
A point at a camera centre gives 0 * inf: those components are compared as "is NaN"."""
from __future__ import annotations

import numpy as np

MAP_POINT_DTYPE = np.dtype([("pos", "<f4", 3), ("min_dist", "<f4"), ("normal", "<f4", 3),
                            ("max_dist", "<f4")])
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
FRAME_POSE_DTYPE = np.dtype([("Rcw", "<f4", 9), ("tcw", "<f4", 3), ("Ow", "<f4", 3),
                             ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"),
                             ("mbf", "<f4"), ("min_x", "<f4"), ("max_x", "<f4"),
                             ("min_y", "<f4"), ("max_y", "<f4"), ("log_scale_factor", "<f4"),
                             ("nlevels", "<i4"), ("scale", "<f4", 16)])
NORMAL_DEPTH, DESCRIPTOR, BOTH = 1, 2, 3
SKIPPED_BAD, NO_OBS, DESC_KEPT, CAP_OBS, BAD_INDEX = 1, 2, 4, 1 << 8, 1 << 10
REFUSED_ANY = 5 << 8
MAX_OBS = 256
MAX_OBS_CLASSES = (3, 32, 64, 256)
i32, f32, f64 = np.int32, np.float32, np.float64

VARIANTS = ["normal_skips_bad_kf", "desc_keeps_bad_kf", "s_as_float", "divide", "fma", "row_order",
            "last_on_ties", "median_n_half", "absent_ref_refused", "min_by_level"]

_POPCOUNT = np.array([bin(v).count("1") for v in range(256)], np.int32)


def _row(off, i, n_entries):
    b, e = int(off[i]), int(off[i + 1])
    return (b, e) if 0 <= b <= e <= n_entries else None


def _norm_double(v):
    """cv::norm on three floats: the squares summed in double, in order, then sqrt."""
    s = f64(0.0)
    for k in range(3):
        s = s + f64(v[k]) * f64(v[k])
    return np.sqrt(s)


def refresh_one_np(S, pid, what, max_obs, rec, desc, variant=None):
    """One id against the snapshot S; writes rec[pid] / desc[pid] in place.  Returns the info word."""
    n_kf, n_mp = S["n_kf"], S["n_mp"]
    if not 0 <= pid < n_mp:
        return BAD_INDEX
    if S["mp_bad"][pid]:
        return SKIPPED_BAD
    r = _row(S["mp_obs_off"], pid, S["n_obs"])
    if r is None:
        return BAD_INDEX
    b, e = r
    N = e - b
    if N == 0:
        return NO_OBS
    if N > max_obs:
        return CAP_OBS
    entries = []                                     # (rank, position, slot, feature)
    for t in range(N):
        s = int(S["mp_obs"][b + t])
        if not 0 <= s < n_kf:
            return BAD_INDEX
        rank = int(S["kf_order"][s])
        fr = _row(S["kf_mp_off"], s, S["n_kfmp"])
        f = int(S["mp_obs_feat"][b + t])
        if not 0 <= rank < n_kf or fr is None or not 0 <= f < fr[1] - fr[0]:
            return BAD_INDEX
        entries.append((rank, t, s, f))
    if variant != "row_order":
        entries.sort()
    if len({x[0] for x in entries}) < N or len({x[2] for x in entries}) < N:
        return BAD_INDEX
    ref = int(S["mp_ref_kf"][pid])
    if not 0 <= ref < n_kf:
        return BAD_INDEX
    held = [x[3] for x in entries if x[2] == ref]
    if not held and variant == "absent_ref_refused":
        return BAD_INDEX
    ref_feat = held[0] if held else 0                # std::map::operator[] on the copy
    fr = _row(S["kf_mp_off"], ref, S["n_kfmp"])
    nlevels = int(S["kf_pose"]["nlevels"][ref])
    if fr is None or ref_feat >= fr[1] - fr[0] or not 1 <= nlevels <= 16:
        return BAD_INDEX
    level = int(S["kf_keys"]["octave"][fr[0] + ref_feat])
    if not 0 <= level < nlevels:
        return BAD_INDEX

    word = 0
    with np.errstate(all="ignore"):
        if what & NORMAL_DEPTH:
            pos = rec["pos"][pid].astype(f32)
            normal = np.zeros(3, f32)
            n = 0
            for _, _, s, _ in entries:
                if variant == "normal_skips_bad_kf" and S["kf_bad"][s]:
                    continue
                d = pos - S["kf_pose"]["Ow"][s]
                norm = _norm_double(d)
                if variant == "s_as_float":
                    norm = f64(f32(norm))
                if variant == "divide":
                    term = d / f32(norm)
                    normal = term + normal
                elif variant == "fma":
                    alpha = f32(f64(1.0) / norm)
                    normal = (d.astype(f64) * f64(alpha) + normal.astype(f64)).astype(f32)
                else:
                    alpha = f32(f64(1.0) / norm)
                    normal = d * alpha + normal
                n += 1
            a = f64(1.0) / f64(n) if n else f64(np.inf)
            if not abs(a - 1.0) < 2.220446049250313e-16:
                normal = normal * f32(a) + f32(0.0)
            P = S["kf_pose"][ref]
            dist = f32(_norm_double(pos - P["Ow"]))
            max_dist = dist * P["scale"][level]
            min_dist = max_dist / P["scale"][level if variant == "min_by_level" else nlevels - 1]
            rec["normal"][pid] = normal
            rec["max_dist"][pid] = max_dist
            rec["min_dist"][pid] = min_dist
    if what & DESCRIPTOR:
        rows = [S["kf_desc"][int(S["kf_mp_off"][s]) + f] for _, _, s, f in entries
                if variant == "desc_keeps_bad_kf" or not S["kf_bad"][s]]
        if not rows:
            word |= DESC_KEPT
        else:
            D = np.stack(rows)
            M = len(D)
            dist = _POPCOUNT[D[:, None, :] ^ D[None, :, :]].sum(axis=2)
            med = np.sort(dist, axis=1)[:, M // 2 if variant == "median_n_half" else (M - 1) // 2]
            best = int(np.flatnonzero(med == med.min())[-1 if variant == "last_on_ties" else 0])
            desc[pid] = D[best]
    return word


def refresh_np(S, ids, what, max_obs, variant=None, rec=None, desc=None):
    """The call: info per entry of ids, and mp_rec / mp_desc as it leaves them (copies)."""
    rec = (S["mp_rec"] if rec is None else rec).copy()
    desc = (S["mp_desc"] if desc is None else desc).copy()
    # every id reads the state before the call: nothing that is read is written
    info = [refresh_one_np(S, int(p), what, max_obs, rec, desc, variant) for p in ids]
    return dict(info=info, rec=rec, desc=desc)


def same_records(a, b):
    """Bitwise, but a NaN component against a NaN component (0 * inf has no defined sign)."""
    if len(a) != len(b):
        return False
    fa_, fb = a.view(f32).reshape(-1), b.view(f32).reshape(-1)
    na, nb = np.isnan(fa_), np.isnan(fb)
    return bool((na == nb).all() and
                (fa_.view(np.uint32)[~na] == fb.view(np.uint32)[~nb]).all())


def result_key(r):
    rec = r["rec"].view(f32).copy()
    rec[np.isnan(rec)] = f32(7e33)
    return (tuple(r["info"]), rec.tobytes(), r["desc"].tobytes())


# ---- builders ----------------------------------------------------------------------------------------

def _csr(rows):
    off = np.zeros(len(rows) + 1, i32)
    off[1:] = np.cumsum([len(r) for r in rows])
    return off, np.array([x for r in rows for x in r], i32)


def scale_factors(nlevels, factor=1.2):
    """mvScaleFactors as ORBextractor builds them: float products."""
    s = np.zeros(16, f32)
    s[0] = 1.0
    for k in range(1, nlevels):
        s[k] = s[k - 1] * f32(factor)
    return s


def snapshot(n_kf, obs, *, seed=0, order=None, bad_kf=(), bad_mp=(), ref=None, nlevels=8,
             spare_feats=2, octave=None, flips=40):
    """obs: per MapPoint the observing slots, in row order.  Every observation gets a feature of its
    own in its keyframe, after `spare_feats` features no MapPoint holds (so feature 0 is another
    one); ref: per MapPoint the reference slot (default: the row's first, or 0)."""
    rng = np.random.RandomState(1000 + seed)
    n_mp = len(obs)
    nfeat = [spare_feats] * n_kf
    feats = []
    for row in obs:
        fr = []
        for s in row:
            fr.append(nfeat[s])
            nfeat[s] += 1
        feats.append(fr)
    kf_mp_off = np.zeros(n_kf + 1, i32)
    kf_mp_off[1:] = np.cumsum(nfeat)
    n_kfmp = int(kf_mp_off[-1])
    kf_mp = np.full(n_kfmp, -1, i32)
    for p, (row, fr) in enumerate(zip(obs, feats)):
        for s, f in zip(row, fr):
            kf_mp[kf_mp_off[s] + f] = p
    mp_obs_off, mp_obs = _csr(obs)
    _, mp_obs_feat = _csr(feats)
    S = dict(n_kf=n_kf, n_mp=n_mp, n_cov=0, n_child=0, n_kfmp=n_kfmp, n_obs=len(mp_obs))
    S["kf_order"] = np.array(order if order is not None else rng.permutation(n_kf), i32)
    S["kf_bad"] = np.zeros(n_kf, np.uint8)
    S["kf_bad"][list(bad_kf)] = 1
    S["kf_parent"] = np.full(n_kf, -1, i32)
    S["kf_cov_off"], S["kf_cov"] = np.zeros(n_kf + 1, i32), np.zeros(0, i32)
    S["kf_child_off"], S["kf_child"] = np.zeros(n_kf + 1, i32), np.zeros(0, i32)
    S["kf_mp_off"], S["kf_mp"] = kf_mp_off, kf_mp
    S["mp_bad"] = np.zeros(n_mp, np.uint8)
    S["mp_bad"][list(bad_mp)] = 1
    S["mp_obs_off"], S["mp_obs"], S["mp_obs_feat"] = mp_obs_off, mp_obs, mp_obs_feat
    S["mp_ref_kf"] = np.array([(row[0] if row else 0) for row in obs] if ref is None else ref, i32)
    rec = np.zeros(n_mp, MAP_POINT_DTYPE)
    rec["pos"] = rng.uniform(-4, 4, (n_mp, 3)).astype(f32)
    rec["normal"] = rng.uniform(-1, 1, (n_mp, 3)).astype(f32)      # what was there before
    rec["min_dist"], rec["max_dist"] = f32(0.25), f32(40.0)
    S["mp_rec"] = rec
    pose = np.zeros(n_kf, FRAME_POSE_DTYPE)
    pose["Ow"] = rng.uniform(-6, 6, (n_kf, 3)).astype(f32)
    pose["nlevels"] = nlevels
    pose["scale"] = scale_factors(nlevels)
    S["kf_pose"] = pose
    keys = np.zeros(n_kfmp, KEYPOINT_DTYPE)
    keys["octave"] = rng.randint(0, nlevels, n_kfmp) if octave is None else octave
    S["kf_keys"] = keys
    # a descriptor per MapPoint, some bits flipped per observation: medians that mean something
    base = rng.randint(0, 256, (n_mp, 32)).astype(np.uint8)
    kd = rng.randint(0, 256, (n_kfmp, 32)).astype(np.uint8)
    for p, (row, fr) in enumerate(zip(obs, feats)):
        for s, f in zip(row, fr):
            d = np.unpackbits(base[p])
            d[rng.choice(256, rng.randint(0, flips + 1), replace=False)] ^= 1
            kd[kf_mp_off[s] + f] = np.packbits(d)
    S["kf_desc"] = kd
    S["mp_desc"] = rng.randint(0, 256, (n_mp, 32)).astype(np.uint8)
    return S


def case(name, S, ids=None, what=BOTH, max_obs=MAX_OBS):
    ids = np.arange(S["n_mp"], dtype=i32) if ids is None else np.array(ids, i32)
    return dict(name=name, S=S, ids=ids, what=what, max_obs=max_obs)


def _feat_at(S, p, t):
    """Index into kf_keys / kf_desc of observation t of point p."""
    o = int(S["mp_obs_off"][p]) + t
    return int(S["kf_mp_off"][S["mp_obs"][o]]) + int(S["mp_obs_feat"][o])


def directed_cases():
    C = []
    for n in (1, 2, 3, 63, 64, 65, 128, 256, 257):
        n_kf = n + 3
        rng = np.random.RandomState(n)
        rows = [list(rng.permutation(n_kf)[:n]), list(rng.permutation(n_kf)[:max(1, n // 2)])]
        C.append(case(f"row_of_{n}", snapshot(n_kf, rows, seed=n)))
    rows4 = [[0, 1, 2, 3], [3, 1], [2], [1, 0, 3]]
    C.append(case("bad_point", snapshot(4, rows4, seed=1, bad_mp=[1])))
    C.append(case("empty_row", snapshot(4, [[0, 1], [], [2, 3, 1]], seed=2)))
    C.append(case("every_keyframe_bad", snapshot(4, rows4, seed=3, bad_kf=[0, 1, 2, 3])))
    C.append(case("one_keyframe_not_bad", snapshot(4, rows4, seed=4, bad_kf=[0, 1, 2])))
    C.append(case("some_keyframes_bad", snapshot(6, [[0, 1, 2, 3, 4, 5], [5, 3, 1, 0]], seed=5,
                                                 bad_kf=[1, 4])))
    # rank order against row order: float terms whose sum depends on the order, and descriptors
    # whose tie goes to another row
    C.append(case("rank_order_differs", snapshot(7, [[6, 0, 3, 5, 1], [2, 6, 4, 0, 1, 5, 3]], seed=6,
                                                 order=[3, 6, 0, 5, 1, 2, 4])))
    S = snapshot(7, [[0, 1, 2, 3, 4, 5, 6]], seed=7, order=[6, 5, 4, 3, 2, 1, 0])
    # median ties: rows 0 and 6 of the rank order are equally central copies of one descriptor pair
    d = S["kf_desc"]
    a, b = d[_feat_at(S, 0, 0)].copy(), d[_feat_at(S, 0, 0)].copy()
    b[0] ^= 0xff
    for t, v in enumerate((a, b, a, b, a, b, a)):
        d[_feat_at(S, 0, t)] = v
    d[_feat_at(S, 0, 3)][1] ^= 1
    C.append(case("median_ties", S))
    S = snapshot(5, [[0, 1, 2, 3, 4], [4, 2]], seed=8)
    for p, n in ((0, 5), (1, 2)):
        for t in range(n):
            S["kf_desc"][_feat_at(S, p, t)] = S["kf_desc"][_feat_at(S, p, 0)]
    C.append(case("identical_descriptors", S))
    S = snapshot(4, [[0, 1, 2], [3, 1]], seed=9)
    S["mp_rec"]["pos"][0] = S["kf_pose"]["Ow"][1]           # 0 * inf in every component
    S["mp_rec"]["pos"][1] = S["kf_pose"]["Ow"][3]
    C.append(case("point_at_a_camera_centre", S))
    S = snapshot(4, [[0]], seed=10)
    S["mp_rec"]["pos"][0] = S["kf_pose"]["Ow"][0]           # n == 1 there: the copy keeps the NaN
    C.append(case("point_at_its_only_camera", S))
    C.append(case("reference_keyframe_absent", snapshot(5, [[0, 1, 2], [3, 4]], seed=11, ref=[4, 0])))
    C.append(case("n_is_1", snapshot(3, [[2], [0], [1]], seed=12)))
    S = snapshot(3, [[0, 1], [1, 2], [2, 0]], seed=13, nlevels=8)
    S["kf_keys"]["octave"][_feat_at(S, 0, 0)] = 0
    S["kf_keys"]["octave"][_feat_at(S, 1, 0)] = 7
    S["kf_keys"]["octave"][_feat_at(S, 2, 0)] = 3
    C.append(case("octave_0_and_last", S))
    S = snapshot(3, [[0, 1], [1, 2]], seed=14, nlevels=1)
    C.append(case("one_level", S))
    S = snapshot(3, [[0, 1], [1, 2]], seed=15, nlevels=16)
    S["kf_keys"]["octave"][_feat_at(S, 0, 0)] = 15
    C.append(case("sixteen_levels", S))
    C.append(case("repeated_id", snapshot(4, rows4, seed=16), ids=[2, 0, 2, 3, 0, 0]))
    C.append(case("what_normal_depth", snapshot(4, rows4, seed=17, bad_kf=[1]), what=NORMAL_DEPTH))
    C.append(case("what_descriptor", snapshot(4, rows4, seed=17, bad_kf=[1]), what=DESCRIPTOR))
    C.append(case("what_descriptor_all_bad", snapshot(4, rows4, seed=18, bad_kf=[0, 1, 2, 3]),
                  what=DESCRIPTOR))
    C.append(case("what_normal_depth_all_bad", snapshot(4, rows4, seed=18, bad_kf=[0, 1, 2, 3]),
                  what=NORMAL_DEPTH))
    # more than 64 descriptors left after the bad keyframes are dropped, and exactly 64
    C.append(case("multi_pass_with_bad", snapshot(140, [list(range(139, 9, -1))], seed=19,
                                                  bad_kf=range(10, 40))))
    C.append(case("64_left_of_80", snapshot(80, [list(range(80))], seed=20, bad_kf=range(0, 80, 5))))
    # max_obs classes: the same map under every class; longer rows are refused
    lens = (1, 3, 4, 32, 33, 64, 65, 100)
    rng = np.random.RandomState(21)
    rows = [list(rng.permutation(110)[:n]) for n in lens]
    for mo in MAX_OBS_CLASSES:
        C.append(case(f"max_obs_{mo}", snapshot(110, rows, seed=21, bad_kf=[5, 50]), max_obs=mo))
    return C


def bad_index_cases():
    """One corrupt value each, beside healthy points; `cause` names it."""
    rows = [[0, 1, 2], [3, 1], [2, 4, 0, 1], [4]]
    base = lambda: snapshot(5, rows, seed=30)
    C = []

    def add(cause, S, ids=None):
        c = case("bad_" + cause, S, ids)
        c["cause"] = cause
        C.append(c)

    add("id_high", base(), ids=[0, 4, 1])
    add("id_negative", base(), ids=[-1, 2])
    add("id_far", base(), ids=[3, 1 << 20])
    S = base(); S["mp_obs_off"][2] = 2; add("row_decreasing", S)
    S = base(); S["mp_obs_off"][4] = S["n_obs"] + 3; add("row_leaves_mp_obs", S)
    S = base(); S["mp_obs_off"][0] = -2; add("row_negative", S)
    S = base(); S["mp_obs"][4] = 5; add("slot_high", S)
    S = base(); S["mp_obs"][0] = -1; add("slot_negative", S)
    S = base(); S["mp_ref_kf"][1] = 5; add("ref_slot_high", S)
    S = base(); S["mp_ref_kf"][2] = -1; add("ref_slot_negative", S)
    S = base(); S["kf_order"][1] = 5; add("rank_high", S)
    S = base(); S["kf_order"][2] = -3; add("rank_negative", S)
    S = base(); S["mp_obs"][6] = 2; add("slot_twice", S)
    S = base(); S["kf_order"][4] = S["kf_order"][0]; add("rank_twice", S)
    S = base(); S["mp_obs_feat"][3] = 99; add("feature_high", S)
    S = base(); S["mp_obs_feat"][5] = -1; add("feature_negative", S)
    S = base(); S["kf_mp_off"][5] = S["n_kfmp"] + 7; add("feature_row_leaves_kf_keys", S)
    S = base(); S["kf_pose"]["nlevels"][3] = 0; add("nlevels_0", S)
    S = base(); S["kf_pose"]["nlevels"][0] = 17; add("nlevels_17", S)
    S = base(); S["kf_keys"]["octave"][_feat_at(S, 1, 0)] = 8; add("octave_high", S)
    S = base(); S["kf_keys"]["octave"][_feat_at(S, 3, 0)] = -1; add("octave_negative", S)
    # the reference keyframe is absent and has no feature 0
    S = snapshot(5, [[0, 1], [2]], seed=31, spare_feats=0, ref=[3, 2])
    add("feature_0_of_an_empty_reference", S)
    return C


def random_batch(seed, n_kf_max=40, n_mp_max=300):
    rng = np.random.RandomState(seed)
    n_kf = int(rng.randint(2, n_kf_max + 1))
    n_mp = int(rng.randint(1, n_mp_max + 1))
    rows = []
    for _ in range(n_mp):
        n = int(rng.choice([0, 1, 2, 3, 5, 8, 13, n_kf], p=[.04, .1, .2, .2, .2, .12, .1, .04]))
        rows.append(list(rng.permutation(n_kf)[:min(n, n_kf)]))
    bad_kf = list(np.flatnonzero(rng.rand(n_kf) < 0.15))
    bad_mp = list(np.flatnonzero(rng.rand(n_mp) < 0.05))
    ref = [int(rng.choice(r)) if r and rng.rand() < 0.9 else int(rng.randint(n_kf)) for r in rows]
    S = snapshot(n_kf, rows, seed=100 + seed, bad_kf=bad_kf, bad_mp=bad_mp, ref=ref)
    ids = rng.permutation(n_mp)[:max(1, int(n_mp * rng.uniform(0.3, 1.0)))]
    return case(f"random_{seed}", S, ids=ids, what=int(rng.choice([1, 2, 3, 3])),
                max_obs=int(rng.choice([32, 64, 256])))


def random_cases(seeds=range(1, 9)):
    return [random_batch(s) for s in seeds]


_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = directed_cases() + random_cases()
    return _ALL


_REF = {}


def reference(c):
    if c["name"] not in _REF:
        _REF[c["name"]] = refresh_np(c["S"], c["ids"], c["what"], c["max_obs"])
    return _REF[c["name"]]


def case_named(name):
    return next(c for c in all_cases() + bad_index_cases() if c["name"] == name)


ARRAYS = ("kf_order", "kf_bad", "kf_parent", "kf_cov_off", "kf_cov", "kf_child_off", "kf_child",
          "kf_mp_off", "kf_mp", "mp_bad", "mp_obs_off", "mp_obs", "mp_rec")
EXTRA = ("mp_obs_feat", "mp_ref_kf", "kf_pose", "kf_keys", "kf_desc")


# ---- the files of tests/native/mprefresh_ref.cpp -----------------------------------------------------
# The objects know no capacity and cannot be corrupt: a case goes there with every row within
# ORBX_REFRESH_MAX_OBS and comes back as the final records and descriptors of every MapPoint.

MAGIC = 0x4d505246


def write_cases(path, cases):
    w = [np.array([MAGIC, len(cases)], i32).tobytes()]
    for c in cases:
        S = c["S"]
        w.append(np.array([S["n_kf"], S["n_mp"], S["n_kfmp"], S["n_obs"], len(c["ids"]), c["what"]],
                          i32).tobytes())
        for k in ("kf_order", "kf_bad", "kf_mp_off", "mp_bad", "mp_obs_off", "mp_obs", "mp_obs_feat",
                  "mp_ref_kf"):
            w.append(S[k].astype(i32).tobytes())
        w.append(np.ascontiguousarray(S["kf_pose"]["Ow"], f32).tobytes())
        w.append(S["kf_pose"]["nlevels"].astype(i32).tobytes())
        w.append(np.ascontiguousarray(S["kf_pose"]["scale"], f32).tobytes())
        w.append(S["kf_keys"]["octave"].astype(i32).tobytes())
        w.append(np.ascontiguousarray(S["kf_desc"], np.uint8).tobytes())
        w.append(S["mp_rec"].tobytes())
        w.append(np.ascontiguousarray(S["mp_desc"], np.uint8).tobytes())
        w.append(c["ids"].astype(i32).tobytes())
    with open(path, "wb") as f:
        f.write(b"".join(w))


def read_results(path, cases):
    raw = open(path, "rb").read()
    at, out = 0, []
    for c in cases:
        n_mp = c["S"]["n_mp"]
        rec = np.frombuffer(raw, MAP_POINT_DTYPE, n_mp, at).copy()
        at += 32 * n_mp
        desc = np.frombuffer(raw, np.uint8, 32 * n_mp, at).reshape(n_mp, 32).copy()
        at += 32 * n_mp
        out.append(dict(rec=rec, desc=desc))
    assert at == len(raw)
    return out
