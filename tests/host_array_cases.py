"""The nine per-frame host-array entry points (orbx_undistort_keypoints, orbx_is_in_frustum,
orbx_project_map_points, orbx_unproject_stereo, orbx_close_points, orbx_compute_stereo_from_rgbd,
orbx_cvt_color, orbx_remap, orbx_bow_db_score) and the nine of a matcher handle (MATCHER_NAMES: the
BoW, triangulation, projection, Sim3 and initialization searches, the distinctive descriptors and
the brute-force top-2) on one tiny case each, called straight through the C
ABI so that the caller's output arrays can sit inside sentinel-filled allocations: 64 guard bytes
on both sides, padded rows, slots the call does not document as written.

    c = case("frustum")      # the inputs, built once and never modified
    r = c.call()             # {"name": Guarded or a scalar}: fresh outputs, one call

The sentinel tests next to each entry point's GPU tests check `r` against that entry point's
restatement; tests/test_gpu_concurrency.py compares `r` across threads."""
import ctypes
import functools
import threading

import numpy as np

from my_orb_slam2_amd import synth
from my_orb_slam2_amd._lib import KEYPOINT_DTYPE
from my_orb_slam2_amd.features import (DEPTH_F32, DEPTH_U16, MAP_POINT_DTYPE, PROJ_FRAME_MAPPOINTS,
                                       PROJ_FUSE, PROJ_LAST_FRAME, PROJ_QUERY_DTYPE, featureset_c)

f32 = np.float32
SENT = 0xA5
GUARD = 64
NAMES = ("undistort", "frustum", "project", "unproject", "close", "rgbd_u16", "rgbd_f32",
         "cvt_color3", "cvt_color4", "remap", "bow_db_score")


class Guarded:
    """`a`: an array of `dtype` and `shape` filled with SENT bytes, inside an allocation with GUARD
    more SENT bytes on both sides."""

    def __init__(self, dtype, shape):
        dtype = np.dtype(dtype)
        n = int(np.prod(shape)) * dtype.itemsize
        self.alloc = np.full(n + 2 * GUARD, SENT, np.uint8)
        self.a = self.alloc[GUARD:GUARD + n].view(dtype).reshape(shape)

    def guards_intact(self):
        return bool((self.alloc[:GUARD] == SENT).all() and (self.alloc[-GUARD:] == SENT).all())


def sentinel(dtype, n=1):
    """n records of SENT bytes."""
    return np.full(n * np.dtype(dtype).itemsize, SENT, np.uint8).view(dtype)


def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _ok(name, status):
    assert status == 0, (name, status)


class Case:
    def __init__(self, name, call, **inputs):
        self.name, self._call = name, call
        self.__dict__.update(inputs)

    def call(self):
        from my_orb_slam2_amd._lib import load
        return self._call(load(), self)

    def call_bytes(self):
        """(1, every returned byte): the form tests/test_gpu_concurrency.py compares."""
        r = self.call()
        return (1,) + tuple(v.alloc.tobytes() if isinstance(v, Guarded) else v
                            for _, v in sorted(r.items()))


def _keys(rng, n, w=640, h=480):
    k = np.zeros(n, KEYPOINT_DTYPE)
    k["x"], k["y"] = rng.uniform(20, w - 20, n), rng.uniform(20, h - 20, n)
    k["size"], k["angle"] = 31.0, rng.uniform(0, 360, n)
    k["response"], k["octave"], k["class_id"] = rng.uniform(20, 90, n), rng.integers(0, 8, n), -1
    return k


def _undistort():
    K4, dist = synth.TUM1_CAM                       # k1 != 0: the keypoints are undistorted
    K4, dist = np.asarray(K4, f32), np.asarray(dist, f32)
    assert dist[0] != 0

    def call(L, c):
        un = Guarded(KEYPOINT_DTYPE, 3)
        _ok(c.name, L.orbx_undistort_keypoints(_p(c.K4), _p(c.dist), len(c.dist), _p(c.keys), 3,
                                               _p(un.a), 0))
        return dict(keys_un=un)
    return Case("undistort", call, K4=K4, dist=dist, keys=_keys(np.random.default_rng(41), 3))


def _scene(seed):
    import projection_cases as pc
    keys, desc = pc._scene_keys(seed)
    return synth.local_map_points(seed, keys, desc, 60, synth.EUROC_CAM[0],
                                  (0.0, 752.0, 0.0, 480.0), mbf=40.0, skip_frac=0.0)


def _frustum():
    F, mps, _, _ = _scene(3)

    def call(L, c):
        q, nv = Guarded(PROJ_QUERY_DTYPE, 3), Guarded(np.int32, 1)
        _ok(c.name, L.orbx_is_in_frustum(_p(c.F), _p(c.mps), 3, _p(c.skip), 0.5, 1.0, _p(q.a),
                                         _p(nv.a), 0))
        return dict(q=q, nvisible=nv)
    return Case("frustum", call, F=np.ascontiguousarray(F).reshape(()),
                mps=np.ascontiguousarray(mps[:3], MAP_POINT_DTYPE),
                skip=np.array([0, 1, 0], np.uint8))


def _project():
    import projection_cases as pc
    pose, mps, _, _ = _scene(11)
    job = pc.job_from_pose(PROJ_LAST_FRAME, pose, 11)

    def call(L, c):
        q, na = Guarded(PROJ_QUERY_DTYPE, 3), Guarded(np.int32, 1)
        _ok(c.name, L.orbx_project_map_points(PROJ_LAST_FRAME, _p(c.job), _p(c.mps), 3,
                                              _p(c.src_keys), _p(c.skip), _p(q.a), _p(na.a), 0))
        return dict(q=q, nactive=na)
    return Case("project", call, job=np.ascontiguousarray(job).reshape(()),
                mps=np.ascontiguousarray(mps[:3], MAP_POINT_DTYPE),
                src_keys=pc._keys(3, 8, seed=11), skip=np.array([0, 1, 0], np.uint8))


def _unproject():
    import rgbd_cases as rc

    def call(L, c):
        x3d, valid = Guarded(f32, (3, 3)), Guarded(np.uint8, 3)
        _ok(c.name, L.orbx_unproject_stereo(_p(c.F), _p(c.keys), _p(c.depth), 3, _p(x3d.a),
                                            _p(valid.a), 0))
        return dict(x3d=x3d, valid=valid)
    return Case("unproject", call, F=rc.pose(5), keys=_keys(np.random.default_rng(42), 3),
                depth=np.array([2.0, -1.0, 3.5], f32))        # slot 1 has no depth


def _close():
    import rgbd_cases as rc

    def call(L, c):
        order, counts = Guarded(np.int32, 5), Guarded(np.int32, 4)
        create, x3d = Guarded(np.uint8, 5), Guarded(f32, (5, 3))
        _ok(c.name, L.orbx_close_points(_p(c.F), _p(c.keys), _p(c.depth), _p(c.has_point), None, 5,
                                        float(c.th), 100, _p(order.a), _p(counts.a), _p(create.a),
                                        _p(x3d.a), 0))
        return dict(order=order, counts=counts, create=create, x3d=x3d)
    # two close points (one has a MapPoint), the threshold itself, a far one, one without depth
    return Case("close", call, F=rc.pose(6), keys=_keys(np.random.default_rng(43), 5), th=rc.TH,
                depth=np.array([2.5, 1.25, 3.0, 7.0, -1.0], f32),
                has_point=np.array([0, 1, 0, 0, 1], np.uint8))


def _rgbd(depth_type):
    import rgbd_cases as rc
    d = rc.depth_case(5, depth_type, "tum" if depth_type == DEPTH_U16 else "one", 3)
    assert d["row_stride"] > rc.W * d["alloc"].itemsize

    def call(L, c):
        ur, de = Guarded(f32, 3), Guarded(f32, 3)
        _ok(c.name, L.orbx_compute_stereo_from_rgbd(
            _p(c.d["alloc"]), c.d["depth_type"], c.d["row_stride"], rc.W, rc.H,
            float(c.d["factor"]), float(c.d["mbf"]), _p(c.d["kps"]), _p(c.d["kps_un"]), 3, _p(ur.a),
            _p(de.a), 0))
        return dict(u_right=ur, depth=de)
    return Case("rgbd_u16" if depth_type == DEPTH_U16 else "rgbd_f32", call, d=d)


CVT_W, CVT_H = 5, 3


def _cvt_color(channels):
    src_stride, dst_stride = CVT_W * channels + 3, CVT_W + 2      # both padded
    src = np.random.default_rng(44 + channels).integers(0, 256, (CVT_H, src_stride), dtype=np.uint8)

    def call(L, c):
        dst = Guarded(np.uint8, (CVT_H, c.dst_stride))
        _ok(c.name, L.orbx_cvt_color(_p(c.src), CVT_W, CVT_H, c.src_stride, c.channels, 1, _p(dst.a),
                                     c.dst_stride, 0))
        return dict(dst=dst)
    return Case(f"cvt_color{channels}", call, src=src, channels=channels, src_stride=src_stride,
                dst_stride=dst_stride)


def _remap():
    import remap_cases as rc
    from my_orb_slam2_amd import Rectifier, rectify
    c0 = next(c for c in rc.build_cases(rectify.images_per_chunk()) if c["name"] == "border_1x1")
    lay = rc.layout(c0)
    assert lay["dst_rs"] > c0["map1"].shape[1]
    _, sh, sw = c0["src"].shape
    rect = Rectifier(c0["map1"], c0["map2"], src_size=(sw, sh))

    def call(L, c):
        dh = c.c0["map1"].shape[0]
        dst = Guarded(np.uint8, (dh, c.lay["dst_rs"]))              # padding pre-filled
        src = c.lay["src"][c.lay["src_off"]:]
        _ok(c.name, L.orbx_remap(c.rect._h, _p(src), c.lay["src_rs"], _p(dst.a), c.lay["dst_rs"]))
        return dict(dst=dst)
    return Case("remap", call, c0=c0, lay=lay, rect=rect)


def _bow_db_score():
    lead = 5                                                          # kf_off[0] != 0
    q = (np.array([2, 5, 9], np.uint32), np.array([0.5, 0.25, 0.25]))
    kfs = [(np.array([2, 9, 11], np.uint32), np.array([0.125, 0.5, 0.375])),
           (np.array([5], np.uint32), np.array([1.0]))]
    off = (lead + np.concatenate([[0], np.cumsum([len(b[0]) for b in kfs])])).astype(np.int32)
    words = np.concatenate([np.full(lead, 7, np.uint32)] + [b[0] for b in kfs])
    vals = np.concatenate([np.full(lead, 0.25)] + [b[1] for b in kfs])

    def call(L, c):
        common, score = Guarded(np.int32, 2), Guarded(f32, 2)
        _ok(c.name, L.orbx_bow_db_score(_p(c.q[0]), _p(c.q[1]), 3, 2, _p(c.off), _p(c.words),
                                        _p(c.vals), _p(common.a), _p(score.a), 0))
        return dict(common=common, score=score)
    return Case("bow_db_score", call, q=q, kfs=kfs, off=off, words=words, vals=vals)


# ---- the matcher handle's host-array forms -------------------------------------------------------
# 70 and 130 features, 70 queries: more than a wave, and parts that end inside and past a 256-byte
# block (70 int32 = 280 bytes, 70 flag bytes, 130 x 32 descriptor bytes)
N1, N2 = 70, 130
MATCHER_NAMES = ("bow_kf_frame", "bow_kf_kf", "tri_exact", "tri_short", "proj_greedy", "proj_fuse",
                 "proj_ex", "proj_nq0", "by_sim3", "init", "distinctive", "bf", "bf_ndb0")
ERR_CAPACITY = -3
_tls = threading.local()


def _matcher(nnratio, check_ori):
    """The calling thread's handle for these parameters: a handle is not re-entrant."""
    from my_orb_slam2_amd import ORBmatcher
    cache = _tls.__dict__.setdefault("matchers", {})
    if (nnratio, check_ori) not in cache:
        cache[nnratio, check_ori] = ORBmatcher(nnratio, check_ori)
    return cache[nnratio, check_ori]


def _fs(fs):
    return ctypes.byref(featureset_c(fs))


def _bow(kf_kf):
    f1, f2, _ = synth.feature_pair(501, n1=N1, n2=N2, nodes=8)
    rng = np.random.default_rng(501)
    v1, v2 = (rng.random(N1) < 0.85).astype(np.uint8), (rng.random(N2) < 0.85).astype(np.uint8)

    def call(L, c):
        h = _matcher(*c.params)._h
        out, n = Guarded(np.int32, N1 if kf_kf else N2), Guarded(np.int32, 1)
        if kf_kf:
            _ok(c.name, L.orbx_search_by_bow_kf_kf(h, _fs(c.f1), _p(c.v1), _fs(c.f2), _p(c.v2),
                                                   _p(out.a), _p(n.a)))
        else:
            _ok(c.name, L.orbx_search_by_bow_kf_frame(h, _fs(c.f1), _p(c.v1), _fs(c.f2), _p(out.a),
                                                      _p(n.a)))
        return dict(match=out, nmatches=n)
    return Case("bow_kf_kf" if kf_kf else "bow_kf_frame", call, f1=f1, f2=f2, v1=v1, v2=v2,
                params=(0.75, True))


def _tri(short):
    """pair_cap is the number of pairs (needs the GPU: one call with room for every feature), or
    with `short` one less; the pair array has room for the number of pairs either way."""
    k1, k2, F, epi, _ = synth.keyframe_pair(502, n1=N1, n2=N2, nodes=8)
    rng = np.random.default_rng(502)
    h1, h2 = (rng.random(N1) < 0.3).astype(np.uint8), (rng.random(N2) < 0.3).astype(np.uint8)
    scale, sigma2, _ = synth.scale_tables()
    params = (0.6, False)
    count, _ = _matcher(*params).SearchForTriangulation(k1, h1, k2, h2, F, epi, sigma2, scale)
    assert count >= 2

    def call(L, c):
        pairs, n = Guarded(np.int32, (c.count, 2)), Guarded(np.int32, 1)
        status = L.orbx_search_for_triangulation(
            _matcher(*c.params)._h, _fs(c.k1), _p(c.h1), _fs(c.k2), _p(c.h2), _p(c.F),
            float(c.epi[0]), float(c.epi[1]), _p(c.sigma2), _p(c.scale), len(c.sigma2), 0,
            _p(pairs.a), c.pair_cap, _p(n.a))
        return dict(pairs=pairs, nmatches=n, status=status)
    return Case("tri_short" if short else "tri_exact", call, k1=k1, k2=k2, h1=h1, h2=h2,
                F=np.ascontiguousarray(F, f32).reshape(9), epi=epi, sigma2=sigma2, scale=scale,
                params=params, count=count, pair_cap=count - int(short))


def _proj(name):
    """proj_greedy: FRAME_MAPPOINTS with a claimed mask; proj_fuse: FUSE with inv_sigma2; proj_ex:
    LAST_FRAME through _ex with no-claim queries and the prefilter flag; proj_nq0: no query, a
    four-slot match array that stays as it is."""
    mode = {"proj_greedy": PROJ_FRAME_MAPPOINTS, "proj_fuse": PROJ_FUSE, "proj_ex": PROJ_LAST_FRAME,
            "proj_nq0": PROJ_FRAME_MAPPOINTS}[name]
    f1, f2, t = synth.feature_pair(503, n1=N1, n2=N2, dup_frac=0.1)
    q, d = synth.projection_queries(3, f1, f2, t, th=15.0,
                                    mode_levels="kf" if mode == PROJ_FUSE else "frame")
    rng = np.random.default_rng(503)
    claimed = None if mode == PROJ_FUSE else (rng.random(N2) < 0.1).astype(np.uint8)
    qflags = (rng.random(len(q)) < 0.33).astype(np.uint8) if name == "proj_ex" else None
    isg = synth.scale_tables()[2] if mode == PROJ_FUSE else None
    nq = 0 if name == "proj_nq0" else len(q)

    def call(L, c):
        h = _matcher(*c.params)._h
        out, n = Guarded(np.int32, c.nq or 4), Guarded(np.int32, 1)
        nlev = 0 if c.isg is None else len(c.isg)
        if c.qflags is None:
            _ok(c.name, L.orbx_search_by_projection(h, c.mode, _fs(c.f2), _p(c.claimed), _p(c.d),
                                                    _p(c.q), c.nq, _p(c.isg), nlev, 64, _p(out.a),
                                                    _p(n.a)))
        else:
            _ok(c.name, L.orbx_search_by_projection_ex(h, c.mode, _fs(c.f2), _p(c.claimed), _p(c.d),
                                                       _p(c.q), _p(c.qflags), c.nq, _p(c.isg), nlev,
                                                       64, 1, _p(out.a), _p(n.a)))
        return dict(match=out, nmatches=n)
    return Case(name, call, mode=mode, f2=f2, q=q, d=d, claimed=claimed, qflags=qflags, isg=isg,
                nq=nq, params=(0.8, True))


def _sim3():
    f1, f2, t = synth.feature_pair(504, n1=N1, n2=N2)
    q12, d1 = synth.projection_queries(1, f1, f2, t, th=7.5, mode_levels="kf")
    inv = np.full(N2, -1, np.int64)
    inv[t[t >= 0]] = np.nonzero(t >= 0)[0]
    q21, d2 = synth.projection_queries(2, f2, f1, inv, th=7.5, mode_levels="kf")

    def call(L, c):
        out, n = Guarded(np.int32, N1), Guarded(np.int32, 1)
        _ok(c.name, L.orbx_search_by_sim3(_matcher(*c.params)._h, _fs(c.f1), _fs(c.f2), _p(c.d1),
                                          _p(c.q12), N1, _p(c.d2), _p(c.q21), N2, _p(out.a),
                                          _p(n.a)))
        return dict(match=out, nmatches=n)
    return Case("by_sim3", call, f1=f1, f2=f2, q12=q12, d1=d1, q21=q21, d2=d2, params=(0.75, True))


def _init():
    f1, f2, _ = synth.feature_pair(505, n1=N1, n2=N2, dup_frac=0.1)
    prev = np.ascontiguousarray(np.stack([f1.keys["x"], f1.keys["y"]], 1), f32)

    def call(L, c):
        prev, out, n = Guarded(f32, (N1, 2)), Guarded(np.int32, N1), Guarded(np.int32, 1)
        prev.a[:] = c.prev
        _ok(c.name, L.orbx_search_for_initialization(_matcher(*c.params)._h, _fs(c.f1), _fs(c.f2),
                                                     _p(prev.a), c.window, _p(out.a), _p(n.a)))
        return dict(prev_matched=prev, match=out, nmatches=n)
    return Case("init", call, f1=f1, f2=f2, prev=prev, window=100, params=(0.9, True))


def _distinctive():
    from test_oracle_match import _distinctive_case
    lead = 3                                                          # off[0] != 0
    desc, off = _distinctive_case(506, N1, 12)
    desc = np.concatenate([np.full((lead, 32), 0x5A, np.uint8), desc])

    def call(L, c):
        best = Guarded(np.int32, N1)
        _ok(c.name, L.orbx_compute_distinctive_descriptors(_matcher(*c.params)._h, _p(c.desc),
                                                           _p(c.off), N1, _p(best.a)))
        return dict(best=best)
    return Case("distinctive", call, desc=np.ascontiguousarray(desc),
                off=(off + lead).astype(np.int32), params=(0.6, True))


def _bf(ndb):
    rng = np.random.default_rng(507)
    q = rng.integers(0, 256, (N1, 32), dtype=np.uint8)
    db = rng.integers(0, 256, (ndb, 32), dtype=np.uint8)
    if ndb:
        db[rng.choice(ndb, 40, replace=False)] = q[:40]               # exact hits and ties
        db[7] = db[11] = q[50]

    def call(L, c):
        bi, bd, sd = Guarded(np.int32, N1), Guarded(np.int32, N1), Guarded(np.int32, N1)
        _ok(c.name, L.orbx_hamming_bf_top2(_matcher(*c.params)._h, _p(c.q), N1,
                                           _p(c.db) if len(c.db) else None, len(c.db), _p(bi.a),
                                           _p(bd.a), _p(sd.a)))
        return dict(best_idx=bi, best_dist=bd, second_dist=sd)
    return Case("bf" if ndb else "bf_ndb0", call, q=q, db=db, params=(0.6, True))


@functools.lru_cache(maxsize=None)
def case(name):
    """The case of `name` (one of NAMES or MATCHER_NAMES), built once; "remap" (its rectifier) and
    the two "tri_*" (the number of pairs) need the GPU."""
    if name in MATCHER_NAMES:
        return {"bow_kf_frame": lambda: _bow(0), "bow_kf_kf": lambda: _bow(1),
                "tri_exact": lambda: _tri(False), "tri_short": lambda: _tri(True),
                "by_sim3": _sim3, "init": _init, "distinctive": _distinctive,
                "bf": lambda: _bf(300), "bf_ndb0": lambda: _bf(0)}.get(name, lambda: _proj(name))()
    return {"undistort": _undistort, "frustum": _frustum, "project": _project,
            "unproject": _unproject, "close": _close, "rgbd_u16": lambda: _rgbd(DEPTH_U16),
            "rgbd_f32": lambda: _rgbd(DEPTH_F32), "cvt_color3": lambda: _cvt_color(3),
            "cvt_color4": lambda: _cvt_color(4), "remap": _remap, "bow_db_score": _bow_db_score}[name]()
