"""The nine per-frame host-array entry points (orbx_undistort_keypoints, orbx_is_in_frustum,
orbx_project_map_points, orbx_unproject_stereo, orbx_close_points, orbx_compute_stereo_from_rgbd,
orbx_cvt_color, orbx_remap, orbx_bow_db_score) on one tiny case each, called straight through the C
ABI so that the caller's output arrays can sit inside sentinel-filled allocations: 64 guard bytes
on both sides, padded rows, slots the call does not document as written.

    c = case("frustum")      # the inputs, built once and never modified
    r = c.call()             # {"name": Guarded or a scalar}: fresh outputs, one call

The sentinel tests next to each entry point's GPU tests check `r` against that entry point's
restatement; tests/test_gpu_concurrency.py compares `r` across threads."""
import ctypes
import functools

import numpy as np

from my_orb_slam2_amd import synth
from my_orb_slam2_amd._lib import KEYPOINT_DTYPE
from my_orb_slam2_amd.features import (DEPTH_F32, DEPTH_U16, MAP_POINT_DTYPE, PROJ_LAST_FRAME,
                                       PROJ_QUERY_DTYPE)

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


@functools.lru_cache(maxsize=None)
def case(name):
    """The case of `name` (one of NAMES), built once; "remap" needs the GPU (its rectifier)."""
    return {"undistort": _undistort, "frustum": _frustum, "project": _project,
            "unproject": _unproject, "close": _close, "rgbd_u16": lambda: _rgbd(DEPTH_U16),
            "rgbd_f32": lambda: _rgbd(DEPTH_F32), "cvt_color3": lambda: _cvt_color(3),
            "cvt_color4": lambda: _cvt_color(4), "remap": _remap, "bow_db_score": _bow_db_score}[name]()
