"""GPU: the per-frame geometry kernels of csrc/orbx_frame.hip (k_undistort / k_undistort_batch,
k_grid, k_gray, k_frustum) on the directed cases of tests/frame_cases.py, through every entry
point that can express a case -- the host forms, the _device forms and the _batch_device forms,
the latter through the wrappers of my_orb_slam2_amd.features that tracking.py calls -- bit for
bit against the plain restatements.  Records that may hold NaN are compared after
frame_cases.canon_* (float fields only: x86 and the GPU differ in the sign of the default NaN).
Every device output lies inside a sentinel-filled allocation; the guards and the slots an entry
point must leave alone are checked, and refusals are checked to write nothing."""
import ctypes

import numpy as np
import pytest

import frame_cases as fc
from my_orb_slam2_amd._lib import KEYPOINT_DTYPE
from my_orb_slam2_amd.features import (FRAME_POSE_DTYPE, MAP_POINT_DTYPE, PROJ_QUERY_DTYPE,
                                       assign_grid_batch_device, assign_grid_device, cvt_color_gray,
                                       image_bounds, is_in_frustum, is_in_frustum_batch_device,
                                       undistort_keypoints, undistort_keypoints_batch_device)

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD = 256          # sentinel bytes in front of and behind every device output
SENT = 0xA5
SENT32 = np.frombuffer(bytes([SENT] * 4), np.int32)[0]
KP = KEYPOINT_DTYPE.itemsize
PAD = 5              # MapPoint / query records in front of the first frame and behind the last


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


class Guarded:
    """`nbytes` of device memory at `offset` bytes into a sentinel-filled allocation with GUARD
    bytes of sentinel on both sides; `init` (any array) is copied in."""

    def __init__(self, nbytes, gpu, init=None, offset=0):
        import torch
        self.n, self.lo = nbytes, GUARD + offset
        self.full = torch.full((self.lo + nbytes + GUARD,), SENT, dtype=torch.uint8, device=gpu)
        self.view = self.full[self.lo:self.lo + nbytes]
        if init is not None:
            b = _bytes(init)
            assert len(b) == nbytes
            if nbytes:
                self.view.copy_(torch.from_numpy(b.copy()))

    @property
    def addr(self):
        return self.full.data_ptr() + self.lo

    def ptr(self):
        return ctypes.c_void_p(self.addr)

    def read(self, what=""):
        import torch
        torch.cuda.synchronize()
        raw = self.full.cpu().numpy()
        assert (raw[:self.lo] == SENT).all(), f"{what}: wrote in front of the buffer"
        assert (raw[self.lo + self.n:] == SENT).all(), f"{what}: wrote behind the buffer"
        return raw[self.lo:self.lo + self.n]


def _lib():
    from my_orb_slam2_amd import _lib as L
    return L.load()


def _cam_args(K4, dist):
    k = np.ascontiguousarray(K4, np.float32)
    d = np.ascontiguousarray(dist, np.float32)
    return k, d, ctypes.c_void_p(k.ctypes.data), ctypes.c_void_p(d.ctypes.data), len(d)


# ---- k_grid ---------------------------------------------------------------------------------------------

class Failures(list):
    """Every failing case of a loop, not only the first."""

    def check(self, fn, *args):
        try:
            fn(*args)
        except AssertionError as e:
            self.append(" ".join(str(e).split())[:300])

    def none(self):
        assert not self, f"{len(self)} failing case(s):\n" + "\n".join(self)


def _check_grid(c, off_raw, feat_raw, ref, what):
    off, feat, _ = ref
    got_off, got_feat = off_raw.view(np.int32), feat_raw.view(np.int32)
    np.testing.assert_array_equal(got_off, off, f"{what} {c['name']}: grid_off")
    np.testing.assert_array_equal(got_feat[:len(feat)], feat, f"{what} {c['name']}: grid_feat")
    assert (got_feat[len(feat):] == SENT32).all(), f"{what} {c['name']}: wrote past the fill"


def _run_grid_device(c, gpu):
    """orbx_assign_grid_device on one case -> (status, off bytes, feat bytes), guards checked."""
    n, ncell = len(c["keys"]), c["cols"] * c["rows"]
    keys = Guarded(max(n, 1) * KP, gpu, c["keys"] if n else np.zeros(1, KEYPOINT_DTYPE))
    off, feat = Guarded((ncell + 1) * 4, gpu), Guarded(max(n, 1) * 4, gpu)
    st = _lib().orbx_assign_grid_device(keys.ptr(), n, c["cols"], c["rows"], float(c["min_x"]),
                                        float(c["min_y"]), float(c["inv_w"]), float(c["inv_h"]),
                                        off.ptr(), feat.ptr(), None)
    return st, off.read(c["name"]), feat.read(c["name"])


def test_grid_every_case_device(orbx_lib, gpu):
    fails = Failures()
    for c in fc.grid_cases():
        st, o, f = _run_grid_device(c, gpu)
        if (c["cols"], c["rows"]) == (128, 120) and st != 0:
            # 64 KiB of dynamic LDS: a runtime that refuses the launch must be reported
            assert st == -2, st
            continue
        assert st == 0, (c["name"], st)
        fails.check(_check_grid, c, o, f, fc.grid_reference(c), "device")
    fails.none()


def test_grid_default_grid_through_the_wrappers(orbx_lib, gpu):
    """The 64 x 48 cases through features.assign_grid_device / assign_grid_batch_device, the calls
    tracking.py makes (bounds in, inverse cell sizes formed by the wrapper)."""
    import torch
    fails = Failures()
    for c in fc.grid_cases():
        if (c["cols"], c["rows"]) != (64, 48):
            continue
        n = len(c["keys"])
        keys = Guarded(max(n, 1) * KP, gpu, c["keys"] if n else np.zeros(1, KEYPOINT_DTYPE))
        off, feat = Guarded(3073 * 4, gpu), Guarded(max(n, 1) * 4, gpu)
        assign_grid_device(keys.view, n, *c["bounds"], off.view, feat.view)
        fails.check(_check_grid, c, off.read(), feat.read(), fc.grid_reference(c), "wrapper")
        d_n = torch.tensor([n], dtype=torch.int32, device=gpu)
        off, feat = Guarded(3073 * 4, gpu), Guarded(max(n, 1) * 4, gpu)
        inv = assign_grid_batch_device(keys.view, n, d_n, 1, c["bounds"], off.view, feat.view)
        assert (f32(inv[0]), f32(inv[1])) == (c["inv_w"], c["inv_h"])
        fails.check(_check_grid, c, off.read(), feat.read(), fc.grid_reference(c), "batch wrapper")
    fails.none()


def test_grid_every_case_batch_device(orbx_lib, gpu):
    """Every case as both frames of a two-frame batch with kp_stride = n + 3; the three pad slots
    of each frame hold a keypoint inside the grid (a quarter of the way in: the centre of a
    one-column grid rounds out of it), so reading one changes the result."""
    import torch
    fails = Failures()
    for c in fc.grid_cases():
        n, ncell, (mnx, mxx, mny, mxy) = len(c["keys"]), c["cols"] * c["rows"], c["bounds"]
        s = n + 3
        keys = fc.kp(np.full(2 * s, mnx + (mxx - mnx) / 4), np.full(2 * s, mny + (mxy - mny) / 4))
        assert fc.grid_np(keys[:1], c["cols"], c["rows"], c["min_x"], c["min_y"], c["inv_w"], c["inv_h"])[2]["cell"][0] >= 0
        keys[:n], keys[s:s + n] = c["keys"], c["keys"]
        d_keys = Guarded(2 * s * KP, gpu, keys)
        d_n = torch.tensor([n, n], dtype=torch.int32, device=gpu)
        off, feat = Guarded(2 * (ncell + 1) * 4, gpu), Guarded(2 * s * 4, gpu)
        st = _lib().orbx_assign_grid_batch_device(
            d_keys.ptr(), s, ctypes.c_void_p(d_n.data_ptr()), 2, c["cols"], c["rows"], float(c["min_x"]),
            float(c["min_y"]), float(c["inv_w"]), float(c["inv_h"]), off.ptr(), feat.ptr(), None)
        o, f = off.read(c["name"]), feat.read(c["name"])
        if (c["cols"], c["rows"]) == (128, 120) and st != 0:
            assert st == -2, st
            continue
        assert st == 0, (c["name"], st)
        for fr in range(2):
            fails.check(_check_grid, c, o[fr * (ncell + 1) * 4:(fr + 1) * (ncell + 1) * 4],
                        f[fr * s * 4:(fr + 1) * s * 4], fc.grid_reference(c), f"batch frame {fr}")
    fails.none()


def test_grid_batch_counts(orbx_lib, gpu):
    """d_n = [1024, 0, stride + 5, -3, 1, stride] with kp_stride 1100: a count above the stride
    is the stride, a negative one is zero; grid_feat past each frame's fill keeps its sentinel."""
    import torch
    c = fc.grid_batch_case()
    s, nf = c["stride"], len(c["d_n"])
    d_keys = Guarded(nf * s * KP, gpu, c["keys"])
    d_n = torch.from_numpy(c["d_n"].copy()).to(gpu)
    off, feat = Guarded(nf * 3073 * 4, gpu), Guarded(nf * s * 4, gpu)
    assign_grid_batch_device(d_keys.view, s, d_n, nf, c["bounds"], off.view, feat.view)
    o, f = off.read(), feat.read()
    for fr, ref in enumerate(fc.grid_batch_reference(c)):
        _check_grid(c, o[fr * 3073 * 4:(fr + 1) * 3073 * 4], f[fr * s * 4:(fr + 1) * s * 4], ref + (None,),
                    f"frame {fr}")
    assert d_keys.read().tobytes() == _bytes(c["keys"]).tobytes()


def test_grid_refusal_writes_nothing(orbx_lib, gpu):
    """121 x 127 = 15367 cells: ORBX_ERR_INVALID from both entry points, nothing written."""
    import torch
    keys = Guarded(4 * KP, gpu, fc.kp([1.0, 2.0, 3.0, 4.0], [1.0, 2.0, 3.0, 4.0]))
    off, feat = Guarded((121 * 127 + 1) * 4, gpu), Guarded(4 * 4, gpu)
    d_n = torch.tensor([4], dtype=torch.int32, device=gpu)
    L = _lib()
    assert L.orbx_assign_grid_device(keys.ptr(), 4, 121, 127, 0.0, 0.0, 0.125, 0.125, off.ptr(), feat.ptr(), None) == -1
    assert L.orbx_assign_grid_batch_device(keys.ptr(), 4, ctypes.c_void_p(d_n.data_ptr()), 1, 121, 127, 0.0, 0.0,
                                           0.125, 0.125, off.ptr(), feat.ptr(), None) == -1
    assert (off.read() == SENT).all() and (feat.read() == SENT).all()


# ---- k_undistort / k_undistort_batch ----------------------------------------------------------------------

def _same_keys(got, want, what):
    bad = np.nonzero((fc.canon_keys(got) != fc.canon_keys(want)).any(1))[0]
    assert bad.size == 0, f"{what}: keypoints differ at {bad[:8]}"


def test_undistort_every_case_host_and_device(orbx_lib, gpu):
    """Host form, _device out of place and _device in place.  x / y may be NaN or infinite
    (10^4 pixels outside, the pole of rational_pole): NaN canonised in the float fields."""
    L = _lib()
    for c in fc.undistort_cases():
        n = len(c["keys"])
        want = fc.undistort_ref(c["keys"], c["K4"], c["dist"])
        _same_keys(undistort_keypoints(c["keys"], c["K4"], c["dist"]), want, "host " + c["name"])
        k, d, pk, pd, nd = _cam_args(c["K4"], c["dist"])
        src = Guarded(max(n, 1) * KP, gpu, c["keys"] if n else np.zeros(1, KEYPOINT_DTYPE))
        dst = Guarded(n * KP, gpu)
        assert L.orbx_undistort_keypoints_device(pk, pd, nd, src.ptr(), n, dst.ptr(), None) == 0
        _same_keys(dst.read(c["name"]).view(KEYPOINT_DTYPE), want, "device " + c["name"])
        assert L.orbx_undistort_keypoints_device(pk, pd, nd, src.ptr(), n, src.ptr(), None) == 0
        got = src.read(c["name"])
        if n:
            _same_keys(got.view(KEYPOINT_DTYPE), want, "in place " + c["name"])


@pytest.mark.parametrize("cam", list(fc.UNDIST_CAMS))
def test_undistort_batch_counts(orbx_lib, gpu, cam):
    """d_n = [257, 0, stride + 5, -3, 1, stride], kp_stride 300, through the wrapper tracking.py
    calls: slots past d_n[f] keep the sentinel byte for byte, the other fields are the input's."""
    import torch
    c = fc.undistort_batch_case(cam)
    s, nf = c["stride"], len(c["d_n"])
    src = Guarded(nf * s * KP, gpu, c["keys"])
    dst = Guarded(nf * s * KP, gpu)
    d_n = torch.from_numpy(c["d_n"].copy()).to(gpu)
    undistort_keypoints_batch_device(c["K4"], c["dist"], src.view, s, d_n, nf, dst.view)
    raw = dst.read(c["name"])
    for fr, n in enumerate(c["counts"]):
        n = int(n)
        k = c["keys"][fr * s:fr * s + n]
        got = raw[fr * s * KP:(fr * s + n) * KP].view(KEYPOINT_DTYPE)
        _same_keys(got, fc.undistort_ref(k, c["K4"], c["dist"]), f"{c['name']} frame {fr}")
        for fld in ("size", "angle", "response", "octave", "class_id"):
            assert got[fld].tobytes() == k[fld].tobytes(), (fr, fld)
        assert (raw[(fr * s + n) * KP:(fr + 1) * s * KP] == SENT).all(), f"frame {fr}: wrote past d_n"
    assert src.read().tobytes() == _bytes(c["keys"]).tobytes()
    # in place: the same records, the slots past the counts still the input's
    undistort_keypoints_batch_device(c["K4"], c["dist"], src.view, s, d_n, nf, src.view)
    raw = src.read(c["name"])
    for fr, n in enumerate(c["counts"]):
        n = int(n)
        _same_keys(raw[fr * s * KP:(fr * s + n) * KP].view(KEYPOINT_DTYPE),
                   fc.undistort_ref(c["keys"][fr * s:fr * s + n], c["K4"], c["dist"]), f"in place frame {fr}")
        assert raw[(fr * s + n) * KP:(fr + 1) * s * KP].tobytes() == _bytes(c["keys"][fr * s + n:(fr + 1) * s]).tobytes()


@pytest.mark.parametrize("cam", list(fc.UNDIST_CAMS))
def test_corners_on_the_device_equal_the_host_bounds(orbx_lib, gpu, cam):
    """orbx_image_bounds undistorts the four corners on the host with the routine the kernel runs
    on the device: the device's corners, reduced as ComputeImageBounds reduces them, are the four
    returned bounds bit for bit (the two builds must not differ in contraction)."""
    K4, dist = fc.UNDIST_CAMS[cam]
    un = undistort_keypoints(fc.undistort_keys(cam, 4), K4, dist)
    assert np.isfinite(un["x"]).all() and np.isfinite(un["y"]).all()
    want = np.array(image_bounds(K4, dist, fc.WIDTH, fc.HEIGHT), np.float32)
    got = np.array(fc.bounds_from_corners(un), np.float32)
    assert got.tobytes() == want.tobytes(), (got, want)
    if cam == "copy":
        assert want.tolist() == [0.0, fc.WIDTH, 0.0, fc.HEIGHT]


# ---- k_gray ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rgb", [0, 1])
def test_gray_every_triple(orbx_lib, gpu, rgb):
    img = fc.exhaustive_image()
    np.testing.assert_array_equal(cvt_color_gray(img, bool(rgb)), fc.gray_np(img, rgb))


def _padded_rows(img, stride, offset=0):
    """The image's rows in a sentinel-filled byte buffer with `stride` bytes per row."""
    h, w, c = img.shape
    buf = np.full(offset + h * stride, SENT, np.uint8)
    for y in range(h):
        buf[offset + y * stride:offset + y * stride + w * c] = img[y].reshape(-1)
    return buf


def _check_gray_rows(raw, h, w, stride, want, what):
    rows = raw[:h * stride].reshape(h, stride)
    np.testing.assert_array_equal(rows[:, :w], want, what)
    assert (rows[:, w:] == SENT).all(), f"{what}: wrote into the row padding"


def test_gray_widths_and_strides(orbx_lib, gpu):
    """Widths around the 4-pixel thread and the 1024-pixel block, source stride w*c + 7 and
    destination stride w + 5; the device form on sub-buffers at odd byte offsets (+1 / +3).  The
    fourth channel must not influence the result: 4-channel cases run twice, alpha inverted."""
    L = _lib()
    for c in fc.gray_cases():
        img, rgb = c["img"], c["rgb"]
        h, w, ch = img.shape
        ss, ds = w * ch + 7, w + 5
        want = fc.gray_np(img, rgb)
        for im in ([img, fc.with_other_alpha(img)] if ch == 4 else [img]):
            # host form, numpy buffers with a guard row on both sides
            src = _padded_rows(im, ss)
            dst = np.full((h + 2) * ds, SENT, np.uint8)
            st = L.orbx_cvt_color(ctypes.c_void_p(src.ctypes.data), w, h, ss, ch, rgb,
                                  ctypes.c_void_p(dst.ctypes.data + ds), ds, 0)
            assert st == 0, (c["name"], st)
            assert (dst[:ds] == SENT).all() and (dst[(h + 1) * ds:] == SENT).all()
            _check_gray_rows(dst[ds:], h, w, ds, want, "host " + c["name"])
            # device form at odd offsets
            d_src = Guarded(h * ss, gpu, src, offset=1)
            d_dst = Guarded(h * ds, gpu, offset=3)
            st = L.orbx_cvt_color_device(d_src.ptr(), w, h, ss, ch, rgb, d_dst.ptr(), ds, None)
            assert st == 0, (c["name"], st)
            _check_gray_rows(d_dst.read(c["name"]), h, w, ds, want, "device " + c["name"])
            assert d_src.read().tobytes() == src.tobytes()


# ---- k_frustum --------------------------------------------------------------------------------------------------

def _same_queries(got, want, what):
    bad = np.nonzero((fc.canon_queries(got) != fc.canon_queries(want)).any(1))[0]
    assert bad.size == 0, f"{what}: queries differ at points {bad[:8]}"


def run_frustum_batch(frames, mps_list, skip_list, cos_lim, th, gpu, with_skip, with_nvisible,
                      max_mps=None):
    """One orbx_is_in_frustum_batch_device call, PAD MapPoint records in front of the first frame
    and behind the last, d_q and d_nvisible inside sentinel-filled allocations.

    On entry d_nvisible may hold anything: the entry point zeroes the nframes counters on the
    stream before the kernel adds the per-wave counts into them.  The counters are therefore
    filled with the sentinel here, not with zeros."""
    import torch
    sizes = [len(m) for m in mps_list]
    total, nf = sum(sizes), len(frames)
    off = (PAD + np.concatenate([[0], np.cumsum(sizes)])).astype(np.int32)
    mps = np.zeros(total + 2 * PAD, MAP_POINT_DTYPE)
    mps["pos"] = (0.0, 0.0, 4.0)                       # a pad record read as a MapPoint would be visible
    mps["max_dist"], mps["normal"] = 8.0, (0.0, 0.0, 1.0)
    skip = np.zeros(total + 2 * PAD, np.uint8)
    for j, m in enumerate(mps_list):
        mps[off[j]:off[j + 1]] = m
        if skip_list[j] is not None:
            skip[off[j]:off[j + 1]] = skip_list[j]
    d = lambda a: torch.from_numpy(_bytes(a).copy()).to(gpu)
    d_q = Guarded(total * 32, gpu)
    d_nv = Guarded(nf * 4, gpu)
    base_q = d_q.addr - PAD * 32                       # mp_off starts at PAD: the first query is d_q's first
    is_in_frustum_batch_device(d(np.stack(frames).astype(FRAME_POSE_DTYPE)), nf, d(mps), d(off),
                               max(sizes) if max_mps is None else max_mps, d(skip) if with_skip else None,
                               base_q, d_nv.addr if with_nvisible else None, cos_lim, th)
    q = d_q.read("d_q").view(PROJ_QUERY_DTYPE)
    nv = d_nv.read("d_nvisible").view(np.int32)
    if not with_nvisible:
        assert (nv == SENT32).all()
    return [q[off[j] - PAD:off[j + 1] - PAD] for j in range(nf)], (nv if with_nvisible else None)


def test_frustum_every_case_host_form(orbx_lib, gpu):
    for c in fc.frustum_cases():
        q_ref, n_ref, _ = fc.frustum_reference(c)
        q, n = is_in_frustum(c["F"], c["mps"], c["skip"], c["cos_lim"], c["th"])
        _same_queries(q, q_ref, c["name"])
        assert n == n_ref, c["name"]


def test_frustum_every_case_batch_device(orbx_lib, gpu):
    """The cases that share (cos_lim, th, skip given or NULL) are the frames of one batched call,
    through the wrapper tracking.py calls; once with d_nvisible and once with NULL."""
    groups = {}
    for c in fc.frustum_cases():
        groups.setdefault((c["cos_lim"], c["th"], c["skip"] is not None), []).append(c)
    assert any(not k[2] for k in groups) and any(k[2] for k in groups)
    for (cos_lim, th, has_skip), cases in groups.items():
        for with_nv in (True, False):
            qs, nv = run_frustum_batch([c["F"] for c in cases], [c["mps"] for c in cases],
                                       [c["skip"] for c in cases], cos_lim, th, gpu, has_skip, with_nv)
            for j, c in enumerate(cases):
                q_ref, n_ref, _ = fc.frustum_reference(c)
                _same_queries(qs[j], q_ref, "batch " + c["name"])
                if with_nv:
                    assert nv[j] == n_ref, c["name"]


@pytest.mark.parametrize("with_skip", [True, False])
@pytest.mark.parametrize("with_nvisible", [True, False])
def test_frustum_batch_with_empty_frames(orbx_lib, gpu, with_skip, with_nvisible):
    """Frames with 257, 0, 1, 0 and 64 MapPoints, d_skip and d_nvisible given and NULL, max_mps
    at and above the largest frame."""
    b = fc.frustum_batch_case()
    for max_mps in (None, 1000):
        qs, nv = run_frustum_batch(b["frames"], b["mps"], b["skip"], 0.5, 1.0, gpu, with_skip,
                                   with_nvisible, max_mps)
        for j, (F, m, s) in enumerate(zip(b["frames"], b["mps"], b["skip"])):
            q_ref, n_ref, _ = fc.frustum_np(F, m, s if with_skip else None)
            _same_queries(qs[j], q_ref, f"frame {j}")
            if with_nvisible:
                assert nv[j] == n_ref, j
        assert sum(len(q) for q in qs) == 322
