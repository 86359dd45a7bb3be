"""Stereo rectification of raw pairs ahead of the stereo frame (include/orbx_frame.h).

The reference's EuRoC stereo program builds two maps once with cv::initUndistortRectifyMap
(Examples/Stereo/stereo_euroc.cc:96-98) and runs cv::remap(..., cv::INTER_LINEAR) on both
images of every frame before TrackStereo (:136-137).  Here:

* ``init_undistort_rectify_map`` / ``remap_fixed_point`` — the host helpers (no GPU needed)
* ``Rectifier`` — one camera's map on the device; ``remap`` (a host image), ``remap_batch_device``
* ``load_stereo_settings`` — LEFT / RIGHT.{K, D, R, P, width, height}, Camera.bf / Camera.fx of the
  reference's OpenCV-YAML settings files (Examples/Stereo/EuRoC.yaml)
* ``RectifiedStereoBatch`` — ``StereoBatch`` on raw pairs: both views remapped in one launch
  straight into the extractor's level-0 slots, then the resident stereo front-end
"""
from __future__ import annotations

import ctypes
import re

import numpy as np

from ._lib import check, load, ptr
from .extractor import StereoBatch


def init_undistort_rectify_map(K, dist, R, P, width: int, height: int):
    """cv::initUndistortRectifyMap(K, D, R, P, size, CV_32F, map1, map2): (map1, map2), two
    [height, width] float32 arrays.  K 3x3; dist 4, 5 or 8 coefficients; R 3x3 or None
    (identity); P 3x3 or 3x4 (its first three columns are used)."""
    K = np.ascontiguousarray(np.asarray(K, np.float64).reshape(3, 3))
    D = np.ascontiguousarray(np.asarray(dist, np.float64).reshape(-1))
    Rm = None if R is None else np.ascontiguousarray(np.asarray(R, np.float64).reshape(3, 3))
    P33 = np.ascontiguousarray(np.asarray(P, np.float64).reshape(3, -1)[:, :3])
    m1 = np.empty((height, width), np.float32)
    m2 = np.empty((height, width), np.float32)
    check("orbx_init_undistort_rectify_map", load().orbx_init_undistort_rectify_map(
        ptr(K), ptr(D), len(D), ptr(Rm), ptr(P33), width, height, ptr(m1), ptr(m2)))
    return m1, m2


def remap_fixed_point(map1, map2):
    """cv::remap's fixed-point conversion of a float map pair: (xy int16 [..., 2], a uint16 [...])
    with a = b * 32 + a (OpenCV's CV_16SC2 + CV_16UC1 layout)."""
    m1 = np.ascontiguousarray(map1, np.float32)
    m2 = np.ascontiguousarray(map2, np.float32)
    if m1.shape != m2.shape:
        raise ValueError("map1 and map2 differ in shape")
    xy = np.empty(m1.shape + (2,), np.int16)
    a = np.empty(m1.shape, np.uint16)
    check("orbx_remap_fixed_point", load().orbx_remap_fixed_point(
        ptr(m1), ptr(m2), m1.size, ptr(xy), ptr(a)))
    return xy, a


def images_per_chunk() -> int:
    """Images the remap kernel handles with one read of its map entries."""
    return int(load().orbx_remap_images_per_chunk())


class Rectifier:
    """One camera's remap (orbx_rectifier): map1 / map2 are [dst_h, dst_w] float32 maps into a
    source image of ``src_size`` = (src_w, src_h) (default: the destination size)."""

    def __init__(self, map1, map2, src_size=None, device: int = 0):
        self._h = None
        self._L = load()
        m1 = np.ascontiguousarray(map1, np.float32)
        m2 = np.ascontiguousarray(map2, np.float32)
        if m1.ndim != 2 or m1.shape != m2.shape:
            raise ValueError("map1 and map2 must be 2-D arrays of one shape")
        self.dst_h, self.dst_w = m1.shape
        self.src_w, self.src_h = src_size if src_size is not None else (self.dst_w, self.dst_h)
        self.device = device
        h = ctypes.c_void_p()
        check("orbx_rectifier_create", self._L.orbx_rectifier_create(
            ptr(m1), ptr(m2), self.dst_w, self.dst_h, self.src_w, self.src_h, device,
            ctypes.byref(h)))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.orbx_rectifier_destroy(self._h)
            self._h = None

    def remap(self, src: np.ndarray, dst: np.ndarray | None = None) -> np.ndarray:
        """One host image [src_h, src_w] uint8 (rows may be padded); returns dst [dst_h, dst_w]."""
        if src.dtype != np.uint8 or src.shape != (self.src_h, self.src_w) or src.strides[1] != 1:
            raise ValueError(f"expected a uint8 image of {self.src_h} x {self.src_w}")
        if dst is None:
            dst = np.empty((self.dst_h, self.dst_w), np.uint8)
        if dst.dtype != np.uint8 or dst.shape != (self.dst_h, self.dst_w) or dst.strides[1] != 1:
            raise ValueError(f"expected a uint8 destination of {self.dst_h} x {self.dst_w}")
        check("orbx_remap", self._L.orbx_remap(self._h, ptr(src), src.strides[0], ptr(dst),
                                               dst.strides[0]))
        return dst

    def remap_batch_device(self, src, dst, stream=None):
        """[B, src_h, src_w] -> [B, dst_h, dst_w] uint8 device tensors (unit column stride, any
        row / image strides) on `stream` (default: torch's current stream)."""
        import torch
        B = _check_batch(src, self.src_h, self.src_w)
        if _check_batch(dst, self.dst_h, self.dst_w) != B:
            raise ValueError("src and dst differ in batch")
        st = stream if stream is not None else torch.cuda.current_stream(src.device).cuda_stream
        check("orbx_remap_batch_device", self._L.orbx_remap_batch_device(
            self._h, ptr(src), src.stride(1), src.stride(0), ptr(dst), dst.stride(1),
            dst.stride(0), B, ctypes.c_void_p(st)))
        return dst


def _check_batch(t, h, w) -> int:
    import torch
    if t.dtype != torch.uint8 or t.dim() != 3 or tuple(t.shape[1:]) != (h, w) or t.stride(2) != 1:
        raise ValueError(f"expected a [B, {h}, {w}] uint8 tensor with unit column stride")
    return t.shape[0]


def remap_stereo_batch_device(r_left: Rectifier, r_right: Rectifier, src_left, src_right,
                              dst_left, dst_right, stream=None):
    """Both views of B pairs, each with its own map, in one launch
    (orbx_remap_stereo_batch_device).  Left and right tensors share their strides."""
    import torch
    B = _check_batch(src_left, r_left.src_h, r_left.src_w)
    if (_check_batch(src_right, r_right.src_h, r_right.src_w) != B or
            _check_batch(dst_left, r_left.dst_h, r_left.dst_w) != B or
            _check_batch(dst_right, r_right.dst_h, r_right.dst_w) != B):
        raise ValueError("the four tensors differ in batch")
    if src_left.stride() != src_right.stride() or dst_left.stride() != dst_right.stride():
        raise ValueError("left / right tensors need equal strides")
    st = stream if stream is not None else torch.cuda.current_stream(src_left.device).cuda_stream
    check("orbx_remap_stereo_batch_device", r_left._L.orbx_remap_stereo_batch_device(
        r_left._h, r_right._h, ptr(src_left), ptr(src_right), src_left.stride(1),
        src_left.stride(0), ptr(dst_left), ptr(dst_right), dst_left.stride(1), dst_left.stride(0),
        B, ctypes.c_void_p(st)))


# ---- the reference's settings files (OpenCV FileStorage YAML 1.0) ------------------------------
_NUM = r"[-+]?(?:\d+\.?\d*|\.\d+)(?:[eE][-+]?\d+)?"


def parse_opencv_yaml(text: str) -> dict:
    """The scalars and !!opencv-matrix entries of an OpenCV-YAML settings file: {key: float |
    str | ndarray}.  (PyYAML rejects the %YAML:1.0 header and the !!opencv-matrix tag.)"""
    out: dict = {}
    lines = [ln.split("#", 1)[0].rstrip() for ln in text.splitlines()]
    i = 0
    while i < len(lines):
        ln = lines[i]
        i += 1
        m = re.match(r"^([A-Za-z_][\w.]*)\s*:\s*(.*)$", ln)
        if not m or ln[0].isspace():
            continue
        key, val = m.group(1), m.group(2).strip()
        if val.startswith("!!opencv-matrix"):
            body = ""
            while i < len(lines) and (not lines[i] or lines[i][0].isspace()):
                body += " " + lines[i].strip()
                i += 1
            rows = int(re.search(r"rows\s*:\s*(\d+)", body).group(1))
            cols = int(re.search(r"cols\s*:\s*(\d+)", body).group(1))
            data = re.search(r"data\s*:\s*\[(.*?)\]", body).group(1)
            vals = [float(v) for v in re.findall(_NUM, data)]
            if len(vals) != rows * cols:
                raise ValueError(f"{key}: {len(vals)} values for {rows} x {cols}")
            out[key] = np.array(vals, np.float64).reshape(rows, cols)
        elif re.fullmatch(_NUM, val):
            out[key] = float(val)
        elif val:
            out[key] = val.strip('"')
    return out


def load_stereo_settings(path) -> dict:
    """{"left": {K, D, R, P, width, height}, "right": {...}, "bf", "fx"} of a stereo settings
    file with rectification entries (stereo_euroc.cc:64-94 reads the same keys)."""
    with open(path, "r", encoding="utf-8", errors="replace") as f:
        y = parse_opencv_yaml(f.read())
    res = {"bf": y["Camera.bf"], "fx": y["Camera.fx"]}
    for side, tag in (("left", "LEFT"), ("right", "RIGHT")):
        cam = {k: y[f"{tag}.{k}"] for k in ("K", "D", "R", "P")}
        cam["D"] = cam["D"].reshape(-1)
        cam["width"] = int(y[f"{tag}.width"])
        cam["height"] = int(y[f"{tag}.height"])
        res[side] = cam
    return res


class RectifiedStereoBatch(StereoBatch):
    """``StereoBatch`` for raw (unrectified) pairs: ``__call__(raw_left, raw_right, mbf, mb)``
    remaps both views with their own maps in one launch into ``input_views`` (no intermediate
    image, no copy) and runs the resident stereo front-end.  Outputs as in ``StereoBatch``."""

    def __init__(self, batch: int, rect_left: Rectifier, rect_right: Rectifier, **kw):
        if (rect_left.dst_w, rect_left.dst_h) != (rect_right.dst_w, rect_right.dst_h):
            raise ValueError("the two rectifiers differ in destination size")
        super().__init__(batch, **kw)
        self.rect_left, self.rect_right = rect_left, rect_right

    def __call__(self, raw_left, raw_right, mbf: float, mb: float, stream=None):
        if raw_left.shape[0] != self.batch:
            raise ValueError(f"expected {self.batch} pairs")
        dl, dr = self.input_views(self.rect_left.dst_w, self.rect_left.dst_h)
        remap_stereo_batch_device(self.rect_left, self.rect_right, raw_left, raw_right, dl, dr,
                                  stream)
        return self.run_resident(mbf, mb, stream)
