"""Tracking::UpdateLocalMap on the device (include/orbx_localmap.h): the CSR snapshot of the map
(``LocalMapView``) and the batched call over it (``update_local_map``).

The reference rebuilds a frame's local map between TrackWithMotionModel's pose fit and
TrackLocalMap (src/Tracking.cc:1288-1442).  ``update_local_map`` does it for every frame of a batch
in one launch and writes the MapPoint block ``MonoTrackBatch.project_local_map``,
``search_local_points``, ``matches_to_features`` and ``pose_optimization`` read, at the constant
offsets ``f * cap_mp``.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import KEYPOINT_DTYPE, MapRefreshC, MapViewC, check, load, ptr
from .features import FRAME_POSE_DTYPE, MAP_POINT_DTYPE

# d_info bits (include/orbx_localmap.h)
LOCALMAP_KEPT = 1 << 0
LOCALMAP_CAP_KF = 1 << 8
LOCALMAP_CAP_MP = 1 << 9
LOCALMAP_BAD_INDEX = 1 << 10
LOCALMAP_REFUSED_ANY = 7 << 8
LOCALMAP_MAX_KF = 131072
LOCALMAP_MAX_FEAT = 32768

# the arrays of orbx_map_view, the count each one's length gives, and the element type
_ARRAYS = (("kf_order", np.int32), ("kf_bad", np.uint8), ("kf_parent", np.int32),
           ("kf_cov_off", np.int32), ("kf_cov", np.int32), ("kf_child_off", np.int32),
           ("kf_child", np.int32), ("kf_mp_off", np.int32), ("kf_mp", np.int32),
           ("mp_bad", np.uint8), ("mp_obs_off", np.int32), ("mp_obs", np.int32),
           ("mp_rec", MAP_POINT_DTYPE))
# the arrays of orbx_map_refresh_inputs
_REFRESH_ARRAYS = (("mp_obs_feat", np.int32), ("mp_ref_kf", np.int32), ("kf_pose", FRAME_POSE_DTYPE),
                   ("kf_keys", KEYPOINT_DTYPE), ("kf_desc", np.uint8))
# what (include/orbx_localmap.h)
REFRESH_NORMAL_DEPTH = 1
REFRESH_DESCRIPTOR = 2
REFRESH_MAX_OBS = 256
# d_info of refresh_map_points
REFRESH_SKIPPED_BAD = 1 << 0
REFRESH_NO_OBS = 1 << 1
REFRESH_DESC_KEPT = 1 << 2
REFRESH_CAP_OBS = 1 << 8
REFRESH_BAD_INDEX = 1 << 10
REFRESH_REFUSED_ANY = 5 << 8

_COUNTS = (("n_kf", "kf_order"), ("n_mp", "mp_bad"), ("n_cov", "kf_cov"), ("n_child", "kf_child"),
           ("n_kfmp", "kf_mp"), ("n_obs", "mp_obs"))


def _csr(rows, n):
    rows = list(rows)
    if len(rows) != n:
        raise ValueError(f"{len(rows)} rows for {n} entries")
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum([len(r) for r in rows])
    flat = np.fromiter((x for r in rows for x in r), np.int32, int(off[-1]))
    return off, flat


def map_arrays_from_lists(kf_order, kf_bad, kf_parent, kf_cov, kf_child, kf_mp, mp_bad, mp_obs,
                          mp_rec) -> dict:
    """The arrays of orbx_map_view as numpy arrays, from plain lists: kf_order / kf_bad /
    kf_parent per keyframe slot, kf_cov / kf_child / kf_mp one list per slot (the ordered
    covisibles, the children in any order, the MapPoint id or -1 of each feature), mp_bad per
    MapPoint id, mp_obs one list of observing slots per id, mp_rec the MAP_POINT_DTYPE records.
    The children are sorted by kf_order here: the order std::set<KeyFrame*> iterates them in."""
    order = np.ascontiguousarray(kf_order, np.int32)
    n_kf = len(order)
    bad_mp = np.ascontiguousarray(mp_bad, np.uint8)
    n_mp = len(bad_mp)
    rank = [int(r) for r in order]
    a = dict(kf_order=order, kf_bad=np.ascontiguousarray(kf_bad, np.uint8),
             kf_parent=np.ascontiguousarray(kf_parent, np.int32), mp_bad=bad_mp,
             mp_rec=np.ascontiguousarray(mp_rec, MAP_POINT_DTYPE))
    a["kf_cov_off"], a["kf_cov"] = _csr(kf_cov, n_kf)
    a["kf_child_off"], a["kf_child"] = _csr(
        [sorted((int(c) for c in r), key=lambda c: rank[c] if 0 <= c < n_kf else c)
         for r in kf_child], n_kf)
    a["kf_mp_off"], a["kf_mp"] = _csr(kf_mp, n_kf)
    a["mp_obs_off"], a["mp_obs"] = _csr(mp_obs, n_mp)
    if len(a["kf_bad"]) != n_kf or len(a["kf_parent"]) != n_kf or len(a["mp_rec"]) != n_mp:
        raise ValueError("per-keyframe / per-MapPoint arrays differ in length")
    return a


def _counts(arrays) -> dict:
    n = {c: int(len(arrays[a])) for c, a in _COUNTS}
    for off, rows in (("kf_cov_off", "n_kf"), ("kf_child_off", "n_kf"), ("kf_mp_off", "n_kf"),
                      ("mp_obs_off", "n_mp")):
        if len(arrays[off]) != n[rows] + 1:
            raise ValueError(f"{off} has {len(arrays[off])} entries for {n[rows]} rows")
    for a, c in (("kf_bad", "n_kf"), ("kf_parent", "n_kf"), ("mp_rec", "n_mp")):
        if len(arrays[a]) != n[c]:
            raise ValueError(f"{a} has {len(arrays[a])} entries, expected {n[c]}")
    return n


class LocalMapView:
    """orbx_map_view on one device: the snapshot tensors (owned here, or the caller's), the C
    struct over them and the scratch of ``update_local_map``.  Build it once per map state."""

    def __init__(self, arrays: dict, device: int = 0):
        """arrays: name -> numpy array (uploaded) or device tensor (used as it is; mp_rec as
        bytes or [n_mp, 8] float32)."""
        import torch
        self.dev = torch.device("cuda", device)
        self.t = {}
        for name, dt in _ARRAYS:
            a = arrays[name]
            if isinstance(a, np.ndarray):
                a = np.ascontiguousarray(a, dt)
                raw = a.view(np.float32).reshape(-1, 8) if name == "mp_rec" else a
                a = torch.from_numpy(raw.copy()).to(self.dev)
            elif name == "mp_rec":
                a = a.reshape(-1).view(torch.float32).reshape(-1, 8)
            elif a.dtype != (torch.uint8 if dt == np.uint8 else torch.int32) or not a.is_contiguous():
                raise ValueError(f"{name}: a contiguous {np.dtype(dt).name} tensor is expected")
            self.t[name] = a
        n = _counts(self.t)
        c = MapViewC()
        for k, v in n.items():
            setattr(c, k, v)
        # a tensor of no entries has no address: every pointer of the struct must be one
        self._pad = torch.zeros(64, dtype=torch.uint8, device=self.dev)
        for name, _ in _ARRAYS:
            t = self.t[name]
            setattr(c, name, t.data_ptr() if t.numel() else self._pad.data_ptr())
        self.c = c
        self.n_kf, self.n_mp = n["n_kf"], n["n_mp"]
        self._scratch = None
        self.refresh_t, self.refresh_c = None, None      # set_refresh_inputs

    @classmethod
    def from_lists(cls, kf_order, kf_bad, kf_parent, kf_cov, kf_child, kf_mp, mp_bad, mp_obs,
                   mp_rec, device: int = 0):
        return cls(map_arrays_from_lists(kf_order, kf_bad, kf_parent, kf_cov, kf_child, kf_mp,
                                         mp_bad, mp_obs, mp_rec), device)

    def scratch_bytes(self, nframes: int, cap_kf: int, cap_mp: int) -> int:
        return int(load().orbx_update_local_map_scratch_bytes(self.n_kf, self.n_mp, int(nframes),
                                                              int(cap_kf), int(cap_mp)))

    def scratch(self, nframes: int, cap_kf: int, cap_mp: int):
        """The call's scratch, grown when needed: ask for it once ahead of a graph capture."""
        import torch
        need = max(self.scratch_bytes(nframes, cap_kf, cap_mp), 256)
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=self.dev)
        return self._scratch


    def set_refresh_inputs(self, arrays: dict):
        """The arrays ``refresh_map_points`` reads next to the view (orbx_map_refresh_inputs):
        mp_obs_feat [n_obs] and mp_ref_kf [n_mp] int32, kf_pose [n_kf] FRAME_POSE_DTYPE, kf_keys
        [n_kfmp] KEYPOINT_DTYPE, kf_desc [n_kfmp, 32] uint8 -- numpy arrays (uploaded) or device
        tensors (used as they are: int32 / bytes).  Returns self."""
        import torch
        n_obs, n_kfmp = len(self.t["mp_obs"]), len(self.t["kf_mp"])
        want = {"mp_obs_feat": 4 * n_obs, "mp_ref_kf": 4 * self.n_mp,
                "kf_pose": FRAME_POSE_DTYPE.itemsize * self.n_kf,
                "kf_keys": KEYPOINT_DTYPE.itemsize * n_kfmp, "kf_desc": 32 * n_kfmp}
        c, held = MapRefreshC(), {}
        for name, dt in _REFRESH_ARRAYS:
            a = arrays[name]
            if isinstance(a, np.ndarray):
                raw = np.ascontiguousarray(a, dt).reshape(-1).view(np.uint8)
                a = torch.from_numpy(raw.copy()).to(self.dev)
            elif not a.is_contiguous():
                raise ValueError(f"{name}: a contiguous tensor is expected")
            if a.numel() * a.element_size() != want[name]:
                raise ValueError(f"{name} holds {a.numel() * a.element_size()} bytes, expected "
                                 f"{want[name]}")
            held[name] = a
            setattr(c, name, a.data_ptr() if a.numel() else self._pad.data_ptr())
        self.refresh_t, self.refresh_c = held, c
        return self


def update_local_map(view: LocalMapView, nframes: int, d_feat_mp, feat_stride: int, d_nfeat,
                     d_outlier, cap_kf: int, cap_mp: int, d_local_kf, d_n_local_kf, d_ref_kf,
                     d_local_mp, d_n_local_mp, d_mps, d_skip, d_mp_of_feat, d_info,
                     stream: int = 0):
    """orbx_update_local_map_batch_device on device tensors: frame f's mvpMapPoints as MapPoint
    ids at d_feat_mp[f*feat_stride:], d_nfeat[f] of them, d_outlier (or None) laid out alike;
    d_local_kf [B, cap_kf], d_n_local_kf [B] and d_ref_kf [B] in/out; d_local_mp [B, cap_mp],
    d_n_local_mp [B, 2] (locals, locals + extras), the block d_mps / d_skip [B, cap_mp],
    d_mp_of_feat [B, feat_stride] and the LOCALMAP_* words d_info [B] out."""
    s = view.scratch(nframes, cap_kf, cap_mp)
    check("orbx_update_local_map_batch_device", load().orbx_update_local_map_batch_device(
        ctypes.byref(view.c), int(nframes), ptr(d_feat_mp), int(feat_stride), ptr(d_nfeat),
        ptr(d_outlier), int(cap_kf), int(cap_mp), ptr(d_local_kf), ptr(d_n_local_kf),
        ptr(d_ref_kf), ptr(d_local_mp), ptr(d_n_local_mp), ptr(d_mps), ptr(d_skip),
        ptr(d_mp_of_feat), ptr(d_info), ptr(s), s.numel(), ctypes.c_void_p(stream)))


def local_map_search_inputs(view: LocalMapView, d_mp_desc, nframes: int, d_local_mp, d_n_local_mp,
                            cap_mp: int, d_mp_of_feat, feat_stride: int, d_nfeat, d_qdesc,
                            d_claimed, stream: int = 0):
    """orbx_local_map_search_inputs_batch_device: what the projection search needs next to the
    block ``update_local_map`` wrote -- d_qdesc [B, cap_mp, 32], the descriptor (d_mp_desc
    [n_mp, 32]) of every block entry, and d_claimed [B, feat_stride], 1 where a feature holds a
    MapPoint with observations (ORBmatcher.cc:90-92)."""
    check("orbx_local_map_search_inputs_batch_device",
          load().orbx_local_map_search_inputs_batch_device(
              ctypes.byref(view.c), ptr(d_mp_desc), int(nframes), ptr(d_local_mp),
              ptr(d_n_local_mp), int(cap_mp), ptr(d_mp_of_feat), int(feat_stride), ptr(d_nfeat),
              ptr(d_qdesc), ptr(d_claimed), ctypes.c_void_p(stream)))


def refresh_map_points(view: LocalMapView, d_ids, what: int, max_obs: int, d_mp_desc, d_info,
                       d_mp_rec=None, n: int | None = None, stream: int = 0):
    """orbx_refresh_map_points_batch_device on device tensors: MapPoint::UpdateNormalAndDepth
    (REFRESH_NORMAL_DEPTH) and / or ComputeDistinctiveDescriptors (REFRESH_DESCRIPTOR) of the
    MapPoints d_ids [n] int32, in place: normal / min_dist / max_dist of d_mp_rec (the view's own
    mp_rec when None), d_mp_desc [n_mp, 32], and the REFRESH_* words d_info [n].  max_obs: no row
    of the ids is longer (a longer one is refused with REFRESH_CAP_OBS).  The view holds the extra
    arrays (``LocalMapView.set_refresh_inputs``)."""
    if view.refresh_c is None:
        raise ValueError("LocalMapView.set_refresh_inputs has not been called")
    rec = view.t["mp_rec"] if d_mp_rec is None else d_mp_rec
    check("orbx_refresh_map_points_batch_device", load().orbx_refresh_map_points_batch_device(
        ctypes.byref(view.c), ctypes.byref(view.refresh_c), ptr(d_ids),
        int(len(d_ids) if n is None else n), int(what), int(max_obs), ptr(rec), ptr(d_mp_desc),
        ptr(d_info), ctypes.c_void_p(stream)))


def refresh_map_points_host(arrays: dict, extra: dict, ids, what: int, max_obs: int, mp_desc,
                            device: int = 0) -> dict:
    """orbx_refresh_map_points: host arrays (``arrays`` as ``map_arrays_from_lists`` gives them,
    ``extra`` the arrays of ``LocalMapView.set_refresh_inputs``, mp_desc [n_mp, 32]).  Returns
    info [n], and copies of mp_rec and mp_desc as the call left them."""
    keep = {n: np.ascontiguousarray(arrays[n], dt) for n, dt in _ARRAYS}
    ex = {n: np.ascontiguousarray(extra[n], dt) for n, dt in _REFRESH_ARRAYS}
    c, r = MapViewC(), MapRefreshC()
    for k, v in _counts(keep).items():
        setattr(c, k, v)
    for n, _ in _ARRAYS:
        setattr(c, n, keep[n].ctypes.data if len(keep[n]) else None)
    for n, _ in _REFRESH_ARRAYS:
        setattr(r, n, ex[n].ctypes.data if ex[n].size else None)
    if (len(ex["mp_obs_feat"]), len(ex["mp_ref_kf"]), len(ex["kf_pose"]), len(ex["kf_keys"]),
            ex["kf_desc"].size) != (c.n_obs, c.n_mp, c.n_kf, c.n_kfmp, 32 * c.n_kfmp):
        raise ValueError("the refresh inputs do not fit the view's counts")
    ids = np.ascontiguousarray(ids, np.int32)
    rec = keep["mp_rec"].copy()
    desc = np.ascontiguousarray(mp_desc, np.uint8).copy()
    if desc.size != 32 * c.n_mp:
        raise ValueError("mp_desc holds 32 bytes per MapPoint")
    info = np.zeros(len(ids), np.uint32)
    check("orbx_refresh_map_points", load().orbx_refresh_map_points(
        ctypes.byref(c), ctypes.byref(r), ptr(ids) if len(ids) else None, len(ids), int(what),
        int(max_obs), ptr(rec) if len(rec) else None, ptr(desc) if desc.size else None,
        ptr(info) if len(ids) else None, int(device)))
    return dict(info=info, mp_rec=rec, mp_desc=desc)


def update_local_map_host(arrays: dict, feat_mp, cap_kf: int, cap_mp: int, local_kf=(),
                          ref_kf: int = -1, outlier=None, device: int = 0) -> dict:
    """orbx_update_local_map: one frame, host arrays (``map_arrays_from_lists``).  local_kf /
    ref_kf: the list and the reference keyframe before the call.  Returns info, local_kf, ref_kf,
    n_local, local_mp (the ids of the block: the locals, then the extras), mps, skip (cap_mp
    entries each) and mp_of_feat."""
    keep = {n: np.ascontiguousarray(arrays[n], dt) for n, dt in _ARRAYS}
    c = MapViewC()
    for k, v in _counts(keep).items():
        setattr(c, k, v)
    for n, _ in _ARRAYS:
        setattr(c, n, keep[n].ctypes.data if len(keep[n]) else None)
    feat = np.ascontiguousarray(feat_mp, np.int32)
    ol = None if outlier is None else np.ascontiguousarray(outlier, np.uint8)
    if ol is not None and len(ol) != len(feat):
        raise ValueError("outlier has one entry per feature")
    if len(local_kf) > cap_kf:
        raise ValueError("the list that comes in exceeds cap_kf")
    lk = np.full(cap_kf, -1, np.int32)
    lk[:len(local_kf)] = local_kf
    nlk, ref = ctypes.c_int32(len(local_kf)), ctypes.c_int32(ref_kf)
    lmp = np.full(cap_mp, -1, np.int32)
    nlmp = np.zeros(2, np.int32)
    mps, skip = np.zeros(cap_mp, MAP_POINT_DTYPE), np.zeros(cap_mp, np.uint8)
    mpf = np.full(len(feat), -1, np.int32)
    info = ctypes.c_uint32(0)
    check("orbx_update_local_map", load().orbx_update_local_map(
        ctypes.byref(c), ptr(feat), len(feat), ptr(ol), int(cap_kf), int(cap_mp), ptr(lk),
        ctypes.byref(nlk), ctypes.byref(ref), ptr(lmp), ptr(nlmp), ptr(mps), ptr(skip), ptr(mpf),
        ctypes.byref(info), int(device)))
    return dict(info=info.value, local_kf=lk[:nlk.value].copy(), ref_kf=ref.value,
                n_local=int(nlmp[0]), n_block=int(nlmp[1]), local_mp=lmp, mps=mps, skip=skip,
                mp_of_feat=mpf)
