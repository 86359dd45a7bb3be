"""Per-frame feature arrays the matchers read (the POD view of Frame / KeyFrame).

``FeatureSet`` holds what ORBmatcher touches on a Frame or KeyFrame (src/Frame.h,
src/KeyFrame.h): mvKeysUn, mDescriptors, mvuRight, mFeatVec and mGrid.  The grid and the
FeatureVector are built here with the reference's host rules:

* ``assign_features_to_grid`` — Frame::AssignFeaturesToGrid + PosInGrid
  (src/Frame.cc:243-258, 407-417) with the cell size of Frame.cc:114-115 / 168-169 / 225-226
  (mfGridElementWidthInv = float(FRAME_GRID_COLS) / float(mnMaxX - mnMinX)).
* ``feature_vector`` — DBoW2::FeatureVector (Thirdparty/DBoW2/DBoW2/FeatureVector.cpp:31-45):
  std::map<NodeId, vector<feature index>>, features appended in extraction order.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import numpy as np

from ._lib import KEYPOINT_DTYPE

FRAME_GRID_COLS = 64   # include/Frame.h:38
FRAME_GRID_ROWS = 48   # include/Frame.h:37


def round_half_away(v) -> np.ndarray:
    """std::round on float values (half away from zero), exactly, via float64."""
    v = np.asarray(v, np.float64)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


@dataclass
class Grid:
    cols: int
    rows: int
    off: np.ndarray        # int32 [cols*rows + 1], cell c = ix*rows + iy
    feat: np.ndarray       # int32
    min_x: float
    min_y: float
    max_x: float
    max_y: float
    inv_w: float
    inv_h: float


def assign_features_to_grid(keys: np.ndarray, min_x: float, max_x: float, min_y: float,
                            max_y: float, cols: int = FRAME_GRID_COLS,
                            rows: int = FRAME_GRID_ROWS) -> Grid:
    """Frame::AssignFeaturesToGrid (src/Frame.cc:243-258) as a CSR grid."""
    f32 = np.float32
    inv_w = f32(cols) / f32(f32(max_x) - f32(min_x))
    inv_h = f32(rows) / f32(f32(max_y) - f32(min_y))
    x = np.asarray(keys["x"], f32)
    y = np.asarray(keys["y"], f32)
    px = round_half_away((x - f32(min_x)) * inv_w)     # PosInGrid, Frame.cc:409-410
    py = round_half_away((y - f32(min_y)) * inv_h)
    ok = (px >= 0) & (px < cols) & (py >= 0) & (py < rows)
    idx = np.nonzero(ok)[0]
    cell = px[idx] * rows + py[idx]
    order = np.argsort(cell, kind="stable")            # within a cell: index order
    feat = idx[order].astype(np.int32)
    counts = np.bincount(cell, minlength=cols * rows)
    off = np.zeros(cols * rows + 1, np.int32)
    np.cumsum(counts, out=off[1:])
    return Grid(cols, rows, off, feat, float(f32(min_x)), float(f32(min_y)), float(f32(max_x)),
                float(f32(max_y)), float(inv_w), float(inv_h))


@dataclass
class FeatureVector:
    node_id: np.ndarray    # uint32, ascending
    off: np.ndarray        # int32 [n_nodes + 1]
    feat: np.ndarray       # int32


def feature_vector(node_of_feature: np.ndarray) -> FeatureVector:
    """FeatureVector from the node each feature was assigned to (-1 = none)."""
    nodes = np.asarray(node_of_feature, np.int64)
    idx = np.nonzero(nodes >= 0)[0]
    order = np.argsort(nodes[idx], kind="stable")
    feat = idx[order].astype(np.int32)
    ids, counts = np.unique(nodes[idx][order], return_counts=True)
    off = np.zeros(len(ids) + 1, np.int32)
    np.cumsum(counts, out=off[1:])
    return FeatureVector(ids.astype(np.uint32), off, feat)


@dataclass
class FeatureSet:
    """mvKeysUn / mDescriptors / mvuRight / mFeatVec / mGrid of one Frame or KeyFrame."""
    keys: np.ndarray                      # KEYPOINT_DTYPE [n]
    desc: np.ndarray                      # uint8 [n, 32]
    u_right: np.ndarray | None = None     # float32 [n] (None = monocular)
    fvec: FeatureVector | None = None
    grid: Grid | None = None
    _keep: list = field(default_factory=list, repr=False)

    def __post_init__(self):
        self.keys = np.ascontiguousarray(self.keys, KEYPOINT_DTYPE)
        self.desc = np.ascontiguousarray(self.desc, np.uint8).reshape(-1, 32)
        if self.u_right is not None:
            self.u_right = np.ascontiguousarray(self.u_right, np.float32)
        if len(self.keys) != len(self.desc):
            raise ValueError("keys and descriptors differ in length")

    @property
    def n(self) -> int:
        return len(self.keys)


class FeatureSetC(ctypes.Structure):
    """orbx_featureset (include/orbx_match.h)."""
    _fields_ = [("n", ctypes.c_int32), ("keys", ctypes.c_void_p), ("desc", ctypes.c_void_p),
                ("u_right", ctypes.c_void_p), ("n_nodes", ctypes.c_int32),
                ("node_id", ctypes.c_void_p), ("node_off", ctypes.c_void_p),
                ("node_feat", ctypes.c_void_p), ("grid_cols", ctypes.c_int32),
                ("grid_rows", ctypes.c_int32), ("grid_off", ctypes.c_void_p),
                ("grid_feat", ctypes.c_void_p), ("min_x", ctypes.c_float),
                ("min_y", ctypes.c_float), ("max_x", ctypes.c_float), ("max_y", ctypes.c_float),
                ("grid_inv_w", ctypes.c_float), ("grid_inv_h", ctypes.c_float)]


def _addr(a):
    return None if a is None else a.ctypes.data


def featureset_c(fs: FeatureSet) -> FeatureSetC:
    """The C view of a FeatureSet (host pointers; `fs` must outlive the struct)."""
    s = FeatureSetC()
    s.n = fs.n
    s.keys = _addr(fs.keys)
    s.desc = _addr(fs.desc)
    s.u_right = _addr(fs.u_right)
    if fs.fvec is not None:
        s.n_nodes = len(fs.fvec.node_id)
        s.node_id, s.node_off, s.node_feat = (_addr(fs.fvec.node_id), _addr(fs.fvec.off),
                                              _addr(fs.fvec.feat))
    if fs.grid is not None:
        g = fs.grid
        s.grid_cols, s.grid_rows = g.cols, g.rows
        s.grid_off, s.grid_feat = _addr(g.off), _addr(g.feat)
        s.min_x, s.min_y, s.max_x, s.max_y = g.min_x, g.min_y, g.max_x, g.max_y
        s.grid_inv_w, s.grid_inv_h = g.inv_w, g.inv_h
    return s


PROJ_QUERY_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("radius", "<f4"),
                             ("min_level", "<i4"), ("max_level", "<i4"),
                             ("pred_level", "<i4"), ("angle", "<f4")])

# orbx_proj_mode (include/orbx_match.h)
PROJ_FRAME_MAPPOINTS = 0
PROJ_KF_SCW = 1
PROJ_LAST_FRAME = 2
PROJ_KEYFRAME = 3
PROJ_FUSE = 4
PROJ_FUSE_SCW = 5
PROJ_SIM3 = 6


# ---- Frame geometry (include/orbx_frame.h) ------------------------------------------------

def _cam(K4, dist):
    k = np.ascontiguousarray(K4, np.float32).reshape(4)
    d = np.ascontiguousarray(dist, np.float32).reshape(-1)
    if len(d) not in (4, 5, 8):
        raise ValueError("distortion needs 4, 5 or 8 coefficients")
    return k, d


def undistort_keypoints(keys: np.ndarray, K4, dist, device: int = 0) -> np.ndarray:
    """Frame::UndistortKeyPoints (src/Frame.cc:429-459) on the GPU: mvKeysUn from mvKeys."""
    from ._lib import check, load, ptr
    k, d = _cam(K4, dist)
    src = np.ascontiguousarray(keys, KEYPOINT_DTYPE)
    out = src.copy()
    check("orbx_undistort_keypoints", load().orbx_undistort_keypoints(
        ptr(k), ptr(d), len(d), ptr(src), len(src), ptr(out), device))
    return out


def image_bounds(K4, dist, width: int, height: int):
    """Frame::ComputeImageBounds (src/Frame.cc:461-489) -> (minX, maxX, minY, maxY)."""
    from ._lib import check, load, ptr
    k, d = _cam(K4, dist)
    b = np.zeros(4, np.float32)
    check("orbx_image_bounds", load().orbx_image_bounds(ptr(k), ptr(d), len(d), width, height,
                                                         ptr(b)))
    return tuple(float(v) for v in b)


def assign_grid_device(d_keys, n: int, min_x: float, max_x: float, min_y: float, max_y: float,
                       d_off, d_feat, cols: int = FRAME_GRID_COLS, rows: int = FRAME_GRID_ROWS,
                       stream: int = 0):
    """Frame::AssignFeaturesToGrid on device keypoints (torch tensors) -> fills d_off
    (cols*rows + 1) and d_feat (n)."""
    from ._lib import check, load, ptr
    f32 = np.float32
    inv_w = f32(cols) / f32(f32(max_x) - f32(min_x))
    inv_h = f32(rows) / f32(f32(max_y) - f32(min_y))
    check("orbx_assign_grid_device", load().orbx_assign_grid_device(
        ptr(d_keys), n, cols, rows, float(f32(min_x)), float(f32(min_y)), float(inv_w),
        float(inv_h), ptr(d_off), ptr(d_feat), ctypes.c_void_p(stream)))


def assign_grid_batch_device(d_keys, kp_stride: int, d_n, batch: int, bounds, d_off, d_feat,
                             cols: int = FRAME_GRID_COLS, rows: int = FRAME_GRID_ROWS,
                             stream: int = 0):
    """AssignFeaturesToGrid for `batch` frames laid out like orbx_batch_view (device
    tensors): d_off [batch][cols*rows + 1], d_feat [batch][kp_stride].  bounds =
    (min_x, max_x, min_y, max_y)."""
    from ._lib import check, load, ptr
    f32 = np.float32
    min_x, max_x, min_y, max_y = (f32(b) for b in bounds)
    inv_w = f32(cols) / f32(max_x - min_x)
    inv_h = f32(rows) / f32(max_y - min_y)
    check("orbx_assign_grid_batch_device", load().orbx_assign_grid_batch_device(
        ptr(d_keys), int(kp_stride), ptr(d_n), int(batch), cols, rows, float(min_x),
        float(min_y), float(inv_w), float(inv_h), ptr(d_off), ptr(d_feat),
        ctypes.c_void_p(stream)))
    return float(inv_w), float(inv_h)


def undistort_keypoints_batch_device(K4, dist, d_keys, kp_stride: int, d_n, batch: int,
                                     d_out, stream: int = 0):
    """Frame::UndistortKeyPoints for `batch` frames laid out like orbx_batch_view."""
    from ._lib import check, load, ptr
    k = np.ascontiguousarray(K4, np.float32)
    d = np.ascontiguousarray(dist, np.float32)
    check("orbx_undistort_keypoints_batch_device", load().orbx_undistort_keypoints_batch_device(
        ptr(k), ptr(d), len(d), ptr(d_keys), int(kp_stride), ptr(d_n), int(batch), ptr(d_out),
        ctypes.c_void_p(stream)))


def cvt_color_gray(img: np.ndarray, rgb: bool = False, device: int = 0) -> np.ndarray:
    """Tracking's colour conversion (src/Tracking.cc:189-214): cvtColor(*2GRAY) of an 8-bit
    3- or 4-channel image on the GPU (rgb=True for RGB/RGBA order, mbRGB)."""
    from ._lib import check, load, ptr
    src = np.ascontiguousarray(img, np.uint8)
    if src.ndim != 3 or src.shape[2] not in (3, 4):
        raise ValueError("expected an H x W x 3 or H x W x 4 uint8 image")
    h, w, c = src.shape
    out = np.zeros((h, w), np.uint8)
    check("orbx_cvt_color", load().orbx_cvt_color(ptr(src), w, h, w * c, c, int(rgb), ptr(out),
                                                   w, device))
    return out


# ---- Frame::isInFrustum + MapPoint::PredictScale (include/orbx_frame.h) ---------------------

# orbx_map_point: GetWorldPos, mfMinDistance, GetNormal, mfMaxDistance (32 bytes)
MAP_POINT_DTYPE = np.dtype([("pos", "<f4", 3), ("min_dist", "<f4"), ("normal", "<f4", 3),
                            ("max_dist", "<f4")])
# orbx_frame_pose: mRcw (row-major), mtcw, mOw, fx fy cx cy mbf, image bounds,
# mfLogScaleFactor, mnScaleLevels, mvScaleFactors
FRAME_POSE_DTYPE = np.dtype([("Rcw", "<f4", 9), ("tcw", "<f4", 3), ("Ow", "<f4", 3),
                             ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"),
                             ("mbf", "<f4"), ("min_x", "<f4"), ("max_x", "<f4"),
                             ("min_y", "<f4"), ("max_y", "<f4"), ("log_scale_factor", "<f4"),
                             ("nlevels", "<i4"), ("scale", "<f4", 16)])


def frame_pose(Rcw, tcw, K4, bounds, scale_factors, mbf: float = 0.0,
               scale_factor: float = 1.2) -> np.ndarray:
    """One orbx_frame_pose record from a pose (Rcw, tcw): Ow = -Rcw^T tcw (the Frame's mOw,
    Frame::UpdatePoseMatrices, Frame.cc:271-278; the caller passes its own mOw, so only its
    value matters here), mfLogScaleFactor = logf(mfScaleFactor) (Frame.cc:82; for 1.2f the
    double log rounded to float is glibc's logf value, tests/test_frustum.py)."""
    import math
    f = np.zeros((), FRAME_POSE_DTYPE)
    R = np.asarray(Rcw, np.float32).reshape(3, 3)
    t = np.asarray(tcw, np.float32).reshape(3)
    f["Rcw"] = R.reshape(9)
    f["tcw"] = t
    f["Ow"] = (-(R.astype(np.float64).T @ t.astype(np.float64))).astype(np.float32)
    f["fx"], f["fy"], f["cx"], f["cy"] = (np.float32(v) for v in np.asarray(K4, np.float32))
    f["mbf"] = np.float32(mbf)
    f["min_x"], f["max_x"], f["min_y"], f["max_y"] = (np.float32(b) for b in bounds)
    sc = np.asarray(scale_factors, np.float32)
    f["nlevels"] = len(sc)
    f["scale"][:len(sc)] = sc
    f["log_scale_factor"] = np.float32(math.log(float(np.float32(scale_factor))))
    return f


def is_in_frustum(frame: np.ndarray, mps: np.ndarray, skip=None, viewing_cos_limit: float = 0.5,
                  th: float = 1.0, device: int = 0):
    """Tracking::SearchLocalPoints' projection of one frame's local map on the GPU
    (Frame::isInFrustum + PredictScale, Frame.cc:285-349, MapPoint.cc:430-444): returns the
    SearchByProjection queries (PROJ_QUERY_DTYPE, radius -1 = not in view) and nToMatch."""
    from ._lib import check, load, ptr
    fr = np.ascontiguousarray(frame, FRAME_POSE_DTYPE).reshape(())
    m = np.ascontiguousarray(mps, MAP_POINT_DTYPE)
    sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
    q = np.zeros(len(m), PROJ_QUERY_DTYPE)
    nv = ctypes.c_int32(0)
    check("orbx_is_in_frustum", load().orbx_is_in_frustum(
        ptr(fr), ptr(m), len(m), ptr(sk), float(viewing_cos_limit), float(th), ptr(q),
        ctypes.byref(nv), device))
    return q, nv.value


def is_in_frustum_batch_device(d_frames, nframes: int, d_mps, d_mp_off, max_mps: int, d_skip,
                               d_q, d_nvisible=None, viewing_cos_limit: float = 0.5,
                               th: float = 1.0, stream: int = 0):
    """The same for `nframes` frames on device arrays (torch tensors): frame f's MapPoints at
    [d_mp_off[f], d_mp_off[f+1]) of d_mps, queries into d_q at the same indices."""
    from ._lib import check, load, ptr
    check("orbx_is_in_frustum_batch_device", load().orbx_is_in_frustum_batch_device(
        ptr(d_frames), int(nframes), ptr(d_mps), ptr(d_mp_off), int(max_mps), ptr(d_skip),
        float(viewing_cos_limit), float(th), ptr(d_q), ptr(d_nvisible), ctypes.c_void_p(stream)))


# ---- the projection loops of the other six projection modes (include/orbx_frame.h) ------------

# orbx_proj_job: the view projected into, SIM3's first transform / LAST_FRAME's last-frame pose,
# CurrentFrame.mb and bMono (LAST_FRAME), th (240 bytes)
PROJ_JOB_DTYPE = np.dtype([("cam", FRAME_POSE_DTYPE), ("pre_R", "<f4", 9), ("pre_t", "<f4", 3),
                           ("mb", "<f4"), ("th", "<f4"), ("mono", "<i4"),
                           ("reserved", "<i4", 3)])


def proj_job(cam, th: float, pre_R=None, pre_t=None, mb: float = 0.0,
             mono: bool = True) -> np.ndarray:
    """One orbx_proj_job record.  `cam` is a frame_pose record of the view projected into (the
    current Frame, the KeyFrame with Rcw / tcw / Ow decomposed from Scw, or for SIM3 Rcw = sR21,
    tcw = t21); pre_R / pre_t: SIM3's (R1w, t1w) or LAST_FRAME's (Rlw, tlw); mb / mono:
    LAST_FRAME's CurrentFrame.mb and bMono."""
    j = np.zeros((), PROJ_JOB_DTYPE)
    j["cam"] = np.asarray(cam, FRAME_POSE_DTYPE).reshape(())
    j["pre_R"] = np.eye(3, dtype=np.float32).reshape(9) if pre_R is None else \
        np.asarray(pre_R, np.float32).reshape(9)
    j["pre_t"] = 0 if pre_t is None else np.asarray(pre_t, np.float32).reshape(3)
    j["mb"], j["th"], j["mono"] = np.float32(mb), np.float32(th), int(bool(mono))
    return j


def project_map_points(mode: int, job: np.ndarray, mps: np.ndarray, src_keys=None, skip=None,
                       device: int = 0):
    """The per-MapPoint projection loop of one projection search on the GPU (k_project; every
    orbx_proj_mode but PROJ_FRAME_MAPPOINTS, which is is_in_frustum): returns the queries
    (PROJ_QUERY_DTYPE, radius -1 = rejected or skipped) and the active count.  src_keys
    (KEYPOINT_DTYPE, point i's source feature) is needed by PROJ_LAST_FRAME / PROJ_KEYFRAME."""
    from ._lib import check, load, ptr
    jb = np.ascontiguousarray(job, PROJ_JOB_DTYPE).reshape(())
    m = np.ascontiguousarray(mps, MAP_POINT_DTYPE)
    sk = None if skip is None else np.ascontiguousarray(skip, np.uint8)
    ks = None if src_keys is None else np.ascontiguousarray(src_keys, KEYPOINT_DTYPE)
    if (sk is not None and len(sk) != len(m)) or (ks is not None and len(ks) != len(m)):
        raise ValueError("one skip flag and one source keypoint per MapPoint")
    q = np.zeros(len(m), PROJ_QUERY_DTYPE)
    na = ctypes.c_int32(0)
    check("orbx_project_map_points", load().orbx_project_map_points(
        int(mode), ptr(jb), ptr(m), len(m), ptr(ks), ptr(sk), ptr(q), ctypes.byref(na), device))
    return q, na.value


def project_map_points_batch_device(mode: int, d_jobs, njobs: int, d_mps, d_mp_off, max_mps: int,
                                    d_src_keys, d_skip, d_q, d_nactive=None, stream: int = 0):
    """The same for `njobs` jobs on device arrays (torch tensors): job j's MapPoints at
    [d_mp_off[j], d_mp_off[j+1]) of d_mps, its constants in d_jobs[j] (PROJ_JOB_DTYPE), queries
    into d_q at the same indices, active counts into d_nactive[j]."""
    from ._lib import check, load, ptr
    check("orbx_project_map_points_batch_device", load().orbx_project_map_points_batch_device(
        int(mode), ptr(d_jobs), int(njobs), ptr(d_mps), ptr(d_mp_off), int(max_mps),
        ptr(d_src_keys), ptr(d_skip), ptr(d_q), ptr(d_nactive), ctypes.c_void_p(stream)))


# ---- Optimizer::PoseOptimization (include/orbx_frame.h) ----------------------------------------

# the info word of orbx_pose_optimization* (ORBX_POSEOPT_*)
POSEOPT_ROUNDS_MASK = 0x7
POSEOPT_ITERS_SHIFT, POSEOPT_ITERS_MASK = 3, 0x7f
POSEOPT_TRIALS_SHIFT, POSEOPT_TRIALS_MASK = 10, 0x1ff
POSEOPT_REFUSED_MP_INDEX = 1 << 24
POSEOPT_REFUSED_OCTAVE = 1 << 25
POSEOPT_REFUSED_NLEVELS = 1 << 26
POSEOPT_REFUSED_COUNT = 1 << 27
POSEOPT_THETA_LIMIT = 1 << 28
POSEOPT_NONPOSITIVE_SOLVE = 1 << 29
POSEOPT_FEW_EDGES = 1 << 30
POSEOPT_REFUSED_ANY = 0xf << 24


def pose_optimization(pose: np.ndarray, keys_un: np.ndarray, mp_of_feat, mps: np.ndarray,
                      u_right=None, outlier=None, device: int = 0):
    """Optimizer::PoseOptimization(&frame) on the GPU for one frame (Optimizer.cc:245-457):
    pose is the frame's FRAME_POSE_DTYPE record (mTcw, the camera, the scale table), keys_un
    mvKeysUn, mp_of_feat[i] the index into mps (MAP_POINT_DTYPE; pos is read) of feature i's
    MapPoint or -1, u_right mvuRight (None: every edge is mono), outlier mvbOutlier before the
    call (None: zeros).  Returns (pose_out, outlier, ngood, info): the record with Rcw, tcw, Ow
    replaced, mvbOutlier (written where a MapPoint is), the reference's return value and the
    POSEOPT_* info word."""
    from ._lib import check, load, ptr
    p = np.ascontiguousarray(pose, FRAME_POSE_DTYPE).reshape(())
    k = np.ascontiguousarray(keys_un, KEYPOINT_DTYPE)
    m = np.ascontiguousarray(mp_of_feat, np.int32)
    mp = np.ascontiguousarray(mps, MAP_POINT_DTYPE)
    ur = None if u_right is None else np.ascontiguousarray(u_right, np.float32)
    out = np.zeros(len(k), np.uint8) if outlier is None else \
        np.array(outlier, np.uint8, copy=True, order="C")
    if len(m) != len(k) or len(out) != len(k) or (ur is not None and len(ur) != len(k)):
        raise ValueError("per-feature arrays have one entry per keypoint")
    po = np.zeros((), FRAME_POSE_DTYPE)
    ngood, info = ctypes.c_int32(0), ctypes.c_uint32(0)
    check("orbx_pose_optimization", load().orbx_pose_optimization(
        ptr(p), ptr(k), ptr(ur), len(k), ptr(m), ptr(mp), len(mp), ptr(po), ptr(out),
        ctypes.byref(ngood), ctypes.byref(info), int(device)))
    return po, out, ngood.value, info.value


def pose_optimization_batch_device(d_poses, nframes: int, d_keys_un, d_u_right, d_feat_off,
                                   max_feat: int, d_mp_of_feat, d_mps, d_mp_off, d_poses_out,
                                   d_outlier, d_ngood, d_info, stream: int = 0):
    """The same for `nframes` frames on device arrays (torch tensors), one launch: frame f's
    features at [d_feat_off[f], d_feat_off[f+1]) of d_keys_un / d_u_right (None: mono) /
    d_mp_of_feat / d_outlier, its MapPoints at [d_mp_off[f], d_mp_off[f+1]) of d_mps;
    d_poses_out (may be d_poses), d_ngood [nframes] int32 and d_info [nframes] uint32 (int32
    tensors hold the same bits)."""
    from ._lib import check, load, ptr
    check("orbx_pose_optimization_batch_device", load().orbx_pose_optimization_batch_device(
        ptr(d_poses), int(nframes), ptr(d_keys_un), ptr(d_u_right), ptr(d_feat_off),
        int(max_feat), ptr(d_mp_of_feat), ptr(d_mps), ptr(d_mp_off), ptr(d_poses_out),
        ptr(d_outlier), ptr(d_ngood), ptr(d_info), ctypes.c_void_p(stream)))


def matches_to_features_batch_device(d_match, d_q_off, d_feat_off, njobs: int, max_q: int,
                                     max_feat: int, d_mp_of_feat, d_flagged, d_prior=None,
                                     stream: int = 0):
    """A batched projection search's d_match (the job-local feature of each query, or -1) as
    mvpMapPoints: d_mp_of_feat (the job-local query of each feature, or -1); the highest query
    wins a feature, d_prior (optional) fills the features no query names, d_flagged (one
    int32) becomes 1 when a feature index lies outside its job."""
    from ._lib import check, load, ptr
    check("orbx_matches_to_features_batch_device", load().orbx_matches_to_features_batch_device(
        ptr(d_match), ptr(d_q_off), ptr(d_feat_off), int(njobs), int(max_q), int(max_feat),
        ptr(d_prior), ptr(d_mp_of_feat), ptr(d_flagged), ctypes.c_void_p(stream)))


# ---- RGB-D frames (include/orbx_frame.h) -----------------------------------------------------

# orbx_depth_type
DEPTH_U16 = 0
DEPTH_F32 = 1
CLOSE_MAX_FEATURES = 8192   # orbx_close_points*: features per frame sorted on chip


def _depth_type(img) -> int:
    dt = img.dtype if isinstance(img, np.ndarray) else str(img.dtype).replace("torch.", "")
    if dt == np.uint16 or dt in ("uint16", "int16"):   # torch carries u16 bits in int16 too
        return DEPTH_U16
    if dt == np.float32 or dt == "float32":
        return DEPTH_F32
    raise ValueError(f"depth image of {dt}: uint16 or float32 expected")


def compute_stereo_from_rgbd(depth_img: np.ndarray, factor: float, mbf: float, keys: np.ndarray,
                             keys_un: np.ndarray | None = None, depth_type: int | None = None,
                             device: int = 0):
    """Frame::ComputeStereoFromRGBD (src/Frame.cc:689-710) with Tracking.cc:244-245's scaling on
    the sampled pixels: (mvuRight, mvDepth) from the raw depth image (H x W uint16 or float32,
    any row stride), mvKeys and mvKeysUn (None: mvKeys)."""
    from ._lib import check, load, ptr
    if depth_img.ndim != 2 or depth_img.strides[1] != depth_img.itemsize:
        raise ValueError("expected an H x W depth image with contiguous rows")
    k = np.ascontiguousarray(keys, KEYPOINT_DTYPE)
    ku = k if keys_un is None else np.ascontiguousarray(keys_un, KEYPOINT_DTYPE)
    if len(ku) != len(k):
        raise ValueError("keys and keys_un differ in length")
    h, w = depth_img.shape
    ur = np.zeros(len(k), np.float32)
    de = np.zeros(len(k), np.float32)
    t = _depth_type(depth_img) if depth_type is None else int(depth_type)
    check("orbx_compute_stereo_from_rgbd", load().orbx_compute_stereo_from_rgbd(
        ptr(depth_img), t, depth_img.strides[0], w, h, float(np.float32(factor)),
        float(np.float32(mbf)), ptr(k), ptr(ku), len(k), ptr(ur), ptr(de), device))
    return ur, de


def compute_stereo_from_rgbd_batch_device(d_depth_img, depth_type: int, row_stride: int,
                                          image_stride: int, width: int, height: int,
                                          factor: float, mbf: float, d_keys, d_keys_un,
                                          kp_stride: int, d_n, batch: int, d_u_right, d_depth,
                                          stream: int = 0):
    """The same for `batch` frames laid out like orbx_batch_view (device tensors; strides in
    bytes): fills d_u_right / d_depth [batch][kp_stride]."""
    from ._lib import check, load, ptr
    check("orbx_compute_stereo_from_rgbd_batch_device",
          load().orbx_compute_stereo_from_rgbd_batch_device(
              ptr(d_depth_img), int(depth_type), int(row_stride), int(image_stride), int(width),
              int(height), float(np.float32(factor)), float(np.float32(mbf)), ptr(d_keys),
              ptr(d_keys_un), int(kp_stride), ptr(d_n), int(batch), ptr(d_u_right), ptr(d_depth),
              ctypes.c_void_p(stream)))


def rgbd_frame_geometry_batch_device(K4, dist, d_depth_img, depth_type: int, row_stride: int,
                                     image_stride: int, width: int, height: int, factor: float,
                                     mbf: float, d_keys, kp_stride: int, d_n, batch: int,
                                     d_keys_un, d_u_right, d_depth, stream: int = 0):
    """UndistortKeyPoints + ComputeStereoFromRGBD in one launch: d_keys_un, d_u_right and
    d_depth from the raw keypoints and the raw depth images."""
    from ._lib import check, load, ptr
    k = np.ascontiguousarray(K4, np.float32)
    d = np.ascontiguousarray(dist, np.float32)
    check("orbx_rgbd_frame_geometry_batch_device", load().orbx_rgbd_frame_geometry_batch_device(
        ptr(k), ptr(d), len(d), ptr(d_depth_img), int(depth_type), int(row_stride),
        int(image_stride), int(width), int(height), float(np.float32(factor)),
        float(np.float32(mbf)), ptr(d_keys), int(kp_stride), ptr(d_n), int(batch),
        ptr(d_keys_un), ptr(d_u_right), ptr(d_depth), ctypes.c_void_p(stream)))


def unproject_stereo(frame: np.ndarray, keys: np.ndarray, depth: np.ndarray, x3d=None,
                     device: int = 0):
    """Frame::UnprojectStereo (src/Frame.cc:713-727; KeyFrame.cc:629-645 with mvKeys) for every
    feature: (x3d [n, 3], valid [n]); rows without depth keep the values of `x3d` (zeros)."""
    from ._lib import check, load, ptr
    fr = np.ascontiguousarray(frame, FRAME_POSE_DTYPE).reshape(())
    k = np.ascontiguousarray(keys, KEYPOINT_DTYPE)
    z = np.ascontiguousarray(depth, np.float32)
    out = (np.zeros((len(k), 3), np.float32) if x3d is None
           else np.ascontiguousarray(x3d, np.float32).reshape(len(k), 3).copy())
    valid = np.zeros(len(k), np.uint8)
    check("orbx_unproject_stereo", load().orbx_unproject_stereo(
        ptr(fr), ptr(k), ptr(z), len(k), ptr(out), ptr(valid), device))
    return out, valid


def unproject_stereo_batch_device(d_poses, d_keys, kp_stride: int, d_depth, d_n, batch: int,
                                  d_x3d, d_valid=None, stream: int = 0):
    """UnprojectStereo for `batch` frames on device tensors (d_x3d [batch][kp_stride][3])."""
    from ._lib import check, load, ptr
    check("orbx_unproject_stereo_batch_device", load().orbx_unproject_stereo_batch_device(
        ptr(d_poses), ptr(d_keys), int(kp_stride), ptr(d_depth), ptr(d_n), int(batch),
        ptr(d_x3d), ptr(d_valid), ctypes.c_void_p(stream)))


def close_points(frame: np.ndarray, keys: np.ndarray, depth: np.ndarray, th_depth: float,
                 has_point=None, tracked=None, min_points: int = 100, out=None,
                 device: int = 0):
    """The close-point pass of Tracking::UpdateLastFrame / CreateNewKeyFrame (src/Tracking.cc:
    862-912, 1164-1217) with NeedNewKeyFrame's counts (:1080-1089) for one frame: returns
    (order [n], counts {M, V, nTrackedClose, nNonTrackedClose}, create [n], x3d [n, 3]); only
    order[:M], create[:V] and x3d[:V] are written (`out` = (order, create, x3d) to write into)."""
    from ._lib import check, load, ptr
    fr = np.ascontiguousarray(frame, FRAME_POSE_DTYPE).reshape(())
    k = np.ascontiguousarray(keys, KEYPOINT_DTYPE)
    z = np.ascontiguousarray(depth, np.float32)
    n = len(k)
    hp = None if has_point is None else np.ascontiguousarray(has_point, np.uint8)
    tr = None if tracked is None else np.ascontiguousarray(tracked, np.uint8)
    if out is None:
        out = (np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros((n, 3), np.float32))
    order, create, x3d = out
    counts = np.zeros(4, np.int32)
    check("orbx_close_points", load().orbx_close_points(
        ptr(fr), ptr(k), ptr(z), ptr(hp), ptr(tr), n, float(np.float32(th_depth)),
        int(min_points), ptr(order), ptr(counts), ptr(create), ptr(x3d), device))
    return order, counts, create, x3d


def close_points_batch_device(d_poses, d_keys, kp_stride: int, d_depth, d_has_point, d_tracked,
                              d_n, batch: int, th_depth: float, d_order, d_counts, d_create,
                              d_x3d, min_points: int = 100, stream: int = 0):
    """The close-point pass for `batch` frames on device tensors: d_order [batch][kp_stride]
    int32, d_counts [batch][4] int32, d_create [batch][kp_stride] uint8, d_x3d
    [batch][kp_stride][3] float32; d_has_point / d_tracked may be None."""
    from ._lib import check, load, ptr
    check("orbx_close_points_batch_device", load().orbx_close_points_batch_device(
        ptr(d_poses), ptr(d_keys), int(kp_stride), ptr(d_depth), ptr(d_has_point),
        ptr(d_tracked), ptr(d_n), int(batch), float(np.float32(th_depth)), int(min_points),
        ptr(d_order), ptr(d_counts), ptr(d_create), ptr(d_x3d), ctypes.c_void_p(stream)))
