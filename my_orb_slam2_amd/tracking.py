"""Batched monocular tracking front-end: B frames per call, device-resident end to end.

Per frame, the reference's mono Tracking does (src/Tracking.cc):
  Frame::Frame (mono)      ExtractORB (Frame.cc:204), UndistortKeyPoints (:429-458),
                           AssignFeaturesToGrid (:243-258); image bounds once per camera
                           (ComputeImageBounds :461-489)
  SearchLocalPoints        Frame::isInFrustum + MapPoint::PredictScale on every local MapPoint
                           (Tracking.cc:1322-1335, Frame.cc:285-349, MapPoint.cc:430-444),
                           then ORBmatcher(0.8).SearchByProjection(mCurrentFrame,
                           mvpLocalMapPoints, th) (Tracking.cc:1337-1346, ORBmatcher.cc:41-136)

``MonoTrackBatch`` runs those stages for B frames on one HIP stream: one batched extraction
(orbx_extract_batch_device), one batched undistortion and grid pass (orbx_frame.h batch
forms), one batched projection of the frames' local maps (orbx_is_in_frustum_batch_device:
the pose, the MapPoints' positions, normals and distances in; the SearchByProjection queries
out) and one batched projection search (orbx_search_by_projection_batch_device) whose job j is
frame j.  ``search_local_points`` also takes ready-made queries (the caller's own projection).
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._lib import KEYPOINT_DTYPE, check
from .extractor import ORBextractor
from .features import (CLOSE_MAX_FEATURES, FRAME_GRID_COLS, FRAME_GRID_ROWS, PROJ_FRAME_MAPPOINTS,
                       PROJ_LAST_FRAME, PROJ_QUERY_DTYPE, FeatureSetC, _depth_type,
                       assign_grid_batch_device, close_points_batch_device, image_bounds,
                       is_in_frustum_batch_device, matches_to_features_batch_device,
                       pose_optimization_batch_device, project_map_points_batch_device,
                       rgbd_frame_geometry_batch_device, undistort_keypoints_batch_device)
from .localmap import local_map_search_inputs, update_local_map
from .matcher import ORBmatcher


class MonoTrackBatch:
    def __init__(self, batch: int, width: int, height: int, K4, dist, nfeatures: int = 1000,
                 scaleFactor: float = 1.2, nlevels: int = 8, iniThFAST: int = 20,
                 minThFAST: int = 7, nnratio: float = 0.8, device: int = 0):
        import torch
        self.batch, self.width, self.height = batch, width, height
        self.K4 = np.asarray(K4, np.float32)
        self.dist = np.asarray(dist, np.float32)
        self.dev = torch.device("cuda", device)
        self.ext = ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST,
                                max_batch=batch, device=device)
        self.kp_cap = self.ext.prepare(width, height, batch)
        self.matcher = ORBmatcher(nnratio, True, device=device)   # Tracking.cc:1338
        self.bounds = image_bounds(self.K4, self.dist, width, height)
        cells = FRAME_GRID_COLS * FRAME_GRID_ROWS
        kc = self.kp_cap
        self.keys_un = torch.empty(batch * kc * KEYPOINT_DTYPE.itemsize, dtype=torch.uint8,
                                   device=self.dev)
        self.grid_off = torch.empty((batch, cells + 1), dtype=torch.int32, device=self.dev)
        self.grid_feat = torch.empty((batch, kc), dtype=torch.int32, device=self.dev)
        offs = torch.arange(batch + 1, dtype=torch.int32, device=self.dev) * kc
        self.feat_off = offs            # frame j's slots [j*kp_cap, (j+1)*kp_cap)
        self.grid_pos_off = offs        # frame j's grid entries at j*kp_cap
        self.max_feat = kc
        self.njobs = batch
        self._c = None

    def _featureset(self):
        v = self.ext.batch_view()
        b = self.bounds
        inv_w = np.float32(FRAME_GRID_COLS) / np.float32(np.float32(b[1]) - np.float32(b[0]))
        inv_h = np.float32(FRAME_GRID_ROWS) / np.float32(np.float32(b[3]) - np.float32(b[2]))
        c = FeatureSetC()
        c.n = self.batch * self.kp_cap
        c.keys, c.desc, c.u_right = self.keys_un.data_ptr(), v.desc, None
        c.grid_cols, c.grid_rows = FRAME_GRID_COLS, FRAME_GRID_ROWS
        c.grid_off, c.grid_feat = self.grid_off.data_ptr(), self.grid_feat.data_ptr()
        c.min_x, c.max_x, c.min_y, c.max_y = b
        c.grid_inv_w, c.grid_inv_h = float(inv_w), float(inv_h)
        self.c = c
        return v

    def frames(self, images, stream: int = 0):
        """Frame construction for a [B, H, W] uint8 device tensor: extraction, undistortion and
        grid.  Returns the orbx_batch_view of the extraction."""
        B, H, W = images.shape
        if B != self.batch or (W, H) != (self.width, self.height):
            raise ValueError("batch shape differs from the prepared one")
        self.ext.extract_batch_device(images, stream)
        v = self._featureset()
        undistort_keypoints_batch_device(self.K4, self.dist, v.kps, self.kp_cap, v.nkp, B,
                                         self.keys_un, stream)
        assign_grid_batch_device(self.keys_un, self.kp_cap, v.nkp, B, self.bounds,
                                 self.grid_off, self.grid_feat, stream=stream)
        return v

    def search_local_points(self, d_qdesc, d_q, d_q_off, d_match, d_nmatches, d_claimed=None,
                            stream: int = 0):
        """SearchByProjection(Frame, local MapPoints) for every frame of the last ``frames``
        call: frame j's projected MapPoints at [d_q_off[j], d_q_off[j+1]) of d_q / d_qdesc;
        d_claimed (B * kp_cap bytes) marks features already matched by the motion-model
        search (mvpMapPoints set, ORBmatcher.cc:90-92)."""
        self.matcher.search_by_projection_batch_device(
            PROJ_FRAME_MAPPOINTS, self, d_qdesc, d_q, d_q_off, d_match, d_nmatches, d_claimed,
            stream=stream)

    def project_local_map(self, d_frames, d_mps, d_mp_off, max_mps: int, d_skip, d_q,
                          d_nvisible=None, th: float = 1.0, stream: int = 0):
        """SearchLocalPoints' projection loop for every frame (Tracking.cc:1322-1335): frame j's
        local MapPoints at [d_mp_off[j], d_mp_off[j+1]) of d_mps (MAP_POINT_DTYPE records),
        its pose in d_frames[j] (FRAME_POSE_DTYPE); isInFrustum(pMP, 0.5) writes the
        SearchByProjection query of each MapPoint into d_q (radius -1: not in view or d_skip
        set, i.e. bad or already matched), nToMatch into d_nvisible[j]."""
        is_in_frustum_batch_device(d_frames, self.batch, d_mps, d_mp_off, max_mps, d_skip, d_q,
                                   d_nvisible, 0.5, th, stream)

    def project_last_frame(self, d_jobs, d_mps, d_mp_off, max_mps: int, d_src_keys, d_skip, d_q,
                           d_nactive=None, stream: int = 0):
        """TrackWithMotionModel's projection loop for every frame (ORBmatcher.cc:1402-1458):
        frame j's last-frame MapPoints at [d_mp_off[j], d_mp_off[j+1]) of d_mps, the last
        frame's feature of each in d_src_keys (octave and angle are read), the job constants in
        d_jobs[j] (PROJ_JOB_DTYPE: the current pose as `cam`, the last frame's Rlw / tlw as
        pre_R / pre_t, mb, mono, th); d_skip marks slots without a MapPoint and outliers
        (:1419-1421).  Writes the SearchByProjection queries into d_q (radius -1: rejected or
        skipped) and the active count into d_nactive[j]."""
        project_map_points_batch_device(PROJ_LAST_FRAME, d_jobs, self.batch, d_mps, d_mp_off,
                                        max_mps, d_src_keys, d_skip, d_q, d_nactive, stream)

    def track_with_motion_model(self, d_jobs, d_mps, d_mp_off, max_mps: int, d_src_keys, d_skip,
                                d_q, d_qdesc, d_match, d_nmatches, d_claimed=None,
                                d_nactive=None, stream: int = 0):
        """SearchByProjection(CurrentFrame, LastFrame, th, bMono) for every frame of the last
        ``frames`` call (Tracking.cc:915-946, ORBmatcher.cc:1392-1538): ``project_last_frame``,
        then the batched LAST_FRAME search on the same stream, queries indexed like the
        MapPoints (d_mp_off).  d_match holds the frame-local feature of each MapPoint or -1; a
        mask of those features is the d_claimed ``search_local_points`` takes afterwards.
        The batched search has no per-query ORBX_QF_NO_CLAIM: temporal points without
        observations (Tracking::UpdateLastFrame) go through orbx_search_by_projection_ex
        (ORBmatcher.search_by_projection_ex) frame by frame, as before."""
        self.project_last_frame(d_jobs, d_mps, d_mp_off, max_mps, d_src_keys, d_skip, d_q,
                                d_nactive, stream)
        self.matcher.search_by_projection_batch_device(
            PROJ_LAST_FRAME, self, d_qdesc, d_q, d_mp_off, d_match, d_nmatches, d_claimed,
            stream=stream)

    _u_right = None     # the mono frames have no mvuRight: every PoseOptimization edge is mono

    def matches_to_features(self, d_match, d_q_off, max_q: int, d_mp_of_feat, d_flagged,
                            d_prior=None, stream: int = 0):
        """A batched search's d_match (frame-local feature of each MapPoint) as mvpMapPoints:
        d_mp_of_feat [B, kp_cap] int32, the index into the frame's MapPoint block of each
        feature's MapPoint or -1 (the highest query wins a feature, ORBmatcher.cc:91, :1472);
        d_prior: the MapPoints of an earlier search over the same block, kept where this one
        names none."""
        matches_to_features_batch_device(d_match, d_q_off, self.feat_off, self.batch, max_q,
                                         self.max_feat, d_mp_of_feat, d_flagged, d_prior, stream)

    def pose_optimization(self, d_poses, d_mp_of_feat, d_mps, d_mp_off, d_poses_out, d_outlier,
                          d_ngood, d_info, stream: int = 0):
        """Optimizer::PoseOptimization(&mCurrentFrame) for every frame of the last ``frames``
        call (Tracking.cc:823, :953, :1001): d_poses [B] FRAME_POSE_DTYPE records (mTcw and the
        camera), d_mp_of_feat [B, kp_cap] as ``matches_to_features`` writes it, frame j's
        MapPoints at [d_mp_off[j], d_mp_off[j+1]) of d_mps.  Writes d_poses_out (the records
        with the refined pose; may be d_poses), d_outlier [B, kp_cap] bytes (mvbOutlier, where a
        MapPoint is), d_ngood [B] and the info words d_info [B].  RGBDTrackBatch's u_right makes
        the edges of features with depth stereo."""
        pose_optimization_batch_device(d_poses, self.batch, self.keys_un, self._u_right,
                                       self.feat_off, self.max_feat, d_mp_of_feat, d_mps,
                                       d_mp_off, d_poses_out, d_outlier, d_ngood, d_info, stream)

    def track_with_motion_model_and_optimize(self, d_jobs, d_poses, d_mps, d_mp_off, max_mps: int,
                                             d_src_keys, d_skip, d_q, d_qdesc, d_match,
                                             d_nmatches, d_mp_of_feat, d_flagged, d_poses_out,
                                             d_outlier, d_ngood, d_info, d_claimed=None,
                                             d_nactive=None, stream: int = 0):
        """TrackWithMotionModel up to and including its PoseOptimization (Tracking.cc:915-953)
        on one stream with no host step: ``track_with_motion_model``, the scatter of d_match
        into d_mp_of_feat, then ``pose_optimization`` from d_poses (the records d_jobs[j].cam
        was built from).  d_poses_out is ready to be the d_frames of ``project_local_map``;
        d_outlier masks the next d_skip / d_claimed (Tracking.cc:955-975 stays with the caller)."""
        self.track_with_motion_model(d_jobs, d_mps, d_mp_off, max_mps, d_src_keys, d_skip, d_q,
                                     d_qdesc, d_match, d_nmatches, d_claimed, d_nactive, stream)
        self.matches_to_features(d_match, d_mp_off, max_mps, d_mp_of_feat, d_flagged,
                                 stream=stream)
        self.pose_optimization(d_poses, d_mp_of_feat, d_mps, d_mp_off, d_poses_out, d_outlier,
                               d_ngood, d_info, stream)

    def local_map_offsets(self, cap_mp: int):
        """d_mp_off of the blocks ``update_local_map`` writes: frame j's at j * cap_mp (a device
        tensor, made once per cap_mp: ask for it ahead of a graph capture)."""
        import torch
        if self._lm_off is None or self._lm_off[0] != cap_mp:
            off = torch.arange(self.batch + 1, dtype=torch.int32, device=self.dev) * cap_mp
            self._lm_off = (cap_mp, off)
        return self._lm_off[1]

    _lm_off = None

    def update_local_map(self, view, d_feat_mp, d_outlier, cap_kf: int, cap_mp: int, d_local_kf,
                         d_n_local_kf, d_ref_kf, d_local_mp, d_n_local_mp, d_mps, d_skip,
                         d_mp_of_feat, d_info, stream: int = 0):
        """Tracking::UpdateLocalMap for every frame of the last ``frames`` call
        (Tracking.cc:1288-1442) over the map snapshot `view` (LocalMapView): d_feat_mp
        [B, kp_cap] the MapPoint id of each feature or -1 (mvpMapPoints after
        TrackWithMotionModel), d_outlier [B, kp_cap] (or None) what ``pose_optimization`` flagged;
        d_local_kf [B, cap_kf], d_n_local_kf [B], d_ref_kf [B] in/out.  Writes d_local_mp
        [B, cap_mp], d_n_local_mp [B, 2], the block d_mps / d_skip [B, cap_mp] that
        ``project_local_map`` reads at ``local_map_offsets(cap_mp)``, d_mp_of_feat [B, kp_cap]
        (block indices) and the LOCALMAP_* words d_info [B]."""
        v = self.ext.batch_view()
        update_local_map(view, self.batch, d_feat_mp, self.kp_cap, v.nkp, d_outlier, cap_kf,
                         cap_mp, d_local_kf, d_n_local_kf, d_ref_kf, d_local_mp, d_n_local_mp,
                         d_mps, d_skip, d_mp_of_feat, d_info, stream)

    def track_local_map(self, view, d_mp_desc, d_feat_mp, d_outlier_in, cap_kf: int, cap_mp: int,
                        d_local_kf, d_n_local_kf, d_ref_kf, d_local_mp, d_n_local_mp, d_mps,
                        d_skip, d_mp_prior, d_lm_info, d_poses, d_q, d_qdesc, d_claimed, d_match,
                        d_nmatches, d_mp_of_feat, d_flagged, d_poses_out, d_outlier, d_ngood,
                        d_info, d_nvisible=None, th: float = 1.0, stream: int = 0):
        """TrackLocalMap up to and including its PoseOptimization (Tracking.cc:991-1001) on one
        stream with no host step: ``update_local_map`` (block indices into d_mp_prior), the
        block's descriptors (d_mp_desc [n_mp, 32] -> d_qdesc [B, cap_mp, 32]) and the claimed
        features (d_claimed [B, kp_cap]), ``project_local_map`` from d_poses, ``search_local_points``,
        ``matches_to_features`` with d_mp_prior as the earlier search's MapPoints (-> d_mp_of_feat),
        then ``pose_optimization`` (d_poses_out, d_outlier, d_ngood, d_info).  A frame whose
        d_lm_info has a LOCALMAP_REFUSED_ANY bit kept its old block: its results mean nothing."""
        off = self.local_map_offsets(cap_mp)
        self.update_local_map(view, d_feat_mp, d_outlier_in, cap_kf, cap_mp, d_local_kf,
                              d_n_local_kf, d_ref_kf, d_local_mp, d_n_local_mp, d_mps, d_skip,
                              d_mp_prior, d_lm_info, stream)
        local_map_search_inputs(view, d_mp_desc, self.batch, d_local_mp, d_n_local_mp, cap_mp,
                                d_mp_prior, self.kp_cap, self.ext.batch_view().nkp, d_qdesc,
                                d_claimed, stream)
        self.project_local_map(d_poses, d_mps, off, cap_mp, d_skip, d_q, d_nvisible, th, stream)
        self.search_local_points(d_qdesc, d_q, off, d_match, d_nmatches, d_claimed, stream)
        self.matches_to_features(d_match, off, cap_mp, d_mp_of_feat, d_flagged, d_mp_prior, stream)
        self.pose_optimization(d_poses, d_mp_of_feat, d_mps, off, d_poses_out, d_outlier, d_ngood,
                               d_info, stream)

    def __call__(self, images, d_qdesc, d_q, d_q_off, d_match, d_nmatches, d_claimed=None,
                 stream: int = 0, local_map=None):
        """One tracking step of the B frames.  With `local_map` = (d_frames, d_mps, max_mps,
        d_skip, d_nvisible, th) the queries d_q are first projected from the local map
        (project_local_map, MapPoints indexed like the queries: d_q_off); without it d_q
        holds the caller's projections."""
        self.frames(images, stream)
        if local_map is not None:
            d_frames, d_mps, max_mps, d_skip, d_nvis, th = local_map
            self.project_local_map(d_frames, d_mps, d_q_off, max_mps, d_skip, d_q, d_nvis, th,
                                   stream)
        self.search_local_points(d_qdesc, d_q, d_q_off, d_match, d_nmatches, d_claimed, stream)

    def fetch_undistorted(self):
        """Host copies (nkp [B], undistorted keypoints [B, kp_cap], descriptors
        [B, kp_cap, 32]) of the last ``frames`` call."""
        import torch
        torch.cuda.synchronize(self.dev)
        nkp, _, desc = self.ext.batch_fetch(0, self.batch)
        ku = self.keys_un.cpu().numpy().view(KEYPOINT_DTYPE).reshape(self.batch, self.kp_cap)
        return nkp, ku, desc


class RGBDTrackBatch(MonoTrackBatch):
    """The RGB-D front-end on top of the mono one.  Per frame, the reference's RGB-D Tracking
    adds (src/Tracking.cc:208-260, the RGB-D Frame constructor src/Frame.cc:132-184):

      imDepth.convertTo(CV_32F, mDepthMapFactor)   Tracking.cc:244-245 (applied here to the
                                                   sampled pixels, not to the image)
      Frame::ComputeStereoFromRGBD                 Frame.cc:689-710: mvuRight, mvDepth
      Frame::UnprojectStereo + the close-point pass  Frame.cc:713-727; Tracking.cc:862-912,
                                                   1164-1217 and the counts of :1080-1089

    ``frames(images, depth)`` runs the extraction, then undistortion and depth sampling in one
    launch (orbx_rgbd_frame_geometry_batch_device), then the grid; ``u_right`` / ``depth`` are
    [B, kp_cap] device tensors and the featureset carries u_right, so the projection searches
    (search_by_projection_batch_device, LAST_FRAME / FUSE) see it.  ``depth_factor`` is
    mDepthMapFactor after Tracking.cc:159-163 (already inverted: 1/5000 for TUM)."""

    def __init__(self, batch: int, width: int, height: int, K4, dist, mbf: float,
                 depth_factor: float = 1.0, th_depth: float = float("inf"), **kw):
        import torch
        super().__init__(batch, width, height, K4, dist, **kw)
        if self.kp_cap > CLOSE_MAX_FEATURES:
            raise ValueError(f"{self.kp_cap} keypoint slots per frame: the close-point pass "
                             f"sorts at most {CLOSE_MAX_FEATURES}")
        self.mbf = float(np.float32(mbf))
        self.depth_factor = float(np.float32(depth_factor))
        self.th_depth = float(np.float32(th_depth))
        kc = self.kp_cap
        f32 = dict(dtype=torch.float32, device=self.dev)
        self.u_right = torch.full((batch, kc), -1.0, **f32)
        self._u_right = self.u_right
        self.depth = torch.full((batch, kc), -1.0, **f32)
        self.order = torch.zeros((batch, kc), dtype=torch.int32, device=self.dev)
        self.counts = torch.zeros((batch, 4), dtype=torch.int32, device=self.dev)
        self.create = torch.zeros((batch, kc), dtype=torch.uint8, device=self.dev)
        self.x3d = torch.zeros((batch, kc, 3), **f32)

    def _featureset(self):
        v = super()._featureset()
        self.c.u_right = self.u_right.data_ptr()
        return v

    def frames(self, images, depth, stream: int = 0):
        """Frame construction for [B, H, W] uint8 images and their [B, H, W] raw depth maps
        (uint16 -- or int16 holding the same bits -- or float32 device tensors, rows and
        images at any stride)."""
        B, H, W = images.shape
        if B != self.batch or (W, H) != (self.width, self.height):
            raise ValueError("batch shape differs from the prepared one")
        if tuple(depth.shape) != (B, H, W) or depth.stride(2) != 1:
            raise ValueError("depth maps must be [B, H, W] with contiguous rows")
        dtype = _depth_type(depth)
        es = depth.element_size()
        self.ext.extract_batch_device(images, stream)
        v = self._featureset()
        rgbd_frame_geometry_batch_device(
            self.K4, self.dist, depth, dtype, depth.stride(1) * es, depth.stride(0) * es, W, H,
            self.depth_factor, self.mbf, v.kps, self.kp_cap, v.nkp, B, self.keys_un,
            self.u_right, self.depth, stream)
        assign_grid_batch_device(self.keys_un, self.kp_cap, v.nkp, B, self.bounds,
                                 self.grid_off, self.grid_feat, stream=stream)
        return v

    def close_points(self, d_poses, d_has_point=None, d_tracked=None, th_depth=None,
                     min_points: int = 100, stream: int = 0):
        """The close-point pass of every frame of the last ``frames`` call with the poses
        d_poses (FRAME_POSE_DTYPE records, device): fills ``order``, ``counts`` ({M, V,
        nTrackedClose, nNonTrackedClose}), ``create`` and ``x3d``.  d_has_point / d_tracked:
        [B, kp_cap] byte masks or None."""
        v = self.ext.batch_view()
        close_points_batch_device(
            d_poses, self.keys_un, self.kp_cap, self.depth, d_has_point, d_tracked, v.nkp,
            self.batch, self.th_depth if th_depth is None else th_depth, self.order,
            self.counts, self.create, self.x3d, min_points, stream)
        return self.order, self.counts, self.create, self.x3d

    def fetch_stereo(self):
        """Host copies (u_right [B, kp_cap], depth [B, kp_cap]) of the last ``frames`` call."""
        import torch
        torch.cuda.synchronize(self.dev)
        return self.u_right.cpu().numpy(), self.depth.cpu().numpy()
