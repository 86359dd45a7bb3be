"""my_orb_slam2_amd — MI355X-native ORB front-end (ORB-SLAM2 hot path) on gfx950 HIP kernels.

Host-side mirror of the reference's operator interface for this path:

* ``ORBextractor`` — ORB_SLAM2::ORBextractor (include/ORBextractor.h:45-111)
* ``compute_stereo_matches`` — Frame::ComputeStereoMatches (src/Frame.cc:496-686)
* ``ORBmatcher`` — ORB_SLAM2::ORBmatcher descriptor matching (include/ORBmatcher.h)
* ``triangulate_matches`` / ``ORBmatcher.triangulate_matches_batch_device`` — the per-match loop of
  LocalMapping::CreateNewMapPoints behind SearchForTriangulation (src/LocalMapping.cc:356-507)
* ``pose_optimization`` / ``MonoTrackBatch.pose_optimization`` — Optimizer::PoseOptimization, the
  pose-only fit of a frame to its MapPoints (src/Optimizer.cc:245-457)
* ``Sim3Solver`` / ``ORBmatcher.sim3_iterate_batch_device`` — Horn's closed form inside the
  reference's RANSAC loop for loop-closure candidates (src/Sim3Solver.cc)
* ``OptimizeSim3`` / ``ORBmatcher.sim3_optimize_batch_device`` — Optimizer::OptimizeSim3, the
  refinement of the candidate's Sim3 over its matches (src/Optimizer.cc:1070-1265)
* ``PnPsolver`` / ``ORBmatcher.pnp_iterate_batch_device`` — EPnP inside the reference's RANSAC
  loop for relocalisation candidates (src/PnPsolver.cc), with
  ``pnp_correspondences_batch_device`` / ``pnp_apply_batch_device`` around it
* ``LocalMapView`` / ``update_local_map`` / ``MonoTrackBatch.track_local_map`` —
  Tracking::UpdateLocalMap over a CSR snapshot of the map (src/Tracking.cc:1288-1442)
* ``refresh_map_points`` / ``LocalMapView.set_refresh_inputs`` — MapPoint::UpdateNormalAndDepth and
  MapPoint::ComputeDistinctiveDescriptors over the same snapshot (src/MapPoint.cc:252-392)
* ``Vocabulary`` — ORBVocabulary / DBoW2 transform (Frame::ComputeBoW, src/Frame.cc:420-427)
* ``KeyFrameDatabase`` — ORB_SLAM2::KeyFrameDatabase candidate detection (src/KeyFrameDatabase.cc)
* ``MonoTrackBatch`` / ``RGBDTrackBatch`` — the batched monocular and RGB-D Frame front-ends
  (src/Frame.cc:132-236; ComputeStereoFromRGBD :689-710, UnprojectStereo :713-727)
* ``Rectifier`` / ``RectifiedStereoBatch`` — cv::initUndistortRectifyMap + cv::remap on raw stereo
  pairs ahead of the stereo frame (Examples/Stereo/stereo_euroc.cc:96-98, :136-137)

Everything routes through liborbx.so (include/orbx.h).  There is no CPU fallback.
"""
from __future__ import annotations

from ._lib import KEYPOINT_DTYPE, OrbxError, load
from .extractor import (ORBextractor, compute_stereo_matches, compute_stereo_matches_batch_device,
                        extract_stereo, StereoBatch)
from .matcher import (ORBmatcher, TRI_CODES, descriptor_distance, parallax_stereo_cos,
                      triangulate_matches)
from .vocabulary import Vocabulary, bow_score_l1
from .kfdb import KeyFrameDatabase
from .tracking import MonoTrackBatch, RGBDTrackBatch
from .features import (PROJ_JOB_DTYPE, PROJ_SIM3, matches_to_features_batch_device,
                       pose_optimization, pose_optimization_batch_device, proj_job,
                       project_map_points, project_map_points_batch_device)
from .pnp import (PnPsolver, pnp_iterate, pnp_job, pnp_limits, pnp_ransac_parameters,
                  pnp_sample_quads, pnp_window)
from .sim3 import (OptimizeSim3, Sim3Solver, sim3_iterate, sim3_job, sim3_limits, sim3_optimize,
                   sim3_ransac_iterations, sim3_sample_triples, sim3opt_job, sim3opt_limits)
from .localmap import (LocalMapView, local_map_search_inputs, map_arrays_from_lists,
                       refresh_map_points, refresh_map_points_host, update_local_map,
                       update_local_map_host)
from .rectify import (Rectifier, RectifiedStereoBatch, init_undistort_rectify_map,
                      load_stereo_settings, remap_fixed_point, remap_stereo_batch_device)

__all__ = ["ORBextractor", "ORBmatcher", "compute_stereo_matches", "compute_stereo_matches_batch_device",
           "extract_stereo", "descriptor_distance",
           "StereoBatch", "MonoTrackBatch", "RGBDTrackBatch", "Vocabulary", "bow_score_l1", "KeyFrameDatabase", "KEYPOINT_DTYPE", "OrbxError", "load",
           "Rectifier", "RectifiedStereoBatch", "init_undistort_rectify_map", "load_stereo_settings",
           "remap_fixed_point", "remap_stereo_batch_device",
           "PROJ_JOB_DTYPE", "PROJ_SIM3", "proj_job", "project_map_points",
           "project_map_points_batch_device", "TRI_CODES", "parallax_stereo_cos",
           "triangulate_matches", "pose_optimization", "pose_optimization_batch_device",
           "matches_to_features_batch_device", "Sim3Solver", "sim3_iterate", "sim3_job",
           "sim3_limits", "sim3_ransac_iterations", "sim3_sample_triples", "OptimizeSim3",
           "sim3_optimize", "sim3opt_job", "sim3opt_limits", "PnPsolver", "pnp_iterate", "pnp_job",
           "pnp_limits", "pnp_ransac_parameters", "pnp_sample_quads", "pnp_window", "LocalMapView",
           "local_map_search_inputs", "map_arrays_from_lists", "update_local_map",
           "update_local_map_host", "refresh_map_points", "refresh_map_points_host"]
