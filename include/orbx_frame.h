/* orbx_frame.h — per-frame geometry helpers around the matchers (src/Frame.cc).
 *
 * Frame::UndistortKeyPoints (src/Frame.cc:429-459) and Frame::ComputeImageBounds (:461-489)
 * call cv::undistortPoints(points, K, DistCoef, noArgument, K).  The OpenCV 3.2 algorithm is
 * restated (modules/imgproc/src/undistort.cpp, cvUndistortPoints): normalise with 1/fx,
 * 1/fy in double, 5 fixed-point iterations of the inverse distortion (k1 k2 p1 p2 [k3 [k4 k5
 * k6]]), re-project with P = K, store as float.  PARITY UNPINNED against the real OpenCV
 * (absent from this image); bit-exact between GPU and the CPU restatement.
 * K is passed as (fx, fy, cx, cy): the reference's K is diag(fx, fy, 1) with (cx, cy) in the
 * last column (Tracking.cc:56-64).
 */
#ifndef ORBX_FRAME_H
#define ORBX_FRAME_H

#include "orbx.h"
#include "orbx_match.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mvKeysUn from mvKeys: a copy when dist[0] == 0 (Frame.cc:431-435), else every keypoint's
 * pt undistorted (other fields copied).  ndist: 4, 5 or 8. */
orbx_status orbx_undistort_keypoints(const float* K4, const float* dist, int32_t ndist,
                                     const orbx_keypoint* kps, int32_t n,
                                     orbx_keypoint* kps_un, int device);
/* Same on device keypoints (n entries, in place allowed), on the caller's stream. */
orbx_status orbx_undistort_keypoints_device(const float* K4, const float* dist, int32_t ndist,
                                            const orbx_keypoint* d_kps, int32_t n,
                                            orbx_keypoint* d_kps_un, void* stream);
/* Frame::ComputeImageBounds: bounds = (mnMinX, mnMaxX, mnMinY, mnMaxY). */
orbx_status orbx_image_bounds(const float* K4, const float* dist, int32_t ndist, int32_t width,
                              int32_t height, float* bounds);

/* Frame::AssignFeaturesToGrid (Frame.cc:243-258, PosInGrid :407-417) on device keypoints:
 * grid_off (cols*rows + 1) and grid_feat (n; features outside the grid are dropped) in the
 * orbx_featureset layout (cell c = ix*rows + iy, indices ascending within a cell). */
orbx_status orbx_assign_grid_device(const orbx_keypoint* d_kps, int32_t n, int32_t cols,
                                    int32_t rows, float min_x, float min_y, float inv_w,
                                    float inv_h, int32_t* d_grid_off, int32_t* d_grid_feat,
                                    void* stream);

/* Batched forms for frames laid out like orbx_batch_view (frame f's keypoints at
 * d_kps + f*kp_stride, d_n[f] of them, device counts).  Grid: frame f's grid_off block at
 * d_grid_off + f*(cols*rows+1), its grid_feat (frame-local indices) at
 * d_grid_feat + f*kp_stride.  Undistort: slots past d_n[f] are left untouched. */
orbx_status orbx_assign_grid_batch_device(const orbx_keypoint* d_kps, int32_t kp_stride,
                                          const int32_t* d_n, int32_t batch, int32_t cols,
                                          int32_t rows, float min_x, float min_y, float inv_w,
                                          float inv_h, int32_t* d_grid_off,
                                          int32_t* d_grid_feat, void* stream);
orbx_status orbx_undistort_keypoints_batch_device(const float* K4, const float* dist,
                                                  int32_t ndist, const orbx_keypoint* d_kps,
                                                  int32_t kp_stride, const int32_t* d_n,
                                                  int32_t batch, orbx_keypoint* d_kps_un,
                                                  void* stream);

/* ---- Frame::isInFrustum + MapPoint::PredictScale (Tracking::SearchLocalPoints' projection of
 * the local map, src/Tracking.cc:1297-1335; src/Frame.cc:285-349; src/MapPoint.cc:394-444) ----
 *
 * One MapPoint as isInFrustum reads it: GetWorldPos(), GetNormal(), and mfMinDistance /
 * mfMaxDistance (the invariance limits 0.8f * min and 1.2f * max are applied here,
 * MapPoint.cc:394-404).  32 bytes. */
typedef struct {
    float pos[3];
    float min_dist;
    float normal[3];
    float max_dist;
} orbx_map_point;

/* A frame's pose and camera as isInFrustum reads them: mRcw (row-major 3x3), mtcw, mOw,
 * fx fy cx cy, mbf, the image bounds (mnMinX, mnMaxX, mnMinY, mnMaxY), mvScaleFactors (nlevels
 * entries) and mfLogScaleFactor (= logf(mfScaleFactor), Frame.cc:82).  The projection query
 * of a MapPoint in view is the one SearchByProjection(Frame&, vpMapPoints, th) builds from
 * mTrackProjX / mTrackProjY / mTrackProjXR / mnTrackScaleLevel / mTrackViewCos
 * (ORBmatcher.cc:46-80). */
typedef struct orbx_frame_pose {
    float Rcw[9];
    float tcw[3];
    float Ow[3];
    float fx, fy, cx, cy, mbf;
    float min_x, max_x, min_y, max_y;
    float log_scale_factor;
    int32_t nlevels;
    float scale[16];
} orbx_frame_pose;

/* For every MapPoint i of every frame f (frame f's MapPoints at [d_mp_off[f], d_mp_off[f+1])
 * of d_mps, d_mp_off on the device): isInFrustum(pMP, viewing_cos_limit) with
 *   Pc = mRcw*P + mtcw as OpenCV 3.2's cv::gemm small-matrix path evaluates it (float
 *        products and sums, + tcw in double, rounded to float),
 *   dist = cv::norm(P - mOw) (squares summed in double, sqrt, float),
 *   viewCos = (P - mOw).dot(normal) / dist (double), rounded to float,
 *   level = PredictScale: ceilf(logf(max_dist / dist) / mfLogScaleFactor) clamped to
 *           [0, nlevels - 1] (glibc 2.35 logf, restated bit for bit, orbx_math.h),
 * and, when in view, the SearchByProjection query d_q[i] = {u, v, ur = u - mbf*invz,
 * radius = RadiusByViewingCos(viewCos) [* th if th != 1] * scale[level], level - 1, level,
 * level, 0}; not in view (or d_skip[i] != 0: the MapPoint is bad or already matched in this
 * frame, Tracking.cc:1316-1320): radius = -1 (the matcher skips it).  d_nvisible[f] (optional)
 * = nToMatch, the frame's MapPoints in view.  max_mps >= every frame's MapPoint count. */
orbx_status orbx_is_in_frustum_batch_device(const orbx_frame_pose* d_frames, int32_t nframes,
                                            const orbx_map_point* d_mps,
                                            const int32_t* d_mp_off, int32_t max_mps,
                                            const uint8_t* d_skip, float viewing_cos_limit,
                                            float th, orbx_proj_query* d_q,
                                            int32_t* d_nvisible, void* stream);
/* One frame, host arrays (copied to the device for the call). */
orbx_status orbx_is_in_frustum(const orbx_frame_pose* frame, const orbx_map_point* mps,
                               int32_t n, const uint8_t* skip, float viewing_cos_limit,
                               float th, orbx_proj_query* q, int32_t* nvisible, int device);

/* ---- The per-MapPoint projection loop of the other six projection searches (orbx_proj_mode
 * LAST_FRAME :1402-1458, KEYFRAME :1544-1596, KF_SCW :321-390, FUSE :881-946, FUSE_SCW :1035-1105,
 * SIM3 :1166-1247 / :1284-1327 of src/ORBmatcher.cc) ----
 *
 * One job's constants.  cam: the view projected into -- the current Frame (LAST_FRAME, KEYFRAME),
 * the KeyFrame (KF_SCW, FUSE, FUSE_SCW; for the Scw modes Rcw / tcw / Ow already decomposed from
 * Scw as ORBmatcher.cc:1042-1046 does once per call), or for SIM3 Rcw = sR21, tcw = t21 (Ow
 * unused) with the target keyframe's intrinsics, bounds and scale tables.  pre_R / pre_t: SIM3's
 * first transform (R1w, t1w); LAST_FRAME's last-frame pose (Rlw, tlw); otherwise unused.  mb /
 * mono: LAST_FRAME only (CurrentFrame.mb, bMono).  th: the search window factor.  240 bytes. */
typedef struct {
    orbx_frame_pose cam;
    float pre_R[9];
    float pre_t[3];
    float mb;
    float th;
    int32_t mono;
    int32_t reserved[3];
} orbx_proj_job;

/* For every MapPoint i of every job j (job j's MapPoints at [d_mp_off[j], d_mp_off[j+1]) of
 * d_mps, queries written at the same indices of d_q), the projection the reference's loop of
 * `mode` computes, in its types and order (all jobs of a call share the mode):
 *   Pc     = cam.Rcw*P + cam.tcw in cv::gemm's small-matrix form (as orbx_is_in_frustum); SIM3:
 *            of P1 = pre_R*P + pre_t
 *   depth  LAST_FRAME: invz < 0 rejects (after invz); KEYFRAME: no test; others: Pc.z < 0 rejects
 *   invz   KF_SCW, FUSE: 1.0f / z; others: (float)(1.0 / (double)z)
 *   u, v   LAST_FRAME, KEYFRAME: (fx*xc)*invz + cx with the Frame bounds (u < min_x || u > max_x
 *          rejects, so NaN passes); others: x = xc*invz, fx*x + cx with KeyFrame::IsInImage
 *          (u >= min_x && u < max_x, so NaN fails)
 *   d      (float)cv::norm(P - cam.Ow) (SIM3: of Pc; LAST_FRAME: none), d < 0.8f*min_dist ||
 *          d > 1.2f*max_dist rejects; KF_SCW, FUSE, FUSE_SCW: (P - Ow).dot(normal) < 0.5*d in
 *          double rejects
 *   level  L = PredictScale(d) on the raw max_dist (as orbx_is_in_frustum); LAST_FRAME:
 *          L = d_src_keys[i].octave, an octave outside [0, cam.nlevels) gives an inactive query
 *          (the reference indexes mvScaleFactors unchecked)
 *   query  {u, v, ur, th*scale[L], min_level, max_level, L, angle}: ur = u - mbf*invz for
 *          LAST_FRAME and FUSE, else 0; levels (L-1, L+1) for KEYFRAME and for LAST_FRAME unless
 *          forward (L, -1) or backward (0, L), else (-1, -1); angle = d_src_keys[i].angle for
 *          LAST_FRAME and KEYFRAME, else 0.  LAST_FRAME per job: tlc.z = row 2 of pre_R*cam.Ow +
 *          pre_t (gemm form), forward = tlc.z > mb && !mono, backward = -tlc.z > mb && !mono.
 * Rejected, or d_skip[i] != 0 (no MapPoint, outlier, bad, already found, IsInKeyFrame): the
 * inactive query {0, 0, 0, -1, -1, -1, -1, 0}.  A job whose cam.nlevels is outside [1, 16] gets
 * inactive queries only.  d_nactive[j] (optional) = job j's active queries.  d_src_keys (point
 * i's source feature; octave and angle are read) is required for LAST_FRAME and KEYFRAME.
 * max_mps >= every job's MapPoint count; the MapPoints of a call number at most 1 << 24.
 * d_mps and d_q are read and written as 16-byte accesses: a base that is not 16-byte aligned
 * is ORBX_ERR_INVALID.  mode outside the six (ORBX_PROJ_FRAME_MAPPOINTS is orbx_is_in_frustum*): ORBX_ERR_INVALID. */
orbx_status orbx_project_map_points_batch_device(
    int32_t mode, const orbx_proj_job* d_jobs, int32_t njobs, const orbx_map_point* d_mps,
    const int32_t* d_mp_off, int32_t max_mps, const orbx_keypoint* d_src_keys,
    const uint8_t* d_skip, orbx_proj_query* d_q, int32_t* d_nactive, void* stream);
/* One job, host arrays (copied to the device for the call).  The argument checks run before the
 * device is touched; without a GPU: ORBX_ERR_DEVICE. */
orbx_status orbx_project_map_points(int32_t mode, const orbx_proj_job* job,
                                    const orbx_map_point* mps, int32_t n,
                                    const orbx_keypoint* src_keys, const uint8_t* skip,
                                    orbx_proj_query* q, int32_t* nactive, int device);

/* ---- Optimizer::PoseOptimization (src/Optimizer.cc:245-457; called at Tracking.cc:823, :953,
 * :1001 and :1564-1603): the pose-only fit of a frame to its MapPoints ----
 *
 * One edge per feature i with a MapPoint (d_mp_of_feat[i] >= 0, an index into the frame's block
 * [d_mp_off[f], d_mp_off[f+1]) of d_mps), in feature order: mono when d_u_right is NULL or
 * d_u_right[i] < 0, else stereo; observation d_keys_un[i].x / .y (and d_u_right[i]) widened to
 * double, information 1.0f / (scale[octave] * scale[octave]) of the pose record's scale table,
 * Huber deltas (float)sqrt(5.991) / (float)sqrt(7.815), camera fx fy cx cy mbf of the record.
 * g2o's single-vertex Levenberg-Marquardt is restated as it runs there (four rounds of
 * optimize(10) from the input pose, at most 10 trials per iteration, the 1e-5 tau, the 1/3..2/3
 * crop, the three-in-a-row stop; errors are not recomputed after a rejected trial; edges classified
 * by `(float)chi2 > 5.991f / 7.815f`; the kernel dropped for the fourth round; a frame with fewer
 * than 10 edges runs one round).  H, b and chi2 are summed edge by edge in edge order.  Forms
 * evaluated inside Eigen (Quaterniond(Matrix3d), quaternion * vector, the pivoted LDLT) are
 * restated from the published algorithms [unverified-Eigen]; sin / cos are the library's own
 * fdlibm-style routine, defined for theta <= 2^20: no bit-equality with a g2o build is claimed,
 * the GPU equals the two CPU restatements of tests/ bit for bit.
 *
 * Per frame f: d_outlier[i] (mvbOutlier, indexed like the features) is written for every feature
 * with a MapPoint and for no other; d_ngood[f] = nInitialCorrespondences - nBad (0 with fewer than
 * 3 edges, the pose then copied through); d_poses_out[f] = d_poses[f] with Rcw, tcw (the optimised
 * SE3Quat's matrix rounded to float, Converter.cc:49-71) and Ow (-Rcw^T tcw as cv::gemm's
 * small-matrix form: float products summed left to right) replaced.  d_poses_out may be d_poses.
 * d_info[f]: */
#define ORBX_POSEOPT_ROUNDS_MASK 0x7u            /* bits 0-2: rounds run (0-4) */
#define ORBX_POSEOPT_ITERS_SHIFT 3               /* bits 3-9: Levenberg iterations (solve calls), <= 40 */
#define ORBX_POSEOPT_ITERS_MASK 0x7fu
#define ORBX_POSEOPT_TRIALS_SHIFT 10             /* bits 10-18: Levenberg trials (linear solves), <= 400 */
#define ORBX_POSEOPT_TRIALS_MASK 0x1ffu
#define ORBX_POSEOPT_REFUSED_MP_INDEX (1u << 24) /* a MapPoint index < -1 or outside the block */
#define ORBX_POSEOPT_REFUSED_OCTAVE (1u << 25)   /* a matched feature's octave outside [0, nlevels) */
#define ORBX_POSEOPT_REFUSED_NLEVELS (1u << 26)  /* nlevels outside [1, 16] */
#define ORBX_POSEOPT_REFUSED_COUNT (1u << 27)    /* more than max_feat features (or a negative count) */
#define ORBX_POSEOPT_THETA_LIMIT (1u << 28)      /* an update's |omega| above 2^20 or not finite: that trial failed */
#define ORBX_POSEOPT_NONPOSITIVE_SOLVE (1u << 29) /* LDLT::isPositive() was false in some trial */
#define ORBX_POSEOPT_FEW_EDGES (1u << 30)        /* fewer than 3 edges: returned 0 */
#define ORBX_POSEOPT_REFUSED_ANY (0xfu << 24)
/* A refused frame (what only the device can see): nothing of it is read further, d_ngood[f] = 0,
 * the pose is copied through and the flags are untouched.  A frame's features: [d_feat_off[f],
 * d_feat_off[f+1]) of d_keys_un / d_u_right / d_mp_of_feat / d_outlier.
 * ORBX_ERR_INVALID: a NULL required pointer when nframes > 0; nframes < 0 or > 65535; max_feat
 * outside [0, 32768].  nframes == 0: ORBX_OK, nothing touched.  Without a GPU: ORBX_ERR_DEVICE. */
orbx_status orbx_pose_optimization_batch_device(
    const orbx_frame_pose* d_poses, int32_t nframes, const orbx_keypoint* d_keys_un,
    const float* d_u_right, const int32_t* d_feat_off, int32_t max_feat,
    const int32_t* d_mp_of_feat, const orbx_map_point* d_mps, const int32_t* d_mp_off,
    orbx_frame_pose* d_poses_out, uint8_t* d_outlier, int32_t* d_ngood, uint32_t* d_info,
    void* stream);
/* One frame, host arrays (copied to the device for the call): n features, nmp MapPoints.
 * outlier is read (the flags before the call) and written; info may be NULL.  The argument checks
 * run before the device is touched (ORBX_ERR_INVALID: a NULL pose, pose_out or ngood, n outside
 * [0, 32768], nmp < 0, a NULL array that n or nmp makes required); without a GPU: ORBX_ERR_DEVICE. */
orbx_status orbx_pose_optimization(const orbx_frame_pose* pose, const orbx_keypoint* keys_un,
                                   const float* u_right, int32_t n, const int32_t* mp_of_feat,
                                   const orbx_map_point* mps, int32_t nmp,
                                   orbx_frame_pose* pose_out, uint8_t* outlier, int32_t* ngood,
                                   uint32_t* info, int device);

/* A batched projection search's d_match (per query / MapPoint q of job j, the job-local feature
 * or -1; queries [d_q_off[j], d_q_off[j+1])) turned into mvpMapPoints: d_mp_of_feat (per feature
 * of job j, [d_feat_off[j], d_feat_off[j+1]), the job-local query index or -1).  Two queries
 * naming one feature: the highest query index wins, the "later match overwrites" of
 * ORBmatcher.cc:91, :1472.  d_prior (optional, laid out like d_mp_of_feat, not the same memory):
 * a feature no query names keeps d_prior's entry, i.e. d_prior is copied in and the scatter
 * overwrites it (TrackLocalMap sees the MapPoints of both searches when both index one block).
 * A feature index outside the job's features is skipped and *d_flagged (one device word, zeroed
 * by the call) becomes 1.  max_q / max_feat: at least every job's query / feature count. */
orbx_status orbx_matches_to_features_batch_device(const int32_t* d_match, const int32_t* d_q_off,
                                                  const int32_t* d_feat_off, int32_t njobs,
                                                  int32_t max_q, int32_t max_feat,
                                                  const int32_t* d_prior, int32_t* d_mp_of_feat,
                                                  uint32_t* d_flagged, void* stream);

/* Tracking's colour input (src/Tracking.cc:189-214): cv::cvtColor(*2GRAY) for 3- or 4-channel
 * 8-bit images, OpenCV 3.2's integer path RGB2Gray<uchar> (Y = (R*4899 + G*9617 + B*1868 +
 * 8192) >> 14).  rgb = 1 for RGB/RGBA order (mbRGB), 0 for BGR/BGRA.  OpenCV builds with IPP
 * may route BGR2GRAY through ippiColorToGray instead: PARITY UNPINNED against the library. */
orbx_status orbx_cvt_color_device(const uint8_t* d_src, int32_t width, int32_t height,
                                  size_t src_stride, int32_t channels, int32_t rgb,
                                  uint8_t* d_dst, size_t dst_stride, void* stream);
orbx_status orbx_cvt_color(const uint8_t* src, int32_t width, int32_t height, size_t src_stride,
                           int32_t channels, int32_t rgb, uint8_t* dst, size_t dst_stride,
                           int device);

/* ---- RGB-D frames (System::RGBD): depth at the keypoints, unprojection, the close-point pass ----
 *
 * The raw depth image as the sensor delivers it; Tracking::GrabImageRGBD scales it to CV_32F
 * (src/Tracking.cc:244-245) with mDepthMapFactor, here `factor`: the value after
 * Tracking.cc:159-163, i.e. already inverted (1.0f / 5000 for TUM). */
typedef enum {
    ORBX_DEPTH_U16 = 0, /* CV_16U: d = (float)raw * factor (cvtScale_<ushort, float, float>) */
    ORBX_DEPTH_F32 = 1  /* CV_32F: d = raw * factor when fabs(factor - 1.0f) > 1e-5, else raw */
} orbx_depth_type;

/* Frame::ComputeStereoFromRGBD (src/Frame.cc:689-710) with the depth scaling in front of it
 * (Tracking.cc:244-245) applied to the sampled pixels only: for every keypoint slot i < d_n[f] of
 * frame f (layout of orbx_batch_view), d = the depth image of frame f (at d_depth +
 * f*image_stride bytes, rows row_stride bytes apart) at row (int)kps[i].y, column (int)kps[i].x
 * (C++ truncation, x86 cvttss2si for NaN / out of range); d > 0: d_depth_out[i] = d,
 * d_u_right[i] = kps_un[i].x - mbf / d; otherwise (0, -0.0f, negative, NaN) both are -1.  A
 * pixel outside [0, width) x [0, height) gives -1 / -1 (the reference reads out of bounds).
 * Slots past d_n[f] are left untouched.  d_kps_un may equal d_kps.  Depth types other than
 * orbx_depth_type's: ORBX_ERR_UNSUPPORTED. */
orbx_status orbx_compute_stereo_from_rgbd_batch_device(
    const void* d_depth, int32_t depth_type, size_t row_stride, size_t image_stride,
    int32_t width, int32_t height, float factor, float mbf, const orbx_keypoint* d_kps,
    const orbx_keypoint* d_kps_un, int32_t kp_stride, const int32_t* d_n, int32_t batch,
    float* d_u_right, float* d_depth_out, void* stream);
/* One frame, host arrays (copied to the device for the call). */
orbx_status orbx_compute_stereo_from_rgbd(const void* depth, int32_t depth_type,
                                          size_t row_stride, int32_t width, int32_t height,
                                          float factor, float mbf, const orbx_keypoint* kps,
                                          const orbx_keypoint* kps_un, int32_t n,
                                          float* u_right, float* depth_out, int device);
/* The same fused with Frame::UndistortKeyPoints (Frame.cc:429-459): one launch and one read of
 * each keypoint; d_kps_un is written too (a copy when dist[0] == 0; in place allowed).  Outputs
 * are bitwise those of orbx_undistort_keypoints_batch_device followed by the call above. */
orbx_status orbx_rgbd_frame_geometry_batch_device(
    const float* K4, const float* dist, int32_t ndist, const void* d_depth, int32_t depth_type,
    size_t row_stride, size_t image_stride, int32_t width, int32_t height, float factor,
    float mbf, const orbx_keypoint* d_kps, int32_t kp_stride, const int32_t* d_n, int32_t batch,
    orbx_keypoint* d_kps_un, float* d_u_right, float* d_depth_out, void* stream);

/* Frame::UnprojectStereo (src/Frame.cc:713-727) / KeyFrame::UnprojectStereo (src/KeyFrame.cc:
 * 629-645) for every slot i < d_n[f]: z = d_depth[i] > 0: x = ((u - cx) * z) * invfx, y likewise
 * (invfx = 1.0f / fx), d_x3d[3i..] = Rwc * (x, y, z) + Ow in cv::gemm's small-matrix form (float
 * products summed left to right, + Ow in double, rounded to float), Rwc the transpose of
 * d_poses[f].Rcw; d_valid[i] (optional) = 1.  z <= 0: d_valid[i] = 0, the point is untouched.
 * d_keys: mvKeysUn for a Frame, mvKeys for a KeyFrame. */
orbx_status orbx_unproject_stereo_batch_device(const orbx_frame_pose* d_poses,
                                               const orbx_keypoint* d_keys, int32_t kp_stride,
                                               const float* d_depth, const int32_t* d_n,
                                               int32_t batch, float* d_x3d, uint8_t* d_valid,
                                               void* stream);
orbx_status orbx_unproject_stereo(const orbx_frame_pose* pose, const orbx_keypoint* keys,
                                  const float* depth, int32_t n, float* x3d, uint8_t* valid,
                                  int device);

/* The close-point pass Tracking::UpdateLastFrame (src/Tracking.cc:862-912) and
 * Tracking::CreateNewKeyFrame (:1164-1217) both write, with NeedNewKeyFrame's close counts
 * (:1076-1092), one workgroup per frame.  d_has_point[i] (optional; absent = none): slot i holds
 * a MapPoint with Observations() >= 1.  d_tracked[i] (optional; absent = none):
 * mvpMapPoints[i] && !mvbOutlier[i].  Per frame f (arrays indexed like the keypoints):
 *   d_order[j], j < M      the slots with z > 0 in ascending (z, index) order: std::sort on
 *                          vector<pair<float,int>>
 *   d_counts[4f..]         {M, V, nTrackedClose, nNonTrackedClose}: M = #{z > 0}; V = the sorted
 *                          entries the loop body runs on before its break (z > th_depth &&
 *                          nPoints > min_points; the reference's min_points is 100); the close
 *                          counts take 0 < z < th_depth
 *   d_create[j], j < V     !has_point[order[j]] (bCreateNew)
 *   d_x3d[3j..], j < V     UnprojectStereo(order[j])
 * Entries past M (order) and V (create, x3d) are untouched.  th_depth = +inf gives V = M
 * (StereoInitialization, Tracking.cc:570-585, takes every z > 0).  kp_stride (n for the host
 * form) above 8192: ORBX_ERR_UNSUPPORTED. */
orbx_status orbx_close_points_batch_device(const orbx_frame_pose* d_poses,
                                           const orbx_keypoint* d_keys, int32_t kp_stride,
                                           const float* d_depth, const uint8_t* d_has_point,
                                           const uint8_t* d_tracked, const int32_t* d_n,
                                           int32_t batch, float th_depth, int32_t min_points,
                                           int32_t* d_order, int32_t* d_counts,
                                           uint8_t* d_create, float* d_x3d, void* stream);
orbx_status orbx_close_points(const orbx_frame_pose* pose, const orbx_keypoint* keys,
                              const float* depth, const uint8_t* has_point,
                              const uint8_t* tracked, int32_t n, float th_depth,
                              int32_t min_points, int32_t* order, int32_t* counts,
                              uint8_t* create, float* x3d, int device);

/* ---- Stereo rectification of raw pairs (Examples/Stereo/stereo_euroc.cc:96-98 builds the two
 * maps with cv::initUndistortRectifyMap, :136-137 run cv::remap(..., cv::INTER_LINEAR) on both
 * images of every frame before TrackStereo; Examples/ROS/ORB_SLAM2/src/ros_stereo.cc:106-107,
 * 161-162 likewise) ----
 *
 * OpenCV 3.2's algorithms restated (modules/imgproc/src/undistort.cpp, imgwarp.cpp): PARITY
 * UNPINNED against the library; bit-exact between the GPU, these host helpers and the numpy
 * restatement of tests/remap_cases.py.
 *
 * cv::initUndistortRectifyMap(K, D, R, P(:, :3), size, CV_32F, map1, map2)
 * (stereo_euroc.cc:96-98), host only, in double as written (no contraction): iR = (P33 * R)^-1
 * by the 3x3 closed form, then per pixel the forward distortion k1 k2 p1 p2 [k3 [k4 k5 k6]] of
 * the normalised ray.  K, R, P33 row-major 3x3; R9_or_null == NULL: identity; ndist 4, 5 or 8
 * (12 / 14, the thin-prism and tilt terms: ORBX_ERR_UNSUPPORTED); map1 / map2 width*height
 * floats. */
orbx_status orbx_init_undistort_rectify_map(const double K[9], const double* dist, int32_t ndist,
                                            const double* R9_or_null, const double P33[9],
                                            int32_t width, int32_t height, float* map1,
                                            float* map2);
/* cv::remap's conversion of a CV_32FC1 map pair to fixed point (stereo_euroc.cc:136-137, the
 * first step of remap INTER_LINEAR), host only: sx = cvRound(map1 * 32.0f) (float product, x86
 * cvtss2si: half to even, NaN / out of range INT_MIN), xy[2i] = saturate_cast<short>(sx >> 5),
 * a[i] = (sy & 31) * 32 + (sx & 31); the layout of OpenCV's CV_16SC2 + CV_16UC1 maps. */
orbx_status orbx_remap_fixed_point(const float* map1, const float* map2, size_t n, int16_t* xy,
                                   uint16_t* a);

/* One camera's map on the device (dst_w x dst_h entries from map1 / map2, tightly packed rows),
 * converted at create time for a source of src_w x src_h pixels.  Immutable after create and
 * usable from several threads.  src_w or src_h above 32767 (the short saturation):
 * ORBX_ERR_UNSUPPORTED; without a GPU: ORBX_ERR_DEVICE. */
typedef struct orbx_rectifier orbx_rectifier;
orbx_status orbx_rectifier_create(const float* map1, const float* map2, int32_t dst_w,
                                  int32_t dst_h, int32_t src_w, int32_t src_h, int device,
                                  orbx_rectifier** out);
orbx_status orbx_rectifier_destroy(orbx_rectifier* r);

/* cv::remap(src 8UC1, dst, map1, map2, cv::INTER_LINEAR) with BORDER_CONSTANT 0
 * (stereo_euroc.cc:136-137) on `batch` device images (image i at base + i*image_stride, rows
 * row_stride bytes apart): dst = (sum of the four taps times their 5-bit weight products + 512)
 * >> 10, taps outside the source 0.  Any base address, any row stride >= width; src and dst must
 * not overlap; bytes of a destination row past dst_w are left untouched.  Rows of one image
 * spanning 4 GiB or more: ORBX_ERR_UNSUPPORTED. */
orbx_status orbx_remap_batch_device(const orbx_rectifier* r, const uint8_t* d_src,
                                    size_t src_row_stride, size_t src_image_stride,
                                    uint8_t* d_dst, size_t dst_row_stride,
                                    size_t dst_image_stride, int32_t batch, void* stream);
/* Both views of `batch` pairs, each with its own map, in one launch (stereo_euroc.cc:136-137;
 * ros_stereo.cc:161-162); the strides are shared by the two sides.  Rectifiers of different
 * destination size or on different devices: ORBX_ERR_INVALID. */
orbx_status orbx_remap_stereo_batch_device(
    const orbx_rectifier* r_left, const orbx_rectifier* r_right, const uint8_t* d_src_left,
    const uint8_t* d_src_right, size_t src_row_stride, size_t src_image_stride,
    uint8_t* d_dst_left, uint8_t* d_dst_right, size_t dst_row_stride, size_t dst_image_stride,
    int32_t batch, void* stream);
/* One host image (copied to the device for the call), stereo_euroc.cc:136. */
orbx_status orbx_remap(const orbx_rectifier* r, const uint8_t* src, size_t src_stride,
                       uint8_t* dst, size_t dst_stride);
/* Images a lane of the remap kernel handles with one read of its map entries. */
int32_t orbx_remap_images_per_chunk(void);

/* ---- PnPsolver's neighbours in Tracking::Relocalization (orbx_match.h, orbx_pnp_*) ---------- */

/* The solvers' correspondences from the matches of orbx_search_by_bow_kf_frame_batch_device, one
 * workgroup per job, an ordered compaction: for every frame feature i < n_feat (ascending) with
 * m = d_match[j * match_stride + i] >= 0, the record {i, d_mps[d_mp_off[j] + m].pos, d_kp[i].x,
 * d_kp[i].y, d_kp[i].octave} is appended to d_corr[j * corr_stride ..], and d_N[j] receives their
 * number.  A match outside job j's block [0, d_mp_off[j + 1] - d_mp_off[j]) is dropped and sets
 * bit 0 of d_N_flags[j] when d_N_flags is not NULL.  n_feat <= corr_stride.
 * ORBX_ERR_INVALID: m NULL, a NULL array with njobs > 0, a negative count, n_feat above a stride.
 * njobs == 0: ORBX_OK, nothing touched. */
orbx_status orbx_pnp_correspondences_batch_device(
    orbx_matcher* m, int32_t njobs, const int32_t* d_match, int64_t match_stride,
    const orbx_keypoint* d_kp, int32_t n_feat, const orbx_map_point* d_mps,
    const int32_t* d_mp_off, orbx_pnp_corr* d_corr, int64_t corr_stride, int32_t* d_N,
    int32_t* d_N_flags, void* stream);

/* Tracking.cc:1546-1562 for njobs candidates: for a found job j (d_results[j].found),
 * d_poses[j] = *d_template with Rcw / tcw from Tcw and Ow = -Rcw.t() * tcw in PoseOptimization's
 * form, and d_mp_of_feat[j * feat_stride + i] = inlier[i] ? d_match[j * match_stride + i] : -1
 * for i < n_feat with inlier = d_inliers[d_jobs[j].inlier_off ..]; otherwise d_poses[j] =
 * *d_template and every entry is -1.  A job whose inlier block lies outside [0, ninlier_bytes) or
 * whose n_matches differs from n_feat is treated as not found.
 * ORBX_ERR_INVALID: m NULL, a NULL array with njobs > 0, a negative count, n_feat above a stride.
 * njobs == 0: ORBX_OK, nothing touched. */
orbx_status orbx_pnp_apply_batch_device(
    orbx_matcher* m, int32_t njobs, const orbx_pnp_job* d_jobs, const orbx_pnp_result* d_results,
    const uint8_t* d_inliers, int64_t ninlier_bytes, const int32_t* d_match, int64_t match_stride,
    int32_t n_feat, const orbx_frame_pose* d_template, orbx_frame_pose* d_poses,
    int32_t* d_mp_of_feat, int64_t feat_stride, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_FRAME_H */
