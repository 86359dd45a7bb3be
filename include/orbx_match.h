/* orbx_match.h — C ABI of the descriptor matchers (replaces ORB_SLAM2::ORBmatcher).
 *
 * The reference class is include/ORBmatcher.h:37-128 / src/ORBmatcher.cc.  Its methods read
 * Frame / KeyFrame / MapPoint objects; this boundary takes the plain arrays those objects
 * hold instead, so a thin C++ facade can keep the reference signatures:
 *
 *   orbx_featureset  = the per-frame arrays a matcher reads: mvKeysUn, mDescriptors,
 *                      mvuRight, mFeatVec (DBoW2::FeatureVector, as CSR) and mGrid (as CSR).
 *   "valid" / "has_mp" / "claimed" masks = the MapPoint* arrays reduced to the one bit each
 *                      method tests (non-NULL and !isBad(), Observations()>0, ...).
 *   orbx_proj_query  = the projection of one MapPoint (u, v, ur, radius, levels), computed by
 *                      the caller with the reference's own cv::Mat code, as SURVEY §8(b) puts
 *                      the boundary; the window search, Hamming distances, greedy claims and
 *                      rotation-consistency filter run on the GPU.
 *
 * Outputs are feature indices (-1 = no match); the facade turns them back into MapPoint*.
 * Every function returns the reference method's return value in *nmatches.  All host-pointer
 * entry points copy their inputs to the device, run on a stream of their own and wait.
 * Functions named *_device take device pointers and run on the caller's stream.
 *
 * A matcher handle is not re-entrant (its device workspace is reused); use one per thread,
 * as the reference's Tracking / LocalMapping / LoopClosing threads each own their ORBmatcher.
 * A host-pointer call reports ORBX_ERR_CAPACITY from a word of its own: it neither clears nor
 * reads the flag that *_device calls on the same handle leave for orbx_matcher_sync.
 */
#ifndef ORBX_MATCH_H
#define ORBX_MATCH_H

#include "orbx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* src/ORBmatcher.cc:37-39 */
enum { ORBX_TH_HIGH = 100, ORBX_TH_LOW = 50, ORBX_HISTO_LENGTH = 30 };

/* One Frame or KeyFrame as seen by the matchers.  Feature i has keys[i] (mvKeysUn: pt,
 * octave and angle are read), desc + 32*i (mDescriptors row i) and u_right[i] (mvuRight;
 * NULL = every feature monocular, i.e. -1).
 * FeatureVector (Thirdparty/DBoW2/DBoW2/FeatureVector.h): node j has id node_id[j] (strictly
 * ascending, the std::map order) and features node_feat[node_off[j] .. node_off[j+1]) in the
 * order DBoW2 pushed them; every feature index appears in at most one node (transform()
 * adds each feature to exactly one node, FeatureVector.cpp:31-45).
 * Grid (Frame::mGrid / KeyFrame::mGrid): cell (ix, iy) = grid_feat[grid_off[c] ..
 * grid_off[c+1]) with c = ix*grid_rows + iy, indices in AssignFeaturesToGrid order
 * (Frame.cc:243-258); min_x/min_y/max_x/max_y = mnMinX.., grid_inv_w/h =
 * mfGridElementWidthInv / mfGridElementHeightInv.  Grid fields are only read by the
 * projection searches and may be zero/NULL elsewhere. */
typedef struct {
    int32_t n;
    const orbx_keypoint* keys;
    const uint8_t* desc;
    const float* u_right;
    int32_t n_nodes;
    const uint32_t* node_id;
    const int32_t* node_off;
    const int32_t* node_feat;
    int32_t grid_cols, grid_rows;
    const int32_t* grid_off;
    const int32_t* grid_feat;
    float min_x, min_y, max_x, max_y;
    float grid_inv_w, grid_inv_h;
} orbx_featureset;

typedef struct {
    float nnratio;              /* ORBmatcher(nnratio, ...) default 0.6       */
    int32_t check_orientation;  /* ORBmatcher(..., checkOri) default true     */
    int32_t device;             /* HIP device ordinal                         */
} orbx_matcher_params;

typedef struct orbx_matcher orbx_matcher;

/* ORBmatcher::ORBmatcher (src/ORBmatcher.cc:41-43). */
orbx_status orbx_matcher_create(const orbx_matcher_params* params, orbx_matcher** out);
orbx_status orbx_matcher_destroy(orbx_matcher* m);

/* ORBmatcher::ComputeThreeMaxima (src/ORBmatcher.cc:1669-1710) on bin counts histo[L]
 * (host, no device work). */
void orbx_compute_three_maxima(const int32_t* histo, int32_t L, int32_t* ind1, int32_t* ind2,
                               int32_t* ind3);

/* ORBmatcher::SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&) (src/ORBmatcher.cc:182-319).
 * kf_valid[i] = pKF->GetMapPointMatches()[i] && !isBad().  match_f[n_f]: for each frame
 * feature, the keyframe feature whose MapPoint it received (vpMapPointMatches), or -1. */
orbx_status orbx_search_by_bow_kf_frame(orbx_matcher* m, const orbx_featureset* kf,
                                        const uint8_t* kf_valid, const orbx_featureset* f,
                                        int32_t* match_f, int32_t* nmatches);

/* ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vector<MapPoint*>&) (:563-696).
 * valid1/valid2 as above; match12[n1] = KF2 feature matched to each KF1 feature or -1. */
orbx_status orbx_search_by_bow_kf_kf(orbx_matcher* m, const orbx_featureset* kf1,
                                     const uint8_t* valid1, const orbx_featureset* kf2,
                                     const uint8_t* valid2, int32_t* match12, int32_t* nmatches);

/* ORBmatcher::SearchForTriangulation (:702-872) + CheckDistEpipolarLine (:147-167).
 * has_mp1/has_mp2[i] = GetMapPoint(i) != NULL.  F12: row-major 3x3 (F12.at<float>(r,c) =
 * F12[3r+c]).  (ex, ey): the epipole the reference computes at :709-715.  sigma2_2 /
 * scale_2: pKF2->mvLevelSigma2 / mvScaleFactors (nlevels).  pairs: (idx1, idx2) in idx1
 * order, up to pair_cap pairs (ORBX_ERR_CAPACITY if more; *nmatches = the count). */
orbx_status orbx_search_for_triangulation(orbx_matcher* m, const orbx_featureset* kf1,
                                          const uint8_t* has_mp1, const orbx_featureset* kf2,
                                          const uint8_t* has_mp2, const float* F12, float ex,
                                          float ey, const float* sigma2_2,
                                          const float* scale_2, int32_t nlevels,
                                          int32_t only_stereo, int32_t* pairs,
                                          int32_t pair_cap, int32_t* nmatches);

/* Projection searches: one query per MapPoint, in the reference's MapPoint order (the
 * greedy claims follow it).  u, v, radius: the GetFeaturesInArea arguments; ur: projected
 * right-image x (mTrackProjXR at :96, u - mbf*invzc at :1477, u - bf*invz at :924);
 * min_level/max_level: Frame::GetFeaturesInArea level arguments (-1 = unused, Frame.cc:373);
 * pred_level: the predicted octave for the matcher-side octave filters; angle: the source
 * keypoint angle for the rotation check (LastFrame / KeyFrame variants).  A query with
 * radius < 0 is inactive (no search, result -1). */
typedef struct {
    float u, v, ur, radius;
    int32_t min_level, max_level, pred_level;
    float angle;
} orbx_proj_query;

typedef enum {
    /* SearchByProjection(Frame&, vector<MapPoint*>, th)   :46-132  (Frame grid + levels,
       skip claimed, stereo check, best+2nd with levels, TH_HIGH, ratio if same level) */
    ORBX_PROJ_FRAME_MAPPOINTS = 0,
    /* SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th)  :321-434 (KeyFrame grid,
       skip claimed, octave in [pred-1, pred], TH_LOW) */
    ORBX_PROJ_KF_SCW = 1,
    /* SearchByProjection(Frame&, const Frame& LastFrame, th, bMono) :1392-1538 (Frame grid +
       levels, skip claimed, stereo check, TH_HIGH, rotation check) */
    ORBX_PROJ_LAST_FRAME = 2,
    /* SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist) :1540-1667 (Frame
       grid + levels, skip claimed, ORBdist, rotation check) */
    ORBX_PROJ_KEYFRAME = 3,
    /* Fuse(KeyFrame*, vpMapPoints, th) :879-1029 (KeyFrame grid, octave filter, reprojection
       chi2 test, TH_LOW; no claims: the caller applies Replace/AddMapPoint in query order) */
    ORBX_PROJ_FUSE = 4,
    /* Fuse(KeyFrame*, Scw, vpPoints, th, vpReplacePoint) :1033-1156 (TH_LOW, no claims) */
    ORBX_PROJ_FUSE_SCW = 5,
    /* one direction of SearchBySim3 :1204-1281 / :1284-1361 (TH_HIGH, no claims) */
    ORBX_PROJ_SIM3 = 6,
    ORBX_PROJ_MODE_COUNT = 7
} orbx_proj_mode;

/* Runs one projection search of `mode` against `target`.  qdesc: nq x 32 query (MapPoint)
 * descriptors.  claimed[target->n] (may be NULL = none): features the search must skip from
 * the start (F.mvpMapPoints[i] with Observations()>0 for FRAME_MAPPOINTS / LAST_FRAME,
 * non-NULL for KEYFRAME, vpMatched[i] non-NULL for KF_SCW); ignored by FUSE/FUSE_SCW/SIM3.
 * inv_sigma2: target mvInvLevelSigma2 (FUSE only, may be NULL otherwise); nlevels its size.
 * orb_dist: the ORBdist argument (KEYFRAME only).  match_q[nq]: target feature matched to
 * each query, or -1, after the rotation-consistency filter where the mode has one. */
orbx_status orbx_search_by_projection(orbx_matcher* m, int32_t mode,
                                      const orbx_featureset* target, const uint8_t* claimed,
                                      const uint8_t* qdesc, const orbx_proj_query* q,
                                      int32_t nq, const float* inv_sigma2, int32_t nlevels,
                                      int32_t orb_dist, int32_t* match_q, int32_t* nmatches);

/* orbx_search_by_projection with per-query flags and call flags.
 * qflags[nq] (may be NULL = all 0): ORBX_QF_NO_CLAIM marks a query whose MapPoint has no
 * observations (Observations() == 0, e.g. the stereo "temporal" points Tracking::UpdateLastFrame
 * puts into the last frame).  The reference's skip test for an already matched feature is
 * F.mvpMapPoints[i] && F.mvpMapPoints[i]->Observations() > 0 (:90-92, :1471-1473), so such a
 * query's match does not keep later queries off its feature (a later match overwrites it).
 * Only the FRAME_MAPPOINTS and LAST_FRAME modes read the flag.
 * flags: ORBX_PROJ_PREFILTER returns every accepted query's feature without the
 * rotation-consistency filter (LAST_FRAME / KEYFRAME), *nmatches = the accepted count, so the
 * caller can apply the reference's per-feature filter itself (rotHist holds feature indices,
 * :1508 / :1637: with overwritten matches a feature can sit in two bins).  LAST_FRAME with
 * check_orientation and any ORBX_QF_NO_CLAIM query requires ORBX_PROJ_PREFILTER
 * (ORBX_ERR_INVALID otherwise): the reference clears per feature (:1516-1535), which a
 * per-query filter cannot reproduce once a feature is matched twice.
 * Replaces the same ORBmatcher methods as orbx_search_by_projection, which equals this call
 * with qflags = NULL and flags = 0. */
enum { ORBX_QF_NO_CLAIM = 1 };
enum { ORBX_PROJ_PREFILTER = 1 };
orbx_status orbx_search_by_projection_ex(orbx_matcher* m, int32_t mode,
                                         const orbx_featureset* target, const uint8_t* claimed,
                                         const uint8_t* qdesc, const orbx_proj_query* q,
                                         const uint8_t* qflags, int32_t nq,
                                         const float* inv_sigma2, int32_t nlevels,
                                         int32_t orb_dist, int32_t flags, int32_t* match_q,
                                         int32_t* nmatches);

/* ORBmatcher::SearchBySim3 (:1158-1382).  q12[n1]: KF1 feature i's MapPoint projected into
 * KF2 (radius < 0 when the reference skips i1: no MapPoint, already matched, bad, or failed
 * the depth/image/distance tests); qdesc1: n1 x 32 MapPoint descriptors.  q21[n2] likewise
 * for KF2's MapPoints projected into KF1.  match12[n1] = idx2 where both directions agree
 * (vpMatches12[i1] = vpMapPoints2[idx2]), else -1; *nmatches = nFound. */
orbx_status orbx_search_by_sim3(orbx_matcher* m, const orbx_featureset* kf1,
                                const orbx_featureset* kf2, const uint8_t* qdesc1,
                                const orbx_proj_query* q12, int32_t n1, const uint8_t* qdesc2,
                                const orbx_proj_query* q21, int32_t n2, int32_t* match12,
                                int32_t* nmatches);

/* ORBmatcher::SearchForInitialization (:446-561).  prev_matched: n1 x 2 floats
 * (vbPrevMatched), updated in place for matched features like the reference (:555-558).
 * match12[n1] = vnMatches12. */
orbx_status orbx_search_for_initialization(orbx_matcher* m, const orbx_featureset* f1,
                                           const orbx_featureset* f2, float* prev_matched,
                                           int32_t window_size, int32_t* match12,
                                           int32_t* nmatches);

/* ---- batched, device-resident API (relocalisation / loop closure / local mapping) -------
 * A keyframe database: nkf featuresets concatenated.  Keyframe k owns features
 * [feat_off[k], feat_off[k+1]) of keys/desc/u_right/flag (feature indices inside a keyframe
 * are local, 0-based) and FeatureVector nodes [node_off[k], node_off[k+1]) of node_id /
 * node_feat_off (absolute offsets into node_feat, which holds local feature indices;
 * node_feat_off has node_off[nkf] + 1 entries).  flag[i]: MapPoint mask (valid for BoW,
 * has_mp for triangulation).  All pointers are device memory. */
typedef struct {
    int32_t nkf;
    int32_t max_feat;              /* host-known bound on any keyframe's feature count
                                      (sizes the on-chip workspace); a keyframe above it
                                      is skipped (outputs -1, count 0) and flagged for
                                      orbx_matcher_sync */
    const int32_t* feat_off;
    const orbx_keypoint* keys;
    const uint8_t* desc;
    const float* u_right;          /* may be NULL (all monocular) */
    const uint8_t* flag;
    const int32_t* node_off;
    const uint32_t* node_id;
    const int32_t* node_feat_off;
    const int32_t* node_feat;
    /* Optional (all NULL, or all set by orbx_kf_db_node_order): the features again in node
     * order, entry p = keyframe-local feature node_feat[p] of p's keyframe.  A per-node matcher
     * (SearchForTriangulation) then reads each node's keys, descriptors, stereo and flag as
     * contiguous runs instead of one gather per feature (each gather a cache line of its own:
     * 4.3x the bytes it uses).  node_desc 16-byte aligned; node_u_right NULL iff u_right is. */
    const orbx_keypoint* node_keys;
    const uint8_t* node_desc;
    const float* node_u_right;
    const uint8_t* node_flag;
} orbx_kf_db;

/* Fills a database's node-order copies (orbx_kf_db node_keys / node_desc / node_u_right /
 * node_flag): device arrays of n = db->node_feat_off[db->node_off[db->nkf]] entries each
 * (d_u_right may be NULL when db->u_right is), on `stream`; the caller then points the
 * database's node_* fields at them.  A database whose flags change (MapPoints added) must be
 * reordered again. */
orbx_status orbx_kf_db_node_order(orbx_matcher* m, const orbx_kf_db* db, int32_t n,
                                  orbx_keypoint* d_keys, uint8_t* d_desc, float* d_u_right,
                                  uint8_t* d_flag, void* stream);

/* SearchByBoW(KeyFrame*, Frame&) of every keyframe of `db` against one frame `f` (device
 * featureset; grid unused) — the relocalisation candidate loop of Tracking.cc:1479-1500.
 * d_match: device [db->nkf][f->n] (KF-local feature index per frame feature, or -1);
 * d_nmatches: device [db->nkf]. */
orbx_status orbx_search_by_bow_kf_frame_batch_device(orbx_matcher* m, const orbx_kf_db* db,
                                                     const orbx_featureset* f,
                                                     int32_t* d_match, int32_t* d_nmatches,
                                                     void* stream);

/* SearchForTriangulation over njobs keyframe pairs (kf1[j], kf2[j]) of `db` (the
 * LocalMapping::CreateNewMapPoints loop, LocalMapping.cc:271-276).  d_F12: device njobs x 9,
 * d_epi: device njobs x 2 (ex, ey); sigma2 / scale: HOST tables of nlevels floats shared by
 * all keyframes.  d_match12: device, one slot per KF1 feature of each job laid out at
 * d_job_off[j] (device, njobs+1, = prefix of KF1 sizes); d_nmatches: device [njobs]. */
orbx_status orbx_search_for_triangulation_batch_device(
    orbx_matcher* m, const orbx_kf_db* db, int32_t njobs, const int32_t* d_kf1,
    const int32_t* d_kf2, const float* d_F12, const float* d_epi, const float* sigma2,
    const float* scale, int32_t nlevels, int32_t only_stereo, const int32_t* d_job_off,
    int32_t* d_match12, int32_t* d_nmatches, void* stream);

/* ---- The per-match loop behind SearchForTriangulation: LocalMapping::CreateNewMapPoints,
 * src/LocalMapping.cc:356-507 (parallax test :370-394, linear triangulation :398-413 or
 * KeyFrame::UnprojectStereo :416-423, depth signs :430-436, reprojection chi2 :439-489, scale
 * consistency :492-507).  What stays with the caller per job: the baseline / median-depth skip
 * (:308-327), ComputeF12 (:331), ratio_factor = 1.5f * mfScaleFactor (:294); per success:
 * new MapPoint, AddObservation, AddMapPoint (:510-525). ----
 *
 * One code per exit of the loop body: the three ways to succeed, the empty slot, then the
 * `continue` statements. */
typedef enum {
    ORBX_TRI_OK_TRIANGULATED = 0, /* :394-415 the SVD branch, all tests passed                 */
    ORBX_TRI_OK_STEREO1 = 1,      /* :416-419 mpCurrentKeyFrame->UnprojectStereo(idx1)         */
    ORBX_TRI_OK_STEREO2 = 2,      /* :420-423 pKF2->UnprojectStereo(idx2)                      */
    ORBX_TRI_NO_MATCH = 3,        /* the slot holds -1 (no pair), or the slot was refused      */
    ORBX_TRI_LOW_PARALLAX = 4,    /* :424-425; also UnprojectStereo's empty Mat (depth <= 0)   */
    ORBX_TRI_W_ZERO = 5,          /* :409-410 x3D.at<float>(3) == 0                            */
    ORBX_TRI_BEHIND_1 = 6,        /* :431-432 z1 <= 0                                          */
    ORBX_TRI_BEHIND_2 = 7,        /* :435-436 z2 <= 0                                          */
    ORBX_TRI_REPROJ_1 = 8,        /* :450-451 / :461-462                                       */
    ORBX_TRI_REPROJ_2 = 9,        /* :476-477 / :487-488                                       */
    ORBX_TRI_DIST_ZERO = 10,      /* :498-499                                                  */
    ORBX_TRI_SCALE = 11,          /* :506-507                                                  */
    ORBX_TRI_CODE_COUNT = 12
} orbx_tri_code;

typedef struct orbx_frame_pose orbx_frame_pose;   /* include/orbx_frame.h */

/* cosParallaxStereo of every feature of one keyframe (:387, :389), host only:
 * out[i] = (float)cos(2 * atan2(mb / 2, depth[i])) with mb / 2 a float division and libm's double
 * atan2 and cos.  Computed once per keyframe when it is uploaded: the device never evaluates a
 * double cos or atan2, and the term is exactly what the host's libm gives.
 * (With libstdc++ and the `using namespace std` the reference's DBoW2 headers bring in, the
 * unqualified calls at :387 resolve to the float overloads; glibc 2.35's float forms differ from
 * this by one unit in the last place for about 0.16 % of depths.  A caller that wants those fills
 * the table itself: the kernel only reads it.)  n < 0 or a NULL array with n > 0:
 * ORBX_ERR_INVALID. */
orbx_status orbx_parallax_stereo_cos(float mb, const float* depth, int32_t n, float* out);

/* The loop for njobs keyframe pairs (kf1[j] = mpCurrentKeyFrame, kf2[j] = pKF2) of `db`, fed by
 * exactly what orbx_search_for_triangulation_batch_device wrote: d_match12 / d_job_off, one slot
 * per KF1 feature holding the KF2 feature or -1.  On one stream the two calls chain with no host
 * step.
 *   d_poses       one orbx_frame_pose per keyframe of db; read: Rcw, tcw, Ow, fx, fy, cx, cy, mbf,
 *                 scale[] (mvScaleFactors; mvLevelSigma2[o] = scale[o] * scale[o],
 *                 ORBextractor.cc:421-422) and nlevels
 *   d_depth       mvDepth, d_cos_stereo: orbx_parallax_stereo_cos of it; per feature of db, indexed
 *                 like db->keys (keyframe k's at feat_off[k])
 *   d_keys_raw    mvKeys (KeyFrame::UnprojectStereo reads the raw keypoint, KeyFrame.cc:634-635);
 *                 NULL: db->keys.  db->keys is mvKeysUn, db->u_right mvuRight (NULL: monocular)
 *   mb            the baseline d_cos_stereo was built with; the kernel reads the table only
 *   ratio_factor  1.5f * mpCurrentKeyFrame->mfScaleFactor
 *   d_status      [slot] an orbx_tri_code; -1 slots get ORBX_TRI_NO_MATCH
 *   d_x3d         [3 * slot ..] x3D, written on the three OK codes only, otherwise untouched
 *   d_nnew        [njobs] the OK slots of each job (nnew of :525)
 * Arithmetic: xn from float products with a 1.0 third entry; ray = Rwc * xn in cv::gemm's
 * small-matrix form; ray.dot(ray) and cv::norm in double; cosParallaxRays < 0.9998, 5.991 *
 * sigmaSquare and 7.8 * sigmaSquare compared in double; invz = (float)(1.0 / z); :388 is an
 * `else if` (with both features stereo only cosParallaxStereo1 is read); :482 uses the current
 * keyframe's mbf for keyframe 2.  Restated from OpenCV 3.2 [unverified-OpenCV]:
 * the rows of A (cv::addWeighted in double), cv::SVD::compute (one-sided Jacobi, at most 30
 * sweeps) and x3D.rowRange(0,3) / w (Mat::convertTo).  hypot is glibc 2.35's.
 * UnprojectStereo with depth <= 0 returns an empty Mat, on which the reference's next statement
 * throws; the slot gets ORBX_TRI_LOW_PARALLAX (the exit for "no point could be formed").
 * Statuses: m, db, d_poses, d_depth, d_cos_stereo, d_kf1, d_kf2, d_job_off, d_match12, d_status,
 * d_x3d or d_nnew NULL (with njobs > 0), njobs < 0 or > 65535, db->max_feat outside [0, 32768],
 * mb negative or NaN: ORBX_ERR_INVALID; njobs == 0: ORBX_OK, nothing is touched.  What only the
 * device can see is refused per slot: a keyframe index outside [0, nkf) or a pose whose nlevels
 * is outside [1, 16] (the whole job), a match outside KF2's features, or an octave outside
 * [0, nlevels): the slots get ORBX_TRI_NO_MATCH, nothing of them is read, and the matcher is
 * flagged, so the next orbx_matcher_sync returns ORBX_ERR_CAPACITY. */
orbx_status orbx_triangulate_matches_batch_device(
    orbx_matcher* m, const orbx_kf_db* db, int32_t njobs, const int32_t* d_kf1,
    const int32_t* d_kf2, const orbx_frame_pose* d_poses, const float* d_depth,
    const float* d_cos_stereo, const orbx_keypoint* d_keys_raw, float mb, float ratio_factor,
    const int32_t* d_job_off, const int32_t* d_match12, int32_t* d_status, float* d_x3d,
    int32_t* d_nnew, void* stream);

/* One keyframe pair from host arrays (copied to the device for the call), taking the (idx1, idx2)
 * list orbx_search_for_triangulation returns: status[p] and x3d[3p ..] belong to pair p, x3d
 * written on the OK codes only; *nnew (optional) the OK count.  keys: mvKeysUn; keys_raw: mvKeys
 * (NULL: keys); u_right NULL: monocular; depth (mvDepth) may be NULL where u_right is.
 * cos_stereo1 / cos_stereo2 NULL: orbx_parallax_stereo_cos(mb, depth) is computed here.
 * The checks run before the device is touched.  ORBX_ERR_INVALID: a NULL pose, keys, pairs,
 * status or x3d (with npairs > 0), a negative count, depth NULL with u_right given, mb negative or
 * NaN, a pair index outside its keyframe, an idx1 that occurs twice, an octave of a paired
 * feature outside [0, nlevels), nlevels < 1.  nlevels > 16 or a keyframe above 32768 features:
 * ORBX_ERR_UNSUPPORTED.  npairs == 0: ORBX_OK.  Without a GPU: ORBX_ERR_DEVICE.  Calls from
 * several threads run beside each other, each on a device stream and staging buffer of its own. */
orbx_status orbx_triangulate_matches(
    const orbx_frame_pose* pose1, const orbx_frame_pose* pose2, const orbx_keypoint* keys1,
    const orbx_keypoint* keys_raw1, const float* u_right1, const float* depth1,
    const float* cos_stereo1, int32_t n1, const orbx_keypoint* keys2,
    const orbx_keypoint* keys_raw2, const float* u_right2, const float* depth2,
    const float* cos_stereo2, int32_t n2, float mb, float ratio_factor, const int32_t* pairs,
    int32_t npairs, int32_t* status, float* x3d, int32_t* nnew, int device);

/* SearchByProjection over njobs frames at once — one Tracking::SearchLocalPoints
 * (Tracking.cc:1297-1347, ORBmatcher.cc:41-136) per frame, or any other
 * non-initialisation orbx_proj_mode, each job independent of the others.
 * `frames` holds DEVICE pointers to the concatenation of the frames: keys / desc / u_right
 * (u_right may be NULL) with frame j's features at [d_feat_off[j], d_feat_off[j+1]);
 * grid_off = njobs blocks of grid_cols*grid_rows+1 entries (frame-local positions, frame j's
 * block at j*(cells+1)); grid_feat with frame j's entries from d_grid_off[j] (frame-local
 * feature indices).  Grid geometry (cols, rows, bounds, inverse cell sizes) is shared: one
 * camera.  frames->n is ignored; max_feat (host) bounds every frame's size.
 * Queries: d_qdesc / d_q with frame j's at [d_q_off[j], d_q_off[j+1]), nq in total.
 * d_claimed: device, one byte per feature of the concatenation (already-matched features of
 * the KEYFRAME / FUSE modes), or NULL.  inv_sigma2: HOST table of nlevels floats.
 * Outputs (device): d_match[nq] frame-local feature index or -1, d_nmatches[njobs].
 * Scratch belongs to the matcher: calls on one matcher must share `stream` or be serialised.
 * A frame above max_feat gets no matches and is flagged for orbx_matcher_sync. */
orbx_status orbx_search_by_projection_batch_device(
    orbx_matcher* m, int32_t mode, const orbx_featureset* frames, int32_t njobs,
    const int32_t* d_feat_off, const int32_t* d_grid_off, int32_t max_feat,
    const uint8_t* d_claimed, const uint8_t* d_qdesc, const orbx_proj_query* d_q,
    const int32_t* d_q_off, int32_t nq, const float* inv_sigma2, int32_t nlevels,
    int32_t orb_dist, int32_t* d_match, int32_t* d_nmatches, void* stream);

/* Brute-force Hamming top-2 of nq query descriptors (q: nq x 32) against ndb database rows
 * (db: ndb x 32) — SURVEY §8(b) orbx_hamming_bf_top2 / §8(e) C4.  The semantics are the best /
 * second loop of the ORBmatcher searches (src/ORBmatcher.cc:232-256) run over every row in
 * order: bestDist1 = bestDist2 = 256 initially, `dist < bestDist1` moves the best to the
 * second, else `dist < bestDist2` updates the second.  best_idx[i] = the first row at the least
 * distance (-1 if no row is below 256), best_dist[i] that distance (256 if none),
 * second_dist[i] the second least distance (equal to best_dist[i] on a tie, 256 if none).
 * Host pointers; the database is copied to the device for the call (keep a large database
 * resident and use the _device form instead). */
orbx_status orbx_hamming_bf_top2(orbx_matcher* m, const uint8_t* q, int32_t nq,
                                 const uint8_t* db, int64_t ndb, int32_t* best_idx,
                                 int32_t* best_dist, int32_t* second_dist);
/* The same on device arrays, on the caller's stream; best_idx is offset by idx_base (a shard
 * of a larger database reports global row numbers, so per-shard results merge in shard order
 * with distributed.merge_top2; -1 stays -1).  idx_base >= 0 and ndb + idx_base < 2^31 - 1.
 * d_q and d_db must be 4-byte aligned: the kernels read them as dwords, and the scalar loads
 * of k_bf_top2 would drop the low address bits of a byte-offset view without a fault.  A call
 * that breaks either rule returns ORBX_ERR_INVALID before anything is launched.  The partial
 * results live in the matcher's scratch: a call on another stream than the previous call's
 * waits (on the device, by an event) until that call's kernels are done with it. */
orbx_status orbx_hamming_bf_top2_device(orbx_matcher* m, const uint8_t* d_q, int32_t nq,
                                        const uint8_t* d_db, int64_t ndb, int64_t idx_base,
                                        int32_t* d_best_idx, int32_t* d_best_dist,
                                        int32_t* d_second_dist, void* stream);

/* The kernel the brute-force top-2 of a matcher runs its distances in (results are identical):
 * ORBX_BF_MFMA (the default): k_bf_mfma, +-1 int8 dot products on the matrix cores;
 * ORBX_BF_VALU: k_bf_top2, v_xor + v_bcnt on the vector ALUs (north_star's "no MFMA" form). */
enum { ORBX_BF_MFMA = 0, ORBX_BF_VALU = 1 };
orbx_status orbx_matcher_set_bf_kernel(orbx_matcher* m, int32_t kernel);
/* The kernel name of that choice ("k_bf_mfma" / "k_bf_top2"); NULL for an unknown value. */
const char* orbx_bf_kernel_name(int32_t kernel);
/* The default's name ("k_bf_mfma"). */
const char* orbx_bf_kernel(void);

/* Rows per chunk of the brute-force top-2 (one workgroup per chunk and query block; the
 * chunks' partial top-2 are folded by k_bf_merge).  A tuning and test knob: the results never
 * depend on it.  0 (the default) = automatic, from the row and query counts and the device's
 * CU count; any other value must be a multiple of 64 in [256, 2^23 - 64], else
 * ORBX_ERR_INVALID and the setting stays as it was.  Launches nothing. */
orbx_status orbx_matcher_set_bf_chunk(orbx_matcher* m, int64_t rows);

/* The launch geometry a brute-force top-2 of nq queries against ndb rows would use with the
 * handle's kernel, chunk setting and CU count (host only; the launcher evaluates the same
 * functions).  The directed tests assert the regime they mean with it before they rely on it. */
typedef struct {
    int32_t chunk;          /* rows per chunk                                               */
    int32_t nchunks;        /* ceil(ndb / chunk); 0 for an empty database                   */
    int32_t query_blocks;   /* workgroups per chunk: 1024 (k_bf_mfma) / 256 (k_bf_top2)
                               queries each                                                 */
    int32_t nqpad;          /* query stride of the partial results (a multiple of 1024)     */
    int32_t merge_slice;    /* chunks per thread slice of k_bf_merge: ceil(nchunks / 8)     */
    int64_t partial_bytes;  /* scratch the partial results take                             */
} orbx_bf_launch_info;
orbx_status orbx_matcher_bf_launch_info(orbx_matcher* m, int32_t nq, int64_t ndb,
                                        orbx_bf_launch_info* out);

/* Waits for `stream` and returns ORBX_ERR_CAPACITY if a batched call on this matcher met a
 * keyframe above max_feat since the last sync (the flag is then cleared). */
orbx_status orbx_matcher_sync(orbx_matcher* m, void* stream);

/* MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:252-313) for npoints map points:
 * point p's observed descriptors are rows [off[p], off[p+1]) of desc (n x 32, in the order
 * the reference walks mObservations, skipping bad keyframes).  best[p] = the row (relative
 * to off[p]) with the least median distance to the others (first on ties), or -1 when the
 * point has no descriptor (the reference then keeps mDescriptor).  At most
 * ORBX_MAX_OBSERVATIONS rows per point (ORBX_ERR_UNSUPPORTED above). */
enum { ORBX_MAX_OBSERVATIONS = 256 };
orbx_status orbx_compute_distinctive_descriptors(orbx_matcher* m, const uint8_t* desc,
                                                 const int32_t* off, int32_t npoints,
                                                 int32_t* best);
/* Same on device arrays, on the caller's stream (points above the limit get -1 and are
 * flagged for orbx_matcher_sync). */
orbx_status orbx_compute_distinctive_descriptors_device(orbx_matcher* m, const uint8_t* d_desc,
                                                        const int32_t* d_off, int32_t npoints,
                                                        int32_t* d_best, void* stream);

/* Which kernel variant a call of the given sizes runs (host only: no device, no handle).
 * kind: ORBX_VK_BOW_KF_FRAME / ORBX_VK_BOW_KF_KF with n_a / n_b = the feature counts of the
 * first / second featureset (nq unused); ORBX_VK_INIT with n_a / n_b = the feature counts of
 * F1 / F2; ORBX_VK_PROJ + an orbx_proj_mode with n_b = the target's feature count and nq the
 * query count (n_a unused).  Returns 0 for the on-chip variant (SearchByBoW: the second set's
 * descriptors staged in LDS; claim-mode projections: an owner word per target feature in
 * k_proj_claim; also every kind that has a single variant, such as ORBX_VK_INIT's k_proj_init), 1
 * for the fallback (descriptors read from global memory; one query per replay round), or the
 * ORBX_ERR_INVALID /
 * ORBX_ERR_UNSUPPORTED the entry point itself returns for these sizes. */
enum { ORBX_VK_BOW_KF_FRAME = 0, ORBX_VK_BOW_KF_KF = 1, ORBX_VK_INIT = 2, ORBX_VK_PROJ = 16 };
int32_t orbx_matcher_variant(int32_t kind, int32_t n_a, int32_t n_b, int32_t nq);

/* ---- Sim3Solver (src/Sim3Solver.cc; LoopClosing::ComputeSim3, LoopClosing.cc:285-413) -------
 * Horn's closed-form similarity from three correspondences inside the reference's RANSAC loop,
 * between SearchByBoW(KF, KF) and SearchBySim3.  What stays with the caller: the object tests of
 * the constructor (isBad, GetIndexInKeyFrame, :64-79), the rand() stream (the library never calls
 * rand(): orbx_sim3_sample_triples turns the caller's raw rand() values into the minimal sets of
 * :163-177).  OptimizeSim3 is orbx_sim3_optimize* below.  The arithmetic is the reference's
 * statement by statement; the forms evaluated inside OpenCV 3.2 are restated and PARITY UNPINNED
 * (DESIGN.md §2). */

/* One kept correspondence (:81-100): i1 = the slot in vpMatched12, the two world positions
 * (pMP1 / pMP2 ->GetWorldPos()) and the octaves of the two undistorted keypoints. */
typedef struct {
    int32_t i1;
    float X1w[3];
    float X2w[3];
    int32_t octave1, octave2;
} orbx_sim3_corr;

/* One solver.  kf1 / kf2 index the pose array (read: Rcw, tcw, fx, fy, cx, cy); sigma2_1 / _2 are
 * the keyframes' mvLevelSigma2 with nlevels1 / nlevels2 entries in [1, 16].  The N correspondences
 * are corr[corr_off .. corr_off + N); the inlier bytes are inliers[inlier_off .. + mN1); the
 * minimal set of iteration k (0-based, counted from SetRansacParameters on) is
 * triples[3 * (triple_off + k) ..], k < max_its.  max_its is mRansacMaxIts as
 * orbx_sim3_ransac_iterations returns it; n_iterations is the argument of iterate(). */
typedef struct {
    int32_t kf1, kf2;
    float sigma2_1[16], sigma2_2[16];
    int32_t nlevels1, nlevels2;
    int32_t mN1, N, corr_off, inlier_off, triple_off;
    int32_t fix_scale, min_inliers, max_its, n_iterations;
} orbx_sim3_job;

/* mnIterations and mnBestInliers, kept across calls of iterate() (in / out). */
typedef struct {
    int32_t iterations, best_inliers;
} orbx_sim3_state;

#define ORBX_SIM3_REFUSED_OCTAVE (1u << 24)  /* an octave outside [0, nlevels), or nlevels outside [1, 16] */
#define ORBX_SIM3_REFUSED_TRIPLE (1u << 25)  /* a minimal-set index outside [0, N) or repeated            */
#define ORBX_SIM3_REFUSED_I1 (1u << 26)      /* an i1 outside [0, mN1)                                     */
#define ORBX_SIM3_REFUSED_LIMIT (1u << 27)   /* N above max_n, the call's iterations above max_call_its,
                                                max_its outside [1, limit], a negative count or state    */
#define ORBX_SIM3_REFUSED_RANGE (1u << 28)   /* kf1 / kf2 or an offset outside the arrays of the call      */
#define ORBX_SIM3_REFUSED_ANY (0x1fu << 24)

/* What one iterate() call gives.  found: a model was returned (:192-199) at the 1-based iteration
 * `iteration` with n_inliers inliers, and the job's inlier bytes are set through i1.  no_more:
 * bNoMore.  best_updated: `mnInliersi >= mnBestInliers` held at least once in this call; R12
 * (mBestRotation, row-major), t12, s12, T12 (mBestT12) and best_inliers then hold the last such
 * iteration's model, which is the returned one when found; otherwise they are not written, and
 * iteration / n_inliers are 0.  info: ORBX_SIM3_REFUSED_* bits; a refused job gets found = 0 and
 * info, and nothing else of its outputs, its state or its inlier bytes is touched. */
typedef struct {
    int32_t found, iteration, n_inliers, no_more;
    uint32_t info;
    int32_t best_updated, best_inliers;
    float R12[9], t12[3], s12, T12[16];
} orbx_sim3_result;

/* SetRansacParameters (:114-138), host only: epsilon = (float)min_inliers / N, nIterations =
 * ceil(log(1 - prob) / log(1 - pow(epsilon, 3))) in double with the host's libm (1 when
 * min_inliers == N), converted to int as x86-64 does (out of range or NaN: INT_MIN), and
 * max(1, min(nIterations, max_its)) returned. */
int32_t orbx_sim3_ransac_iterations(double prob, int32_t min_inliers, int32_t max_its, int32_t N);

/* The minimal sets of n_its iterations (:163-177) from 3 * n_its raw rand() values in
 * [0, RAND_MAX]: three draws without replacement by swap-with-last over 0 .. N-1, each draw
 * DUtils::Random::RandomInt(0, size - 1) = int(((double)r / ((double)RAND_MAX + 1.0)) * size).
 * ORBX_ERR_INVALID: N < 3, n_its < 0, a NULL array with n_its > 0, a value outside [0, RAND_MAX]. */
orbx_status orbx_sim3_sample_triples(int32_t N, int32_t n_its, const int32_t* rand_values,
                                     int32_t* triples);

/* The largest N (max_n), iterations per call (max_call_its, also the largest max_its) and jobs a
 * call takes, and the scratch bytes a call may need at most (host only; the launcher evaluates
 * the same expressions).  NULL outputs are skipped. */
orbx_status orbx_sim3_limits(int32_t* max_n, int32_t* max_its, int32_t* max_jobs,
                             int64_t* max_scratch_bytes);

/* iterate(n_iterations) of njobs solvers at once, every array on the device, on `stream` with no
 * host step: k_sim3_prepare (camera-frame points, image points, the two size_t bounds),
 * k_sim3_hypotheses (one wave per iteration of the call: the model, then the inlier count) and
 * k_sim3_select (the first returning iteration in order, the last `>=` record, the inlier bytes,
 * the state).  max_n >= every job's N and max_call_its >= every job's iterations in this call
 * (min(max_its - iterations, n_iterations)) size the grids and the matcher's scratch; ncorr,
 * ntriples (triples, i.e. 3 ints each), ninlier_bytes and nposes are the lengths of the arrays,
 * and a job that points outside them is refused.  d_state is in / out, d_results and d_inliers out.
 * ORBX_ERR_INVALID: m NULL, a NULL array with njobs > 0, a negative count.  max_n, max_call_its or
 * njobs above orbx_sim3_limits, or their scratch above its bound: ORBX_ERR_UNSUPPORTED.
 * njobs == 0: ORBX_OK, nothing touched.  Calls on one matcher share its scratch: one stream, or
 * serialised. */
orbx_status orbx_sim3_iterate_batch_device(
    orbx_matcher* m, const orbx_sim3_job* d_jobs, int32_t njobs, int32_t max_n,
    int32_t max_call_its, const orbx_frame_pose* d_poses, int32_t nposes,
    const orbx_sim3_corr* d_corr, int64_t ncorr, const int32_t* d_triples, int64_t ntriples,
    orbx_sim3_state* d_state, orbx_sim3_result* d_results, uint8_t* d_inliers,
    int64_t ninlier_bytes, void* stream);

/* One solver from host arrays (copied to the device for the call).  job->kf1, kf2 and the three
 * offsets are ignored: corr holds job->N records, triples 3 * job->max_its ints, inliers job->mN1
 * bytes.  ORBX_ERR_INVALID: a NULL argument, N, mN1 or n_iterations negative, max_its < 1; N or
 * max_its above orbx_sim3_limits: ORBX_ERR_UNSUPPORTED; the checks run before the device is
 * touched, and without a GPU the call returns ORBX_ERR_DEVICE.  What the batched form refuses per
 * job comes back the same way, in res->info.  Calls from several threads run beside each other,
 * each on a device stream and staging buffer of its own. */
orbx_status orbx_sim3_iterate(const orbx_frame_pose* pose1, const orbx_frame_pose* pose2,
                              const orbx_sim3_job* job, const orbx_sim3_corr* corr,
                              const int32_t* triples, orbx_sim3_state* state,
                              orbx_sim3_result* res, uint8_t* inliers, int device);

/* ---- Optimizer::OptimizeSim3 (src/Optimizer.cc:1070-1265; LoopClosing.cc:376) ---------------
 * The refinement of the solver's Sim3 over the matches SearchBySim3 added: one VertexSim3Expmap,
 * an EdgeSim3ProjectXYZ and an EdgeInverseSim3ProjectXYZ per correspondence with numerically
 * differentiated Jacobians and Huber kernels, Levenberg over the dense 7x7 solver: optimize(5),
 * the chi2 > th2 classification, optimize(10 or 5).  k_sim3_opt restates g2o decision for
 * decision (csrc/orbx_sim3opt.hip); the forms evaluated inside Eigen are restated from the
 * published algorithms [unverified-Eigen].  What stays with the caller: the
 * object tests that decide the correspondence list (isBad, GetIndexInKeyFrame >= 0, both
 * MapPoints present), gScm * gSmw, and the nInliers >= 20 decision. */

/* One kept correspondence (:1123-1202), in increasing i1: i1 = the slot in vpMatches1, the two
 * world positions, the undistorted keypoints mvKeysUn[i1].pt of KF1 and mvKeysUn[i2].pt of KF2,
 * and their octaves. */
typedef struct {
    int32_t i1;
    float X1w[3];
    float X2w[3];
    float kp1[2];
    float kp2[2];
    int32_t octave1, octave2;
} orbx_sim3opt_corr;

/* One call.  kf1 / kf2 index the pose array (read: Rcw, tcw, fx, fy, cx, cy); sigma2_1 / _2 are
 * the keyframes' mvLevelSigma2 (the information is 1.0f / sigma2[octave]) with nlevels1 / nlevels2
 * entries in [1, 16].  The N correspondences are corr[corr_off .. corr_off + N); the keep bytes
 * (vpMatches1 after the call) are keep[flag_off .. flag_off + mN1).  th2 is the reference's th2
 * (10 at its call site), fix_scale its bFixScale. */
typedef struct {
    int32_t kf1, kf2;
    float sigma2_1[16], sigma2_2[16];
    int32_t nlevels1, nlevels2;
    int32_t mN1, N, corr_off, flag_off;
    float th2;
    int32_t fix_scale;
} orbx_sim3opt_job;

/* The Sim3 a call starts from: the solver's mBestRotation, mBestTranslation and mBestScale, i.e.
 * g2o::Sim3(toMatrix3d(R12), toVector3d(t12), s12).  These are the fields R12 .. s12 of
 * orbx_sim3_result in its order, so a batch call may point d_sim3_in at &d_results[0].R12 of
 * orbx_sim3_iterate_batch_device with sim3_in_stride = sizeof(orbx_sim3_result). */
typedef struct {
    float R12[9], t12[3], s12;
} orbx_sim3opt_in;

/* info: bits 0-2 optimize() calls that ran (0-2), bits 3-9 Levenberg iterations (<= 15), bits
 * 10-18 trials (<= 150), then the flags. */
#define ORBX_SIM3OPT_ROUNDS_MASK 0x7u
#define ORBX_SIM3OPT_ITERS_SHIFT 3
#define ORBX_SIM3OPT_ITERS_MASK 0x7fu
#define ORBX_SIM3OPT_TRIALS_SHIFT 10
#define ORBX_SIM3OPT_TRIALS_MASK 0x1ffu
#define ORBX_SIM3OPT_REFUSED_OCTAVE (1u << 23)  /* an octave outside [0, nlevels), or nlevels outside [1, 16] */
#define ORBX_SIM3OPT_REFUSED_I1 (1u << 24)      /* an i1 outside [0, mN1), or not increasing                 */
#define ORBX_SIM3OPT_REFUSED_LIMIT (1u << 25)   /* N above max_n or negative, mN1 negative                    */
#define ORBX_SIM3OPT_REFUSED_RANGE (1u << 26)   /* kf1 / kf2 or an offset outside the arrays of the call      */
#define ORBX_SIM3OPT_REFUSED_ANY (0xfu << 23)
#define ORBX_SIM3OPT_THETA_LIMIT (1u << 27)     /* an update's |omega| outside orbx_sincos_f64: that trial failed */
#define ORBX_SIM3OPT_EXP_LIMIT (1u << 28)       /* an update's sigma outside orbx_exp_f64: that trial failed  */
#define ORBX_SIM3OPT_NONPOSITIVE_SOLVE (1u << 29) /* LDLT::isPositive() was false in some trial              */
#define ORBX_SIM3OPT_FEW_INLIERS (1u << 30)     /* nCorrespondences - nBad < 10: returned 0, Sim3 unchanged   */
#define ORBX_SIM3OPT_DROPPED (1u << 31)         /* nBad > 0 after the first stage (nMoreIterations = 10)      */

/* What one call gives.  n_inliers is the reference's return value; n_bad the pairs dropped after
 * the first stage.  q (x, y, z, w; not normalised, as g2o keeps it), t and s are g2oS12 after the
 * call; T12 is Converter::toCvMat(g2oS12) (s * R, t, rounded to float; row-major 4x4).  When the
 * call returns 0 early (FEW_INLIERS) and for a refused job, n_inliers = 0 and q, t, s, T12 are
 * the input Sim3; a refused job's keep bytes are not touched. */
typedef struct {
    int32_t n_inliers, n_correspondences, n_bad;
    uint32_t info;
    double q[4], t[3], s;
    float T12[16];
} orbx_sim3opt_result;

/* The largest N and the most jobs a call takes (host only).  NULL outputs are skipped. */
orbx_status orbx_sim3opt_limits(int32_t* max_n, int32_t* max_jobs);

/* OptimizeSim3 of njobs candidates at once, every array on the device, on `stream` with no host
 * step and no scratch: k_sim3_opt, one wave per job.  max_n >= every job's N; nposes, ncorr and
 * nkeep_bytes are the lengths of the arrays, and a job that points outside them is refused in its
 * info word.  Job j starts from the record at (const char*)d_sim3_in + j * sim3_in_stride
 * (sim3_in_stride >= sizeof(orbx_sim3opt_in), a multiple of 4).  d_keep: entry i1 becomes 0 when
 * the pair is dropped in either classification; entries that name no correspondence, and kept
 * pairs, are not written.
 * ORBX_ERR_INVALID: m NULL, a NULL array with njobs > 0, a negative count, a bad stride.  max_n or
 * njobs above orbx_sim3opt_limits: ORBX_ERR_UNSUPPORTED.  njobs == 0: ORBX_OK, nothing touched. */
orbx_status orbx_sim3_optimize_batch_device(
    orbx_matcher* m, const orbx_sim3opt_job* d_jobs, int32_t njobs, int32_t max_n,
    const orbx_frame_pose* d_poses, int32_t nposes, const orbx_sim3opt_corr* d_corr, int64_t ncorr,
    const void* d_sim3_in, int64_t sim3_in_stride, orbx_sim3opt_result* d_results,
    uint8_t* d_keep, int64_t nkeep_bytes, void* stream);

/* One call from host arrays (copied to the device for the call).  job->kf1, kf2 and the two
 * offsets are ignored: corr holds job->N records, keep job->mN1 bytes (in / out).
 * ORBX_ERR_INVALID: a NULL argument, N or mN1 negative; N above orbx_sim3opt_limits:
 * ORBX_ERR_UNSUPPORTED; the checks run before the device is touched, and without a GPU the call
 * returns ORBX_ERR_DEVICE.  What the batched form refuses per job comes back the same way, in
 * res->info.  Calls from several threads run beside each other, each on a device stream and
 * staging buffer of its own. */
orbx_status orbx_sim3_optimize(const orbx_frame_pose* pose1, const orbx_frame_pose* pose2,
                               const orbx_sim3opt_job* job, const orbx_sim3opt_corr* corr,
                               const orbx_sim3opt_in* sim3_in, orbx_sim3opt_result* res,
                               uint8_t* keep, int device);

/* ---- PnPsolver (src/PnPsolver.cc; Tracking::Relocalization, Tracking.cc:1444-1635) ----------
 * EPnP inside the reference's RANSAC loop, between SearchByBoW(KF, Frame) and PoseOptimization:
 * four sampled correspondences per iteration (compute_pose, :477-525), CheckInliers over all of
 * them (:308-339), Refine over the best inlier set (:260-305).  What stays with the caller: the
 * object tests of the constructor (isBad, :79-101; orbx_pnp_correspondences_batch_device keeps
 * every matched slot), the rand() stream (the library never calls rand(): orbx_pnp_sample_quads
 * turns the caller's raw rand() values into the minimal sets of :188-201), and every decision
 * between the calls (nmatches < 15, nGood < 10, < 50, ...).  The arithmetic is the reference's
 * statement by statement in its own types; the forms evaluated inside OpenCV 3.2
 * (cvMulTransposed, cvSVD, cvInvert, cvSolve, convertTo) are restated and PARITY UNPINNED
 * (DESIGN.md §2). */

/* One kept correspondence (:79-101), in increasing i: i = the slot in vpMapPointMatches
 * (mvKeyPointIndices), the MapPoint's world position, the undistorted keypoint mvKeysUn[i].pt
 * and its octave. */
typedef struct {
    int32_t i;
    float X[3];
    float u, v;
    int32_t octave;
} orbx_pnp_corr;

/* One solver.  sigma2 is the frame's mvLevelSigma2 with nlevels entries in [1, 16]; th2 the th2 of
 * SetRansacParameters (mvMaxError[i] = sigma2[octave] * th2, a float product).  The N
 * correspondences are corr[corr_off .. corr_off + N); the inlier bytes are inliers[inlier_off ..
 * inlier_off + n_matches); the best inlier bytes are best[best_off .. best_off + N); the minimal
 * set of iteration k (0-based, counted from the solver's construction on) is
 * quads[4 * (quad_off + k) ..].  min_inliers (>= 1) and max_its are mRansacMinInliers and
 * mRansacMaxIts as orbx_pnp_ransac_parameters gives them; n_iterations is the argument of
 * iterate().  A call runs the iterations [state.iterations, state.iterations + window) with
 * window = max(max_its - state.iterations, n_iterations, 0) (`||` at :182) unless it returns
 * early. */
typedef struct {
    float fx, fy, cx, cy;
    float sigma2[16];
    int32_t nlevels;
    float th2;
    int32_t n_matches, N, corr_off, inlier_off, quad_off, best_off;
    int32_t min_inliers, max_its, n_iterations;
} orbx_pnp_job;

/* mnIterations, mnBestInliers and mBestTcw (row-major), kept across calls of iterate() (in /
 * out) together with the job's best inlier bytes (mvbBestInliers): a later call may Refine on a
 * set an earlier call found.  When best_inliers > 0 the best bytes hold exactly best_inliers
 * non-zero entries (anything else is refused). */
typedef struct {
    int32_t iterations, best_inliers;
    float best_Tcw[16];
} orbx_pnp_state;

#define ORBX_PNP_REFINES_MASK 0xffffu        /* Refine() calls of this iterate()                           */
#define ORBX_PNP_REFUSED_OCTAVE (1u << 24)  /* an octave outside [0, nlevels), or nlevels outside [1, 16] */
#define ORBX_PNP_REFUSED_QUAD (1u << 25)    /* a minimal-set index outside [0, N) or repeated             */
#define ORBX_PNP_REFUSED_I (1u << 26)       /* an i outside [0, n_matches), or not increasing             */
#define ORBX_PNP_REFUSED_LIMIT (1u << 27)   /* N above max_n, the call's window above max_call_its,
                                               max_its outside [1, limit], min_inliers < 1, a negative
                                               count, a state that contradicts its best bytes          */
#define ORBX_PNP_REFUSED_RANGE (1u << 28)   /* an offset outside the arrays of the call                   */
#define ORBX_PNP_REFUSED_ANY (0x1fu << 24)
#define ORBX_PNP_QR_SINGULAR (1u << 29)     /* qr_solve left through its singular exit (:887-890)         */
#define ORBX_PNP_SVD_COMPLETED (1u << 30)   /* a singular vector came from cv::SVD's completion path      */

/* What one iterate() call gives.  found: a pose was returned, source 1 = mRefinedTcw (:235) at
 * the 1-based iteration `iteration`, source 2 = mBestTcw when the loop ended (:253, iteration =
 * mnIterations); n_inliers and Tcw (row-major 4x4) are that pose's, and all n_matches inlier bytes
 * of the job are written (vbInliers).  Not found: source, iteration, n_inliers and Tcw are 0 and
 * the inlier bytes are not touched.  n_run: the iterations this call executed (the reference
 * consumed 4 * n_run rand() values).  no_more: bNoMore.  best_inliers: mnBestInliers after the
 * call.  info: the ORBX_PNP_REFUSED_* bits; a refused job gets found = 0 and info, and nothing
 * else of its outputs, its state, its best bytes or its inlier bytes is touched.  Otherwise info
 * holds the number of Refine() calls and the two diagnostics, over the iterations the call
 * executed. */
typedef struct {
    int32_t found, source, iteration, n_run, n_inliers, no_more;
    uint32_t info;
    int32_t best_inliers;
    float Tcw[16];
} orbx_pnp_result;

/* SetRansacParameters (:121-152) in its types, host only: nMinInliers = (int)(N * epsilon) through
 * float, raised to min_inliers and to min_set; epsilon raised to (float)nMinInliers / N;
 * nIterations = 1 when nMinInliers == N, else ceil(log(1 - prob) / log(1 - pow(epsilon, 3))) in
 * double with the host's libm; both conversions to int as x86-64 does them (out of range or NaN:
 * INT_MIN); *max_its_out = max(1, min(nIterations, max_its)).  N = 0 included.
 * ORBX_ERR_INVALID: N < 0 or a NULL output; min_set != 4: ORBX_ERR_UNSUPPORTED. */
orbx_status orbx_pnp_ransac_parameters(double prob, int32_t min_inliers, int32_t max_its,
                                       int32_t min_set, float epsilon, int32_t N,
                                       int32_t* min_inliers_out, int32_t* max_its_out);

/* The minimal sets of n_its iterations (:188-201) from 4 * n_its raw rand() values in
 * [0, RAND_MAX]: four draws without replacement by swap-with-last over 0 .. N-1, restarted every
 * iteration, each draw DUtils::Random::RandomInt(0, size - 1) = int(((double)r / ((double)RAND_MAX
 * + 1.0)) * size).  ORBX_ERR_INVALID: N < 4, n_its < 0, a NULL array with n_its > 0, a value
 * outside [0, RAND_MAX]. */
orbx_status orbx_pnp_sample_quads(int32_t N, int32_t n_its, const int32_t* rand_values,
                                  int32_t* quads);

/* The largest N (max_n), iterations per call (max_call_its, also the largest max_its) and jobs a
 * call takes, and the scratch bytes a call may need at most (host only; the launcher evaluates
 * the same expressions).  NULL outputs are skipped. */
orbx_status orbx_pnp_limits(int32_t* max_n, int32_t* max_its, int32_t* max_jobs,
                            int64_t* max_scratch_bytes);

/* iterate(n_iterations) of njobs solvers at once, every array on the device, on `stream` with no
 * host step: k_pnp_hypotheses (one wave per iteration of the call: EPnP on the four sampled
 * points, then the inlier count and mask) and k_pnp_select (one wave per job: the iterations
 * walked in order against the carried best, Refine where the reference runs it, the result, the
 * inlier bytes, the state and the best bytes).  max_n >= every job's N and max_call_its >= every
 * job's window size the grids and the matcher's scratch; ncorr, nquads (quads, i.e. 4 ints each),
 * nbest_bytes and ninlier_bytes are the lengths of the arrays, and a job that points outside them
 * is refused.  d_state and d_best are in / out, d_results and d_inliers out.
 * ORBX_ERR_INVALID: m NULL, a NULL array with njobs > 0, a negative count.  max_n, max_call_its or
 * njobs above orbx_pnp_limits, or their scratch above its bound: ORBX_ERR_UNSUPPORTED.
 * njobs == 0: ORBX_OK, nothing touched.  Calls on one matcher share its scratch: one stream, or
 * serialised. */
orbx_status orbx_pnp_iterate_batch_device(
    orbx_matcher* m, const orbx_pnp_job* d_jobs, int32_t njobs, int32_t max_n,
    int32_t max_call_its, const orbx_pnp_corr* d_corr, int64_t ncorr, const int32_t* d_quads,
    int64_t nquads, orbx_pnp_state* d_state, uint8_t* d_best, int64_t nbest_bytes,
    orbx_pnp_result* d_results, uint8_t* d_inliers, int64_t ninlier_bytes, void* stream);

/* One solver from host arrays (copied to the device for the call).  The four offsets of the job
 * are ignored: corr holds job->N records, best job->N bytes (in / out), inliers job->n_matches
 * bytes, quads 4 * (state->iterations + window) ints (the call reads the window's).
 * ORBX_ERR_INVALID: a NULL argument, N, n_matches or state->iterations negative, max_its < 1; N,
 * max_its or the window above orbx_pnp_limits: ORBX_ERR_UNSUPPORTED; the checks run before the
 * device is touched, and without a GPU the call returns ORBX_ERR_DEVICE.  What the batched form
 * refuses per job comes back the same way, in res->info.  Calls from several threads run beside
 * each other, each on a device stream and staging buffer of its own. */
orbx_status orbx_pnp_iterate(const orbx_pnp_job* job, const orbx_pnp_corr* corr,
                             const int32_t* quads, orbx_pnp_state* state, uint8_t* best,
                             orbx_pnp_result* res, uint8_t* inliers, int device);

/* orbx_pnp_correspondences_batch_device and orbx_pnp_apply_batch_device, the two small kernels that
 * tie the solver to the searches around it, are declared in orbx_frame.h next to the records
 * they read and write. */

/* ---- per-kernel timing for the matcher handle ------------------------------------------
 * ORBX_MK_PROJ_RESOLVE ("k_proj_resolve") times the replay after k_proj_search, k_proj_claim or
 * k_proj_init. */
typedef enum {
    ORBX_MK_BOW = 0, ORBX_MK_TRIANGULATE, ORBX_MK_PROJ_SEARCH, ORBX_MK_PROJ_RESOLVE,
    ORBX_MK_DISTINCTIVE, ORBX_MK_BF, ORBX_MK_COUNT
} orbx_match_kernel_id;
orbx_status orbx_matcher_profile_enable(orbx_matcher* m, int on);
orbx_status orbx_matcher_profile_collect(orbx_matcher* m, double* total_ms, int64_t* launches);
const char* orbx_match_kernel_name(int id);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_MATCH_H */
