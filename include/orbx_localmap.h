/* orbx_localmap.h — Tracking::UpdateLocalMap (src/Tracking.cc:1288-1442) on the device.
 *
 * Between TrackWithMotionModel's pose fit and TrackLocalMap the reference rebuilds the frame's
 * local map: UpdateLocalKeyFrames (:1331-1442: every MapPoint of the frame votes for the keyframes
 * that observe it, the voted keyframes form the list, each adds one covisible neighbour, one child
 * and its parent) and UpdateLocalPoints (:1299-1322: the first occurrences of the MapPoints of those
 * keyframes).  The walk is integer and order-dependent; it is restated exactly over a CSR snapshot
 * of the map, one workgroup per frame, and writes the block orbx_is_in_frustum_batch_device,
 * the projection search, orbx_matches_to_features_batch_device and
 * orbx_pose_optimization_batch_device read, so a tracked frame never leaves the device.
 *
 * The records and descriptors that walk reads are local mapping's results:
 * MapPoint::UpdateNormalAndDepth and MapPoint::ComputeDistinctiveDescriptors
 * (src/MapPoint.cc:252-392), restated over the same snapshot by orbx_refresh_map_points* below.
 */
#ifndef ORBX_LOCALMAP_H
#define ORBX_LOCALMAP_H

#include "orbx.h"
#include "orbx_frame.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The map as UpdateLocalMap reads it.  A keyframe is a slot 0..n_kf-1, a MapPoint an id
 * 0..n_mp-1.  The struct lives on the host; every pointer is a device pointer for the *_device
 * form and a host pointer for the host-array form.  The library owns none of it: build it once per
 * map state and share it between the frames of a batch.  An array whose count is 0 may be any
 * non-NULL pointer.
 *
 *   kf_order[n_kf]        the slot's rank in std::map<KeyFrame*, ...> iteration order (a C++
 *                         caller ranks by pointer value): a permutation of 0..n_kf-1.
 *                         keyframeCounter (:1334) is iterated in this order, so this is where
 *                         pointer order decides the list and the reference keyframe
 *   kf_bad[n_kf]          KeyFrame::isBad()
 *   kf_parent[n_kf]       GetParent() as a slot, or -1
 *   kf_cov_off[n_kf+1], kf_cov[n_cov]
 *                         mvpOrderedConnectedKeyFrames as slots; the first min(10, len) of a row
 *                         are read, as GetBestCovisibilityKeyFrames(10) returns them
 *                         (KeyFrame.cc:178-186)
 *   kf_child_off[n_kf+1], kf_child[n_child]
 *                         mspChildrens in the order the std::set iterates it: ascending kf_order
 *                         (the caller sorts)
 *   kf_mp_off[n_kf+1], kf_mp[n_kfmp]
 *                         GetMapPointMatches(): a MapPoint id or -1 per feature, in feature order
 *   mp_bad[n_mp]          MapPoint::isBad()
 *   mp_obs_off[n_mp+1], mp_obs[n_obs]
 *                         GetObservations() as slots, in any order (votes are integer sums); a
 *                         temporal MapPoint (Tracking::UpdateLastFrame) has an empty row
 *   mp_rec[n_mp]          the record orbx_is_in_frustum* reads */
typedef struct orbx_map_view {
    int32_t n_kf, n_mp;
    int32_t n_cov, n_child, n_kfmp, n_obs;
    const int32_t* kf_order;
    const uint8_t* kf_bad;
    const int32_t* kf_parent;
    const int32_t* kf_cov_off;
    const int32_t* kf_cov;
    const int32_t* kf_child_off;
    const int32_t* kf_child;
    const int32_t* kf_mp_off;
    const int32_t* kf_mp;
    const uint8_t* mp_bad;
    const int32_t* mp_obs_off;
    const int32_t* mp_obs;
    const orbx_map_point* mp_rec;
} orbx_map_view;

/* The visited set of a frame (mnTrackReferenceForFrame of the keyframes) is one bit per slot in
 * LDS: 16 KiB. */
#define ORBX_LOCALMAP_MAX_KF 131072
#define ORBX_LOCALMAP_MAX_FEAT 32768

/* d_info[f] */
#define ORBX_LOCALMAP_KEPT (1u << 0)       /* nobody voted (:1355): the list that came in was used */
#define ORBX_LOCALMAP_CAP_KF (1u << 8)     /* refused: the keyframe list would exceed cap_kf */
#define ORBX_LOCALMAP_CAP_MP (1u << 9)     /* refused: locals + extras would exceed cap_mp */
#define ORBX_LOCALMAP_BAD_INDEX (1u << 10) /* refused: an index read from the caller's arrays is out of range */
#define ORBX_LOCALMAP_REFUSED_ANY (7u << 8)

/* UpdateLocalMap for every frame f of a batch, one launch on the caller's stream; allocates
 * nothing (graph-capturable).
 *
 * In: frame f's mvpMapPoints as MapPoint ids (-1: none) at d_feat_mp + f*feat_stride, d_nfeat[f]
 * of them; d_outlier (optional, same layout): a feature flagged here counts as already nulled
 * (Tracking.cc:955-975).  d_local_kf (frame f at f*cap_kf), d_n_local_kf[f] and d_ref_kf[f] are
 * in/out: mvpLocalKeyFrames and mpReferenceKF as slots.
 *
 * UpdateLocalKeyFrames: a feature whose MapPoint isBad() becomes -1 in d_mp_of_feat (:1350) and
 * casts no vote.  Nobody voted: the list and the reference keyframe stay as they came in and
 * ORBX_LOCALMAP_KEPT is set.  Otherwise the voted keyframes that are not bad, in kf_order, are the
 * list; the reference keyframe is the first of them with the strictly largest count (all bad: the
 * list is empty and d_ref_kf[f] stays).  The extension loop (:1385-1435) runs over those first
 * keyframes only: it stops once the list holds more than 80; per keyframe it adds the first of the
 * first 10 neighbours that is neither bad nor listed, the first child that is neither bad nor
 * listed, and the parent if it is not listed (bad or not) -- and then leaves the loop, as the
 * reference's `break` at :1431 does.
 *
 * UpdateLocalPoints: the local keyframes in list order, their features in feature order; every
 * MapPoint that is present, not bad and not seen before is appended: d_local_mp[f*cap_mp + k],
 * k < n_local = d_n_local_mp[2f].
 *
 * The block for TrackLocalMap, cap_mp slots at f*cap_mp of d_mps / d_skip / d_local_mp: the local
 * points' records (mp_rec), then the extras -- the frame's own MapPoints that are not local
 * (temporal points, points only bad keyframes observe), in feature order, one slot per id --
 * d_n_local_mp[2f+1] = n_local + n_extra; then zeroed records (d_local_mp: the extras' ids after
 * the locals', then -1).  d_skip is 1 for a local point a
 * feature of the frame already holds (mnLastFrameSeen == mnId, :1261), for every extra and for the
 * tail.  d_mp_of_feat[f*feat_stride + i]: the block index of feature i's MapPoint, or -1 (-1 also
 * for d_nfeat[f] <= i < feat_stride, so whole strides can be walked).  With
 * d_mp_off[f] = f*cap_mp the block feeds the projection, the search,
 * orbx_matches_to_features_batch_device(d_prior = d_mp_of_feat) and PoseOptimization as it is.
 *
 * Refusals are per frame, in d_info[f] alone; a refused frame's other outputs are untouched.
 * CAP_KF / CAP_MP as above.  BAD_INDEX: every index is range-checked before it is used as an
 * address -- d_nfeat[f] outside [0, feat_stride], kf_order not a permutation, a MapPoint id below
 * -1 or >= n_mp, a slot outside [0, n_kf) (parent: below -1), a row whose offsets decrease or
 * leave its array, d_n_local_kf[f] outside [0, cap_kf] or a kept list naming a slot twice.  Only
 * the rows the frame's walk reads are looked at.
 *
 * ORBX_ERR_INVALID: a NULL map or required pointer (d_outlier alone is optional), a negative
 * count, feat_stride > ORBX_LOCALMAP_MAX_FEAT, scratch_bytes below
 * orbx_update_local_map_scratch_bytes(...).  ORBX_ERR_UNSUPPORTED: n_kf > ORBX_LOCALMAP_MAX_KF or
 * nframes > 65535.  nframes == 0: ORBX_OK, nothing launched.  Without a GPU: ORBX_ERR_DEVICE. */
orbx_status orbx_update_local_map_batch_device(
    const orbx_map_view* map, int32_t nframes, const int32_t* d_feat_mp, int32_t feat_stride,
    const int32_t* d_nfeat, const uint8_t* d_outlier, int32_t cap_kf, int32_t cap_mp,
    int32_t* d_local_kf, int32_t* d_n_local_kf, int32_t* d_ref_kf, int32_t* d_local_mp,
    int32_t* d_n_local_mp, orbx_map_point* d_mps, uint8_t* d_skip, int32_t* d_mp_of_feat,
    uint32_t* d_info, void* d_scratch, size_t scratch_bytes, void* stream);

/* Per frame: two int32 rows of n_kf (votes by rank, rank -> slot), two of n_mp (first-occurrence
 * key, block index), two of cap_kf + 2 (the list, the rows' chunk prefix), each rounded up to 256
 * bytes.  0 for negative arguments. */
size_t orbx_update_local_map_scratch_bytes(int32_t n_kf, int32_t n_mp, int32_t nframes,
                                           int32_t cap_kf, int32_t cap_mp);

/* One frame, host arrays (the view's pointers are host pointers; everything is copied to the
 * device for the call).  local_kf [cap_kf], n_local_kf, ref_kf: in/out.  local_mp / mps / skip:
 * cap_mp entries; n_local_mp: 2; mp_of_feat: nfeat.  The argument checks run before the device is
 * touched (ORBX_ERR_INVALID / ORBX_ERR_UNSUPPORTED as above; a NULL array is accepted where its
 * count is 0); without a GPU: ORBX_ERR_DEVICE. */
orbx_status orbx_update_local_map(const orbx_map_view* map, const int32_t* feat_mp, int32_t nfeat,
                                  const uint8_t* outlier, int32_t cap_kf, int32_t cap_mp,
                                  int32_t* local_kf, int32_t* n_local_kf, int32_t* ref_kf,
                                  int32_t* local_mp, int32_t* n_local_mp, orbx_map_point* mps,
                                  uint8_t* skip, int32_t* mp_of_feat, uint32_t* info, int device);

/* What SearchByProjection(mCurrentFrame, mvpLocalMapPoints, th) needs next to the block, for every
 * frame of a batch: the descriptor of each block entry and the features the search may not take.
 *   d_qdesc[(f*cap_mp + k)*32 ...]  = d_mp_desc[id*32 ...] (MapPoint::GetDescriptor()) of the block's
 *       id k < d_n_local_mp[2f+1]; 32 zero bytes for the tail and for an id outside [0, n_mp)
 *   d_claimed[f*feat_stride + i] = 1 where feature i < d_nfeat[f] holds a MapPoint with
 *       Observations() > 0 (ORBmatcher.cc:90-92): d_mp_of_feat names a block entry whose id has a
 *       non-empty mp_obs row; else 0.  An index out of range claims nothing.
 * d_local_mp / d_n_local_mp / d_mp_of_feat as orbx_update_local_map_batch_device wrote them.
 * d_mp_desc and d_qdesc are 4-byte aligned.  ORBX_ERR_INVALID: a NULL pointer, a negative count,
 * feat_stride > ORBX_LOCALMAP_MAX_FEAT, nframes > 65535, a misaligned descriptor array. */
orbx_status orbx_local_map_search_inputs_batch_device(
    const orbx_map_view* map, const uint8_t* d_mp_desc, int32_t nframes, const int32_t* d_local_mp,
    const int32_t* d_n_local_mp, int32_t cap_mp, const int32_t* d_mp_of_feat, int32_t feat_stride,
    const int32_t* d_nfeat, uint8_t* d_qdesc, uint8_t* d_claimed, void* stream);

/* ---- MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:346-392) and
 * MapPoint::ComputeDistinctiveDescriptors (:252-313) over the view: what local mapping writes
 * after every change of a point's observations, and what the calls above read (mp_rec, d_mp_desc).
 *
 * The arrays the view lacks.  Device pointers for the *_device form, host pointers otherwise.
 *   mp_obs_feat[n_obs]  parallel to mp_obs: the size_t of mObservations, the feature index in
 *                       that keyframe
 *   mp_ref_kf[n_mp]     mpRefKF as a slot
 *   kf_pose[n_kf]       the keyframe's pose; Ow, nlevels and scale[] are read
 *   kf_keys, kf_desc    mvKeysUn and mDescriptors (32 bytes per feature, 4-byte aligned), both
 *                       indexed kf_mp_off[slot] + feature: an orbx_kf_db whose keyframe k is slot k
 *                       passes its keys / desc as they are */
typedef struct orbx_map_refresh_inputs {
    const int32_t* mp_obs_feat;
    const int32_t* mp_ref_kf;
    const orbx_frame_pose* kf_pose;
    const orbx_keypoint* kf_keys;
    const uint8_t* kf_desc;
} orbx_map_refresh_inputs;

/* what */
#define ORBX_REFRESH_NORMAL_DEPTH 1u
#define ORBX_REFRESH_DESCRIPTOR 2u
/* the longest observation row a call can take: ORBX_MAX_OBSERVATIONS of orbx_match.h */
#define ORBX_REFRESH_MAX_OBS 256

/* d_info[i] */
#define ORBX_REFRESH_SKIPPED_BAD (1u << 0) /* mp_bad[id] (:354, :261): nothing written */
#define ORBX_REFRESH_NO_OBS (1u << 1)      /* an empty row (:361, :266): nothing written */
#define ORBX_REFRESH_DESC_KEPT (1u << 2)   /* every observing keyframe is bad (:279): the descriptor stays */
#define ORBX_REFRESH_CAP_OBS (1u << 8)     /* refused: the row is longer than max_obs */
#define ORBX_REFRESH_BAD_INDEX (1u << 10)  /* refused: an index read from the caller's arrays is out of range */
#define ORBX_REFRESH_REFUSED_ANY (5u << 8)

/* Refreshes the MapPoints d_ids[0..n), one wave each, in one launch on the caller's stream;
 * allocates nothing (graph-capturable).  Of the view n_kf, n_mp, n_kfmp, n_obs, kf_order, kf_bad,
 * kf_mp_off, mp_bad, mp_obs_off and mp_obs are read; its other pointers may be NULL.  An id may
 * repeat: the call reads nothing that it writes.
 *
 * Per point: mp_bad[id] -> SKIPPED_BAD; an empty row -> NO_OBS; otherwise the row is walked in
 * ascending kf_order of its keyframes, the order std::map<KeyFrame*, size_t> iterates it in (the
 * kernel sorts it; rows of mp_obs stay in any order).
 *   ORBX_REFRESH_NORMAL_DEPTH  d_mp_rec[id].normal / min_dist / max_dist (pos is read there and
 *       never written; d_mp_rec may equal map->mp_rec).  Every keyframe of the row counts, bad or
 *       not: normali = pos - Ow_i, normal += normali * (float)(1.0 / cv::norm(normali)) (the norm
 *       kept in double; product and sum rounded separately), normal * (float)(1.0 / n) at the end
 *       (a copy for n == 1).  max_dist = (float)cv::norm(pos - Ow_ref) * scale_ref[level],
 *       min_dist = max_dist / scale_ref[nlevels_ref - 1], level the octave of the reference
 *       keyframe's feature -- of its feature 0 when the reference keyframe is not in the row, as
 *       std::map::operator[] on the copy yields.
 *   ORBX_REFRESH_DESCRIPTOR    d_mp_desc[id*32 ..): of the descriptors of the row's keyframes that
 *       are not bad, in that order, the first whose median distance vDists[(N-1)/2] to all of
 *       them is least.  None left: nothing is written and DESC_KEPT is set.
 *
 * Refusals are per point, in d_info[i] alone; nothing of a refused point is written.  CAP_OBS: the
 * row is longer than max_obs.  BAD_INDEX, whatever `what` asks for: an id outside [0, n_mp); a row
 * whose offsets decrease or leave mp_obs; a slot (mp_ref_kf's too) or a kf_order rank outside
 * [0, n_kf); two entries of a row with the same slot or rank; a feature index outside its
 * keyframe's kf_mp_off row (index 0 of an empty reference keyframe too) or a kf_mp_off row that
 * leaves [0, n_kfmp]; the reference keyframe's nlevels outside [1, 16] or its feature's octave
 * outside [0, nlevels).  Every index is checked before it is used as an address.
 *
 * max_obs, in [1, ORBX_REFRESH_MAX_OBS], sizes the LDS of a wave and so the waves per workgroup.
 * ORBX_ERR_INVALID: a NULL map, inputs or required pointer, a negative count, `what` without a
 * bit or with an unknown one, max_obs out of range, kf_desc or d_mp_desc not 4-byte aligned.
 * ORBX_ERR_UNSUPPORTED: n_kf > ORBX_LOCALMAP_MAX_KF.  n == 0: ORBX_OK, nothing launched.
 * Without a GPU: ORBX_ERR_DEVICE. */
orbx_status orbx_refresh_map_points_batch_device(const orbx_map_view* map,
                                                 const orbx_map_refresh_inputs* in,
                                                 const int32_t* d_ids, int32_t n, uint32_t what,
                                                 int32_t max_obs, orbx_map_point* d_mp_rec,
                                                 uint8_t* d_mp_desc, uint32_t* d_info, void* stream);

/* Host arrays: mp_rec [n_mp] and mp_desc [n_mp*32] in/out, info [n] out; everything is copied to
 * the device for the call.  The argument checks run before the device is touched (as above; a NULL
 * array is accepted where its count is 0); without a GPU: ORBX_ERR_DEVICE. */
orbx_status orbx_refresh_map_points(const orbx_map_view* map, const orbx_map_refresh_inputs* in,
                                    const int32_t* ids, int32_t n, uint32_t what, int32_t max_obs,
                                    orbx_map_point* mp_rec, uint8_t* mp_desc, uint32_t* info,
                                    int device);

#ifdef __cplusplus
}
#endif
#endif
