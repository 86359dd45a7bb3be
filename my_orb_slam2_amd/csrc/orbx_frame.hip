// orbx_frame.hip — per-frame geometry around the matchers (include/orbx_frame.h).
//
//   k_undistort    one lane per keypoint: cvUndistortPoints (OpenCV 3.2) in double, the
//                  same __host__ __device__ routine the host uses for ComputeImageBounds
//   k_grid         Frame::AssignFeaturesToGrid as a counting sort, one workgroup per frame:
//                  cell of every keypoint (PosInGrid, std::round half away from zero in
//                  float), per-cell LDS counts, a block scan over the 3072 cells, an atomic
//                  fill, then each cell sorted by feature index (the push_back order)
//   k_frustum      one lane per (frame, local MapPoint): Frame::isInFrustum + PredictScale, the
//                  SearchByProjection query of every MapPoint in view (SearchLocalPoints)
//   k_project      one lane per (job, MapPoint): the projection loop of the other six
//                  SearchByProjection / Fuse / SearchBySim3 modes, one template instance per mode
//   k_rgbd_depth   one lane per (frame, keypoint): Frame::ComputeStereoFromRGBD on the raw depth
//                  image (the samples are scaled, not the image), optionally fused with the
//                  undistortion of the keypoint
//   k_unproject    one lane per (frame, keypoint): Frame / KeyFrame::UnprojectStereo
//   k_close_points one workgroup per frame: the depth-sorted close-point pass of
//                  Tracking::UpdateLastFrame / CreateNewKeyFrame, a bitonic sort of
//                  (depth bits << 32 | index) keys in LDS, and NeedNewKeyFrame's close counts
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>

#include "../../include/orbx_frame.h"
#include "orbx_cv.h"
#include "orbx_device.h"
#include "orbx_host.h"
#include "orbx_math.h"

using namespace orbx;

namespace {

struct UndistParams {
    double k[8];
    double fx, fy, cx, cy, ifx, ify;
    int iters;
};

__host__ __device__ inline void undistort_pt(const UndistParams& P, float xs, float ys,
                                             float& xo, float& yo) {
    const double* k = P.k;
    double x = xs, y = ys;
    const double x0 = x = (x - P.cx) * P.ifx;
    const double y0 = y = (y - P.cy) * P.ify;
    for (int j = 0; j < P.iters; j++) {   // compensate distortion iteratively
        const double r2 = x * x + y * y;
        const double icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) /
                              (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
        const double deltaX = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x);
        const double deltaY = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y;
        x = (x0 - deltaX) * icdist;
        y = (y0 - deltaY) * icdist;
    }
    // RR = P * I = K: xx = RR00*x + RR01*y + RR02, ..., ww = 1/(0*x + 0*y + 1)
    const double xx = P.fx * x + 0.0 * y + P.cx;
    const double yy = 0.0 * x + P.fy * y + P.cy;
    const double ww = 1. / (0.0 * x + 0.0 * y + 1.0);
    xo = (float)(xx * ww);
    yo = (float)(yy * ww);
}

bool make_params(const float* K4, const float* dist, int ndist, UndistParams& P) {
    if (!K4 || !dist || (ndist != 4 && ndist != 5 && ndist != 8)) return false;
    for (int i = 0; i < 8; ++i) P.k[i] = i < ndist ? (double)dist[i] : 0.0;
    P.fx = K4[0];
    P.fy = K4[1];
    P.cx = K4[2];
    P.cy = K4[3];
    P.ifx = 1. / P.fx;
    P.ify = 1. / P.fy;
    P.iters = 5;   // distortion coefficients given (cvUndistortPoints)
    return true;
}

__global__ __launch_bounds__(256) void k_undistort(UndistParams P, const orbx_keypoint* in,
                                                   int n, orbx_keypoint* out, int copy) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    orbx_keypoint kp = in[i];
    if (!copy) undistort_pt(P, kp.x, kp.y, kp.x, kp.y);
    out[i] = kp;
}

// PosInGrid (Frame.cc:407-417): round((x - mnMinX) * inv) in float, half away from zero, then
// the reference's (int): a NaN or out-of-range coordinate becomes INT_MIN and is outside the grid
// (a bare device conversion turns NaN into 0, which is column / row 0).
__device__ inline int grid_cell(const orbx_keypoint& kp, int cols, int rows, float min_x,
                                float min_y, float inv_w, float inv_h) {
    const int px = x86_trunc(roundf((kp.x - min_x) * inv_w));
    const int py = x86_trunc(roundf((kp.y - min_y) * inv_h));
    if (px < 0 || px >= cols || py < 0 || py >= rows) return -1;
    return px * rows + py;
}

// One workgroup per frame: frame f's keypoints at kps + f*kp_stride (n_f = d_n[f] when given,
// else n), grid_off block at f*(cells+1), grid_feat at f*kp_stride.
__global__ __launch_bounds__(1024) void k_grid(const orbx_keypoint* __restrict__ kps, int n,
                                               const int32_t* __restrict__ d_n, int kp_stride,
                                               int cols, int rows, float min_x, float min_y,
                                               float inv_w, float inv_h,
                                               int32_t* __restrict__ grid_off,
                                               int32_t* __restrict__ grid_feat) {
    extern __shared__ int cnt[];   // cells + 1024 (scan partials)
    const int ncell = cols * rows, tid = threadIdx.x, f = blockIdx.x;
    if (d_n) n = min(max(d_n[f], 0), kp_stride);
    kps += (size_t)f * kp_stride;
    int32_t* off = grid_off + (size_t)f * (ncell + 1);
    int32_t* feat = grid_feat + (size_t)f * kp_stride;
    int* part = cnt + ncell;
    for (int c = tid; c < ncell; c += 1024) cnt[c] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 1024) {
        const int c = grid_cell(kps[i], cols, rows, min_x, min_y, inv_w, inv_h);
        if (c >= 0) atomicAdd(&cnt[c], 1);
    }
    __syncthreads();
    // exclusive scan: each thread sums a run of `per` cells, Hillis-Steele over the partials
    const int per = (ncell + 1023) / 1024, c0 = min(tid * per, ncell), c1 = min(c0 + per, ncell);
    int sum = 0;
    for (int c = c0; c < c1; ++c) sum += cnt[c];
    part[tid] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - sum;
    for (int c = c0; c < c1; ++c) {
        const int v = cnt[c];
        cnt[c] = run;   // becomes the fill cursor
        off[c] = run;
        run += v;
    }
    if (tid == 1023) off[ncell] = part[1023];
    __syncthreads();
    for (int i = tid; i < n; i += 1024) {
        const int c = grid_cell(kps[i], cols, rows, min_x, min_y, inv_w, inv_h);
        if (c >= 0) feat[atomicAdd(&cnt[c], 1)] = i;
    }
    __syncthreads();
    // each cell ascending by feature index (the push_back order of Frame.cc:252-256)
    for (int c = tid; c < ncell; c += 1024) {
        const int b = off[c], e = cnt[c];
        for (int k = b + 1; k < e; ++k) {
            const int v = feat[k];
            int j = k - 1;
            while (j >= b && feat[j] > v) {
                feat[j + 1] = feat[j];
                --j;
            }
            feat[j + 1] = v;
        }
    }
}

__global__ __launch_bounds__(256) void k_undistort_batch(UndistParams P,
                                                         const orbx_keypoint* in, int kp_stride,
                                                         const int32_t* d_n,
                                                         orbx_keypoint* out, int copy) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.y;
    if (i >= min(d_n[f], kp_stride)) return;
    const size_t k = (size_t)f * kp_stride + i;
    orbx_keypoint kp = in[k];
    if (!copy) undistort_pt(P, kp.x, kp.y, kp.x, kp.y);
    out[k] = kp;
}

// cvtColor(*2GRAY), OpenCV 3.2 RGB2Gray<uchar>: the three table terms summed with the
// 1 << 13 rounding constant, >> 14.  One thread per 4 output pixels.
__global__ __launch_bounds__(256) void k_gray(const uint8_t* __restrict__ src, int w, int h,
                                              size_t sstride, int scn, int rgb,
                                              uint8_t* __restrict__ dst, size_t dstride) {
    const int y = blockIdx.y;
    const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (x0 >= w) return;
    const uint8_t* s = src + (size_t)y * sstride + (size_t)x0 * scn;
    const int c0 = rgb ? 4899 : 1868, c2 = rgb ? 1868 : 4899;   // coeff of src[0], src[2]
    uint32_t out = 0;
    const int nx = min(4, w - x0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j < nx) {
            const int v = (c0 * s[j * scn] + 9617 * s[j * scn + 1] + c2 * s[j * scn + 2] + (1 << 13)) >> 14;
            out |= (uint32_t)v << (8 * j);
        }
    }
    uint8_t* d = dst + (size_t)y * dstride + x0;
    for (int j = 0; j < nx; ++j) d[j] = (uint8_t)(out >> (8 * j));
}

// Frame::isInFrustum (src/Frame.cc:285-349) with MapPoint::PredictScale (MapPoint.cc:430-444)
// and the query SearchByProjection(Frame&, vpMapPoints, th) forms from its outputs
// (ORBmatcher.cc:55-80).  The float / double steps follow the reference's types (see
// include/orbx_frame.h); the library is built with -ffp-contract=off, so every float op is
// rounded on its own as on x86.  The OpenCV forms are orbx_cv.h's.
__device__ __forceinline__ bool frustum_query(const orbx_frame_pose& F, const orbx_map_point& M,
                                              float cos_lim, float th, orbx_proj_query& q) {
    float Pc[3];
    gemm3(F.Rcw, M.pos, F.tcw, Pc);                       // Pc = mRcw*P + mtcw
    if (Pc[2] < 0.0f) return false;                       // positive depth
    const float invz = __fdiv_rn(1.0f, Pc[2]);
    const float u = pinhole_frame(F.fx, F.cx, Pc[0], invz);
    const float v = pinhole_frame(F.fy, F.cy, Pc[1], invz);
    if (u < F.min_x || u > F.max_x) return false;
    if (v < F.min_y || v > F.max_y) return false;
    const float maxD = __fmul_rn(1.2f, M.max_dist), minD = __fmul_rn(0.8f, M.min_dist);
    // PO = P - mOw; dist = cv::norm(PO), stored in a float
    const float PO[3] = {__fsub_rn(M.pos[0], F.Ow[0]), __fsub_rn(M.pos[1], F.Ow[1]),
                         __fsub_rn(M.pos[2], F.Ow[2])};
    const float dist = norm3(PO);
    if (dist < minD || dist > maxD) return false;
    // viewCos = PO.dot(Pn) / dist: / dist in double
    const float viewCos = (float)__ddiv_rn(dot3(PO, M.normal), (double)dist);
    if (viewCos < cos_lim) return false;
    const int lvl = predict_level(glibc_logf(__fdiv_rn(M.max_dist, dist)), F.log_scale_factor,
                                  F.nlevels);
    // SearchByProjection: r = RadiusByViewingCos (viewCos > 0.998 in double), * th if th != 1
    float r = (double)viewCos > 0.998 ? 2.5f : 4.0f;
    if ((double)th != 1.0) r = __fmul_rn(r, th);
    q.u = u;
    q.v = v;
    q.ur = __fsub_rn(u, __fmul_rn(F.mbf, invz));        // mTrackProjXR
    q.radius = __fmul_rn(r, F.scale[lvl]);
    q.min_level = lvl - 1;
    q.max_level = lvl;
    q.pred_level = lvl;
    q.angle = 0.0f;
    return true;
}

__global__ __launch_bounds__(256) void k_frustum(const orbx_frame_pose* __restrict__ frames,
                                                 const orbx_map_point* __restrict__ mps,
                                                 const int32_t* __restrict__ mp_off,
                                                 const uint8_t* __restrict__ skip, float cos_lim,
                                                 float th, orbx_proj_query* __restrict__ q,
                                                 int32_t* __restrict__ nvisible) {
    const int f = blockIdx.y;
    const int b = mp_off[f], e = mp_off[f + 1];
    const int i = b + blockIdx.x * 256 + threadIdx.x;
    bool vis = false;
    if (i < e) {
        orbx_proj_query out;
        vis = (!skip || !skip[i]) && frustum_query(frames[f], mps[i], cos_lim, th, out);
        if (!vis) {
            out.u = out.v = out.ur = 0.0f;
            out.radius = -1.0f;
            out.min_level = out.max_level = out.pred_level = -1;
            out.angle = 0.0f;
        }
        q[i] = out;
    }
    if (nvisible) {
        const uint64_t m = __ballot(vis);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(&nvisible[f], (int)__popcll(m));
    }
}

// ---- RGB-D: depth at the keypoints, unprojection, the close-point pass -------------------------

// Frame::ComputeStereoFromRGBD (src/Frame.cc:689-710) for keypoint slot i of frame f, on the raw
// depth image: imDepth.at<float>(v, u) truncates the raw keypoint to a pixel; the sample is
// converted as Tracking.cc:244-245 converts the image (u16: (float)raw * factor; f32: raw *
// factor when `scale`, else raw).  A pixel outside the image gives -1 / -1.  FUSED: the
// undistorted keypoint is computed here (Frame::UndistortKeyPoints) and written to kps_un.
template <bool FUSED>
__global__ __launch_bounds__(256) void k_rgbd_depth(UndistParams P, int copy,
                                                    const uint8_t* __restrict__ img, int type,
                                                    int scale, size_t row_stride,
                                                    size_t image_stride, int width, int height,
                                                    float factor, float mbf,
                                                    const orbx_keypoint* kps,
                                                    const orbx_keypoint* kps_un_in,
                                                    orbx_keypoint* kps_un_out, int kp_stride,
                                                    const int32_t* __restrict__ d_n,
                                                    float* __restrict__ u_right,
                                                    float* __restrict__ depth_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.y;
    if (i >= min(d_n[f], kp_stride)) return;
    const size_t k = (size_t)f * kp_stride + i;
    const orbx_keypoint kp = kps[k];
    float xu;
    if (FUSED) {
        orbx_keypoint ku = kp;
        if (!copy) undistort_pt(P, kp.x, kp.y, ku.x, ku.y);
        kps_un_out[k] = ku;
        xu = ku.x;
    } else {
        xu = kps_un_in[k].x;
    }
    const int col = x86_trunc(kp.x), row = x86_trunc(kp.y);
    float d = -1.0f;
    if (col >= 0 && col < width && row >= 0 && row < height) {
        const uint8_t* p = img + (size_t)f * image_stride + (size_t)row * row_stride;
        if (type == ORBX_DEPTH_U16) {
            d = __fmul_rn((float)((const uint16_t*)p)[col], factor);
        } else {
            d = ((const float*)p)[col];
            if (scale) d = __fmul_rn(d, factor);
        }
    }
    if (d > 0.0f) {
        depth_out[k] = d;
        u_right[k] = __fsub_rn(xu, __fdiv_rn(mbf, d));
    } else {
        depth_out[k] = -1.0f;
        u_right[k] = -1.0f;
    }
}

// Frame / KeyFrame::UnprojectStereo (orbx_cv.h's unproject) for every keypoint with z > 0
__global__ __launch_bounds__(256) void k_unproject(const orbx_frame_pose* __restrict__ poses,
                                                   const orbx_keypoint* __restrict__ keys,
                                                   int kp_stride, const float* __restrict__ depth,
                                                   const int32_t* __restrict__ d_n,
                                                   float* __restrict__ x3d,
                                                   uint8_t* __restrict__ valid) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.y;
    if (i >= min(d_n[f], kp_stride)) return;
    const size_t k = (size_t)f * kp_stride + i;
    const float z = depth[k];
    if (z > 0.0f) {
        float o[3];
        unproject(poses[f], keys[k].x, keys[k].y, z, o);
        x3d[3 * k] = o[0];
        x3d[3 * k + 1] = o[1];
        x3d[3 * k + 2] = o[2];
    }
    if (valid) valid[k] = z > 0.0f;
}

#define CLOSE_MAX_FEATURES 8192

// The close-point pass of Tracking::UpdateLastFrame (src/Tracking.cc:862-912) and
// CreateNewKeyFrame (:1164-1217), with NeedNewKeyFrame's close counts (:1080-1089); one
// workgroup per frame.  The features with z > 0 are sorted by (z, index), which is std::sort on
// vector<pair<float,int>>: a positive float orders as its bit pattern, so the u64 key
// (bits(z) << 32 | index) orders the pairs; slots without depth get the all-ones key and sink to
// the end.  A bitonic network over the next power of two >= n sorts them in LDS (8 bytes per
// slot, 64 KiB at 8192 features).  The loop body runs on the first V sorted entries: the break
// (z > th_depth && nPoints > min_points, nPoints = j + 1 in both branches) fires at the first
// position j >= max(L, min_points) with L = #{!(z > th_depth)}, so V = min(M, max(L,
// min_points) + 1).
__global__ __launch_bounds__(1024) void k_close_points(
    const orbx_frame_pose* __restrict__ poses, const orbx_keypoint* __restrict__ keys,
    int kp_stride, const float* __restrict__ depth, const uint8_t* __restrict__ has_point,
    const uint8_t* __restrict__ tracked, const int32_t* __restrict__ d_n, int n_one,
    float th_depth, int min_points, int32_t* __restrict__ order, int32_t* __restrict__ counts,
    uint8_t* __restrict__ create, float* __restrict__ x3d) {
    extern __shared__ unsigned long long skey[];
    const int tid = threadIdx.x, f = blockIdx.x;
    const int n = d_n ? min(max(d_n[f], 0), kp_stride) : n_one;
    const size_t base = (size_t)f * kp_stride;
    int ps = 2;   // sorted span: the power of two >= n
    while (ps < n) ps <<= 1;
    int* red = (int*)skey;   // {M, L, nTrackedClose, nNonTrackedClose} before the keys move in
    if (tid < 4) red[tid] = 0;
    __syncthreads();
    int m = 0, l = 0, tc = 0, ntc = 0;
    for (int i = tid; i < n; i += 1024) {
        const float z = depth[base + i];
        if (z > 0.0f) {
            ++m;
            if (!(z > th_depth)) ++l;
            if (z < th_depth) {
                if (tracked && tracked[base + i]) ++tc;
                else ++ntc;
            }
        }
    }
    if (m) atomicAdd(&red[0], m);
    if (l) atomicAdd(&red[1], l);
    if (tc) atomicAdd(&red[2], tc);
    if (ntc) atomicAdd(&red[3], ntc);
    __syncthreads();
    const int M = red[0], L = red[1], nTC = red[2], nNTC = red[3];
    __syncthreads();
    for (int i = tid; i < ps; i += 1024) {
        unsigned long long key = ~0ull;
        if (i < n) {
            const float z = depth[base + i];
            if (z > 0.0f) key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)i;
        }
        skey[i] = key;
    }
    __syncthreads();
    for (int k = 2; k <= ps; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (ps >> 1); t += 1024) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const unsigned long long a = skey[lo], b = skey[hi];
                if ((a > b) == ((lo & k) == 0)) {
                    skey[lo] = b;
                    skey[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    const int first = max(L, min_points);
    const int V = first >= M ? M : first + 1;
    if (tid == 0) {
        counts[4 * f] = M;
        counts[4 * f + 1] = V;
        counts[4 * f + 2] = nTC;
        counts[4 * f + 3] = nNTC;
    }
    const orbx_frame_pose& F = poses[f];
    for (int j = tid; j < M; j += 1024) {
        const unsigned long long key = skey[j];
        const int i = (int)(unsigned)key;
        order[base + j] = i;
        if (j < V) {
            create[base + j] = has_point ? !has_point[base + i] : 1;
            float o[3];
            unproject(F, keys[base + i].x, keys[base + i].y, __uint_as_float((unsigned)(key >> 32)), o);
            x3d[3 * (base + j)] = o[0];
            x3d[3 * (base + j) + 1] = o[1];
            x3d[3 * (base + j) + 2] = o[2];
        }
    }
}

// Dynamic LDS of k_close_points for a frame capacity; 64 KiB needs no more than the default
// limit, the opt-in is made once per device all the same (a no-op where it is the default).
size_t close_lds(int cap) {
    size_t p = 2;
    while (p < (size_t)cap) p <<= 1;
    return p * sizeof(unsigned long long);
}
bool close_prepare() {
    static std::mutex mu;
    static bool have[ORBX_MAX_DEVICES] = {};
    int dev = 0;
    if (!HIPOK(hipGetDevice(&dev)) || dev < 0 || dev >= ORBX_MAX_DEVICES) return false;
    std::lock_guard<std::mutex> lk(mu);
    if (!have[dev])
        have[dev] = HIPOK(hipFuncSetAttribute((const void*)k_close_points,
                                              hipFuncAttributeMaxDynamicSharedMemorySize,
                                              (int)close_lds(CLOSE_MAX_FEATURES)));
    return have[dev];
}

// ---- the projection loops of the other six SearchByProjection modes ---------------------------

// The per-MapPoint body of the reference's loop for MODE (include/orbx_frame.h lists the steps;
// ORBmatcher.cc LAST_FRAME :1402-1458, KEYFRAME :1544-1596, KF_SCW :321-390, FUSE :881-946,
// FUSE_SCW :1035-1105, SIM3 :1166-1247).  The mode is a template argument, so each instance holds
// one loop only.  key_octave / key_angle: the source feature (LAST_FRAME, KEYFRAME).
template <int MODE>
__device__ __forceinline__ bool project_query(const orbx_proj_job& J, const float* P,
                                              float min_dist, const float* Pn, float max_dist,
                                              int key_octave, float key_angle,
                                              orbx_proj_query& q) {
    constexpr bool FRAME = MODE == ORBX_PROJ_LAST_FRAME || MODE == ORBX_PROJ_KEYFRAME;
    constexpr bool NORMAL = MODE == ORBX_PROJ_KF_SCW || MODE == ORBX_PROJ_FUSE ||
                            MODE == ORBX_PROJ_FUSE_SCW;
    const orbx_frame_pose& F = J.cam;
    const int nlevels = F.nlevels;
    if (nlevels < 1 || nlevels > 16) return false;
    float Pc[3];
    if (MODE == ORBX_PROJ_SIM3) {
        float P1[3];
        gemm3(J.pre_R, P, J.pre_t, P1);
        gemm3(F.Rcw, P1, F.tcw, Pc);
    } else {
        gemm3(F.Rcw, P, F.tcw, Pc);
    }
    if (!FRAME && Pc[2] < 0.0f) return false;
    const float invz = (MODE == ORBX_PROJ_KF_SCW || MODE == ORBX_PROJ_FUSE)
                           ? __fdiv_rn(1.0f, Pc[2])
                           : (float)__ddiv_rn(1.0, (double)Pc[2]);
    if (MODE == ORBX_PROJ_LAST_FRAME && invz < 0.0f) return false;
    float u, v;
    if (FRAME) {
        u = pinhole_frame(F.fx, F.cx, Pc[0], invz);
        v = pinhole_frame(F.fy, F.cy, Pc[1], invz);
        if (u < F.min_x || u > F.max_x) return false;
        if (v < F.min_y || v > F.max_y) return false;
    } else {
        // orbx_cv.h's pinhole_kf written out, both quotients ahead of both coordinates: through
        // the calls k_project<SIM3> comes out with the operands of one packed add exchanged
        const float x = __fmul_rn(Pc[0], invz), y = __fmul_rn(Pc[1], invz);
        u = __fadd_rn(__fmul_rn(F.fx, x), F.cx);
        v = __fadd_rn(__fmul_rn(F.fy, y), F.cy);
        // KeyFrame::IsInImage
        if (!(u >= F.min_x && u < F.max_x && v >= F.min_y && v < F.max_y)) return false;
    }
    int lvl;
    if (MODE == ORBX_PROJ_LAST_FRAME) {
        lvl = key_octave;
        if (lvl < 0 || lvl >= nlevels) return false;   // the reference reads out of bounds
    } else {
        float PO[3] = {0.0f, 0.0f, 0.0f};
        float dist;
        if (MODE == ORBX_PROJ_SIM3) {
            dist = norm3(Pc);
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) PO[k] = __fsub_rn(P[k], F.Ow[k]);
            dist = norm3(PO);
        }
        const float maxD = __fmul_rn(1.2f, max_dist), minD = __fmul_rn(0.8f, min_dist);
        if (dist < minD || dist > maxD) return false;
        if (NORMAL && dot3(PO, Pn) < __dmul_rn(0.5, (double)dist)) return false;
        lvl = predict_level(glibc_logf(__fdiv_rn(max_dist, dist)), F.log_scale_factor, nlevels);
    }
    q.u = u;
    q.v = v;
    q.ur = (MODE == ORBX_PROJ_LAST_FRAME || MODE == ORBX_PROJ_FUSE)
               ? __fsub_rn(u, __fmul_rn(F.mbf, invz)) : 0.0f;
    q.radius = __fmul_rn(J.th, F.scale[lvl]);
    q.min_level = q.max_level = -1;
    if (MODE == ORBX_PROJ_KEYFRAME) {
        q.min_level = lvl - 1;
        q.max_level = lvl + 1;
    } else if (MODE == ORBX_PROJ_LAST_FRAME) {
        float tlc[3];
        gemm3(J.pre_R, F.Ow, J.pre_t, tlc);
        const bool forward = tlc[2] > J.mb && !J.mono, backward = -tlc[2] > J.mb && !J.mono;
        q.min_level = forward ? lvl : backward ? 0 : lvl - 1;
        q.max_level = forward ? -1 : backward ? lvl : lvl + 1;
    }
    q.pred_level = lvl;
    q.angle = FRAME ? key_angle : 0.0f;
    return true;
}

// One lane per (job, MapPoint), grid (ceil(max_mps / 256), njobs).  The job record is indexed by
// the block, so its loads are uniform; the 32-byte MapPoint and query go as two 16-byte accesses.
template <int MODE>
__global__ __launch_bounds__(256) void k_project(const orbx_proj_job* __restrict__ jobs,
                                                 const orbx_map_point* __restrict__ mps,
                                                 const int32_t* __restrict__ mp_off,
                                                 const orbx_keypoint* __restrict__ keys,
                                                 const uint8_t* __restrict__ skip,
                                                 orbx_proj_query* __restrict__ q,
                                                 int32_t* __restrict__ nactive) {
    constexpr bool FRAME = MODE == ORBX_PROJ_LAST_FRAME || MODE == ORBX_PROJ_KEYFRAME;
    const int j = blockIdx.y;
    const int b = mp_off[j], e = mp_off[j + 1];
    const int i = b + blockIdx.x * 256 + threadIdx.x;
    bool act = false;
    if (i < e) {
        orbx_proj_query out;
        if (!skip || !skip[i]) {
            const float4* m4 = reinterpret_cast<const float4*>(mps + i);
            const float4 a = m4[0], c = m4[1];
            const float P[3] = {a.x, a.y, a.z}, Pn[3] = {c.x, c.y, c.z};
            int oct = 0;
            float ang = 0.0f;
            if (FRAME) {
                if (MODE == ORBX_PROJ_LAST_FRAME) oct = keys[i].octave;
                ang = keys[i].angle;
            }
            act = project_query<MODE>(jobs[j], P, a.w, Pn, c.w, oct, ang, out);
        }
        float4 o0, o1;
        if (act) {
            o0 = make_float4(out.u, out.v, out.ur, out.radius);
            o1 = make_float4(__int_as_float(out.min_level), __int_as_float(out.max_level),
                             __int_as_float(out.pred_level), out.angle);
        } else {
            o0 = make_float4(0.0f, 0.0f, 0.0f, -1.0f);
            o1 = make_float4(__int_as_float(-1), __int_as_float(-1), __int_as_float(-1), 0.0f);
        }
        float4* q4 = reinterpret_cast<float4*>(q + i);
        q4[0] = o0;
        q4[1] = o1;
    }
    if (nactive) {
        const uint64_t m = __ballot(act);
        if ((threadIdx.x & 63) == 0 && m) atomicAdd(&nactive[j], (int)__popcll(m));
    }
}

bool proj_mode_ok(int32_t mode) {
    return mode == ORBX_PROJ_KF_SCW || mode == ORBX_PROJ_LAST_FRAME ||
           mode == ORBX_PROJ_KEYFRAME || mode == ORBX_PROJ_FUSE || mode == ORBX_PROJ_FUSE_SCW ||
           mode == ORBX_PROJ_SIM3;
}
constexpr int32_t PROJECT_MAX_POINTS = 1 << 24;

// The depth image arguments of the RGB-D entry points: element size, or 0 when refused.
int depth_elem(int type) { return type == ORBX_DEPTH_U16 ? 2 : type == ORBX_DEPTH_F32 ? 4 : 0; }
// Tracking.cc:244: the image is scaled when fabs(mDepthMapFactor - 1.0f) > 1e-5 or it is not
// CV_32F already
int depth_scales(int type, float factor) {
    return type != ORBX_DEPTH_F32 || std::fabs(factor - 1.0f) > 1e-5;
}

}  // namespace

extern "C" {

orbx_status orbx_cvt_color_device(const uint8_t* d_src, int32_t width, int32_t height,
                                  size_t src_stride, int32_t channels, int32_t rgb,
                                  uint8_t* d_dst, size_t dst_stride, void* stream) {
    if (width < 0 || height < 0 || (channels != 3 && channels != 4)) return ORBX_ERR_INVALID;
    if (width == 0 || height == 0) return ORBX_OK;
    if (!d_src || !d_dst || src_stride < (size_t)width * channels || dst_stride < (size_t)width)
        return ORBX_ERR_INVALID;
    hipLaunchKernelGGL(k_gray, dim3((width + 1023) / 1024, height), dim3(256), 0,
                       (hipStream_t)stream, d_src, width, height, src_stride, channels, rgb,
                       d_dst, dst_stride);
    return HIPOK(hipGetLastError()) ? ORBX_OK : ORBX_ERR_DEVICE;
}

orbx_status orbx_cvt_color(const uint8_t* src, int32_t width, int32_t height, size_t src_stride,
                           int32_t channels, int32_t rgb, uint8_t* dst, size_t dst_stride,
                           int device) {
    if (width < 0 || height < 0 || (channels != 3 && channels != 4)) return ORBX_ERR_INVALID;
    if (width == 0 || height == 0) return ORBX_OK;
    if (!src || !dst || src_stride < (size_t)width * channels || dst_stride < (size_t)width)
        return ORBX_ERR_INVALID;
    HostCall c(device);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    const size_t row = (size_t)width * channels;
    const size_t p_src = c.plan().scratch(row * height), p_dst = c.plan().scratch((size_t)width * height);
    if (!c.upload() || !HIPOK(hipMemcpy2DAsync(c.dev<uint8_t>(p_src), row, src, src_stride, row,
                                               height, hipMemcpyHostToDevice, c.st())))
        return c.finish(ORBX_ERR_DEVICE);
    orbx_status s = orbx_cvt_color_device(c.dev<uint8_t>(p_src), width, height, row, channels, rgb,
                                          c.dev<uint8_t>(p_dst), width, c.st());
    if (s == ORBX_OK && !HIPOK(hipMemcpy2DAsync(dst, dst_stride, c.dev<uint8_t>(p_dst), width,
                                                width, height, hipMemcpyDeviceToHost, c.st())))
        s = ORBX_ERR_DEVICE;
    return c.finish(s);
}

orbx_status orbx_undistort_keypoints_device(const float* K4, const float* dist, int32_t ndist,
                                            const orbx_keypoint* d_kps, int32_t n,
                                            orbx_keypoint* d_kps_un, void* stream) {
    UndistParams P;
    if (!make_params(K4, dist, ndist, P) || n < 0 || (n > 0 && (!d_kps || !d_kps_un)))
        return ORBX_ERR_INVALID;
    if (n == 0) return ORBX_OK;
    const int copy = dist[0] == 0.0f;   // Frame.cc:431: mvKeysUn = mvKeys
    hipLaunchKernelGGL(k_undistort, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, P,
                       d_kps, n, d_kps_un, copy);
    return HIPOK(hipGetLastError()) ? ORBX_OK : ORBX_ERR_DEVICE;
}

orbx_status orbx_undistort_keypoints(const float* K4, const float* dist, int32_t ndist,
                                     const orbx_keypoint* kps, int32_t n,
                                     orbx_keypoint* kps_un, int device) {
    UndistParams P;
    if (!make_params(K4, dist, ndist, P) || n < 0 || (n > 0 && (!kps || !kps_un)))
        return ORBX_ERR_INVALID;
    if (n == 0) return ORBX_OK;
    HostCall c(device);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    const size_t bytes = sizeof(orbx_keypoint) * (size_t)n;
    const size_t p_k = c.plan().in(kps, bytes), p_un = c.plan().out(kps_un, bytes);
    if (!c.upload()) return c.finish(ORBX_ERR_DEVICE);
    return c.finish(orbx_undistort_keypoints_device(K4, dist, ndist, c.dev<orbx_keypoint>(p_k), n,
                                                    c.dev<orbx_keypoint>(p_un), c.st()));
}

orbx_status orbx_image_bounds(const float* K4, const float* dist, int32_t ndist, int32_t width,
                              int32_t height, float* bounds) {
    UndistParams P;
    if (!make_params(K4, dist, ndist, P) || !bounds || width <= 0 || height <= 0)
        return ORBX_ERR_INVALID;
    if (dist[0] != 0.0f) {   // Frame.cc:463-480
        const float cx[4] = {0.0f, (float)width, 0.0f, (float)width};
        const float cy[4] = {0.0f, 0.0f, (float)height, (float)height};
        float ux[4], uy[4];
        for (int i = 0; i < 4; ++i) undistort_pt(P, cx[i], cy[i], ux[i], uy[i]);
        bounds[0] = std::min(ux[0], ux[2]);
        bounds[1] = std::max(ux[1], ux[3]);
        bounds[2] = std::min(uy[0], uy[1]);
        bounds[3] = std::max(uy[2], uy[3]);
    } else {   // :482-487
        bounds[0] = 0.0f;
        bounds[1] = (float)width;
        bounds[2] = 0.0f;
        bounds[3] = (float)height;
    }
    return ORBX_OK;
}

orbx_status orbx_assign_grid_device(const orbx_keypoint* d_kps, int32_t n, int32_t cols,
                                    int32_t rows, float min_x, float min_y, float inv_w,
                                    float inv_h, int32_t* d_grid_off, int32_t* d_grid_feat,
                                    void* stream) {
    if (n < 0 || cols <= 0 || rows <= 0 || (long long)cols * rows > 16384 - 1024 ||
        !d_grid_off || (n > 0 && (!d_kps || !d_grid_feat)))
        return ORBX_ERR_INVALID;
    const size_t lds = 4 * ((size_t)cols * rows + 1024);   // <= 64 KB: no attribute needed
    hipLaunchKernelGGL(k_grid, dim3(1), dim3(1024), lds, (hipStream_t)stream, d_kps, n,
                       (const int32_t*)nullptr, n, cols, rows, min_x, min_y, inv_w, inv_h,
                       d_grid_off, d_grid_feat);
    return HIPOK(hipGetLastError()) ? ORBX_OK : ORBX_ERR_DEVICE;
}

orbx_status orbx_assign_grid_batch_device(const orbx_keypoint* d_kps, int32_t kp_stride,
                                          const int32_t* d_n, int32_t batch, int32_t cols,
                                          int32_t rows, float min_x, float min_y, float inv_w,
                                          float inv_h, int32_t* d_grid_off,
                                          int32_t* d_grid_feat, void* stream) {
    if (batch < 0 || kp_stride < 0 || cols <= 0 || rows <= 0 ||
        (long long)cols * rows > 16384 - 1024)
        return ORBX_ERR_INVALID;
    if (batch == 0) return ORBX_OK;
    if (!d_kps || !d_n || !d_grid_off || !d_grid_feat) return ORBX_ERR_INVALID;
    const size_t lds = 4 * ((size_t)cols * rows + 1024);
    hipLaunchKernelGGL(k_grid, dim3(batch), dim3(1024), lds, (hipStream_t)stream, d_kps, 0, d_n,
                       kp_stride, cols, rows, min_x, min_y, inv_w, inv_h, d_grid_off,
                       d_grid_feat);
    return HIPOK(hipGetLastError()) ? ORBX_OK : ORBX_ERR_DEVICE;
}

orbx_status orbx_undistort_keypoints_batch_device(const float* K4, const float* dist,
                                                  int32_t ndist, const orbx_keypoint* d_kps,
                                                  int32_t kp_stride, const int32_t* d_n,
                                                  int32_t batch, orbx_keypoint* d_kps_un,
                                                  void* stream) {
    UndistParams P;
    if (!make_params(K4, dist, ndist, P) || batch < 0 || kp_stride < 0) return ORBX_ERR_INVALID;
    if (batch == 0 || kp_stride == 0) return ORBX_OK;
    if (!d_kps || !d_n || !d_kps_un || batch > 65535) return ORBX_ERR_INVALID;
    const int copy = dist[0] == 0.0f;
    hipLaunchKernelGGL(k_undistort_batch, dim3((kp_stride + 255) / 256, batch), dim3(256), 0,
                       (hipStream_t)stream, P, d_kps, kp_stride, d_n, d_kps_un, copy);
    return HIPOK(hipGetLastError()) ? ORBX_OK : ORBX_ERR_DEVICE;
}

orbx_status orbx_is_in_frustum_batch_device(const orbx_frame_pose* d_frames, int32_t nframes,
                                            const orbx_map_point* d_mps,
                                            const int32_t* d_mp_off, int32_t max_mps,
                                            const uint8_t* d_skip, float viewing_cos_limit,
                                            float th, orbx_proj_query* d_q,
                                            int32_t* d_nvisible, void* stream) {
    if (nframes < 0 || max_mps < 0 || nframes > 65535) return ORBX_ERR_INVALID;
    if (nframes == 0) return ORBX_OK;
    if (!d_frames || !d_mp_off || (max_mps > 0 && (!d_mps || !d_q))) return ORBX_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (d_nvisible && !HIPOK(hipMemsetAsync(d_nvisible, 0, 4 * (size_t)nframes, st)))
        return ORBX_ERR_DEVICE;
    if (max_mps == 0) return ORBX_OK;
    hipLaunchKernelGGL(k_frustum, dim3((max_mps + 255) / 256, nframes), dim3(256), 0, st,
                       d_frames, d_mps, d_mp_off, d_skip, viewing_cos_limit, th, d_q, d_nvisible);
    return HIPOK(hipGetLastError()) ? ORBX_OK : ORBX_ERR_DEVICE;
}

orbx_status orbx_is_in_frustum(const orbx_frame_pose* frame, const orbx_map_point* mps,
                               int32_t n, const uint8_t* skip, float viewing_cos_limit,
                               float th, orbx_proj_query* q, int32_t* nvisible, int device) {
    if (!frame || n < 0 || (n > 0 && (!mps || !q)) || frame->nlevels < 1 || frame->nlevels > 16)
        return ORBX_ERR_INVALID;
    if (n == 0) {
        if (nvisible) *nvisible = 0;
        return ORBX_OK;
    }
    HostCall c(device);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    StagePlan& p = c.plan();
    const int32_t off[2] = {0, n};
    const size_t p_f = p.in(frame, sizeof(*frame)), p_off = p.in(off, sizeof(off)),
                 p_mp = p.in(mps, sizeof(orbx_map_point) * (size_t)n),
                 p_sk = p.in_opt(skip, (size_t)n),
                 p_q = p.out(q, sizeof(orbx_proj_query) * (size_t)n), p_cnt = p.out(nvisible, 4);
    if (!c.upload()) return c.finish(ORBX_ERR_DEVICE);
    return c.finish(orbx_is_in_frustum_batch_device(
        c.dev<orbx_frame_pose>(p_f), 1, c.dev<orbx_map_point>(p_mp), c.dev<int32_t>(p_off), n,
        c.dev<uint8_t>(p_sk), viewing_cos_limit, th, c.dev<orbx_proj_query>(p_q),
        c.dev<int32_t>(p_cnt), c.st()));
}

orbx_status orbx_project_map_points_batch_device(
    int32_t mode, const orbx_proj_job* d_jobs, int32_t njobs, const orbx_map_point* d_mps,
    const int32_t* d_mp_off, int32_t max_mps, const orbx_keypoint* d_src_keys,
    const uint8_t* d_skip, orbx_proj_query* d_q, int32_t* d_nactive, void* stream) {
    if (!proj_mode_ok(mode) || njobs < 0 || njobs > 65535 || max_mps < 0 ||
        max_mps > PROJECT_MAX_POINTS)
        return ORBX_ERR_INVALID;
    if ((mode == ORBX_PROJ_LAST_FRAME || mode == ORBX_PROJ_KEYFRAME) && !d_src_keys)
        return ORBX_ERR_INVALID;
    if (njobs == 0) return ORBX_OK;
    if (!d_jobs || !d_mp_off || (max_mps > 0 && (!d_mps || !d_q))) return ORBX_ERR_INVALID;
    // the MapPoint and query records move as 16-byte accesses
    if ((((uintptr_t)d_mps) | ((uintptr_t)d_q)) & 15) return ORBX_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (d_nactive && !HIPOK(hipMemsetAsync(d_nactive, 0, 4 * (size_t)njobs, st)))
        return ORBX_ERR_DEVICE;
    if (max_mps == 0) return ORBX_OK;
    const dim3 grid((max_mps + 255) / 256, njobs), block(256);
#define ORBX_LAUNCH_PROJECT(M)                                                                  \
    case M:                                                                                     \
        hipLaunchKernelGGL(k_project<M>, grid, block, 0, st, d_jobs, d_mps, d_mp_off,           \
                           d_src_keys, d_skip, d_q, d_nactive);                                 \
        break;
    switch (mode) {
        ORBX_LAUNCH_PROJECT(ORBX_PROJ_KF_SCW)
        ORBX_LAUNCH_PROJECT(ORBX_PROJ_LAST_FRAME)
        ORBX_LAUNCH_PROJECT(ORBX_PROJ_KEYFRAME)
        ORBX_LAUNCH_PROJECT(ORBX_PROJ_FUSE)
        ORBX_LAUNCH_PROJECT(ORBX_PROJ_FUSE_SCW)
        ORBX_LAUNCH_PROJECT(ORBX_PROJ_SIM3)
    }
#undef ORBX_LAUNCH_PROJECT
    return HIPOK(hipGetLastError()) ? ORBX_OK : ORBX_ERR_DEVICE;
}

orbx_status orbx_project_map_points(int32_t mode, const orbx_proj_job* job,
                                    const orbx_map_point* mps, int32_t n,
                                    const orbx_keypoint* src_keys, const uint8_t* skip,
                                    orbx_proj_query* q, int32_t* nactive, int device) {
    if (!proj_mode_ok(mode) || !job || n < 0 || n > PROJECT_MAX_POINTS ||
        (n > 0 && (!mps || !q)))
        return ORBX_ERR_INVALID;
    const bool keyed = mode == ORBX_PROJ_LAST_FRAME || mode == ORBX_PROJ_KEYFRAME;
    if (keyed && !src_keys) return ORBX_ERR_INVALID;
    if (n == 0) {
        if (nactive) *nactive = 0;
        return ORBX_OK;
    }
    HostCall c(device);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    StagePlan& p = c.plan();
    const int32_t off[2] = {0, n};
    const size_t p_j = p.in(job, sizeof(*job)), p_off = p.in(off, sizeof(off)),
                 p_mp = p.in(mps, sizeof(orbx_map_point) * (size_t)n),
                 p_sk = p.in_opt(skip, (size_t)n),
                 p_k = p.in_opt(keyed ? src_keys : nullptr, sizeof(orbx_keypoint) * (size_t)n),
                 p_q = p.out(q, sizeof(orbx_proj_query) * (size_t)n), p_cnt = p.out(nactive, 4);
    if (!c.upload()) return c.finish(ORBX_ERR_DEVICE);
    return c.finish(orbx_project_map_points_batch_device(
        mode, c.dev<orbx_proj_job>(p_j), 1, c.dev<orbx_map_point>(p_mp), c.dev<int32_t>(p_off), n,
        c.dev<orbx_keypoint>(p_k), c.dev<uint8_t>(p_sk), c.dev<orbx_proj_query>(p_q),
        c.dev<int32_t>(p_cnt), c.st()));
}

// ---- RGB-D ---------------------------------------------------------------------------------

static orbx_status rgbd_args(int32_t depth_type, size_t row_stride, size_t image_stride,
                             int32_t width, int32_t height, int32_t kp_stride, int32_t batch) {
    const int es = depth_elem(depth_type);
    if (!es) return ORBX_ERR_UNSUPPORTED;
    if (width <= 0 || height <= 0 || kp_stride < 0 || batch < 0 || batch > 65535 ||
        row_stride < (size_t)width * es || row_stride % es || image_stride % es ||
        (batch > 1 && image_stride < row_stride * (size_t)height))
        return ORBX_ERR_INVALID;
    return ORBX_OK;
}

orbx_status orbx_compute_stereo_from_rgbd_batch_device(
    const void* d_depth, int32_t depth_type, size_t row_stride, size_t image_stride,
    int32_t width, int32_t height, float factor, float mbf, const orbx_keypoint* d_kps,
    const orbx_keypoint* d_kps_un, int32_t kp_stride, const int32_t* d_n, int32_t batch,
    float* d_u_right, float* d_depth_out, void* stream) {
    const orbx_status a = rgbd_args(depth_type, row_stride, image_stride, width, height,
                                    kp_stride, batch);
    if (a != ORBX_OK) return a;
    if (batch == 0 || kp_stride == 0) return ORBX_OK;
    if (!d_depth || !d_kps || !d_kps_un || !d_n || !d_u_right || !d_depth_out ||
        ((uintptr_t)d_depth & (depth_elem(depth_type) - 1)))
        return ORBX_ERR_INVALID;
    hipLaunchKernelGGL(k_rgbd_depth<false>, dim3((kp_stride + 255) / 256, batch), dim3(256), 0,
                       (hipStream_t)stream, UndistParams{}, 1, (const uint8_t*)d_depth,
                       depth_type, depth_scales(depth_type, factor), row_stride, image_stride,
                       width, height, factor, mbf, d_kps, d_kps_un, (orbx_keypoint*)nullptr,
                       kp_stride, d_n, d_u_right, d_depth_out);
    return HIPOK(hipGetLastError()) ? ORBX_OK : ORBX_ERR_DEVICE;
}

orbx_status orbx_rgbd_frame_geometry_batch_device(
    const float* K4, const float* dist, int32_t ndist, const void* d_depth, int32_t depth_type,
    size_t row_stride, size_t image_stride, int32_t width, int32_t height, float factor,
    float mbf, const orbx_keypoint* d_kps, int32_t kp_stride, const int32_t* d_n, int32_t batch,
    orbx_keypoint* d_kps_un, float* d_u_right, float* d_depth_out, void* stream) {
    UndistParams P;
    if (!make_params(K4, dist, ndist, P)) return ORBX_ERR_INVALID;
    const orbx_status a = rgbd_args(depth_type, row_stride, image_stride, width, height,
                                    kp_stride, batch);
    if (a != ORBX_OK) return a;
    if (batch == 0 || kp_stride == 0) return ORBX_OK;
    if (!d_depth || !d_kps || !d_kps_un || !d_n || !d_u_right || !d_depth_out ||
        ((uintptr_t)d_depth & (depth_elem(depth_type) - 1)))
        return ORBX_ERR_INVALID;
    const int copy = dist[0] == 0.0f;   // Frame.cc:431: mvKeysUn = mvKeys
    hipLaunchKernelGGL(k_rgbd_depth<true>, dim3((kp_stride + 255) / 256, batch), dim3(256), 0,
                       (hipStream_t)stream, P, copy, (const uint8_t*)d_depth, depth_type,
                       depth_scales(depth_type, factor), row_stride, image_stride, width, height,
                       factor, mbf, d_kps, (const orbx_keypoint*)nullptr, d_kps_un, kp_stride,
                       d_n, d_u_right, d_depth_out);
    return HIPOK(hipGetLastError()) ? ORBX_OK : ORBX_ERR_DEVICE;
}

orbx_status orbx_compute_stereo_from_rgbd(const void* depth, int32_t depth_type,
                                          size_t row_stride, int32_t width, int32_t height,
                                          float factor, float mbf, const orbx_keypoint* kps,
                                          const orbx_keypoint* kps_un, int32_t n,
                                          float* u_right, float* depth_out, int device) {
    const orbx_status a = rgbd_args(depth_type, row_stride, 0, width, height, n, 1);
    if (a != ORBX_OK) return a;
    if (n == 0) return ORBX_OK;
    if (!depth || !kps || !kps_un || !u_right || !depth_out) return ORBX_ERR_INVALID;
    HostCall c(device);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    StagePlan& p = c.plan();
    const size_t tight = (size_t)width * depth_elem(depth_type), kb = sizeof(orbx_keypoint) * (size_t)n;
    const size_t p_k = p.in(kps, kb), p_ku = p.in(kps_un, kb), p_n = p.in(&n, 4),
                 p_ur = p.out(u_right, 4 * (size_t)n), p_d = p.out(depth_out, 4 * (size_t)n),
                 p_img = p.scratch(tight * height);
    if (!c.upload() || !HIPOK(hipMemcpy2DAsync(c.dev<uint8_t>(p_img), tight, depth, row_stride,
                                               tight, height, hipMemcpyHostToDevice, c.st())))
        return c.finish(ORBX_ERR_DEVICE);
    return c.finish(orbx_compute_stereo_from_rgbd_batch_device(
        c.dev<uint8_t>(p_img), depth_type, tight, 0, width, height, factor, mbf,
        c.dev<orbx_keypoint>(p_k), c.dev<orbx_keypoint>(p_ku), n, c.dev<int32_t>(p_n), 1,
        c.dev<float>(p_ur), c.dev<float>(p_d), c.st()));
}

orbx_status orbx_unproject_stereo_batch_device(const orbx_frame_pose* d_poses,
                                               const orbx_keypoint* d_keys, int32_t kp_stride,
                                               const float* d_depth, const int32_t* d_n,
                                               int32_t batch, float* d_x3d, uint8_t* d_valid,
                                               void* stream) {
    if (batch < 0 || kp_stride < 0 || batch > 65535) return ORBX_ERR_INVALID;
    if (batch == 0 || kp_stride == 0) return ORBX_OK;
    if (!d_poses || !d_keys || !d_depth || !d_n || !d_x3d) return ORBX_ERR_INVALID;
    hipLaunchKernelGGL(k_unproject, dim3((kp_stride + 255) / 256, batch), dim3(256), 0,
                       (hipStream_t)stream, d_poses, d_keys, kp_stride, d_depth, d_n, d_x3d,
                       d_valid);
    return HIPOK(hipGetLastError()) ? ORBX_OK : ORBX_ERR_DEVICE;
}

orbx_status orbx_unproject_stereo(const orbx_frame_pose* pose, const orbx_keypoint* keys,
                                  const float* depth, int32_t n, float* x3d, uint8_t* valid,
                                  int device) {
    if (!pose || n < 0 || (n > 0 && (!keys || !depth || !x3d))) return ORBX_ERR_INVALID;
    if (n == 0) return ORBX_OK;
    HostCall c(device);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    StagePlan& p = c.plan();
    // x3d goes up too: slots without depth come back as the caller left them
    const size_t p_f = p.in(pose, sizeof(*pose)), p_n = p.in(&n, 4),
                 p_k = p.in(keys, sizeof(orbx_keypoint) * (size_t)n),
                 p_d = p.in(depth, 4 * (size_t)n), p_x = p.inout(x3d, 12 * (size_t)n),
                 p_v = p.out(valid, (size_t)n);
    if (!c.upload()) return c.finish(ORBX_ERR_DEVICE);
    return c.finish(orbx_unproject_stereo_batch_device(
        c.dev<orbx_frame_pose>(p_f), c.dev<orbx_keypoint>(p_k), n, c.dev<float>(p_d),
        c.dev<int32_t>(p_n), 1, c.dev<float>(p_x), c.dev<uint8_t>(p_v), c.st()));
}

orbx_status orbx_close_points_batch_device(const orbx_frame_pose* d_poses,
                                           const orbx_keypoint* d_keys, int32_t kp_stride,
                                           const float* d_depth, const uint8_t* d_has_point,
                                           const uint8_t* d_tracked, const int32_t* d_n,
                                           int32_t batch, float th_depth, int32_t min_points,
                                           int32_t* d_order, int32_t* d_counts,
                                           uint8_t* d_create, float* d_x3d, void* stream) {
    if (batch < 0 || kp_stride < 0) return ORBX_ERR_INVALID;
    if (kp_stride > CLOSE_MAX_FEATURES) return ORBX_ERR_UNSUPPORTED;
    if (batch == 0) return ORBX_OK;
    if (!d_poses || !d_n || !d_counts ||
        (kp_stride > 0 && (!d_keys || !d_depth || !d_order || !d_create || !d_x3d)))
        return ORBX_ERR_INVALID;
    if (!close_prepare()) return ORBX_ERR_DEVICE;
    hipLaunchKernelGGL(k_close_points, dim3(batch), dim3(1024), close_lds(kp_stride),
                       (hipStream_t)stream, d_poses, d_keys, kp_stride, d_depth, d_has_point,
                       d_tracked, d_n, 0, th_depth, min_points, d_order, d_counts, d_create,
                       d_x3d);
    return HIPOK(hipGetLastError()) ? ORBX_OK : ORBX_ERR_DEVICE;
}

orbx_status orbx_close_points(const orbx_frame_pose* pose, const orbx_keypoint* keys,
                              const float* depth, const uint8_t* has_point,
                              const uint8_t* tracked, int32_t n, float th_depth,
                              int32_t min_points, int32_t* order, int32_t* counts,
                              uint8_t* create, float* x3d, int device) {
    if (!pose || !counts || n < 0 || (n > 0 && (!keys || !depth || !order || !create || !x3d)))
        return ORBX_ERR_INVALID;
    if (n > CLOSE_MAX_FEATURES) return ORBX_ERR_UNSUPPORTED;
    HostCall c(device);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    StagePlan& p = c.plan();
    const size_t p_f = p.in(pose, sizeof(*pose)), p_n = p.in(&n, 4),
                 p_k = p.in(keys, sizeof(orbx_keypoint) * (size_t)n),
                 p_d = p.in(depth, 4 * (size_t)n), p_h = p.in_opt(has_point, (size_t)n),
                 p_t = p.in_opt(tracked, (size_t)n), p_c = p.out(counts, 16),
                 p_o = p.out(nullptr, 4 * (size_t)n), p_cr = p.out(nullptr, (size_t)n),
                 p_x = p.out(nullptr, 12 * (size_t)n);
    if (!c.upload()) return c.finish(ORBX_ERR_DEVICE);
    const orbx_status s = c.finish(orbx_close_points_batch_device(
        c.dev<orbx_frame_pose>(p_f), c.dev<orbx_keypoint>(p_k), n, c.dev<float>(p_d),
        c.dev<uint8_t>(p_h), c.dev<uint8_t>(p_t), c.dev<int32_t>(p_n), 1, th_depth, min_points,
        c.dev<int32_t>(p_o), c.dev<int32_t>(p_c), c.dev<uint8_t>(p_cr), c.dev<float>(p_x), c.st()));
    if (s != ORBX_OK) return s;
    // only what the pass wrote comes back: order[0, M), create / x3d [0, V)
    if (counts[0] > 0) std::memcpy(order, p.host<int32_t>(p_o), 4 * (size_t)counts[0]);
    if (counts[1] > 0) {
        std::memcpy(create, p.host<uint8_t>(p_cr), (size_t)counts[1]);
        std::memcpy(x3d, p.host<float>(p_x), 12 * (size_t)counts[1]);
    }
    return s;
}

}  // extern "C"
