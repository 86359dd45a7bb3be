// orbx_rectify.hip — stereo rectification ahead of the stereo frame (include/orbx_frame.h):
// cv::initUndistortRectifyMap once per camera on the host, cv::remap(INTER_LINEAR,
// BORDER_CONSTANT 0) per frame on the device (Examples/Stereo/stereo_euroc.cc:96-98, :136-137).
//
//   k_remap   one lane per 4 consecutive destination pixels of one row, looping over a chunk of
//             REMAP_CHUNK images: the lane's four map entries (32 bytes) are read once into
//             registers and reused for every image of the chunk, so the map (8 B per pixel
//             against 1 B read + 1 B written per image) costs 1 B per pixel per image.
//
// The device map, 8 bytes per destination pixel, built by the host at create time from the
// fixed-point conversion of cv::remap (orbx_remap_fixed_point):
//   word 0   Xc | dx << 15 | Yc << 16 | dy << 31    Xc = clamp(X, 0, src_w - 1), dx = clamp(X + 1)
//                                                   - Xc (0 or 1); rows likewise
//   word 1   wx0 | wx1 << 8 | wy0 << 16 | wy1 << 24 the 1-D weights 32 - a, a, 32 - b, b, each 0
//                                                   when its column / row is outside the source
// A tap is outside exactly when its row or its column is, so zeroing the 1-D weight zeroes the
// tap (BORDER_CONSTANT 0), and every address is inside the source whatever the map held: a NaN
// map entry converts to X = Y = -32768 on the host, i.e. address 0 and four zero weights.  The
// kernel has one form for inliers and border pixels.
//   dst = (wy0 * (wx0*v00 + wx1*v01) + wy1 * (wx0*v10 + wx1*v11) + 512) >> 10
// is the closed form of OpenCV's (sum v*w + (1 << 14)) >> 15 (all integers, any order).
//
// Source access.  With DESIGN §4's texture-addresser model (about 2.4 cycles per 64-byte sector
// per load instruction) what counts is the number of load instructions: a wave's load covers
// 64 lanes x 4 pixels = about 256 source bytes of one or two rows, 4-6 sectors, whatever its
// width.  Byte loads need 16 of them per image (4 taps x 4 pixels); measured, that form ran at
// 6x its share of bytes (1.11 ms for 512 EuRoC pairs).  The kernel therefore reads, where a
// lane's four pixels fit it, one 8-byte window per source row (3 rows: a lane's group may step
// one row), at any byte address (no aligned-dword + v_alignbyte realignment: base addresses and
// strides are arbitrary, so the alignment would change per row and image), and falls back to
// the byte gather per lane for arbitrary maps.  See k_remap.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/orbx_frame.h"
#include "orbx_host.h"
#include "orbx_math.h"

using namespace orbx;

#define REMAP_CHUNK 8

struct orbx_rectifier {
    int device = 0;
    int dst_w = 0, dst_h = 0, src_w = 0, src_h = 0;
    int pitch = 0;          // map entries per row: dst_w rounded up to 4 (padding: zero weights)
    uint2* d_map = nullptr;
};

namespace {

struct RemapSide {
    const uint4* map;
    const uint8_t* src;
    uint8_t* dst;
    uint32_t srs, drs;      // row strides (an image's rows span < 4 GiB, checked by the caller)
    size_t sis, dis;        // image strides
};

__device__ __forceinline__ uint32_t remap_px(const uint8_t* __restrict__ s, uint32_t o0,
                                             uint32_t o1, uint32_t dx, uint32_t w) {
    const uint32_t v00 = s[o0], v01 = s[o0 + dx], v10 = s[o1], v11 = s[o1 + dx];
    const uint32_t wx0 = w & 0xff, wx1 = (w >> 8) & 0xff, wy0 = (w >> 16) & 0xff, wy1 = w >> 24;
    const uint32_t h0 = wx0 * v00 + wx1 * v01, h1 = wx0 * v10 + wx1 * v11;
    return (wy0 * h0 + wy1 * h1 + 512u) >> 10;
}

// 8 source bytes at any address (the compiler picks the load: one dwordx2 where the target
// allows unaligned access, as gfx950 under HSA does)
__device__ __forceinline__ uint2 load_window(const uint8_t* __restrict__ p) {
    uint2 v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

__device__ __forceinline__ void store_px4(uint8_t* __restrict__ d, uint32_t out, int nx) {
    if (nx == 4 && ((uintptr_t)d & 3u) == 0) {
        *(uint32_t*)d = out;
    } else {
        d[0] = (uint8_t)out;
        if (nx > 1) d[1] = (uint8_t)(out >> 8);
        if (nx > 2) d[2] = (uint8_t)(out >> 16);
        if (nx > 3) d[3] = (uint8_t)(out >> 24);
    }
}

// grid (ceil(dst_w / 256), ceil(dst_h / 4), sides * nchunk), block (64, 4).  blockIdx.z <
// nchunk: side 0 (left), else side 1; a chunk never mixes the two maps.
//
// Two forms, chosen per lane from the footprint of its own four map entries:
//   window  the taps of the four pixels lie in 8 consecutive source columns of 3 consecutive
//           rows (every lane of a smooth map near unit scale, a row step inside the group
//           included): 3 loads of 8 bytes per image; v_perm_b32 picks each pixel's two
//           horizontal taps of a row, v_dot4 applies the column weights, and the row weights are
//           spread over the three rows (0 for the row a pixel does not use)
//   gather  anything else (and sources narrower than 8 columns): 4 byte loads per pixel
__global__ __launch_bounds__(256) void k_remap(RemapSide L, RemapSide R, int dst_w, int dst_h,
                                               int src_w, int src_h, int pitch4, int batch,
                                               int nchunk) {
    const bool right = (int)blockIdx.z >= nchunk;
    const int chunk = (int)blockIdx.z - (right ? nchunk : 0);
    const uint4* __restrict__ map = right ? R.map : L.map;
    const uint8_t* __restrict__ src = right ? R.src : L.src;
    uint8_t* __restrict__ dst = right ? R.dst : L.dst;
    const uint32_t srs = right ? R.srs : L.srs, drs = right ? R.drs : L.drs;
    const size_t sis = right ? R.sis : L.sis, dis = right ? R.dis : L.dis;

    const int g = blockIdx.x * 64 + threadIdx.x;      // group of 4 pixels
    const int x0 = g * 4, y = blockIdx.y * 4 + threadIdx.y;
    if (x0 >= dst_w || y >= dst_h) return;
    const uint4* mp = map + ((size_t)y * pitch4 + g) * 2;
    const uint4 m0 = mp[0], m1 = mp[1];
    const uint32_t e[4] = {m0.x, m0.z, m1.x, m1.z}, w[4] = {m0.y, m0.w, m1.y, m1.w};
    const uint32_t doff = (uint32_t)y * drs + (uint32_t)x0;
    const int nx = min(4, dst_w - x0);
    const int i0 = chunk * REMAP_CHUNK, i1 = min(batch, i0 + REMAP_CHUNK);

    uint32_t xc[4], yc[4], dx[4], dy[4];
    uint32_t xmin = 0x7fffu, xmax = 0, ymin = 0x7fffu, ymax = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        xc[j] = e[j] & 0x7fffu;
        dx[j] = (e[j] >> 15) & 1u;
        yc[j] = (e[j] >> 16) & 0x7fffu;
        dy[j] = e[j] >> 31;
        xmin = min(xmin, xc[j]);
        xmax = max(xmax, xc[j] + dx[j]);
        ymin = min(ymin, yc[j]);
        ymax = max(ymax, yc[j] + dy[j]);
    }
    // the window starts at xl <= xmin and ends inside the row: xl + 7 <= src_w - 1
    const uint32_t xl = min(xmin, (uint32_t)max(src_w - 8, 0));
    if (src_w >= 8 && xmax - xl <= 7u && ymax - ymin <= 2u) {
        uint32_t ow[3], sel[4], wr[4][3];
#pragma unroll
        for (int r = 0; r < 3; ++r) ow[r] = min(ymin + r, (uint32_t)(src_h - 1)) * srs + xl;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t k0 = xc[j] - xl, rt = yc[j] - ymin, rb = rt + dy[j];
            sel[j] = k0 | (k0 + dx[j]) << 8 | 0x0c0c0000u;      // bytes k0, k0 + dx, 0, 0
            const uint32_t wy0 = (w[j] >> 16) & 0xff, wy1 = w[j] >> 24;
#pragma unroll
            for (int r = 0; r < 3; ++r)
                wr[j][r] = (rt == (uint32_t)r ? wy0 : 0u) + (rb == (uint32_t)r ? wy1 : 0u);
        }
        for (int i = i0; i < i1; ++i) {
            const uint8_t* __restrict__ s = src + (size_t)i * sis;
            const uint2 r0 = load_window(s + ow[0]), r1 = load_window(s + ow[1]),
                        r2 = load_window(s + ow[2]);
            uint32_t out = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t wx = w[j] & 0xffffu;             // bytes wx0, wx1, 0, 0
                const uint32_t h0 = __builtin_amdgcn_udot4(__builtin_amdgcn_perm(r0.y, r0.x, sel[j]), wx, 0u, false);
                const uint32_t h1 = __builtin_amdgcn_udot4(__builtin_amdgcn_perm(r1.y, r1.x, sel[j]), wx, 0u, false);
                const uint32_t h2 = __builtin_amdgcn_udot4(__builtin_amdgcn_perm(r2.y, r2.x, sel[j]), wx, 0u, false);
                out |= ((wr[j][0] * h0 + wr[j][1] * h1 + wr[j][2] * h2 + 512u) >> 10) << (8 * j);
            }
            store_px4(dst + (size_t)i * dis + doff, out, nx);
        }
        return;
    }
    uint32_t o0[4], o1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        o0[j] = yc[j] * srs + xc[j];
        o1[j] = o0[j] + dy[j] * srs;
    }
    for (int i = i0; i < i1; ++i) {
        const uint8_t* __restrict__ s = src + (size_t)i * sis;
        uint32_t out = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) out |= remap_px(s, o0[j], o1[j], dx[j], w[j]) << (8 * j);
        store_px4(dst + (size_t)i * dis + doff, out, nx);
    }
}

inline int sat_short(int v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }

orbx_status side_args(const orbx_rectifier* r, const uint8_t* d_src, size_t srs, size_t sis,
                      uint8_t* d_dst, size_t drs, size_t dis, int32_t batch) {
    if (!r || !d_src || !d_dst || batch <= 0 || srs < (size_t)r->src_w || drs < (size_t)r->dst_w ||
        (batch > 1 && (sis < srs * (size_t)(r->src_h - 1) + (size_t)r->src_w ||
                       dis < drs * (size_t)(r->dst_h - 1) + (size_t)r->dst_w)))
        return ORBX_ERR_INVALID;
    // the kernel's 32-bit offsets inside one image
    if (srs * (size_t)r->src_h > 0xffffffffull || drs * (size_t)r->dst_h > 0xffffffffull)
        return ORBX_ERR_UNSUPPORTED;
    return ORBX_OK;
}

RemapSide make_side(const orbx_rectifier* r, const uint8_t* d_src, size_t srs, size_t sis,
                    uint8_t* d_dst, size_t drs, size_t dis) {
    RemapSide s;
    s.map = (const uint4*)r->d_map;
    s.src = d_src;
    s.dst = d_dst;
    s.srs = (uint32_t)srs;
    s.drs = (uint32_t)drs;
    s.sis = sis;
    s.dis = dis;
    return s;
}

orbx_status launch(const orbx_rectifier* r, const RemapSide& L, const RemapSide& R, int sides,
                   int32_t batch, void* stream) {
    const int nchunk = (batch + REMAP_CHUNK - 1) / REMAP_CHUNK;
    if ((long long)nchunk * sides > 65535) return ORBX_ERR_UNSUPPORTED;
    if (!HIPOK(hipSetDevice(r->device))) return ORBX_ERR_DEVICE;
    hipLaunchKernelGGL(k_remap, dim3((r->dst_w + 255) / 256, (r->dst_h + 3) / 4, nchunk * sides),
                       dim3(64, 4), 0, (hipStream_t)stream, L, R, r->dst_w, r->dst_h,
                       r->src_w, r->src_h, r->pitch / 4, batch, nchunk);
    return HIPOK(hipGetLastError()) ? ORBX_OK : ORBX_ERR_DEVICE;
}

}  // namespace

extern "C" {

int32_t orbx_remap_images_per_chunk(void) { return REMAP_CHUNK; }

orbx_status orbx_init_undistort_rectify_map(const double K[9], const double* dist, int32_t ndist,
                                            const double* R9_or_null, const double P33[9],
                                            int32_t width, int32_t height, float* map1,
                                            float* map2) {
    if (!K || !P33 || !map1 || !map2 || width <= 0 || height <= 0 || ndist < 0 ||
        (ndist > 0 && !dist))
        return ORBX_ERR_INVALID;
    if (ndist == 12 || ndist == 14) return ORBX_ERR_UNSUPPORTED;   // thin prism / tilt terms
    if (ndist != 4 && ndist != 5 && ndist != 8) return ORBX_ERR_INVALID;
    double d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < ndist; ++i) d[i] = dist[i];
    const double k1 = d[0], k2 = d[1], p1 = d[2], p2 = d[3], k3 = d[4], k4 = d[5], k5 = d[6],
                 k6 = d[7];
    const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
    static const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const double* R = R9_or_null ? R9_or_null : I;
    double M[3][3], iR[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            M[i][j] = P33[3 * i] * R[j] + P33[3 * i + 1] * R[3 + j] + P33[3 * i + 2] * R[6 + j];
    const double det = M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) -
                       M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) +
                       M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
    const double s = 1.0 / det;
    iR[0][0] = (M[1][1] * M[2][2] - M[1][2] * M[2][1]) * s;
    iR[0][1] = (M[0][2] * M[2][1] - M[0][1] * M[2][2]) * s;
    iR[0][2] = (M[0][1] * M[1][2] - M[0][2] * M[1][1]) * s;
    iR[1][0] = (M[1][2] * M[2][0] - M[1][0] * M[2][2]) * s;
    iR[1][1] = (M[0][0] * M[2][2] - M[0][2] * M[2][0]) * s;
    iR[1][2] = (M[0][2] * M[1][0] - M[0][0] * M[1][2]) * s;
    iR[2][0] = (M[1][0] * M[2][1] - M[1][1] * M[2][0]) * s;
    iR[2][1] = (M[0][1] * M[2][0] - M[0][0] * M[2][1]) * s;
    iR[2][2] = (M[0][0] * M[1][1] - M[0][1] * M[1][0]) * s;
    for (int i = 0; i < height; ++i) {
        float* m1 = map1 + (size_t)i * width;
        float* m2 = map2 + (size_t)i * width;
        double _x = i * iR[0][1] + iR[0][2], _y = i * iR[1][1] + iR[1][2],
               _w = i * iR[2][1] + iR[2][2];
        for (int j = 0; j < width; ++j, _x += iR[0][0], _y += iR[1][0], _w += iR[2][0]) {
            const double w = 1. / _w, x = _x * w, y = _y * w;
            const double x2 = x * x, y2 = y * y;
            const double r2 = x2 + y2, _2xy = 2 * x * y;
            const double kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) /
                              (1 + ((k6 * r2 + k5) * r2 + k4) * r2);
            const double xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2);
            const double yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy;
            m1[j] = (float)(fx * xd + cx);
            m2[j] = (float)(fy * yd + cy);
        }
    }
    return ORBX_OK;
}

orbx_status orbx_remap_fixed_point(const float* map1, const float* map2, size_t n, int16_t* xy,
                                   uint16_t* a) {
    if (n > 0 && (!map1 || !map2 || !xy || !a)) return ORBX_ERR_INVALID;
    for (size_t i = 0; i < n; ++i) {
        const int sx = cv_round(map1[i] * 32.0f), sy = cv_round(map2[i] * 32.0f);
        xy[2 * i] = (int16_t)sat_short(sx >> 5);
        xy[2 * i + 1] = (int16_t)sat_short(sy >> 5);
        a[i] = (uint16_t)((sy & 31) * 32 + (sx & 31));
    }
    return ORBX_OK;
}

orbx_status orbx_rectifier_create(const float* map1, const float* map2, int32_t dst_w,
                                  int32_t dst_h, int32_t src_w, int32_t src_h, int device,
                                  orbx_rectifier** out) {
    if (out) *out = nullptr;
    if (!map1 || !map2 || !out || dst_w <= 0 || dst_h <= 0 || src_w <= 0 || src_h <= 0)
        return ORBX_ERR_INVALID;
    if (src_w > 32767 || src_h > 32767) return ORBX_ERR_UNSUPPORTED;   // the short saturation
    if (!HIPOK(hipSetDevice(device))) return ORBX_ERR_DEVICE;
    const int pitch = (dst_w + 3) & ~3;
    std::vector<uint2> m((size_t)pitch * dst_h, make_uint2(0u, 0u));
    std::vector<int16_t> xy(2 * (size_t)dst_w);
    std::vector<uint16_t> ab((size_t)dst_w);
    for (int y = 0; y < dst_h; ++y) {
        orbx_remap_fixed_point(map1 + (size_t)y * dst_w, map2 + (size_t)y * dst_w, (size_t)dst_w,
                               xy.data(), ab.data());
        for (int x = 0; x < dst_w; ++x) {
            const int X = xy[2 * x], Y = xy[2 * x + 1], a = ab[x] & 31, b = ab[x] >> 5;
            auto cl = [](int v, int n) { return v < 0 ? 0 : v > n - 1 ? n - 1 : v; };
            const uint32_t Xc = cl(X, src_w), Yc = cl(Y, src_h);
            const uint32_t dx = cl(X + 1, src_w) - Xc, dy = cl(Y + 1, src_h) - Yc;
            const uint32_t wx0 = (X >= 0 && X < src_w) ? 32 - a : 0;
            const uint32_t wx1 = (X + 1 >= 0 && X + 1 < src_w) ? a : 0;
            const uint32_t wy0 = (Y >= 0 && Y < src_h) ? 32 - b : 0;
            const uint32_t wy1 = (Y + 1 >= 0 && Y + 1 < src_h) ? b : 0;
            m[(size_t)y * pitch + x] = make_uint2(Xc | dx << 15 | Yc << 16 | dy << 31,
                                                  wx0 | wx1 << 8 | wy0 << 16 | wy1 << 24);
        }
        // padding: the last pixel's coordinates (its footprint is the group's), zero weights
        for (int x = dst_w; x < pitch; ++x)
            m[(size_t)y * pitch + x] = make_uint2(m[(size_t)y * pitch + dst_w - 1].x, 0u);
    }
    orbx_rectifier* r = new orbx_rectifier();
    r->device = device;
    r->dst_w = dst_w;
    r->dst_h = dst_h;
    r->src_w = src_w;
    r->src_h = src_h;
    r->pitch = pitch;
    const size_t bytes = m.size() * sizeof(uint2);
    if (!HIPOK(hipMalloc((void**)&r->d_map, bytes)) ||
        !HIPOK(hipMemcpy(r->d_map, m.data(), bytes, hipMemcpyHostToDevice))) {
        if (r->d_map) (void)hipFree(r->d_map);
        delete r;
        return ORBX_ERR_DEVICE;
    }
    *out = r;
    return ORBX_OK;
}

orbx_status orbx_rectifier_destroy(orbx_rectifier* r) {
    if (!r) return ORBX_OK;
    (void)hipSetDevice(r->device);
    if (r->d_map) (void)hipFree(r->d_map);
    delete r;
    return ORBX_OK;
}

orbx_status orbx_remap_batch_device(const orbx_rectifier* r, const uint8_t* d_src,
                                    size_t src_row_stride, size_t src_image_stride,
                                    uint8_t* d_dst, size_t dst_row_stride,
                                    size_t dst_image_stride, int32_t batch, void* stream) {
    const orbx_status a = side_args(r, d_src, src_row_stride, src_image_stride, d_dst,
                                    dst_row_stride, dst_image_stride, batch);
    if (a != ORBX_OK) return a;
    const RemapSide s = make_side(r, d_src, src_row_stride, src_image_stride, d_dst,
                                  dst_row_stride, dst_image_stride);
    return launch(r, s, s, 1, batch, stream);
}

orbx_status orbx_remap_stereo_batch_device(
    const orbx_rectifier* r_left, const orbx_rectifier* r_right, const uint8_t* d_src_left,
    const uint8_t* d_src_right, size_t src_row_stride, size_t src_image_stride,
    uint8_t* d_dst_left, uint8_t* d_dst_right, size_t dst_row_stride, size_t dst_image_stride,
    int32_t batch, void* stream) {
    orbx_status a = side_args(r_left, d_src_left, src_row_stride, src_image_stride, d_dst_left,
                              dst_row_stride, dst_image_stride, batch);
    if (a == ORBX_OK)
        a = side_args(r_right, d_src_right, src_row_stride, src_image_stride, d_dst_right,
                      dst_row_stride, dst_image_stride, batch);
    if (a != ORBX_OK) return a;
    if (r_left->dst_w != r_right->dst_w || r_left->dst_h != r_right->dst_h ||
        r_left->device != r_right->device)
        return ORBX_ERR_INVALID;
    return launch(r_left,
                  make_side(r_left, d_src_left, src_row_stride, src_image_stride, d_dst_left,
                            dst_row_stride, dst_image_stride),
                  make_side(r_right, d_src_right, src_row_stride, src_image_stride, d_dst_right,
                            dst_row_stride, dst_image_stride),
                  2, batch, stream);
}

orbx_status orbx_remap(const orbx_rectifier* r, const uint8_t* src, size_t src_stride,
                       uint8_t* dst, size_t dst_stride) {
    if (!r || !src || !dst || src_stride < (size_t)r->src_w || dst_stride < (size_t)r->dst_w)
        return ORBX_ERR_INVALID;
    HostCall c(r->device);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    const size_t sb = (size_t)r->src_w * r->src_h, db = (size_t)r->dst_w * r->dst_h;
    const size_t p_src = c.plan().scratch(sb), p_dst = c.plan().scratch(db);
    if (!c.upload() || !HIPOK(hipMemcpy2DAsync(c.dev<uint8_t>(p_src), r->src_w, src, src_stride,
                                               r->src_w, r->src_h, hipMemcpyHostToDevice, c.st())))
        return c.finish(ORBX_ERR_DEVICE);
    orbx_status s = orbx_remap_batch_device(r, c.dev<uint8_t>(p_src), r->src_w, sb,
                                            c.dev<uint8_t>(p_dst), r->dst_w, db, 1, c.st());
    // only the dst_w bytes of each row come back: the rest of the caller's rows is untouched
    if (s == ORBX_OK && !HIPOK(hipMemcpy2DAsync(dst, dst_stride, c.dev<uint8_t>(p_dst), r->dst_w,
                                                r->dst_w, r->dst_h, hipMemcpyDeviceToHost, c.st())))
        s = ORBX_ERR_DEVICE;
    return c.finish(s);
}

}  // extern "C"
