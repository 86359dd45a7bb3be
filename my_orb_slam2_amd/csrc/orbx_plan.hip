// orbx_plan.hip — what the host works out ahead of a launch: the ORBextractor constructor tables
// (src/ORBextractor.cc:410-470), the per-image-size geometry (pyramid sizes :1134, FAST cell grid
// :793-818, octree roots :543-545, OpenCV resize coefficient tables) and the batch-size policies
// of one extraction.  No HIP runtime call: the handle uploads what build_geometry fills.
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>

#include "orbx_extractor.h"
#include "orbx_math.h"

namespace orbx {
namespace {

inline int cvRound(float v) { return cv_round(v); }
inline int cvRound(double v) { return (int)lrint(v); }
inline int cvFloor(float v) { int i = cvRound(v); float d = (float)(v - i); return i - (d < 0); }
inline int cvCeil(float v) { int i = cvRound(v); float d = (float)(i - v); return i + (d < 0); }
inline short sat_short(float v) {
    int i = cvRound(v);
    return (short)std::min(std::max(i, (int)SHRT_MIN), (int)SHRT_MAX);
}

int reflect101_h(int p, int len) {
    if ((unsigned)p < (unsigned)len) return p;
    if (len == 1) return 0;
    do {
        if (p < 0) p = -p;
        else p = 2 * len - 2 - p;
    } while ((unsigned)p >= (unsigned)len);
    return p;
}

int vresize_simd_end(int width) {
    int x = 0;
    for (; x <= width - 16; x += 16) {}
    for (; x < width - 4; x += 4) {}
    return x;
}

// Strip height of a level for a batch of nimg images: STRIP_TH rows while the level's strip
// walks give every SIMD of the device (ncu CUs x 4) two waves, else the tallest of 32 / 16 / 8
// rows that does (8 at most).  A strip walk is a serial chain of rows, so a small batch (one
// stereo frame at a time: the tracking thread's case) is latency-bound on the few long walks
// of each level: 8-row strips take one stereo pair's pyramid from 0.218 to 0.082 ms (the
// halo rows cost more work, which only large batches would notice).
static int strip_default(const LevelGeom& lv, int nimg, int ncu) {
    const long long target = 2LL * ncu * 4;
    int th = STRIP_TH;
    while (th > 8 && (long long)lv.snw * ((lv.h + th - 1) / th) * nimg < target) th /= 2;
    return th;
}

// k_level_strip tables of level l (StripLane per half-strip lane, rows -3 .. h+2); the level
// takes the plain kernels (strip = 0) for modes 1 / 2 or when a group's taps do not fit the
// 8-byte window the strip kernel reads.  Level 0 (mode 0) always strips.
void build_strip_tables(ExtractPlan& p, int l, int mode, const int16_t* xofs,
                        const int16_t* alpha, const int16_t* yofs, const int16_t* beta) {
    Geometry& G = p.hg;
    LevelGeom& lv = G.lv[l];
    lv.strip = 0;
    if (mode != 0 && mode != 3) return;
    const LevelGeom& S = G.lv[l > 0 ? l - 1 : 0];
    lv.snh = (lv.w + SW_PX - 1) / SW_PX;
    lv.snw = (lv.snh + 1) / 2;
    std::vector<StripLane> sl((size_t)lv.snh * 32);
    for (int hs = 0; hs < lv.snh; ++hs)
        for (int q = 0; q < 32; ++q) {
            StripLane& e = sl[(size_t)hs * 32 + q];
            memset(&e, 0, sizeof(e));
            int xr[4];
            const int xg = hs * SW_PX - 4 + 4 * q;
            for (int j = 0; j < 4; ++j)   // groups past every output's halo: any in-row column
                xr[j] = xg > lv.w + 3 ? lv.w - 1 : reflect101_h(xg + j, lv.w);
            if (mode == 0) {
                const int mn = std::min(std::min(xr[0], xr[1]), std::min(xr[2], xr[3]));
                e.base = (uint32_t)mn;
                // offsets <= 3 (+ the row address's low 2 bits <= 7, the bytes one v_perm reads):
                // BORDER_REFLECT_101 moves by at most 1 per column, so the four columns of a
                // group lie within 3 of each other at every width
                for (int j = 0; j < 4; ++j) e.sel |= (uint32_t)(xr[j] - mn) << (8 * j);
            } else {
                int sx[4];
                for (int j = 0; j < 4; ++j) sx[j] = xofs[xr[j]];
                const int mn = std::min(std::min(sx[0], sx[1]), std::min(sx[2], sx[3]));
                e.base = (uint32_t)mn;
                for (int j = 0; j < 4; ++j) {
                    const int k = sx[j] - mn;
                    // taps k, k+1 of the 8 bytes from the first tap column (o0 + 11 < 16 read)
                    if (k > 6) return;
                    e.psel[j] = (uint32_t)k | (0x0Cu << 8) | ((uint32_t)(k + 1) << 16) | (0x0Cu << 24);
                    uint32_t a0 = (uint16_t)alpha[2 * xr[j]], a1 = (uint16_t)alpha[2 * xr[j] + 1];
                    if (xr[j] >= lv.xmax) { a0 = 2048; a1 = 0; }   // HResizeLinear: S[sx] * 2048
                    e.alp[j] = (a0 << 4) | ((a1 << 4) << 16);
                    e.flags |= (uint32_t)((xr[j] < lv.xmax ? 1 : 0) | (xr[j] < lv.rsimd_end ? 2 : 0))
                               << (2 * j);
                }
            }
        }
    std::vector<uint32_t> rt((size_t)4 * (lv.h + 6));
    for (int k = 0; k < lv.h + 6; ++k) {
        const int yr = reflect101_h(k - 3, lv.h);
        if (mode == 0) {
            rt[4 * k] = (uint32_t)yr;
        } else {
            const int sy = yofs[yr];
            const uint32_t r0 = (uint32_t)std::min(std::max(sy, 0), S.h - 1);
            const uint32_t r1 = (uint32_t)std::min(std::max(sy + 1, 0), S.h - 1);
            rt[4 * k] = r0 * (uint32_t)S.pitch;       // byte offsets of the two source rows
            rt[4 * k + 1] = r1 * (uint32_t)S.pitch;
            rt[4 * k + 2] = (uint32_t)(uint16_t)beta[2 * yr] | ((uint32_t)(uint16_t)beta[2 * yr + 1] << 16);
        }
    }
    p.ltab.resize(align_up(p.ltab.size(), 16));
    lv.stab = (int)p.ltab.size();
    p.ltab.insert(p.ltab.end(), (const uint8_t*)sl.data(), (const uint8_t*)(sl.data() + sl.size()));
    p.ltab.resize(align_up(p.ltab.size(), 16));
    lv.srow = (int)p.ltab.size();
    p.ltab.insert(p.ltab.end(), (const uint8_t*)rt.data(), (const uint8_t*)(rt.data() + rt.size()));
    p.ltab.resize(align_up(p.ltab.size(), 16));
    lv.strip = 1;
}

// k_pyr_chain tiles (orbx_pyramid.hip): per tile of a gx x gy grid and per level, the owned
// rectangle and the footprint, built from the deepest level up: a level's footprint is its
// owned rectangle + the blur halo, joined with the source rows / columns the next level's
// footprint reads through the resize tables (xofs / yofs of level l + 1, as cv::resize's
// HResizeLinear / VResizeLinear index them).  chain_ok stays 0 (per-level launches) unless
// every level l >= 1 is INTER_LINEAR and the two level buffers + row sums fit the LDS.
static void build_chain(ExtractPlan& p) {
    Geometry& G = p.hg;
    const int L = G.nlevels;
    G.chain_ok = 0;
    G.chain_gx = G.chain_gy = 1;
    G.chain_tab = G.chain_toffs = 0;
    G.chain_buf = G.chain_rs = G.chain_lds = 0;
    for (int l = 1; l < L; ++l) {
        if (G.lv[l].copy || G.lv[l].area2) return;
        // a 4-pixel group's taps must fit the 8 bytes one v_perm pair reads (source span <= 6,
        // i.e. scale factors up to about 2.3; groups start at multiples of 4)
        const int16_t* xofs = p.rtab.data() + G.lv[l].rtab_off;
        for (int x = 0; x < G.lv[l].w; x += 4)
            if (xofs[std::min(x + 3, G.lv[l].w - 1)] - xofs[x] > 5) return;
    }
    const int gx = std::max(1, (G.lv[0].w + CHAIN_TW - 1) / CHAIN_TW);
    const int gy = std::max(1, (G.lv[0].h + CHAIN_TH - 1) / CHAIN_TH);
    std::vector<ChainRect> rects((size_t)gx * gy * L);
    // k_pyr_chain table offsets per tile: [L + 1] entry prefix, then [L + 1] word prefix
    std::vector<int32_t> toffs((size_t)gx * gy * 2 * (L + 1), 0);
    size_t buf = 16, rs = 16, ct = 16;
    for (int ty = 0; ty < gy; ++ty)
        for (int tx = 0; tx < gx; ++tx) {
            size_t tab = 0;   // table entries of the tile's levels 1.. (k_pyr_chain phase 1)
            bool have_next = false;
            int nx0 = 0, nx1 = -1, ny0 = 0, ny1 = -1;   // footprint of level l + 1
            for (int l = L - 1; l >= 0; --l) {
                const LevelGeom& lv = G.lv[l];
                const int W = lv.w, Hh = lv.h;
                const int ox0 = tx == 0 ? 0 : ((int)((long long)tx * W / gx) & ~3);
                const int ox1 = std::max(ox0, tx == gx - 1 ? W : ((int)((long long)(tx + 1) * W / gx) & ~3));
                const int oy0 = (int)((long long)ty * Hh / gy);
                const int oy1 = std::max(oy0, ty == gy - 1 ? Hh : (int)((long long)(ty + 1) * Hh / gy));
                int fx0 = INT_MAX, fx1 = -1, fy0 = INT_MAX, fy1 = -1;
                if (ox1 > ox0 && oy1 > oy0) {
                    fx0 = std::max(ox0 - 3, 0);
                    fx1 = std::min(ox1 + 2, W - 1);
                    fy0 = std::max(oy0 - 3, 0);
                    fy1 = std::min(oy1 + 2, Hh - 1);
                }
                if (have_next) {
                    const LevelGeom& D = G.lv[l + 1];
                    const int16_t* xofs = p.rtab.data() + D.rtab_off;
                    const int16_t* yofs = xofs + 3 * D.w;
                    fx0 = std::min(fx0, std::min(std::max((int)xofs[nx0], 0), W - 1));
                    fx1 = std::max(fx1, std::min((int)xofs[nx1] + 1, W - 1));
                    fy0 = std::min(fy0, std::min(std::max((int)yofs[ny0], 0), Hh - 1));
                    fy1 = std::max(fy1, std::min(std::max((int)yofs[ny1] + 1, 0), Hh - 1));
                }
                ChainRect& c = rects[((size_t)ty * gx + tx) * L + l];
                c.ox0 = (int16_t)ox0;
                c.ox1 = (int16_t)ox1;
                c.oy0 = (int16_t)oy0;
                c.oy1 = (int16_t)oy1;
                if (fx1 < 0) {
                    c.fx0 = c.fy0 = 0;
                    c.fx1 = c.fy1 = -1;
                    have_next = false;
                    continue;
                }
                fx0 &= ~3;
                c.fx0 = (int16_t)fx0;
                c.fx1 = (int16_t)fx1;
                c.fy0 = (int16_t)fy0;
                c.fy1 = (int16_t)fy1;
                have_next = true;
                nx0 = fx0;
                nx1 = fx1;
                ny0 = fy0;
                ny1 = fy1;
                const int fw = fx1 - fx0 + 1;
                buf = std::max(buf, (size_t)chain_pitch(fw) * (fy1 - fy0 + 1) + 16);
                rs = std::max(rs, (size_t)4 * ((ox1 - ox0 + 3) & ~3) * (oy1 - oy0 + 6));
                if (l > 0) tab += chain_level_words((fw + 3) >> 2, fy1 - fy0 + 1);
            }
            ct = std::max(ct, 4 * tab);
            int32_t* te = &toffs[((size_t)ty * gx + tx) * 2 * (L + 1)];
            int32_t* tw = te + (L + 1);
            for (int l = 1; l < L; ++l) {
                const ChainRect& c = rects[((size_t)ty * gx + tx) * L + l];
                const int fw = c.fx1 - c.fx0 + 1, fh = c.fy1 - c.fy0 + 1;
                te[l + 1] = te[l] + (fw > 0 ? ((fw + 3) >> 2) + ((fh + 1) & ~1) : 0);
                tw[l + 1] = tw[l] + (fw > 0 ? chain_level_words((fw + 3) >> 2, fh) : 0);
            }
        }
    auto r16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t lds = 2 * r16(buf) + r16(rs) + r16(ct);
    if (lds > 150 * 1024) return;
    G.chain_gx = gx;
    G.chain_gy = gy;
    G.chain_buf = (int)r16(buf);
    G.chain_rs = (int)r16(rs);
    G.chain_lds = (int)lds;
    while (p.ltab.size() % 16) p.ltab.push_back(0);
    G.chain_tab = (int)p.ltab.size();
    p.ltab.insert(p.ltab.end(), (const uint8_t*)rects.data(), (const uint8_t*)(rects.data() + rects.size()));
    while (p.ltab.size() % 16) p.ltab.push_back(0);
    G.chain_toffs = (int)p.ltab.size();
    p.ltab.insert(p.ltab.end(), (const uint8_t*)toffs.data(), (const uint8_t*)(toffs.data() + toffs.size()));
    G.chain_ok = 1;
}

}  // namespace

// Small-batch launch policies.
#define OCT_LDS_SMALL_KB 152   // octree LDS budget for small batches (one workgroup per list)
#define OCT_SMALL_BATCH 16
// images per call up to which the octree takes that budget (one workgroup per CU is still
// every list at once up to 32 images; a frame-server batch of 2-16 images: 46.4 -> 42.0 us
// with 16 instead of 4, r4aa)
#define CHAIN_MAX_BATCH 8      // images per call up to which the pyramid is one k_pyr_chain launch
                               // (r5c16: 16 images lost at K = 8 sessions, 9.5-9.9 k vs 10.2-10.7 k pairs/s)
#define SIDE_MIN_BATCH 16      // images per call from which the default side branch forks

void compute_tables(const orbx_extractor_params& prm, ExtractPlan& p) {
    const int L = prm.nlevels;
    const double scaleFactor = (double)prm.scale_factor;   // ORBextractor::scaleFactor is double
    p.scale.assign(L, 0.f);
    p.sigma2.assign(L, 0.f);
    p.inv_scale.assign(L, 0.f);
    p.inv_sigma2.assign(L, 0.f);
    p.nfeat.assign(L, 0);
    p.scale[0] = 1.0f;
    p.sigma2[0] = 1.0f;
    for (int i = 1; i < L; i++) {
        p.scale[i] = (float)(p.scale[i - 1] * scaleFactor);
        p.sigma2[i] = p.scale[i] * p.scale[i];
    }
    for (int i = 0; i < L; i++) {
        p.inv_scale[i] = 1.0f / p.scale[i];
        p.inv_sigma2[i] = 1.0f / p.sigma2[i];
    }
    const int nfeatures = prm.nfeatures;
    float factor = (float)(1.0f / scaleFactor);
    float nDesired = nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)L));
    int sum = 0;
    for (int level = 0; level < L - 1; level++) {
        p.nfeat[level] = cvRound(nDesired);
        sum += p.nfeat[level];
        nDesired *= factor;
    }
    p.nfeat[L - 1] = std::max(nfeatures - sum, 0);
    // umax (src/ORBextractor.cc:454-469)
    const int HP = 15;
    int v, v0, vmax = cvFloor((float)(HP * std::sqrt(2.f) / 2 + 1));
    int vmin = cvCeil((float)(HP * std::sqrt(2.f) / 2));
    const double hp2 = HP * HP;
    for (v = 0; v <= vmax; ++v) p.umax[v] = cvRound(std::sqrt(hp2 - v * v));
    for (v = HP, v0 = 0; v >= vmin; --v) {
        while (p.umax[v0] == p.umax[v0 + 1]) ++v0;
        p.umax[v] = v0;
        ++v0;
    }
    // getGaussianKernel(7, 2, CV_32F) -> x256 fixed point (FilterEngine 8U path)
    float cf[7];
    double s2 = -0.5 / (2.0 * 2.0), ksum = 0;
    for (int i = 0; i < 7; ++i) {
        double x = i - 3.0;
        cf[i] = (float)std::exp(s2 * x * x);
        ksum += cf[i];
    }
    ksum = 1. / ksum;
    for (int i = 0; i < 7; ++i) cf[i] = (float)(cf[i] * ksum);
    for (int i = 0; i < 7; ++i) p.taps[i] = cvRound(cf[i] * 256.f);
}

// Per-size geometry.  Returns ORBX_OK or ORBX_ERR_UNSUPPORTED.
orbx_status build_geometry(const orbx_extractor_params& prm, int W, int H, ExtractPlan& p) {
    Geometry& G = p.hg;
    memset(&G, 0, sizeof(G));
    // the blur's column pass folds the symmetric Gaussian taps (getGaussianKernel is symmetric)
    for (int i = 0; i < 3; ++i)
        if (p.taps[i] != p.taps[6 - i]) return ORBX_ERR_UNSUPPORTED;
    p.cells.clear();
    p.rtab.clear();
    const int L = prm.nlevels;
    G.width = W;
    G.height = H;
    G.nlevels = L;
    G.ini_th = std::min(std::max(prm.ini_th_fast, 0), 255);
    G.min_th = std::min(std::max(prm.min_th_fast, 0), 255);
    memcpy(G.taps, p.taps, sizeof(G.taps));
    memcpy(G.umax, p.umax, sizeof(G.umax));
    // k_stereo buckets right keypoints by (octave, row); a keypoint of octave o lists itself
    // in the rows of its band [floor(y - 2 scale[o]), ceil(y + 2 scale[o])] (src/Frame.cc:522-530)
    for (int l = 0; l < L; ++l)
        G.lv[l].stereo_win = (int)std::ceil(2.0f * p.scale[l]) + 2;
    long long off = 0, cand = 0;
    int out = 0, blur_tiles = 0, oblocks = 0;
    for (int l = 0; l < L; ++l) {
        LevelGeom& lv = G.lv[l];
        lv.w = cvRound((float)W * p.inv_scale[l]);
        lv.h = cvRound((float)H * p.inv_scale[l]);
        if (lv.w <= 0 || lv.h <= 0) return ORBX_ERR_UNSUPPORTED;
        if (lv.w > 4096 + 32 || lv.h > 4096 + 32) return ORBX_ERR_UNSUPPORTED;   // 12-bit packing
        lv.pitch = (int)align_up(lv.w + 4, 64);   // >= 4 bytes of slack for dword staging
        lv.off = off;
        // whole bands of 4 rows: the blurred pyramid (same offsets) is stored in 16x4 tiles
        off += (long long)align_up((size_t)lv.pitch * align_up((size_t)lv.h, 4), 256);
        lv.scale = p.scale[l];
        lv.inv_scale = p.inv_scale[l];
        lv.nfeat = p.nfeat[l];
        lv.patch_size = (int)(31 * p.scale[l]);
        // FAST cell grid (src/ORBextractor.cc:785-818)
        const int minB = ORBX_MIN_BORDER;
        const int maxBX = lv.w - ORBX_EDGE + 3, maxBY = lv.h - ORBX_EDGE + 3;
        const float width = (float)(maxBX - minB), height = (float)(maxBY - minB);
        const int nCols = (int)(width / 30.f), nRows = (int)(height / 30.f);
        lv.ncols = nCols;
        lv.nrows = nRows;
        lv.cell_begin = (int)p.cells.size();
        lv.cand_off = cand;
        int lcap = 0;
        if (nCols > 0 && nRows > 0) {
            const int wCell = (int)std::ceil(width / nCols);
            const int hCell = (int)std::ceil(height / nRows);
            lv.wcell = wCell;
            lv.hcell = hCell;
            for (int i = 0; i < nRows; i++) {
                const float iniY = (float)(minB + i * hCell);
                float maxY = iniY + hCell + 6;
                if (iniY >= maxBY - 3) continue;
                if (maxY > maxBY) maxY = (float)maxBY;
                for (int j = 0; j < nCols; j++) {
                    const float iniX = (float)(minB + j * wCell);
                    float maxX = iniX + wCell + 6;
                    if (iniX >= maxBX - 6) continue;
                    if (maxX > maxBX) maxX = (float)maxBX;
                    CellDesc c;
                    memset(&c, 0, sizeof(c));
                    c.level = (int16_t)l;
                    c.ini_x = (int16_t)(int)iniX;
                    c.ini_y = (int16_t)(int)iniY;
                    c.cols = (int16_t)((int)maxX - (int)iniX);
                    c.rows = (int16_t)((int)maxY - (int)iniY);
                    const int dh = c.rows - 6, dw = c.cols - 6;
                    c.cap = (dh > 0 && dw > 0) ? ((dw + 1) / 2) * ((dh + 1) / 2) : 0;
                    c.slot = (int32_t)cand;
                    cand += c.cap;
                    lcap += c.cap;
                    // k_fast stages the ROI with detection column 0 on a 16-byte boundary
                    G.max_roi_bytes = std::max(G.max_roi_bytes, fast_roi_bytes(c.rows, dw));
                    if (dh > 0 && dw > 0) {
                        G.max_mbuf_bytes = std::max(G.max_mbuf_bytes, ((dh + 2) * (dw + 2) + 3) & ~3);
                        G.max_cell_px = std::max(G.max_cell_px, dh * dw);
                    }
                    // k_fast lane mapping; its staging takes a ROI row, before and after the
                    // realignment, in 16 lanes of a dword each (a 30-pixel cell target gives
                    // cols <= 59)
                    if (dw > 64 || dh > 511 || c.cols > 60) return ORBX_ERR_UNSUPPORTED;
                    p.cells.push_back(c);
                }
            }
        }
        lv.ncells = (int)p.cells.size() - lv.cell_begin;
        lv.cand_cap = lcap;
        G.max_ncand_level = std::max(G.max_ncand_level, lcap);
        // octree roots (src/ORBextractor.cc:543-545)
        lv.n_ini = 0;
        lv.hx = 0.f;
        if (maxBY - minB > 0) {
            const float r = std::round(static_cast<float>(maxBX - minB) / (maxBY - minB));
            if (r >= 1.f && r < 4096.f) {
                lv.n_ini = (int)r;
                lv.hx = static_cast<float>(maxBX - minB) / lv.n_ini;
            }
        }
        lv.out_cap = std::max(std::max(lv.nfeat + 3, 4 * lv.n_ini), 4);
        lv.kp_level_cap = lv.out_cap;
        lv.out_off = out;
        out += lv.out_cap;
        G.max_out_cap = std::max(G.max_out_cap, lv.out_cap);
        G.blur_tile_begin[l] = blur_tiles;
        blur_tiles += ((lv.w + 63) / 64) * ((lv.h + 15) / 16);
        G.orient_block_begin[l] = oblocks;
        oblocks += (lv.out_cap + 4 * OD_NK - 1) / (4 * OD_NK);
        lv.bsimd_end = prm.cv_simd ? (lv.w / 4) * 4 : 0;
        // resize tables (cv::resize INTER_LINEAR 8U, imgwarp.cpp)
        lv.copy = lv.area2 = 0;
        lv.rtab_off = 0;
        lv.xmax = lv.w;
        lv.rsimd_end = 0;
        if (l > 0) {
            const LevelGeom& S = G.lv[l - 1];
            const int sw = S.w, sh = S.h, dw = lv.w, dh = lv.h;
            if (sw == dw && sh == dh) {
                lv.copy = 1;
            } else {
                const double inv_sx = (double)dw / sw, inv_sy = (double)dh / sh;
                const double scale_x = 1. / inv_sx, scale_y = 1. / inv_sy;
                const int isx = cvRound(scale_x), isy = cvRound(scale_y);
                const bool area_fast = std::abs(scale_x - isx) < DBL_EPSILON &&
                                       std::abs(scale_y - isy) < DBL_EPSILON;
                if (area_fast && isx == 2 && isy == 2) {
                    lv.area2 = 1;
                } else {
                    lv.rtab_off = (int)p.rtab.size();
                    std::vector<int16_t> xofs(dw), alpha(2 * dw), yofs(dh), beta(2 * dh);
                    int xmax = dw;
                    for (int dx = 0; dx < dw; ++dx) {
                        float fx = (float)((dx + 0.5) * scale_x - 0.5);
                        int sx = cvFloor(fx);
                        fx -= sx;
                        if (sx < 0) { fx = 0, sx = 0; }
                        if (sx + 1 >= sw) {
                            xmax = std::min(xmax, dx);
                            if (sx >= sw - 1) fx = 0, sx = sw - 1;
                        }
                        xofs[dx] = (int16_t)sx;
                        alpha[2 * dx] = sat_short((1.f - fx) * 2048);
                        alpha[2 * dx + 1] = sat_short(fx * 2048);
                    }
                    for (int dy = 0; dy < dh; ++dy) {
                        float fy = (float)((dy + 0.5) * scale_y - 0.5);
                        int sy = cvFloor(fy);
                        fy -= sy;
                        yofs[dy] = (int16_t)sy;
                        beta[2 * dy] = sat_short((1.f - fy) * 2048);
                        beta[2 * dy + 1] = sat_short(fy * 2048);
                    }
                    p.rtab.insert(p.rtab.end(), xofs.begin(), xofs.end());
                    p.rtab.insert(p.rtab.end(), alpha.begin(), alpha.end());
                    p.rtab.insert(p.rtab.end(), yofs.begin(), yofs.end());
                    p.rtab.insert(p.rtab.end(), beta.begin(), beta.end());
                    lv.xmax = xmax;
                    lv.rsimd_end = prm.cv_simd ? vresize_simd_end(dw) : 0;
                }
            }
        }
    }
    // k_level_strip tables of the levels that take the strip walk
    p.ltab.clear();
    for (int l = 0; l < L; ++l) {
        const LevelGeom& lv = G.lv[l];
        const int mode = l == 0 ? 0 : (lv.copy ? 1 : (lv.area2 ? 2 : 3));
        const int16_t* xofs = p.rtab.data() + lv.rtab_off;
        const int16_t* alpha = xofs + lv.w;
        const int16_t* yofs = alpha + 2 * lv.w;
        const int16_t* beta = yofs + lv.h;
        build_strip_tables(p, l, mode, xofs, alpha, yofs, beta);
    }
    build_chain(p);
    G.blur_tile_begin[L] = blur_tiles;
    G.orient_block_begin[L] = oblocks;
    G.blur_tiles = blur_tiles;
    G.orient_blocks = oblocks;
    G.n_cells = (int)p.cells.size();
    G.kp_cap = out;
    G.out_words = out;
    G.pyr_bytes = off;
    G.cand_words = std::max(cand, 1LL);
    if (G.max_roi_bytes == 0) G.max_roi_bytes = 16;
    if (G.max_mbuf_bytes == 0) G.max_mbuf_bytes = 16;
    if (G.max_out_cap > 8192) return ORBX_ERR_UNSUPPORTED;
    p.kscratch_per_image = 0;
    for (int l = 0; l < L; ++l) p.kscratch_per_image += (long long)G.lv[l].cand_cap * 8;
    p.kscratch_per_image = (long long)align_up((size_t)std::max(p.kscratch_per_image, 16LL), 256);
    // octree LDS (all levels in one launch): node arrays for the largest level's list, the
    // candidate arrays in LDS up to the OCT_LDS_KB budget (a level with more candidates keeps
    // them in global scratch)
    p.ncap = (int)align_up((size_t)std::max(G.max_out_cap, 16), 16);
    auto kcap_within = [&](bool packed, size_t kb) {
        int kc = std::min(std::max(G.max_ncand_level, 64), 8192);
        while (kc > 64 && OctreeCarve(p.ncap, kc, packed).bytes > kb * 1024) kc -= 64;
        return kc;
    };
    p.kcap = kcap_within(true, OCT_LDS_KB);
    p.octree_lds = OctreeCarve(p.ncap, p.kcap, true).bytes;
    // small batches: the same node arrays, candidates in LDS up to OCT_LDS_SMALL_KB
    p.kcap_small = std::max(kcap_within(false, OCT_LDS_SMALL_KB), p.kcap);
    p.octree_lds_small = std::max(OctreeCarve(p.ncap, p.kcap_small, false).bytes, p.octree_lds);
    G.stereo_ob = G.nlevels;
    p.stereo_lds = stereo_lds_bytes(G.kp_cap, G.lv[0].h, G.stereo_ob);
    if (p.stereo_lds > 160 * 1024) {   // row buckets only (octaves tested per candidate)
        G.stereo_ob = 1;
        p.stereo_lds = stereo_lds_bytes(G.kp_cap, G.lv[0].h, G.stereo_ob);
    }
    if (p.octree_lds > 160 * 1024 || p.stereo_lds > 160 * 1024) return ORBX_ERR_UNSUPPORTED;
    if (G.kp_cap > 32767) return ORBX_ERR_UNSUPPORTED;   // 16-bit keypoint indices in stereo
    return ORBX_OK;
}

// Every strip level's height for a batch of nimg images (a launch argument of k_level_strip,
// so a batch-size change touches no device state).
void strip_heights(const orbx_extractor* h, int nimg, int* sth) {
    for (int l = 0; l < ORBX_MAX_LEVELS; ++l) sth[l] = STRIP_TH;
    for (int l = 0; l < h->hg.nlevels; ++l) {
        const LevelGeom& lv = h->hg.lv[l];
        if (lv.strip) sth[l] = strip_default(lv, nimg, h->ncu);
    }
}

// k_fast cells per wave: FAST_NC (the next cell's ROI loads overlap the current cell) while the
// launch gives every CU two workgroups, fewer for small batches (a wave's cells run in series,
// so one image's FAST is a chain of FAST_NC cells otherwise).
int fast_cells_per_wave(int ncells, int batch, int ncu) {
    int nc = FAST_NC;
    while (nc > 1 && (long long)ncells * batch / (4 * nc) < 2LL * ncu) nc >>= 1;
    return nc;
}

// The other batch-size switches of extract_launch (orbx_extractor_regime_info reports them).
int octree_small(int batch) { return batch <= OCT_SMALL_BATCH ? 1 : 0; }
int side_mode_of(const orbx_extractor* h, int batch) {
    return (h->side_auto && batch < SIDE_MIN_BATCH) ? 0 : h->side_mode;
}
int chain_of(const orbx_extractor* h, int in_place, int side_mode, int batch) {
    return (h->hg.chain_ok && in_place && side_mode == 0 && batch <= CHAIN_MAX_BATCH) ? 1 : 0;
}

}  // namespace orbx
