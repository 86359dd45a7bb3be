// orbx_localmap.hip — Tracking::UpdateLocalMap (src/Tracking.cc:1288-1442) on the device
// (include/orbx_localmap.h).
//
// k_update_local_map: one workgroup of 16 waves per frame, over a CSR snapshot of the map.
//   vote       every feature's MapPoint adds 1 to the row entry (by kf_order rank) of each keyframe
//              that observes it: integer atomics, so the counts are exact whatever the order
//   first list the voted, not-bad keyframes in rank order: every wave takes a contiguous range of
//              ranks, counts, and after one exchange of the 16 counts writes its part in place; the
//              reference keyframe is a 64-bit max over (count, lowest rank)
//   extension  wave 0 walks the first list serially (:1385-1435); a ballot over the first 10
//              neighbours / over the child row picks the first eligible one.  The visited set
//              (mnTrackReferenceForFrame) is one bit per slot in LDS
//   points     the rows of the listed keyframes, then the frame's own features as one more row, are
//              cut into chunks of 64 entries; chunk number * 64 + lane is an entry's key, ascending in
//              (list position, feature).  Every MapPoint takes the minimum key (atomicMin), an entry
//              emits its MapPoint only where its key is that minimum, and the waves, each on a
//              contiguous range of chunks, count and then write in key order: the reference's order
//              without a serial walk.  A frame feature's key has the top bit set, so a MapPoint no
//              listed keyframe holds is first seen there: the extras, in feature order.
// Every index read from the caller's arrays is range-checked before it addresses anything; nothing
// of a refused frame is written but its info word, so every output is written after the last check.
//
// k_refresh_map_points (further down): MapPoint::UpdateNormalAndDepth and
// ComputeDistinctiveDescriptors over the same snapshot, one wave per MapPoint.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/orbx_localmap.h"
#include "../../include/orbx_match.h"
#include "orbx_cv.h"
#include "orbx_device.h"
#include "orbx_distinctive.h"
#include "orbx_host.h"

using namespace orbx;

namespace {

constexpr int LM_WAVES = 16;
constexpr int LM_THREADS = 64 * LM_WAVES;
constexpr uint32_t LM_KEY_NONE = 0xffffffffu;
constexpr uint32_t LM_KEY_EXTRA = 0x80000000u;      // | feature index: after every keyframe's key
constexpr uint64_t LM_MAX_UNITS = 1u << 25;         // chunks of 64 entries per frame: keys < 2^31

struct LocalMapLaunch {
    orbx_map_view m;
    const int32_t* feat_mp;
    int32_t feat_stride;
    const int32_t* nfeat;
    const uint8_t* outlier;
    int32_t cap_kf, cap_mp;
    int32_t* local_kf;
    int32_t* n_local_kf;
    int32_t* ref_kf;
    int32_t* local_mp;
    int32_t* n_local_mp;
    orbx_map_point* mps;
    uint8_t* skip;
    int32_t* mp_of_feat;
    uint32_t* info;
    uint8_t* scratch;
};

// One frame's scratch: offsets of its six rows and its size.
struct LmLayout { size_t votes, inv, key, slot, list, ubase, frame; };
__host__ __device__ inline LmLayout lm_layout(int32_t n_kf, int32_t n_mp, int32_t cap_kf) {
    LmLayout l;
    const size_t kf = al256(4 * (size_t)n_kf), mp = al256(4 * (size_t)n_mp),
                 ls = al256(4 * ((size_t)cap_kf + 2));
    l.votes = 0;
    l.inv = kf;
    l.key = 2 * kf;
    l.slot = l.key + mp;
    l.list = l.slot + mp;
    l.ubase = l.list + ls;
    l.frame = l.ubase + ls;
    return l;
}

// Row i of a CSR array of n_entries: false (and an empty row) when its offsets decrease or leave
// the array.
__device__ inline bool lm_row(const int32_t* __restrict__ off, int i, int n_entries, int& b, int& e) {
    b = off[i];
    e = off[i + 1];
    if (b < 0 || e < b || e > n_entries) {
        b = e = 0;
        return false;
    }
    return true;
}

__device__ inline uint64_t lm_shfl_up64(uint64_t v, int d) {
    const uint32_t lo = __shfl_up((uint32_t)v, d), hi = __shfl_up((uint32_t)(v >> 32), d);
    return ((uint64_t)hi << 32) | lo;
}

// Exclusive scan of v over the workgroup; `total` is the sum.  s_w: LM_WAVES words of LDS.
__device__ inline uint64_t lm_block_scan(uint64_t v, uint64_t* s_w, uint64_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint64_t inc = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t t = lm_shfl_up64(inc, d);
        if (lane >= d) inc += t;
    }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    uint64_t before = 0;
    total = 0;
    for (int w = 0; w < LM_WAVES; ++w) {
        if (w < wave) before += s_w[w];
        total += s_w[w];
    }
    __syncthreads();
    return before + inc - v;
}

__device__ inline uint64_t lm_lanes_below() { return (1ull << (threadIdx.x & 63)) - 1; }

__global__ __launch_bounds__(LM_THREADS) void k_update_local_map(const LocalMapLaunch a) {
    __shared__ uint32_t s_visited[ORBX_LOCALMAP_MAX_KF / 32];
    __shared__ uint32_t s_flag[6];      // one word per check: written before its barrier only
    __shared__ uint32_t s_anyvote;
    __shared__ unsigned long long s_best;
    __shared__ uint64_t s_scan[LM_WAVES];
    __shared__ int s_cnt[LM_WAVES], s_cnt2[LM_WAVES];
    __shared__ int s_nlist;

    const orbx_map_view& m = a.m;
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n_kf = m.n_kf, n_mp = m.n_mp;
    const LmLayout lay = lm_layout(n_kf, n_mp, a.cap_kf);
    uint8_t* const base = a.scratch + (size_t)f * lay.frame;
    int32_t* const votes = (int32_t*)(base + lay.votes);
    int32_t* const inv = (int32_t*)(base + lay.inv);
    uint32_t* const key = (uint32_t*)(base + lay.key);
    int32_t* const slot = (int32_t*)(base + lay.slot);
    int32_t* const list = (int32_t*)(base + lay.list);
    uint32_t* const ubase = (uint32_t*)(base + lay.ubase);
    const int32_t* const feat_mp = a.feat_mp + (size_t)f * a.feat_stride;
    const uint8_t* const outlier = a.outlier ? a.outlier + (size_t)f * a.feat_stride : nullptr;

#define LM_REFUSE_IF_FLAGGED(k)                       \
    __syncthreads();                                  \
    if (s_flag[k]) {                                  \
        if (tid == 0) a.info[f] = s_flag[k];          \
        return;                                       \
    }

    // ---- setup: the rank -> slot table, checked to be a permutation -------------------------------
    if (tid < 6) s_flag[tid] = 0;
    if (tid == 0) s_anyvote = 0, s_best = 0, s_nlist = 0;
    for (int w = tid; w < (n_kf + 31) / 32; w += LM_THREADS) s_visited[w] = 0;
    for (int s = tid; s < n_kf; s += LM_THREADS) votes[s] = 0, inv[s] = -1;
    __syncthreads();
    int nfeat = a.nfeat[f];
    if (nfeat < 0 || nfeat > a.feat_stride) {
        if (tid == 0) s_flag[0] = ORBX_LOCALMAP_BAD_INDEX;
        nfeat = 0;
    }
    for (int s = tid; s < n_kf; s += LM_THREADS) {
        const int r = m.kf_order[s];
        if ((uint32_t)r >= (uint32_t)n_kf) s_flag[0] = ORBX_LOCALMAP_BAD_INDEX;
        else inv[r] = s;
    }
    __syncthreads();
    for (int s = tid; s < n_kf; s += LM_THREADS) {
        const int r = m.kf_order[s];
        if ((uint32_t)r < (uint32_t)n_kf && inv[r] != s) s_flag[0] = ORBX_LOCALMAP_BAD_INDEX;
    }
    LM_REFUSE_IF_FLAGGED(0)

    // mvpMapPoints[i] as UpdateLocalKeyFrames leaves it (:1339-1351): -1 for none, an outlier
    // (already nulled, :955-975) or a bad MapPoint.  `bad`: the id is out of range.
    auto feature_id = [&](int i, bool& bad) -> int {
        if (outlier && outlier[i]) return -1;
        const int id = feat_mp[i];
        if (id < -1 || id >= n_mp) {
            bad = true;
            return -1;
        }
        return (id >= 0 && m.mp_bad[id]) ? -1 : id;
    };

    // ---- vote (:1337-1353) ------------------------------------------------------------------------
    {
        bool bad = false, voted = false;
        for (int i = tid; i < nfeat; i += LM_THREADS) {
            const int id = feature_id(i, bad);
            if (id < 0) continue;
            int b, e;
            if (!lm_row(m.mp_obs_off, id, m.n_obs, b, e)) bad = true;
            for (int k = b; k < e; ++k) {
                const int s = m.mp_obs[k];
                if ((uint32_t)s >= (uint32_t)n_kf) {
                    bad = true;
                    continue;
                }
                atomicAdd(&votes[m.kf_order[s]], 1);
                voted = true;
            }
        }
        if (bad) s_flag[1] = ORBX_LOCALMAP_BAD_INDEX;
        if (voted) s_anyvote = 1;
    }
    LM_REFUSE_IF_FLAGGED(1)
    const bool kept = !s_anyvote;          // :1355
    int nfirst = 0;

    if (kept) {
        // the list as it came in; a slot named twice would put its row's entries in twice
        const int n_in = a.n_local_kf[f];
        if (n_in < 0 || n_in > a.cap_kf) {
            if (tid == 0) s_flag[2] = ORBX_LOCALMAP_BAD_INDEX;
        } else {
            for (int p = tid; p < n_in; p += LM_THREADS) {
                const int s = a.local_kf[(size_t)f * a.cap_kf + p];
                if ((uint32_t)s >= (uint32_t)n_kf) {
                    s_flag[2] = ORBX_LOCALMAP_BAD_INDEX;
                    continue;
                }
                list[p] = s;
                const uint32_t bit = 1u << (s & 31);
                if (atomicOr(&s_visited[s >> 5], bit) & bit) s_flag[2] = ORBX_LOCALMAP_BAD_INDEX;
            }
            if (tid == 0) s_nlist = n_in;
        }
    } else {
        // ---- the voted keyframes in rank order (:1366-1381) ----------------------------------------
        const int lo = (int)((int64_t)n_kf * wave / LM_WAVES),
                  hi = (int)((int64_t)n_kf * (wave + 1) / LM_WAVES);
        int cnt = 0;
        unsigned long long best = 0;
        for (int r0 = lo; r0 < hi; r0 += 64) {
            const int r = r0 + lane;
            int v = 0;
            if (r < hi) {
                v = votes[r];
                if (v > 0 && m.kf_bad[inv[r]]) v = 0;     // counted, then skipped (:1370)
            }
            cnt += __popcll(__ballot(v > 0));
            // the strictly largest count at the lowest rank (`>` at :1373)
            if (v > 0) {
                const unsigned long long k = ((unsigned long long)(uint32_t)v << 32) | (uint32_t)~r;
                best = k > best ? k : best;
            }
        }
        if (best) atomicMax(&s_best, best);
        if (lane == 0) s_cnt[wave] = cnt;
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < LM_WAVES; ++w) {
            if (w < wave) before += s_cnt[w];
            total += s_cnt[w];
        }
        if (total > a.cap_kf) {            // the same in every thread
            if (tid == 0) a.info[f] = ORBX_LOCALMAP_CAP_KF;
            return;
        }
        for (int r0 = lo; r0 < hi; r0 += 64) {
            const int r = r0 + lane;
            int s = -1;
            if (r < hi && votes[r] > 0 && !m.kf_bad[inv[r]]) s = inv[r];
            const uint64_t mask = __ballot(s >= 0);
            if (s >= 0) {
                list[before + __popcll(mask & lm_lanes_below())] = s;
                atomicOr(&s_visited[s >> 5], 1u << (s & 31));
            }
            before += __popcll(mask);
        }
        nfirst = total;
        if (tid == 0) s_nlist = total;
    }
    LM_REFUSE_IF_FLAGGED(2)

    // ---- the extension loop (:1385-1435), one wave ------------------------------------------------
    if (wave == 0 && !kept) {
        int n = nfirst;
        uint32_t fl = 0;
        auto visited = [&](int s) { return (s_visited[s >> 5] >> (s & 31)) & 1u; };
        // false: the list is full
        auto push = [&](int s) {
            if (n >= a.cap_kf) {
                fl |= ORBX_LOCALMAP_CAP_KF;
                return false;
            }
            if (lane == 0) {
                list[n] = s;
                s_visited[s >> 5] |= 1u << (s & 31);
            }
            __threadfence_block();
            ++n;
            return true;
        };
        for (int i = 0; i < nfirst; ++i) {
            if (n > 80) break;                                   // :1388
            const int kf = list[i];
            int b, e;
            // GetBestCovisibilityKeyFrames(10): the first not bad, not listed one (:1393-1407)
            if (!lm_row(m.kf_cov_off, kf, m.n_cov, b, e)) fl |= ORBX_LOCALMAP_BAD_INDEX;
            {
                const int len = e - b < 10 ? e - b : 10;
                int nb = -1;
                bool ok = false;
                if (lane < len) {
                    nb = m.kf_cov[b + lane];
                    if ((uint32_t)nb >= (uint32_t)n_kf) fl |= ORBX_LOCALMAP_BAD_INDEX;
                    else ok = !m.kf_bad[nb] && !visited(nb);
                }
                const uint64_t mask = __ballot(ok);
                if (mask && !push(__shfl(nb, __ffsll((unsigned long long)mask) - 1))) break;
            }
            // GetChilds(): the first not bad, not listed one (:1409-1422); the whole row is read
            if (!lm_row(m.kf_child_off, kf, m.n_child, b, e)) fl |= ORBX_LOCALMAP_BAD_INDEX;
            int child = -1;
            for (int c0 = b; c0 < e; c0 += 64) {
                int ch = -1;
                bool ok = false;
                if (c0 + lane < e) {
                    ch = m.kf_child[c0 + lane];
                    if ((uint32_t)ch >= (uint32_t)n_kf) fl |= ORBX_LOCALMAP_BAD_INDEX;
                    else ok = !m.kf_bad[ch] && !visited(ch);
                }
                const uint64_t mask = __ballot(ok);
                const int first = __shfl(ch, mask ? __ffsll((unsigned long long)mask) - 1 : 0);
                if (child < 0 && mask) child = first;
            }
            if (child >= 0 && !push(child)) break;
            // GetParent(): no isBad() test, and the break leaves this loop (:1424-1433)
            const int p = m.kf_parent[kf];
            if (p < -1 || p >= n_kf) fl |= ORBX_LOCALMAP_BAD_INDEX;
            else if (p >= 0 && !visited(p)) {
                push(p);
                break;
            }
        }
        if (fl) atomicOr(&s_flag[3], fl);
        if (lane == 0) s_nlist = n;
    }
    LM_REFUSE_IF_FLAGGED(3)
    const int nl = s_nlist;

    // ---- UpdateLocalPoints (:1299-1322) and the frame's block ---------------------------------------
    // chunks of 64 entries per row; row nl is the frame's own features
    {
        uint64_t carry = 0;
        bool bad = false;
        for (int p0 = 0; p0 <= nl; p0 += LM_THREADS) {
            const int p = p0 + tid;
            uint64_t units = 0;
            if (p < nl) {
                int b, e;
                if (!lm_row(m.kf_mp_off, list[p], m.n_kfmp, b, e)) bad = true;
                units = ((uint64_t)(e - b) + 63) / 64;
            } else if (p == nl) {
                units = ((uint64_t)nfeat + 63) / 64;
            }
            uint64_t total;
            const uint64_t ex = carry + lm_block_scan(units, s_scan, total);
            if (p <= nl) ubase[p] = (uint32_t)ex;
            carry += total;
        }
        if (carry >= LM_MAX_UNITS) bad = true;
        if (tid == 0) ubase[nl + 1] = (uint32_t)carry;
        if (bad) s_flag[4] = ORBX_LOCALMAP_BAD_INDEX;
    }
    LM_REFUSE_IF_FLAGGED(4)
    const uint32_t nunits = ubase[nl + 1];
    const uint32_t u_lo = (uint32_t)((uint64_t)nunits * wave / LM_WAVES),
                   u_hi = (uint32_t)((uint64_t)nunits * (wave + 1) / LM_WAVES);
    int n_local = 0, n_total = 0, base_l = 0, base_e = 0;

    // pass 0: every MapPoint named gets an empty key; 1: the minimum key; 2: count the entries that
    // hold their MapPoint's minimum; 3: write them
    for (int pass = 0; pass < 4; ++pass) {
        bool bad = false;
        int cnt_l = 0, cnt_e = 0;
        if (u_lo < u_hi) {
            int pos = 0;
            {   // the last row whose first chunk is at or before u_lo (rows without entries are passed)
                int lo = 0, hi = nl + 1;
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (ubase[mid] <= u_lo) lo = mid;
                    else hi = mid;
                }
                pos = lo;
            }
            int row_b = 0, row_len = 0, row_pos = -1;
            for (uint32_t u = u_lo; u < u_hi; ++u) {
                while (u >= ubase[pos + 1]) ++pos;
                const bool is_feat = pos == nl;
                if (pos != row_pos) {
                    row_pos = pos;
                    if (is_feat) {
                        row_b = 0, row_len = nfeat;
                    } else {
                        int e;
                        lm_row(m.kf_mp_off, list[pos], m.n_kfmp, row_b, e);
                        row_len = e - row_b;
                    }
                }
                const int j = (int)(u - ubase[pos]) * 64 + lane;
                int id = -1;
                bool live = false;
                uint32_t k;
                if (is_feat) {
                    bool ignored = false;
                    if (j < row_len) id = feature_id(j, ignored);
                    live = id >= 0;
                    k = LM_KEY_EXTRA | (uint32_t)j;
                } else {
                    if (j < row_len) id = m.kf_mp[row_b + j];
                    if (id < -1 || id >= n_mp) {
                        bad = true;
                        id = -1;
                    }
                    live = id >= 0 && !m.mp_bad[id];
                    k = u * 64 + (uint32_t)lane;
                }
                if (pass == 0) {
                    if (id >= 0) key[id] = LM_KEY_NONE;
                } else if (pass == 1) {
                    if (live) atomicMin(&key[id], k);
                } else {
                    const bool first = live && key[id] == k;
                    const uint64_t mask = __ballot(first);
                    const int c = __popcll(mask);
                    if (pass == 2) {
                        if (is_feat) cnt_e += c;
                        else cnt_l += c;
                    } else {
                        int& at = is_feat ? base_e : base_l;
                        if (first) {
                            const int idx = at + __popcll(mask & lm_lanes_below());
                            const size_t o = (size_t)f * a.cap_mp + idx;
                            a.local_mp[o] = id;
                            a.mps[o] = m.mp_rec[id];
                            a.skip[o] = is_feat ? 1 : 0;
                            slot[id] = idx;
                        }
                        at += c;
                    }
                }
            }
        }
        if (pass == 0) {
            if (bad) s_flag[5] = ORBX_LOCALMAP_BAD_INDEX;
            LM_REFUSE_IF_FLAGGED(5)
        } else if (pass == 2) {
            if (lane == 0) s_cnt[wave] = cnt_l, s_cnt2[wave] = cnt_e;
            __syncthreads();
            int extra = 0;
            for (int w = 0; w < LM_WAVES; ++w) {
                if (w < wave) base_l += s_cnt[w], base_e += s_cnt2[w];
                n_local += s_cnt[w];
                extra += s_cnt2[w];
            }
            base_e += n_local;
            n_total = n_local + extra;
            if (n_total > a.cap_mp) {      // the same in every thread
                if (tid == 0) a.info[f] = ORBX_LOCALMAP_CAP_MP;
                return;
            }
        } else {
            __syncthreads();
        }
    }

    // mvpMapPoints as block indices (-1 up to the stride: the scatter and PoseOptimization walk
    // whole strides); a local point the frame holds is not projected (:1261)
    for (int i = tid; i < a.feat_stride; i += LM_THREADS) {
        bool ignored = false;
        const int id = i < nfeat ? feature_id(i, ignored) : -1;
        int idx = -1;
        if (id >= 0) {
            idx = slot[id];
            if (idx < n_local) a.skip[(size_t)f * a.cap_mp + idx] = 1;
        }
        a.mp_of_feat[(size_t)f * a.feat_stride + i] = idx;
    }
    for (int idx = n_total + tid; idx < a.cap_mp; idx += LM_THREADS) {
        const size_t o = (size_t)f * a.cap_mp + idx;
        a.local_mp[o] = -1;
        a.mps[o] = orbx_map_point{};
        a.skip[o] = 1;
    }
    if (!kept) {
        for (int p = tid; p < nl; p += LM_THREADS) a.local_kf[(size_t)f * a.cap_kf + p] = list[p];
        if (tid == 0) {
            a.n_local_kf[f] = nl;
            if (s_best) a.ref_kf[f] = inv[~(uint32_t)s_best];      // :1437-1441
        }
    }
    if (tid == 0) {
        a.n_local_mp[2 * f] = n_local;
        a.n_local_mp[2 * f + 1] = n_total;
        a.info[f] = kept ? ORBX_LOCALMAP_KEPT : 0u;
    }
#undef LM_REFUSE_IF_FLAGGED
}

// ---- the search's inputs next to the block: descriptors per entry, the claimed features --------------
__global__ __launch_bounds__(256) void k_local_map_qdesc(const uint32_t* __restrict__ mp_desc,
                                                         int n_mp, const int32_t* __restrict__ local_mp,
                                                         const int32_t* __restrict__ n_local_mp,
                                                         int cap_mp, uint32_t* __restrict__ qdesc) {
    const int f = blockIdx.y;
    const int nb = n_local_mp[2 * f + 1];
    // 8 threads per descriptor, one word each
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < (int64_t)cap_mp * 8;
         t += (int64_t)gridDim.x * 256) {
        const int k = (int)(t >> 3), w = (int)(t & 7);
        const size_t o = (size_t)f * cap_mp + k;
        uint32_t v = 0;
        if (k < nb) {
            const int id = local_mp[o];
            if ((uint32_t)id < (uint32_t)n_mp) v = mp_desc[(size_t)id * 8 + w];
        }
        qdesc[o * 8 + w] = v;
    }
}

__global__ __launch_bounds__(256) void k_local_map_claimed(
    const int32_t* __restrict__ mp_obs_off, int n_mp, const int32_t* __restrict__ local_mp,
    const int32_t* __restrict__ n_local_mp, int cap_mp, const int32_t* __restrict__ mp_of_feat,
    int feat_stride, const int32_t* __restrict__ nfeat, uint8_t* __restrict__ claimed) {
    const int f = blockIdx.y;
    const int nb = n_local_mp[2 * f + 1], n = nfeat[f];
    for (int i = blockIdx.x * 256 + threadIdx.x; i < feat_stride; i += gridDim.x * 256) {
        uint8_t c = 0;
        if (i < n) {
            const int k = mp_of_feat[(size_t)f * feat_stride + i];
            if (k >= 0 && k < nb && k < cap_mp) {
                const int id = local_mp[(size_t)f * cap_mp + k];
                if ((uint32_t)id < (uint32_t)n_mp) c = mp_obs_off[id + 1] > mp_obs_off[id];
            }
        }
        claimed[(size_t)f * feat_stride + i] = c;
    }
}

// ---- k_refresh_map_points: MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:346-392) and
// MapPoint::ComputeDistinctiveDescriptors (:252-313), one wave per MapPoint ---------------------------
//   order      the row's keys (kf_order rank << 8 | position in the row) are sorted by a bitonic
//              network in LDS: the order std::map<KeyFrame*, size_t> iterates the observations in
//   normal     lane per observation: normali = pos - Ow_i, its double norm, the scaleAdd products
//              into LDS; lanes 0..2 add them in that order, one component each
//   depth      the reference keyframe's feature (feature 0 when it is not in the row)
//   descriptor the descriptors of the keyframes that are not bad, gathered in that order straight
//              into LDS, then distinctive_best (orbx_distinctive.h)
// The waves of a workgroup share nothing and meet at no barrier.  Every index is checked before it
// addresses anything and every check precedes the first write.
constexpr int RF_MAX_WAVES = 4;
constexpr size_t RF_MAX_LDS = 64 * 1024;      // the default dynamic LDS limit: no attribute call
static_assert(ORBX_REFRESH_MAX_OBS == ORBX_MAX_OBSERVATIONS, "one limit on the observation row");

struct RefreshLaunch {
    orbx_map_view m;
    orbx_map_refresh_inputs in;
    const int32_t* ids;
    int32_t n;
    uint32_t what;
    int32_t max_obs;
    orbx_map_point* rec;
    uint32_t* desc;
    uint32_t* info;
};

// One wave's dynamic LDS in 4-byte words from its base: the sort keys (a power of two), the normal
// terms, the descriptors, 64 u16 distance rows of max_obs + 1.
struct RefreshCarve {
    int keys = 0, terms, desc, rows, row_stride, words;
    __host__ __device__ explicit RefreshCarve(int max_obs) {
        int p = 1;
        while (p < max_obs) p <<= 1;
        terms = p;
        desc = terms + 3 * max_obs;
        rows = desc + 8 * max_obs;
        row_stride = max_obs + 1;
        words = rows + 32 * row_stride;
    }
};

// LDS written by some lanes of the wave, read by others
__device__ __forceinline__ void rf_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(64 * RF_MAX_WAVES) void k_refresh_map_points(const RefreshLaunch a) {
    extern __shared__ uint32_t rf_lds[];
    const orbx_map_view& m = a.m;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = (int)blockIdx.x * (int)(blockDim.x >> 6) + wave;
    if (i >= a.n) return;
    const RefreshCarve carve(a.max_obs);
    uint32_t* const base = rf_lds + (size_t)wave * carve.words;
    uint32_t* const keys = base + carve.keys;
    float* const terms = (float*)(base + carve.terms);
    uint32_t* const dl = base + carve.desc;
    uint16_t* const rows = (uint16_t*)(base + carve.rows);
    const int n_kf = m.n_kf;

#define RF_DONE(word)                      \
    {                                      \
        if (lane == 0) a.info[i] = (word); \
        return;                            \
    }
    // everything up to the sort is the same in every lane but `bad`
    const int id = a.ids[i];
    if ((uint32_t)id >= (uint32_t)m.n_mp) RF_DONE(ORBX_REFRESH_BAD_INDEX)
    if (m.mp_bad[id]) RF_DONE(ORBX_REFRESH_SKIPPED_BAD)                     // :354, :261
    int b, e;
    if (!lm_row(m.mp_obs_off, id, m.n_obs, b, e)) RF_DONE(ORBX_REFRESH_BAD_INDEX)
    const int N = e - b;
    if (N == 0) RF_DONE(ORBX_REFRESH_NO_OBS)                                // :361, :266
    if (N > a.max_obs) RF_DONE(ORBX_REFRESH_CAP_OBS)

    // ---- the row's keys, every entry checked ------------------------------------------------------
    int P = 1;
    while (P < N) P <<= 1;
    bool bad = false;
    for (int t = lane; t < P; t += 64) {
        uint32_t key = 0xffffffffu;
        if (t < N) {
            const int s = m.mp_obs[b + t];
            if ((uint32_t)s >= (uint32_t)n_kf) {
                bad = true;
            } else {
                const int r = m.kf_order[s];
                if ((uint32_t)r >= (uint32_t)n_kf) bad = true;
                else key = (uint32_t)r << 8 | (uint32_t)t;
                int fb, fe;
                if (!lm_row(m.kf_mp_off, s, m.n_kfmp, fb, fe) ||
                    (uint32_t)a.in.mp_obs_feat[b + t] >= (uint32_t)(fe - fb))
                    bad = true;
            }
        }
        keys[t] = key;
    }
    if (__ballot(bad)) RF_DONE(ORBX_REFRESH_BAD_INDEX)
    rf_wave_sync();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = lane; t < P; t += 64) {
                const int u = t ^ j;
                if (u > t) {
                    const uint32_t x = keys[t], y = keys[u];
                    if ((x > y) == ((t & k) == 0)) keys[t] = y, keys[u] = x;
                }
            }
            rf_wave_sync();
        }

    // ---- no keyframe twice; the reference keyframe's feature ----------------------------------------
    const int ref = a.in.mp_ref_kf[id];
    if ((uint32_t)ref >= (uint32_t)n_kf) RF_DONE(ORBX_REFRESH_BAD_INDEX)
    int mine = -1;
    for (int t = lane; t < N; t += 64) {
        const uint32_t key = keys[t];
        if (t + 1 < N && (keys[t + 1] >> 8) == (key >> 8)) bad = true;
        const int o = b + (int)(key & 255u);
        if (m.mp_obs[o] == ref) mine = a.in.mp_obs_feat[o];
    }
    const uint64_t holds = __ballot(mine >= 0);
    // observations[pRefKF] on the copy (:377): a keyframe that is not there gets index 0
    const int ref_feat = holds ? __shfl(mine, __ffsll((unsigned long long)holds) - 1) : 0;
    int rb, re;
    if (!lm_row(m.kf_mp_off, ref, m.n_kfmp, rb, re) || ref_feat >= re - rb) bad = true;
    const int nlevels = a.in.kf_pose[ref].nlevels;
    if (nlevels < 1 || nlevels > 16) bad = true;
    int level = 0;
    if (!bad) {
        level = a.in.kf_keys[rb + ref_feat].octave;
        if (level < 0 || level >= nlevels) bad = true;
    }
    if (__ballot(bad)) RF_DONE(ORBX_REFRESH_BAD_INDEX)

    // ---- UpdateNormalAndDepth (:364-390): bad keyframes count -----------------------------------------
    if (a.what & ORBX_REFRESH_NORMAL_DEPTH) {
        const float pos[3] = {a.rec[id].pos[0], a.rec[id].pos[1], a.rec[id].pos[2]};
        for (int t = lane; t < N; t += 64) {
            const float* Ow = a.in.kf_pose[m.mp_obs[b + (int)(keys[t] & 255u)]].Ow;
            const float d[3] = {fs(pos[0], Ow[0]), fs(pos[1], Ow[1]), fs(pos[2], Ow[2])};
            const float alpha = scale_add_alpha(norm3d(d));
#pragma unroll
            for (int k = 0; k < 3; ++k) terms[3 * t + k] = scale_add_term(d[k], alpha);
        }
        rf_wave_sync();
        const orbx_frame_pose& R = a.in.kf_pose[ref];
        const float pc[3] = {fs(pos[0], R.Ow[0]), fs(pos[1], R.Ow[1]), fs(pos[2], R.Ow[2])};
        const float max_dist = fm(norm3(pc), R.scale[level]);
        const float min_dist = fdiv(max_dist, R.scale[nlevels - 1]);
        if (lane < 3) {
            float acc = 0.0f;
            for (int t = 0; t < N; ++t) acc = scale_add_sum(terms[3 * t + lane], acc);
            a.rec[id].normal[lane] = cvt_scale(acc, dv(1.0, (double)N));
        }
        if (lane == 0) {
            a.rec[id].min_dist = min_dist;
            a.rec[id].max_dist = max_dist;
        }
    }

    // ---- ComputeDistinctiveDescriptors (:271-317): bad keyframes are skipped --------------------------
    uint32_t word = 0;
    if (a.what & ORBX_REFRESH_DESCRIPTOR) {
        int M = 0;
        for (int t0 = 0; t0 < N; t0 += 64) {
            const int t = t0 + lane;
            bool good = false;
            long long src = 0;
            if (t < N) {
                const int o = b + (int)(keys[t] & 255u);
                const int s = m.mp_obs[o];
                good = !m.kf_bad[s];
                src = (long long)m.kf_mp_off[s] + a.in.mp_obs_feat[o];
            }
            const uint64_t mask = __ballot(good);
            if (good) {
                const int j = M + lanes_below(mask);
                const uint32_t* sp = (const uint32_t*)a.in.kf_desc + 8 * src;
#pragma unroll
                for (int w = 0; w < 8; ++w) dl[8 * j + w] = sp[w];
            }
            M += __popcll(mask);
        }
        rf_wave_sync();
        if (M == 0) {
            word = ORBX_REFRESH_DESC_KEPT;                                  // :279
        } else {
            const int best = distinctive_best(dl, rows, carve.row_stride, M);
            if (lane < 8) a.desc[(size_t)id * 8 + lane] = dl[best * 8 + lane];
        }
    }
    if (lane == 0) a.info[i] = word;
#undef RF_DONE
}

// The launch geometry of a max_obs: as many waves per workgroup as RF_MAX_LDS holds, RF_MAX_WAVES
// at the most.
struct RefreshGeometry { int waves; size_t lds; };
RefreshGeometry refresh_geometry(int max_obs) {
    const size_t per = 4 * (size_t)RefreshCarve(max_obs).words;
    int waves = (int)(RF_MAX_LDS / per);
    waves = waves < 1 ? 1 : waves > RF_MAX_WAVES ? RF_MAX_WAVES : waves;
    return {waves, per * (size_t)waves};
}

orbx_status rf_check_counts(const orbx_map_view* map, const orbx_map_refresh_inputs* in, int32_t n,
                            uint32_t what, int32_t max_obs) {
    if (!map || !in || n < 0 || map->n_kf < 0 || map->n_mp < 0 || map->n_kfmp < 0 ||
        map->n_obs < 0 || !what || (what & ~(ORBX_REFRESH_NORMAL_DEPTH | ORBX_REFRESH_DESCRIPTOR)) ||
        max_obs < 1 || max_obs > ORBX_REFRESH_MAX_OBS)
        return ORBX_ERR_INVALID;
    if (map->n_kf > ORBX_LOCALMAP_MAX_KF) return ORBX_ERR_UNSUPPORTED;
    return ORBX_OK;
}

// The checks both forms share, on the counts alone.
orbx_status lm_check_counts(const orbx_map_view* map, int32_t nframes, int32_t feat_stride,
                            int32_t cap_kf, int32_t cap_mp) {
    if (!map || nframes < 0 || feat_stride < 0 || feat_stride > ORBX_LOCALMAP_MAX_FEAT ||
        cap_kf < 0 || cap_mp < 0 || map->n_kf < 0 || map->n_mp < 0 || map->n_cov < 0 ||
        map->n_child < 0 || map->n_kfmp < 0 || map->n_obs < 0)
        return ORBX_ERR_INVALID;
    if (map->n_kf > ORBX_LOCALMAP_MAX_KF || nframes > 65535) return ORBX_ERR_UNSUPPORTED;
    return ORBX_OK;
}

}  // namespace

extern "C" {

size_t orbx_update_local_map_scratch_bytes(int32_t n_kf, int32_t n_mp, int32_t nframes,
                                           int32_t cap_kf, int32_t cap_mp) {
    if (n_kf < 0 || n_mp < 0 || nframes < 0 || cap_kf < 0 || cap_mp < 0) return 0;
    return lm_layout(n_kf, n_mp, cap_kf).frame * (size_t)nframes;
}

orbx_status orbx_update_local_map_batch_device(
    const orbx_map_view* map, int32_t nframes, const int32_t* d_feat_mp, int32_t feat_stride,
    const int32_t* d_nfeat, const uint8_t* d_outlier, int32_t cap_kf, int32_t cap_mp,
    int32_t* d_local_kf, int32_t* d_n_local_kf, int32_t* d_ref_kf, int32_t* d_local_mp,
    int32_t* d_n_local_mp, orbx_map_point* d_mps, uint8_t* d_skip, int32_t* d_mp_of_feat,
    uint32_t* d_info, void* d_scratch, size_t scratch_bytes, void* stream) {
    const orbx_status counts = lm_check_counts(map, nframes, feat_stride, cap_kf, cap_mp);
    if (counts != ORBX_OK) return counts;
    if (nframes == 0) return ORBX_OK;
    if (!map->kf_order || !map->kf_bad || !map->kf_parent || !map->kf_cov_off || !map->kf_cov ||
        !map->kf_child_off || !map->kf_child || !map->kf_mp_off || !map->kf_mp || !map->mp_bad ||
        !map->mp_obs_off || !map->mp_obs || !map->mp_rec)
        return ORBX_ERR_INVALID;
    if (!d_feat_mp || !d_nfeat || !d_local_kf || !d_n_local_kf || !d_ref_kf || !d_local_mp ||
        !d_n_local_mp || !d_mps || !d_skip || !d_mp_of_feat || !d_info || !d_scratch)
        return ORBX_ERR_INVALID;
    if (scratch_bytes <
        orbx_update_local_map_scratch_bytes(map->n_kf, map->n_mp, nframes, cap_kf, cap_mp))
        return ORBX_ERR_INVALID;
    int ndev = 0;
    if (!HIPOK(hipGetDeviceCount(&ndev)) || ndev < 1) return ORBX_ERR_DEVICE;
    const LocalMapLaunch L{*map, d_feat_mp, feat_stride, d_nfeat, d_outlier, cap_kf, cap_mp,
                           d_local_kf, d_n_local_kf, d_ref_kf, d_local_mp, d_n_local_mp, d_mps,
                           d_skip, d_mp_of_feat, d_info, (uint8_t*)d_scratch};
    hipLaunchKernelGGL(k_update_local_map, dim3(nframes), dim3(LM_THREADS), 0, (hipStream_t)stream,
                       L);
    return HIPOK(hipGetLastError()) ? ORBX_OK : ORBX_ERR_DEVICE;
}

orbx_status orbx_local_map_search_inputs_batch_device(
    const orbx_map_view* map, const uint8_t* d_mp_desc, int32_t nframes, const int32_t* d_local_mp,
    const int32_t* d_n_local_mp, int32_t cap_mp, const int32_t* d_mp_of_feat, int32_t feat_stride,
    const int32_t* d_nfeat, uint8_t* d_qdesc, uint8_t* d_claimed, void* stream) {
    if (!map || nframes < 0 || nframes > 65535 || cap_mp < 0 || feat_stride < 0 ||
        feat_stride > ORBX_LOCALMAP_MAX_FEAT || map->n_mp < 0)
        return ORBX_ERR_INVALID;
    if (nframes == 0) return ORBX_OK;
    if (!map->mp_obs_off || !d_mp_desc || !d_local_mp || !d_n_local_mp || !d_mp_of_feat || !d_nfeat ||
        !d_qdesc || !d_claimed || ((uintptr_t)d_mp_desc & 3) || ((uintptr_t)d_qdesc & 3))
        return ORBX_ERR_INVALID;
    int ndev = 0;
    if (!HIPOK(hipGetDeviceCount(&ndev)) || ndev < 1) return ORBX_ERR_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    if (cap_mp > 0) {
        const int64_t words = (int64_t)cap_mp * 8;
        hipLaunchKernelGGL(k_local_map_qdesc, dim3((unsigned)((words + 255) / 256), nframes), dim3(256),
                           0, st, (const uint32_t*)d_mp_desc, map->n_mp, d_local_mp, d_n_local_mp,
                           cap_mp, (uint32_t*)d_qdesc);
    }
    if (feat_stride > 0)
        hipLaunchKernelGGL(k_local_map_claimed, dim3((feat_stride + 255) / 256, nframes), dim3(256), 0,
                           st, map->mp_obs_off, map->n_mp, d_local_mp, d_n_local_mp, cap_mp,
                           d_mp_of_feat, feat_stride, d_nfeat, d_claimed);
    return HIPOK(hipGetLastError()) ? ORBX_OK : ORBX_ERR_DEVICE;
}

orbx_status orbx_update_local_map(const orbx_map_view* map, const int32_t* feat_mp, int32_t nfeat,
                                  const uint8_t* outlier, int32_t cap_kf, int32_t cap_mp,
                                  int32_t* local_kf, int32_t* n_local_kf, int32_t* ref_kf,
                                  int32_t* local_mp, int32_t* n_local_mp, orbx_map_point* mps,
                                  uint8_t* skip, int32_t* mp_of_feat, uint32_t* info, int device) {
    const orbx_status counts = lm_check_counts(map, 1, nfeat, cap_kf, cap_mp);
    if (counts != ORBX_OK) return counts;
    const orbx_map_view& m = *map;
    if (!n_local_kf || !ref_kf || !n_local_mp || !info || (nfeat > 0 && (!feat_mp || !mp_of_feat)) ||
        (cap_kf > 0 && !local_kf) || (cap_mp > 0 && (!local_mp || !mps || !skip)) ||
        (m.n_kf > 0 && (!m.kf_order || !m.kf_bad || !m.kf_parent)) || !m.kf_cov_off ||
        !m.kf_child_off || !m.kf_mp_off || !m.mp_obs_off || (m.n_cov > 0 && !m.kf_cov) ||
        (m.n_child > 0 && !m.kf_child) || (m.n_kfmp > 0 && !m.kf_mp) || (m.n_obs > 0 && !m.mp_obs) ||
        (m.n_mp > 0 && (!m.mp_bad || !m.mp_rec)))
        return ORBX_ERR_INVALID;
    HostCall c(device);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    StagePlan& p = c.plan();
    const size_t kf = (size_t)m.n_kf, mp = (size_t)m.n_mp;
    const size_t scratch_bytes = orbx_update_local_map_scratch_bytes(m.n_kf, m.n_mp, 1, cap_kf, cap_mp);
    // an absent array of no entries still needs an address: 4 bytes of zeros
    auto arr = [&](const void* src, size_t bytes) { return p.in(bytes ? src : nullptr, bytes ? bytes : 4); };
    const size_t p_order = arr(m.kf_order, 4 * kf), p_kbad = arr(m.kf_bad, kf),
                 p_par = arr(m.kf_parent, 4 * kf), p_covo = p.in(m.kf_cov_off, 4 * (kf + 1)),
                 p_cov = arr(m.kf_cov, 4 * (size_t)m.n_cov),
                 p_cho = p.in(m.kf_child_off, 4 * (kf + 1)),
                 p_ch = arr(m.kf_child, 4 * (size_t)m.n_child),
                 p_mpo = p.in(m.kf_mp_off, 4 * (kf + 1)), p_kmp = arr(m.kf_mp, 4 * (size_t)m.n_kfmp),
                 p_mbad = arr(m.mp_bad, mp), p_obso = p.in(m.mp_obs_off, 4 * (mp + 1)),
                 p_obs = arr(m.mp_obs, 4 * (size_t)m.n_obs),
                 p_rec = arr(m.mp_rec, sizeof(orbx_map_point) * mp),
                 p_feat = arr(feat_mp, 4 * (size_t)nfeat), p_nfeat = p.in(&nfeat, 4),
                 p_outl = outlier && nfeat ? p.in(outlier, (size_t)nfeat) : StagePlan::NONE;
    // in/out, all of them: a refused frame leaves them as they came in
    auto io = [&](void* q, size_t bytes) { return bytes ? p.inout(q, bytes) : p.in(nullptr, 4); };
    const size_t p_lkf = io(local_kf, 4 * (size_t)cap_kf), p_nlkf = p.inout(n_local_kf, 4),
                 p_ref = p.inout(ref_kf, 4), p_lmp = io(local_mp, 4 * (size_t)cap_mp),
                 p_nlmp = p.inout(n_local_mp, 8),
                 p_mps = io(mps, sizeof(orbx_map_point) * (size_t)cap_mp),
                 p_skip = io(skip, (size_t)cap_mp), p_mpf = io(mp_of_feat, 4 * (size_t)nfeat),
                 p_info = p.inout(info, 4), p_scr = p.scratch(scratch_bytes ? scratch_bytes : 4);
    if (!c.upload()) return c.finish(ORBX_ERR_DEVICE);
    orbx_map_view d = m;
    d.kf_order = c.dev<int32_t>(p_order), d.kf_bad = c.dev<uint8_t>(p_kbad);
    d.kf_parent = c.dev<int32_t>(p_par), d.kf_cov_off = c.dev<int32_t>(p_covo);
    d.kf_cov = c.dev<int32_t>(p_cov), d.kf_child_off = c.dev<int32_t>(p_cho);
    d.kf_child = c.dev<int32_t>(p_ch), d.kf_mp_off = c.dev<int32_t>(p_mpo);
    d.kf_mp = c.dev<int32_t>(p_kmp), d.mp_bad = c.dev<uint8_t>(p_mbad);
    d.mp_obs_off = c.dev<int32_t>(p_obso), d.mp_obs = c.dev<int32_t>(p_obs);
    d.mp_rec = c.dev<orbx_map_point>(p_rec);
    return c.finish(orbx_update_local_map_batch_device(
        &d, 1, c.dev<int32_t>(p_feat), nfeat, c.dev<int32_t>(p_nfeat), c.dev<uint8_t>(p_outl),
        cap_kf, cap_mp, c.dev<int32_t>(p_lkf), c.dev<int32_t>(p_nlkf), c.dev<int32_t>(p_ref),
        c.dev<int32_t>(p_lmp), c.dev<int32_t>(p_nlmp), c.dev<orbx_map_point>(p_mps),
        c.dev<uint8_t>(p_skip), c.dev<int32_t>(p_mpf), c.dev<uint32_t>(p_info),
        c.dev<uint8_t>(p_scr), scratch_bytes ? scratch_bytes : 4, c.st()));
}

orbx_status orbx_refresh_map_points_batch_device(const orbx_map_view* map,
                                                 const orbx_map_refresh_inputs* in,
                                                 const int32_t* d_ids, int32_t n, uint32_t what,
                                                 int32_t max_obs, orbx_map_point* d_mp_rec,
                                                 uint8_t* d_mp_desc, uint32_t* d_info, void* stream) {
    const orbx_status counts = rf_check_counts(map, in, n, what, max_obs);
    if (counts != ORBX_OK) return counts;
    if (n == 0) return ORBX_OK;
    if (!map->kf_order || !map->kf_bad || !map->kf_mp_off || !map->mp_bad || !map->mp_obs_off ||
        !map->mp_obs || !in->mp_obs_feat || !in->mp_ref_kf || !in->kf_pose || !in->kf_keys ||
        !in->kf_desc || !d_ids || !d_mp_rec || !d_mp_desc || !d_info ||
        ((uintptr_t)in->kf_desc & 3) || ((uintptr_t)d_mp_desc & 3))
        return ORBX_ERR_INVALID;
    int ndev = 0;
    if (!HIPOK(hipGetDeviceCount(&ndev)) || ndev < 1) return ORBX_ERR_DEVICE;
    const RefreshLaunch L{*map, *in, d_ids, n, what, max_obs, d_mp_rec, (uint32_t*)d_mp_desc, d_info};
    const RefreshGeometry g = refresh_geometry(max_obs);
    hipLaunchKernelGGL(k_refresh_map_points, dim3((unsigned)((n + g.waves - 1) / g.waves)),
                       dim3(64 * g.waves), g.lds, (hipStream_t)stream, L);
    return HIPOK(hipGetLastError()) ? ORBX_OK : ORBX_ERR_DEVICE;
}

orbx_status orbx_refresh_map_points(const orbx_map_view* map, const orbx_map_refresh_inputs* in,
                                    const int32_t* ids, int32_t n, uint32_t what, int32_t max_obs,
                                    orbx_map_point* mp_rec, uint8_t* mp_desc, uint32_t* info,
                                    int device) {
    const orbx_status counts = rf_check_counts(map, in, n, what, max_obs);
    if (counts != ORBX_OK) return counts;
    const orbx_map_view& m = *map;
    if ((n > 0 && (!ids || !info)) || !m.kf_mp_off || !m.mp_obs_off ||
        (m.n_kf > 0 && (!m.kf_order || !m.kf_bad || !in->kf_pose)) ||
        (m.n_mp > 0 && (!m.mp_bad || !in->mp_ref_kf || !mp_rec || !mp_desc)) ||
        (m.n_obs > 0 && (!m.mp_obs || !in->mp_obs_feat)) ||
        (m.n_kfmp > 0 && (!in->kf_keys || !in->kf_desc)))
        return ORBX_ERR_INVALID;
    if (n == 0) return ORBX_OK;
    HostCall c(device);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    StagePlan& p = c.plan();
    const size_t kf = (size_t)m.n_kf, mp = (size_t)m.n_mp, obs = (size_t)m.n_obs,
                 feat = (size_t)m.n_kfmp;
    // an absent array of no entries still needs an address: 4 bytes of zeros
    auto arr = [&](const void* src, size_t bytes) { return p.in(bytes ? src : nullptr, bytes ? bytes : 4); };
    const size_t p_order = arr(m.kf_order, 4 * kf), p_kbad = arr(m.kf_bad, kf),
                 p_mpo = p.in(m.kf_mp_off, 4 * (kf + 1)), p_mbad = arr(m.mp_bad, mp),
                 p_obso = p.in(m.mp_obs_off, 4 * (mp + 1)), p_obs = arr(m.mp_obs, 4 * obs),
                 p_ofeat = arr(in->mp_obs_feat, 4 * obs), p_ref = arr(in->mp_ref_kf, 4 * mp),
                 p_pose = arr(in->kf_pose, sizeof(orbx_frame_pose) * kf),
                 p_keys = arr(in->kf_keys, sizeof(orbx_keypoint) * feat),
                 p_kdesc = arr(in->kf_desc, 32 * feat), p_ids = p.in(ids, 4 * (size_t)n);
    auto io = [&](void* q, size_t bytes) { return bytes ? p.inout(q, bytes) : p.in(nullptr, 4); };
    const size_t p_rec = io(mp_rec, sizeof(orbx_map_point) * mp), p_desc = io(mp_desc, 32 * mp),
                 p_info = p.inout(info, 4 * (size_t)n);
    if (!c.upload()) return c.finish(ORBX_ERR_DEVICE);
    orbx_map_view d = m;
    d.kf_order = c.dev<int32_t>(p_order), d.kf_bad = c.dev<uint8_t>(p_kbad);
    d.kf_mp_off = c.dev<int32_t>(p_mpo), d.mp_bad = c.dev<uint8_t>(p_mbad);
    d.mp_obs_off = c.dev<int32_t>(p_obso), d.mp_obs = c.dev<int32_t>(p_obs);
    const orbx_map_refresh_inputs di{c.dev<int32_t>(p_ofeat), c.dev<int32_t>(p_ref),
                                     c.dev<orbx_frame_pose>(p_pose), c.dev<orbx_keypoint>(p_keys),
                                     c.dev<uint8_t>(p_kdesc)};
    return c.finish(orbx_refresh_map_points_batch_device(
        &d, &di, c.dev<int32_t>(p_ids), n, what, max_obs, c.dev<orbx_map_point>(p_rec),
        c.dev<uint8_t>(p_desc), c.dev<uint32_t>(p_info), c.st()));
}

}  // extern "C"
