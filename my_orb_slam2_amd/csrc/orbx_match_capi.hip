// orbx_match_capi.hip — the extern "C" matcher boundary (include/orbx_match.h).
//
// Host side: argument validation, one function per launch struct that both the host-array form
// and the *_batch_device form run with the handle's mutex held, the host forms' staging through
// HostCall (orbx_host.h), and the host-only tails of the reference methods (SearchBySim3's
// agreement check :1363-1379, SearchForInitialization's vbPrevMatched update :555-558, the
// (idx1, idx2) pair list of SearchForTriangulation :861-869).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/orbx_match.h"
#include "orbx_host.h"
#include "orbx_kernels.h"
#include "orbx_match_kernels.h"
#include "orbx_matcher.h"

using namespace orbx;

static_assert((int)ORBX_MK_COUNT <= (int)orbx::K_COUNT, "the matcher timer shares KernelTimer's slots");

namespace {

constexpr int MAX_FEAT = 32768;        // per featureset (on-chip claim / state arrays)
constexpr int MAX_POS = 1 << 23;       // grid CSR positions in the 32-bit search keys

bool valid_nodes(const orbx_featureset* f) {
    if (f->n_nodes < 0) return false;
    if (f->n_nodes == 0) return true;
    if (!f->node_id || !f->node_off || !f->node_feat) return false;
    for (int j = 0; j < f->n_nodes; ++j) {
        if (f->node_off[j + 1] < f->node_off[j]) return false;
        if (j > 0 && f->node_id[j] <= f->node_id[j - 1]) return false;
    }
    if (f->node_off[0] < 0) return false;
    for (int k = f->node_off[0]; k < f->node_off[f->n_nodes]; ++k)
        if (f->node_feat[k] < 0 || f->node_feat[k] >= f->n) return false;
    return true;
}

bool valid_grid(const orbx_featureset* f) {
    if (f->grid_cols <= 0 || f->grid_rows <= 0 || !f->grid_off) return false;
    const long long cells = (long long)f->grid_cols * f->grid_rows;
    if (cells > (1 << 20) || f->grid_off[0] != 0) return false;
    for (long long c = 0; c < cells; ++c)
        if (f->grid_off[c + 1] < f->grid_off[c]) return false;
    const int tot = f->grid_off[cells];
    if (tot > MAX_POS || (tot > 0 && !f->grid_feat)) return false;
    for (int k = 0; k < tot; ++k)
        if (f->grid_feat[k] < 0 || f->grid_feat[k] >= f->n) return false;
    return true;
}

bool valid_feat(const orbx_featureset* f, bool nodes, bool grid) {
    if (!f || f->n < 0 || f->n > MAX_FEAT) return false;
    if (f->n > 0 && (!f->keys || !f->desc)) return false;
    if (nodes && !valid_nodes(f)) return false;
    if (grid && !valid_grid(f)) return false;
    return true;
}

// The members of a device orbx_kf_db that a call reads: the feature arrays and the node CSR
// always, node_id (DB_NODE_ID) for the matchers that pair nodes by id, and (DB_NODE_ORDERED) the
// optional node-ordered copies, all there or none.  desc and node_desc are read as 16-byte words.
enum { DB_NODE_ID = 1, DB_NODE_ORDERED = 2 };
bool valid_kf_db(const orbx_kf_db* db, int need) {
    if (!db->feat_off || !db->keys || !db->desc || !db->flag || !db->node_off ||
        !db->node_feat_off || !db->node_feat || ((need & DB_NODE_ID) && !db->node_id) ||
        ((uintptr_t)db->desc & 15))
        return false;
    if ((need & DB_NODE_ORDERED) &&
        (db->node_keys || db->node_desc || db->node_flag || db->node_u_right) &&
        (!db->node_keys || !db->node_desc || !db->node_flag ||
         (db->u_right != nullptr) != (db->node_u_right != nullptr) ||
         ((uintptr_t)db->node_desc & 15)))
        return false;
    return true;
}

// A keyframe database built from host featuresets: its parts in the call's plan.
struct DbParts {
    size_t feat_off, keys, desc, u_right, flag, node_off, node_id, node_feat_off, node_feat;
    int nkf, max_feat;
};

DbParts pack_db(StagePlan& P, const orbx_featureset* const* fs, const uint8_t* const* flags,
                int nkf) {
    DbParts o{};
    o.nkf = nkf;
    int nf = 0, nn = 0, nnf = 0;
    for (int k = 0; k < nkf; ++k) {
        nf += fs[k]->n;
        nn += fs[k]->n_nodes;
        if (fs[k]->n_nodes > 0) nnf += fs[k]->node_off[fs[k]->n_nodes] - fs[k]->node_off[0];
        o.max_feat = std::max(o.max_feat, fs[k]->n);
    }
    o.feat_off = P.in(nullptr, 4 * (nkf + 1));
    o.keys = P.in(nullptr, sizeof(orbx_keypoint) * (size_t)nf);
    o.desc = P.in(nullptr, 32 * (size_t)nf);
    o.u_right = P.in(nullptr, 4 * (size_t)nf);
    o.flag = P.in(nullptr, (size_t)nf);
    o.node_off = P.in(nullptr, 4 * (nkf + 1));
    o.node_id = P.in(nullptr, 4 * (size_t)nn);
    o.node_feat_off = P.in(nullptr, 4 * ((size_t)nn + 1));
    o.node_feat = P.in(nullptr, 4 * (size_t)nnf);
    // every part is declared: the block stays where it is while they are filled
    int32_t* feat_off = P.host<int32_t>(o.feat_off);
    int32_t* node_off = P.host<int32_t>(o.node_off);
    int32_t* node_feat_off = P.host<int32_t>(o.node_feat_off);
    int f0 = 0, n0 = 0, e0 = 0;
    for (int k = 0; k < nkf; ++k) {
        const orbx_featureset* f = fs[k];
        feat_off[k] = f0;
        node_off[k] = n0;
        if (f->n > 0) {
            std::memcpy(P.host<orbx_keypoint>(o.keys) + f0, f->keys, sizeof(orbx_keypoint) * f->n);
            std::memcpy(P.host<uint8_t>(o.desc) + 32 * (size_t)f0, f->desc, 32 * (size_t)f->n);
            float* ur = P.host<float>(o.u_right) + f0;
            for (int i = 0; i < f->n; ++i) ur[i] = f->u_right ? f->u_right[i] : -1.0f;
            uint8_t* fl = P.host<uint8_t>(o.flag) + f0;
            for (int i = 0; i < f->n; ++i) fl[i] = (flags && flags[k]) ? (flags[k][i] != 0) : 0;
        }
        for (int j = 0; j < f->n_nodes; ++j) {
            P.host<uint32_t>(o.node_id)[n0 + j] = f->node_id[j];
            node_feat_off[n0 + j] = e0 + f->node_off[j] - f->node_off[0];
        }
        if (f->n_nodes > 0) {
            const int cnt = f->node_off[f->n_nodes] - f->node_off[0];
            std::memcpy(P.host<int32_t>(o.node_feat) + e0, f->node_feat + f->node_off[0], 4 * (size_t)cnt);
            e0 += cnt;
        }
        f0 += f->n;
        n0 += f->n_nodes;
    }
    feat_off[nkf] = f0;
    node_off[nkf] = n0;
    node_feat_off[n0] = e0;
    return o;
}

orbx_kf_db dev_db(const DbParts& o, uint8_t* base) {
    orbx_kf_db d{};
    d.nkf = o.nkf;
    d.max_feat = o.max_feat;
    d.feat_off = (const int32_t*)(base + o.feat_off);
    d.keys = (const orbx_keypoint*)(base + o.keys);
    d.desc = base + o.desc;
    d.u_right = (const float*)(base + o.u_right);
    d.flag = base + o.flag;
    d.node_off = (const int32_t*)(base + o.node_off);
    d.node_id = (const uint32_t*)(base + o.node_id);
    d.node_feat_off = (const int32_t*)(base + o.node_feat_off);
    d.node_feat = (const int32_t*)(base + o.node_feat);
    return d;
}

// A single featureset with its grid (projection searches).
struct FeatParts {
    size_t keys, desc, u_right, grid_off, grid_feat;
};

FeatParts pack_feat(StagePlan& P, const orbx_featureset* f) {
    FeatParts o{};
    const size_t cells = (size_t)f->grid_cols * f->grid_rows;
    o.keys = P.in(f->keys, sizeof(orbx_keypoint) * (size_t)f->n);
    o.desc = P.in(f->desc, 32 * (size_t)f->n);
    o.u_right = P.in(nullptr, 4 * (size_t)f->n);
    o.grid_off = P.in(f->grid_off, 4 * (cells + 1));
    o.grid_feat = P.in(f->grid_feat, 4 * (size_t)f->grid_off[cells]);
    float* ur = P.host<float>(o.u_right);
    for (int i = 0; i < f->n; ++i) ur[i] = f->u_right ? f->u_right[i] : -1.0f;
    return o;
}

orbx_featureset dev_feat(const orbx_featureset* f, const FeatParts& o, uint8_t* base) {
    orbx_featureset d = *f;
    d.keys = (const orbx_keypoint*)(base + o.keys);
    d.desc = base + o.desc;
    d.u_right = (const float*)(base + o.u_right);
    d.n_nodes = 0;
    d.node_id = nullptr;
    d.node_off = nullptr;
    d.node_feat = nullptr;
    d.grid_off = (const int32_t*)(base + o.grid_off);
    d.grid_feat = (const int32_t*)(base + o.grid_feat);
    return d;
}

// The capacity word of one host-array call: a part of its own, zeroed on the device too because
// k_bow, k_triangulate, k_proj_claim / k_proj_init and k_distinctive only ever OR into it.  The handle's
// d_err belongs to the *_device forms alone.
size_t err_part(StagePlan& P) { return P.out(nullptr, sizeof(int), /*zeroed=*/true); }

orbx_status finish(HostCall& c, size_t p_err, orbx_status s) {
    s = c.finish(s);
    return (s == ORBX_OK && *c.plan().host<int>(p_err)) ? ORBX_ERR_CAPACITY : s;
}

// The three launch bodies below run with m->mu held, from the host-array form (device pointers
// into its HostCall block, `err` its own word) and from the *_batch_device form (the caller's
// pointers, m->d_err).

orbx_status run_bow(orbx_matcher* m, const orbx_kf_db& A, const orbx_kf_db& B, int a_fixed,
                    int kf_kf, int njobs, int32_t* out, int out_stride, int32_t* nmatches,
                    int* err, hipStream_t st) {
    BowLaunch L{};
    L.A = A;
    L.B = B;
    L.a_fixed = a_fixed;
    L.b_fixed = 1;
    L.kf_kf = kf_kf;
    L.njobs = njobs;
    L.ratio = m->prm.nnratio;
    L.check_ori = m->prm.check_orientation;
    L.out = out;
    L.out_stride = out_stride;
    L.nmatches = nmatches;
    L.err = err;
    if (bow_lds_bytes(L) > MATCH_MAX_LDS) return ORBX_ERR_UNSUPPORTED;
    hipEvent_t e = m->timer.start(st);
    if (!HIPOK(launch_bow(L, st))) return ORBX_ERR_DEVICE;
    m->timer.stop(ORBX_MK_BOW, e, st);
    return ORBX_OK;
}

orbx_status run_tri(orbx_matcher* m, const orbx_kf_db& db, int njobs, const int32_t* kf1,
                    const int32_t* kf2, const float* F12, const float* epi, const float* sigma2,
                    const float* scale, int nlevels, int only_stereo, const int32_t* job_off,
                    int32_t* out, int32_t* nmatches, int* err, hipStream_t st) {
    TriLaunch L{};
    L.db = db;
    L.njobs = njobs;
    L.kf1 = kf1;
    L.kf2 = kf2;
    L.F12 = F12;
    L.epi = epi;
    for (int l = 0; l < MATCH_MAX_LEVELS; ++l) {
        L.sigma2[l] = l < nlevels ? sigma2[l] : 0.f;
        L.scale[l] = l < nlevels ? scale[l] : 0.f;
    }
    L.only_stereo = only_stereo;
    L.check_ori = m->prm.check_orientation;
    L.job_off = job_off;
    L.out = out;
    L.nmatches = nmatches;
    L.err = err;
    if (tri_lds_bytes(db.max_feat) > TRI_MAX_LDS) return ORBX_ERR_UNSUPPORTED;
    hipEvent_t e = m->timer.start(st);
    if (!HIPOK(launch_triangulate(L, st))) return ORBX_ERR_DEVICE;
    m->timer.stop(ORBX_MK_TRIANGULATE, e, st);
    return ORBX_OK;
}

// The scratch of one projection search over njobs targets and nq queries in all: offsets from a
// 256-byte aligned base.  A kernel writes every region before one reads it, so none is zeroed:
// k_proj_search writes cand / ncand for k_proj_claim, top2 for k_proj_init; either replay writes
// the bins of its matches and hist (counted from zero in its LDS) for k_proj_finish.
struct ProjScratch {
    size_t hist, top2, bins, cand, ncand, end;
};
ProjScratch proj_scratch(int njobs, size_t nq) {
    ProjScratch s{};
    s.top2 = al256(128 * (size_t)njobs);
    s.bins = s.top2 + al256(16 * nq);
    s.cand = s.bins + al256(nq);
    s.ncand = s.cand + al256(8 * PROJ_K * nq);
    s.end = s.ncand + al256(4 * nq);
    return s;
}

// T: the targets' device arrays with T.n = the largest target; t_off / g_off / q_off are null
// for a single job.  scratch: proj_scratch(njobs, nq).end bytes.
orbx_status run_proj(orbx_matcher* m, int mode, const orbx_featureset& T, int njobs,
                     const int32_t* t_off, const int32_t* g_off, const int32_t* q_off,
                     const uint8_t* claimed, const uint8_t* qdesc, const orbx_proj_query* q,
                     const uint8_t* qflags, int nq, const float* inv_sigma2, int nlevels,
                     int orb_dist, int flags, uint8_t* scratch, int32_t* out, int32_t* nmatches,
                     int* err, hipStream_t st) {
    const ProjScratch s = proj_scratch(njobs, (size_t)nq);
    ProjLaunch L{};
    L.mode = mode;
    L.T = T;
    L.T.n_nodes = 0;
    L.T.node_id = nullptr;
    L.T.node_off = nullptr;
    L.T.node_feat = nullptr;
    L.njobs = njobs;
    L.t_off = t_off;
    L.g_off = g_off;
    L.q_off = q_off;
    L.max_t = T.n;
    L.qdesc = qdesc;
    L.q = q;
    L.nq = nq;
    for (int l = 0; l < MATCH_MAX_LEVELS; ++l)
        L.inv_sigma2[l] = (inv_sigma2 && l < nlevels) ? inv_sigma2[l] : 0.f;
    L.orb_dist = orb_dist;
    L.ratio = m->prm.nnratio;
    L.check_ori = m->prm.check_orientation;
    L.claimed_in = claimed;
    L.qflags = qflags;
    L.prefilter = (flags & ORBX_PROJ_PREFILTER) != 0;
    L.out = out;
    L.top2 = (int4*)(scratch + s.top2);
    L.cand = (int2*)(scratch + s.cand);
    L.ncand = (int32_t*)(scratch + s.ncand);
    L.out_bin = (int8_t*)(scratch + s.bins);
    L.hist = (int32_t*)(scratch + s.hist);
    L.nmatches = nmatches;
    L.err = err;
    if (proj_replay_lds_bytes(mode, L.max_t, nq) > MATCH_MAX_LDS) return ORBX_ERR_UNSUPPORTED;
    if (nq == 0)   // every job: no queries, no matches
        return HIPOK(hipMemsetAsync(nmatches, 0, 4 * (size_t)njobs, st)) ? ORBX_OK : ORBX_ERR_DEVICE;
    return HIPOK(launch_proj(L, st, &m->timer)) ? ORBX_OK : ORBX_ERR_DEVICE;
}

orbx_status bow_common(orbx_matcher* m, const orbx_featureset* a, const uint8_t* va,
                       const orbx_featureset* b, const uint8_t* vb, int kf_kf, int32_t* out,
                       int32_t* nmatches) {
    if (!m || !out || !nmatches || !va || (kf_kf && !vb)) return ORBX_ERR_INVALID;
    if (!valid_feat(a, true, false) || !valid_feat(b, true, false)) return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(m->mu);
    HostCall c(m->prm.device);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    StagePlan& P = c.plan();
    const DbParts pa = pack_db(P, &a, &va, 1), pb = pack_db(P, &b, &vb, 1);
    const int nout = kf_kf ? a->n : b->n;
    const size_t p_out = P.out(out, 4 * (size_t)nout), p_n = P.out(nmatches, 4),
                 p_err = err_part(P);
    if (!c.upload()) return c.finish(ORBX_ERR_DEVICE);
    uint8_t* base = c.dev<uint8_t>(0);
    return finish(c, p_err, run_bow(m, dev_db(pa, base), dev_db(pb, base), 1, kf_kf, 1,
                                    c.dev<int32_t>(p_out), nout, c.dev<int32_t>(p_n),
                                    c.dev<int>(p_err), c.st()));
}

// The size limits of one projection search (any mode, PROJ_INIT included) as the host forms
// apply them (valid_feat, proj_common, run_proj), for orbx_matcher_variant.
orbx_status proj_size_status(int mode, int n_target, int nq) {
    if (nq < 0 || nq > (1 << 22) || n_target < 0 || n_target > MAX_FEAT) return ORBX_ERR_INVALID;
    if (proj_replay_lds_bytes(mode, n_target, nq) > MATCH_MAX_LDS) return ORBX_ERR_UNSUPPORTED;
    return ORBX_OK;
}

orbx_status proj_common(orbx_matcher* m, int mode, const orbx_featureset* T,
                        const uint8_t* claimed, const uint8_t* qdesc, const orbx_proj_query* q,
                        int nq, const float* inv_sigma2, int nlevels, int orb_dist, int32_t* out,
                        int32_t* nmatches, const uint8_t* qflags = nullptr, int flags = 0) {
    if (!m || !out || !nmatches || nq < 0 || nq > (1 << 22)) return ORBX_ERR_INVALID;
    if (nq > 0 && (!qdesc || !q)) return ORBX_ERR_INVALID;
    if (!valid_feat(T, false, true)) return ORBX_ERR_INVALID;
    if (mode == ORBX_PROJ_FUSE && (!inv_sigma2 || nlevels <= 0)) return ORBX_ERR_INVALID;
    if (nlevels > MATCH_MAX_LEVELS) return ORBX_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(m->mu);
    HostCall c(m->prm.device);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    StagePlan& P = c.plan();
    const FeatParts pt = pack_feat(P, T);
    const size_t p_q = P.in(q, sizeof(orbx_proj_query) * (size_t)nq), p_d = P.in(qdesc, 32 * (size_t)nq),
                 p_c = P.in_opt(claimed, (size_t)T->n), p_f = P.in_opt(qflags, (size_t)nq),
                 p_out = P.out(out, 4 * (size_t)nq), p_n = P.out(nmatches, 4),
                 p_err = err_part(P), p_scr = P.scratch(proj_scratch(1, (size_t)nq).end);
    if (!c.upload()) return c.finish(ORBX_ERR_DEVICE);
    return finish(c, p_err,
                  run_proj(m, mode, dev_feat(T, pt, c.dev<uint8_t>(0)), 1, nullptr, nullptr,
                           nullptr, c.dev<uint8_t>(p_c), c.dev<uint8_t>(p_d),
                           c.dev<orbx_proj_query>(p_q), c.dev<uint8_t>(p_f), nq, inv_sigma2,
                           nlevels, orb_dist, flags, c.dev<uint8_t>(p_scr), c.dev<int32_t>(p_out),
                           c.dev<int32_t>(p_n), c.dev<int>(p_err), c.st()));
}

}  // namespace

extern "C" {

orbx_status orbx_matcher_create(const orbx_matcher_params* params, orbx_matcher** out) {
    if (!out) return ORBX_ERR_INVALID;
    *out = nullptr;
    orbx_matcher_params p{0.6f, 1, 0};
    if (params) p = *params;
    if (!(p.nnratio > 0.f) || p.device < 0) return ORBX_ERR_INVALID;
    int ndev = 0;
    if (!HIPOK(hipGetDeviceCount(&ndev)) || ndev <= 0) return ORBX_ERR_DEVICE;
    if (p.device >= ndev) return ORBX_ERR_INVALID;
    orbx_matcher* m = new orbx_matcher();
    m->prm = p;
    if (!HIPOK(hipSetDevice(p.device)) ||
        !HIPOK(hipMalloc((void**)&m->d_err, 64)) || !HIPOK(hipMemset(m->d_err, 0, 64)) ||
        !HIPOK(hipEventCreateWithFlags(&m->bf_done, hipEventDisableTiming)) ||
        !HIPOK(prepare_match_kernels())) {
        orbx_matcher_destroy(m);
        return ORBX_ERR_DEVICE;
    }
    hipDeviceProp_t prop;
    if (HIPOK(hipGetDeviceProperties(&prop, p.device)) && prop.multiProcessorCount > 0)
        m->ncu = prop.multiProcessorCount;
    *out = m;
    return ORBX_OK;
}

orbx_status orbx_matcher_destroy(orbx_matcher* m) {
    if (!m) return ORBX_ERR_INVALID;
    (void)hipSetDevice(m->prm.device);
    if (m->have_bf) (void)hipEventSynchronize(m->bf_done);
    if (m->bf_done) (void)hipEventDestroy(m->bf_done);
    m->d_aux.release();
    m->d_proj.release();
    m->d_bf.release();
    m->d_bf_db.release();
    m->d_sim3.release();
    m->d_pnp.release();
    if (m->d_err) (void)hipFree(m->d_err);
    m->timer.destroy();
    delete m;
    return ORBX_OK;
}

void orbx_compute_three_maxima(const int32_t* histo, int32_t L, int32_t* ind1, int32_t* ind2,
                               int32_t* ind3) {
    int max1 = 0, max2 = 0, max3 = 0;
    int a = ind1 ? *ind1 : -1, b = ind2 ? *ind2 : -1, c = ind3 ? *ind3 : -1;
    for (int i = 0; histo && i < L; i++) {
        const int s = histo[i];
        if (s > max1) {
            max3 = max2; max2 = max1; max1 = s;
            c = b; b = a; a = i;
        } else if (s > max2) {
            max3 = max2; max2 = s;
            c = b; b = i;
        } else if (s > max3) {
            max3 = s; c = i;
        }
    }
    if (max2 < 0.1f * (float)max1) {
        b = -1; c = -1;
    } else if (max3 < 0.1f * (float)max1) {
        c = -1;
    }
    if (ind1) *ind1 = a;
    if (ind2) *ind2 = b;
    if (ind3) *ind3 = c;
}

orbx_status orbx_search_by_bow_kf_frame(orbx_matcher* m, const orbx_featureset* kf,
                                        const uint8_t* kf_valid, const orbx_featureset* f,
                                        int32_t* match_f, int32_t* nmatches) {
    return bow_common(m, kf, kf_valid, f, nullptr, 0, match_f, nmatches);
}

orbx_status orbx_search_by_bow_kf_kf(orbx_matcher* m, const orbx_featureset* kf1,
                                     const uint8_t* valid1, const orbx_featureset* kf2,
                                     const uint8_t* valid2, int32_t* match12, int32_t* nmatches) {
    return bow_common(m, kf1, valid1, kf2, valid2, 1, match12, nmatches);
}

orbx_status orbx_search_for_triangulation(orbx_matcher* m, const orbx_featureset* kf1,
                                          const uint8_t* has_mp1, const orbx_featureset* kf2,
                                          const uint8_t* has_mp2, const float* F12, float ex,
                                          float ey, const float* sigma2_2, const float* scale_2,
                                          int32_t nlevels, int32_t only_stereo, int32_t* pairs,
                                          int32_t pair_cap, int32_t* nmatches) {
    if (!m || !has_mp1 || !has_mp2 || !F12 || !sigma2_2 || !scale_2 || !nmatches ||
        nlevels <= 0 || pair_cap < 0 || (pair_cap > 0 && !pairs))
        return ORBX_ERR_INVALID;
    if (nlevels > MATCH_MAX_LEVELS) return ORBX_ERR_UNSUPPORTED;
    if (!valid_feat(kf1, true, false) || !valid_feat(kf2, true, false)) return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(m->mu);
    HostCall c(m->prm.device);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    StagePlan& P = c.plan();
    const orbx_featureset* fs[2] = {kf1, kf2};
    const uint8_t* fl[2] = {has_mp1, has_mp2};
    const DbParts pd = pack_db(P, fs, fl, 2);
    const int32_t job[4] = {0, 1, 0, kf1->n};   // kf1, kf2, job_off[0], job_off[1]
    const float epi[2] = {ex, ey};
    const size_t p_job = P.in(job, sizeof(job)), p_F = P.in(F12, 9 * sizeof(float)),
                 p_epi = P.in(epi, sizeof(epi)), p_m12 = P.out(nullptr, 4 * (size_t)kf1->n),
                 p_n = P.out(nmatches, 4), p_err = err_part(P);
    if (!c.upload()) return c.finish(ORBX_ERR_DEVICE);
    const int32_t* d_job = c.dev<int32_t>(p_job);
    const orbx_status s =
        finish(c, p_err,
               run_tri(m, dev_db(pd, c.dev<uint8_t>(0)), 1, d_job, d_job + 1, c.dev<float>(p_F),
                       c.dev<float>(p_epi), sigma2_2, scale_2, nlevels, only_stereo, d_job + 2,
                       c.dev<int32_t>(p_m12), c.dev<int32_t>(p_n), c.dev<int>(p_err), c.st()));
    if (s != ORBX_OK) return s;
    // vMatchedPairs in idx1 order (:861-869)
    const int32_t* m12 = P.host<int32_t>(p_m12);
    int np = 0;
    for (int i = 0; i < kf1->n; ++i) {
        if (m12[i] < 0) continue;
        if (np < pair_cap) {
            pairs[2 * np] = i;
            pairs[2 * np + 1] = m12[i];
        }
        ++np;
    }
    return np > pair_cap ? ORBX_ERR_CAPACITY : ORBX_OK;
}

orbx_status orbx_search_by_projection(orbx_matcher* m, int32_t mode,
                                      const orbx_featureset* target, const uint8_t* claimed,
                                      const uint8_t* qdesc, const orbx_proj_query* q,
                                      int32_t nq, const float* inv_sigma2, int32_t nlevels,
                                      int32_t orb_dist, int32_t* match_q, int32_t* nmatches) {
    if (mode < 0 || mode >= ORBX_PROJ_MODE_COUNT) return ORBX_ERR_INVALID;
    return proj_common(m, mode, target, claimed, qdesc, q, nq, inv_sigma2, nlevels, orb_dist,
                       match_q, nmatches);
}

orbx_status orbx_search_by_projection_ex(orbx_matcher* m, int32_t mode,
                                         const orbx_featureset* target, const uint8_t* claimed,
                                         const uint8_t* qdesc, const orbx_proj_query* q,
                                         const uint8_t* qflags, int32_t nq,
                                         const float* inv_sigma2, int32_t nlevels,
                                         int32_t orb_dist, int32_t flags, int32_t* match_q,
                                         int32_t* nmatches) {
    if (mode < 0 || mode >= ORBX_PROJ_MODE_COUNT || (flags & ~ORBX_PROJ_PREFILTER) || !m)
        return ORBX_ERR_INVALID;
    // LAST_FRAME's rotation filter runs per feature in the reference (:1516-1535): with
    // no-claim queries a feature can be matched twice and sit in two bins, which a per-query
    // filter cannot reproduce, so that combination needs the caller's own filter (PREFILTER)
    if (mode == ORBX_PROJ_LAST_FRAME && m->prm.check_orientation && !(flags & ORBX_PROJ_PREFILTER) &&
        qflags && nq > 0)
        for (int32_t i = 0; i < nq; ++i)
            if (qflags[i] & ORBX_QF_NO_CLAIM) return ORBX_ERR_INVALID;
    return proj_common(m, mode, target, claimed, qdesc, q, nq, inv_sigma2, nlevels, orb_dist,
                       match_q, nmatches, qflags, flags);
}

orbx_status orbx_search_by_sim3(orbx_matcher* m, const orbx_featureset* kf1,
                                const orbx_featureset* kf2, const uint8_t* qdesc1,
                                const orbx_proj_query* q12, int32_t n1, const uint8_t* qdesc2,
                                const orbx_proj_query* q21, int32_t n2, int32_t* match12,
                                int32_t* nmatches) {
    if (!kf1 || !kf2 || !match12 || !nmatches || n1 < 0 || n2 < 0) return ORBX_ERR_INVALID;
    std::vector<int32_t> v1((size_t)n1 + 1), v2((size_t)n2 + 1);
    int32_t c1 = 0, c2 = 0;
    orbx_status s = proj_common(m, ORBX_PROJ_SIM3, kf2, nullptr, qdesc1, q12, n1, nullptr, 0, 0,
                                v1.data(), &c1);
    if (s != ORBX_OK) return s;
    s = proj_common(m, ORBX_PROJ_SIM3, kf1, nullptr, qdesc2, q21, n2, nullptr, 0, 0, v2.data(),
                    &c2);
    if (s != ORBX_OK) return s;
    int nFound = 0;
    for (int i1 = 0; i1 < n1; ++i1) {   // :1366-1379
        match12[i1] = -1;
        const int idx2 = v1[i1];
        if (idx2 >= 0 && idx2 < n2 && v2[idx2] == i1) {
            match12[i1] = idx2;
            ++nFound;
        }
    }
    *nmatches = nFound;
    return ORBX_OK;
}

orbx_status orbx_search_for_initialization(orbx_matcher* m, const orbx_featureset* f1,
                                           const orbx_featureset* f2, float* prev_matched,
                                           int32_t window_size, int32_t* match12,
                                           int32_t* nmatches) {
    if (!f1 || !f2 || !prev_matched || !match12 || !nmatches) return ORBX_ERR_INVALID;
    if (!valid_feat(f1, false, false)) return ORBX_ERR_INVALID;
    const int n1 = f1->n;
    // one query per F1 feature (:459-466): level-0 features search F2 around vbPrevMatched
    std::vector<orbx_proj_query> q((size_t)n1);
    for (int i = 0; i < n1; ++i) {
        const int level1 = f1->keys[i].octave;
        q[i].u = prev_matched[2 * i];
        q[i].v = prev_matched[2 * i + 1];
        q[i].ur = 0.f;
        q[i].radius = level1 > 0 ? -1.0f : (float)window_size;
        q[i].min_level = level1;
        q[i].max_level = level1;
        q[i].pred_level = 0;
        q[i].angle = f1->keys[i].angle;
    }
    orbx_status s = proj_common(m, PROJ_INIT, f2, nullptr, f1->desc, q.data(), n1, nullptr, 0,
                                0, match12, nmatches);
    if (s != ORBX_OK) return s;
    for (int i = 0; i < n1; ++i)   // :555-558
        if (match12[i] >= 0) {
            prev_matched[2 * i] = f2->keys[match12[i]].x;
            prev_matched[2 * i + 1] = f2->keys[match12[i]].y;
        }
    return ORBX_OK;
}

orbx_status orbx_search_by_bow_kf_frame_batch_device(orbx_matcher* m, const orbx_kf_db* db,
                                                     const orbx_featureset* f,
                                                     int32_t* d_match, int32_t* d_nmatches,
                                                     void* stream) {
    if (!m || !db || !f || !d_match || !d_nmatches) return ORBX_ERR_INVALID;
    if (db->nkf < 0 || db->max_feat < 0 || db->max_feat > MAX_FEAT || f->n < 0 || f->n > MAX_FEAT)
        return ORBX_ERR_INVALID;
    if (db->nkf == 0) return ORBX_OK;
    if (!valid_kf_db(db, DB_NODE_ID) || (f->n > 0 && (!f->keys || !f->desc)) ||
        (f->n_nodes > 0 && (!f->node_id || !f->node_off || !f->node_feat)) ||
        ((uintptr_t)f->desc & 15))
        return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(m->mu);
    if (!HIPOK(hipSetDevice(m->prm.device))) return ORBX_ERR_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    // The frame as a one-keyframe database: its CSR offsets are already absolute.
    if (!m->d_aux.ensure(64)) return ORBX_ERR_DEVICE;
    int32_t offs[4] = {0, f->n, 0, f->n_nodes};
    if (!HIPOK(hipMemcpyAsync(m->d_aux.p, offs, sizeof(offs), hipMemcpyHostToDevice, st)))
        return ORBX_ERR_DEVICE;
    orbx_kf_db B{};
    B.nkf = 1;
    B.max_feat = f->n;
    B.feat_off = m->d_aux.as<int32_t>();
    B.keys = f->keys;
    B.desc = f->desc;
    B.u_right = f->u_right;
    B.flag = db->flag;   // not read for SearchByBoW(KeyFrame*, Frame&)
    B.node_off = m->d_aux.as<int32_t>() + 2;
    B.node_id = f->node_id;
    B.node_feat_off = f->node_off;
    B.node_feat = f->node_feat;
    return run_bow(m, *db, B, 0, 0, db->nkf, d_match, f->n, d_nmatches, m->d_err, st);
}

orbx_status orbx_search_for_triangulation_batch_device(
    orbx_matcher* m, const orbx_kf_db* db, int32_t njobs, const int32_t* d_kf1,
    const int32_t* d_kf2, const float* d_F12, const float* d_epi, const float* sigma2,
    const float* scale, int32_t nlevels, int32_t only_stereo, const int32_t* d_job_off,
    int32_t* d_match12, int32_t* d_nmatches, void* stream) {
    if (!m || !db || njobs < 0 || !sigma2 || !scale || nlevels <= 0) return ORBX_ERR_INVALID;
    if (nlevels > MATCH_MAX_LEVELS) return ORBX_ERR_UNSUPPORTED;
    if (db->max_feat < 0 || db->max_feat > MAX_FEAT) return ORBX_ERR_INVALID;
    if (njobs == 0) return ORBX_OK;
    if (!d_kf1 || !d_kf2 || !d_F12 || !d_epi || !d_job_off || !d_match12 || !d_nmatches ||
        !valid_kf_db(db, DB_NODE_ID | DB_NODE_ORDERED))
        return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(m->mu);
    if (!HIPOK(hipSetDevice(m->prm.device))) return ORBX_ERR_DEVICE;
    return run_tri(m, *db, njobs, d_kf1, d_kf2, d_F12, d_epi, sigma2, scale, nlevels, only_stereo,
                   d_job_off, d_match12, d_nmatches, m->d_err, (hipStream_t)stream);
}


orbx_status orbx_triangulate_matches_batch_device(
    orbx_matcher* m, const orbx_kf_db* db, int32_t njobs, const int32_t* d_kf1,
    const int32_t* d_kf2, const orbx_frame_pose* d_poses, const float* d_depth,
    const float* d_cos_stereo, const orbx_keypoint* d_keys_raw, float mb, float ratio_factor,
    const int32_t* d_job_off, const int32_t* d_match12, int32_t* d_status, float* d_x3d,
    int32_t* d_nnew, void* stream) {
    if (!m || !db || njobs < 0 || njobs > 65535 || !(mb >= 0.0f)) return ORBX_ERR_INVALID;
    if (db->max_feat < 0 || db->max_feat > MAX_FEAT) return ORBX_ERR_INVALID;
    if (njobs == 0) return ORBX_OK;
    if (!d_kf1 || !d_kf2 || !d_poses || !d_depth || !d_cos_stereo || !d_job_off || !d_match12 ||
        !d_status || !d_x3d || !d_nnew || !db->feat_off || !db->keys)
        return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(m->mu);
    if (!HIPOK(hipSetDevice(m->prm.device))) return ORBX_ERR_DEVICE;
    TriPointsLaunch L{};
    L.nkf = db->nkf;
    L.feat_off = db->feat_off;
    L.keys = db->keys;
    L.keys_raw = d_keys_raw;
    L.u_right = db->u_right;
    L.depth = d_depth;
    L.cos_stereo = d_cos_stereo;
    L.poses = d_poses;
    L.kf1 = d_kf1;
    L.kf2 = d_kf2;
    L.job_off = d_job_off;
    L.match12 = d_match12;
    L.ratio_factor = ratio_factor;
    L.status = d_status;
    L.x3d = d_x3d;
    L.nnew = d_nnew;
    L.err = m->d_err;
    if (!HIPOK(launch_triangulate_points(L, db->max_feat, njobs, (hipStream_t)stream)))
        return ORBX_ERR_DEVICE;
    return ORBX_OK;
}

orbx_status orbx_search_by_projection_batch_device(
    orbx_matcher* m, int32_t mode, const orbx_featureset* frames, int32_t njobs,
    const int32_t* d_feat_off, const int32_t* d_grid_off, int32_t max_feat,
    const uint8_t* d_claimed, const uint8_t* d_qdesc, const orbx_proj_query* d_q,
    const int32_t* d_q_off, int32_t nq, const float* inv_sigma2, int32_t nlevels,
    int32_t orb_dist, int32_t* d_match, int32_t* d_nmatches, void* stream) {
    if (!m || !frames || njobs < 0 || nq < 0 || nq > (1 << 24)) return ORBX_ERR_INVALID;
    if (mode < 0 || mode >= ORBX_PROJ_MODE_COUNT) return ORBX_ERR_INVALID;
    if (max_feat < 0 || max_feat > MAX_FEAT) return ORBX_ERR_INVALID;
    if (mode == ORBX_PROJ_FUSE && (!inv_sigma2 || nlevels <= 0)) return ORBX_ERR_INVALID;
    if (nlevels > MATCH_MAX_LEVELS) return ORBX_ERR_UNSUPPORTED;
    if (frames->grid_cols <= 0 || frames->grid_rows <= 0 ||
        (long long)frames->grid_cols * frames->grid_rows > (1 << 20))
        return ORBX_ERR_INVALID;
    if (njobs == 0) return ORBX_OK;
    if (!d_feat_off || !d_grid_off || !d_q_off || !d_match || !d_nmatches || !frames->keys ||
        !frames->desc || !frames->grid_off || !frames->grid_feat || (nq > 0 && (!d_qdesc || !d_q)))
        return ORBX_ERR_INVALID;
    if (((uintptr_t)frames->desc & 15) || ((uintptr_t)d_qdesc & 15)) return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(m->mu);
    if (!HIPOK(hipSetDevice(m->prm.device))) return ORBX_ERR_DEVICE;
    if (!m->d_proj.ensure(proj_scratch(njobs, (size_t)nq).end)) return ORBX_ERR_DEVICE;
    orbx_featureset T = *frames;
    T.n = max_feat;
    return run_proj(m, mode, T, njobs, d_feat_off, d_grid_off, d_q_off, d_claimed, d_qdesc, d_q,
                    nullptr, nq, inv_sigma2, nlevels, orb_dist, 0, m->d_proj.as<uint8_t>(), d_match,
                    d_nmatches, m->d_err, (hipStream_t)stream);
}

orbx_status orbx_compute_distinctive_descriptors(orbx_matcher* m, const uint8_t* desc,
                                                 const int32_t* off, int32_t npoints,
                                                 int32_t* best) {
    if (!m || !off || !best || npoints < 0) return ORBX_ERR_INVALID;
    if (npoints == 0) return ORBX_OK;
    if (off[0] < 0) return ORBX_ERR_INVALID;
    for (int p = 0; p < npoints; ++p) {
        if (off[p + 1] < off[p]) return ORBX_ERR_INVALID;
        if (off[p + 1] - off[p] > ORBX_MAX_OBSERVATIONS) return ORBX_ERR_UNSUPPORTED;
    }
    const int n = off[npoints] - off[0];
    if (n > 0 && !desc) return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(m->mu);
    HostCall c(m->prm.device);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    StagePlan& P = c.plan();
    const size_t p_d = P.in(n > 0 ? desc + 32 * (size_t)off[0] : nullptr, 32 * (size_t)n),
                 p_off = P.in(nullptr, 4 * ((size_t)npoints + 1)),
                 p_best = P.out(best, 4 * (size_t)npoints), p_err = err_part(P);
    int32_t* rel = P.host<int32_t>(p_off);
    for (int p = 0; p <= npoints; ++p) rel[p] = off[p] - off[0];
    if (!c.upload()) return c.finish(ORBX_ERR_DEVICE);
    hipEvent_t e = m->timer.start(c.st());
    if (!HIPOK(launch_distinctive(c.dev<uint8_t>(p_d), c.dev<int32_t>(p_off), npoints,
                                  c.dev<int32_t>(p_best), c.dev<int>(p_err), c.st())))
        return c.finish(ORBX_ERR_DEVICE);
    m->timer.stop(ORBX_MK_DISTINCTIVE, e, c.st());
    return finish(c, p_err, ORBX_OK);
}


orbx_status orbx_compute_distinctive_descriptors_device(orbx_matcher* m, const uint8_t* d_desc,
                                                        const int32_t* d_off, int32_t npoints,
                                                        int32_t* d_best, void* stream) {
    if (!m || !d_off || !d_best || !d_desc || npoints < 0) return ORBX_ERR_INVALID;
    if (npoints == 0) return ORBX_OK;
    std::lock_guard<std::mutex> lk(m->mu);
    if (!HIPOK(hipSetDevice(m->prm.device))) return ORBX_ERR_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    hipEvent_t e = m->timer.start(st);
    if (!HIPOK(launch_distinctive(d_desc, d_off, npoints, d_best, m->d_err, st)))
        return ORBX_ERR_DEVICE;
    m->timer.stop(ORBX_MK_DISTINCTIVE, e, st);
    return ORBX_OK;
}

namespace {
// Rows per chunk of a call on this handle: the caller's override, else bf_chunk_rows
int bf_chunk_of(const orbx_matcher* m, long long ndb, int nq) {
    return m->bf_chunk ? m->bf_chunk : bf_chunk_rows(ndb, nq, m->ncu, m->bf_kernel);
}

orbx_status bf_run(orbx_matcher* m, const uint8_t* d_q, int nq, const uint8_t* d_db,
                   long long ndb, long long idx_base, int32_t* bi, int32_t* bd, int32_t* sd,
                   hipStream_t st) {
    BfLaunch a{};
    a.q = d_q;
    a.nq = nq;
    a.db = d_db;
    a.ndb = ndb;
    a.idx_base = idx_base;
    a.chunk = bf_chunk_of(m, ndb, nq);
    const size_t need = bf_partial_bytes(ndb, nq, a.chunk);
    // growing frees the scratch an earlier launch (any stream) may still use
    if (need > m->d_bf.n && m->have_bf && !HIPOK(hipEventSynchronize(m->bf_done)))
        return ORBX_ERR_DEVICE;
    if (!m->d_bf.ensure(need)) return ORBX_ERR_DEVICE;
    // the previous launch on another stream must be done with the scratch
    if (m->have_bf && m->bf_stream != st && !HIPOK(hipStreamWaitEvent(st, m->bf_done, 0)))
        return ORBX_ERR_DEVICE;
    a.part = m->d_bf.p;
    a.best_idx = bi;
    a.best_dist = bd;
    a.second_dist = sd;
    a.kernel = m->bf_kernel;
    if (!HIPOK(launch_bf_top2(a, st, &m->timer)) || !HIPOK(hipEventRecord(m->bf_done, st)))
        return ORBX_ERR_DEVICE;
    m->bf_stream = st;
    m->have_bf = true;
    return ORBX_OK;
}
}  // namespace

orbx_status orbx_hamming_bf_top2(orbx_matcher* m, const uint8_t* q, int32_t nq,
                                 const uint8_t* db, int64_t ndb, int32_t* best_idx,
                                 int32_t* best_dist, int32_t* second_dist) {
    if (!m || nq < 0 || ndb < 0 || ndb >= INT32_MAX) return ORBX_ERR_INVALID;
    if (nq == 0) return ORBX_OK;
    if (!q || !best_idx || !best_dist || !second_dist || (ndb > 0 && !db)) return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(m->mu);
    HostCall c(m->prm.device);
    if (!c.ok()) return ORBX_ERR_DEVICE;
    StagePlan& P = c.plan();
    const size_t dbb = 32 * (size_t)ndb, ob = 4 * (size_t)nq;
    const size_t p_q = P.in(q, 32 * (size_t)nq), p_bi = P.out(best_idx, ob),
                 p_bd = P.out(best_dist, ob), p_sd = P.out(second_dist, ob);
    // the database goes from the caller's pointer to the handle's own buffer, past the host
    // block; the call drains c.st() before it returns, so the next one may overwrite or grow it
    if (!m->d_bf_db.ensure(std::max<size_t>(dbb, 32)) || !c.upload() ||
        (dbb && !HIPOK(hipMemcpyAsync(m->d_bf_db.p, db, dbb, hipMemcpyHostToDevice, c.st()))))
        return c.finish(ORBX_ERR_DEVICE);
    return c.finish(bf_run(m, c.dev<uint8_t>(p_q), nq, m->d_bf_db.as<uint8_t>(), ndb, 0,
                           c.dev<int32_t>(p_bi), c.dev<int32_t>(p_bd), c.dev<int32_t>(p_sd),
                           c.st()));
}


const char* orbx_bf_kernel(void) { return orbx::bf_kernel_name(ORBX_BF_MFMA); }

const char* orbx_bf_kernel_name(int32_t kernel) { return orbx::bf_kernel_name(kernel); }

orbx_status orbx_matcher_set_bf_kernel(orbx_matcher* m, int32_t kernel) {
    if (!m || !orbx::bf_kernel_name(kernel)) return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(m->mu);
    m->bf_kernel = kernel;
    return ORBX_OK;
}

orbx_status orbx_matcher_set_bf_chunk(orbx_matcher* m, int64_t rows) {
    if (!m || (rows != 0 && !orbx::bf_chunk_valid(rows))) return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(m->mu);
    m->bf_chunk = (int)rows;
    return ORBX_OK;
}

orbx_status orbx_matcher_bf_launch_info(orbx_matcher* m, int32_t nq, int64_t ndb,
                                        orbx_bf_launch_info* out) {
    if (!m || !out || nq < 0 || ndb < 0 || ndb >= INT32_MAX) return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(m->mu);
    const int chunk = bf_chunk_of(m, ndb, nq);
    const orbx::BfGeometry g = orbx::bf_geometry(ndb, nq, chunk, m->bf_kernel);
    out->chunk = chunk;
    out->nchunks = (int32_t)g.nchunks;
    out->query_blocks = g.query_blocks;
    out->nqpad = g.nqpad;
    out->merge_slice = g.merge_slice;
    out->partial_bytes = (int64_t)g.partial_bytes;
    return ORBX_OK;
}

orbx_status orbx_hamming_bf_top2_device(orbx_matcher* m, const uint8_t* d_q, int32_t nq,
                                        const uint8_t* d_db, int64_t ndb, int64_t idx_base,
                                        int32_t* d_best_idx, int32_t* d_best_dist,
                                        int32_t* d_second_dist, void* stream) {
    if (!m || nq < 0 || ndb < 0 || idx_base < 0 || ndb + idx_base >= INT32_MAX)
        return ORBX_ERR_INVALID;
    // the kernels read both arrays as dwords (k_bf_top2 by scalar loads, which drop the
    // address's low two bits without a fault)
    if ((((uintptr_t)d_q) | ((uintptr_t)d_db)) & 3u) return ORBX_ERR_INVALID;
    if (nq == 0) return ORBX_OK;
    if (!d_q || !d_best_idx || !d_best_dist || !d_second_dist || (ndb > 0 && !d_db))
        return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(m->mu);
    if (!HIPOK(hipSetDevice(m->prm.device))) return ORBX_ERR_DEVICE;
    return bf_run(m, d_q, nq, d_db, ndb, idx_base, d_best_idx, d_best_dist, d_second_dist,
                  (hipStream_t)stream);
}

orbx_status orbx_kf_db_node_order(orbx_matcher* m, const orbx_kf_db* db, int32_t n,
                                  orbx_keypoint* d_keys, uint8_t* d_desc, float* d_u_right,
                                  uint8_t* d_flag, void* stream) {
    if (!m || !db || n < 0 || db->nkf < 0) return ORBX_ERR_INVALID;
    if (db->nkf == 0 || n == 0) return ORBX_OK;
    if (!valid_kf_db(db, 0) || !d_keys || !d_desc || !d_flag || (db->u_right && !d_u_right) ||
        ((uintptr_t)d_desc & 15))
        return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(m->mu);
    if (!HIPOK(hipSetDevice(m->prm.device))) return ORBX_ERR_DEVICE;
    orbx_kf_db d = *db;
    d.node_keys = nullptr;
    d.node_desc = nullptr;
    d.node_u_right = nullptr;
    d.node_flag = nullptr;
    if (!HIPOK(launch_node_order(d, n, d_keys, d_desc, db->u_right ? d_u_right : nullptr, d_flag,
                                 (hipStream_t)stream)))
        return ORBX_ERR_DEVICE;
    return ORBX_OK;
}

orbx_status orbx_matcher_sync(orbx_matcher* m, void* stream) {
    if (!m) return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(m->mu);
    if (!HIPOK(hipSetDevice(m->prm.device))) return ORBX_ERR_DEVICE;
    int err = 0;
    hipStream_t st = (hipStream_t)stream;
    if (!HIPOK(hipMemcpyAsync(&err, m->d_err, sizeof(int), hipMemcpyDeviceToHost, st)) ||
        !HIPOK(hipStreamSynchronize(st)) || !HIPOK(hipMemset(m->d_err, 0, sizeof(int))))
        return ORBX_ERR_DEVICE;
    return err ? ORBX_ERR_CAPACITY : ORBX_OK;
}

orbx_status orbx_matcher_profile_enable(orbx_matcher* m, int on) {
    if (!m) return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(m->mu);
    m->timer.on = on != 0;
    return ORBX_OK;
}

orbx_status orbx_matcher_profile_collect(orbx_matcher* m, double* total_ms, int64_t* launches) {
    if (!m) return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(m->mu);
    m->timer.collect();
    for (int k = 0; k < ORBX_MK_COUNT; ++k) {
        if (total_ms) total_ms[k] = m->timer.ms[k];
        if (launches) launches[k] = m->timer.n[k];
        m->timer.ms[k] = 0;
        m->timer.n[k] = 0;
    }
    return ORBX_OK;
}

int32_t orbx_matcher_variant(int32_t kind, int32_t n_a, int32_t n_b, int32_t nq) {
    if (kind == ORBX_VK_BOW_KF_FRAME || kind == ORBX_VK_BOW_KF_KF) {
        if (n_a < 0 || n_a > MAX_FEAT || n_b < 0 || n_b > MAX_FEAT) return ORBX_ERR_INVALID;
        BowLaunch L{};   // bow_lds_bytes / bow_b_in_lds read the two bounds and the flavour only
        L.A.max_feat = n_a;
        L.B.max_feat = n_b;
        L.kf_kf = kind == ORBX_VK_BOW_KF_KF;
        if (bow_lds_bytes(L) > MATCH_MAX_LDS) return ORBX_ERR_UNSUPPORTED;
        return bow_b_in_lds(L) ? 0 : 1;
    }
    if (kind == ORBX_VK_INIT) {
        if (n_a < 0 || n_a > MAX_FEAT) return ORBX_ERR_INVALID;
        return proj_size_status(PROJ_INIT, n_b, n_a);   // one query per F1 feature
    }
    const int mode = kind - ORBX_VK_PROJ;
    if (mode < 0 || mode >= ORBX_PROJ_MODE_COUNT) return ORBX_ERR_INVALID;
    const orbx_status s = proj_size_status(mode, n_b, nq);
    if (s != ORBX_OK) return s;
    return (proj_replay(mode) != REPLAY_CLAIM || ClaimCarve(n_b).owner_words) ? 0 : 1;
}

const char* orbx_match_kernel_name(int id) {
    static const char* names[ORBX_MK_COUNT] = {"k_bow", "k_triangulate", "k_proj_search",
                                               "k_proj_resolve", "k_distinctive"};
    return (id >= 0 && id < ORBX_MK_COUNT) ? names[id] : "";
}

}  // extern "C"
