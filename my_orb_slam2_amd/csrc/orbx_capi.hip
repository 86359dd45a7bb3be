// orbx_capi.hip — the extern "C" boundary (include/orbx.h) over the gfx950 kernels.
//
// Host responsibilities: the handle, its HBM workspace, the ordering of its calls across
// streams, the launch descriptors and the graphed host-image sequence.  The tables and the
// per-size geometry come from orbx_plan.hip; orbx_stereo_frame_view is orbx_stereo_frame.hip.
#include <algorithm>
#include <chrono>
#include <shared_mutex>
#include <thread>

#include "orbx_extractor.h"

#ifndef ORBX_SRC_HASH
#define ORBX_SRC_HASH "0000000000000000"   // my_orb_slam2_amd/build.py passes the real one
#endif
// "orbx-src:<hash>" is also how build.py finds the hash in the binary (staleness check)
#define ORBX_VERSION "orbx 0.3.0 (gfx950) orbx-src:" ORBX_SRC_HASH

using namespace orbx;

namespace orbx {

// Stream captures (graph_current) against waits on an event recorded on another stream: the
// runtime refuses hipStreamWaitEvent (hipErrorStreamCaptureIsolation) while the stream the event
// was last recorded on is being captured, even when the record came before the capture began.
// A handle's done event can sit on another handle's stream (orbx_stereo_match records the right
// handle's on the left's), whose thread may be capturing a graph just then (a handle re-captures
// when its pinned blocks grow), so such waits and the captures exclude each other.  Captures
// happen on a handle's first calls and after a regrowth; the waits take the lock shared.
static std::shared_mutex g_capture_mu;

// Orders stream st after all work issued so far for this handle (on whatever stream).
bool order_after_last(orbx_extractor* h, hipStream_t st) {
    if (h->have_done && h->done_stream != st) {
        std::shared_lock<std::shared_mutex> lk(g_capture_mu);
        return HIPOK(hipStreamWaitEvent(st, h->done, 0));
    }
    return true;
}

// Marks the end of the work just issued for this handle on st.
bool mark_done(orbx_extractor* h, hipStream_t st) {
    h->done_stream = st;
    h->have_done = true;
    return HIPOK(hipEventRecord(h->done, st));
}

// Waits (host) until the handle's issued work has finished: its tables may then change and
// its buffers grow.  Other streams and handles on the device keep running.
bool wait_idle(orbx_extractor* h) {
    return !h->have_done || HIPOK(hipEventSynchronize(h->done));
}

// The host wait of the single-image calls (orbx_extract, orbx_stereo_match): polls the handle's
// last event for up to WAIT_SPIN_US (yielding the core between polls) before a blocking wait.
// A blocking wait returns tens of microseconds after the work ends (the thread sleeps); the
// drop-in path waits twice per stereo frame on its critical path.
#define WAIT_SPIN_US 400
bool wait_done(orbx_extractor* h) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipEventQuery(h->done);
        if (e == hipSuccess) return true;
        if (e != hipErrorNotReady) return HIPOK(e);
        if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(WAIT_SPIN_US)) break;
        std::this_thread::yield();
    }
    return HIPOK(hipEventSynchronize(h->done));
}

// Host staging buffer (pinned) of at least n bytes.
bool ensure_pinned(uint8_t*& p, size_t& cap, size_t n) {
    if (p && cap >= n) return true;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    if (!HIPOK(hipHostMalloc((void**)&p, n, hipHostMallocDefault))) { p = nullptr; return false; }
    cap = n;
    return true;
}

void set_last(orbx_extractor* h, int batch, bool valid, int pyr_images, int n) {
    if (batch) h->last_batch = batch;
    h->last_valid = valid;
    if (valid) h->last_n = n;
    h->pyr_images = pyr_images;
    ++h->serial;
}

orbx_status ensure_workspace(orbx_extractor* h, int W, int H, int batch) {
    if (batch < 1) return ORBX_ERR_INVALID;
    if (!HIPOK(hipSetDevice(h->device))) return ORBX_ERR_DEVICE;
    const bool same = h->have_geom && h->hg.width == W && h->hg.height == H;
    if (!same) {
        // this handle's earlier calls may still read the old tables (on their streams)
        if (!wait_idle(h)) return ORBX_ERR_DEVICE;
        // Everything the handle holds was laid out by the old geometry, and every query
        // describes it with h->hg: the host pyramid copy (orbx_host_pyramid_view), the device
        // pyramids (orbx_pyramid_level) and the outputs of the last call (orbx_batch_fetch,
        // orbx_stereo_match) stop being valid here, whether or not the new size is supported
        // or the uploads below succeed; the next extraction refills them.
        h->have_geom = false;
        h->host_pyr_ok = false;
        set_last(h, 0, false, 0);
        orbx_status s = build_geometry(h->prm, W, H, *h);
        if (s != ORBX_OK) return s;
        if (!h->d_geom.ensure(sizeof(Geometry))) return ORBX_ERR_DEVICE;
        if (!h->d_cells.ensure(std::max<size_t>(h->cells.size(), 1) * sizeof(CellDesc))) return ORBX_ERR_DEVICE;
        if (!h->d_rtab.ensure(std::max<size_t>(h->rtab.size(), 1) * 2)) return ORBX_ERR_DEVICE;
        if (!h->d_ltab.ensure(std::max<size_t>(h->ltab.size(), 16))) return ORBX_ERR_DEVICE;
        // uploads on the handle's own (non-blocking) stream: nothing else on the device waits
        hipStream_t st = h->stream;
        if (!HIPOK(hipMemcpyAsync(h->d_ltab.p, h->ltab.data(), h->ltab.size(), hipMemcpyHostToDevice, st)) ||
            !HIPOK(hipMemcpyAsync(h->d_geom.p, &h->hg, sizeof(Geometry), hipMemcpyHostToDevice, st)))
            return ORBX_ERR_DEVICE;
        if (!h->cells.empty() &&
            !HIPOK(hipMemcpyAsync(h->d_cells.p, h->cells.data(), h->cells.size() * sizeof(CellDesc),
                                  hipMemcpyHostToDevice, st)))
            return ORBX_ERR_DEVICE;
        if (!h->rtab.empty() &&
            !HIPOK(hipMemcpyAsync(h->d_rtab.p, h->rtab.data(), h->rtab.size() * 2, hipMemcpyHostToDevice, st)))
            return ORBX_ERR_DEVICE;
        if (!HIPOK(hipStreamSynchronize(st))) return ORBX_ERR_DEVICE;
        if (!HIPOK(prepare_kernels(std::max(h->octree_lds, h->octree_lds_small), h->stereo_lds,
                                   (size_t)h->hg.chain_lds, fast_lds_bytes(h->hg))))
            return ORBX_ERR_DEVICE;
        h->have_geom = true;
        h->cap_batch = 0;
    }
    if (batch > h->cap_batch) {
        // growing frees the old buffers: the handle's work in flight must be done
        if (!wait_idle(h)) return ORBX_ERR_DEVICE;
        set_last(h, 0, false, 0);   // the pyramids and the last call's outputs go with them
        const Geometry& G = h->hg;
        const size_t B = (size_t)batch;
        // k_fast reads up to 4 * FAST_PF2D rows past a cell's ROI
        const size_t pyr_slack = (size_t)4 * FAST_PF2D * G.lv[0].pitch + 256;
        bool ok = h->d_pyr.ensure(B * G.pyr_bytes + pyr_slack) &&
                  h->d_blur.ensure(B * G.pyr_bytes) &&
                  h->d_ccnt.ensure(B * std::max(G.n_cells, 1) * 4) &&
                  h->d_cand.ensure(B * G.cand_words * 4) &&
                  h->d_ocnt.ensure(B * G.nlevels * 4) && h->d_okp.ensure(B * G.out_words * 6) &&
                  h->d_kscr.ensure(B * h->kscratch_per_image);
        // the outputs of the B images, then one pair's stereo block
        const OutLayout ol(B, (size_t)G.kp_cap);
        ok = ok && h->d_outs.ensure(ol.after(B) + StereoLayout(1, ol.KC).end);
        if (!ok) return ORBX_ERR_DEVICE;
        h->out = ol;   // with the views below and cap_batch: only once everything is allocated
        uint8_t* ob = h->d_outs.as<uint8_t>();
        h->d_nkp.view(ob, B * 4);
        h->d_kps.view(ob + h->out.o_kps, h->out.kps_end(B) - h->out.o_kps);
        h->d_desc.view(ob + h->out.o_desc, h->out.desc_end(B) - h->out.o_desc);
        h->cap_batch = batch;
    }
    return ORBX_OK;
}

// The launch descriptor of one batched extraction (d_imgs == nullptr: level 0 of every image
// is already in the pyramid, in place).
ExtractLaunch extract_launch(orbx_extractor* h, const uint8_t* d_imgs, const uint8_t* d_imgs2,
                             int split, int batch, size_t stride, size_t batch_stride) {
    ExtractLaunch a;
    a.in_place = d_imgs == nullptr;
    if (a.in_place) {
        d_imgs = h->d_pyr.as<uint8_t>();
        d_imgs2 = nullptr;
        stride = (size_t)h->hg.lv[0].pitch;
        batch_stride = (size_t)h->hg.pyr_bytes;
    }
    a.hg = &h->hg;
    a.dg = h->d_geom.as<Geometry>();
    a.cells = h->d_cells.as<CellDesc>();
    a.rtab = h->d_rtab.as<int16_t>();
    a.ltab = h->d_ltab.as<uint8_t>();
    a.d_imgs = d_imgs;
    a.d_imgs2 = d_imgs2 ? d_imgs2 : d_imgs;
    a.split = d_imgs2 ? split : batch;
    a.stride = stride;
    a.batch_stride = batch_stride;
    a.batch = batch;
    a.pyr = h->d_pyr.as<uint8_t>();
    a.blur = h->d_blur.as<uint8_t>();
    a.ccnt = h->d_ccnt.as<int>();
    a.cand = h->d_cand.as<uint32_t>();
    a.ocnt = h->d_ocnt.as<int>();
    a.okp = h->d_okp.as<uint32_t>();
    a.operm = (uint16_t*)(a.okp + (size_t)batch * h->hg.out_words);
    a.kscratch = h->d_kscr.as<uint8_t>();
    a.kscratch_per_image = h->kscratch_per_image;
    a.ncap = h->ncap;
    a.kcap = h->kcap;
    a.octree_lds = h->octree_lds;
    a.kcap_small = h->kcap_small;
    a.octree_lds_small = h->octree_lds_small;
    a.oct_small = octree_small(batch);
    a.fast_nc = fast_cells_per_wave(h->hg.n_cells, batch, h->ncu);
    a.kps = h->d_kps.as<float>();
    a.desc = h->d_desc.as<uint8_t>();
    a.nkp = h->d_nkp.as<int>();
    a.timer = &h->timer;
    a.side = h->side;
    a.ev_fork = h->ev_fork;
    a.ev_join = h->ev_join;
    // the default schedule forks the side branch only for batches that can fill the chip: a
    // small batch's kernels are latency chains, and the fork / join events between the two
    // streams cost more than the overlap gives (an explicit orbx_extractor_set_overlap applies
    // at every batch size)
    a.side_mode = side_mode_of(h, batch);
    a.side_at = h->side_at;
    a.side_lv = h->side_lv;
    a.chain = chain_of(h, a.in_place, a.side_mode, batch);
    strip_heights(h, batch, a.sth);
    return a;
}

static orbx_status run_extract(orbx_extractor* h, const uint8_t* d_imgs, const uint8_t* d_imgs2,
                               int split, int batch, size_t stride, size_t batch_stride,
                               hipStream_t st) {
    const ExtractLaunch a = extract_launch(h, d_imgs, d_imgs2, split, batch, stride, batch_stride);
    if (!order_after_last(h, st)) return ORBX_ERR_DEVICE;
    if (!HIPOK(launch_extract(a, st)) || !mark_done(h, st)) return ORBX_ERR_DEVICE;
    set_last(h, batch, true, batch);   // the count: orbx_extract records it once copied back
    return ORBX_OK;
}

// The launch of stereo over pairs (image i of L at offset offL, image i of R at offset offR),
// its scratch allocated: nothing in it allocates or waits, so it can be enqueued in a graph
// capture.  The images' extraction must be issued (not necessarily run) before the launch.
orbx_status stereo_launch_args(orbx_extractor* L, orbx_extractor* R, int batch, int offL,
                               int offR, float mbf, float mb, float* d_uR, float* d_dep,
                               int* d_nv, hipStream_t st, StereoLaunch& a) {
    if (L->hg.width != R->hg.width || L->hg.height != R->hg.height ||
        L->hg.nlevels != R->hg.nlevels || L->hg.kp_cap != R->hg.kp_cap)
        return ORBX_ERR_INVALID;
    const size_t KC = (size_t)L->hg.kp_cap;
    a.dg = L->d_geom.as<Geometry>();
    a.batch = batch;
    a.kpsL = L->d_kps.as<float>() + offL * KC * 7;
    a.descL = L->d_desc.as<uint8_t>() + offL * KC * 32;
    a.nkpL = L->d_nkp.as<int>() + offL;
    a.pyrL = L->d_pyr.as<uint8_t>() + offL * (size_t)L->hg.pyr_bytes;
    a.kpsR = R->d_kps.as<float>() + offR * KC * 7;
    a.descR = R->d_desc.as<uint8_t>() + offR * KC * 32;
    a.nkpR = R->d_nkp.as<int>() + offR;
    a.pyrR = R->d_pyr.as<uint8_t>() + offR * (size_t)R->hg.pyr_bytes;
    a.mbf = mbf;
    a.mb = mb;
    a.uR = d_uR;
    a.depth = d_dep;
    a.nvalid = d_nv;
    a.lds = L->stereo_lds;
    a.timer = &L->timer;
    a.scnt = nullptr;
    a.ssad = nullptr;
    a.sidx = nullptr;
    if (stereo_split(batch) > 1) {
        // split path scratch: counters (zeroed when allocated; the median cut leaves them zero),
        // then per pair kp_cap SADs and left indices
        // (a fixed counter block: one slot per pair of the largest split batch, so a later
        // call with another batch finds its counters zero)
        // (stereo_split(batch) > 1 only for batch <= 128, so 256 counters always suffice)
        // (then 256 done-counters of the fused cut, also zero on entry and left zero)
        const size_t cnt_bytes = 2 * 256 * 4;
        const size_t need = cnt_bytes + (size_t)batch * KC * 6;
        // a reallocation (detected by capacity: the allocator may hand back the same
        // address) starts from zeroed counters
        const size_t cap_before = L->d_sscr.n;
        if (need > cap_before && !wait_idle(L)) return ORBX_ERR_DEVICE;
        if (!L->d_sscr.ensure(need)) return ORBX_ERR_DEVICE;
        if (L->d_sscr.n != cap_before &&
            !HIPOK(hipMemsetAsync(L->d_sscr.p, 0, cnt_bytes, st)))
            return ORBX_ERR_DEVICE;
        uint8_t* base = L->d_sscr.as<uint8_t>();
        a.scnt = (int*)base;
        a.ssad = (int*)(base + cnt_bytes);
        a.sidx = (int16_t*)(base + cnt_bytes + (size_t)batch * KC * 4);
    }
    return ORBX_OK;
}

// Stereo over pairs of the handles' last extractions.
static orbx_status run_stereo(orbx_extractor* L, orbx_extractor* R, int batch, int offL, int offR,
                              float mbf, float mb, float* d_uR, float* d_dep, int* d_nv,
                              hipStream_t st) {
    if (!L->last_valid || !R->last_valid) return ORBX_ERR_STATE;
    if (offL + batch > L->last_batch || offR + batch > R->last_batch) return ORBX_ERR_INVALID;
    StereoLaunch a;
    const orbx_status s = stereo_launch_args(L, R, batch, offL, offR, mbf, mb, d_uR, d_dep, d_nv,
                                             st, a);
    if (s != ORBX_OK) return s;
    if (!order_after_last(L, st) || (R != L && !order_after_last(R, st))) return ORBX_ERR_DEVICE;
    if (!HIPOK(launch_stereo(a, st)) || !mark_done(L, st) || (R != L && !mark_done(R, st)))
        return ORBX_ERR_DEVICE;
    return ORBX_OK;
}

// The graph of a host-image sequence for the handle's current state, captured on st when the
// slot's is missing or stale.
static bool graph_current(orbx_extractor* h, const ExtractLaunch& a, hipStream_t st, int width,
                          int height, const std::function<bool(const ExtractLaunch&)>& enqueue,
                          GraphSlot& slot, const std::vector<uint64_t>& extra) {
    const DevBuf* bufs[] = {&h->d_geom, &h->d_cells, &h->d_rtab, &h->d_ltab, &h->d_pyr,
                            &h->d_blur, &h->d_ccnt, &h->d_cand, &h->d_ocnt, &h->d_okp,
                            &h->d_kscr, &h->d_outs};
    std::vector<uint64_t> key = {(uint64_t)width, (uint64_t)height, (uint64_t)a.side_mode,
                                 (uint64_t)a.side_at, (uint64_t)a.side_lv, key_word(h->h_in),
                                 key_word(h->h_out),
                                 // the output block's layout (a regrown buffer may come back at
                                 // the same address)
                                 (uint64_t)h->cap_batch, (uint64_t)h->hg.kp_cap};
    for (const DevBuf* b : bufs) key.push_back(key_word(b->p));
    key.insert(key.end(), extra.begin(), extra.end());
    if (slot.exec && key == slot.key) return true;
    slot.destroy();
    hipGraph_t g = nullptr;
    bool ok = false, ended = false;
    {
        std::unique_lock<std::shared_mutex> lk(g_capture_mu);   // see order_after_last
        if (!HIPOK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal))) return false;
        ok = enqueue(a);
        ended = HIPOK(hipStreamEndCapture(st, &g));
    }
    hipGraphExec_t ex = nullptr;
    const bool inst = ok && ended && g && HIPOK(hipGraphInstantiate(&ex, g, nullptr, nullptr, 0));
    if (g) (void)hipGraphDestroy(g);
    if (!inst) return false;
    slot.exec = ex;
    slot.key = std::move(key);
    return true;
}

// One launch instead of ~15 enqueues: sessions on one GPU contend for the runtime's per-call work.
bool run_graphed(orbx_extractor* h, const ExtractLaunch& a, hipStream_t st, int width, int height,
                 const std::function<bool(const ExtractLaunch&)>& enqueue, GraphSlot& slot,
                 std::vector<uint64_t> extra, hipEvent_t wait_ev) {
    const bool graph = !h->timer.on && graph_current(h, a, st, width, height, enqueue, slot, extra);
    return (!wait_ev || HIPOK(hipStreamWaitEvent(st, wait_ev, 0))) &&
           (graph ? HIPOK(hipGraphLaunch(slot.exec, st)) : enqueue(a)) && mark_done(h, st) &&
           wait_done(h);
}

}  // namespace orbx

extern "C" {

const char* orbx_version(void) { return ORBX_VERSION; }

const char* orbx_last_error(void) { return g_err; }

const char* orbx_kernel_name(int id) {
    static const char* names[K_COUNT] = {"k_level", "k_fast", "k_octree", "k_orient_desc",
                                         "k_stereo", "k_level0"};
    return (id >= 0 && id < K_COUNT) ? names[id] : "";
}

orbx_status orbx_extractor_set_overlap(orbx_extractor* h, int mode, int fork_level, int levels) {
    if (!h || mode > 4 || (mode > 0 && (fork_level < 0 || levels < 1))) return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (mode < 0) {
        h->side_mode = FAST_SIDE;
        h->side_at = FAST_SIDE_AT;
        h->side_lv = FAST_SIDE_LV;
        h->side_auto = true;
    } else {
        h->side_mode = mode;
        h->side_at = fork_level;
        h->side_lv = levels;
        h->side_auto = false;
    }
    return ORBX_OK;
}

orbx_status orbx_extractor_get_overlap(const orbx_extractor* h, int* mode, int* fork_level,
                                       int* levels) {
    if (!h) return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (mode) *mode = h->side_mode;
    if (fork_level) *fork_level = h->side_at;
    if (levels) *levels = h->side_lv;
    return ORBX_OK;
}

orbx_status orbx_profile_enable(orbx_extractor* h, int on) {
    if (!h) return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    h->timer.on = on != 0;
    return ORBX_OK;
}

orbx_status orbx_profile_collect(orbx_extractor* h, double* total_ms, int64_t* launches) {
    if (!h) return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    h->timer.collect();
    for (int k = 0; k < K_COUNT; ++k) {
        if (total_ms) total_ms[k] = h->timer.ms[k];
        if (launches) launches[k] = h->timer.n[k];
        h->timer.ms[k] = 0;
        h->timer.n[k] = 0;
    }
    return ORBX_OK;
}

orbx_status orbx_extractor_launch_info(const orbx_extractor* h, int batch, int* strip_rows,
                                       int* stereo_split) {
    if (!h || batch < 1) return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->have_geom) return ORBX_ERR_STATE;
    int sth[ORBX_MAX_LEVELS];
    strip_heights(h, batch, sth);
    if (strip_rows)
        for (int l = 0; l < h->hg.nlevels; ++l) strip_rows[l] = h->hg.lv[l].strip ? sth[l] : 0;
    if (stereo_split) *stereo_split = orbx::stereo_split(std::max(batch / 2, 1));
    return ORBX_OK;
}

orbx_status orbx_extractor_regime_info(const orbx_extractor* h, int batch, int in_place,
                                       orbx_regime_info* out) {
    if (!h || !out || batch < 1) return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->have_geom) return ORBX_ERR_STATE;
    const Geometry& G = h->hg;
    static_assert(sizeof(out->cand_cap) / sizeof(out->cand_cap[0]) == ORBX_MAX_LEVELS, "levels");
    memset(out, 0, sizeof(*out));
    const int small = octree_small(batch);
    out->octree_threads = octree_threads(batch, G.nlevels);
    out->packed = small ? 0 : 1;
    out->ncap = h->ncap;
    out->kcap = small ? h->kcap_small : h->kcap;
    out->spatial = orient_spatial(batch) ? 1 : 0;
    out->fast_cells_per_wave = fast_cells_per_wave(G.n_cells, batch, h->ncu);
    out->chain = chain_of(h, in_place ? 1 : 0, side_mode_of(h, batch), batch);
    out->nlevels = G.nlevels;
    for (int l = 0; l < G.nlevels; ++l) {
        out->cand_cap[l] = G.lv[l].cand_cap;
        out->nfeat[l] = G.lv[l].nfeat;
    }
    return ORBX_OK;
}

orbx_status orbx_device_count(int* n) {
    if (!n) return ORBX_ERR_INVALID;
    int c = 0;
    if (!HIPOK(hipGetDeviceCount(&c))) { *n = 0; return ORBX_ERR_DEVICE; }
    *n = c;
    return ORBX_OK;
}

int orbx_descriptor_distance(const uint8_t* a, const uint8_t* b) {
    int d = 0;
    for (int i = 0; i < 32; ++i) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
    return d;
}

orbx_status orbx_extractor_create(const orbx_extractor_params* p, orbx_extractor** out) {
    if (!p || !out) return ORBX_ERR_INVALID;
    *out = nullptr;
    if (p->nlevels < 1 || p->nlevels > ORBX_MAX_LEVELS || p->nfeatures < 0 ||
        !(p->scale_factor > 0.f) || p->max_batch < 0)
        return ORBX_ERR_INVALID;
    int ndev = 0;
    if (!HIPOK(hipGetDeviceCount(&ndev)) || ndev <= 0) return ORBX_ERR_DEVICE;
    if (p->device < 0 || p->device >= ndev) return ORBX_ERR_INVALID;
    orbx_extractor* h = new orbx_extractor();
    h->prm = *p;
    if (h->prm.max_batch < 1) h->prm.max_batch = 1;
    h->device = p->device;
    compute_tables(h->prm, *h);
    hipDeviceProp_t prop;
    if (!HIPOK(hipSetDevice(h->device)) || !HIPOK(hipGetDeviceProperties(&prop, h->device)) ||
        !HIPOK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) ||
        !HIPOK(hipEventCreateWithFlags(&h->done, hipEventDisableTiming)) ||
        !HIPOK(hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking)) ||
        !HIPOK(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming)) ||
        !HIPOK(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming))) {
        (void)orbx_extractor_destroy(h);   // whatever was created
        return ORBX_ERR_DEVICE;
    }
    h->ncu = std::max(prop.multiProcessorCount, 1);
    *out = h;
    return ORBX_OK;
}

orbx_status orbx_extractor_destroy(orbx_extractor* h) {
    if (!h) return ORBX_ERR_INVALID;
    frame_server_unuse(h);
    (void)hipSetDevice(h->device);
    (void)wait_idle(h);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->h_in) (void)hipHostFree(h->h_in);
    if (h->h_out) (void)hipHostFree(h->h_out);
    if (h->h_pyr) (void)hipHostFree(h->h_pyr);
    DevBuf* bufs[] = {&h->d_geom, &h->d_cells, &h->d_rtab, &h->d_ltab, &h->d_pyr, &h->d_blur,
                      &h->d_ccnt, &h->d_cand, &h->d_ocnt, &h->d_okp, &h->d_kscr, &h->d_kps,
                      &h->d_desc, &h->d_nkp, &h->d_uR, &h->d_sscr, &h->d_outs};
    for (DevBuf* b : bufs) b->release();
    h->timer.destroy();
    h->g_extract.destroy();
    h->g_frame.destroy();
    if (h->side) (void)hipStreamSynchronize(h->side);
    if (h->done) (void)hipEventDestroy(h->done);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    if (h->side) (void)hipStreamDestroy(h->side);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    return ORBX_OK;
}

orbx_status orbx_extractor_tables(const orbx_extractor* h, float* scale, float* inv_scale,
                                  float* sigma2, float* inv_sigma2, int* features_per_level) {
    if (!h) return ORBX_ERR_INVALID;
    for (int i = 0; i < h->prm.nlevels; ++i) {
        if (scale) scale[i] = h->scale[i];
        if (inv_scale) inv_scale[i] = h->inv_scale[i];
        if (sigma2) sigma2[i] = h->sigma2[i];
        if (inv_sigma2) inv_sigma2[i] = h->inv_sigma2[i];
        if (features_per_level) features_per_level[i] = h->nfeat[i];
    }
    return ORBX_OK;
}

// orbx_extract's device sequence for one host image, up to the outputs in the handle's pinned
// block (nkp at 0, keypoints at h->out.o_kps, descriptors at h->out.o_desc) and the count in
// *n_out.  Called with h->mu held.
static orbx_status extract_host(orbx_extractor* h, const uint8_t* img, int width, int height,
                                size_t stride, int* n_out) {
    orbx_status s = ensure_workspace(h, width, height, 1);
    if (s != ORBX_OK) return s;
    hipStream_t st = h->stream;
    // The image goes through the handle's pinned staging, laid out with the pyramid's row
    // pitch, and one linear DMA writes it straight into pyramid level 0 (mvImagePyramid[0]):
    // the extraction then only blurs it (no device-side copy of the input; a pitched 2-D
    // host copy would run row by row).  Every output comes back in one pinned block: one
    // host wait per call.
    const LevelGeom& L0 = h->hg.lv[0];
    const size_t pitch0 = (size_t)L0.pitch, img_bytes = pitch0 * (size_t)height;
    const size_t o_end = h->out.desc_end(1);   // image 0's outputs in the device block
    h->host_pyr_ok = false;
    if (!ensure_pinned(h->h_in, h->h_in_n, img_bytes) ||
        !ensure_pinned(h->h_out, h->h_out_n, o_end) ||
        (h->host_pyr && !ensure_pinned(h->h_pyr, h->h_pyr_n, (size_t)h->hg.pyr_bytes)))
        return ORBX_ERR_DEVICE;
    for (int y = 0; y < height; ++y)
        std::memcpy(h->h_in + (size_t)y * pitch0, img + (size_t)y * stride, (size_t)width);
    if (!order_after_last(h, st)) return ORBX_ERR_DEVICE;
    // the device sequence: one linear DMA into level 0, the kernels, one DMA of the outputs
    auto enqueue = [&](const ExtractLaunch& a) {
        return HIPOK(hipMemcpyAsync(h->d_pyr.as<uint8_t>() + L0.off, h->h_in, img_bytes,
                                    hipMemcpyHostToDevice, st)) &&
               HIPOK(launch_extract(a, st)) &&
               HIPOK(hipMemcpyAsync(h->h_out, h->d_outs.p, o_end, hipMemcpyDeviceToHost, st));
    };
    ExtractLaunch a = extract_launch(h, nullptr, nullptr, 1, 1, 0, 0);
    if (h->host_pyr) {
        a.pyr_host = h->h_pyr;
        a.pyr_host_bytes = (size_t)h->hg.pyr_bytes;
    }
    if (!run_graphed(h, a, st, width, height, enqueue, h->g_extract, {key_word(a.pyr_host)}))
        return ORBX_ERR_DEVICE;
    std::memcpy(n_out, h->h_out, 4);
    set_last(h, 1, true, 1, *n_out);
    h->host_pyr_ok = h->host_pyr;
    return ORBX_OK;
}

orbx_status orbx_extract(orbx_extractor* h, const uint8_t* img, int width, int height,
                         size_t stride, orbx_keypoint* kps, int kp_cap, uint8_t* desc,
                         int* n_out) {
    if (!h || !n_out) return ORBX_ERR_INVALID;
    if (width <= 0 || height <= 0 || !img) {   // cv::Mat::empty(): silent return
        *n_out = -1;
        return ORBX_OK;
    }
    if (stride < (size_t)width) return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    const orbx_status s = extract_host(h, img, width, height, stride, n_out);
    if (s != ORBX_OK) return s;
    const int n = *n_out, m = std::min(n, kp_cap);
    if (m > 0) {
        if (kps) std::memcpy(kps, h->h_out + h->out.o_kps, (size_t)m * sizeof(orbx_keypoint));
        if (desc) std::memcpy(desc, h->h_out + h->out.o_desc, (size_t)m * 32);
    }
    return n > kp_cap ? ORBX_ERR_CAPACITY : ORBX_OK;
}

orbx_status orbx_extract_view(orbx_extractor* h, const uint8_t* img, int width, int height,
                              size_t stride, const orbx_keypoint** kps, const uint8_t** desc,
                              int* n_out) {
    if (!h || !n_out || !kps || !desc) return ORBX_ERR_INVALID;
    *kps = nullptr;
    *desc = nullptr;
    if (width <= 0 || height <= 0 || !img) {   // cv::Mat::empty(): silent return
        *n_out = -1;
        return ORBX_OK;
    }
    if (stride < (size_t)width) return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    const orbx_status s = extract_host(h, img, width, height, stride, n_out);
    if (s != ORBX_OK) return s;
    *kps = (const orbx_keypoint*)(h->h_out + h->out.o_kps);
    *desc = h->h_out + h->out.o_desc;
    return ORBX_OK;
}

uint64_t orbx_extractor_serial(const orbx_extractor* h) {
    if (!h) return 0;
    std::lock_guard<std::mutex> lk(h->mu);
    return h->serial;
}

orbx_status orbx_extractor_host_pyramid(orbx_extractor* h, int on) {
    if (!h) return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    h->host_pyr = on != 0;
    if (!h->host_pyr) h->host_pyr_ok = false;
    return ORBX_OK;
}

orbx_status orbx_host_pyramid_view(const orbx_extractor* h, orbx_host_pyramid* out) {
    if (!h || !out) return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->host_pyr_ok || !h->have_geom || !h->h_pyr) return ORBX_ERR_STATE;
    std::memset(out, 0, sizeof(*out));
    out->nlevels = h->hg.nlevels;
    for (int l = 0; l < h->hg.nlevels && l < 16; ++l) {
        const LevelGeom& L = h->hg.lv[l];
        out->data[l] = h->h_pyr + L.off;
        out->width[l] = L.w;
        out->height[l] = L.h;
        out->step[l] = (size_t)L.pitch;
    }
    return ORBX_OK;
}

orbx_status orbx_extractor_keep_pyramid(orbx_extractor* h, int on) {
    if (!h) return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    h->keep_pyr = on != 0;
    return ORBX_OK;
}

static orbx_status copy_level(orbx_extractor* h, const DevBuf& buf, int index, int level,
                              uint8_t* out, int* width, int* height, bool blurred = false) {
    std::lock_guard<std::mutex> lk(h->mu);
    if (level < 0 || level >= h->hg.nlevels || index < 0) return ORBX_ERR_INVALID;
    // the raw pyramid of images [0, pyr_images); the blurred one of a full last call only
    if (index >= h->pyr_images || (blurred && (!h->last_valid || index >= h->last_batch)))
        return ORBX_ERR_STATE;
    const LevelGeom& lv = h->hg.lv[level];
    if (width) *width = lv.w;
    if (height) *height = lv.h;
    if (!out) return ORBX_OK;
    (void)hipSetDevice(h->device);
    const uint8_t* src = buf.as<uint8_t>() + (size_t)index * h->hg.pyr_bytes + lv.off;
    if (blurred) {
        // 16x4 tiles (blur_off): the level's whole bands to the host, then de-tiled
        const size_t bytes = (size_t)lv.pitch * align_up((size_t)lv.h, 4);
        std::vector<uint8_t> tiles(bytes);
        if (!order_after_last(h, h->stream) ||
            !HIPOK(hipMemcpyAsync(tiles.data(), src, bytes, hipMemcpyDeviceToHost, h->stream)) ||
            !HIPOK(hipStreamSynchronize(h->stream)))
            return ORBX_ERR_DEVICE;
        for (int y = 0; y < lv.h; ++y)
            for (int x = 0; x < lv.w; x += 16)
                std::memcpy(out + (size_t)y * lv.w + x, tiles.data() + blur_off(x, y, lv.pitch, lv.h),
                            (size_t)std::min(16, lv.w - x));
        return ORBX_OK;
    }
    if (!order_after_last(h, h->stream) ||
        !HIPOK(hipMemcpy2DAsync(out, lv.w, src, lv.pitch, lv.w, lv.h, hipMemcpyDeviceToHost, h->stream)) ||
        !HIPOK(hipStreamSynchronize(h->stream)))
        return ORBX_ERR_DEVICE;
    return ORBX_OK;
}

orbx_status orbx_pyramid_level(orbx_extractor* h, int index, int level, uint8_t* out, int* width,
                               int* height) {
    return h ? copy_level(h, h->d_pyr, index, level, out, width, height) : ORBX_ERR_INVALID;
}

orbx_status orbx_blur_level(orbx_extractor* h, int index, int level, uint8_t* out, int* width,
                            int* height) {
    return h ? copy_level(h, h->d_blur, index, level, out, width, height, true) : ORBX_ERR_INVALID;
}

orbx_status orbx_extractor_prepare(orbx_extractor* h, int width, int height, int batch,
                                   int* kp_cap) {
    if (!h || width <= 0 || height <= 0 || batch < 1) return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    orbx_status s = ensure_workspace(h, width, height, batch);
    if (s == ORBX_OK && kp_cap) *kp_cap = h->hg.kp_cap;
    return s;
}

orbx_status orbx_extract_batch_device(orbx_extractor* h, const uint8_t* d_imgs, int batch,
                                      int width, int height, size_t stride, size_t batch_stride,
                                      void* stream) {
    if (!h || !d_imgs || batch < 1 || width <= 0 || height <= 0 || stride < (size_t)width)
        return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    orbx_status s = ensure_workspace(h, width, height, batch);
    if (s != ORBX_OK) return s;
    return run_extract(h, d_imgs, nullptr, batch, batch, stride, batch_stride, (hipStream_t)stream);
}

orbx_status orbx_batch_input_view(orbx_extractor* h, int width, int height, int batch,
                                  uint8_t** d_level0, size_t* pitch, size_t* image_stride) {
    if (!h || width <= 0 || height <= 0 || batch < 1 || !d_level0) return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    orbx_status s = ensure_workspace(h, width, height, batch);
    if (s != ORBX_OK) return s;
    *d_level0 = h->d_pyr.as<uint8_t>() + h->hg.lv[0].off;
    if (pitch) *pitch = (size_t)h->hg.lv[0].pitch;
    if (image_stride) *image_stride = (size_t)h->hg.pyr_bytes;
    return ORBX_OK;
}

orbx_status orbx_extract_batch_resident(orbx_extractor* h, int batch, void* stream) {
    if (!h || batch < 1) return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->have_geom) return ORBX_ERR_STATE;
    if (batch > h->cap_batch) return ORBX_ERR_INVALID;
    if (!HIPOK(hipSetDevice(h->device))) return ORBX_ERR_DEVICE;
    return run_extract(h, nullptr, nullptr, batch, batch, 0, 0, (hipStream_t)stream);
}

orbx_status orbx_stereo_frames_resident(orbx_extractor* h, int batch, float mbf, float mb,
                                        float* d_uRight, float* d_depth, int32_t* d_nvalid,
                                        void* stream) {
    if (!h || batch < 1 || !d_uRight || !d_depth) return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->have_geom) return ORBX_ERR_STATE;
    if (2 * batch > h->cap_batch) return ORBX_ERR_INVALID;
    if (!HIPOK(hipSetDevice(h->device))) return ORBX_ERR_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    orbx_status s = run_extract(h, nullptr, nullptr, 2 * batch, 2 * batch, 0, 0, st);
    if (s != ORBX_OK) return s;
    return run_stereo(h, h, batch, 0, batch, mbf, mb, d_uRight, d_depth, d_nvalid, st);
}

orbx_status orbx_batch_view_get(const orbx_extractor* h, orbx_batch_view* v) {
    if (!h || !v) return ORBX_ERR_STATE;
    // a snapshot under the handle's lock: an extraction running on another thread cannot
    // change the batch size or reallocate the buffers halfway through the copy
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->last_valid) return ORBX_ERR_STATE;
    memset(v, 0, sizeof(*v));
    v->batch = h->last_batch;
    v->kp_cap = h->hg.kp_cap;
    v->kps = h->d_kps.as<orbx_keypoint>();
    v->desc = h->d_desc.as<uint8_t>();
    v->nkp = h->d_nkp.as<int32_t>();
    v->pyramid = h->d_pyr.as<uint8_t>();
    v->pyr_bytes = (size_t)h->hg.pyr_bytes;
    for (int l = 0; l < h->hg.nlevels && l < 16; ++l) {
        v->level_w[l] = h->hg.lv[l].w;
        v->level_h[l] = h->hg.lv[l].h;
        v->level_pitch[l] = h->hg.lv[l].pitch;
        v->level_off[l] = (size_t)h->hg.lv[l].off;
    }
    return ORBX_OK;
}

orbx_status orbx_batch_fetch(orbx_extractor* h, int first, int count, int32_t* nkp,
                             orbx_keypoint* kps, uint8_t* desc) {
    if (!h || first < 0 || count < 0) return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->last_valid || first + count > h->last_batch) return ORBX_ERR_INVALID;
    (void)hipSetDevice(h->device);
    // after the handle's last launches (on whatever stream), on the handle's own stream
    hipStream_t st = h->stream;
    if (!order_after_last(h, st)) return ORBX_ERR_DEVICE;
    const size_t KC = (size_t)h->hg.kp_cap;
    if (nkp && !HIPOK(hipMemcpyAsync(nkp, h->d_nkp.as<int32_t>() + first, (size_t)count * 4,
                                     hipMemcpyDeviceToHost, st)))
        return ORBX_ERR_DEVICE;
    if (kps && !HIPOK(hipMemcpyAsync(kps, h->d_kps.as<orbx_keypoint>() + first * KC,
                                     (size_t)count * KC * sizeof(orbx_keypoint),
                                     hipMemcpyDeviceToHost, st)))
        return ORBX_ERR_DEVICE;
    if (desc && !HIPOK(hipMemcpyAsync(desc, h->d_desc.as<uint8_t>() + first * KC * 32,
                                      (size_t)count * KC * 32, hipMemcpyDeviceToHost, st)))
        return ORBX_ERR_DEVICE;
    return HIPOK(hipStreamSynchronize(st)) ? ORBX_OK : ORBX_ERR_DEVICE;
}

orbx_status orbx_stereo_match(orbx_extractor* left, orbx_extractor* right, float mbf, float mb,
                              float* uRight, float* depth, int n_left, int* n_valid) {
    if (!left || !right || left == right) return ORBX_ERR_INVALID;
    // both handles: the right pyramid is read, so neither may be re-extracted meanwhile
    std::scoped_lock lk(left->mu, right->mu);
    if (!left->last_valid || !right->last_valid || left->last_batch != 1 || right->last_batch != 1)
        return ORBX_ERR_STATE;
    (void)hipSetDevice(left->device);
    // the results in one device block, copied back by one DMA into one pinned block:
    // [nvalid | uRight[KC] | depth[KC]]; the left keypoint count is the handle's own (its
    // orbx_extract returned it)
    const StereoLayout sl(1, (size_t)left->hg.kp_cap);
    if (!left->d_uR.ensure(sl.end)) return ORBX_ERR_DEVICE;
    if (!ensure_pinned(left->h_out, left->h_out_n, sl.end)) return ORBX_ERR_DEVICE;
    uint8_t* dso = left->d_uR.as<uint8_t>();
    hipStream_t st = left->stream;
    orbx_status s = run_stereo(left, right, 1, 0, 0, mbf, mb, (float*)(dso + sl.o_u),
                               (float*)(dso + sl.o_d), (int*)dso, st);
    if (s != ORBX_OK) return s;
    uint8_t* ho = left->h_out;
    const bool known = left->last_n >= 0;   // else a batched call of one image set the state
    if (!HIPOK(hipMemcpyAsync(ho, dso, sl.end, hipMemcpyDeviceToHost, st)) ||
        (!known && !HIPOK(hipMemcpyAsync(ho + 8, left->d_nkp.p, 4, hipMemcpyDeviceToHost, st))) ||
        !mark_done(left, st) || !wait_done(left))
        return ORBX_ERR_DEVICE;
    int n = left->last_n;
    if (!known) std::memcpy(&n, ho + 8, 4);
    int nv = 0;
    std::memcpy(&nv, ho, 4);
    const int m = std::min(n, n_left);
    if (m > 0) {
        if (uRight) std::memcpy(uRight, ho + sl.o_u, (size_t)m * 4);
        if (depth) std::memcpy(depth, ho + sl.o_d, (size_t)m * 4);
    }
    if (n_valid) *n_valid = nv;
    return n > n_left ? ORBX_ERR_CAPACITY : ORBX_OK;
}

orbx_status orbx_stereo_match_batch_device(orbx_extractor* left, orbx_extractor* right, float mbf,
                                           float mb, float* d_uRight, float* d_depth,
                                           int32_t* d_nvalid, void* stream) {
    if (!left || !right || left == right || !d_uRight || !d_depth) return ORBX_ERR_INVALID;
    std::scoped_lock lk(left->mu, right->mu);
    (void)hipSetDevice(left->device);
    if (left->last_batch != right->last_batch) return ORBX_ERR_INVALID;
    return run_stereo(left, right, left->last_batch, 0, 0, mbf, mb, d_uRight, d_depth, d_nvalid,
                      (hipStream_t)stream);
}

orbx_status orbx_stereo_frames_device(orbx_extractor* h, const uint8_t* d_left,
                                      const uint8_t* d_right, int batch, int width, int height,
                                      size_t stride, size_t batch_stride, float mbf, float mb,
                                      float* d_uRight, float* d_depth, int32_t* d_nvalid,
                                      void* stream) {
    if (!h || !d_left || !d_right || batch < 1 || width <= 0 || height <= 0 ||
        stride < (size_t)width || !d_uRight || !d_depth)
        return ORBX_ERR_INVALID;
    std::lock_guard<std::mutex> lk(h->mu);
    orbx_status s = ensure_workspace(h, width, height, 2 * batch);
    if (s != ORBX_OK) return s;
    hipStream_t st = (hipStream_t)stream;
    s = run_extract(h, d_left, d_right, batch, 2 * batch, stride, batch_stride, st);
    if (s != ORBX_OK) return s;
    return run_stereo(h, h, batch, 0, batch, mbf, mb, d_uRight, d_depth, d_nvalid, st);
}

}  // extern "C"
