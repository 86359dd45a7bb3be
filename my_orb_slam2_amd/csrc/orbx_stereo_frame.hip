// orbx_stereo_frame.hip — orbx_stereo_frame_view: a stereo frame's extraction and matching in one
// call, on the caller's own handle or as part of a batch on the frame server's.
#include <algorithm>
#include <condition_variable>
#include <map>
#include <thread>

#include "orbx_extractor.h"

using namespace orbx;

// A helper thread that stages the right image of a stereo frame while the calling thread
// stages the left one (orbx_stereo_frame_view): the copy of a cold 0.47 MB image into pinned
// memory is tens of microseconds on one core.
struct OrbxStager {
    std::mutex mu;
    std::condition_variable cv;
    std::function<void()> job;
    bool has_job = false, done = true, stop = false;
    std::thread th;
    OrbxStager() : th([this] { run(); }) {}
    ~OrbxStager() {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
        }
        cv.notify_all();
        th.join();
    }
    void run() {
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            cv.wait(lk, [&] { return has_job || stop; });
            if (stop) return;
            std::function<void()> j = std::move(job);
            has_job = false;
            lk.unlock();
            j();
            lk.lock();
            done = true;
            cv.notify_all();
        }
    }
    void post(std::function<void()> j) {
        std::lock_guard<std::mutex> lk(mu);
        job = std::move(j);
        has_job = true;
        done = false;
        cv.notify_all();
    }
    void wait() {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return done; });
    }
};

// ---- several sessions' stereo frames as one batch (orbx_stereo_frame_view) -----------------
// Tracking sessions on one device each call orbx_stereo_frame_view on their own handle.  A
// call that finds the device's frame server idle (nothing running, nothing queued) runs on its
// own handle (one graph replay, stereo_frame_solo).  A call that arrives while another runs
// joins the batch being formed: it stages its two images into its slot of the server's pinned
// input block and issues that slot's DMA to the server's device staging on the server's copy
// stream right away (the copy overlaps the running batch).  When the device frees, a waiting
// thread takes the formed batch (up to FS_MAX_FRAMES frames of one image size and camera) and
// replays the server's graph for its size on the server's own handle: the lefts as images
// [0, m), the rights as [m, 2m), one extraction of the 2m images, one stereo launch over the
// m pairs, the outputs back into the pair's pinned output block.  Each waiting thread then
// copies its frame's outputs into its own handle's pinned block.  Two block pairs alternate,
// each with its own server handle: a batch forms in one while the other's runs, and up to
// FS_INFLIGHT batches run at once.  With several sessions the runtime's submission path,
// not the GPU, bounded the rate of one-call frames (14 submissions each).
//
// Batches on the device at once (each on its block pair's own server handle): a batch of a
// few frames is a latency-bound chain that leaves most of the GPU idle, so the next one runs
// beside it.
#define FS_INFLIGHT 2
#define FS_MAX_FRAMES 8
struct FsReq {
    orbx_extractor* h;            // the caller's handle (its stager)
    int slot = -1, blk = -1;      // its frame in the batch, the block pair of that batch
    orbx_status st = ORBX_OK;
    bool taken = false;           // its batch has a lead (only an untaken frame may lead)
    bool done = false;
};
// One server output block: the outputs of the batch's 2m images, laid out as the server handle's
// workspace lays them out, then at out.after(2m) the stereo block of its m pairs.
struct FsLayout {
    OutLayout out;
    StereoLayout st;
    int m = 0;
};
struct FsBatch {                   // the size and camera of a batch's frames
    int width = 0, height = 0;
    float mbf = 0.f, mb = 0.f;
    size_t pitch0 = 0, img_bytes = 0;
};
struct FrameServer {
    std::mutex mu;
    std::condition_variable cv;
    int inflight = 0;              // batches (and lone calls) on the device
    bool pair_busy[2] = {false, false};   // a batch of block pair i is on the device
    orbx_extractor* sh[2] = {nullptr, nullptr};   // the server's handle per block pair
    // the batch being formed: n frames joined, `staged` of them copied into input block blk
    int blk = 0, n = 0, staged = 0;
    FsBatch geo;
    FsReq* req[FS_MAX_FRAMES] = {};
    // block pair i: the input block (frame j's left at 2j, its right at 2j+1, img_bytes each)
    // and the output block of a batch; the next batch forms in the other pair
    uint8_t* hin[2] = {nullptr, nullptr};
    size_t hin_n[2] = {0, 0};
    // each frame's images go on to the device as soon as they are staged, on the copy stream
    // (while the batch before runs), into the device staging block of its pair
    DevBuf dstage[2];
    hipStream_t cst = nullptr;
    hipEvent_t cev[2] = {nullptr, nullptr};   // recorded on cst when a pair's batch is taken
    uint8_t* hout[2] = {nullptr, nullptr};
    size_t hout_n[2] = {0, 0};
    int readers[2] = {0, 0};       // threads still copying out of each output block
    FsLayout lay[2];
    GraphSlot graphs[2][FS_MAX_FRAMES + 1];   // per block pair and batch size
    int users = 0;                 // live handles that called orbx_stereo_frame_view
    orbx_frame_server_stats stats{};   // always counted (orbx_frame_server_get_stats)
    // Frees every device / pinned resource (server handles, graphs, staging, streams); the
    // object itself (mutex, condition variable) stays, so references held by callers stay
    // valid.  Only when idle: nothing forming, running or being copied out.
    bool idle() const { return n == 0 && inflight == 0 && readers[0] == 0 && readers[1] == 0; }
    void release_resources() {
        // first drain every copy that may still read or write the pinned / staging blocks: a
        // batch whose event record failed returns without run_served, and its staging copies
        // on cst can still be pending; the server handles' graphs DMA into hout
        if (cst) (void)hipStreamSynchronize(cst);
        for (int b = 0; b < 2; ++b)
            if (sh[b]) {
                (void)wait_idle(sh[b]);
                if (sh[b]->stream) (void)hipStreamSynchronize(sh[b]->stream);
                if (sh[b]->side) (void)hipStreamSynchronize(sh[b]->side);
            }
        for (int b = 0; b < 2; ++b) {
            for (GraphSlot& G : graphs[b]) G.destroy();
            if (sh[b]) (void)orbx_extractor_destroy(sh[b]);
            sh[b] = nullptr;
            if (hin[b]) (void)hipHostFree(hin[b]);
            if (hout[b]) (void)hipHostFree(hout[b]);
            hin[b] = hout[b] = nullptr;
            hin_n[b] = hout_n[b] = 0;
            dstage[b].release();
            if (cev[b]) (void)hipEventDestroy(cev[b]);
            cev[b] = nullptr;
            pair_busy[b] = false;
            lay[b] = FsLayout{};
        }
        if (cst) {
            (void)hipStreamSynchronize(cst);
            (void)hipStreamDestroy(cst);
        }
        cst = nullptr;
        blk = n = staged = 0;
        stats.resident = 0;
    }
};

// One server per (device, extractor parameters).  The registry owns them for the life of the
// process; their resources are freed when the last handle that used one is destroyed
// (frame_server_unuse) or on orbx_frame_server_release.
static FrameServer& frame_server(const orbx_extractor* h) {
    static std::mutex mu;
    static std::map<std::vector<int>, std::unique_ptr<FrameServer>> servers;
    const orbx_extractor_params& p = h->prm;
    const std::vector<int> key = {h->device, p.nfeatures, (int)key_word(p.scale_factor), p.nlevels,
                                  p.ini_th_fast, p.min_th_fast, p.cv_simd};
    std::lock_guard<std::mutex> lk(mu);
    std::unique_ptr<FrameServer>& s = servers[key];
    if (!s) s.reset(new FrameServer());
    return *s;
}

// A handle that called orbx_stereo_frame_view counts as a user of its server until destroyed.
static void frame_server_use(orbx_extractor* h, FrameServer& fs) {
    std::lock_guard<std::mutex> hl(h->mu);
    if (h->fs_user) return;
    h->fs_user = true;
    std::lock_guard<std::mutex> lk(fs.mu);
    ++fs.users;
}
void orbx::frame_server_unuse(orbx_extractor* h) {
    if (!h->fs_user) return;
    FrameServer& fs = frame_server(h);
    std::lock_guard<std::mutex> lk(fs.mu);
    h->fs_user = false;
    if (--fs.users == 0 && fs.idle()) fs.release_resources();
}

// One batch of m frames (staged in input block `blk`) on the server's handle, replayed from
// the server's graph for (blk, m): two 2-D DMAs (the lefts, the rights), the extraction of
// the 2m images, the stereo match of the m pairs, two DMAs back into output block blk.
static orbx_status run_served(FrameServer& fs, const orbx_extractor* h0, int m, int blk,
                              const FsBatch& g) {
    if (!fs.sh[blk]) {
        orbx_extractor_params p = h0->prm;
        p.max_batch = 2 * FS_MAX_FRAMES;
        const orbx_status s = orbx_extractor_create(&p, &fs.sh[blk]);
        if (s != ORBX_OK) return s;
    }
    orbx_extractor* S = fs.sh[blk];
    std::lock_guard<std::mutex> lk(S->mu);
    // the workspace for the largest batch: one layout (and graph key) for every m
    orbx_status s = ensure_workspace(S, g.width, g.height, 2 * FS_MAX_FRAMES);
    if (s != ORBX_OK) return s;
    const LevelGeom& L0 = S->hg.lv[0];
    if ((size_t)L0.pitch != g.pitch0) return ORBX_ERR_INVALID;   // the staging layout
    const size_t pyrb = (size_t)S->hg.pyr_bytes;
    const OutLayout& ol = S->out;
    const StereoLayout sl((size_t)m, ol.KC);
    const size_t m2 = 2 * (size_t)m, o_desc = ol.o_desc, o_end = ol.desc_end(m2), o_st = ol.after(m2);
    // both blocks sized for the largest batch
    const size_t s_max = StereoLayout(FS_MAX_FRAMES, ol.KC).end;
    const size_t o_max = ol.after(2 * FS_MAX_FRAMES);
    if (!S->d_uR.ensure(s_max) || !ensure_pinned(fs.hout[blk], fs.hout_n[blk], o_max + s_max))
        return ORBX_ERR_DEVICE;
    hipStream_t st = S->stream;
    if (!order_after_last(S, st)) return ORBX_ERR_DEVICE;
    uint8_t* d_l0 = S->d_pyr.as<uint8_t>() + L0.off;
    uint8_t* dso = S->d_uR.as<uint8_t>();
    const uint8_t* dsg = fs.dstage[blk].as<uint8_t>();
    uint8_t* hout = fs.hout[blk];
    const size_t ib = g.img_bytes;
    const ExtractLaunch a = extract_launch(S, nullptr, nullptr, 2 * m, 2 * m, 0, 0);
    StereoLaunch sa;
    s = stereo_launch_args(S, S, m, 0, m, g.mbf, g.mb, (float*)(dso + sl.o_u),
                           (float*)(dso + sl.o_d), (int*)dso, st, sa);
    if (s != ORBX_OK) return s;
    // frame i's left into image slot i, its right into slot m + i (from the device staging);
    // back: the counts and keypoints of the 2m images, their descriptors, the stereo block
    const size_t kps_end = ol.kps_end(m2);
    auto enqueue = [&](const ExtractLaunch& ea) {
        return HIPOK(hipMemcpy2DAsync(d_l0, pyrb, dsg, 2 * ib, ib, (size_t)m,
                                      hipMemcpyDeviceToDevice, st)) &&
               HIPOK(hipMemcpy2DAsync(d_l0 + (size_t)m * pyrb, pyrb, dsg + ib, 2 * ib, ib,
                                      (size_t)m, hipMemcpyDeviceToDevice, st)) &&
               HIPOK(launch_extract(ea, st)) && HIPOK(launch_stereo(sa, st)) &&
               HIPOK(hipMemcpyAsync(hout, S->d_outs.p, kps_end, hipMemcpyDeviceToHost, st)) &&
               HIPOK(hipMemcpyAsync(hout + o_desc, S->d_outs.as<uint8_t>() + o_desc,
                                    o_end - o_desc, hipMemcpyDeviceToHost, st)) &&
               HIPOK(hipMemcpyAsync(hout + o_st, dso, sl.end, hipMemcpyDeviceToHost, st));
    };
    // the launch waits for cev[blk]: the frames' copies to the device
    if (!run_graphed(S, a, st, g.width, g.height, enqueue, fs.graphs[blk][m],
                     {key_word(dsg), key_word(hout), key_word(S->d_sscr.p), key_word(dso),
                      key_word(g.mbf), key_word(g.mb), (uint64_t)m, (uint64_t)ib},
                     fs.cev[blk]))
        return ORBX_ERR_DEVICE;
    set_last(S, 2 * m, true, 2 * m);
    fs.lay[blk] = FsLayout{ol, sl, m};
    return ORBX_OK;
}

// The waiting thread's own frame, from the server block into its handle's pinned block.
static orbx_status copy_served(FrameServer& fs, const FsReq& r, const FsBatch& g,
                               orbx_stereo_frame_out* out) {
    const FsLayout& ly = fs.lay[r.blk];
    const uint8_t* ho = fs.hout[r.blk];
    const size_t KC = ly.out.KC, KP = sizeof(orbx_keypoint);
    int32_t n[2];
    std::memcpy(&n[0], ho + 4 * (size_t)r.slot, 4);
    std::memcpy(&n[1], ho + 4 * (size_t)(ly.m + r.slot), 4);
    const size_t nl = (size_t)std::max(n[0], 0), nr = (size_t)std::max(n[1], 0);
    orbx_extractor* h = r.h;
    std::lock_guard<std::mutex> lk(h->mu);
    const size_t need = (nl + nr) * (KP + 32) + nl * 8 + 64;
    if (!ensure_pinned(h->h_out, h->h_out_n, need)) return ORBX_ERR_DEVICE;
    uint8_t* o = h->h_out;
    const size_t img[2] = {(size_t)r.slot, (size_t)(ly.m + r.slot)};
    const size_t cnt[2] = {nl, nr};
    for (int v = 0; v < 2; ++v) {
        std::memcpy(o, ho + ly.out.kps_end(img[v]), cnt[v] * KP);
        out->kps[v] = (const orbx_keypoint*)o;
        o += cnt[v] * KP;
    }
    for (int v = 0; v < 2; ++v) {
        std::memcpy(o, ho + ly.out.desc_end(img[v]), cnt[v] * 32);
        out->desc[v] = o;
        o += cnt[v] * 32;
    }
    const uint8_t* sb = ho + ly.out.after(2 * (size_t)ly.m);
    std::memcpy(&out->n_valid, sb + 4 * (size_t)r.slot, 4);
    std::memcpy(o, sb + ly.st.o_u + (size_t)r.slot * KC * 4, nl * 4);
    out->u_right = (const float*)o;
    o += nl * 4;
    std::memcpy(o, sb + ly.st.o_d + (size_t)r.slot * KC * 4, nl * 4);
    out->depth = (const float*)o;
    std::memcpy(out->n, n, 8);
    // this handle's own workspace does not hold the frame's keypoints ...
    set_last(h, 0, false, 0);
    if (!h->keep_pyr) return ORBX_OK;
    // ... but its pyramids when asked for (orbx_extractor_keep_pyramid): both views' blocks,
    // device to device from the server handle, whose workspace this block pair's next batch
    // does not touch while this thread holds its reader count
    // The frame's keypoints, descriptors and stereo outputs are complete at this point: a
    // failure below leaves the handle in the "no pyramid" state (orbx_pyramid_level returns
    // ORBX_ERR_STATE) and the frame still succeeds.  The handle's workspace is the two-image
    // one its own solo frames run in (the server serves only handles that run solo when it is
    // idle), so sizing it here allocates nothing those would not.
    const orbx_extractor* S = fs.sh[r.blk];
    if (ensure_workspace(h, g.width, g.height, 2) != ORBX_OK) return ORBX_OK;
    const size_t pyrb = (size_t)h->hg.pyr_bytes;
    if (!S || (size_t)S->hg.pyr_bytes != pyrb || S->hg.lv[0].pitch != h->hg.lv[0].pitch)
        return ORBX_OK;
    const uint8_t* src = S->d_pyr.as<uint8_t>();
    uint8_t* dst = h->d_pyr.as<uint8_t>();
    if (!HIPOK(hipSetDevice(h->device)) || !order_after_last(h, h->stream) ||
        !HIPOK(hipMemcpyAsync(dst, src + img[0] * pyrb, pyrb, hipMemcpyDeviceToDevice, h->stream)) ||
        !HIPOK(hipMemcpyAsync(dst + pyrb, src + img[1] * pyrb, pyrb, hipMemcpyDeviceToDevice,
                              h->stream)) ||
        !mark_done(h, h->stream) || !wait_done(h))
        return ORBX_OK;
    set_last(h, 2, false, 2);
    return ORBX_OK;
}

// Both images of a stereo frame into pinned staging at dst, rows at the pyramid's level-0
// pitch, the left at dst and the right at dst + img_bytes.  Called with h->mu held.  The helper
// thread stages the right image only for a frame that queues for the frame server.  Measured
// (r04_ab_runs.txt, r4i): its wake-up costs a lone caller with cache-hot images more (0.239 ->
// 0.257 ms) than it saves on cold ones (0.268 -> 0.259 ms); with 8 sessions it raised 9.4-9.6k
// to 9.6-9.9k pairs/s.
static void stage_frame(orbx_extractor* h, uint8_t* dst, size_t pitch0, size_t img_bytes,
                        const uint8_t* left, size_t stride_left, const uint8_t* right,
                        size_t stride_right, int width, int height, bool queued) {
    auto copy = [=](int v) {
        const uint8_t* img = v ? right : left;
        const size_t stride = v ? stride_right : stride_left;
        uint8_t* d = dst + (size_t)v * img_bytes;
        for (int y = 0; y < height; ++y)
            std::memcpy(d + (size_t)y * pitch0, img + (size_t)y * stride, (size_t)width);
    };
    if (queued) {
        if (!h->stager) h->stager.reset(new OrbxStager());
        h->stager->post([=] { copy(1); });
        copy(0);
        h->stager->wait();
    } else {
        copy(0);
        copy(1);
    }
}

// orbx_stereo_frame_view on the caller's own handle (one graph replay).
static orbx_status stereo_frame_solo(orbx_extractor* h, const uint8_t* left, size_t stride_left,
                                     const uint8_t* right, size_t stride_right, int width,
                                     int height, float mbf, float mb,
                                     orbx_stereo_frame_out* out) {
    std::lock_guard<std::mutex> lk(h->mu);
    orbx_status s = ensure_workspace(h, width, height, 2);
    if (s != ORBX_OK) return s;
    hipStream_t st = h->stream;
    const LevelGeom& L0 = h->hg.lv[0];
    const size_t pitch0 = (size_t)L0.pitch, img_bytes = pitch0 * (size_t)height;
    // outputs of both images in the handle's output block (two images of its capacity), the
    // pair's stereo block behind the whole block; one DMA back when the block holds just the
    // two images, else two
    const OutLayout& ol = h->out;
    const StereoLayout sl(1, ol.KC);
    const size_t o_end = ol.desc_end(2), o_s = ol.after(ol.B);
    const bool one_dma = h->cap_batch == 2;
    if (!ensure_pinned(h->h_out, h->h_out_n, o_s + sl.end)) return ORBX_ERR_DEVICE;
    if (!ensure_pinned(h->h_in, h->h_in_n, 2 * img_bytes)) return ORBX_ERR_DEVICE;
    stage_frame(h, h->h_in, pitch0, img_bytes, left, stride_left, right, stride_right, width,
                height, false);
    uint8_t* d_l0 = h->d_pyr.as<uint8_t>() + L0.off;   // image 0's level-0 slot
    const size_t pyrb = (size_t)h->hg.pyr_bytes;
    if (!order_after_last(h, st)) return ORBX_ERR_DEVICE;
    uint8_t* dso = h->d_outs.as<uint8_t>() + o_s;
    const ExtractLaunch a = extract_launch(h, nullptr, nullptr, 2, 2, 0, 0);
    StereoLaunch sa;   // pair 0 = (image 0, image 1) of this handle
    s = stereo_launch_args(h, h, 1, 0, 1, mbf, mb, (float*)(dso + sl.o_u),
                           (float*)(dso + sl.o_d), (int*)dso, st, sa);
    if (s != ORBX_OK) return s;
    // the device sequence: both images into their level-0 slots by one 2-D DMA (a row = one
    // image; an image DMA'd ahead of the graph while the other is staged measured the same at
    // one session and slower at eight: one more submission), the two-image extraction, the
    // stereo match, the outputs back
    auto enqueue = [&](const ExtractLaunch& ea) {
        bool ok = HIPOK(hipMemcpy2DAsync(d_l0, pyrb, h->h_in, img_bytes, img_bytes, 2,
                                         hipMemcpyHostToDevice, st)) &&
                  HIPOK(launch_extract(ea, st)) && HIPOK(launch_stereo(sa, st));
        if (one_dma)
            return ok && HIPOK(hipMemcpyAsync(h->h_out, h->d_outs.p, o_s + sl.end,
                                              hipMemcpyDeviceToHost, st));
        return ok &&
               HIPOK(hipMemcpyAsync(h->h_out, h->d_outs.p, o_end, hipMemcpyDeviceToHost, st)) &&
               HIPOK(hipMemcpyAsync(h->h_out + o_s, dso, sl.end, hipMemcpyDeviceToHost, st));
    };
    if (!run_graphed(h, a, st, width, height, enqueue, h->g_frame,
                     {key_word(h->d_sscr.p), key_word(mbf), key_word(mb), (uint64_t)one_dma}))
        return ORBX_ERR_DEVICE;
    // the stereo-frame pyramid contract (keep_pyr); no keypoint count: not the single-image
    // state orbx_stereo_match expects
    set_last(h, 2, true, h->keep_pyr ? 2 : 0);
    const uint8_t* ho = h->h_out;
    std::memcpy(out->n, ho, 8);
    for (int v = 0; v < 2; ++v) {
        out->kps[v] = (const orbx_keypoint*)(ho + ol.kps_end(v));
        out->desc[v] = ho + ol.desc_end(v);
    }
    std::memcpy(&out->n_valid, ho + o_s, 4);
    out->u_right = (const float*)(ho + o_s + sl.o_u);
    out->depth = (const float*)(ho + o_s + sl.o_d);
    return ORBX_OK;
}

extern "C" {

orbx_status orbx_stereo_frame_view(orbx_extractor* h, const uint8_t* left, size_t stride_left,
                                   const uint8_t* right, size_t stride_right, int width,
                                   int height, float mbf, float mb, orbx_stereo_frame_out* out) {
    if (!h || !out || !left || !right || width <= 0 || height <= 0 ||
        stride_left < (size_t)width || stride_right < (size_t)width)
        return ORBX_ERR_INVALID;
    FrameServer& fs = frame_server(h);
    frame_server_use(h, fs);
    std::unique_lock<std::mutex> lk(fs.mu);
    if (fs.inflight == 0 && fs.n == 0) {   // alone on the device: on this handle
        ++fs.inflight;
        fs.stats.solo_calls++;
        lk.unlock();
        const orbx_status s = stereo_frame_solo(h, left, stride_left, right, stride_right, width,
                                                height, mbf, mb, out);
        lk.lock();
        --fs.inflight;
        fs.cv.notify_all();
        return s;
    }
    lk.unlock();
    FsBatch g{width, height, mbf, mb, 0, 0};
    {
        std::lock_guard<std::mutex> hl(h->mu);
        const orbx_status s = ensure_workspace(h, width, height, 1);   // the level-0 pitch
        if (s != ORBX_OK) return s;
        g.pitch0 = (size_t)h->hg.lv[0].pitch;
        g.img_bytes = g.pitch0 * (size_t)height;
    }
    auto same = [](const FsBatch& x, const FsBatch& y) {
        return x.width == y.width && x.height == y.height && x.pitch0 == y.pitch0 &&
               std::memcmp(&x.mbf, &y.mbf, 4) == 0 && std::memcmp(&x.mb, &y.mb, 4) == 0;
    };
    FsReq r{h};
    lk.lock();
    // join the batch being formed (after a full one, or one of another size or camera, goes)
    // (a batch opens in a block pair whose last batch has finished)
    fs.cv.wait(lk, [&] {
        return fs.n == 0 ? !fs.pair_busy[fs.blk] : fs.n < FS_MAX_FRAMES && same(fs.geo, g);
    });
    if (fs.n == 0) {   // open it: its blocks were last used by a batch that has finished
        const size_t bytes = 2 * FS_MAX_FRAMES * g.img_bytes;
        if (!HIPOK(hipSetDevice(h->device)) ||
            (!fs.cst && !HIPOK(hipStreamCreateWithFlags(&fs.cst, hipStreamNonBlocking))) ||
            (!fs.cev[fs.blk] &&
             !HIPOK(hipEventCreateWithFlags(&fs.cev[fs.blk], hipEventDisableTiming))) ||
            !ensure_pinned(fs.hin[fs.blk], fs.hin_n[fs.blk], bytes) ||
            !fs.dstage[fs.blk].ensure(bytes))
            return ORBX_ERR_DEVICE;
        fs.geo = g;
    }
    r.slot = fs.n++;
    r.blk = fs.blk;
    fs.req[r.slot] = &r;
    const size_t fofs = (size_t)r.slot * 2 * g.img_bytes;
    uint8_t* dst = fs.hin[r.blk] + fofs;
    uint8_t* ddst = fs.dstage[r.blk].as<uint8_t>() + fofs;
    lk.unlock();
    bool copied;
    {
        std::lock_guard<std::mutex> hl(h->mu);
        stage_frame(h, dst, g.pitch0, g.img_bytes, left, stride_left, right, stride_right, width,
                    height, true);
        copied = HIPOK(hipSetDevice(h->device)) &&
                 HIPOK(hipMemcpyAsync(ddst, dst, 2 * g.img_bytes, hipMemcpyHostToDevice, fs.cst));
    }
    lk.lock();
    if (!copied) r.st = ORBX_ERR_DEVICE;   // the batch still counts the slot
    ++fs.staged;
    fs.cv.notify_all();
    while (!r.done) {
        // only a frame of the batch being formed leads it (a frame whose batch already has a
        // lead waits for it, instead of leading someone else's batch and holding its reader
        // slot meanwhile)
        if (r.taken || fs.inflight >= FS_INFLIGHT || fs.n == 0 || fs.staged < fs.n) {
            fs.cv.wait(lk);
            continue;
        }
        // lead: the batch being formed goes, the next one forms in the other block pair
        const int m = fs.n, blk = fs.blk;
        FsReq* take[FS_MAX_FRAMES];
        std::copy(fs.req, fs.req + m, take);
        for (int i = 0; i < m; ++i) take[i]->taken = true;
        // every frame's copy is on the stream by now (each was issued before its `staged`)
        const bool recorded = HIPOK(hipEventRecord(fs.cev[blk], fs.cst));
        const FsBatch bg = fs.geo;
        fs.n = fs.staged = 0;
        fs.blk ^= 1;
        ++fs.inflight;
        fs.pair_busy[blk] = true;
        fs.stats.batches++;
        fs.stats.served_frames += m;
        fs.stats.batches_of_size[m]++;
        fs.stats.batches_per_pair[blk]++;
        fs.stats.peak_inflight = std::max(fs.stats.peak_inflight, fs.inflight);
        fs.stats.resident = 1;
        fs.cv.notify_all();
        fs.cv.wait(lk, [&] { return fs.readers[blk] == 0; });   // two batches ago: copied out
        lk.unlock();
        orbx_status bs = recorded ? run_served(fs, take[0]->h, m, blk, bg) : ORBX_ERR_DEVICE;
        for (int i = 0; i < m; ++i)
            if (take[i]->st != ORBX_OK) bs = take[i]->st;   // a frame's copy failed
        lk.lock();
        for (int i = 0; i < m; ++i) {
            take[i]->st = bs;
            take[i]->done = true;
        }
        if (bs == ORBX_OK) fs.readers[blk] += m;
        --fs.inflight;
        fs.pair_busy[blk] = false;
        fs.cv.notify_all();
    }
    lk.unlock();
    const orbx_status s = r.st == ORBX_OK ? copy_served(fs, r, g, out) : r.st;
    if (r.st == ORBX_OK) {
        lk.lock();
        --fs.readers[r.blk];
        fs.cv.notify_all();
    }
    return s;
}

orbx_status orbx_frame_server_get_stats(const orbx_extractor* h, orbx_frame_server_stats* out,
                                        int reset) {
    if (!h || !out) return ORBX_ERR_INVALID;
    FrameServer& fs = frame_server(h);
    std::lock_guard<std::mutex> lk(fs.mu);
    *out = fs.stats;
    out->users = fs.users;
    if (reset) {
        const int32_t resident = fs.stats.resident;
        fs.stats = orbx_frame_server_stats{};
        fs.stats.resident = resident;
    }
    return ORBX_OK;
}

orbx_status orbx_frame_server_release(const orbx_extractor* h) {
    if (!h) return ORBX_ERR_INVALID;
    FrameServer& fs = frame_server(h);
    std::lock_guard<std::mutex> lk(fs.mu);
    if (!fs.idle()) return ORBX_ERR_STATE;
    fs.release_resources();
    return ORBX_OK;
}

}  // extern "C"
