// orbx_extractor.h — the extractor handle and what its translation units share (private: not
// installed).  orbx_plan.hip builds the tables and the per-size geometry, orbx_capi.hip owns the
// handle, its workspace and the C ABI, orbx_stereo_frame.hip the one-call stereo frame.
#pragma once
#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <vector>

#include "orbx_host.h"
#include "orbx_kernels.h"
#include "orbx_layout.h"

namespace orbx {

// What orbx_plan.hip builds from the extractor parameters (compute_tables) and one image size
// (build_geometry); the handle embeds it.
struct ExtractPlan {
    // ORBextractor tables
    std::vector<float> scale, inv_scale, sigma2, inv_sigma2;
    std::vector<int> nfeat;
    int umax[16], taps[7];
    // geometry of the current image size
    Geometry hg;
    std::vector<CellDesc> cells;
    std::vector<int16_t> rtab;
    std::vector<uint8_t> ltab;   // k_level_strip / k_pyr_chain tables (StripLane, ChainRect, ...)
    int ncap = 0, kcap = 0;
    size_t octree_lds = 0, stereo_lds = 0;
    int kcap_small = 0;               // small-batch octree: candidates held in LDS
    size_t octree_lds_small = 0;
    long long kscratch_per_image = 0;
};

// A captured device sequence and what it was captured for: image size, effective schedule, the
// output block's layout and every buffer address the sequence names (a regrown buffer can come
// back at the same address, so the sizes that lay it out are part of the key).
struct GraphSlot {
    hipGraphExec_t exec = nullptr;
    std::vector<uint64_t> key;
    void destroy() { if (exec) (void)hipGraphExecDestroy(exec); exec = nullptr; key.clear(); }
};
inline uint64_t key_word(const void* p) { return (uint64_t)(uintptr_t)p; }
inline uint64_t key_word(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }

}  // namespace orbx

struct OrbxStager;   // orbx_stereo_frame.hip

struct orbx_extractor : orbx::ExtractPlan {
    orbx_extractor_params prm;
    int device = 0;
    int ncu = 256;                // compute units of the device (strip-height heuristic)
    hipStream_t stream = nullptr;
    // `done` is recorded after the last work issued for this handle (on `done_stream`): a
    // later call on another stream waits for it, and table updates / buffer growth / host
    // fetches wait on it instead of on the whole device
    hipEvent_t done = nullptr;
    hipStream_t done_stream = nullptr;
    bool have_done = false;
    // side branch of launch_extract (level-0 FAST beside the level launches): a stream of its
    // own, forked from and joined back into the call's stream by two events
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    int side_mode = FAST_SIDE, side_at = FAST_SIDE_AT, side_lv = FAST_SIDE_LV;
    bool side_auto = true;   // the built-in default: no side branch below SIDE_MIN_BATCH images
    // the device sequences of orbx_extract (H2D, kernels, D2H) and of orbx_stereo_frame_view
    // (2-D H2D, two-image extraction, stereo, D2H) as HIP graphs (run_graphed)
    orbx::GraphSlot g_extract, g_frame;
    // pinned staging of the host-image path (orbx_extract / orbx_stereo_match)
    uint8_t* h_in = nullptr;
    size_t h_in_n = 0;
    uint8_t* h_out = nullptr;
    size_t h_out_n = 0;
    // mvImagePyramid on the host (orbx_extractor_host_pyramid): every orbx_extract(_view) also
    // copies its image's pyramid block here (a pinned block of its own: no other call writes it)
    bool host_pyr = false;
    bool host_pyr_ok = false;   // h_pyr holds the last orbx_extract(_view)'s pyramid
    uint8_t* h_pyr = nullptr;
    size_t h_pyr_n = 0;
    bool have_geom = false;     // the plan's geometry (hg, ...) is built and on the device
    int cap_batch = 0;
    orbx::DevBuf d_geom, d_cells, d_rtab, d_ltab, d_pyr, d_blur, d_ccnt, d_cand, d_ocnt, d_okp,
        d_kscr, d_kps, d_desc, d_nkp, d_uR, d_sscr;
    // one allocation, so that one DMA returns a call's results: the extraction outputs (d_nkp /
    // d_kps / d_desc are views of it, laid out by `out`), at out.after(cap_batch) a stereo block
    orbx::DevBuf d_outs;
    orbx::OutLayout out;
    orbx::KernelTimer timer;
    // last extraction
    int last_batch = 0;
    bool last_valid = false;
    int last_n = 0;          // keypoints of the last orbx_extract (host image path)
    // images [0, pyr_images) of d_pyr hold the raw pyramids of the last call (mvImagePyramid,
    // orbx_pyramid_level).  A stereo frame (orbx_stereo_frame_view) leaves them only when
    // keep_pyr is set, solo or served alike (orbx_extractor_keep_pyramid)
    int pyr_images = 0;
    uint64_t serial = 0;     // +1 whenever the pyramids change (orbx_extractor_serial)
    bool keep_pyr = false;
    bool fs_user = false;    // counted as a user of its frame server (released with the last)
    // of the first queued stereo frame (shared_ptr: destroyed without OrbxStager's definition)
    std::shared_ptr<OrbxStager> stager;
    // guards every field above against concurrent calls on one handle (const queries too)
    mutable std::mutex mu;
};

namespace orbx {

// ---- orbx_plan.hip: the plan and the batch-size policies of a launch ------------------------
void compute_tables(const orbx_extractor_params& prm, ExtractPlan& p);
orbx_status build_geometry(const orbx_extractor_params& prm, int W, int H, ExtractPlan& p);
void strip_heights(const orbx_extractor* h, int nimg, int* sth);
int fast_cells_per_wave(int ncells, int batch, int ncu);
int octree_small(int batch);
int side_mode_of(const orbx_extractor* h, int batch);
int chain_of(const orbx_extractor* h, int in_place, int side_mode, int batch);

// ---- orbx_capi.hip: ordering, workspace and launch descriptors (h->mu held) -------------------
bool order_after_last(orbx_extractor* h, hipStream_t st);
bool mark_done(orbx_extractor* h, hipStream_t st);
bool wait_idle(orbx_extractor* h);
bool wait_done(orbx_extractor* h);
bool ensure_pinned(uint8_t*& p, size_t& cap, size_t n);
orbx_status ensure_workspace(orbx_extractor* h, int W, int H, int batch);
ExtractLaunch extract_launch(orbx_extractor* h, const uint8_t* d_imgs, const uint8_t* d_imgs2,
                             int split, int batch, size_t stride, size_t batch_stride);
orbx_status stereo_launch_args(orbx_extractor* L, orbx_extractor* R, int batch, int offL,
                               int offR, float mbf, float mb, float* d_uR, float* d_dep,
                               int* d_nv, hipStream_t st, StereoLaunch& a);
// The "last extraction" state after a call: the outputs of `batch` images are in the workspace
// and valid or not (batch 0: they are gone, last_batch stays), the raw pyramids of images
// [0, pyr_images) are, and n is the keypoint count of a lone host image (-1: on the device only).
void set_last(orbx_extractor* h, int batch, bool valid, int pyr_images, int n = -1);
// One host-image sequence on st, whose earlier work the caller has ordered it after: `enqueue`
// (copies in, kernels, copies out) replayed from `slot`, captured first when the slot's key is
// stale (the handle's own words, then `extra`), or run eagerly while kernels are timed; then the
// handle's done event and the host wait.  wait_ev (or null) is waited for on st between the
// capture and the launch.  False: a HIP call failed (recorded).
bool run_graphed(orbx_extractor* h, const ExtractLaunch& a, hipStream_t st, int width, int height,
                 const std::function<bool(const ExtractLaunch&)>& enqueue, GraphSlot& slot,
                 std::vector<uint64_t> extra, hipEvent_t wait_ev = nullptr);

// ---- orbx_stereo_frame.hip --------------------------------------------------------------------
void frame_server_unuse(orbx_extractor* h);

}  // namespace orbx
