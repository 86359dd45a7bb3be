// orbx_match_kernels.h — launch descriptors of the matcher kernels (orbx_match.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/orbx_frame.h"
#include "../../include/orbx_match.h"

namespace orbx {

// Internal projection mode after the public ones: SearchForInitialization (:446-561).
constexpr int PROJ_INIT = ORBX_PROJ_MODE_COUNT;
constexpr int PROJ_K = 8;             // candidate list length of the claim-mode replay
constexpr int MATCH_MAX_LEVELS = 16;

// SearchByBoW over jobs: job j pairs keyframe (a_fixed ? 0 : j) of A with keyframe
// (b_fixed ? 0 : j) of B.  kf_kf = 0: SearchByBoW(KeyFrame*, Frame&) (A = keyframe, B = frame,
// outputs indexed by B feature); kf_kf = 1: SearchByBoW(KeyFrame*, KeyFrame*) (outputs indexed
// by A feature).
struct BowLaunch {
    orbx_kf_db A, B;
    int a_fixed, b_fixed, kf_kf, njobs;
    float ratio;
    int check_ori;
    int32_t* out;
    int out_stride;
    int32_t* nmatches;
    int* err;
};

hipError_t launch_node_order(const orbx_kf_db& db, int n, orbx_keypoint* keys, uint8_t* desc,
                             float* ur, uint8_t* flag, hipStream_t st);

struct TriLaunch {
    orbx_kf_db db;
    int njobs;
    const int32_t* kf1;
    const int32_t* kf2;
    const float* F12;
    const float* epi;
    float sigma2[MATCH_MAX_LEVELS];
    float scale[MATCH_MAX_LEVELS];
    int only_stereo, check_ori;
    const int32_t* job_off;
    int32_t* out;
    int32_t* nmatches;
    int* err;
};

// The per-match loop behind SearchForTriangulation (orbx_triangulate.hip): job j's slots are
// [job_off[j], job_off[j + 1]), one per KF1 feature, match12[slot] the KF2 feature or -1.
// feat_off / keys / u_right are the database's; depth / cos_stereo / keys_raw (may be null) are
// indexed like keys.  err: set when a lane refuses its slot (see include/orbx_match.h).
struct TriPointsLaunch {
    int nkf;
    const int32_t* feat_off;
    const orbx_keypoint* keys;
    const orbx_keypoint* keys_raw;
    const float* u_right;
    const float* depth;
    const float* cos_stereo;
    const orbx_frame_pose* poses;
    const int32_t* kf1;
    const int32_t* kf2;
    const int32_t* job_off;
    const int32_t* match12;
    float ratio_factor;
    int32_t* status;
    float* x3d;
    int32_t* nnew;
    int* err;
};
// Zeroes nnew[njobs] and launches k_triangulate_points over (max_feat, njobs).
hipError_t launch_triangulate_points(const TriPointsLaunch& a, int max_feat, int njobs,
                                     hipStream_t st);

// Sim3Solver::iterate over njobs solvers (orbx_sim3.hip, which launches it and sizes scratch).  The
// array lengths bound what a job may point at.
struct Sim3Launch {
    const orbx_sim3_job* jobs;
    int njobs, max_n, max_call;
    const orbx_frame_pose* poses;
    int nposes;
    const orbx_sim3_corr* corr;
    long long ncorr;
    const int32_t* triples;
    long long ntriples;
    orbx_sim3_state* state;
    orbx_sim3_result* res;
    uint8_t* inliers;
    long long ninliers;
    void* scratch;
};
constexpr int SIM3_MAX_N = 8192, SIM3_MAX_ITS = 4096, SIM3_MAX_JOBS = 65535;
constexpr size_t SIM3_MAX_SCRATCH = (size_t)1 << 30;

// Optimizer::OptimizeSim3 over njobs candidates (orbx_sim3opt.hip): one wave per job, no scratch.
// The array lengths bound what a job may point at.
struct Sim3OptLaunch {
    const orbx_sim3opt_job* jobs;
    int njobs, max_n;
    const orbx_frame_pose* poses;
    int nposes;
    const orbx_sim3opt_corr* corr;
    long long ncorr;
    const uint8_t* sim3_in;
    long long in_stride;
    orbx_sim3opt_result* res;
    uint8_t* keep;
    long long nkeep;
};
constexpr int SIM3OPT_MAX_N = 4096, SIM3OPT_MAX_JOBS = 65535;

// PnPsolver::iterate over njobs solvers (orbx_pnp.hip, which launches it and sizes scratch).  The
// array lengths bound what a job may point at.
struct PnpLaunch {
    const orbx_pnp_job* jobs;
    int njobs, max_n, max_call;
    const orbx_pnp_corr* corr;
    long long ncorr;
    const int32_t* quads;
    long long nquads;
    orbx_pnp_state* state;
    uint8_t* best;
    long long nbest;
    orbx_pnp_result* res;
    uint8_t* inliers;
    long long ninliers;
    void* scratch;
};
constexpr int PNP_MAX_N = 4096, PNP_MAX_ITS = 1024, PNP_MAX_JOBS = 4096;
constexpr size_t PNP_MAX_SCRATCH = (size_t)1 << 30;

// Projection searches (modes of orbx_proj_mode plus PROJ_INIT) over njobs independent jobs
// (frames).  With t_off == nullptr there is one job: target T, queries [0, nq).  Otherwise
// job j's target is T's arrays offset by t_off[j] features (keys/desc/u_right/claimed) and
// g_off[j] grid entries (grid_feat, job-local indices), with its own grid_off block of
// cols*rows+1 entries; its queries are [q_off[j], q_off[j+1]).
struct ProjLaunch {
    int mode;
    orbx_featureset T;           // device pointers
    int njobs;
    const int32_t* t_off;
    const int32_t* g_off;
    const int32_t* q_off;
    int max_t;                   // largest target (LDS sizing of the replay kernels)
    const uint8_t* qdesc;
    const orbx_proj_query* q;
    int nq;
    float inv_sigma2[MATCH_MAX_LEVELS];
    int orb_dist;
    float ratio;
    int check_ori;
    const uint8_t* claimed_in;   // may be null
    const uint8_t* qflags;       // nq ORBX_QF_* per query, may be null
    int prefilter;               // ORBX_PROJ_PREFILTER: no rotation-consistency filter
    int32_t* out;                // nq
    int4* top2;                  // nq (PROJ_INIT: static best and second)
    int2* cand;                  // nq x PROJ_K (claim modes: sorted candidate lists)
    int32_t* ncand;              // nq (list length; PROJ_K + 1 = truncated)
    int8_t* out_bin;             // nq
    int32_t* hist;               // 32 per job
    int32_t* nmatches;           // per job
    int* err;
};

hipError_t launch_bow(const BowLaunch& a, hipStream_t st);
size_t bow_lds_bytes(const BowLaunch& a);
// launch_bow's choice: k_bow<true> (B descriptors staged in LDS) or k_bow<false> (global reads)
bool bow_b_in_lds(const BowLaunch& a);
hipError_t launch_triangulate(const TriLaunch& a, hipStream_t st);
size_t tri_lds_bytes(int max_feat);
// Phase A (k_proj_search: window search), B (the mode's sequential replay, if it has one), C
// (k_proj_finish: rotation filter and count).  launch_proj runs the phases the mode needs;
// `timer` ids ORBX_MK_*, both replay kernels under ORBX_MK_PROJ_RESOLVE.
struct KernelTimer;
hipError_t launch_proj(const ProjLaunch& a, hipStream_t st, KernelTimer* timer);
// The replay after k_proj_search in a mode: none (the search's answer is final), k_proj_claim
// (greedy claims of target features) or k_proj_init (SearchForInitialization).
enum ProjReplay { REPLAY_NONE, REPLAY_CLAIM, REPLAY_INIT };
ProjReplay proj_replay(int mode);
// Its dynamic LDS (0 without one); above MATCH_MAX_LDS the search is unsupported.
size_t proj_replay_lds_bytes(int mode, int max_t, int nq);
hipError_t prepare_match_kernels();
// Brute-force Hamming top-2 (orbx_bf.hip): q nq x 32, db ndb x 32 (device); part = scratch of
// bf_partial_bytes(ndb, nq, chunk) bytes.
struct BfLaunch {
    const uint8_t* q;
    int nq;
    const uint8_t* db;
    long long ndb;
    long long idx_base;
    int chunk;
    void* part;
    int32_t* best_idx;
    int32_t* best_dist;
    int32_t* second_dist;
    int kernel;            // ORBX_BF_MFMA / ORBX_BF_VALU
};
int bf_chunk_rows(long long ndb, int nq, int ncu, int kernel);
// A caller's chunk (orbx_matcher_set_bf_chunk): a multiple of 64 in [256, 2^23 - 64]
bool bf_chunk_valid(long long rows);
// The launch geometry of (ndb, nq, chunk, kernel): launch_bf_top2 sizes its grids, the
// partials' stride and k_bf_merge's slices from it, bf_partial_bytes the scratch, and
// orbx_matcher_bf_launch_info reports it.
struct BfGeometry {
    long long nchunks;     // ceil(ndb / chunk): the grids' y
    int query_blocks;      // the distance kernel's grid x (256 / 1024 queries per workgroup)
    int nqpad;             // the partials' query stride
    int merge_slice;       // chunks per thread slice of k_bf_merge (its L)
    size_t partial_bytes;
};
BfGeometry bf_geometry(long long ndb, int nq, int chunk, int kernel);
size_t bf_partial_bytes(long long ndb, int nq, int chunk);
hipError_t launch_bf_top2(const BfLaunch& a, hipStream_t st, KernelTimer* timer);
const char* bf_kernel_name(int kernel);
hipError_t launch_distinctive(const uint8_t* desc, const int32_t* off, int np, int32_t* best,
                              int* err, hipStream_t st);
size_t distinctive_lds_bytes();
// 160 KB of LDS per workgroup on gfx950, minus room for the kernels' static arrays
constexpr size_t MATCH_MAX_LDS = 160 * 1024 - 256;
// k_triangulate also holds 12 KiB of static LDS (one staged KF2 node slice per wave)
constexpr size_t TRI_MAX_LDS = MATCH_MAX_LDS - 16 * 1024;

// The dynamic LDS of the replay kernels in ints from its base, for their pointers and the host's
// sizes.  k_proj_claim, for a largest target of max_t features: hist, an owner word per feature
// while that fits (many queries per round; else one), a claimed byte per feature, 16 spare bytes.
struct ClaimCarve {
    bool owner_words;
    int hist = 0, owner = 32, claimed;
    size_t bytes;
    __host__ __device__ explicit ClaimCarve(int max_t, bool ow = true) : owner_words(ow) {
        claimed = owner + (ow ? max_t : 0);
        bytes = 4 * (size_t)claimed + (size_t)max_t + 16;
        if (ow && bytes > MATCH_MAX_LDS) *this = ClaimCarve(max_t, false);
    }
};
// k_proj_init: hist, vMatchedDistance and vnMatches21 per F2 feature, vnMatches12 per F1 feature.
struct InitCarve {
    int hist = 0, mdist = 32, m21, m12;
    size_t bytes;
    __host__ __device__ InitCarve(int n_target, int nq)
        : m21(mdist + n_target), m12(m21 + n_target), bytes(4 * ((size_t)m12 + (size_t)nq)) {}
};

}  // namespace orbx
