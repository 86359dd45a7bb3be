// orbx_matcher.h — the matcher handle (orbx_matcher_create), for the translation units whose
// *_batch_device entries hold its mutex, make its device current and size its scratch buffers.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>

#include "../../include/orbx_match.h"
#include "orbx_host.h"
#include "orbx_kernels.h"

struct orbx_matcher {
    orbx_matcher_params prm;
    int ncu = 256;                     // compute units of the device (BF chunk sizing)
    // d_bf_db: the database of orbx_hamming_bf_top2 (it may be gigabytes: not in a pooled slot)
    orbx::DevBuf d_aux, d_proj, d_bf, d_bf_db, d_sim3, d_pnp;
    int* d_err = nullptr;    // the capacity word of the *_device forms (orbx_matcher_sync)
    orbx::KernelTimer timer;
    std::mutex mu;
    // recorded after the last brute-force launch (its partial-result scratch d_bf is shared by
    // every call): a call on another stream waits for it before reusing the scratch
    hipEvent_t bf_done = nullptr;
    hipStream_t bf_stream = nullptr;
    bool have_bf = false;
    int bf_kernel = ORBX_BF_MFMA;
    int bf_chunk = 0;               // orbx_matcher_set_bf_chunk: 0 = bf_chunk_rows
};
