// orbx_host.hip — the out-of-line part of orbx_host.h: the HIP error record, the slot pool behind
// ScratchLease, and the two transfers of a host-array call.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <mutex>
#include <vector>

#include "orbx_host.h"

namespace orbx {

thread_local char g_err[256] = "";
bool hip_ok(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    snprintf(g_err, sizeof(g_err), "%s: %s (%d)", what, hipGetErrorString(e), (int)e);
    return false;
}

namespace {
// the slots no call holds at the moment
std::mutex g_scratch_mu;
std::vector<Scratch*> g_scratch_free;
}  // namespace

ScratchLease::ScratchLease(int device) {
    if (device < 0 || device >= ORBX_MAX_DEVICES || !HIPOK(hipSetDevice(device))) return;
    {
        std::lock_guard<std::mutex> lk(g_scratch_mu);
        for (size_t i = 0; i < g_scratch_free.size(); ++i)
            if (g_scratch_free[i]->device == device) {
                s = g_scratch_free[i];
                g_scratch_free.erase(g_scratch_free.begin() + i);
                break;
            }
    }
    if (!s) {
        Scratch* n = new Scratch();
        n->device = device;
        if (!HIPOK(hipStreamCreateWithFlags(&n->st, hipStreamNonBlocking))) {
            delete n;
            return;
        }
        s = n;
    }
}
ScratchLease::~ScratchLease() {
    if (!s) return;
    std::lock_guard<std::mutex> lk(g_scratch_mu);
    g_scratch_free.push_back(s);   // slots live for the process (no teardown-order hazards)
}

bool HostCall::upload() {
    Scratch& s = *lease_.s;
    const StagePlan& p = s.plan;
    if (!s.buf.ensure(p.end)) return false;
    base_ = s.buf.p;
    return p.up_hi == p.up_lo ||
           HIPOK(hipMemcpyAsync((uint8_t*)base_ + p.up_lo, p.block.data() + p.up_lo,
                                p.up_hi - p.up_lo, hipMemcpyHostToDevice, s.st));
}

orbx_status HostCall::finish(orbx_status status) {
    Scratch& s = *lease_.s;
    StagePlan& p = s.plan;
    if (status == ORBX_OK && p.dn_hi > p.dn_lo &&
        !HIPOK(hipMemcpyAsync(p.block.data() + p.dn_lo, (const uint8_t*)base_ + p.dn_lo,
                              p.dn_hi - p.dn_lo, hipMemcpyDeviceToHost, s.st)))
        status = ORBX_ERR_DEVICE;
    if (!HIPOK(hipStreamSynchronize(s.st))) status = ORBX_ERR_DEVICE;
    p.copy_out(status == ORBX_OK);
    return status;
}

}  // namespace orbx
