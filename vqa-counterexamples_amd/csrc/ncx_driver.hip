// ncx_driver.hip -- host-side plumbing of the launches (host only): the GEMM driver, the opt-in side stream, the opt-in
// profiler / stamp state and the dropout epilogue arguments.
#include "ncx_driver.h"

namespace ncx {
// Internal side stream: independent small kernels (each under-fills 256 CUs, or is HBM-bound while the other is
// MFMA-bound) are forked from the caller's stream and joined back with events, so the work stays fully ordered
// with respect to `stream`.  One lazily created (stream, 2 events) triple per device.  Measured on MI355X at
// configs[1]: round 1 (Gt, Sh || k_prep; dW1ak || dE) 1.236-1.253 ms/step with it vs 1.221-1.228 without; round 2 (the
// whole answer-embedding chain || k_dw_km as well) 1.001-1.003 vs 0.985-0.992: the fork/join events cost what the
// overlap wins and a full round of long workgroups leaves the short ones no slots, so it is OFF unless NCX_SIDE_STREAM=1.
SideStream* side_stream() {
    static SideStream tab[16];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) { (void)hipGetLastError(); return nullptr; }
    SideStream& t = tab[dev];
    if (t.state == 0) {
        const char* on = getenv("NCX_SIDE_STREAM");
        t.state = -1;
        t.mode = on ? atoi(on) : 0;
        if ((on && atoi(on)) &&
            hipStreamCreateWithFlags(&t.s, hipStreamNonBlocking) == hipSuccess &&
            hipEventCreateWithFlags(&t.fork, hipEventDisableTiming) == hipSuccess &&
            hipEventCreateWithFlags(&t.join, hipEventDisableTiming) == hipSuccess) t.state = 1;
        else (void)hipGetLastError();
    }
    return t.state == 1 ? &t : nullptr;
}

// backward_impl's choices for a whole backward (phases 0 / 1 + 2): the per-triplet fold kernel waits for the side stream's chain
// (opt-in: NCX_SIDE_STREAM)
bool km_defers_to_side_stream(const ncx_dims& d, const StepRoutes& r) {
    return r.km && (d.flags & NCX_F_A_EMB) && side_stream() != nullptr && side_stream()->mode != 2;
}
// fork: the side stream waits for everything enqueued on `main` so far
int side_fork(SideStream* ss, hipStream_t main) {
    NCX_HIP_TRY(hipEventRecord(ss->fork, main));
    NCX_HIP_TRY(hipStreamWaitEvent(ss->s, ss->fork, 0));
    return 0;
}
// join: `main` waits for everything enqueued on the side stream so far
int side_join(SideStream* ss, hipStream_t main) {
    NCX_HIP_TRY(hipEventRecord(ss->join, ss->s));
    NCX_HIP_TRY(hipStreamWaitEvent(main, ss->join, 0));
    return 0;
}

// -------------------------------------------------------------------------------------------------
// Opt-in diagnostics (ncx_profile_begin/_end): HIP events around every launch of ONE chosen GEMM, on the
// stream it is launched on.  Off by default; the only process-global state of the library.
// -------------------------------------------------------------------------------------------------
ProfState g_prof = {false, 0u, 0, 0, nullptr, nullptr};
// ncx_profile_stamps: in-kernel clock stamps of MAIN (diagnostic passes only).  One slot per DEVICE, like side_stream()'s table: the
// buffer is a device pointer, so a forward on another GPU of the same process must never see it; pointer and capacity are published
// together (the capacity is written first, the pointer last, and read in the opposite order) so a concurrent forward sees either
// the old pair or the new one.
StampSlot g_stamps[16];
unsigned long long* stamps_for_current_device(long long need_words) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) { (void)hipGetLastError(); return nullptr; }
    unsigned long long* p = g_stamps[dev].ptr.load(std::memory_order_acquire);
    if (!p || g_stamps[dev].words.load(std::memory_order_acquire) < need_words) return nullptr;
    return p;
}

// HIP-event bracket of a launch sequence that is not a run_gemm call (the bf16 variant's GEMMs)
int prof_open(int use_id, hipStream_t s) {
    if (g_prof.on && ((g_prof.mask >> use_id) & 1u) && g_prof.n < g_prof.cap) NCX_HIP_TRY(hipEventRecord(g_prof.ev[2 * g_prof.n], s));
    return NCX_OK;
}
int prof_close(int use_id, hipStream_t s) {
    if (g_prof.on && ((g_prof.mask >> use_id) & 1u) && g_prof.n < g_prof.cap) {
        NCX_HIP_TRY(hipEventRecord(g_prof.ev[2 * g_prof.n + 1], s)); g_prof.ids[g_prof.n] = use_id; ++g_prof.n;
    }
    return NCX_OK;
}

// The GEMM driver (ncx_internal.h).  Defaults the per-problem splits in place; bytes of the split-K slab the launch needs.
static size_t default_splits(GemmArgs& a, const GemmPlan& pl) {
    const int np = a.mode == MODE_GROUP ? a.nseg : 1;
    bool any = false;
    for (int i = 0; i < np; ++i) {
        if (a.split[i] == 0) a.split[i] = pl.split;              // callers may preset per-problem splits
        any |= a.split[i] > 1;
    }
    if (!any) return 0;
    int bm, bn; cfg_tile(pl.cfg, bm, bn);
    return (size_t)gemm_layout(a, bm, bn, nullptr) * bm * bn * 4;
}
size_t gemm_slab_bytes(GemmArgs a, const GemmPlan& pl) { return default_splits(a, pl); }
int run_gemm_planned(GemmArgs& a, int form, const GemmPlan& pl, float* slab, size_t slab_bytes, const float* reduce_bias, hipStream_t s, bool no_fast) {
    { const char* nf = hook_env("NCX_NO_FAST"); a.pad_ = (no_fast || (nf && atoi(nf))) ? 1 : 0; }
    const size_t need = default_splits(a, pl);
    if (need > slab_bytes) return NCX_E_WORKSPACE;
    if (need) a.slab = slab;
    if (reduce_bias) a.epi.bias = reduce_bias;                   // applied by the epilogue or by the fix-up kernel
    if (form == FORM_NT) return run_gemm_nt(a, pl.cfg, s);
    if (form == FORM_TN) return run_gemm_tn(a, pl.cfg, s);
    return run_gemm_nn(a, pl.cfg, s);
}
int run_gemm(int use_id, GemmArgs& a, int form, const GemmPlan& pl, float* slab, size_t slab_bytes, const float* reduce_bias, hipStream_t s) {
    return profiled(use_id, s, [&] { return run_gemm_planned(a, form, pl, slab, slab_bytes, reduce_bias, s); });
}

void set_dropout(EpiArgs& e, const ncx_dims& d, const ncx_inputs& in, int layer, long long M) {
    e.relu = 1;
    if (d.training && d.drop_p > 0.f) {
        e.drop_p = d.drop_p; e.drop_scale = 1.f / (1.f - d.drop_p);
        if (in.keep_mask) { e.dropout = 2; e.keep_mask = in.keep_mask + (long long)(layer - 1) * M * d.H; e.ld_mask = d.H; }
        else { e.dropout = 1; e.seed_lo = (unsigned)(d.seed & 0xFFFFFFFFull); e.seed_hi = (unsigned)(d.seed >> 32); e.layer = (unsigned)layer; }
    }
}
}  // namespace ncx
