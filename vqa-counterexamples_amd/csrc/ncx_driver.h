// ncx_driver.h -- host-side plumbing of the launches (ncx_driver.hip): side stream, profiler / stamp state, the profiled GEMM driver.
#pragma once
#include "ncx_plan.h"
#include <atomic>

#pragma GCC visibility push(hidden)
namespace ncx {
struct SideStream { hipStream_t s; hipEvent_t fork, join; int state, mode; };     // state: 0 new, 1 ready, -1 unavailable; mode = NCX_SIDE_STREAM (1 both passes, 2 forward only, 3 backward only)
SideStream* side_stream();                                   // null unless NCX_SIDE_STREAM is on
int side_fork(SideStream* ss, hipStream_t main);
int side_join(SideStream* ss, hipStream_t main);
bool km_defers_to_side_stream(const ncx_dims& d, const StepRoutes& r);
bool fused_adam_route(const ncx_dims& d, const StepRoutes& r);   // ncx_backward.hip: ncx_backward_adam applies Adam inside the dE launch

struct ProfState { bool on; unsigned mask; int n, cap; hipEvent_t* ev; int* ids; };
extern ProfState g_prof;
struct StampSlot { std::atomic<unsigned long long*> ptr; std::atomic<long long> words; };
extern StampSlot g_stamps[16];
unsigned long long* stamps_for_current_device(long long need_words);
int prof_open(int use_id, hipStream_t s);
int prof_close(int use_id, hipStream_t s);
template <class F> static inline int profiled(int use_id, hipStream_t s, F&& launch) {      // launch() between the two events
    int rc = prof_open(use_id, s); if (rc) return rc;
    rc = launch(); if (rc) return rc;
    return prof_close(use_id, s);
}
// run_gemm_planned (ncx_internal.h) between the profiler's events of use `use_id`
int run_gemm(int use_id, GemmArgs& a, int form, const GemmPlan& pl, float* slab, size_t slab_bytes, const float* reduce_bias, hipStream_t s);
void set_dropout(EpiArgs& e, const ncx_dims& d, const ncx_inputs& in, int layer, long long M);
}  // namespace ncx
#pragma GCC visibility pop
