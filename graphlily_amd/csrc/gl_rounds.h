// The scheduling idiom of the round-based graph kernels on the row copy (gl_rows.h) -- gl_cc's hook, gl_kcore, gl_color, gl_truss,
// gl_msf, gl_match, gl_lpa, gl_scc, gl_bicc's level search, gl_topo, gl_msbfs (the atomics and the host loop) -- stated once: the atomics of the memory rule, the wavefront-aggregated append to a queue, the control
// record of the two peeling kernels, and the host loop that enqueues gated batches blindly and reads the record back once per batch.
//
// MEMORY RULE (gfx950: eight XCDs with private L2s -- a plain store is not seen across them within a launch): a word that one
// workgroup writes and another reads IN THE SAME LAUNCH is touched only through the ga_* wrappers below, relaxed agent-scope atomics
// on a global-address-space pointer.  Plain loads and stores only behind a launch boundary.  No spin-waits, no tickets, no hand-offs
// between workgroups.  Each kernel's header names its atomic-only arrays.
// GATING: every launch is correct whatever the previous one left in the control record -- it returns at once when the record says
// that its phase is not on, or that the run is done -- so the host enqueues `batch` rounds blindly, copies the record to the
// page-locked staging words (gl_common.h: staging_words) and waits ONCE per batch.  The result does not depend on `batch`.  Each
// kernel's header says why its step cap holds.
#ifndef GL_ROUNDS_H_
#define GL_ROUNDS_H_

#include "gl_rows.h"

namespace gl {

typedef __attribute__((address_space(1))) uint32_t ga_u32;
typedef __attribute__((address_space(1))) unsigned long long ga_u64;
#define GA_ORDER __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// add and sub -> the word's value before
__device__ __forceinline__ uint32_t ga_load(uint32_t *p) { return __hip_atomic_load((ga_u32 *)p, GA_ORDER); }
__device__ __forceinline__ void ga_store(uint32_t *p, uint32_t v) { __hip_atomic_store((ga_u32 *)p, v, GA_ORDER); }
__device__ __forceinline__ uint32_t ga_add(uint32_t *p, uint32_t v) { return __hip_atomic_fetch_add((ga_u32 *)p, v, GA_ORDER); }
__device__ __forceinline__ uint32_t ga_sub(uint32_t *p, uint32_t v) { return __hip_atomic_fetch_sub((ga_u32 *)p, v, GA_ORDER); }
__device__ __forceinline__ void ga_min(uint32_t *p, uint32_t v) { (void)__hip_atomic_fetch_min((ga_u32 *)p, v, GA_ORDER); }
__device__ __forceinline__ void ga_max(uint32_t *p, uint32_t v) { (void)__hip_atomic_fetch_max((ga_u32 *)p, v, GA_ORDER); }
// -> did the swap take place?  `expect` becomes the value found either way: a retry goes on from it, never from a re-read
__device__ __forceinline__ bool ga_cas(uint32_t *p, uint32_t &expect, uint32_t desired) {
    return __hip_atomic_compare_exchange_strong((ga_u32 *)p, &expect, desired, __ATOMIC_RELAXED, GA_ORDER);
}
__device__ __forceinline__ unsigned long long ga_load(unsigned long long *p) { return __hip_atomic_load((ga_u64 *)p, GA_ORDER); }
__device__ __forceinline__ void ga_store(unsigned long long *p, unsigned long long v) { __hip_atomic_store((ga_u64 *)p, v, GA_ORDER); }
__device__ __forceinline__ void ga_add(unsigned long long *p, unsigned long long v) { (void)__hip_atomic_fetch_add((ga_u64 *)p, v, GA_ORDER); }
__device__ __forceinline__ void ga_min(unsigned long long *p, unsigned long long v) { (void)__hip_atomic_fetch_min((ga_u64 *)p, v, GA_ORDER); }

// Wavefront-aggregated append: EVERY lane of the wavefront calls it; the lanes with `hit` get consecutive positions behind
// *counter -- one ballot and one atomic add per wavefront.  A lane without `hit` gets a position it must not use.  The caller
// keeps its own bound check and its own stores.
__device__ __forceinline__ uint32_t wave_append(bool hit, uint32_t *counter, uint32_t lane) {
    const unsigned long long m = __ballot(hit);
    uint32_t base = 0;
    if (m != 0ull) {
        const int leader = __ffsll(m) - 1;
        if ((int)lane == leader) base = ga_add(counter, (uint32_t)__popcll(m));
        base = __shfl(base, leader);
    }
    return base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

// Every control record takes two 128-byte lines: the words a turn kernel owns in the first, the words that the launches between
// two turns add to -- the queue's tail first of all -- in the second.
constexpr uint32_t kRoundsCtlBytes = 256;

// The control record of the peeling kernels (words), gl_kcore.hip over vertices and gl_truss.hip over edges: the level, the queue
// slice [lo, hi) of the sub-round, the phase, the counters a turn keeps, the tail.  Their turn kernels differ (truss jumps empty
// levels and counts a sub-round when its slice is cut, k-core when it was peeled) and stay apart.
enum : uint32_t { kPeelLevel = 0, kPeelLo = 1, kPeelHi = 2, kPeelPhase = 3, kPeelLevels = 4, kPeelSubRounds = 5, kPeelLevelStart = 6,
                  kPeelTop = 7, kPeelRecordWords = 8, kPeelTail = 32 };
enum : uint32_t { kPeelScan = 0, kPeelPeel = 1, kPeelDone = 2 };
// ... and the words gl_truss.hip adds: the smallest support a scan saw above its level, and the 64-bit sum of the supports
enum : uint32_t { kTrussNext = 8, kTrussRecordWords = 9, kTrussSum = 34 };

enum RoundsVerdict { kRoundsGoOn, kRoundsDone, kRoundsStuck };

// The gated host loop.  Per batch: enqueue() enqueues `batch` steps and whatever rides behind them and returns the launches it
// enqueued (`launches` is added to); copy() enqueues the copies of the record into the staging words and returns their hipError_t;
// after ONE synchronisation verdict() reads the staging words; a run that is stuck, or not done after max_steps steps, ends with
// what fail(steps) returns (set_error, in the caller's wording).  kcore(), color(), truss(), msf(), match(), lpa(), scc(), bicc(), topo() and msbfs() all fit without a flag.
template <typename Enqueue, typename Copy, typename Verdict, typename Fail>
int rounds_run(uint32_t batch, uint64_t max_steps, uint64_t &launches, Enqueue enqueue, Copy copy, Verdict verdict, Fail fail) {
    for (uint64_t steps = batch;; steps += batch) {
        launches += enqueue();
        GL_LAUNCH_CHECK();
        GL_HIP(copy());
        GL_HIP(hipStreamSynchronize(ctx().stream));
        const RoundsVerdict v = verdict();
        if (v == kRoundsDone) return GL_OK;
        if (v == kRoundsStuck || steps >= max_steps) return fail(steps);
    }
}

}  // namespace gl

#endif  // GL_ROUNDS_H_
