// The one device-side group hand-out of the persistent ("loop") kernels.  The host half is loop_grid in pf_launch.h: it sizes the grid
// to the resident set and passes a {next, done} counter pair only where a workgroup loops (`ctr == nullptr`: one group per workgroup or a
// plain stride of the grid, no hand-out).
//
// The protocol:
//   * ctr[0] = next, ctr[1] = done.  take_counters (pf_host.h) hands the pair out zeroed, and every launch leaves it zeroed.
//   * The first TWO groups of a workgroup are static: its index, and that plus the grid (`g = blockIdx.x`, `pend = blockIdx.x +
//     gridDim.x` at the site).  The counter hands out what follows: value v = group 2 grid + v.  (Every workgroup used to open with two
//     grabs: ~2 000 atomics on one address, served at ~80 M/s, stood between the launch and the last workgroup's first load - 25-35 us of
//     every launch, tools/r4_small_batch.py.)
//   * At the top of pass `it` ONE thread publishes the group of pass it + 1 in s_next[(it + 1) & 1] and grabs the one of pass it + 2
//     (handout_grab): the atomic's latency is never exposed.  s_next is double-buffered by `it & 1`, so the thread that runs ahead into
//     pass it + 1 writes the other word.
//   * The site's first barrier of the pass publishes s_next to the workgroup; every thread then reads its next group (handout_next).
//     That barrier is usually the first exchange barrier of the transform: it stays where the kernel has it.
//   * A workgroup leaves its loop at the first group past the end; the groups it grabbed beyond that are nobody's.  The thread that
//     grabbed then counts the workgroup done - after a __threadfence, so that the re-armed words are ordered behind its last grab - and
//     the LAST workgroup of the grid zeroes both words for the next launch (handout_rearm).
//
// Each site keeps its own condition (`dyn && threadIdx.x == 0`, `threadIdx.x == 0`, `tid == 0`), its `pend` / `g` variables and its
// barrier: only the bodies are here, by value.  As a struct, with `pend` by reference or with the condition inside the helper the
// compiler schedules some kernels differently; these forms leave the device code of every kernel as it was.
// The kernels that always run on counters (fft_aux.h, fft_pfb.h, fft_c1024.h, pfdsp_mix.h) keep the plain read of s_next for the same
// reason: handout_next(true, ...) changes their code.
// fft_fir32.h, fft_split.h, fft_tile.h, fft_tileg.h, fft_stock.h and fft_one.h run other protocols and do not come here.
#pragma once
#include <hip/hip_runtime.h>

namespace pf {

// publish the group of the next pass, grab the one after it; returns the new `pend`
__device__ __forceinline__ unsigned handout_grab(unsigned* s_next, unsigned it, unsigned pend, unsigned* ctr) {
    s_next[(it + 1) & 1] = pend;
    return 2u * gridDim.x + atomicAdd(&ctr[0], 1u);
}

// after the pass's first barrier: the group of the next pass (without counters: the plain stride of the grid)
__device__ __forceinline__ unsigned handout_next(bool dyn, const unsigned* s_next, unsigned it, unsigned g) {
    return dyn ? s_next[(it + 1) & 1] : g + gridDim.x;
}

// after the loop: count this workgroup done; the last one re-arms both words
__device__ __forceinline__ void handout_rearm(unsigned* ctr) {
    __threadfence();
    unsigned d = atomicAdd(&ctr[1], 1u);
    if (d == gridDim.x - 1) { atomicExch(&ctr[0], 0u); atomicExch(&ctr[1], 0u); }
}

}  // namespace pf
