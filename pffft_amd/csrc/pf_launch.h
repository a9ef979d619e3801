// The one host launch path of the persistent ("loop") kernels: resident workgroups pull groups of vectors in order from a {next, done}
// counter pair, and short launches run one group per workgroup in hardware dispatch order instead.  Every launcher of such a kernel
// takes its grid and its counters from here and keeps only its own typed hipLaunchKernelGGL line, or leaves that to loop_launch_last too.  The tile passes, launch_one, the
// N = 1024 launchers, the compile-time path of launch_stock and the zreorder / zconvolve launches follow other rules and stay on their own.
// Also here: the dispatchers from run-time (direction, layout) flags to the template arguments of a kernel.
#pragma once
#include <type_traits>

#include "pf_host.h"

namespace pf {

// The launch rule of the convolution kernel, followed by conv_tu.hip and bluestein_host.h (fft_conv_kernel), xcorr_tu.hip (fft_xcorr_kernel)
// and fft2d_host.h (fft_fft2_kernel, fft_rfft2_kernel): a constant, NOT env().oneshot - PFFFT_HIP_ONESHOT does not move these launches
// (tests/launch_shapes.py fused_long_batch mirrors it)
constexpr int CONV_ONESHOT = 4;

struct LoopGrid { size_t grid; bool needs_counters; };

// The rule, on plain integers.  resident: workgroups the device holds at once; groups: units of work; oneshot: launches of up to this
// many groups per resident workgroup run ONE group per workgroup (0 = never).  Counters are needed only where a workgroup loops.
constexpr LoopGrid loop_grid(size_t resident, size_t groups, int oneshot) {
    size_t grid = resident;
    if (oneshot > 0 && groups <= (size_t)oneshot * resident && groups < 0x7fffffffull) grid = groups;
    if (grid > groups) grid = groups;
    return {grid, groups > grid};
}
static_assert(loop_grid(512, 2048, 4).grid == 2048 && !loop_grid(512, 2048, 4).needs_counters, "four groups per workgroup: dispatch order");
static_assert(loop_grid(512, 2049, 4).grid == 512 && loop_grid(512, 2049, 4).needs_counters, "one more: the loop");
static_assert(loop_grid(512, 100, 0).grid == 100 && !loop_grid(512, 100, 0).needs_counters, "never above the groups");
static_assert(loop_grid(512, 512, 0).grid == 512 && !loop_grid(512, 512, 0).needs_counters, "one pass of the resident set: no counters");
static_assert(loop_grid(512, 513, 0).grid == 512 && loop_grid(512, 513, 0).needs_counters, "the loop without a dispatch-order bound");
static_assert(loop_grid(512, 3, 4).grid == 3 && !loop_grid(512, 3, 4).needs_counters, "fewer groups than workgroups");

// workgroups of `kernel` the device holds at once (LDS opt-in, then CUs x the cached occupancy)
template <typename K>
static int loop_resident(K kernel, int threads, size_t lds, size_t* resident) {
    int rc = allow_big_lds(kernel, lds);
    if (rc) return rc;
    int per_cu = 0;
    if ((rc = cached_occupancy(reinterpret_cast<const void*>(kernel), threads, lds, &per_cu))) return rc;
    *resident = (size_t)num_cus() * per_cu;
    return 0;
}

struct LoopLaunch { unsigned grid = 0; unsigned* ctr = nullptr; };

// grid and counters of one launch on a known resident set (a site with a fixed one - one workgroup per CU - passes it).  A site whose
// number of counter pairs depends on the grid calls loop_grid and take_counters itself.
inline LoopLaunch loop_take(Setup* s, hipStream_t st, size_t resident, size_t groups, int oneshot) {
    const LoopGrid g = loop_grid(resident, groups, oneshot);
    return {(unsigned)g.grid, g.needs_counters ? take_counters(s, st) : nullptr};
}

template <typename K>
static int loop_launch(Setup* s, hipStream_t st, K kernel, int threads, size_t lds, size_t groups, int oneshot, LoopLaunch* ll) {
    size_t resident = 0;
    if (int rc = loop_resident(kernel, threads, lds, &resident)) return rc;
    *ll = loop_take(s, st, resident, groups, oneshot);
    return 0;
}

// ... and the launch itself, for a kernel whose counter pointer is its LAST parameter: `args` are the parameters before it.  A site whose
// counters sit elsewhere, or that asks loop_resident once for several slices, keeps its own hipLaunchKernelGGL line.
template <typename K, typename... Args>
static int loop_launch_last(Setup* s, hipStream_t st, K kernel, int threads, size_t lds, size_t groups, int oneshot, const Args&... args) {
    LoopLaunch ll;
    if (int rc = loop_launch(s, st, kernel, threads, lds, groups, oneshot, &ll)) return rc;
    hipLaunchKernelGGL(kernel, dim3(ll.grid), dim3(threads), lds, st, args..., ll.ctr);
    PF_CHECK(hipGetLastError());
    return 0;
}

// (direction, layout) -> the <DIR, IN_INTERNAL, OUT_INTERNAL> template triple of the kernels that read or write the internal layout
// themselves (fft_c1024.h, fft_tiny.h).  `f` is a generic lambda called with three std::integral_constant<int, .>; exactly these four
// triples exist as kernels: the forward transform never reads the layout, the backward one never writes it.
template <class F>
static int with_dir_layout(int dir, int ordered, F&& f) {
    typedef std::integral_constant<int, 0> No;
    typedef std::integral_constant<int, 1> Yes;
    if (dir == FWD) return ordered ? f(std::integral_constant<int, FWD>{}, No{}, No{}) : f(std::integral_constant<int, FWD>{}, No{}, Yes{});
    return ordered ? f(std::integral_constant<int, BWD>{}, No{}, No{}) : f(std::integral_constant<int, BWD>{}, Yes{}, No{});
}
// the two-way sibling: a run-time flag as a template argument
template <class F>
static int with_flag(bool on, F&& f) {
    return on ? f(std::integral_constant<int, 1>{}) : f(std::integral_constant<int, 0>{});
}
// the three-way sibling: a run-time value out of {A, B, C} as a template argument (the caller has refused every other value)
template <int A, int B, int C, class F>
static auto with_one_of(int v, F&& f) {
    return v == A ? f(std::integral_constant<int, A>{}) : v == B ? f(std::integral_constant<int, B>{}) : f(std::integral_constant<int, C>{});
}

}  // namespace pf
