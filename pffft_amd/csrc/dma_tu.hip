// libpffft_hip.so, translation unit of the FIR block kernels on long blocks: LDS-DMA staged (fft_dma.h), split (fft_split.h), 32 points per
// thread (fft_fir32.h) - instantiations + launchers.  Each takes one FirCall (pf_host.h) on the blocks fir_route chose (fastconv_tu.hip).
#include <hip/hip_runtime.h>

#include "../../include/pffft_hip.h"
#include "pf_launch.h"
#include "fft_dma.h"
#include "fft_split.h"
#include "fft_fir32.h"
#include <utility>

namespace pf {

template <class C>
static int fir_dma_cfg(Setup* ps, const float* d_Hc, const FirCall& c) {
    ps = for_device(ps);
    typedef DmaGeom<C> G;
    auto k = fastconv_dma_kernel<C>;
    if (int rc = allow_big_lds(k, G::LDS_BYTES)) return rc;
    const size_t groups = ((size_t)c.nblk * c.fb.nsig + C::T_PER_WG - 1) / C::T_PER_WG;
    const LoopLaunch ll = loop_take(ps, c.st, (size_t)num_cus(), groups, 0);   // (one workgroup per CU)
    hipLaunchKernelGGL(k, dim3(ll.grid), dim3(C::WG_THREADS), G::LDS_BYTES, c.st, c.x, c.y, (const cx<float>*)d_Hc,
                       c.nblk, c.step, c.inputLen, c.lastOut, ps->d_tw.as<cx<float>>(), ps->d_twr.as<cx<float>>(), ll.ctr,
                       c.fb.nsig, c.fb.xstride, c.fb.ystride);
    PF_CHECK(hipGetLastError());
    return 0;
}

// what fc_refuse_capture (fastconv_tu.hip) says, for the tables the launchers here build on first use
static int refuse_capture(const char* what) {
    return bad((std::string("pffastconv: ") + what + " would have to be built during graph capture: run a call of this shape once before "
                "capturing").c_str(), hipErrorStreamCaptureUnsupported);
}

// W_m^j (m = 1024, 512) for the wave-local sub-transforms of the split kernels: one table per device and length, uploaded at the first
// call of the PROCESS that needs it (whatever setup it belongs to) - not while `st` records into a HIP graph
static int split_sub_table(const cx<float>** out, hipStream_t st, int m = 1024) {
    static std::mutex mu;
    static std::map<long long, cx<float>*> tabs;
    int dev = 0;
    PF_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    const long long key = (long long)dev * 65536 + m;
    auto it = tabs.find(key);
    if (it == tabs.end()) {
        if (stream_capturing(st)) return refuse_capture("the process-wide sub-transform table of the split kernels");
        const std::vector<cx<float>> tw = unit_roots<float>(m, m);
        cx<float>* d = nullptr;   // (cached for the life of the process, never freed: no owner with static storage, pf_devmem.h)
        PF_CHECK(hipMalloc((void**)&d, sizeof(cx<float>) * m));
        PF_CHECK(hipMemcpy(d, tw.data(), sizeof(cx<float>) * m, hipMemcpyHostToDevice));
        it = tabs.emplace(key, d).first;
    }
    *out = it->second;
    return 0;
}

// A per-filter coefficient table of a block kernel (`floats` floats out of the canonical spectrum d_Hc by `coef_kernel` on `wg` threads):
// built ONCE and COMPLETE before the pointer is published - null stream + synchronisation, like every other lazily built table
// (fc_spectrum, split_sub_table).  Built on the caller's stream (round 4) a second call on another non-blocking stream saw the pointer set
// and could read a half-written table: the setup's mutex orders hosts, not streams.  `st`, the call's stream, is only asked whether it
// records into a HIP graph: a missing table is then refused, named by `what`.
template <class K>
static int fir_coef_table(DevBuf& cache, K coef_kernel, const char* name, const char* what, int wg, size_t floats, Setup* ps, const float* d_Hc,
                          hipStream_t st) {
    if (cache) return 0;
    if (stream_capturing(st)) return refuse_capture(what);
    DevBuf t;
    if (int rc = t.grow(sizeof(float) * floats)) return rc;
    hipLaunchKernelGGL(coef_kernel, dim3(1), dim3(wg), 0, nullptr, (const cx<float>*)d_Hc, ps->d_twr.as<cx<float>>(), t.as<vec4<float>>());
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) return fail(e, name);
    cache = std::move(t);
    return 0;
}

template <int W>
static int fir_split1(Setup* ps, const float* d_Hc, const FirCall& c, DevBuf& ab_cache) {
    typedef SplitOneT<W> S;
    ps = for_device(ps);
    auto k = fastconv_split1_kernel<W>;
    const cx<float>* tw512 = nullptr;
    int rc = split_sub_table(&tw512, c.st, S::M);
    if (rc) return rc;
    if ((rc = fir_coef_table(ab_cache, fastconv_split1_coef_kernel<W>, "fastconv_split1_coef_kernel", "the split1 coefficient table of this setup",
                             S::WG, 4 * (size_t)S::n, ps, d_Hc, c.st)))
        return rc;
    size_t resident = 0;
    if ((rc = loop_resident(k, S::WG, S::LDS_BYTES, &resident))) return rc;
    const size_t grid = loop_grid(resident, (size_t)c.nblk * c.fb.nsig, 0).grid;   // (a static stride: no counters)
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(S::WG), S::LDS_BYTES, c.st, c.x, c.y, ab_cache.as<vec4<float>>(), c.nblk, c.step, c.inputLen,
                       c.lastOut, ps->d_tw.as<cx<float>>(), tw512, c.fb.nsig, c.fb.xstride, c.fb.ystride, env().fir_xcd);
    PF_CHECK(hipGetLastError());
    return 0;
}

// calls with few blocks on reference-sized blocks of 2 ps->n samples: W wavefronts x 512-point wave-local transforms (fft_split.h)
int launch_fir_split1(Setup* ps, const float* d_Hc, const FirCall& c, DevBuf& ab_cache) {
    switch (ps->n) {
        case 4096: return fir_split1<8>(ps, d_Hc, c, ab_cache);
        case 2048: return fir_split1<4>(ps, d_Hc, c, ab_cache);
        default: return bad("launch_fir_split1: blocks of 8192 or 4096 samples only");
    }
}

// workgroups and counters of a launch over `groups` blocks of a kernel that hands out per-XCD ranges (fft_split.h, fft_fir32.h xmode): the
// ranges of the in-order case are pulled by the workgroups of that XCD only, so every XCD needs one
struct XcdLaunch { unsigned grid; int xmode; unsigned* ctr; };
static XcdLaunch xcd_take(Setup* ps, hipStream_t st, size_t resident, size_t groups) {
    const LoopGrid g = loop_grid(resident, groups, 0);
    const int xmode = (env().fir_xcd && g.grid >= 8 && groups < 0xfffffff0ull) ? 1 : 0;
    return {(unsigned)g.grid, xmode, g.needs_counters ? take_counters(ps, st, xmode ? 5 : 1) : nullptr};   // (per-XCD counters: nine words)
}

template <int PSYNC, int SPREAD, int W = 8>
static int fir_split(Setup* ps, const float* d_Hc, const FirCall& c) {
    typedef SplitFirT<W> S;
    ps = for_device(ps);
    auto k = fastconv_split_kernel<PSYNC, SPREAD, W>;
    const cx<float>* tw1024 = nullptr;
    size_t resident = 0;
    int rc = split_sub_table(&tw1024, c.st);
    if (!rc) rc = loop_resident(k, S::WG, S::LDS_BYTES, &resident);
    if (rc) return rc;
    const XcdLaunch l = xcd_take(ps, c.st, resident, (size_t)c.nblk * c.fb.nsig);
    hipLaunchKernelGGL(k, dim3(l.grid), dim3(S::WG), S::LDS_BYTES, c.st, c.x, c.y, (const cx<float>*)d_Hc,
                       c.nblk, c.step, c.inputLen, c.lastOut, ps->d_tw.as<cx<float>>(), tw1024, ps->d_twr.as<cx<float>>(), l.ctr,
                       c.fb.nsig, c.fb.xstride, c.fb.ystride, l.xmode);
    PF_CHECK(hipGetLastError());
    return 0;
}

// 16384-sample blocks: cross-wave radix 8 + wave-local 1024-point transforms (fft_split.h).  plain (development build): without the
// pairwise flags and the spread pieces
int launch_fir_split(Setup* ps, const float* d_Hc, const FirCall& c, bool plain) {
    if (ps->n != 8192) return bad("launch_fir_split: blocks of 16384 samples only");
#ifdef PFFFT_HIP_VARIANTS
    if (plain) return fir_split<0, 0>(ps, d_Hc, c);
#endif
    return plain ? bad("launch_fir_split: the plain form is a development-build kernel") : fir_split<1, 1>(ps, d_Hc, c);
}

// 16384-sample blocks on 256 threads, 32 points per thread (fft_fir32.h).  hp_cache: the thread-major copy of the filter spectrum, built
// once per filter (fir_coef_table)
template <int PREF>
static int fir32(Setup* ps, const float* d_Hc, const FirCall& c, DevBuf& hp_cache) {
    ps = for_device(ps);
    auto k = fastconv_fused32_kernel<PREF>;
    int rc = fir_coef_table(hp_cache, fir32_coef_kernel, "fir32_coef_kernel", "the fir32 coefficient table of this setup", Fir32::WG,
                            4 * (size_t)Fir32::n, ps, d_Hc, c.st);
    if (rc) return rc;
    size_t resident = 0;
    if ((rc = loop_resident(k, Fir32::WG, Fir32::LDS_BYTES, &resident))) return rc;
    const XcdLaunch l = xcd_take(ps, c.st, resident, (size_t)c.nblk * c.fb.nsig);
    hipLaunchKernelGGL(k, dim3(l.grid), dim3(Fir32::WG), Fir32::LDS_BYTES, c.st, c.x, c.y, hp_cache.as<vec4<float>>(),
                       c.nblk, c.step, c.inputLen, c.lastOut, ps->d_tw.as<cx<float>>(), ps->d_twr.as<cx<float>>(), l.ctr,
                       c.fb.nsig, c.fb.xstride, c.fb.ystride, l.xmode);
    PF_CHECK(hipGetLastError());
    return 0;
}
// pref: the next block's samples are requested 2 = in four pieces between the phases of the inverse transform; development build: 1 = at once after the product, 0 = after the output stores
int launch_fir32(Setup* ps, const float* d_Hc, const FirCall& c, DevBuf& hp_cache, int pref) {
    if (ps->n != Fir32::n) return bad("launch_fir32: blocks of 16384 samples only");
#ifdef PFFFT_HIP_VARIANTS
    if (pref == 1) return fir32<1>(ps, d_Hc, c, hp_cache);
    if (pref == 0) return fir32<0>(ps, d_Hc, c, hp_cache);
#endif
    return pref == 2 ? fir32<2>(ps, d_Hc, c, hp_cache) : bad("launch_fir32: this prefetch form is a development-build kernel");
}

// The lock-step overlap-save block kernel.  fir_route names it for 16384-sample blocks in the development build (AB_FIR_LOCKSTEP: the kernel the
// split one replaced); the shorter ones tied with the register-staged fused kernel (tools/dma_ab.py) and stay part of the library's device code.
int launch_fir_dma(Setup* ps, const float* d_Hc, const FirCall& c) {
    switch (ps->n) {
        case 2048: return fir_dma_cfg<DmaCfgF32::D2048>(ps, d_Hc, c);
        case 4096:
            // (the split kernel on FOUR wavefronts and 8192-sample blocks, two workgroups per CU - fft_split.h W = 4, tools/dma_timeline.hip -
            //  moves 6 % more samples per CU and second than the eight-wavefront one: not enough to pay for 75 % instead of 87 % overlap-save
            //  efficiency at 2048 taps (0.394 against 0.428); not instantiated here)
            return fir_dma_cfg<DmaCfgF32::D4096>(ps, d_Hc, c);
#ifdef PFFFT_HIP_VARIANTS
        case 8192: return fir_dma_cfg<DmaCfgF32::D8192>(ps, d_Hc, c);
#endif
        default: return bad("launch_fir_dma: no LDS-DMA block kernel for this block length in this build");
    }
}

}  // namespace pf
