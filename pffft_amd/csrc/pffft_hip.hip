// libpffft_hip.so, the core translation unit: the lazy device state of a setup (tables, counter ring), the launchers of the LDS-resident
// families - N = 1024 float, register-tiled, tiny, Stockham - and transform_batch, which runs the route the planner (plan_tu.hip) chose.
// The ABI is declared in include/pffft_hip.h (abi_tu.hip); the beyond-LDS passes are big_tu.hip, the spectral helpers aux_tu.hip.
// There is NO CPU arithmetic path here: every transform runs as a HIP kernel on gfx950.
#include <hip/hip_runtime.h>

#include <cmath>
#include <map>
#include <mutex>
#include <utility>

#include "../../include/pffft_hip.h"
#include "pf_host.h"
#include "pf_launch.h"
#include "fft_c1024.h"
#include "fft_tiled.h"
#include "fft_stock.h"
#include "stock_ct.h"
#include "fft_tiny.h"
#include "pfdsp_mix.h"

namespace pf {

// The device state of an object lives on ONE device; for_device() hands every entry the object of the calling thread's device, so a
// mismatch here means the caller switched devices between resolving and launching (or handed a replica around): an error, not a fault
// inside a kernel.
static int check_device(Setup* s) {
    int key = -1;
    int rc = current_device_key(&key);
    if (rc) return rc;
    int bound = s->device.load();
    if (bound < 0) { s->device.store(key); bound = key; }
    if (bound != key) {
        char buf[160];
        snprintf(buf, sizeof buf, "pffft_hip: setup state is bound to device %d but the calling thread's current device is %d",
                 bound, key);
        g_last_error = buf;
        return (int)hipErrorInvalidDevice;
    }
    return 0;
}

static int alloc_counter_ring(Setup* s) {
    // Each launch of a dynamic kernel takes its own {next, done} counter pair from this ring; the
    // kernel re-arms the pair when its last workgroup retires.  A pair is reused only CTR_RING
    // launches later, i.e. at most CTR_RING launches of one setup may be in flight at once
    // (stated in include/pffft_hip.h; launches on one stream serialise, so this bounds concurrent streams x depth).
    if (s->d_ctr) return 0;
    // (+ 16 after each region: a launch may take several consecutive pairs from the last slot)
    constexpr size_t words = 2 * (size_t)CTR_RING + 16 + 2 * (size_t)CTR_CAPTURED + 16;
    int rc = s->d_ctr.grow(sizeof(unsigned) * words);
    if (rc) return rc;
    hipError_t e = hipMemset(s->d_ctr.get(), 0, sizeof(unsigned) * words);
    if (e != hipSuccess) { s->d_ctr.reset(); return fail(e, "hipMemset of the counter ring"); }   // (never a ring that was not cleared)
    return 0;
}

bool stream_capturing(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return false; }
    return cs == hipStreamCaptureStatusActive;
}

unsigned* take_counters(Setup* s, hipStream_t st, unsigned pairs) {
    unsigned* ring = s->d_ctr.as<unsigned>();
    if (stream_capturing(st)) return ring + 2 * (size_t)CTR_RING + 16 + 2 * (s->cap_slot.fetch_add(pairs) % CTR_CAPTURED);
    return ring + 2 * (s->ctr_slot.fetch_add(pairs) % CTR_RING);
}

// The lazy device state of `s`, built at its first call with hipMalloc / hipMemset / hipMemcpy - none of which may run while `st` records
// into a HIP graph: such a first call is refused before anything is allocated (the stream is asked on this branch only: a setup whose
// tables stand pays no query).
template <typename T>
int ensure_device(Setup* s, hipStream_t st) {
    std::lock_guard<std::mutex> lk(s->mu);
    if (s->dev_ready) return check_device(s);
    int rc = check_device(s);
    if (rc) return rc;
    if (stream_capturing(st))
        return bad("the tables of this setup would have to be built during graph capture: run the call once before capturing",
                   hipErrorStreamCaptureUnsupported);
    if ((rc = alloc_counter_ring(s))) return rc;   // every kernel family may take the in-order path (zconvolve on K_BIG too)
    if (s->kernel == K_BIG) {
        for (int i = 0; i < 2; ++i) {
            const int m = s->bigp[i].n;
            if (padded_image_bytes((size_t)m, sizeof(cx<T>)) > LDS_MAX) {
                g_last_error = "pffft_hip: N too large even for the four-step path in this precision";
                return (int)hipErrorInvalidValue;
            }
            if ((rc = upload_roots<T>(s->d_bigtw[i], m, m))) return rc;
        }
        if (s->one_ok) {   // single-image kernel: compact base twiddles per direction, W_N^k of the pair pass
            for (int d = 0; d < 3; ++d)
                if ((rc = upload_stock_table<T>(d < 2 ? s->d_twc[d] : s->d_one_tw2, s->one[d]))) return rc;
            if (s->transform == PFFFT_REAL && (rc = upload_roots<T>(s->d_twr, s->n / 2 + 1, 2LL * s->n))) return rc;
        }
        s->dev_ready = true;
        return 0;
    }
    const int n = s->n;
    if ((rc = upload_roots<T>(s->d_tw, n, n))) return rc;
    if (s->transform == PFFFT_REAL && (rc = upload_roots<T>(s->d_twr, n / 2 + 1, 2LL * n))) return rc;
    for (int d = 0; d < 2; ++d) {
        const StockPlan* sp = (s->sk_ok && s->sk[d].twmode == 2) ? &s->sk[d] : (s->skw_ok && s->skw[d].twmode == 2) ? &s->skw[d] : nullptr;
        if (sp && (rc = upload_stock_table<T>(s->d_twc[d], *sp))) return rc;
    }
    s->dev_ready = true;
    return 0;
}
template int ensure_device<float>(Setup*, hipStream_t);
template int ensure_device<double>(Setup*, hipStream_t);

// ------------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------------
// (both tables are per DEVICE: the attribute is a property of the function on one device, and one process may drive several)
int allow_big_lds_impl(const void* kernel, size_t bytes) {
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, size_t> done;           // largest size already granted per (device, kernel)
    int dev = 0;
    PF_CHECK(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(mu);
    const auto key = std::make_pair(dev, kernel);
    auto it = done.find(key);
    if (it != done.end() && it->second >= bytes) return 0;
    PF_CHECK(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    done[key] = bytes;
    return 0;
}

int cached_occupancy(const void* kernel, int threads, size_t lds, int* per_cu) {
    struct Key {
        int dev; const void* k; int th; size_t lds;
        bool operator<(const Key& o) const {
            return dev != o.dev ? dev < o.dev : k != o.k ? k < o.k : th != o.th ? th < o.th : lds < o.lds;
        }
    };
    static std::mutex mu;
    static std::map<Key, int> tab;
    int dev = 0;
    PF_CHECK(hipGetDevice(&dev));
    const Key key{dev, kernel, threads, lds};
    {
        std::lock_guard<std::mutex> lk(mu);
        auto it = tab.find(key);
        if (it != tab.end()) { *per_cu = it->second; return 0; }
    }
    int v = 0;
    PF_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, kernel, threads, lds));
    if (v < 1) v = 1;
    std::lock_guard<std::mutex> lk(mu);
    tab[key] = v;
    *per_cu = v;
    return 0;
}

int num_cus() {
    static int cus = 0;
    if (!cus) {
        hipDeviceProp_t prop;
        int dev = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
            cus = prop.multiProcessorCount;
        if (cus <= 0) cus = 256;
    }
    return cus;
}

template <int W>
static int launch_c1024_once(Setup* s, const float* in, float* out, size_t batch, int dir, int ordered, hipStream_t st) {
    const unsigned grid = (unsigned)((batch + W - 1) / W);
    const size_t lds = (size_t)W * C1024_WAVE_BYTES;
    const cx<float>* tw = s->d_tw.as<cx<float>>();
    return with_dir_layout(dir, ordered, [&](auto D, auto I, auto O) {
        auto k = fft_c1024_f32_once_kernel<decltype(D)::value, decltype(I)::value, decltype(O)::value, W>;
        if (int rc = allow_big_lds(k, lds)) return rc;
        hipLaunchKernelGGL(k, dim3(grid), dim3(W * 64), lds, st, in, out, (unsigned)batch, tw);
        PF_CHECK(hipGetLastError());
        return 0;
    });
}

static int launch_c1024(Setup* s, const Route& r, const float* in, float* out, size_t batch, int dir, int ordered, hipStream_t st) {
    // Short launches - up to r.oneshot resident sets of 16 wavefronts per CU - run one transform per wavefront in dispatch order
    // (fft_c1024.h once kernel; tools/r5_c1024_batch.py, us per launch, loop -> once: batch 2^10 12.5 -> 7.7, 2^11 19.3 -> 8.2, 2^12 24.1 -> 14.0,
    // 2^13 34.8 -> 27.6, 2^14 55.2 -> 50.8; from 2^15 on the loop wins: 96 against 99 us; 2- and 8-wavefront workgroups within 1 us of these).
    if (r.oneshot > 0 && batch <= (size_t)r.oneshot * C1024_ONCE_RESIDENT * (size_t)num_cus())
        return launch_c1024_once<C1024_ONCE_W>(s, in, out, batch, dir, ordered, st);
    // the persistent in-order loop: ONE 8-wavefront workgroup per CU (two per CU measured 2^12 .. 2^17 10-50 % slower, 2^18 on equal)
    const unsigned wgs_needed = (unsigned)((batch + C1024_WAVES - 1) / C1024_WAVES);
    unsigned grid = (unsigned)num_cus();
    if (grid > wgs_needed) grid = wgs_needed;
    const dim3 blk(C1024_WAVES * 64);
    const size_t lds = C1024_LDS_BYTES;
    const cx<float>* tw = s->d_tw.as<cx<float>>();
    const unsigned b = (unsigned)batch;
    unsigned* ctr = take_counters(s, st);
    return with_dir_layout(dir, ordered, [&](auto D, auto I, auto O) {
        auto k = fft_c1024_f32_dyn_kernel<decltype(D)::value, decltype(I)::value, decltype(O)::value>;
        if (int rc = allow_big_lds(k, lds)) return rc;
        hipLaunchKernelGGL(k, dim3(grid), blk, lds, st, in, out, b, tw, ctr);
        PF_CHECK(hipGetLastError());
        return 0;
    });
}

// forward transform of the frequency-shifted stream (fused mixer, fft_c1024.h C1024Mix)
static int launch_c1024_mix(Setup* s, const float* in, float* out, size_t batch, int ordered, double step_turns,
                            double phase_turns, hipStream_t st) {
    const unsigned wgs_needed = (unsigned)((batch + C1024_WAVES - 1) / C1024_WAVES);
    unsigned grid = (unsigned)num_cus();
    if (grid > wgs_needed) grid = wgs_needed;
    const dim3 blk(C1024_WAVES * 64);
    const size_t lds = C1024_LDS_BYTES;
    const cx<float>* tw = s->d_tw.as<cx<float>>();
    const unsigned b = (unsigned)batch;
    unsigned* ctr = take_counters(s, st);
    C1024Mix mix;
    step_turns -= std::rint(step_turns);
    phase_turns -= std::rint(phase_turns);
    mix.step = step_turns;
    mix.phase0 = phase_turns;
    for (int j = 1; j < 8; ++j) {
        double a = step_turns * 128.0 * j;
        a -= std::rint(a);
        mix.g[j - 1][0] = (float)std::cos(pfmix::MIX_TWO_PI * a);
        mix.g[j - 1][1] = (float)std::sin(pfmix::MIX_TWO_PI * a);
    }
    return with_flag(!ordered, [&](auto O) {
        auto k = fft_c1024_f32_mix_kernel<decltype(O)::value>;
        if (int rc = allow_big_lds(k, lds)) return rc;
        hipLaunchKernelGGL(k, dim3(grid), blk, lds, st, in, out, b, tw, ctr, mix);
        PF_CHECK(hipGetLastError());
        return 0;
    });
}

// ------------------------------------------------------------------------------------------------
// register-tiled power-of-two family (fft_tiled.h): which configuration serves (n, direction, transform, layout)
// ------------------------------------------------------------------------------------------------
template <typename T>
using TiledFn = void (*)(const T*, T*, unsigned, int, const cx<T>*, const cx<T>*, unsigned*);

template <typename T, class C>
static TiledSel tiled_sel(int dir, int real, const char* name) {
    TiledSel e;
    e.lds = C::LDS_BYTES; e.wg = C::WG_THREADS; e.t_per_wg = C::T_PER_WG; e.cfg = name;
    TiledFn<T> fn;
    if (dir == PFFFT_FORWARD) fn = real ? fft_tiled_kernel<C, FWD, 1> : fft_tiled_kernel<C, FWD, 0>;
    else fn = real ? fft_tiled_kernel<C, BWD, 1> : fft_tiled_kernel<C, BWD, 0>;
    e.fn = reinterpret_cast<const void*>(fn);
    return e;
}
#define PF_TSEL(C) tiled_sel<T, C>(dir, real, #C)
#define PF_TSELP(C) tiled_sel<T, typename TiledPick<T>::C>(dir, real, "TiledPick::" #C)

// A measured table.  Constraint: both layouts of a direction share one configuration wherever the configurations differ in their twiddle
// arithmetic, because pffft_transform_ordered == pffft_zreorder(pffft_transform) holds bit for bit (benchmarks/bench_pffft.c:343-349).
template <typename T>
static bool tiled_pick(int n, int dir, int real, int ordered, TiledSel* e) {
    const bool fwd = dir == PFFFT_FORWARD;
    if constexpr (sizeof(T) == 4) {
        // round 3, after the packed-arithmetic change (tools/route_ab.py, 1 GiB per launch, sum of both layouts of a direction):
        //   n = 8192: real forward (C3) three-stage T8192np 0.657 / 0.706; complex forward runs the Stockham plan (0.70 / 0.76 against
        //             0.68 / 0.68), complex backward the four-stage TiledPick (0.77 / 0.71 against 0.70 / 0.70)
        //   n = 4096: forward three-stage (complex 0.72 / 0.73 against 0.69 / 0.71; real N = 8192 0.66 / 0.71 against 0.59 / 0.66), backward
        //             the four-stage TiledPick (complex 0.79 / 0.74 against 0.73 / 0.73; real 0.70 / 0.71 against 0.71 / 0.66)
        //   n = 2048: complex forward three-stage, one wavefront per transform (0.76 / 0.76 against 0.75 / 0.74); complex backward and real
        //             (N = 4096) the four-stage TiledPick (0.81 / 0.76 against 0.75 / 0.76)
        //   n = 16384: 512 threads x 32 points with the register prefetch (tools/c16k_quick.py, 1024-thread configuration -> this one):
        //             complex fwd canonical 0.66 -> 0.69, bwd 0.63 / 0.67 -> 0.68 / 0.70, real N = 32768 bwd 0.52 / 0.59 -> 0.54 / 0.64; real
        //             forward spills into the internal layout (0.55 -> 0.45) and stays on TiledPick
        if (n == 8192 && real && fwd) { *e = PF_TSEL(TiledAltF32b::T8192np); return true; }
        if (n == 2048 && !real && fwd) { *e = PF_TSEL(TiledAltF32b::T2048); return true; }
        if (n == 4096 && fwd) {
            *e = (!real && ordered) ? PF_TSEL(TiledAltF32b::T4096) : PF_TSEL(TiledAltF32b::T4096np);
            return true;
        }
        if (n == 16384 && (!real || !fwd)) { *e = PF_TSEL(TiledAltF32b::T16384); return true; }
    }
    if constexpr (sizeof(T) == 8) {
        // alt: 0 = TiledPick, 1 = A (register base twiddles), 3 = C (A + prefetch); fft_tiled.h TiledAltF64.  tools/c5_ab.py on MI355X;
        // 2048 / 4096: these beat the Stockham kernel that had taken double >= 2048 over (0.65-0.73 -> 0.70-0.80)
        int alt = 0;
        if (n == 1024) alt = (real && fwd) ? 1 : 3;
        else if (n == 512) alt = (real && fwd && !ordered) ? 1 : 3;
        else if (n == 256) alt = !real ? (fwd ? 1 : 3) : (fwd ? 0 : 3);
        else if (n == 128) alt = (real && !fwd) ? 3 : 0;
        else if (n == 2048) alt = (real && fwd && !ordered) ? 1 : 3;
        else if (n == 4096) alt = !real ? ((!fwd && ordered) ? 1 : 3) : ((fwd && !ordered) ? 1 : 3);
#define PF_ALT64(N)                                                                   \
        case N:                                                                       \
            if (alt == 1) { *e = PF_TSEL(TiledAltF64::A##N); return true; }           \
            if (alt == 3) { *e = PF_TSEL(TiledAltF64::C##N); return true; }           \
            break;
        switch (n) { PF_ALT64(128) PF_ALT64(256) PF_ALT64(512) PF_ALT64(1024) PF_ALT64(2048) PF_ALT64(4096) }
#undef PF_ALT64
    }
    switch (n) {
        case 16: *e = PF_TSELP(C16); return true;
        case 32: *e = PF_TSELP(C32); return true;
        case 64: *e = PF_TSELP(C64); return true;
        case 128: *e = PF_TSELP(C128); return true;
        case 256: *e = PF_TSELP(C256); return true;
        case 512: *e = PF_TSELP(C512); return true;
        case 1024: *e = PF_TSELP(C1024); return true;
        case 2048: *e = PF_TSELP(C2048); return true;
        case 4096: *e = PF_TSELP(C4096); return true;
        case 8192: *e = PF_TSELP(C8192); return true;
        case 16384: *e = PF_TSELP(C16384); return true;
    }
    return false;
}
#undef PF_TSEL
#undef PF_TSELP

// the planner's door to the table (plan_tu.hip instantiates no kernel): the configuration and its kernel address, erased over the scalar type
bool tiled_pick_any(bool is_double, int n, int dir, int real, int ordered, TiledSel* e) {
    return is_double ? tiled_pick<double>(n, dir, real, ordered, e) : tiled_pick<float>(n, dir, real, ordered, e);
}

template <typename T>
static int launch_tiled(Setup* s, const Route& r, const T* in, T* out, size_t batch, int dir, int ordered, hipStream_t st) {
    const TiledSel& e = r.tiled;
    TiledFn<T> fn = reinterpret_cast<TiledFn<T>>(const_cast<void*>(e.fn));
    // LR_INORDER: launches of up to r.oneshot groups per resident workgroup run as ONE group per workgroup in hardware dispatch order instead of
    // the persistent in-order loop (pf_launch.h), which pays for itself only over a long run of groups (tools/r4_small_batch.py, us per call, loop ->
    // dispatch order: C3's kernel at 64 / 128 MiB of vectors 46 / 72 -> 30 / 60, N = 4096 complex 44 / 69 -> 24 / 49, N = 256 at 32 MiB 25 -> 14,
    // N = 1024 double at 64 MiB 34 -> 27; from 8 groups per workgroup on the loop wins: N = 1024 double at 256 MiB 98 against 110)
    LoopLaunch ll;
    if (int rc = loop_launch(s, st, fn, e.wg, e.lds, (batch + e.t_per_wg - 1) / e.t_per_wg, r.oneshot, &ll)) return rc;
    hipLaunchKernelGGL(fn, dim3(ll.grid), dim3(e.wg), e.lds, st, in, out, (unsigned)batch, layout_flags(dir, ordered, false) & 3,
                       s->d_tw.as<cx<T>>(), s->d_twr.as<cx<T>>(), ll.ctr);
    PF_CHECK(hipGetLastError());
    return 0;
}

template <typename T>
static int launch_stock(Setup* s, const Route& r, const T* in, T* out, size_t batch, int dir, hipStream_t st) {
    const StockSel& k = r.stock;
    const bool bwd = dir == PFFFT_BACKWARD;
    const StockPlan& sp = k.wl ? s->skw[bwd ? 1 : 0] : s->sk[bwd ? 1 : 0];
    const cx<T>* twp = (sp.twmode == 2 ? s->d_twc[bwd ? 1 : 0] : s->d_tw).as<cx<T>>();
    const size_t groups = (batch + sp.G - 1) / sp.G;
    const bool dyn = r.rule == LR_INORDER;
    // in-order groups are pulled in chunks of ONE group from 44 KiB per group on (double n = 3072 .. 4000 0.71-0.75 -> 0.78-0.82 against two),
    // below that of as many as keep one counter address under its ~80 M atomics/s; never so large that a workgroup sees fewer than ~8 chunks
    const size_t gbytes = (size_t)sp.G * sp.n * sizeof(cx<T>);
    auto chunk_for = [&](size_t grid) -> unsigned {
        size_t kk = (44000 + gbytes - 1) / gbytes, cap = groups / (8 * grid);
        if (kk > cap) kk = cap;
        return (unsigned)(kk < 1 ? 1 : (kk > 64 ? 64 : kk));
    };
    if (k.fn) {
        StockCtFn<T> cf = reinterpret_cast<StockCtFn<T>>(const_cast<void*>(k.fn));
        int rc = allow_big_lds(cf, k.lds);
        if (rc) return rc;
        int per_cu = 0;
        if ((rc = cached_occupancy(k.fn, k.threads, k.lds, &per_cu))) return rc;
        size_t grid = (size_t)num_cus() * per_cu;
        if (k.groups_per_wg > 0) {
            const size_t want = (groups + (size_t)k.groups_per_wg - 1) / (size_t)k.groups_per_wg;
            if (want > grid) grid = want;                       // (never below the resident set)
        } else {
            grid *= (size_t)k.grid_mul;
        }
#ifdef PFFFT_HIP_VARIANTS
        {   // the tuner's knob (tools/tune_stock_grid.py): selectors 210 + i force SK_ITS[i] groups per workgroup, 208 the size rule alone
            static const int SK_ITS[12] = {1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64};
            const int v = ab().raw;
            if (v >= 210 && v <= 221) { grid = (size_t)num_cus() * per_cu; const size_t want = (groups + SK_ITS[v - 210] - 1) / SK_ITS[v - 210]; if (want > grid) grid = want; }
            if (v == 208) grid = (size_t)num_cus() * per_cu * (size_t)k.grid_mul;
        }
#endif
        if (dyn && r.oneshot > 0 && groups <= (size_t)r.oneshot * grid) grid = groups;   // (n = 8192 complex float at 32 MiB of vectors 25 -> 16 us)
        if (grid > groups) grid = groups;
        if (grid > 0x7fffffffu) grid = 0x7fffffffu;
        unsigned* ctr = (groups <= grid || !dyn) ? nullptr : take_counters(s, st);
        hipLaunchKernelGGL(cf, dim3((unsigned)grid), dim3(k.threads), k.lds, st, in, out, batch, twp, s->d_twr.as<cx<T>>(), ctr, chunk_for(grid));
        PF_CHECK(hipGetLastError());
        return 0;
    }
#ifdef PFFFT_HIP_VARIANTS
    // the same bodies on the run-time plan (0.3 of the roofline: issue-bound).  Every legal size has a compile-time plan
    // (tests/test_generated_sources.py), so the product build does not carry these kernels (2 MB); AB_STOCK_RUNTIME forces them here.
    auto kf = k.wl ? fft_stock_wl_kernel<T> : fft_stock_kernel<T>;
    size_t resident = 0;
    if (int rc = loop_resident(kf, k.threads, k.lds, &resident)) return rc;
    const LoopGrid g = loop_grid(resident, groups, 0);
    unsigned* ctr = (g.needs_counters && dyn) ? take_counters(s, st) : nullptr;   // (the static stride reads no counter)
    hipLaunchKernelGGL(kf, dim3((unsigned)g.grid), dim3(k.threads), k.lds, st, in, out, batch, sp, k.flags, twp, s->d_twr.as<cx<T>>(), ctr, chunk_for(g.grid));
    PF_CHECK(hipGetLastError());
    return 0;
#else
    (void)twp; (void)chunk_for;
    g_last_error = "pffft_hip: no compile-time Stockham plan for this size (product build)";
    return (int)hipErrorInvalidValue;
#endif
}

// n = 16 / 32: one thread per transform (fft_tiny.h)
template <typename T, int n>
static int launch_tiny(Setup* s, const T* in, T* out, size_t batch, int dir, int ordered, hipStream_t st) {
    constexpr int CPV = 2 * n * (int)sizeof(T) / 16;
    const int waves = CPV >= 32 ? 2 : 4;
    const size_t lds = (size_t)waves * 64 * (CPV + 1) * 16;
    const size_t groups = (batch + 63) / 64;
    size_t grid = (groups + waves - 1) / waves;
    // (one group of 64 vectors per wavefront in hardware dispatch order: plan_route has the measurement)
    const bool real = s->transform == PFFFT_REAL;
    const cx<T>* twr = s->d_twr.as<cx<T>>();
    return with_dir_layout(dir, ordered, [&](auto D, auto I, auto O) {
        return with_flag(real, [&](auto R) {
            auto k = fft_tiny_kernel<T, n, decltype(D)::value, decltype(R)::value, decltype(I)::value, decltype(O)::value>;
            if (int rc = allow_big_lds(k, lds)) return rc;
            hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(waves * 64), lds, st, in, out, batch, twr);
            PF_CHECK(hipGetLastError());
            return 0;
        });
    });
}

template <typename T>
int transform_batch(Setup* s, const T* in, T* out, size_t batch, int dir, int ordered, hipStream_t st) {
    if (int rc = check_setup<T>(s)) return rc;
    if ((dir != PFFFT_FORWARD && dir != PFFFT_BACKWARD)) { g_last_error = "pffft_hip: bad direction"; return (int)hipErrorInvalidValue; }
    if (batch == 0) return 0;
    s = for_device(s);        // the object that holds this setup's tables on the calling thread's device
    int rc = ensure_device<T>(s, st);
    if (rc) return rc;
    const AbSel sel = ab();
    Route tmp;
    const Route* r = &s->route[dir][ordered ? 1 : 0];
    if (sel.any()) { tmp = plan_route(s, dir, ordered ? 1 : 0, sel); r = &tmp; }
    switch (r->fam) {
        case FAM_TINY:
            if (s->n == 16) return launch_tiny<T, 16>(s, in, out, batch, dir, ordered, st);
            if constexpr (sizeof(T) == 4) return launch_tiny<T, 32>(s, in, out, batch, dir, ordered, st);
            break;
        case FAM_C1024:
        case FAM_TILED: {
            // (these kernels count vectors in 32 bits: longer batches go out in slices on the same stream)
            constexpr size_t SLICE = (size_t)3 << 30;
            for (size_t b0 = 0; b0 < batch; b0 += SLICE) {
                const size_t nb = batch - b0 < SLICE ? batch - b0 : SLICE;
                const T* pi = in + b0 * s->vec_scalars;
                T* po = out + b0 * s->vec_scalars;
                if constexpr (sizeof(T) == 4) {
                    if (r->fam == FAM_C1024) { if ((rc = launch_c1024(s, *r, pi, po, nb, dir, ordered, st))) return rc; continue; }
                }
                if ((rc = launch_tiled<T>(s, *r, pi, po, nb, dir, ordered, st))) return rc;
            }
            return 0;
        }
        case FAM_STOCK: return launch_stock<T>(s, *r, in, out, batch, dir, st);
        case FAM_BIG: return launch_big(s, *r, in, out, batch, dir, ordered, st);
        case FAM_ONE: return launch_one(s, in, out, batch, dir, ordered ? 1 : 0, st);
        default: break;
    }
    g_last_error = "pffft_hip: no kernel for this size";
    return (int)hipErrorInvalidValue;
}

template int transform_batch<float>(Setup*, const float*, float*, size_t, int, int, hipStream_t);
template int transform_batch<double>(Setup*, const double*, double*, size_t, int, int, hipStream_t);

// frames_tu.hip: the batched transform and the lazy device state behind type-erased pointers
int transform_batch_any(Setup* s, const void* in, void* out, size_t batch, int dir, int ordered, hipStream_t st) {
    if (s->is_double) return transform_batch<double>(s, (const double*)in, (double*)out, batch, dir, ordered, st);
    return transform_batch<float>(s, (const float*)in, (float*)out, batch, dir, ordered, st);
}
int ensure_device_any(Setup* s, hipStream_t st) { return s->is_double ? ensure_device<double>(s, st) : ensure_device<float>(s, st); }

// frequency shift (src/pf_mixer.cpp) immediately followed by the forward FFT, the usual SDR
// chain.  The batch is ONE stream of batch*N complex samples, sample g gets exp(j (phase_rad + 2 pi rate g)).
// N = 1024: fused into the load stage of the headline kernel (one pass over HBM); other sizes: mixer kernel
// into `out`, then the transform in place (two passes).
int shift_transform_batch(Setup* s, const float* in, float* out, size_t batch, int ordered, double rate,
                                 double phase_rad, hipStream_t st) {
    if (!s || s->magic != MAGIC || s->is_double || s->transform != PFFFT_COMPLEX) {
        g_last_error = "pffft_hip: shift_transform_batch needs a complex single-precision setup";
        return (int)hipErrorInvalidHandle;
    }
    if (batch == 0) return 0;
    s = for_device(s);
    int rc = ensure_device<float>(s, st);
    if (rc) return rc;
    const double phase_turns = phase_rad / pfmix::MIX_TWO_PI;
    if (s->kernel == K_C1024_F32 && !ab().is(AB_AUX_DIRECT) && batch < (1ull << 32))   // AB_AUX_DIRECT: the two-pass composition (second route of the tests)
        return launch_c1024_mix(s, in, out, batch, ordered, rate, phase_turns, st);
    const double S[1][2] = {{std::cos(phase_rad), std::sin(phase_rad)}};
    rc = pfmix::launch_mix(reinterpret_cast<const float2*>(in), reinterpret_cast<float2*>(out), batch * (size_t)s->N, 1, S,
                           rate, false, st);
    if (rc) { g_last_error = pfmix::last_error; return rc; }
    return transform_batch<float>(s, out, out, batch, PFFFT_FORWARD, ordered, st);
}

}  // namespace pf

// resident workgroups per CU of the LDS-resident kernel a (direction, layout) runs on, as the launcher sees it (the occupancy query of
// the runtime for the route's kernel, threads and LDS bytes); 0 where the route has no single persistent kernel.  Needs a device.
PF_EXPORT int pffft_hip_route_occupancy(const void* setup, int dir, int ordered) {
    const pf::Setup* s = static_cast<const pf::Setup*>(setup);
    if (!s || s->magic != pf::MAGIC || dir < 0 || dir > 1) return -1;
    const pf::Route& r = s->route[dir][ordered ? 1 : 0];
    int per_cu = 0;
    if (r.fam == pf::FAM_TILED) { if (pf::allow_big_lds_impl(r.tiled.fn, r.tiled.lds) || pf::cached_occupancy(r.tiled.fn, r.tiled.wg, r.tiled.lds, &per_cu)) return -1; }
    else if (r.fam == pf::FAM_STOCK && r.stock.fn) { if (pf::allow_big_lds_impl(r.stock.fn, r.stock.lds) || pf::cached_occupancy(r.stock.fn, r.stock.threads, r.stock.lds, &per_cu)) return -1; }
    else if (r.fam == pf::FAM_ONE) {
        const bool real = s->transform == PFFFT_REAL;
        const int flags = pf::layout_flags(dir, ordered, real);
        const void* fn = pf::one_kernel_ptr(s->is_double != 0, flags);
        const int pi = pf::one_plan_index(s->is_double != 0, flags);
        const size_t lds = pf::one_lds_bytes(s->one[pi], s->is_double != 0, real);
        if (pf::allow_big_lds_impl(fn, lds) || pf::cached_occupancy(fn, s->one[pi].C, lds, &per_cu)) return -1;
    }
    return per_cu;
}
