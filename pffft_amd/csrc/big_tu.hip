// libpffft_hip.so, translation unit of the transforms beyond LDS (fft_big.h): the balanced strided pair, the streaming passes
// n = R x N2, the one-sweep layout / pair kernels, and launch_big, which executes the BigPlan the planner (plan_tu.hip plan_big) wrote.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>

#include "../../include/pffft_hip.h"
#include "pf_host.h"
#include "pf_launch.h"
#include "fft_big.h"

namespace pf {

template <typename T>
static int launch_strided(Setup* s, int which, const cx<T>* in, cx<T>* out, size_t batch, int dir, hipStream_t st) {
    const StridedPlan& sp = s->bigp[which];
    const size_t lds = padded_image_bytes((size_t)sp.G * sp.n, sizeof(cx<T>));
    long long groups = (long long)batch * ((sp.count + sp.G - 1) / sp.G);
    long long grid = (long long)num_cus() * 4;
    if (grid > groups) grid = groups;
    const int th = strided_threads((size_t)sp.G * sp.n);
    auto kf = fft_strided_kernel<T, FWD>;
    auto kb = fft_strided_kernel<T, BWD>;
    int rc = allow_big_lds(dir == PFFFT_FORWARD ? kf : kb, lds);
    if (rc) return rc;
    hipLaunchKernelGGL(dir == PFFFT_FORWARD ? kf : kb, dim3((unsigned)grid), dim3(th), lds, st, in, out, (long long)batch, sp,
                       s->d_bigtw[which].as<cx<T>>());
    PF_CHECK(hipGetLastError());
    return 0;
}

// n = R x N2: columns in registers -> batched LDS-resident rows -> tiled transpose (fft_big.h)
template <typename T, int RR>
static int big_small_factor_r(Setup* s, const cx<T>* in, cx<T>* work, cx<T>* out, size_t batch, int dir, hipStream_t st, bool out_int, bool in_int) {
    const int N2 = s->sub->n;
    const unsigned tgrid_int = (unsigned)(batch * (size_t)((N2 / 4 + 63) / 64));
    const long long total = (long long)batch * N2;
    const unsigned grid = (unsigned)((total + 255) / 256);
    const double inv_n = 1.0 / (double)s->n;
    const unsigned tgrid = (unsigned)(batch * (size_t)((N2 + 255) / 256));
    bool col_done = false;
    if constexpr (RR % 4 == 0) {
        if (in_int) {
            auto kc = big_col_int_kernel<T, RR, BWD>;
            const size_t ldsc = (size_t)RR * 257 * sizeof(cx<T>);
            if (int rcc = allow_big_lds(kc, ldsc)) return rcc;
            hipLaunchKernelGGL(kc, dim3(tgrid), dim3(256), ldsc, st, (const T*)in, work, (long long)batch, N2, inv_n);
            col_done = true;
        }
    }
    if (!col_done) {
        if (dir == PFFFT_FORWARD) hipLaunchKernelGGL((big_col_kernel<T, RR, FWD>), dim3(grid), dim3(256), 0, st, in, work, total, N2, inv_n);
        else hipLaunchKernelGGL((big_col_kernel<T, RR, BWD>), dim3(grid), dim3(256), 0, st, in, work, total, N2, inv_n);
    }
    PF_CHECK(hipGetLastError());
    int rc = transform_batch<T>(s->sub, (const T*)work, (T*)work, batch * (size_t)RR, dir, 1, st);
    if (rc) return rc;
    const size_t lds = (size_t)256 * (RR + 1) * sizeof(cx<T>);
    if (out_int) {
        auto ki = big_transpose_int_kernel<T, RR>;
        if ((rc = allow_big_lds(ki, lds))) return rc;
        hipLaunchKernelGGL(ki, dim3(tgrid_int), dim3(256), lds, st, (const cx<T>*)work, (T*)out, (long long)batch, N2);
    } else {
        auto k = big_transpose_kernel<T, RR>;
        if ((rc = allow_big_lds(k, lds))) return rc;
        hipLaunchKernelGGL(k, dim3(tgrid), dim3(256), lds, st, (const cx<T>*)work, out, (long long)batch, N2);
    }
    PF_CHECK(hipGetLastError());
    return 0;
}

template <typename T>
static int big_small_factor(Setup* s, const cx<T>* in, cx<T>* work, cx<T>* out, size_t batch, int dir, hipStream_t st, bool out_int = false,
                            bool in_int = false) {
    // in_int (backward only, R a multiple of 4): the column pass reads the internal layout itself (big_col_int_kernel)
    // out_int (forward only): the transpose stores the internal layout itself (big_transpose_int_kernel)
#define PF_BIG_R(RR) case RR: return big_small_factor_r<T, RR>(s, in, work, out, batch, dir, st, out_int, in_int);
    switch (s->bigR) {
        PF_BIG_R(2) PF_BIG_R(3) PF_BIG_R(4) PF_BIG_R(5) PF_BIG_R(6) PF_BIG_R(8) PF_BIG_R(9) PF_BIG_R(10) PF_BIG_R(12) PF_BIG_R(15) PF_BIG_R(16)
        PF_BIG_R(25) PF_BIG_R(27) PF_BIG_R(32)
    }
#undef PF_BIG_R
    g_last_error = "pffft_hip: unsupported small factor";
    return (int)hipErrorInvalidValue;
}

// one-sweep layout / pair kernels of the beyond-LDS path (fft_big.h big_block_kernel): mode 0 complex canonical -> internal,
// 1 complex internal -> canonical, 2 real forward Z -> X (internal), 3 real backward X (internal) -> Z', 4 real backward
// X (canonical) -> Z', 5 real X (canonical) -> X (internal), a pure permutation.  in != out.
template <typename T>
static int launch_block(Setup* s, int mode, const T* in, T* out, size_t batch, hipStream_t st) {
    const long long n = s->n, tiles = (long long)batch * ((n / 4 + 63) / 64);
    long long grid = (tiles + BLK_WAVES - 1) / BLK_WAVES;
    // ONE tile per wavefront in hardware dispatch order (grid = every tile): real N = 2^18 forward unordered 0.210 -> 0.224 of the
    // roofline for the whole transform, backward 0.200-0.204 -> 0.213-0.214, against persistent wavefronts on a static stride
    // or chunks of 4 .. 32 consecutive tiles per wavefront (no better) - the order of the accesses again
    if (grid > 0x7fffffffll) grid = 0x7fffffffll;
    static constexpr void (*KERNEL[6])(const T*, T*, long long, long long, int) = {
        big_block_kernel<T, 0>, big_block_kernel<T, 1>, big_block_kernel<T, 2>, big_block_kernel<T, 3>, big_block_kernel<T, 4>, big_block_kernel<T, 5>};
    hipLaunchKernelGGL(KERNEL[mode >= 0 && mode < 5 ? mode : 5], dim3((unsigned)grid), dim3(BLK_WAVES * 64), 0, st, in, out, (long long)batch, n,
                       1 /* tiles per wavefront */);
    PF_CHECK(hipGetLastError());
    return 0;
}

template <typename T>
static int launch_big_t(Setup* s, const Route& r, const T* in, T* out, size_t batch, int dir, int ordered, hipStream_t st) {
    const BigPlan& b = r.big;
    size_t bytes = batch * (size_t)s->n * sizeof(cx<T>);
    // (the work rows of the real two-sweep route - k1 <= N1/2, whole row tiles - need a little more than n)
    if (b.core == BIG_RFFT2) bytes = std::max(bytes, batch * tile_rfft_work_elems(2LL * s->n, s->is_double != 0) * sizeof(cx<T>));
    cx<T>*bufA, *bufB;
    std::lock_guard<std::mutex> lk(s->big.mu);   // held until EVERY pass of this call is enqueued (StreamScratch)
    {
        StreamScratch::Entry& sc = s->big.acquire(st);
        for (int i = 0; i < 2; ++i)
            if (int rcs = s->big.grow(sc, i, bytes)) return rcs;
        bufA = sc.buf[0].as<cx<T>>();
        bufB = sc.buf[1].as<cx<T>>();
    }
    const bool real = s->transform == PFFFT_REAL;
    int rc;
    if (b.core == BIG_RFFT2) {
        rc = launch_tile_rfft(s, in, bufB, ordered ? (void*)out : (void*)bufA, batch, 2LL * s->n, dir, st);
        if (rc < 0) { g_last_error = "pffft_hip: the planned two-sweep real route has no kernel"; return (int)hipErrorInvalidValue; }
        if (rc) return rc;
        return b.post == 5 ? launch_block<T>(s, 5, (const T*)bufA, out, batch, st) : 0;
    }
    // in-place pair pass: one pair per thread, every workgroup once, in dispatch order
    const size_t pair_wgs = (batch * ((size_t)s->n / 2 + 1) + 255) / 256;
    const unsigned egrid = (unsigned)std::min<size_t>(pair_wgs, (size_t)0x7fffffff);
    // ---- before the core
    const cx<T>* cur = (const cx<T>*)in;
    if (b.pre >= 0 && !b.pre_separate) {
        if ((rc = launch_block<T>(s, b.pre, in, (T*)bufA, batch, st))) return rc;
        cur = bufA;
    } else if (b.pre >= 0) {
        if (b.pre != 4) {     // internal -> canonical
            if ((rc = zreorder_batch<T>(s, in, (T*)bufA, batch, PFFFT_FORWARD, st))) return rc;
            cur = bufA;
        }
        if (real) {           // half-complex spectrum -> packed spectrum (in place, never on the caller's input)
            if (cur != bufA) { PF_CHECK(hipMemcpyAsync(bufA, cur, bytes, hipMemcpyDeviceToDevice, st)); cur = bufA; }
            hipLaunchKernelGGL((real_pair_kernel<T, BWD>), dim3(egrid), dim3(256), 0, st, bufA, (long long)batch, (long long)s->n);
            PF_CHECK(hipGetLastError());
        }
    }
    // ---- the core: canonical complex transform cur -> dest (or straight into `out` in the internal layout)
    cx<T>* dest = (b.post >= 0) ? bufA : (cx<T>*)out;
    switch (b.core) {
        case BIG_TILES:
            rc = launch_tile_fft(s, cur, bufB, dest, batch, (long long)s->n, dir, st, b.rfuse ? 3 : b.fuse_out ? 1 : b.fuse_in ? 2 : 0, b.tmode);
            if (rc < 0) { g_last_error = "pffft_hip: the planned tile passes have no kernel"; return (int)hipErrorInvalidValue; }
            if (rc) return rc;
            break;
        case BIG_STREAM:
            if ((rc = big_small_factor<T>(s, cur, bufB, dest, batch, dir, st, b.fuse_out, b.col_in))) return rc;
            break;
        default:
            if ((rc = launch_strided<T>(s, 0, cur, bufB, batch, dir, st))) return rc;
            if ((rc = launch_strided<T>(s, 1, bufB, dest, batch, dir, st))) return rc;
            break;
    }
    // ---- after the core
    if (b.post >= 0 && !b.post_separate) return launch_block<T>(s, b.post, (const T*)bufA, out, batch, st);
    if (b.pair_after || (b.post == 2 && b.post_separate)) {
        hipLaunchKernelGGL((real_pair_kernel<T, FWD>), dim3(egrid), dim3(256), 0, st, dest, (long long)batch, (long long)s->n);
        PF_CHECK(hipGetLastError());
    }
    if (b.post >= 0) return zreorder_batch<T>(s, (const T*)bufA, out, batch, PFFFT_BACKWARD, st);   // canonical -> internal
    return 0;
}

int launch_big(Setup* s, const Route& r, const void* in, void* out, size_t batch, int dir, int ordered, hipStream_t st) {
    if (s->is_double) return launch_big_t<double>(s, r, (const double*)in, (double*)out, batch, dir, ordered, st);
    return launch_big_t<float>(s, r, (const float*)in, (float*)out, batch, dir, ordered, st);
}

}  // namespace pf
