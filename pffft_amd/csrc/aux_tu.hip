// libpffft_hip.so, translation unit of the spectral helpers in the internal layout: pffft_zreorder / pffft_zconvolve_* batched (the
// kernels of fft_aux.h and the direct ones of fft_generic.h) and pffft_hip_convolve_batch where it is composed of the batched entries.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>

#include "../../include/pffft_hip.h"
#include "pf_host.h"
#include "pf_launch.h"
#include "fft_generic.h"
#include "fft_stock.h"
#include "fft_aux.h"

namespace pf {

template <typename T>
int zreorder_batch(Setup* s, const T* in, T* out, size_t batch, int dir, hipStream_t st) {
    if (!s || s->magic != MAGIC) return (int)hipErrorInvalidHandle;
    if (batch == 0) return 0;
    s = for_device(s);
    // (every route, also the direct kernel that reads no table: one rule for the first call of a setup, in or outside a stream capture)
    if (int rc = ensure_device<T>(s, st)) return rc;
    // through an LDS image of the internal layout when a vector fits (fft_aux.h); AB_AUX_DIRECT = the direct kernel
    constexpr int CH = 16 / (int)sizeof(T), BCH = SkIbs<T>::v / CH;
    const size_t vimg = ((size_t)(s->n / 16) * BCH + 1) * 16;   // block image of one vector, bytes
    const size_t vbytes = s->vec_scalars * sizeof(T);
    // long batches of vectors <= 64 KiB: in-order streaming kernel with next-group prefetch (fft_aux.h); AB_AUX_NO_STREAM = off
    const AbSel sel = ab();
    const bool direct = sel.is(AB_AUX_DIRECT), inorder_small = sel.is(AB_INORDER_SMALL);
    if (vbytes <= ZRD_GROUP_BYTES && batch * vbytes >= ((size_t)64 << 20) && !direct && !sel.is(AB_AUX_NO_STREAM) && !inorder_small && in != out) {
        const int G = (int)(ZRD_GROUP_BYTES / vbytes);
        const bool to_canon = dir == PFFFT_FORWARD;
        const size_t img = to_canon ? (size_t)zrd_canon_img16<T>(s->n) * 16 : vimg;
        const size_t lds = (size_t)G * img + 16;
        if (lds <= LDS_MAX) {
            unsigned* ctr = take_counters(s, st);
            const int nchk = 2 * s->n / CH;
            const dim3 grid((unsigned)num_cus()), blk(ZRD_THREADS);
            const int real = s->transform == PFFFT_REAL;
            return with_flag(to_canon, [&](auto TO_CANON) {
                auto k = zreorder_dyn_kernel<T, decltype(TO_CANON)::value>;
                if (int rcl = allow_big_lds(k, lds)) return rcl;
                hipLaunchKernelGGL(k, grid, blk, lds, st, in, out, batch, s->n, real, G, sk_magic(s->n / 4), sk_magic(nchk), ctr);
                PF_CHECK(hipGetLastError());
                return 0;
            });
        }
    }
    if (vimg <= 128 * 1024 && !direct && in != out) {
        int rc = 0;
        int G = (int)(16384 / vimg);
        if (G < 1) G = 1;
        const size_t lds = (size_t)G * vimg + 16;
        auto k = zreorder_lds_kernel<T>;
        if ((rc = allow_big_lds(k, lds))) return rc;
        size_t per_cu = LDS_MAX / lds;
        if (per_cu > 8) per_cu = 8;
        if (per_cu < 1) per_cu = 1;
        const size_t groups = (batch + G - 1) / G;
        size_t grid = (size_t)num_cus() * per_cu;
        if (grid > groups) grid = groups;
        // >= 128 KiB per atomic (one counter address serves ~80 M atomics/s), >= 8 chunks per workgroup
        size_t kc = (131072 + G * vimg - 1) / (G * vimg), cap = groups / (8 * grid);
        if (kc > cap) kc = cap;
        if (kc > 64) kc = 64;
        // static by default: 0.61-0.70 of the roofline against 0.47-0.62 with in-order chunks (AB_INORDER_SMALL) and
        // 0.41-0.61 for the direct kernel (tools/aux_bench.py)
        unsigned* ctr = (kc < 1 || !inorder_small) ? nullptr : take_counters(s, st);
        if (kc < 1) kc = 1;
        const int nchk = 2 * s->n / CH;
        hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(ZR_THREADS), lds, st, in, out, batch, s->n,
                           (int)(s->transform == PFFFT_REAL), (int)(dir == PFFFT_FORWARD), G, sk_magic(s->n / 4),
                           sk_magic(nchk), ctr, (unsigned)kc);
        PF_CHECK(hipGetLastError());
        return 0;
    }
    size_t total = batch * (size_t)(s->n / 2);
    size_t grid = (total + 255) / 256;
    if (grid > (size_t)num_cus() * 16) grid = (size_t)num_cus() * 16;
    hipLaunchKernelGGL((zreorder_kernel<T>), dim3((unsigned)grid), dim3(256), 0, st, in, out, batch, s->n,
                       (int)(s->transform == PFFFT_REAL), (int)(dir == PFFFT_FORWARD));
    PF_CHECK(hipGetLastError());
    return 0;
}

template <typename T>
int zconvolve_batch(Setup* s, const T* a, const T* b, T* ab, T scaling, size_t batch, int accumulate,
                           int b_broadcast, hipStream_t st) {
    if (!s || s->magic != MAGIC) return (int)hipErrorInvalidHandle;
    if (batch == 0) return 0;
    s = for_device(s);
    if (int rc = ensure_device<T>(s, st)) return rc;   // (every route: see zreorder_batch)
    const AbSel sel = ::pf::ab();      // (`ab` is also this function's output vector)
    const bool direct = sel.is(AB_AUX_DIRECT), inorder_small = sel.is(AB_INORDER_SMALL);
    size_t total = batch * (size_t)(s->n / 4);
    // float: streaming kernel, two pairs per thread with all loads issued first (fft_aux.h): 0.69-0.70 against 0.65-0.70
    // for the grid-stride kernel, which stays for double (0.65 vs 0.41) and as AB_AUX_DIRECT; in-order chunks (AB_INORDER_SMALL)
    // measured 0.57-0.60
    // long batches (>= 64 MiB per stream): in-order streaming kernel with DPP pair exchange (fft_aux.h); AB_AUX_NO_STREAM = off
    {
        const unsigned long long Q = 2ull * total * Zd<T>::UPG;   // 16-byte units in the batch
        if (!direct && !sel.is(AB_AUX_NO_STREAM) && !inorder_small && Q / Zd<T>::CHUNK >= 8192u &&
            Q / Zd<T>::CHUNK < 0xffffffffull) {
            unsigned* ctr = take_counters(s, st);
            const int real = s->transform == PFFFT_REAL;
            const dim3 grid((unsigned)num_cus()), blk(ZD_WAVES * 64);
            const unsigned nq = (unsigned)(s->n / 2) * Zd<T>::UPG;   // units per vector
            return with_flag(accumulate != 0, [&](auto ACC) {
                return with_flag(b_broadcast != 0, [&](auto BC) {
                    hipLaunchKernelGGL((zconvolve_dyn_kernel<T, decltype(ACC)::value, decltype(BC)::value>), grid, blk, 0, st, a, b, ab, Q, nq, real, scaling, ctr);
                    PF_CHECK(hipGetLastError());
                    return 0;
                });
            });
        }
    }
    if (!direct && sizeof(T) == 4) {
        const size_t chunks = (total + ZC_CHUNK - 1) / ZC_CHUNK;
        size_t grid = (size_t)num_cus() * 4;
        if (grid > chunks) grid = chunks;
        size_t kc = 4, cap = chunks / (8 * grid);
        if (kc > cap) kc = cap;
        unsigned* ctr = (kc < 1 || !inorder_small) ? nullptr : take_counters(s, st);
        if (kc < 1) kc = 1;
        const int real = s->transform == PFFFT_REAL;
        return with_flag(accumulate != 0, [&](auto ACC) {
            hipLaunchKernelGGL((zconvolve_stream_kernel<T, decltype(ACC)::value>), dim3((unsigned)grid), dim3(ZC_THREADS), 0, st, a, b, ab, total,
                               (unsigned)(s->n / 4), real, scaling, b_broadcast, ctr, (unsigned)kc);
            PF_CHECK(hipGetLastError());
            return 0;
        });
    }
    size_t grid = (total + 255) / 256;
    if (grid > (size_t)num_cus() * 16) grid = (size_t)num_cus() * 16;
    const size_t vs = s->vec_scalars;
    const int is_real = s->transform == PFFFT_REAL;
    return with_flag(accumulate != 0, [&](auto ACC) {
        hipLaunchKernelGGL((zconvolve_kernel<T, decltype(ACC)::value>), dim3((unsigned)grid), dim3(256), 0, st, a, b, ab, batch, s->n,
                           is_real, scaling, vs, b_broadcast ? (size_t)0 : vs);
        PF_CHECK(hipGetLastError());
        return 0;
    });
}

// out += x, 16-byte units (the accumulate leg of the composed convolution)
template <typename T>
__global__ void vec_add_kernel(const T* __restrict__ x, T* __restrict__ out, size_t units) {
    const vec4<float>* x16 = reinterpret_cast<const vec4<float>*>(x);
    vec4<float>* o16 = reinterpret_cast<vec4<float>*>(out);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < units; i += (size_t)gridDim.x * blockDim.x) {
        const vec4<float> a = x16[i], b = o16[i];
        if constexpr (sizeof(T) == 4) {
            vec4<float> r; r.x = a.x + b.x; r.y = a.y + b.y; r.z = a.z + b.z; r.w = a.w + b.w;
            o16[i] = r;
        } else {
            const vec2<double> da = __builtin_bit_cast(vec2<double>, a), db = __builtin_bit_cast(vec2<double>, b);
            vec2<double> r; r.x = da.x + db.x; r.y = da.y + db.y;
            o16[i] = __builtin_bit_cast(vec4<float>, r);
        }
    }
}

// pffft_hip_convolve_batch: out (+)= backward(forward(in) . H) scaling.  One kernel where fft_conv.h has one (conv_tu.hip);
// otherwise the three batched entries through a per-stream spectrum image (AB_CONV_COMPOSED forces the composition: the second route of the tests).
template <typename T>
int convolve_batch(Setup* s, const T* in, const T* H, T* out, T scaling, size_t batch, int accumulate, int h_broadcast,
                          hipStream_t st) {
    if (int rc = check_setup<T>(s)) return rc;
    if (batch == 0) return 0;
    s = for_device(s);
    int rc = ensure_device<T>(s, st);
    if (rc) return rc;
    if (h_broadcast && !ab().is(AB_CONV_COMPOSED)) {
        rc = launch_conv_fused(s, in, H, out, batch, (double)scaling, accumulate, st);
        if (rc != -1) return rc;
    }
    const size_t bytes = batch * s->vec_scalars * sizeof(T);
    std::lock_guard<std::mutex> lk(s->conv.mu);
    StreamScratch::Entry& sc = s->conv.acquire(st);
    if ((rc = s->conv.grow(sc, 0, bytes))) return rc;
    T* X = sc.buf[0].as<T>();
    if ((rc = transform_batch<T>(s, in, X, batch, PFFFT_FORWARD, 0, st))) return rc;
    if ((rc = zconvolve_batch<T>(s, X, H, X, scaling, batch, 0, h_broadcast, st))) return rc;
    if (!accumulate) return transform_batch<T>(s, X, out, batch, PFFFT_BACKWARD, 0, st);
    if ((rc = transform_batch<T>(s, X, X, batch, PFFFT_BACKWARD, 0, st))) return rc;
    const size_t units = bytes / 16;
    const unsigned grid = (unsigned)std::min<size_t>((units + 255) / 256, (size_t)num_cus() * 16);
    hipLaunchKernelGGL((vec_add_kernel<T>), dim3(grid), dim3(256), 0, st, (const T*)X, out, units);
    PF_CHECK(hipGetLastError());
    return 0;
}

#define PF_AUX_INSTANTIATE(T)                                                                                        \
    template int zreorder_batch<T>(Setup*, const T*, T*, size_t, int, hipStream_t);                                  \
    template int zconvolve_batch<T>(Setup*, const T*, const T*, T*, T, size_t, int, int, hipStream_t);               \
    template int convolve_batch<T>(Setup*, const T*, const T*, T*, T, size_t, int, int, hipStream_t);
PF_AUX_INSTANTIATE(float)
PF_AUX_INSTANTIATE(double)
#undef PF_AUX_INSTANTIATE

}  // namespace pf
