// Zoom transforms (the chirp-z transform on the unit circle): K spectral lines from f0 in steps of df, of rows of N samples,
//   out[k] = sum_{n<N} in[n] exp(-2 pi j n (f0 + k df)) = c[k] . sum_n (in[n] a[n]) b[k - n]
//   a[n] = exp(-2 pi j (n f0 + n^2 df / 2)), n < N;   c[k] = exp(-2 pi j k^2 df / 2), k < K;   b[m] = conj(c[|m|]), -(N-1) <= m <= K-1
// - Bluestein's algorithm like fft_any.h, but the rows differ in length (N in, K out) and the two ends take different tables.  The
// convolution (circular length M >= N + K - 1) is the library's own (fft_conv.h / pffft_hip_convolve_batch); this file holds the two ends:
//   ZoomIO           the loader / store policy of fft_conv_kernel: one kernel reads N samples and writes K samples per row;
//   zoom_pad_kernel  / zoom_crop_kernel: the same two ends as grid-stride kernels around convolve_batch (the composed route).
// The backward direction is the conjugate kernel, conj(zoom(conj x)): both ends conjugate (`cj`), the tables and the filter spectrum stay.
#pragma once
#include "fft_conv.h"

namespace pf {

// Loader: a thread fetches the samples of its first-stage operands whose index is below N (8-byte loads: rows of odd length are only
// 8-byte aligned), zeros above, and multiplies by a[] when the operands are formed (the raw samples of the NEXT row wait in the prefetch
// registers unmultiplied).  Store: the results below K times c[], 8-byte non-temporal stores; nothing at or above K.  A thread stores the
// sample indices it loaded (R0 == RL), but the two ends take DIFFERENT tables: HOLD = 1 keeps 2 E values in registers across the
// persistent loop, HOLD = 0 reads both at the point of use (the tables are a few KiB: L1 / L2 hits).  Both tables hold n (= M) entries,
// `a` zero from N on and `c` zero from K on.
template <class C, int HOLD>
struct ZoomIO {
    typedef typename C::real_t T;
    typedef cx<T> CX;
    typedef Tiled<C, FWD, 0> KF;
    typedef typename KF::S0 S0;
    static constexpr int n = C::n, E = C::E, TPT = C::TPT, NCH = C::NCH;
    static constexpr int R0 = C::rad(0);
    static_assert(C::VEC == 2, "float configurations only");
    static_assert(C::rad(0) == C::rad(C::NS - 1), "a thread must store the sample indices it loaded: one slot numbering serves both ends");
    struct Regs { CX a[HOLD ? E : 1], c[HOLD ? E : 1]; };
    const T* in;
    T* out;
    const CX* __restrict__ ta;   // a[], n entries
    const CX* __restrict__ tc;   // c[], n entries
    unsigned N, K;
    int cj;
    // sample index of the first point of raw slot (ii, q); the second is the next one
    static __device__ __forceinline__ int sample(int t, int ii, int q) { return 2 * (t + TPT * ii + q * (n / (2 * R0))); }
    __device__ __forceinline__ void init(Regs& r, int t) const {
        if constexpr (HOLD) {
#pragma unroll
            for (int ii = 0; ii < S0::B / 2; ++ii)
#pragma unroll
                for (int q = 0; q < R0; ++q) {
                    const int s = sample(t, ii, q), i0 = (2 * ii) * R0 + q, i1 = (2 * ii + 1) * R0 + q;
                    r.a[i0] = ta[s]; r.a[i1] = ta[s + 1];
                    r.c[i0] = tc[s]; r.c[i1] = tc[s + 1];
                }
        }
    }
    __device__ __forceinline__ void load(chunk16 (&raw)[NCH], size_t vec, int t) const {
        const CX* src = reinterpret_cast<const CX*>(in) + vec * (size_t)N;
#pragma unroll
        for (int ii = 0; ii < S0::B / 2; ++ii)
#pragma unroll
            for (int q = 0; q < R0; ++q) {
                const unsigned s = (unsigned)sample(t, ii, q);
                CX a = mk<T>(0, 0), b = mk<T>(0, 0);
                if (s < N) a = __builtin_nontemporal_load(src + s);
                if (s + 1 < N) b = __builtin_nontemporal_load(src + s + 1);
                chunk16 c; c.x = a.x; c.y = a.y; c.z = b.x; c.w = b.y;
                raw[ii * R0 + q] = c;
            }
    }
    __device__ __forceinline__ CX a_of(const Regs& r, int slot, int s) const {
        if constexpr (HOLD) return r.a[slot];
        else return ta[s];
    }
    __device__ __forceinline__ CX c_of(const Regs& r, int slot, int s) const {
        if constexpr (HOLD) return r.c[slot];
        else return tc[s];
    }
    __device__ __forceinline__ void unpack(const chunk16 (&raw)[NCH], CX (&v)[E], const Regs& r, int t) const {
        const T sg = cj ? (T)-1 : (T)1;   // (exact: conj of the sample)
#pragma unroll
        for (int ii = 0; ii < S0::B / 2; ++ii)
#pragma unroll
            for (int q = 0; q < R0; ++q) {
                const chunk16 c = raw[ii * R0 + q];
                const int s = sample(t, ii, q), i0 = (2 * ii) * R0 + q, i1 = (2 * ii + 1) * R0 + q;
                v[i0] = cmul(mk<T>(c.x, c.y * sg), a_of(r, i0, s));
                v[i1] = cmul(mk<T>(c.z, c.w * sg), a_of(r, i1, s + 1));
            }
    }
    __device__ __forceinline__ void store(const CX (&v)[E], size_t vec, const Regs& r, int t) const {
        CX* dst = reinterpret_cast<CX*>(out) + vec * (size_t)K;
        const T sg = cj ? (T)-1 : (T)1;
#pragma unroll
        for (int ii = 0; ii < S0::B / 2; ++ii)
#pragma unroll
            for (int d = 0; d < R0; ++d) {
                const unsigned s = (unsigned)sample(t, ii, d);
                const int i0 = (2 * ii) * R0 + d, i1 = (2 * ii + 1) * R0 + d;
                if (s < K) {
                    const CX y = cmul(v[i0], c_of(r, i0, (int)s));
                    __builtin_nontemporal_store(mk<T>(y.x, y.y * sg), dst + s);
                }
                if (s + 1 < K) {
                    const CX y = cmul(v[i1], c_of(r, i1, (int)s + 1));
                    __builtin_nontemporal_store(mk<T>(y.x, y.y * sg), dst + s + 1);
                }
            }
    }
};

// The kernel is fft_conv_kernel<C, 0, ZoomIO<C, HOLD>> (fft_conv.h): the convolution kernel's body with these two ends.

// Which configurations hold the two tables (4 E registers): those where the compiler's resource remarks for gfx950 show no scratch and
// the resident workgroups of AnyChirpIO at that length (DESIGN.md §3.15 has the figures).  n <= 2048: 210 / 224 / 228 VGPRs, two waves
// per SIMD like AnyChirpIO's 178 / 192 / 196.  n = 4096: holding takes 194 VGPRs and the third resident workgroup that AnyChirpIO keeps
// (152); read at the point of use it takes 168 and keeps it.
template <class C> struct ZoomHold { static constexpr int value = C::n <= 2048 ? 1 : 0; };

// ---- the composed route's two ends: X[v][m] = (cj ? conj(in[v][m]) : in[v][m]) a[m] for m < N, 0 up to M; and
//      out[v][k] = X[v][k] c[k] (conjugated under cj), k < K.  One complex sample (8 / 16 bytes) per access, 64-bit indices.
template <typename T>
__global__ void __launch_bounds__(256) zoom_pad_kernel(const cx<T>* in, cx<T>* X, const cx<T>* __restrict__ ta, size_t cnt, size_t N, size_t M,
                                                       int cj) {
    const size_t total = cnt * M, stride = (size_t)gridDim.x * blockDim.x;
    const T sg = cj ? (T)-1 : (T)1;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t v = i / M, m = i - v * M;
        cx<T> y = mk<T>(0, 0);
        if (m < N) {
            const cx<T> x = in[v * N + m], w = ta[m];
            y = mk<T>(fma_(x.x, w.x, -((x.y * sg) * w.y)), fma_(x.x, w.y, (x.y * sg) * w.x));
        }
        X[i] = y;
    }
}

template <typename T>
__global__ void __launch_bounds__(256) zoom_crop_kernel(const cx<T>* X, cx<T>* out, const cx<T>* __restrict__ tc, size_t cnt, size_t K, size_t M,
                                                        int cj) {
    const size_t total = cnt * K, stride = (size_t)gridDim.x * blockDim.x;
    const T sg = cj ? (T)-1 : (T)1;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t v = i / K, k = i - v * K;
        const cx<T> y = X[v * M + k], w = tc[k];
        out[i] = mk<T>(fma_(y.x, w.x, -(y.y * w.y)), fma_(y.x, w.y, y.y * w.x) * sg);
    }
}

}  // namespace pf
