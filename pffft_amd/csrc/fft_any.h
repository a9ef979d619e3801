// Any-length complex transforms (Bluestein): out[k] = w[k] . sum_n (in[n] w[n]) conj(w[k - n]),  w[n] = exp(-j pi n^2 / N)
// - a circular convolution of length M >= 2N - 1 with the fixed filter b[m] = conj(w[m]) (b[M - m] = b[m]), framed by two products with
// the chirp.  The convolution is the library's own (fft_conv.h / pffft_hip_convolve_batch); this file holds the two ends:
//   AnyChirpIO      the loader / store policy of fft_conv_kernel: one kernel reads N samples and writes N samples per vector;
//   any_pad_kernel  / any_crop_kernel: the same two ends as grid-stride kernels around convolve_batch (the composed route).
// The backward direction needs no second table: conj(DFT(conj x)) is the backward transform, so both ends conjugate (`cj`) and the chirp
// and the filter spectrum stay what they are.
#pragma once
#include "fft_conv.h"

namespace pf {

// Loader: a thread fetches the samples of its first-stage operands whose index is below N (8-byte loads: rows of odd N are only 8-byte
// aligned), zeros above; the product with the chirp is taken when the operands are formed, so the raw samples of the NEXT vector wait
// in the prefetch registers unmultiplied.  Store: the results below N times the chirp, 8-byte non-temporal stores; nothing at or above N.
// A thread loads and stores the SAME sample indices (R0 == RL in every convolution configuration), so one chirp value per point serves
// both ends.  HOLD = 1 keeps those E values in registers across the persistent loop; HOLD = 0 reads them at the point of use (the
// table is a few KiB: L1 / L2 hits) where 16 points per thread and the filter spectrum leave no room.  The table holds n (= M) entries,
// zero from N on.  Chirp-z / zoom variants would differ in the two tables only.
template <class C, int HOLD>
struct AnyChirpIO {
    typedef typename C::real_t T;
    typedef cx<T> CX;
    typedef Tiled<C, FWD, 0> KF;
    typedef typename KF::S0 S0;
    static constexpr int n = C::n, E = C::E, TPT = C::TPT, NCH = C::NCH;
    static constexpr int R0 = C::rad(0);
    static_assert(C::VEC == 2, "float configurations only");
    static_assert(C::rad(0) == C::rad(C::NS - 1), "a thread must store the sample indices it loaded: one chirp value per point serves both ends");
    struct Regs { CX w[HOLD ? E : 1]; };
    const T* in;
    T* out;
    const CX* __restrict__ chirp;   // n entries
    unsigned N;
    int cj;
    // sample index of the first point of raw slot (ii, q); the second is the next one
    static __device__ __forceinline__ int sample(int t, int ii, int q) { return 2 * (t + TPT * ii + q * (n / (2 * R0))); }
    __device__ __forceinline__ void init(Regs& r, int t) const {
        if constexpr (HOLD) {
#pragma unroll
            for (int ii = 0; ii < S0::B / 2; ++ii)
#pragma unroll
                for (int q = 0; q < R0; ++q) {
                    const int s = sample(t, ii, q);
                    r.w[(2 * ii) * R0 + q] = chirp[s];
                    r.w[(2 * ii + 1) * R0 + q] = chirp[s + 1];
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
    __device__ __forceinline__ CX w_of(const Regs& r, int slot, int s) const {
        if constexpr (HOLD) return r.w[slot];
        else return chirp[s];
    }
    __device__ __forceinline__ void unpack(const chunk16 (&raw)[NCH], CX (&v)[E], const Regs& r, int t) const {
        const T sg = cj ? (T)-1 : (T)1;   // (exact: conj of the sample)
#pragma unroll
        for (int ii = 0; ii < S0::B / 2; ++ii)
#pragma unroll
            for (int q = 0; q < R0; ++q) {
                const chunk16 c = raw[ii * R0 + q];
                const int s = sample(t, ii, q), i0 = (2 * ii) * R0 + q, i1 = (2 * ii + 1) * R0 + q;
                v[i0] = cmul(mk<T>(c.x, c.y * sg), w_of(r, i0, s));
                v[i1] = cmul(mk<T>(c.z, c.w * sg), w_of(r, i1, s + 1));
            }
    }
    __device__ __forceinline__ void store(const CX (&v)[E], size_t vec, const Regs& r, int t) const {
        CX* dst = reinterpret_cast<CX*>(out) + vec * (size_t)N;
        const T sg = cj ? (T)-1 : (T)1;
#pragma unroll
        for (int ii = 0; ii < S0::B / 2; ++ii)
#pragma unroll
            for (int d = 0; d < R0; ++d) {
                const unsigned s = (unsigned)sample(t, ii, d);
                const int i0 = (2 * ii) * R0 + d, i1 = (2 * ii + 1) * R0 + d;
                if (s < N) {
                    const CX y = cmul(v[i0], w_of(r, i0, (int)s));
                    __builtin_nontemporal_store(mk<T>(y.x, y.y * sg), dst + s);
                }
                if (s + 1 < N) {
                    const CX y = cmul(v[i1], w_of(r, i1, (int)s + 1));
                    __builtin_nontemporal_store(mk<T>(y.x, y.y * sg), dst + s + 1);
                }
            }
    }
};

// The kernel is fft_conv_kernel<C, 0, AnyChirpIO<C, HOLD>> (fft_conv.h): the convolution kernel's body with these two ends.

// which configurations hold the chirp: those whose register count keeps the resident workgroups of the convolution kernel with 32 more
// registers (n <= 2048: one 512-thread workgroup per CU either way); n = 4096 reads it at the point of use
template <class C> struct AnyHold { static constexpr int value = C::n <= 2048 ? 1 : 0; };

// ---- the composed route's two ends: X[v][m] = (cj ? conj(in[v][m]) : in[v][m]) w[m] for m < N, 0 up to M; and
//      out[v][k] = X[v][k] w[k] (conjugated under cj), k < N.  One complex sample (8 / 16 bytes) per access, 64-bit indices.
template <typename T>
__global__ void __launch_bounds__(256) any_pad_kernel(const cx<T>* in, cx<T>* X, const cx<T>* __restrict__ chirp, size_t cnt, size_t N, size_t M,
                                                      int cj) {
    const size_t total = cnt * M, stride = (size_t)gridDim.x * blockDim.x;
    const T sg = cj ? (T)-1 : (T)1;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t v = i / M, m = i - v * M;
        cx<T> y = mk<T>(0, 0);
        if (m < N) {
            const cx<T> a = in[v * N + m], w = chirp[m];
            y = mk<T>(fma_(a.x, w.x, -((a.y * sg) * w.y)), fma_(a.x, w.y, (a.y * sg) * w.x));
        }
        X[i] = y;
    }
}

template <typename T>
__global__ void __launch_bounds__(256) any_crop_kernel(const cx<T>* X, cx<T>* out, const cx<T>* __restrict__ chirp, size_t cnt, size_t N, size_t M,
                                                       int cj) {
    const size_t total = cnt * N, stride = (size_t)gridDim.x * blockDim.x;
    const T sg = cj ? (T)-1 : (T)1;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t v = i / N, k = i - v * N;
        const cx<T> a = X[v * M + k], w = chirp[k];
        out[i] = mk<T>(fma_(a.x, w.x, -(a.y * w.y)), fma_(a.x, w.y, a.y * w.x) * sg);
    }
}

}  // namespace pf
