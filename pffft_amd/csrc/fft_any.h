// Any-length complex transforms (Bluestein): out[k] = w[k] . sum_n (in[n] w[n]) conj(w[k - n]),  w[n] = exp(-j pi n^2 / N)
// - a circular convolution of length M >= 2N - 1 with the fixed filter b[m] = conj(w[m]) (b[M - m] = b[m]), framed by two products with
// the chirp.  The convolution is the library's own (fft_conv.h / pffft_hip_convolve_batch); this file holds the two ends:
//   AnyChirpIO      the loader / store policy of fft_conv_kernel: one kernel reads N samples and writes N samples per vector;
//   any_pad_kernel  / any_crop_kernel: the same two ends as grid-stride kernels around convolve_batch (the composed route).
//   AnyRealIO, any_real_*: real rows <-> half spectra (further down).
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
// zero from N on.  The zoom transforms (fft_zoom.h) are this policy with rows of N in and K out and one table per end.
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

// ---- real input, half-spectrum output (pffft[d]_hip_any_new_real_setup).  Only the bins k <= N/2 are wanted, so the index k - n of the
// convolution runs over [-(N-1), N/2] and a circular length M >= N + N/2 suffices; forward and backward take their own filter spectrum
// (the supports are mirror images).  With H = N/2 + 1:
//   forward   a[n] = (x[n] w[n].re, x[n] w[n].im), n < N;   out[k] = y[k] w[k], k < H
//   backward  a[k] = c_k conj(X[k]) w[k], k < H, c_k = 2 but 1 for k = 0 and k = N/2 (even N), the imaginary parts of those two bins read
//             as zero whatever the input holds;   out[n] = Re(y[n] w[n]), n < N
// AnyRealIO is the loader / store policy of fft_conv_kernel, DIRN = FWD / BWD at compile time.  The real side moves 4-byte accesses (rows
// of odd N are aligned to one scalar only), the complex side 8-byte ones; per vector 4 N + 8 H bytes.  Like AnyChirpIO a thread stores
// the indices it loaded, so one chirp value per point (held or read at use, AnyHold) serves both ends; the table has n entries, zero
// from N on.
template <class C, int HOLD, int DIRN>
struct AnyRealIO {
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
    unsigned N, H;
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
    __device__ __forceinline__ CX w_of(const Regs& r, int slot, int s) const {
        if constexpr (HOLD) return r.w[slot];
        else return chirp[s];
    }
    // forward: the two real samples of a slot in (x, y) of its chunk; backward: the two bins in (x, y) and (z, w).  Zero beyond the row.
    __device__ __forceinline__ void load(chunk16 (&raw)[NCH], size_t vec, int t) const {
#pragma unroll
        for (int ii = 0; ii < S0::B / 2; ++ii)
#pragma unroll
            for (int q = 0; q < R0; ++q) {
                const unsigned s = (unsigned)sample(t, ii, q);
                chunk16 c; c.x = 0; c.y = 0; c.z = 0; c.w = 0;
                if constexpr (DIRN == FWD) {
                    const T* src = in + vec * (size_t)N;
                    if (s < N) c.x = __builtin_nontemporal_load(src + s);
                    if (s + 1 < N) c.y = __builtin_nontemporal_load(src + s + 1);
                } else {
                    const CX* src = reinterpret_cast<const CX*>(in) + vec * (size_t)H;
                    if (s < H) { const CX a = __builtin_nontemporal_load(src + s); c.x = a.x; c.y = a.y; }
                    if (s + 1 < H) { const CX b = __builtin_nontemporal_load(src + s + 1); c.z = b.x; c.w = b.y; }
                }
                raw[ii * R0 + q] = c;
            }
    }
    // backward operand of bin k: c_k conj(X[k]) w[k]; the doubling is exact, and the imaginary part of bin 0 / N/2 is not read
    __device__ __forceinline__ CX bin(T re, T im, unsigned k, CX w) const {
        const bool edge = k == 0 || 2 * k == N;
        const T ck = edge ? (T)1 : (T)2;
        return cmul(mk<T>(ck * re, edge ? (T)0 : -(ck * im)), w);
    }
    __device__ __forceinline__ void unpack(const chunk16 (&raw)[NCH], CX (&v)[E], const Regs& r, int t) const {
#pragma unroll
        for (int ii = 0; ii < S0::B / 2; ++ii)
#pragma unroll
            for (int q = 0; q < R0; ++q) {
                const chunk16 c = raw[ii * R0 + q];
                const int s = sample(t, ii, q), i0 = (2 * ii) * R0 + q, i1 = (2 * ii + 1) * R0 + q;
                const CX w0 = w_of(r, i0, s), w1 = w_of(r, i1, s + 1);
                if constexpr (DIRN == FWD) {
                    v[i0] = mk<T>(c.x * w0.x, c.x * w0.y);
                    v[i1] = mk<T>(c.y * w1.x, c.y * w1.y);
                } else {
                    v[i0] = bin(c.x, c.y, (unsigned)s, w0);
                    v[i1] = bin(c.z, c.w, (unsigned)s + 1, w1);
                }
            }
    }
    __device__ __forceinline__ void put(const CX v, CX w, unsigned s, size_t vec) const {
        if constexpr (DIRN == FWD) {
            if (s < H) __builtin_nontemporal_store(cmul(v, w), reinterpret_cast<CX*>(out) + vec * (size_t)H + s);
        } else {
            // (the real part of cmul, in its operations)
            if (s < N) __builtin_nontemporal_store(fma_(v.x, w.x, -(v.y * w.y)), out + vec * (size_t)N + s);
        }
    }
    __device__ __forceinline__ void store(const CX (&v)[E], size_t vec, const Regs& r, int t) const {
#pragma unroll
        for (int ii = 0; ii < S0::B / 2; ++ii)
#pragma unroll
            for (int d = 0; d < R0; ++d) {
                const unsigned s = (unsigned)sample(t, ii, d);
                const int i0 = (2 * ii) * R0 + d, i1 = (2 * ii + 1) * R0 + d;
                put(v[i0], w_of(r, i0, (int)s), s, vec);
                put(v[i1], w_of(r, i1, (int)s + 1), s + 1, vec);
            }
    }
};

// the composed route's two ends for real setups: `back` selects the direction.  One scalar / one complex value per access, 64-bit indices.
template <typename T>
__global__ void __launch_bounds__(256) any_real_pad_kernel(const T* in, cx<T>* X, const cx<T>* __restrict__ chirp, size_t cnt, size_t N, size_t H,
                                                           size_t M, int back) {
    const size_t total = cnt * M, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t v = i / M, m = i - v * M;
        cx<T> y = mk<T>(0, 0);
        if (!back) {
            if (m < N) { const T a = in[v * N + m]; const cx<T> w = chirp[m]; y = mk<T>(a * w.x, a * w.y); }
        } else if (m < H) {
            const cx<T> z = reinterpret_cast<const cx<T>*>(in)[v * H + m], w = chirp[m];
            const bool edge = m == 0 || 2 * m == N;
            const T ck = edge ? (T)1 : (T)2;
            const T re = ck * z.x, im = edge ? (T)0 : -(ck * z.y);
            y = mk<T>(fma_(re, w.x, -(im * w.y)), fma_(re, w.y, im * w.x));
        }
        X[i] = y;
    }
}

template <typename T>
__global__ void __launch_bounds__(256) any_real_crop_kernel(const cx<T>* X, T* out, const cx<T>* __restrict__ chirp, size_t cnt, size_t N, size_t H,
                                                            size_t M, int back) {
    const size_t L = back ? N : H, total = cnt * L, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t v = i / L, k = i - v * L;
        const cx<T> a = X[v * M + k], w = chirp[k];
        const T re = fma_(a.x, w.x, -(a.y * w.y));
        if (back) out[i] = re;
        else reinterpret_cast<cx<T>*>(out)[i] = mk<T>(re, fma_(a.x, w.y, a.y * w.x));
    }
}

// the direct route's two ends: the canonical real spectrum of pffft (DC and Nyquist in elements 0 and 1) <-> H interleaved bins.
// Values move unchanged; the imaginary parts of bin 0 and bin N/2 are written as +0 and not read.
template <typename T>
__global__ void __launch_bounds__(256) any_real_unpack_kernel(const T* S, cx<T>* out, size_t cnt, size_t N) {
    const size_t H = N / 2 + 1, total = cnt * H, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t v = i / H, k = i - v * H;
        const T* s = S + v * N;
        out[i] = k == 0 ? mk<T>(s[0], (T)0) : k == H - 1 ? mk<T>(s[1], (T)0) : mk<T>(s[2 * k], s[2 * k + 1]);
    }
}

template <typename T>
__global__ void __launch_bounds__(256) any_real_pack_kernel(const cx<T>* in, T* S, size_t cnt, size_t N) {
    const size_t H = N / 2 + 1, total = cnt * H, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t v = i / H, k = i - v * H;
        T* s = S + v * N;
        const cx<T> z = in[i];
        if (k == 0) s[0] = z.x;
        else if (k == H - 1) s[1] = z.x;
        else { s[2 * k] = z.x; s[2 * k + 1] = z.y; }
    }
}

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
