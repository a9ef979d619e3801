// Analytic signals of real rows (scipy.signal.hilbert):  z = IDFT(H . DFT(x)),  H[k] = c_k gain[k] for k <= n/2 (c_0 = c_{n/2} = 1, else 2),
// zero above - a circular convolution of length n with a GIVEN real spectrum, so it is the library's own convolution
// (fft_conv.h / pffft_hip_convolve_batch) with a real-side loader and one of three stores.  This file holds the two ends:
//   AnalyticIO             the loader / store policy of fft_conv_kernel: one kernel reads n reals and writes n complex values (ANALYTIC) or
//                          n reals (HILBERT = Im z, ENVELOPE = |z|) per row: 12 n / 8 n bytes where the composed route moves 28 n / 40 n;
//   analytic_widen_kernel  / analytic_narrow_kernel: the same two ends as grid-stride kernels around convolve_batch (the composed route).
// The kernel body is untouched and the zero imaginary part the loader forms is exact, so the fused kernel computes what
// fft_conv_kernel<C, 0> computes on the widened row: the routes agree BIT FOR BIT in all three outputs (the envelope through the one
// function below).
#pragma once
#include "fft_conv.h"

namespace pf {

enum AnalyticWhat { AN_ANALYTIC = 0, AN_HILBERT = 1, AN_ENVELOPE = 2 };   // pffft_hip_analytic_what_t

// |z| of every route: one product, one fused multiply-add, the correctly rounded square root.  No scaling: it overflows to +inf where
// re^2 + im^2 does (|z| above ~1.8e19 in float) and loses the bits of a sum that falls below the smallest normal number.
__device__ __forceinline__ float analytic_envelope(float re, float im) { return __builtin_sqrtf(fma_(re, re, im * im)); }
__device__ __forceinline__ double analytic_envelope(double re, double im) { return __builtin_sqrt(fma_(re, re, im * im)); }

// Loader: a raw slot holds the two ADJACENT samples of its two first-stage operands (sample(t, ii, q) and the next one), so a slot is one
// 8-byte non-temporal load - rows of n reals are 8-byte aligned for every legal n, and the row length is n: no predicate.  The imaginary
// parts are an exact zero.  Store: a thread holds the results at the sample indices it loaded (R0 == RL), two adjacent ones per slot:
// the dense 16-byte store of ConvDenseIO (ANALYTIC) or one 8-byte store of the two imaginary parts / the two envelopes.  A slot has
// all samples of its row in registers before its first store and no other slot stores into that row (idle slots and the prefetch past
// the end re-read the last row and store nothing), so out == in is legal for the two real outputs.  Nothing is held across the
// persistent loop.
template <class C, int WHAT>
struct AnalyticIO {
    typedef typename C::real_t T;
    typedef cx<T> CX;
    typedef Tiled<C, FWD, 0> KF;
    typedef typename KF::S0 S0;
    static constexpr int n = C::n, E = C::E, TPT = C::TPT, NCH = C::NCH;
    static constexpr int R0 = C::rad(0);
    static_assert(C::VEC == 2, "float configurations only");
    static_assert(C::rad(0) == C::rad(C::NS - 1), "a thread must store the sample indices it loaded");
    static_assert(WHAT == AN_ANALYTIC || WHAT == AN_HILBERT || WHAT == AN_ENVELOPE, "three outputs");
    struct Regs {};
    const T* in;
    T* out;
    // index, in units of two samples, of raw slot (ii, q): samples 2 pair(...) and 2 pair(...) + 1
    static __device__ __forceinline__ int pair(int t, int ii, int q) { return t + TPT * ii + q * (n / (2 * R0)); }
    __device__ __forceinline__ void init(Regs&, int) const {}
    __device__ __forceinline__ void load(chunk16 (&raw)[NCH], size_t vec, int t) const {
        const CX* src = reinterpret_cast<const CX*>(in + vec * (size_t)n);
#pragma unroll
        for (int ii = 0; ii < S0::B / 2; ++ii)
#pragma unroll
            for (int q = 0; q < R0; ++q) {
                const CX a = __builtin_nontemporal_load(src + pair(t, ii, q));
                chunk16 c; c.x = a.x; c.y = a.y; c.z = 0; c.w = 0;
                raw[ii * R0 + q] = c;
            }
    }
    __device__ __forceinline__ void unpack(const chunk16 (&raw)[NCH], CX (&v)[E], const Regs&, int) const {
#pragma unroll
        for (int ii = 0; ii < S0::B / 2; ++ii)
#pragma unroll
            for (int q = 0; q < R0; ++q) {
                const chunk16 c = raw[ii * R0 + q];
                v[(2 * ii) * R0 + q] = mk<T>(c.x, (T)0);
                v[(2 * ii + 1) * R0 + q] = mk<T>(c.y, (T)0);
            }
    }
    __device__ __forceinline__ void store(const CX (&v)[E], size_t vec, const Regs&, int t) const {
#pragma unroll
        for (int ii = 0; ii < S0::B / 2; ++ii)
#pragma unroll
            for (int d = 0; d < R0; ++d) {
                const CX a = v[(2 * ii) * R0 + d], b = v[(2 * ii + 1) * R0 + d];
                if constexpr (WHAT == AN_ANALYTIC) {
                    chunk16 x; x.x = a.x; x.y = a.y; x.z = b.x; x.w = b.y;
                    __builtin_nontemporal_store(x, reinterpret_cast<chunk16*>(out + vec * 2 * (size_t)n) + pair(t, ii, d));
                } else {
                    CX* dst = reinterpret_cast<CX*>(out + vec * (size_t)n) + pair(t, ii, d);
                    if constexpr (WHAT == AN_HILBERT) __builtin_nontemporal_store(mk<T>(a.y, b.y), dst);
                    else __builtin_nontemporal_store(mk<T>(analytic_envelope(a.x, a.y), analytic_envelope(b.x, b.y)), dst);
                }
            }
    }
};

// The kernel is fft_conv_kernel<C, 0, AnalyticIO<C, WHAT>> (fft_conv.h): the convolution kernel's body with these two ends.

// ---- the composed route's two ends.  X[i] = (in[i], 0) over cnt N scalars; out[i] = Im X[i] / |X[i]|.  One scalar / one complex value
//      per access, 64-bit indices.
template <typename T>
__global__ void __launch_bounds__(256) analytic_widen_kernel(const T* in, cx<T>* X, size_t total) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) X[i] = mk<T>(in[i], (T)0);
}

template <typename T, int WHAT>
__global__ void __launch_bounds__(256) analytic_narrow_kernel(const cx<T>* X, T* out, size_t total) {
    static_assert(WHAT == AN_HILBERT || WHAT == AN_ENVELOPE, "the real outputs");
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const cx<T> a = X[i];
        out[i] = WHAT == AN_HILBERT ? a.y : analytic_envelope(a.x, a.y);
    }
}

}  // namespace pf
