// Cross- and autocorrelation of rows (include/pffft_hip.h: pffft[d]_hip_xcorr_*):  r = IDFT( W( conj(DFT x) . DFT y ) ), x and y zero-extended
// to n samples, a window of `nlags` lags from lag0 stored.  BOTH factors change per row, so nothing sits in registers across the persistent
// loop the way the filter spectrum of fft_conv.h does.  This file holds
//   xcorr_bin           the arithmetic between the transforms, ONE function for every route: conj(X) Y without fused multiply-adds, and the
//                       PHAT weighting c / |c| with its zero rule;
//   XcorrIO             the two ends of the fused kernel: predicated element-sized loads of a row of `len` elements (zeros beyond), and
//                       the scatter of the lag window, times s;
//   fft_xcorr_kernel    the FUSED route - fft_conv_kernel's persistent loop (the hand-out of pf_handout.h, inactive slots)
//                       around the forward stage sequence run TWICE per row pair (x, whose bins stay in registers, then y through
//                       the same LDS image), the product and the backward sequence.  AUTO runs the forward sequence once.
//   xcorr_pad_kernel / xcorr_product_kernel / xcorr_crop_kernel: the COMPOSED route's kernels around two transform_batch calls.
// The routes run different butterfly networks (the register-tiled halves here, whatever transform_batch picks there): they agree at the
// accuracy bar, not bit for bit.  Within a route the autocorrelation equals the cross-correlation of a row with its copy bit for bit:
// c_im = a - a = +0.
#pragma once
#include "fft_analytic.h"   // analytic_envelope: |c| in the one form every route uses
#include "pf_handout.h"

namespace pf {

enum { XC_PLAIN = 0, XC_PHAT = 1 };   // pffft_hip_xcorr_weight_t

// G = W(conj(X) Y).  Every product and every sum rounded once (the units are built with -ffp-contract=off, as fft_csd.h relies on).
// PHAT: m = |c| as the envelope forms it, correctly rounded divisions; m == 0 gives (+0, +0).  m = inf (|c| above ~1.8e19 in float) gives
// zeros through c / inf, a sum of squares that underflows to zero counts as an empty bin, NaN and inf inputs propagate as NaN.
template <typename T>
__device__ __forceinline__ cx<T> xcorr_bin_t(const cx<T> X, const cx<T> Y, int weight) {
    const T cre = X.x * Y.x + X.y * Y.y;
    const T cim = X.x * Y.y - X.y * Y.x;
    if (weight == XC_PLAIN) return mk<T>(cre, cim);
    const T m = analytic_envelope(cre, cim);
    if (m == (T)0) return mk<T>((T)0, (T)0);
    return mk<T>(cre / m, cim / m);
}
__device__ __forceinline__ cx<float> xcorr_bin(const cx<float> X, const cx<float> Y, int weight) { return xcorr_bin_t<float>(X, Y, weight); }
__device__ __forceinline__ cx<double> xcorr_bin(const cx<double> X, const cx<double> Y, int weight) { return xcorr_bin_t<double>(X, Y, weight); }

// A stored component: ONE product with s, then + 0.  The addition is exact and changes one thing only: a -0 becomes +0.  The inverse
// transform of an all +0 spectrum (an empty PHAT row) leaves -0 in some places on some routes; with this the row is all +0 on every route.
template <typename T> __device__ __forceinline__ T xcorr_out(T s, T a) { return s * a + (T)0; }

// The two ends of the fused kernel.  sample(t, ii, q) is AnyChirpIO's: raw slot (ii, q) holds the two ADJACENT samples of its two
// first-stage operands.  Rows are aligned to one element only (odd lengths), so every element is its own predicated non-temporal access:
// 4 bytes for the real kind, 8 for the complex one; beyond `len` the operand is an exact zero, and so is the imaginary part of a real
// sample.  A thread stores the sample indices it loaded (R0 == RL): lag index p = s - m0 (+ n if negative), m0 = lag0 mod n, written
// only if p < nlags.
template <class C, int REAL>
struct XcorrIO {
    typedef typename C::real_t T;
    typedef cx<T> CX;
    typedef Tiled<C, FWD, 0> KF;
    typedef typename KF::S0 S0;
    static constexpr int n = C::n, E = C::E, TPT = C::TPT, NCH = C::NCH;
    static constexpr int R0 = C::rad(0);
    static constexpr int SPP = REAL ? 1 : 2;   // scalars per element
    static_assert(C::VEC == 2, "float configurations only");
    static_assert(C::rad(0) == C::rad(C::NS - 1), "a thread must store the sample indices it loaded");
    const T* x;
    const T* y;
    T* out;
    unsigned len_x, len_y, m0, nlags;
    T s;
    static __device__ __forceinline__ int sample(int t, int ii, int q) { return 2 * (t + TPT * ii + q * (n / (2 * R0))); }
    // row `vec` of a set of dense rows of `len` elements
    __device__ __forceinline__ void load(chunk16 (&raw)[NCH], const T* base, unsigned len, size_t vec, int t) const {
        const T* src = base + vec * (size_t)len * SPP;
#pragma unroll
        for (int ii = 0; ii < S0::B / 2; ++ii)
#pragma unroll
            for (int q = 0; q < R0; ++q) {
                const unsigned sm = (unsigned)sample(t, ii, q);
                chunk16 c; c.x = 0; c.y = 0; c.z = 0; c.w = 0;
                if constexpr (REAL) {
                    if (sm < len) c.x = __builtin_nontemporal_load(src + sm);
                    if (sm + 1 < len) c.y = __builtin_nontemporal_load(src + sm + 1);
                } else {
                    const CX* sc = reinterpret_cast<const CX*>(src);
                    if (sm < len) { const CX a = __builtin_nontemporal_load(sc + sm); c.x = a.x; c.y = a.y; }
                    if (sm + 1 < len) { const CX b = __builtin_nontemporal_load(sc + sm + 1); c.z = b.x; c.w = b.y; }
                }
                raw[ii * R0 + q] = c;
            }
    }
    __device__ __forceinline__ void load_x(chunk16 (&raw)[NCH], size_t vec, int t) const { load(raw, x, len_x, vec, t); }
    __device__ __forceinline__ void load_y(chunk16 (&raw)[NCH], size_t vec, int t) const { load(raw, y, len_y, vec, t); }
    __device__ __forceinline__ void unpack(const chunk16 (&raw)[NCH], CX (&v)[E]) const {
#pragma unroll
        for (int ii = 0; ii < S0::B / 2; ++ii)
#pragma unroll
            for (int q = 0; q < R0; ++q) {
                const chunk16 c = raw[ii * R0 + q];
                if constexpr (REAL) {
                    v[(2 * ii) * R0 + q] = mk<T>(c.x, (T)0);
                    v[(2 * ii + 1) * R0 + q] = mk<T>(c.y, (T)0);
                } else {
                    v[(2 * ii) * R0 + q] = mk<T>(c.x, c.y);
                    v[(2 * ii + 1) * R0 + q] = mk<T>(c.z, c.w);
                }
            }
    }
    // xcorr_out per stored component
    __device__ __forceinline__ void put(const CX a, unsigned sm, T* dst) const {
        unsigned p = sm - m0;
        if (sm < m0) p += (unsigned)n;
        if (p < nlags) {
            if constexpr (REAL) __builtin_nontemporal_store(xcorr_out(s, a.x), dst + p);
            else __builtin_nontemporal_store(mk<T>(xcorr_out(s, a.x), xcorr_out(s, a.y)), reinterpret_cast<CX*>(dst) + p);
        }
    }
    __device__ __forceinline__ void store(const CX (&v)[E], size_t vec, int t) const {
        T* dst = out + vec * (size_t)nlags * SPP;
#pragma unroll
        for (int ii = 0; ii < S0::B / 2; ++ii)
#pragma unroll
            for (int d = 0; d < R0; ++d) {
                const unsigned sm = (unsigned)sample(t, ii, d);
                put(v[(2 * ii) * R0 + d], sm, dst);
                put(v[(2 * ii + 1) * R0 + d], sm + 1, dst);
            }
    }
};

// One raw[] set: the y row of a pair is requested after the first barrier of the x pass; the next x row after the first barrier of the y
// pass (XPF 1: its registers are live next to the x bins and the y points) or behind the store (XPF 0).  AUTO has no y pass: XPF 1
// requests the next row after the first barrier, as fft_conv_kernel does.
template <class C, class IO, int AUTO, int XPF>
__global__ void __launch_bounds__(C::WG_THREADS, C::WG_THREADS >= 1024 ? 4 : C::OCC)
fft_xcorr_kernel(const IO io, unsigned batch, int weight, const cx<typename C::real_t>* __restrict__ twg,
                 const cx<typename C::real_t>* __restrict__ twrg, unsigned* ctr) {
    typedef typename C::real_t T;
    typedef cx<T> CX;
    typedef Tiled<C, FWD, 0> KF;
    typedef Tiled<C, BWD, 0> KB;
    typedef typename KF::S0 S0;
    constexpr int E = C::E, TPT = C::TPT, NCH = C::NCH, NS = C::NS;
    static_assert(C::rad(0) == C::rad(NS - 1), "the forward transform must leave the bins where the inverse takes its first operands");
    static_assert(C::VEC == 2 && S0::PAIR, "float configurations with an even butterfly count in the first / last stage");
    static_assert(C::TWMODE == 0 || C::TWMODE == 3, "register twiddles only");
    static_assert(NS > 1, "the image is free after a pass because every exchange ends with the read-side xsync");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int slot = threadIdx.x / TPT, t = threadIdx.x % TPT;
    CX* img = reinterpret_cast<CX*>(smem_raw) + (size_t)slot * C::IMG;
    unsigned* s_next = reinterpret_cast<unsigned*>(smem_raw + (size_t)C::T_PER_WG * C::IMG * sizeof(CX));

    typename KF::Tw wf;
    typename KB::Tw wb;
    KF::load_tw(wf, t, twg, twrg);
    KB::load_tw(wb, t, twg, twrg);
    const CX* twt = twg;

    const bool dyn = ctr != nullptr;
    unsigned g = blockIdx.x;
    unsigned pend = blockIdx.x + gridDim.x;   // hand-out: pf_handout.h
    __syncthreads();
    const size_t last = (size_t)batch - 1;
    chunk16 raw[NCH];
    {
        const size_t t0 = (size_t)g * C::T_PER_WG + slot;
        io.load_x(raw, t0 < last ? t0 : last, t);
    }
    for (unsigned it = 0; (size_t)g * C::T_PER_WG < batch; ++it) {
        if (dyn && threadIdx.x == 0) pend = handout_grab(s_next, it, pend, ctr);
        const size_t tr = (size_t)g * C::T_PER_WG + slot;
        const bool active = tr < batch;  // inactive slots recompute the last row pair and never store
        const size_t dv = active ? tr : last;
        CX v[E];
        // the forward stages behind the first barrier (the sequence of fft_conv_kernel)
        auto finish_forward = [&]() {
            KF::template xread<0>(v, t, img); KF::xsync(); KF::template butterflies<1>(v, t, wf, twt);
            if constexpr (NS > 2) { KF::template xwrite<1>(v, t, img); KF::xsync(); KF::template xread<1>(v, t, img); KF::xsync(); KF::template butterflies<2>(v, t, wf, twt); }
            if constexpr (NS > 3) { KF::template xwrite<2>(v, t, img); KF::xsync(); KF::template xread<2>(v, t, img); KF::xsync(); KF::template butterflies<3>(v, t, wf, twt); }
            if constexpr (NS > 4) { KF::template xwrite<3>(v, t, img); KF::xsync(); KF::template xread<3>(v, t, img); KF::xsync(); KF::template butterflies<4>(v, t, wf, twt); }
        };
        // ---- the x row
        io.unpack(raw, v);
        KF::template butterflies<0>(v, t, wf, twt);
        KF::template xwrite<0>(v, t, img);
        __syncthreads();  // publishes s_next; first half of exchange 0
        const unsigned gn = handout_next(dyn, s_next, it, g);
        const size_t tn = (size_t)gn * C::T_PER_WG + slot, nv = tn < last ? tn : last;
        if constexpr (!AUTO) io.load_y(raw, dv, t);
        else if constexpr (XPF) io.load_x(raw, nv, t);
        finish_forward();
        if constexpr (!AUTO) {
            // ---- the y row through the same image: the x bins wait in gx
            CX gx[E];
#pragma unroll
            for (int i = 0; i < E; ++i) gx[i] = v[i];
            io.unpack(raw, v);
            KF::template butterflies<0>(v, t, wf, twt);
            KF::template xwrite<0>(v, t, img);
            __syncthreads();
            if constexpr (XPF) io.load_x(raw, nv, t);
            finish_forward();
#pragma unroll
            for (int i = 0; i < E; ++i) v[i] = xcorr_bin(gx[i], v[i], weight);
        } else {
#pragma unroll
            for (int i = 0; i < E; ++i) v[i] = xcorr_bin(v[i], v[i], weight);
        }
        // ---- backward transform (its first-stage operands are in place)
        KB::template butterflies<0>(v, t, wb, twt);
        { KB::template xwrite<0>(v, t, img); KB::xsync(); KB::template xread<0>(v, t, img); KB::xsync(); KB::template butterflies<1>(v, t, wb, twt); }
        if constexpr (NS > 2) { KB::template xwrite<1>(v, t, img); KB::xsync(); KB::template xread<1>(v, t, img); KB::xsync(); KB::template butterflies<2>(v, t, wb, twt); }
        if constexpr (NS > 3) { KB::template xwrite<2>(v, t, img); KB::xsync(); KB::template xread<2>(v, t, img); KB::xsync(); KB::template butterflies<3>(v, t, wb, twt); }
        if constexpr (NS > 4) { KB::template xwrite<3>(v, t, img); KB::xsync(); KB::template xread<3>(v, t, img); KB::xsync(); KB::template butterflies<4>(v, t, wb, twt); }
        // ---- the lag window
        if (active) io.store(v, dv, t);
        KB::xsync();
        if constexpr (!XPF) io.load_x(raw, nv, t);
        g = gn;
    }
    if (dyn && threadIdx.x == 0) handout_rearm(ctr);
}

// ------------------------------------------------------------------------------------------------ composed route
// Grid-stride kernels, 64-bit indices, one element per access.  The chunk holds `sets` (2: cross, 1: auto) blocks of cnt rows of N complex
// values: the x rows, then the y rows.
template <typename T, int REAL>
__global__ void __launch_bounds__(256) xcorr_pad_kernel(const T* x, const T* y, cx<T>* X, size_t cnt, size_t N, size_t len_x, size_t len_y,
                                                        int sets) {
    const size_t half = cnt * N, total = half * (size_t)sets, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const bool second = i >= half;
        const size_t r = second ? i - half : i, v = r / N, m = r - v * N;
        const T* src = second ? y : x;
        const size_t len = second ? len_y : len_x;
        cx<T> a = mk<T>((T)0, (T)0);
        if (m < len) {
            if constexpr (REAL) a.x = src[v * len + m];
            else a = reinterpret_cast<const cx<T>*>(src)[v * len + m];
        }
        X[i] = a;
    }
}

// Y[i] = W(conj(X[i]) Y[i]) in place on the y half; X == Y is the autocorrelation
template <typename T>
__global__ void __launch_bounds__(256) xcorr_product_kernel(const cx<T>* X, cx<T>* Y, size_t total, int weight) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) Y[i] = xcorr_bin(X[i], Y[i], weight);
}

// out[v][j] = s R[v][(m0 + j) mod N], j < nlags
template <typename T, int REAL>
__global__ void __launch_bounds__(256) xcorr_crop_kernel(const cx<T>* R, T* out, size_t cnt, size_t N, size_t m0, size_t nlags, T s) {
    const size_t total = cnt * nlags, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t v = i / nlags, j = i - v * nlags;
        size_t k = m0 + j;
        if (k >= N) k -= N;
        const cx<T> a = R[v * N + k];
        if constexpr (REAL) out[i] = xcorr_out(s, a.x);
        else reinterpret_cast<cx<T>*>(out)[i] = mk<T>(xcorr_out(s, a.x), xcorr_out(s, a.y));
    }
}

}  // namespace pf
