// Batched 2-D spectral convolution on the fft2 handle (include/pffft_hip.h: pffft[d]_hip_fft2_convolve_batch):
//     out = s IFFT2u( FFT2(in) . G ),  G = H or conj(H),  IFFT2u the unnormalised backward transform of the fft2 entry,
// of dense row-major images of rows x cols interleaved complex values, H a spectrum in natural order (one image for every image of the
// batch, or one per image).  This file holds
//   fft2conv_mul             the product, ONE function for both routes: every product and every sum rounded once, no fused multiply-add
//                            (the units are built with -ffp-contract=off, as fft_xcorr.h relies on), conj_h a run-time argument;
//   fft2conv_product_kernel  the COMPOSED route's kernel between the handle's own forward and backward transforms: in place, grid stride,
//                            64-bit indices, H indexed modulo one image where it is broadcast;
//   fft_fft2conv_kernel      the FUSED route (float, broadcast H, rows and cols in {16, 32, 64}): fft_fft2_kernel's persistent loop
//                            (the hand-out of pf_handout.h, inactive slots, chunked 16-byte loads and stores;
//                            the launch is loop_launch with CONV_ONESHOT) on Fft2Cfg / Fft2Layout as they are, ONE HBM read and ONE HBM
//                            write per image.
// The routes run different butterfly networks: each is held to the float64 truth at the convolution bar, not to the other bit for bit.
//
// The fused kernel, per image:
//   load       as fft_fft2_kernel: chunk t + T i of the dense run, two 8-byte LDS writes per chunk.
//   rows       forward, fft2_axis as it is: a 64-point row ends in base-8 digit-reversed positions (bin v at position fft2_pos(v)).
//   columns    R < 64: a column is one thread's registers - read, dftR forward, x G, dftR backward, write: ONE LDS round trip.
//              R = 64: forward half pass 1 (group j reads x[j + 8 q], dft8 over q, x W_64^(j k1), writes position j + 8 k1), a barrier,
//              then group k1 reads positions 8 k1 ... 8 k1 + 7, dft8 over j leaves X[k1 + 8 k2] in register k2 - exactly what the first
//              half pass of the TRANSPOSED network (digit-reversed in, natural out) reads: x G[k1 + 8 k2], unnormalised inverse dft8 over
//              k2 -> j, x conj(W_64^(j k1)), write position 8 k1 + j; a barrier; then group j reads positions j + 8 k1, inverse dft8
//              over k1 -> q and writes x[j + 8 q] to position j + 8 q.  Three round trips instead of four, natural order out.
//              The seven W_64 values a thread holds serve both twiddle steps: w[k] = W_64^((t / G) k), t / G being j in the first and k1
//              in the second.
//   rows       backward: C < 64 the ordinary line transform, C = 64 the transposed network again (fft2_axis_t).
//   store      chunk t + T i from NATURAL positions, times s (one product per component; s = 1 changes no bit).  No fft2_pos here.
// G.  A thread's spectrum values depend on t only: G[u][v] for its columns, v = fft2_pos<C>(column position), u = k1 + 8 k2 where R = 64.
// HREG 1: they are loaded once per workgroup and stay in registers across the loop (PT complex values, the conjugation already applied).
// HREG 0: they are re-read per group from L2 at the same indices (H is at most 32 KiB and every workgroup reads all of it).  Either way the
// conjugate is a sign flip, which is exact, so x conj(h) through fft2conv_mul has the bits of the stated a.x h.x + a.y h.y, a.y h.x -
// a.x h.y.  The resource table of every form is tools/fft2_resources.py's; the FFT2CONV_FORM table below follows from it.
// IN PLACE (in == out) as in fft_fft2_kernel: an image is wholly in LDS or registers before any of it is stored.
//
// LDS banks (tools/fft2_lds.py, the layouts of fft_fft2.h untouched): the transposed half passes touch the address sets of the forward
// half passes in the other order, the in-register column step those of the column pass, the store reads what the load wrote.  No access
// is worse than 2-way.
//
// Real images are fft_rfft2c.h (pffft[d]_hip_rfft2_convolve_batch), which reuses fft2conv_mul, fft2conv_product_kernel and fft2_half_t2.
// Out of scope: an accumulate form, linear (zero-padded) convolution and cropping, two images that both change per call,
// a fused per-image-H path, fused double, shapes beyond 64.
#pragma once
#include "fft_fft2.h"
#include "pf_handout.h"

namespace pf {

// a . h (conj_h == 0) or a . conj(h): re = a.x h.x -/+ a.y h.y, im = a.x h.y + a.y h.x / a.y h.x - a.x h.y, every product and sum
// rounded once.  The conjugate is a sign flip of h.y, which is exact: x - (-y) and (-x) + y have the bits of x + y and y - x.
template <typename V>
__device__ __forceinline__ V fft2conv_conj(const V h, int conj_h) { return mk<sc<V>>(h.x, conj_h ? -h.y : h.y); }
template <typename V>
__device__ __forceinline__ V fft2conv_mul_g(const V a, const V g) {
    const sc<V> rr = a.x * g.x, ii = a.y * g.y, ri = a.x * g.y, ir = a.y * g.x;
    return mk<sc<V>>(rr - ii, ri + ir);
}
template <typename V>
__device__ __forceinline__ V fft2conv_mul(const V a, const V h, int conj_h) {
    return fft2conv_mul_g(a, fft2conv_conj(h, conj_h));
}

// ------------------------------------------------------------------------------------------------ composed route
// X[i] = X[i] . G[i mod himage] in place; himage = the elements of one image where H is broadcast, else `total`
template <typename T>
__global__ void __launch_bounds__(256) fft2conv_product_kernel(cx<T>* X, const cx<T>* __restrict__ H, size_t total, size_t himage, int conj_h) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) X[i] = fft2conv_mul(X[i], H[i % himage], conj_h);
}

// ------------------------------------------------------------------------------------------------ fused route
// The transposed 64-point network, NL lines in place: digit-reversed positions in (X[k1 + 8 k2] at 8 k1 + k2), natural positions out,
// unnormalised backward.  Line l starts at img + l LS, elements ES apart; w as in fft2_axis.  The second half alone is fft2_half_t2.
template <int NL, int LS, int ES, int T>
__device__ __forceinline__ void fft2_half_t2(cx<float>* img, int t) {
    constexpr int G = T / 8;
    const int j = t / G, l0 = t % G;
#pragma unroll
    for (int i = 0; i < NL / G; ++i) {
        cx<float>* p = img + (l0 + G * i) * LS + j * ES;
        cx<float> a[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) a[k] = p[8 * k * ES];
        dft8<BWD>(a);
#pragma unroll
        for (int q = 0; q < 8; ++q) p[8 * q * ES] = a[q];
    }
}
template <int NL, int LS, int ES, int T>
__device__ __forceinline__ void fft2_axis_t(cx<float>* img, int t, const cx<float> (&w)[8]) {
    constexpr int G = T / 8;
    static_assert(T % 8 == 0 && NL % G == 0, "eight thread groups, whole lines per thread");
    const int k1 = t / G, l0 = t % G;
#pragma unroll
    for (int i = 0; i < NL / G; ++i) {
        cx<float>* p = img + (l0 + G * i) * LS + 8 * k1 * ES;
        cx<float> a[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) a[k] = p[k * ES];
        dft8<BWD>(a);
#pragma unroll
        for (int j = 1; j < 8; ++j) a[j] = twmul<BWD>(a[j], w[j]);
#pragma unroll
        for (int j = 0; j < 8; ++j) p[j * ES] = a[j];
    }
    __syncthreads();
    fft2_half_t2<NL, LS, ES, T>(img, t);
}

// The form per shape, (rows, cols, PF, HREG).  PF: the next group's chunks are requested before the column step (1) or behind the store
// (0).  HREG: G stays in registers across the loop (1) or is re-read per group from L2 (0).  From the resource remarks of all four forms of
// every shape (tools/fft2_resources.py; the table of DESIGN.md §3.29): a form qualifies with no scratch and waves per SIMD not below what
// the LDS images allow anyway.  Where more than one form qualifies (six shapes) the choice is the one timed fastest on the device at 64 MiB
// of images (the table of DESIGN.md §3.29).
template <int R, int C> struct Fft2ConvForm;
#define FFT2CONV_FORM(R_, C_, PF_, HREG_) \
    template <> struct Fft2ConvForm<R_, C_> { static constexpr int PF = PF_, HREG = HREG_; };
FFT2CONV_FORM(16, 16, 0, 1)
FFT2CONV_FORM(16, 32, 0, 1)
FFT2CONV_FORM(16, 64, 0, 0)
FFT2CONV_FORM(32, 16, 0, 0)
FFT2CONV_FORM(32, 32, 0, 0)
FFT2CONV_FORM(32, 64, 0, 0)
FFT2CONV_FORM(64, 16, 0, 0)
FFT2CONV_FORM(64, 32, 0, 0)
FFT2CONV_FORM(64, 64, 0, 0)
#undef FFT2CONV_FORM

// values of G a thread holds: g[0 ... PT - 1] (an array of the kernel, indexed by constants throughout), in the order its column step meets them
template <int R, int C>
__device__ __forceinline__ void fft2conv_load_g(cx<float>* g, const cx<float>* __restrict__ H, int t, int conj_h) {
    constexpr int T = Fft2Cfg<R, C>::T;
    if constexpr (R < 64) {
#pragma unroll
        for (int i = 0; i < C / T; ++i) {
            const int v = fft2_pos<C>(t + T * i);
#pragma unroll
            for (int u = 0; u < R; ++u) g[i * R + u] = fft2conv_conj(H[u * C + v], conj_h);
        }
    } else {
        constexpr int G = T / 8;
        const int k1 = t / G, l0 = t % G;
#pragma unroll
        for (int i = 0; i < C / G; ++i) {
            const int v = fft2_pos<C>(l0 + G * i);
#pragma unroll
            for (int k2 = 0; k2 < 8; ++k2) g[i * 8 + k2] = fft2conv_conj(H[(k1 + 8 * k2) * C + v], conj_h);
        }
    }
}

// The column step: forward over the columns, x G, backward over the columns; the rows are at whatever positions the row pass left them.
// HREG 1: G from the registers g (fft2conv_load_g); HREG 0: re-read from H (L2) at the same indices, conjugated as it arrives.
template <int R, int C, int HREG>
__device__ __forceinline__ void fft2conv_columns(cx<float>* img, int t, const cx<float> (&w)[8], const cx<float>* g, const cx<float>* __restrict__ H,
                                                 int conj_h) {
    constexpr int T = Fft2Cfg<R, C>::T, PITCH = Fft2Cfg<R, C>::PITCH;
    if constexpr (R < 64) {
        static_assert(C % T == 0, "whole columns per thread");
#pragma unroll
        for (int i = 0; i < C / T; ++i) {
            cx<float>* p = img + (t + T * i);
            cx<float> a[R];
#pragma unroll
            for (int q = 0; q < R; ++q) a[q] = p[q * PITCH];
            dftR<R, FWD>(a);
            [[maybe_unused]] const int v = fft2_pos<C>(t + T * i);
#pragma unroll
            for (int u = 0; u < R; ++u) a[u] = fft2conv_mul_g(a[u], HREG ? g[i * R + u] : fft2conv_conj(H[u * C + v], conj_h));
            dftR<R, BWD>(a);
#pragma unroll
            for (int q = 0; q < R; ++q) p[q * PITCH] = a[q];
        }
    } else {
        constexpr int G = T / 8;
        static_assert(T % 8 == 0 && C % G == 0, "eight thread groups, whole columns per thread");
        const int j = t / G, l0 = t % G;   // j in the first half pass, k1 in the second
#pragma unroll
        for (int i = 0; i < C / G; ++i) {
            cx<float>* p = img + (l0 + G * i) + j * PITCH;
            cx<float> a[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) a[q] = p[8 * q * PITCH];
            dft8<FWD>(a);
#pragma unroll
            for (int k = 1; k < 8; ++k) a[k] = twmul<FWD>(a[k], w[k]);
#pragma unroll
            for (int k = 0; k < 8; ++k) p[8 * k * PITCH] = a[k];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < C / G; ++i) {
            cx<float>* p = img + (l0 + G * i) + 8 * j * PITCH;
            cx<float> a[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) a[q] = p[q * PITCH];
            dft8<FWD>(a);                                                    // a[k2] = X[k1 + 8 k2]
            [[maybe_unused]] const int v = fft2_pos<C>(l0 + G * i);
#pragma unroll
            for (int k2 = 0; k2 < 8; ++k2)
                a[k2] = fft2conv_mul_g(a[k2], HREG ? g[i * 8 + k2] : fft2conv_conj(H[(j + 8 * k2) * C + v], conj_h));
            dft8<BWD>(a);                                                    // k2 -> j
#pragma unroll
            for (int k = 1; k < 8; ++k) a[k] = twmul<BWD>(a[k], w[k]);
#pragma unroll
            for (int k = 0; k < 8; ++k) p[k * PITCH] = a[k];
        }
        __syncthreads();
        fft2_half_t2<C, 1, PITCH, T>(img, t);
    }
}

template <int R, int C, int PF, int HREG>
__global__ void __launch_bounds__(256)
fft_fft2conv_kernel(const float* in, const cx<float>* __restrict__ H, float* out, unsigned batch, float s, int conj_h,
                    const cx<float>* __restrict__ tw64, unsigned* ctr) {
    typedef Fft2Cfg<R, C> Cf;
    typedef cx<float> CX;
    typedef vec4<float> chunk;
    constexpr int T = Cf::T, NCH = Cf::NCH, PITCH = Cf::PITCH, SLOTS = Cf::SLOTS;
    constexpr size_t IMAGE = (size_t)R * C * 2;   // scalars of one image
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int slot = threadIdx.x / T, t = threadIdx.x % T;
    CX* img = reinterpret_cast<CX*>(smem_raw) + (size_t)slot * Cf::IMG;
    unsigned* s_next = reinterpret_cast<unsigned*>(smem_raw + (size_t)SLOTS * Cf::IMG * sizeof(CX));

    CX w[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) w[k] = mk<float>(1.0f, 0.0f);
    if constexpr (R == 64 || C == 64) {
        const int j = t / (T / 8);
#pragma unroll
        for (int k = 1; k < 8; ++k) w[k] = tw64[j * k];
    }
    CX g_[HREG ? Cf::PT : 1];
    if constexpr (HREG) fft2conv_load_g<R, C>(g_, H, t, conj_h);

    const bool dyn = ctr != nullptr;
    unsigned g = blockIdx.x;
    unsigned pend = blockIdx.x + gridDim.x;   // hand-out: pf_handout.h
    const size_t last = (size_t)batch - 1;
    chunk raw[NCH];
    auto load = [&](size_t image) {
        const chunk* src = reinterpret_cast<const chunk*>(in + image * IMAGE);
#pragma unroll
        for (int i = 0; i < NCH; ++i) raw[i] = __builtin_nontemporal_load(src + t + T * i);
    };
    {
        const size_t t0 = (size_t)g * SLOTS + slot;
        load(t0 < last ? t0 : last);
    }
    for (unsigned it = 0; (size_t)g * SLOTS < batch; ++it) {
        if (dyn && threadIdx.x == 0) pend = handout_grab(s_next, it, pend, ctr);
        const size_t tr = (size_t)g * SLOTS + slot;
        const bool active = tr < batch;  // inactive slots recompute the last image and never store
        const size_t dv = active ? tr : last;
        // ---- the image into LDS (free: the previous pass ended with a barrier behind its last read)
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int e = 2 * (t + T * i);
            CX* p = img + (e / C) * PITCH + e % C;
            p[0] = mk<float>(raw[i].x, raw[i].y);
            p[1] = mk<float>(raw[i].z, raw[i].w);
        }
        __syncthreads();  // publishes s_next
        const unsigned gn = handout_next(dyn, s_next, it, g);
        const size_t tn = (size_t)gn * SLOTS + slot, nv = tn < last ? tn : last;
        // ---- rows forward: lines of C points, 1 apart, PITCH from line to line
        fft2_axis<C, R, PITCH, 1, T, FWD>(img, t, w);
        __syncthreads();
        if constexpr (PF) load(nv);
        // ---- columns: forward, x G, backward
        fft2conv_columns<R, C, HREG>(img, t, w, g_, H, conj_h);
        __syncthreads();
        // ---- rows backward, natural positions out
        if constexpr (C < 64) fft2_axis<C, R, PITCH, 1, T, BWD>(img, t, w);
        else fft2_axis_t<R, PITCH, 1, T>(img, t, w);
        __syncthreads();
        // ---- store
        if (active) {
            chunk* dst = reinterpret_cast<chunk*>(out + dv * IMAGE);
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int e = 2 * (t + T * i);
                const CX* p = img + (e / C) * PITCH + e % C;
                const CX a = p[0], b = p[1];
                chunk o;
                o.x = s * a.x; o.y = s * a.y; o.z = s * b.x; o.w = s * b.y;
                __builtin_nontemporal_store(o, dst + t + T * i);
            }
        }
        __syncthreads();
        if constexpr (!PF) load(nv);
        g = gn;
    }
    if (dyn && threadIdx.x == 0) handout_rearm(ctr);
}

}  // namespace pf
