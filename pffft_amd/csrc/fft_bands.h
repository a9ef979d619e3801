// Band energies of framed transforms (pffft_hip_bands_batch: mel / Bark / octave bands, rebinned spectrograms): the kernels.
//
//   fft_bands_kernel   the FUSED route - the framed, windowing loader, the stage sequence and the |X|^2 expressions of
//                      fft_frames_kernel<C, FR_POWER, WMODE>; the N/2 + 1 values of a frame go into the slot's LDS image in natural bin
//                      order instead of to HBM (the image is free after the last exchange), and the slot's TPT threads form the band sums
//                      from it in two steps: thread t takes segments t, t + TPT, ... of the bank and leaves their partials in the image
//                      behind the power values, then bands t, t + TPT, ... and adds each band's partials in order.  A wide band is so
//                      split over the threads without changing bits.  Only the `nbands` scalars of a frame are stored.  It is a kernel of
//                      its own built from the Tiled<> helpers: fft_frames_kernel keeps its code.
//   bands_rows_kernel  the COMPOSED route's reduction: one thread per (row, band) over dense |X|^2 rows that the inner setup's own frame
//                      entry wrote.
//
// The order is the contract (include/pffft_hip.h): band b's entries are cut into segments of BANDS_SEG consecutive entries; a segment's
// partial is the sum of fl(w_j p[first + j]), j ascending, started from its first term; the band's value is the sum of its segment
// partials, segment ascending, started from the first; every product and addition rounded once (the library is built with
// -ffp-contract=off), no atomics.  seg_sum below is the one statement of a segment's partial and bands_finish the one scaling / logarithm:
// both kernels call them, so the routes agree bit for bit, LOG included.
// The bank (descriptors and weights) is read through L2 with __restrict__ loads in both kernels: it is a few KiB for the usual banks, every
// workgroup reads all of it for every frame, and in LDS it would put a cap on the sum of the counts that L2 does not need.  What the fused
// kernel does keep in LDS is one partial per segment of the bank, in what the power values leave free of the slot's image: bands_seg_cap.
#pragma once
#include "fft_frames.h"
#include "pf_handout.h"

namespace pf {

constexpr unsigned BANDS_SEG = 16;   // PFFFT_HIP_BANDS_SEG of include/pffft_hip.h
enum { BANDS_ENERGY = 0, BANDS_LOG = 1 };

// band b: entries off ... off + count - 1 of the weights multiply bins first ... first + count - 1; its segments are seg0 ... of the bank's
struct BandDesc { unsigned first, count, seg0, pad; unsigned long long off; };
// segment s of the bank: `len` <= BANDS_SEG entries from off on multiply bins bin ... bin + len - 1
struct SegDesc { unsigned bin, len; unsigned long long off; };

__device__ __forceinline__ float bands_log(float x) { return logf(x); }
__device__ __forceinline__ double bands_log(double x) { return log(x); }

// a segment's partial over the power values p (LDS in the fused kernel, a scratch row in the composed one): m >= 1 entries, j ascending,
// started from the first term.  A full segment is unrolled, so that its loads are in flight together; the order is the same.
template <typename T>
__device__ __forceinline__ T seg_sum(const T* p, const T* __restrict__ w, unsigned m) {
    T part = w[0] * p[0];
    if (m == BANDS_SEG) {
#pragma unroll
        for (unsigned j = 1; j < BANDS_SEG; ++j) part = part + w[j] * p[j];
    } else {
        for (unsigned j = 1; j < m; ++j) part = part + w[j] * p[j];
    }
    return part;
}

// e_b of the contract by one thread: the segment partials added in order; an empty band gives +0
template <typename T>
__device__ __forceinline__ T band_sum(const T* p, const T* __restrict__ w, unsigned count) {
    T e = (T)0;
    for (unsigned s0 = 0; s0 < count; s0 += BANDS_SEG) {
        const T part = seg_sum<T>(p + s0, w + s0, count - s0 < BANDS_SEG ? count - s0 : BANDS_SEG);
        e = s0 == 0 ? part : e + part;
    }
    return e;
}

// segments the fused kernel has room for: one partial per segment behind the n + 1 power values of the slot's image (n + 2: an even offset)
template <class C> constexpr unsigned bands_seg_cap() { return (unsigned)(C::IMG * 2 - (C::n + 2)); }

// ENERGY: fl(scaling e).  LOG: log(max(fl(scaling e), floor)); a NaN passes through the maximum
template <typename T, int WHAT>
__device__ __forceinline__ T bands_finish(T e, T scaling, T floor) {
    const T x = scaling * e;
    if constexpr (WHAT == BANDS_ENERGY) return x;
    else return bands_log(x < floor ? floor : x);
}

// Frame v = i nframes + f of the launch (v < batch) -> nbands scalars at out + v out_stride.  Parameters up to `batch`, the twiddle
// tables and the counters: those of fft_frames_kernel.
template <class C, int WMODE, int WHAT>
__global__ void __launch_bounds__(C::WG_THREADS, C::OCC)
fft_bands_kernel(const float* signal, size_t signal_stride, unsigned nframes, size_t hop, const float* __restrict__ window,
                 float* out, size_t out_stride, unsigned batch, const BandDesc* __restrict__ bank, const SegDesc* __restrict__ segs,
                 const float* __restrict__ weights, unsigned nbands, unsigned nsegs, float scaling, float floor,
                 const cx<float>* __restrict__ twg, const cx<float>* __restrict__ twrg, unsigned* ctr) {
    typedef float T;
    typedef cx<T> CX;
    typedef Tiled<C, FWD, 1> K;
    typedef typename K::S0 S0;
    typedef typename K::SL SL;
    constexpr int n = C::n, E = C::E, TPT = C::TPT, NCH = C::NCH;
    constexpr int R0 = K::R0, RL = K::RL;
    static_assert(sizeof(typename C::real_t) == 4 && C::VEC == 2 && S0::PAIR && SL::PAIR, "float configurations only");
    static_assert(C::TWMODE == 0 || C::TWMODE == 3, "register twiddles only");
    static_assert(((n / RL) % 64 == 0 && (n / R0) % 64 == 0) || C::PADN == 0, "pad period vs operand stride");
    static_assert((size_t)C::IMG * sizeof(CX) >= (size_t)(n + 1) * sizeof(T), "the slot's image holds the n + 1 power values");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int slot = threadIdx.x / TPT, t = threadIdx.x % TPT;
    CX* img = reinterpret_cast<CX*>(smem_raw) + (size_t)slot * C::IMG;
    T* pim = reinterpret_cast<T*>(img);   // the power values of the slot's frame: bins 0 ... n, natural order, no padding
    T* part = pim + (n + 2);              // ... and behind them one partial per segment of the bank (nsegs <= bands_seg_cap<C>())
    unsigned* s_next = reinterpret_cast<unsigned*>(smem_raw + (size_t)C::T_PER_WG * C::IMG * sizeof(CX));
    const chunk16* wtab = reinterpret_cast<const chunk16*>(smem_raw + (size_t)C::T_PER_WG * C::IMG * sizeof(CX) + 16);

    typename K::Tw w;
    K::load_tw(w, t, twg, twrg);
    const CX* twt = twg;
    chunk16 wreg[WMODE == 1 ? NCH : 1];
    if constexpr (WMODE == 1) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) wreg[i] = reinterpret_cast<const chunk16*>(window)[K::plain_chunk(t, i)];
    }
    if constexpr (WMODE == 2) {
        chunk16* wt = const_cast<chunk16*>(wtab);
        for (int i = threadIdx.x; i < n / 2; i += C::WG_THREADS) wt[i] = reinterpret_cast<const chunk16*>(window)[i];
    }
    const bool dyn = ctr != nullptr;
    unsigned g = blockIdx.x;
    unsigned pend = blockIdx.x + gridDim.x;   // hand-out: pf_handout.h
    __syncthreads();
    const size_t last = (size_t)batch - 1;
    // frame v = i nframes + f starts at signal + i signal_stride + f hop (64-bit offsets; v < 2^32)
    auto src_of = [&](size_t tr) -> const T* {
        const unsigned v = (unsigned)(tr < last ? tr : last);
        const unsigned i = v / nframes, f = v - i * nframes;
        return signal + (size_t)i * signal_stride + (size_t)f * hop;
    };
    chunk16 raw[NCH];
    K::load_raw(raw, src_of((size_t)g * C::T_PER_WG + slot), t, true);
    for (unsigned it = 0; (size_t)g * C::T_PER_WG < batch; ++it) {
        if (dyn && threadIdx.x == 0) pend = handout_grab(s_next, it, pend, ctr);
        const size_t tr = (size_t)g * C::T_PER_WG + slot;
        const bool active = tr < batch;  // inactive slots recompute the last frame and never store
        T* dst = out + (active ? tr : last) * out_stride;
        CX v[E];
        int tl = t;
        asm volatile("" : "+v"(tl));

        // ------------------------------------------------------------------ input: raw chunk x window, ONE rounding per scalar
#pragma unroll
        for (int ii = 0; ii < S0::B / 2; ++ii)
#pragma unroll
            for (int q = 0; q < R0; ++q) {
                chunk16 c = raw[ii * R0 + q];
                if constexpr (WMODE != 0) {
                    chunk16 wv;
                    if constexpr (WMODE == 1) wv = wreg[ii * R0 + q];
                    else wv = wtab[K::plain_chunk(tl, ii * R0 + q)];
                    c.x = c.x * wv.x; c.y = c.y * wv.y; c.z = c.z * wv.z; c.w = c.w * wv.w;
                }
                v[(2 * ii) * R0 + q] = mk<T>(c.x, c.y);
                v[(2 * ii + 1) * R0 + q] = mk<T>(c.z, c.w);
            }

        // ------------------------------------------------------------------ transform (the sequence of fft_tiled_kernel)
        K::template butterflies<0>(v, t, w, twt);
        if constexpr (C::NS > 1) K::template xwrite<0>(v, t, img);
        __syncthreads();  // publishes s_next; first half of exchange 0
        const unsigned gn = handout_next(dyn, s_next, it, g);
        if constexpr (C::PREFETCH) K::load_raw(raw, src_of((size_t)gn * C::T_PER_WG + slot), t, true);
        if constexpr (C::NS > 1) { K::template xread<0>(v, t, img); K::xsync(); K::template butterflies<1>(v, t, w, twt); }
        if constexpr (C::NS > 2) { K::template xwrite<1>(v, t, img); K::xsync(); K::template xread<1>(v, t, img); K::xsync(); K::template butterflies<2>(v, t, w, twt); }
        if constexpr (C::NS > 3) { K::template xwrite<2>(v, t, img); K::xsync(); K::template xread<2>(v, t, img); K::xsync(); K::template butterflies<3>(v, t, w, twt); }
        if constexpr (C::NS > 4) { K::template xwrite<3>(v, t, img); K::xsync(); K::template xread<3>(v, t, img); K::xsync(); K::template butterflies<4>(v, t, w, twt); }

        // ------------------------------------------------------------------ |X|^2 as the POWER branch forms it, into the slot's image
        K::pair_regs(v, t, w);   // v[u RL + d] = bin jm(t, u) + d n/RL of the half-complex spectrum; bin 0 = (DC, Nyquist)
#pragma unroll
        for (int u = 0; u < SL::B; ++u)
#pragma unroll
            for (int d = 0; d < RL; ++d) {
                const int k = K::template jm<C::NS - 1>(t, u) + d * (n / RL);
                const CX x = v[u * RL + d];
                if (k == 0) {
                    pim[0] = x.x * x.x;
                    pim[n] = x.y * x.y;
                } else {
                    pim[k] = x.x * x.x + x.y * x.y;
                }
            }
        K::xsync();

        // ------------------------------------------------------------------ the segment partials: thread t takes segments t, t + TPT, ...
        for (unsigned sg = (unsigned)t; sg < nsegs; sg += TPT) {
            const SegDesc sd = segs[sg];
            part[sg] = seg_sum<T>(pim + sd.bin, weights + sd.off, sd.len);
        }
        K::xsync();
        // ------------------------------------------------------------------ the band sums: thread t takes bands t, t + TPT, ...
        for (unsigned b = (unsigned)t; b < nbands; b += TPT) {
            const BandDesc bd = bank[b];
            const unsigned ns = (bd.count + BANDS_SEG - 1) / BANDS_SEG;
            T e = (T)0;
            for (unsigned j = 0; j < ns; ++j) e = j == 0 ? part[bd.seg0] : e + part[bd.seg0 + j];
            const T r = bands_finish<T, WHAT>(e, scaling, floor);
            if (active) __builtin_nontemporal_store(r, dst + b);
        }
        K::xsync();   // frees the image for the next frame
        if constexpr (!C::PREFETCH) K::load_raw(raw, src_of((size_t)gn * C::T_PER_WG + slot), t, true);
        g = gn;
    }
    if (dyn && threadIdx.x == 0) handout_rearm(ctr);
}

// ------------------------------------------------------------------------------------------------ composed route
// `rows` dense |X|^2 rows of P scalars in X -> nbands scalars per row at dst + r dst_stride.  One thread per (row, band), grid stride.
template <typename T, int WHAT>
__global__ void bands_rows_kernel(const T* __restrict__ X, unsigned P, size_t rows, const BandDesc* __restrict__ bank,
                                  const T* __restrict__ weights, unsigned nbands, T scaling, T floor, T* __restrict__ dst, size_t dst_stride) {
    const size_t total = rows * nbands;
    for (size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (size_t)gridDim.x * blockDim.x) {
        const size_t r = x / nbands;
        const unsigned b = (unsigned)(x - r * nbands);
        const BandDesc bd = bank[b];
        dst[r * dst_stride + b] = bands_finish<T, WHAT>(band_sum<T>(X + r * P + bd.first, weights + bd.off, bd.count), scaling, floor);
    }
}

}  // namespace pf
