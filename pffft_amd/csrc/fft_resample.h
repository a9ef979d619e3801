// Fourier resampling of rows (include/pffft_hip.h: pffft[d]_hip_resample_*): N samples in, M samples out over the same span.
//     X = DFT_N(x);  Y = the M-point spectrum below;  out = s IDFT_M(Y),  s = scaling / N
//     h = min(N, M) / 2:   Y[k] = X[k], k < h;   Y[M - k] = X[N - k], 1 <= k < h;   every other bin but h (and M - h) is +0;
//     Y[h] = X[h] (N == M),  X[h] + X[N - h] (M < N, one addition per component),  Y[h] = Y[M - h] = 0.5 X[h] (M > N, exact)
// This file holds
//   resample_bin           the map, ONE function of (row spectrum, m) for the composed route;
//   resample_widen_kernel / resample_map_kernel / resample_narrow_kernel: the COMPOSED route's kernels around two transform_batch calls
//                          of different lengths (the map writes every one of the M bins, times s);
//   fft_resample_kernel    the FUSED route: two Tiled<> halves of DIFFERENT lengths joined in LDS.  Both are 16-point-per-thread
//                          configurations of ConvPick<float> whose first and last radix is 8, so the larger length nB runs on TB threads,
//                          the smaller nS on TS = TB / R threads, R = nB / nS = 2, 4 or 8.  A slot is TB threads and one image of the
//                          larger configuration; a group of work is R rows per slot.
//                            up (N = nS, M = nB):  the slot's R sub-slots transform R rows forward at once, each in its own sub-image;
//                                                 the last stage's bins are parked there in NATURAL order; every thread of the slot
//                                                 pulls the 16 non-zero first-stage operands of ALL R rows (16 / R per row) into
//                                                 registers; the slot runs the backward transform R times through the whole image.
//                            down (N = nB, M = nS): R forward transforms through the whole image, each leaving the 16 / R kept bins per
//                                                 thread in registers; they are parked as R natural-order sub-images; the R sub-slots
//                                                 run the backward transform at once.
//                          No thread idles in either phase.  The hand-over crosses sub-slot boundaries: it is fenced by the LARGER
//                          configuration's xsync.  Rows past the end of the batch recompute the last row and never store.
//                          The persistent loop, the hand-out and s_next are fft_conv_kernel's.
// The routes run different butterfly networks: they agree at the accuracy bar, not bit for bit.
#pragma once
#include <type_traits>

#include "fft_conv.h"   // ConvPick
#include "pf_handout.h"

namespace pf {

// ------------------------------------------------------------------------------------------------ composed route
// s Y[m] of one row: X its N-point spectrum.  No fused multiply-adds (the units are built with -ffp-contract=off).
template <typename T>
__device__ __forceinline__ cx<T> resample_bin(const cx<T>* X, size_t N, size_t M, size_t m, T s) {
    const size_t h = (N < M ? N : M) / 2;
    cx<T> y = mk<T>((T)0, (T)0);
    if (m < h) y = X[m];
    else if (m > M - h) y = X[(m + N) - M];
    else if (m == h) {
        const cx<T> a = X[h];
        if (N == M) y = a;
        else if (M < N) { const cx<T> b = X[N - h]; y = mk<T>(a.x + b.x, a.y + b.y); }
        else y = mk<T>((T)0.5 * a.x, (T)0.5 * a.y);
    } else if (m == M - h) {   // (M > N only: elsewhere M - h == h)
        const cx<T> a = X[h];
        y = mk<T>((T)0.5 * a.x, (T)0.5 * a.y);
    } else return y;           // +0, unscaled
    return mk<T>(s * y.x, s * y.y);
}

// Grid-stride kernels, 64-bit indices, one element per access.
template <typename T>
__global__ void __launch_bounds__(256) resample_widen_kernel(const T* in, cx<T>* X, size_t total) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) X[i] = mk<T>(in[i], (T)0);
}
template <typename T>
__global__ void __launch_bounds__(256) resample_map_kernel(const cx<T>* X, cx<T>* Y, size_t cnt, size_t N, size_t M, T s) {
    const size_t total = cnt * M, stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const size_t v = i / M, m = i - v * M;
        Y[i] = resample_bin<T>(X + v * N, N, M, m, s);
    }
}
template <typename T>
__global__ void __launch_bounds__(256) resample_narrow_kernel(const cx<T>* Y, T* out, size_t total) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) out[i] = Y[i].x;
}

// ------------------------------------------------------------------------------------------------ fused route
// The two HBM ends, for a 16-point-per-thread configuration with R0 = RL = 8: thread t holds the samples 2t + q n/8 (v[q]) and
// 2t + 1 + q n/8 (v[8 + q]).  Rows are aligned to one element only, so every element is its own non-temporal access (4 bytes real, 8
// complex); a real sample has an exact zero imaginary part, and only Re is stored.
template <class C, int REAL>
struct ResampleIO {
    typedef cx<float> CX;
    static constexpr int SPP = REAL ? 1 : 2, RAWN = 16 * SPP, Q = C::n / 8;
    static __device__ __forceinline__ void load(float (&raw)[RAWN], const float* row, int t) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int sm = 2 * t + q * Q;
            if constexpr (REAL) {
                raw[2 * q] = __builtin_nontemporal_load(row + sm);
                raw[2 * q + 1] = __builtin_nontemporal_load(row + sm + 1);
            } else {
                const CX* sc = reinterpret_cast<const CX*>(row);
                const CX a = __builtin_nontemporal_load(sc + sm), b = __builtin_nontemporal_load(sc + sm + 1);
                raw[4 * q] = a.x; raw[4 * q + 1] = a.y; raw[4 * q + 2] = b.x; raw[4 * q + 3] = b.y;
            }
        }
    }
    static __device__ __forceinline__ void unpack(const float (&raw)[RAWN], CX (&v)[16]) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            if constexpr (REAL) { v[q] = mk<float>(raw[2 * q], 0.0f); v[8 + q] = mk<float>(raw[2 * q + 1], 0.0f); }
            else { v[q] = mk<float>(raw[4 * q], raw[4 * q + 1]); v[8 + q] = mk<float>(raw[4 * q + 2], raw[4 * q + 3]); }
        }
    }
    // one product with s per stored component
    static __device__ __forceinline__ void store(const CX (&v)[16], float* row, int t, float s) {
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            const int sm = 2 * t + d * Q;
            if constexpr (REAL) {
                __builtin_nontemporal_store(s * v[d].x, row + sm);
                __builtin_nontemporal_store(s * v[8 + d].x, row + sm + 1);
            } else {
                CX* dc = reinterpret_cast<CX*>(row);
                __builtin_nontemporal_store(mk<float>(s * v[d].x, s * v[d].y), dc + sm);
                __builtin_nontemporal_store(mk<float>(s * v[8 + d].x, s * v[8 + d].y), dc + sm + 1);
            }
        }
    }
};

// the stages of one transform behind its first exchange write and barrier / the whole transform from operands in place
template <class K, class C>
__device__ __forceinline__ void resample_finish(cx<float> (&v)[16], int t, const typename K::Tw& w, const cx<float>* tw, cx<float>* img) {
    K::template xread<0>(v, t, img); K::xsync(); K::template butterflies<1>(v, t, w, tw);
    if constexpr (C::NS > 2) { K::template xwrite<1>(v, t, img); K::xsync(); K::template xread<1>(v, t, img); K::xsync(); K::template butterflies<2>(v, t, w, tw); }
    if constexpr (C::NS > 3) { K::template xwrite<2>(v, t, img); K::xsync(); K::template xread<2>(v, t, img); K::xsync(); K::template butterflies<3>(v, t, w, tw); }
}
template <class K, class C>
__device__ __forceinline__ void resample_whole(cx<float> (&v)[16], int t, const typename K::Tw& w, const cx<float>* tw, cx<float>* img) {
    K::template butterflies<0>(v, t, w, tw);
    K::template xwrite<0>(v, t, img);
    K::xsync();
    resample_finish<K, C>(v, t, w, tw, img);
}

__device__ __forceinline__ cx<float> resample_pick(bool c, cx<float> a, cx<float> b) { return mk<float>(c ? a.x : b.x, c ? a.y : b.y); }
__device__ __forceinline__ cx<float> resample_half(cx<float> a) { return mk<float>(0.5f * a.x, 0.5f * a.y); }

// up: the first-stage operands of the LARGER backward transform from the 16 / R pairs g[0 .. 2 NPR) of one row's parked spectrum
// (g[2c], g[2c + 1] = X[2t + c nB/8], X[2t + 1 + c nB/8]); v[q], v[8 + q] = Y[2t + q nB/8], Y[2t + 1 + q nB/8].  h = nS / 2.
template <int R, int TB>
__device__ __forceinline__ void resample_spread(const cx<float> (&g)[16], cx<float> (&v)[16], int t) {
    const cx<float> z = mk<float>(0.0f, 0.0f);
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = z;
    if constexpr (R == 2) {          // h = 2 nB/8: quarters 0, 1 stay, 2 and 3 move to q = 6, 7; bin h is thread 0's g[4]
        v[0] = g[0]; v[8] = g[1]; v[1] = g[2]; v[9] = g[3];
        v[2] = resample_pick(t == 0, resample_half(g[4]), z);
        v[6] = resample_pick(t == 0, resample_half(g[4]), g[4]); v[14] = g[5];
        v[7] = g[6]; v[15] = g[7];
    } else if constexpr (R == 4) {   // h = nB/8: half 0 stays, half 1 moves to q = 7; bin h is thread 0's g[2]
        v[0] = g[0]; v[8] = g[1];
        v[1] = resample_pick(t == 0, resample_half(g[2]), z);
        v[7] = resample_pick(t == 0, resample_half(g[2]), g[2]); v[15] = g[3];
    } else {                         // h = nB/16 = TB: threads below TB/2 feed q = 0, above q = 7; bin h is thread TB/2's g[0]
        const cx<float> hb = resample_pick(t == TB / 2, resample_half(g[0]), z);
        v[0] = resample_pick(t < TB / 2, g[0], hb); v[8] = resample_pick(t < TB / 2, g[1], z);
        v[7] = resample_pick(t > TB / 2, g[0], hb); v[15] = resample_pick(t >= TB / 2, g[1], z);
    }
}
// down: the 16 / R kept pairs of one row from the last-stage bins of the LARGER forward transform (v[d], v[8 + d] = X[2t + d nB/8],
// X[2t + 1 + d nB/8]) into g[2c], g[2c + 1] = Y[2t + c nB/8], Y[2t + 1 + c nB/8], c < 8 / R.  h = nS / 2.
template <int R, int TB>
__device__ __forceinline__ void resample_keep(const cx<float> (&v)[16], cx<float> (&g)[16], int t) {
    constexpr int O = 16 - 16 / R;   // the row's place: the last 2 NPR entries
    if constexpr (R == 2) {
        g[O + 0] = v[0]; g[O + 1] = v[8]; g[O + 2] = v[1]; g[O + 3] = v[9];
        g[O + 4] = resample_pick(t == 0, mk<float>(v[2].x + v[6].x, v[2].y + v[6].y), v[6]); g[O + 5] = v[14];
        g[O + 6] = v[7]; g[O + 7] = v[15];
    } else if constexpr (R == 4) {
        g[O + 0] = v[0]; g[O + 1] = v[8];
        g[O + 2] = resample_pick(t == 0, mk<float>(v[1].x + v[7].x, v[1].y + v[7].y), v[7]); g[O + 3] = v[15];
    } else {
        const cx<float> hi = resample_pick(t == TB / 2, mk<float>(v[0].x + v[7].x, v[0].y + v[7].y), v[7]);
        g[O + 0] = resample_pick(t < TB / 2, v[0], hi); g[O + 1] = resample_pick(t < TB / 2, v[8], v[15]);
    }
}
// the next row's entries move to the front
template <int R> __device__ __forceinline__ void resample_shift(cx<float> (&g)[16]) {
#pragma unroll
    for (int i = 0; i + 16 / R < 16; ++i) g[i] = g[i + 16 / R];
}

// CS: the smaller length's configuration, CB: the larger one's.  UP: N = CS::n, M = CB::n; else N = CB::n, M = CS::n.
// PF: where the next group's first loads are requested - 1: behind the first barrier of the pass (registers live through the pass),
// 0: behind the last store.  (down: the rows 1 .. R - 1 of a group are always requested one transform ahead.)
template <class CS, class CB, int UP, int REAL, int PF>
__global__ void __launch_bounds__(512, 2)
fft_resample_kernel(const float* __restrict__ in, float* __restrict__ out, unsigned batch, float s, const cx<float>* __restrict__ tws,
                    const cx<float>* __restrict__ twb, unsigned* ctr) {
    typedef cx<float> CX;
    typedef Tiled<CS, UP ? FWD : BWD, 0> KS;
    typedef Tiled<CB, UP ? BWD : FWD, 0> KB;
    typedef typename std::conditional<UP != 0, ResampleIO<CS, REAL>, ResampleIO<CB, REAL>>::type LD;   // the loading end
    typedef typename std::conditional<UP != 0, ResampleIO<CB, REAL>, ResampleIO<CS, REAL>>::type ST;   // the storing end
    constexpr int TS = CS::TPT, TB = CB::TPT, R = TB / TS, NPR = 8 / R, WG = 512, G = WG / TS, SLOTS = WG / TB;
    constexpr int nS = CS::n, nB = CB::n, SPP = REAL ? 1 : 2;
    constexpr int SIMG = CS::IMG_NAT > CS::IMG_TRN ? CS::IMG_NAT : CS::IMG_TRN;   // a sub-image: the smaller transform's exchanges
    static_assert(CS::E == 16 && CB::E == 16 && CS::VEC == 2 && CB::VEC == 2, "float configurations of 16 points per thread");
    static_assert(CS::rad(0) == 8 && CS::rad(CS::NS - 1) == 8 && CB::rad(0) == 8 && CB::rad(CB::NS - 1) == 8, "first and last radix 8");
    static_assert(CS::TWMODE == 3 && CB::TWMODE == 3, "one base twiddle per butterfly in registers");
    static_assert(CS::WG_THREADS == WG && CB::WG_THREADS == WG, "512-thread workgroups");
    static_assert(nB == R * nS && (R == 2 || R == 4 || R == 8), "length ratio 2, 4 or 8");
    static_assert(R * SIMG <= CB::IMG && SIMG % 2 == 0 && CB::IMG % 2 == 0 && SIMG >= nS, "R sub-images in one image, 16-byte aligned");
    static_assert(CS::NS > 1 && CS::NS <= 4 && CB::NS <= 4, "the image is free after a pass: every exchange ends with the read-side xsync");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int tid = threadIdx.x;
    const int ss = tid / TS, ts = tid % TS, sb = tid / TB, tb = tid % TB;
    CX* imgb = reinterpret_cast<CX*>(smem_raw) + (size_t)sb * CB::IMG;   // the slot's image
    CX* imgs = imgb + (ss % R) * SIMG;                                    // this sub-slot's part of it
    unsigned* s_next = reinterpret_cast<unsigned*>(smem_raw + (size_t)SLOTS * CB::IMG * sizeof(CX));

    typename KS::Tw ws;
    typename KB::Tw wb;
    KS::load_tw(ws, ts, tws, tws);
    KB::load_tw(wb, tb, twb, twb);

    const bool dyn = ctr != nullptr;
    unsigned g = blockIdx.x;
    unsigned pend = blockIdx.x + gridDim.x;   // hand-out: pf_handout.h
    __syncthreads();
    const size_t last = (size_t)batch - 1;
    const size_t in_row = (size_t)(UP ? nS : nB) * SPP, out_row = (size_t)(UP ? nB : nS) * SPP;
    float raw[LD::RAWN];
    {
        const size_t r0 = UP ? (size_t)g * G + ss : (size_t)g * G + (size_t)sb * R;
        LD::load(raw, in + (r0 < last ? r0 : last) * in_row, UP ? ts : tb);
    }
    for (unsigned it = 0; (size_t)g * G < batch; ++it) {
        if (dyn && tid == 0) pend = handout_grab(s_next, it, pend, ctr);
        unsigned gn = g;
        CX gq[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) gq[i] = mk<float>(0.0f, 0.0f);
        if constexpr (UP) {
            // ---- R rows forward at once, one per sub-slot
            CX v[16];
            LD::unpack(raw, v);
            KS::template butterflies<0>(v, ts, ws, tws);
            KS::template xwrite<0>(v, ts, imgs);
            __syncthreads();  // publishes s_next; first half of exchange 0
            gn = handout_next(dyn, s_next, it, g);
            const size_t rn = (size_t)gn * G + ss;
            if constexpr (PF) LD::load(raw, in + (rn < last ? rn : last) * in_row, ts);
            resample_finish<KS, CS>(v, ts, ws, tws, imgs);
            // ---- park the spectrum in natural order (the sub-image is free: the last exchange ended with its read-side xsync)
#pragma unroll
            for (int d = 0; d < 8; ++d) lds_st2(imgs + 2 * ts + d * (nS / 8), v[d], v[8 + d]);
            KB::xsync();
            // ---- every non-zero first-stage operand of the R backward transforms: 16 / R pairs per row
#pragma unroll
            for (int p = 0; p < R; ++p)
#pragma unroll
                for (int c = 0; c < NPR; ++c) {
                    const vec4<float> x = lds_ld2(imgb + p * SIMG + 2 * tb + c * (nB / 8));
                    gq[2 * (p * NPR + c)] = mk<float>(x.x, x.y);
                    gq[2 * (p * NPR + c) + 1] = mk<float>(x.z, x.w);
                }
            KB::xsync();
            // ---- R backward transforms through the whole image, one row each
#pragma unroll 1
            for (int p = 0; p < R; ++p) {
                resample_spread<R, TB>(gq, v, tb);
                resample_shift<R>(gq);
                resample_whole<KB, CB>(v, tb, wb, twb, imgb);
                const size_t row = (size_t)g * G + (size_t)sb * R + p;
                if (row < batch) ST::store(v, out + row * out_row, tb, s);
            }
            if constexpr (!PF) LD::load(raw, in + (rn < last ? rn : last) * in_row, ts);
        } else {
            // ---- R forward transforms through the whole image, the next row requested one transform ahead
#pragma unroll 1
            for (int p = 0; p < R; ++p) {
                CX v[16];
                LD::unpack(raw, v);
                KB::template butterflies<0>(v, tb, wb, twb);
                KB::template xwrite<0>(v, tb, imgb);
                __syncthreads();  // pass 0: publishes s_next; first half of exchange 0
                gn = handout_next(dyn, s_next, it, g);
                if (PF || p + 1 < R) {
                    const size_t rn = p + 1 < R ? (size_t)g * G + (size_t)sb * R + p + 1 : (size_t)gn * G + (size_t)sb * R;
                    LD::load(raw, in + (rn < last ? rn : last) * in_row, tb);
                }
                resample_finish<KB, CB>(v, tb, wb, twb, imgb);
                resample_shift<R>(gq);
                resample_keep<R, TB>(v, gq, tb);
            }
            // ---- park the R cropped spectra in natural order, one per sub-image
#pragma unroll
            for (int p = 0; p < R; ++p)
#pragma unroll
                for (int c = 0; c < NPR; ++c) lds_st2(imgb + p * SIMG + 2 * tb + c * (nB / 8), gq[2 * (p * NPR + c)], gq[2 * (p * NPR + c) + 1]);
            KB::xsync();
            // ---- R rows backward at once: first-stage operands at stride nS / 8
            CX v[16];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const vec4<float> x = lds_ld2(imgs + 2 * ts + q * (nS / 8));
                v[q] = mk<float>(x.x, x.y);
                v[8 + q] = mk<float>(x.z, x.w);
            }
            KS::xsync();
            resample_whole<KS, CS>(v, ts, ws, tws, imgs);
            const size_t row = (size_t)g * G + ss;
            if (row < batch) ST::store(v, out + row * out_row, ts, s);
            KB::xsync();   // the next pass writes the whole image
            if constexpr (!PF) {
                const size_t rn = (size_t)gn * G + (size_t)sb * R;
                LD::load(raw, in + (rn < last ? rn : last) * in_row, tb);
            }
        }
        g = gn;
    }
    if (dyn && tid == 0) handout_rearm(ctr);
}

}  // namespace pf
