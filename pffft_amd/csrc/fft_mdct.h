// MDCT / IMDCT frames and the type-IV cosine transform (pffft[d]_hip_mdct_*): the kernels.  The core is the type-IV cosine sum on ONE
// complex transform of half the length (include/pffft_hip.h; M coefficients, h = n = M/2):
//   C4(u)[k] = sum_i u[i] cos(pi (2k+1)(2i+1) / 4M):   z[m] = (u[2m] + j u[M-1-2m]) a_m;  Z = forward complex transform of z (length n);
//              y_k = Z_k b_k;  C4[2k] = Re y_k, C4[M-1-2k] = -Im y_k;   a_m = exp(-j pi (4m+1) / 4M), b_k = exp(-j pi k / M)
//   fold (forward MDCT of a frame p of 2M windowed samples): u[i] = (-p[3h-1-i]) - p[3h+i], u[h+i] = p[i] - p[M-1-i], i < h
//   unfold (IMDCT): v = C4(X), y = (v2, -reverse(v2), -reverse(v1), -v1) with v1 = v[0..h), v2 = v[h..M), then the overlap-add
// In 16-byte chunks of four reals the input pairing is chunk c with chunk M/4-1-c: points 2c and 2c+1 take (u[4c], u[M-1-4c]) and
// (u[4c+2], u[M-3-4c]); the output pairing is the same: chunk c of the result is (Re y_2c, -Im y_(n-1-2c), Re y_(2c+1), -Im y_(n-2-2c)).
//
//   fft_mdct_kernel     the FUSED route - the register-tiled complex forward transform of fft_tiled.h between two round trips through
//                       the transform's own LDS image, both of LINEAR 16-byte accesses: every thread loads the chunks of its own
//                       stage-0 operands from HBM (the frame policy folds them in registers), writes them to chunk slot c and reads the
//                       mirrored slot n/2-1-c; behind the transform it writes its products y to slot c and reads slot n/2-1-c again.
//                       Lane t of a transform touches slot t + const or const - t, consecutive 16-byte slots without padding: the
//                       writes (8 lanes per access group) are conflict-free, the reads (16 lanes per group) are conflict-free at 32
//                       threads per transform and 2-way at 16, where a group spans two images (DESIGN.md §3.19 has the count).  A kernel
//                       of its own built from the Tiled<> helpers:
//                       fft_tiled_kernel keeps its code.  Everything between the a-product and the b-product is the sequence of
//                       fft_tiled_kernel<C, FWD, 0>, both products are mdct_mul (cxmath.h): the result equals the composed route's bit
//                       for bit (tests/test_gpu_mdct.py).
//   mdct_fold_kernel, mdct_post_kernel, mdct_ola_kernel
//                       the streaming kernels of the COMPOSED route around transform_batch (canonical layout) in a scratch image, and
//                       the output-stationary overlap-add gather of both routes.
#pragma once
#include "fft_tiled.h"
#include "fft_dct.h"   // Quad, Duo
#include "pf_handout.h"

namespace pf {

enum { MDCT_ROW = 0, MDCT_FRAME = 1 };   // loader policies: dense / pitched rows of M reals; frames of 2M samples at hop M

// u[4c ... 4c+3] of the frame at p (2M samples, window NULL: no product) from two chunks: A read forward, B read backward
template <typename T>
__device__ __forceinline__ Quad<T> mdct_fold4(Quad<T> A, Quad<T> B, bool low) {
    Quad<T> u;
#pragma unroll
    for (int e = 0; e < 4; ++e) u.v[e] = low ? (-B.v[3 - e]) - A.v[e] : A.v[e] - B.v[3 - e];
    return u;
}
// four scalars from p: one 16-byte (float) / two 16-byte (double) accesses where WIDE, else scalar accesses
template <typename T, bool WIDE>
__device__ __forceinline__ Quad<T> mdct_ld4(const T* p) {
    if constexpr (WIDE) return *reinterpret_cast<const Quad<T>*>(p);
    else {
        Quad<T> q;
#pragma unroll
        for (int e = 0; e < 4; ++e) q.v[e] = p[e];
        return q;
    }
}
template <typename T, bool WIDE>
__device__ __forceinline__ void mdct_st4(T* p, Quad<T> q) {
    if constexpr (WIDE) *reinterpret_cast<Quad<T>*>(p) = q;
    else {
#pragma unroll
        for (int e = 0; e < 4; ++e) p[e] = q.v[e];
    }
}
// chunk c of u for either policy: the row itself, or the fold of the windowed frame (each product rounded once, each fold one subtraction)
template <typename T, int LOAD, bool WIDE>
__device__ __forceinline__ Quad<T> mdct_u4(const T* src, const T* window, unsigned c, unsigned M) {
    if constexpr (LOAD == MDCT_ROW) return mdct_ld4<T, WIDE>(src + 4 * c);
    else {
        const unsigned h = M / 2, i = 4 * c;
        const bool low = i < h;
        const unsigned fwd = low ? 3 * h + i : i - h, rev = low ? 3 * h - 4 - i : M - 4 - (i - h);
        Quad<T> A = mdct_ld4<T, WIDE>(src + fwd), B = mdct_ld4<T, WIDE>(src + rev);
        if (window) {
            const Quad<T> wa = mdct_ld4<T, true>(window + fwd), wb = mdct_ld4<T, true>(window + rev);
#pragma unroll
            for (int e = 0; e < 4; ++e) { A.v[e] = wa.v[e] * A.v[e]; B.v[e] = wb.v[e] * B.v[e]; }
        }
        return mdct_fold4<T>(A, B, low);
    }
}

// ------------------------------------------------------------------------------------------------ fused route
// Tables resident in registers across the persistent loop: 2 = a and b, 1 = a, 0 = none - the most that the resource remarks of the
// instantiation show without scratch under 2 waves per SIMD (256 VGPRs; DESIGN.md §3.19 has the table of all twelve builds).
__host__ __device__ constexpr int mdct_resident_tables(int n, int load) {
    return n == 512 ? (load == MDCT_ROW ? 2 : 0) : 1;
}
// gain: 1 or 2 (the exact doubling of the dct4 entry), the last operation.  nframes: frames per signal (MDCT_FRAME).
template <class C, int LOAD>
__global__ void __launch_bounds__(C::WG_THREADS, C::OCC)
fft_mdct_kernel(const float* in, size_t in_stride, unsigned nframes, const float* __restrict__ window, float* out, size_t out_stride,
                unsigned batch, float gain, const cx<float>* __restrict__ tab_a, const cx<float>* __restrict__ tab_b,
                const cx<float>* __restrict__ twg, unsigned* ctr) {
    typedef float T;
    typedef cx<T> CX;
    typedef Tiled<C, FWD, 0> K;
    typedef typename K::S0 S0;
    typedef typename K::SL SL;
    constexpr int n = C::n, M = 2 * C::n, E = C::E, TPT = C::TPT, NCH = C::NCH;
    constexpr int R0 = K::R0, RL = K::RL;
    constexpr int QCH = n / 4;   // chunks per quarter frame (h = n samples)
    static_assert(sizeof(typename C::real_t) == 4 && C::VEC == 2 && S0::PAIR && SL::PAIR, "float configurations only");
    static_assert(C::TWMODE == 0 || C::TWMODE == 3, "register twiddles only");
    static_assert(C::IMG >= n, "the linear image of n points");
    // chunk plain_chunk(t, i) = t + (i mod R0) n/(2 R0) lies in the first half of u (the quarters c and d of a frame) for i mod R0 < R0/2
    static_assert(S0::B == 2 && 2 * R0 * TPT == n, "one chunk pair per stage-0 operand, a thread's chunks n/(2 R0) apart");
    auto low_chunk = [](int i) { return i % R0 < R0 / 2; };
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int slot = threadIdx.x / TPT, t = threadIdx.x % TPT;
    CX* img = reinterpret_cast<CX*>(smem_raw) + (size_t)slot * C::IMG;
    chunk16* im16 = reinterpret_cast<chunk16*>(img);
    unsigned* s_next = reinterpret_cast<unsigned*>(smem_raw + (size_t)C::T_PER_WG * C::IMG * sizeof(CX));
    chunk16* wtab = reinterpret_cast<chunk16*>(smem_raw + (size_t)C::T_PER_WG * C::IMG * sizeof(CX) + 16);

    typename K::Tw w;
    K::load_tw(w, t, twg, nullptr);
    const CX* twt = twg;
    // a_m of the thread's own stage-0 chunks and b_k of its own chunks behind the last stage depend on the thread index only: they are
    // loaded once, before the loop, where the registers hold them without a spill (mdct_resident_tables), and from the table (8n bytes
    // each, L1 / L2 hits) where they are used otherwise
    constexpr int TABS = mdct_resident_tables(n, LOAD);
    constexpr bool A_RES = TABS >= 1, B_RES = TABS >= 2;
    const chunk16* ta16 = reinterpret_cast<const chunk16*>(tab_a);
    const chunk16* tb16 = reinterpret_cast<const chunk16*>(tab_b);
    chunk16 ta[A_RES ? NCH : 1], tb[B_RES ? NCH : 1];
    if constexpr (A_RES) {
#pragma unroll
        for (int i = 0; i < NCH; ++i) ta[i] = ta16[K::plain_chunk(t, i)];
    }
    if constexpr (B_RES) {
#pragma unroll
        for (int ii = 0; ii < SL::B / 2; ++ii)
#pragma unroll
            for (int d = 0; d < RL; ++d) tb[ii * RL + d] = tb16[t + TPT * ii + d * (n / (2 * RL))];
    }
    const bool windowed = LOAD == MDCT_FRAME && window != nullptr;
    if (windowed)
        for (int i = threadIdx.x; i < n; i += C::WG_THREADS) wtab[i] = reinterpret_cast<const chunk16*>(window)[i];

    const bool dyn = ctr != nullptr;
    unsigned g = blockIdx.x;
    unsigned pend = blockIdx.x + gridDim.x;   // hand-out: pf_handout.h
    __syncthreads();
    const size_t last = (size_t)batch - 1;
    auto src_of = [&](size_t tr) -> const T* {
        const size_t v = tr < last ? tr : last;
        if constexpr (LOAD == MDCT_ROW) return in + v * in_stride;
        else {
            const unsigned i = (unsigned)v / nframes, f = (unsigned)v - i * nframes;
            return in + (size_t)i * in_stride + (size_t)f * M;
        }
    };
    // MDCT_ROW: raw[i] = chunk plain_chunk(t, i) of the row.  MDCT_FRAME: the two frame chunks that fold into it, forward one first.
    constexpr int NRAW = LOAD == MDCT_FRAME ? 2 * NCH : NCH;
    chunk16 raw[NRAW];
    auto load = [&](const T* src) {
        if constexpr (LOAD == MDCT_ROW) K::load_raw(raw, src, t, true);
        else {
            const chunk16* s16 = reinterpret_cast<const chunk16*>(src);
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int c = K::plain_chunk(t, i);
                raw[2 * i] = __builtin_nontemporal_load(s16 + (low_chunk(i) ? 3 * QCH + c : c - QCH));
                raw[2 * i + 1] = __builtin_nontemporal_load(s16 + (3 * QCH - 1 - c));
            }
        }
    };
    load(src_of((size_t)g * C::T_PER_WG + slot));
    for (unsigned it = 0; (size_t)g * C::T_PER_WG < batch; ++it) {
        if (dyn && threadIdx.x == 0) pend = handout_grab(s_next, it, pend, ctr);
        const size_t tr = (size_t)g * C::T_PER_WG + slot;
        const bool active = tr < batch;  // inactive slots recompute the last row and never store
        T* dst = out + (active ? tr : last) * out_stride;
        CX v[E];
        int tl = t;
        asm volatile("" : "+v"(tl));

        // ------------------------------------------------------------------ input round trip
        chunk16 u[NCH];
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            if constexpr (LOAD == MDCT_ROW) u[i] = raw[i];
            else {
                const int c = K::plain_chunk(tl, i);
                const bool low = low_chunk(i);
                chunk16 A = raw[2 * i], B = raw[2 * i + 1];
                if (windowed) {
                    const chunk16 wa = wtab[low ? 3 * QCH + c : c - QCH], wb = wtab[3 * QCH - 1 - c];
                    A.x = wa.x * A.x; A.y = wa.y * A.y; A.z = wa.z * A.z; A.w = wa.w * A.w;
                    B.x = wb.x * B.x; B.y = wb.y * B.y; B.z = wb.z * B.z; B.w = wb.w * B.w;
                }
                chunk16 f;
                f.x = low ? (-B.w) - A.x : A.x - B.w;
                f.y = low ? (-B.z) - A.y : A.y - B.z;
                f.z = low ? (-B.y) - A.z : A.z - B.y;
                f.w = low ? (-B.x) - A.w : A.w - B.x;
                u[i] = f;
            }
            im16[K::plain_chunk(tl, i)] = u[i];
        }
        K::xsync();
#pragma unroll
        for (int ii = 0; ii < S0::B / 2; ++ii)
#pragma unroll
            for (int q = 0; q < R0; ++q) {
                const int i = ii * R0 + q;
                const chunk16 m = im16[n / 2 - 1 - K::plain_chunk(tl, i)];
                const chunk16 a2 = A_RES ? ta[i] : ta16[K::plain_chunk(tl, i)];
                v[(2 * ii) * R0 + q] = mdct_mul(mk<T>(u[i].x, m.w), mk<T>(a2.x, a2.y));
                v[(2 * ii + 1) * R0 + q] = mdct_mul(mk<T>(u[i].z, m.y), mk<T>(a2.z, a2.w));
            }
        K::xsync();

        // ------------------------------------------------------------------ transform (the sequence of fft_tiled_kernel)
        K::template butterflies<0>(v, t, w, twt);
        if constexpr (C::NS > 1) K::template xwrite<0>(v, t, img);
        __syncthreads();  // publishes s_next; first half of exchange 0
        const unsigned gn = handout_next(dyn, s_next, it, g);
        if constexpr (C::PREFETCH) load(src_of((size_t)gn * C::T_PER_WG + slot));
        if constexpr (C::NS > 1) { K::template xread<0>(v, t, img); K::xsync(); K::template butterflies<1>(v, t, w, twt); }
        if constexpr (C::NS > 2) { K::template xwrite<1>(v, t, img); K::xsync(); K::template xread<1>(v, t, img); K::xsync(); K::template butterflies<2>(v, t, w, twt); }
        if constexpr (C::NS > 3) { K::template xwrite<2>(v, t, img); K::xsync(); K::template xread<2>(v, t, img); K::xsync(); K::template butterflies<3>(v, t, w, twt); }
        if constexpr (C::NS > 4) { K::template xwrite<3>(v, t, img); K::xsync(); K::template xread<3>(v, t, img); K::xsync(); K::template butterflies<4>(v, t, w, twt); }

        // ------------------------------------------------------------------ output round trip
#pragma unroll
        for (int ii = 0; ii < SL::B / 2; ++ii)
#pragma unroll
            for (int d = 0; d < RL; ++d) {
                const int c = tl + TPT * ii + d * (n / (2 * RL));
                const chunk16 b2 = B_RES ? tb[ii * RL + d] : tb16[c];
                const CX y0 = mdct_mul(v[(2 * ii) * RL + d], mk<T>(b2.x, b2.y));
                const CX y1 = mdct_mul(v[(2 * ii + 1) * RL + d], mk<T>(b2.z, b2.w));
                v[(2 * ii) * RL + d] = y0;
                v[(2 * ii + 1) * RL + d] = y1;
                chunk16 x; x.x = y0.x; x.y = y0.y; x.z = y1.x; x.w = y1.y;
                im16[c] = x;
            }
        K::xsync();
        chunk16* d16 = reinterpret_cast<chunk16*>(dst);
#pragma unroll
        for (int ii = 0; ii < SL::B / 2; ++ii)
#pragma unroll
            for (int d = 0; d < RL; ++d) {
                const int c = tl + TPT * ii + d * (n / (2 * RL));
                const chunk16 m = im16[n / 2 - 1 - c];   // bins n-2-2c and n-1-2c
                chunk16 o;
                o.x = gain * v[(2 * ii) * RL + d].x; o.y = gain * (-m.w);
                o.z = gain * v[(2 * ii + 1) * RL + d].x; o.w = gain * (-m.y);
                if (active) __builtin_nontemporal_store(o, d16 + c);
            }
        K::xsync();
        if constexpr (!C::PREFETCH) load(src_of((size_t)gn * C::T_PER_WG + slot));
        g = gn;
    }
    if (dyn && threadIdx.x == 0) handout_rearm(ctr);
}

// LDS of fft_mdct_kernel: the images and the counter slot of fft_tiled_kernel (these configurations have no twiddle table); the frame
// policy keeps the window (2M reals) behind them
template <class C> constexpr size_t mdct_lds_bytes(int load) {
    return (size_t)C::T_PER_WG * C::IMG * 2 * sizeof(float) + 16 + (load == MDCT_FRAME ? (size_t)C::n * 16 : 0);
}

// ------------------------------------------------------------------------------------------------ composed route
// rows v0 ... of the input -> the scratch rows the complex transform starts from: z[m] = (u[2m] + j u[M-1-2m]) a_m.  One thread per chunk
// pair (c, M/4-1-c), M/8 per row: two chunks of u in, the points 2c, 2c+1 and M/2-2-2c, M/2-1-2c out.  MDCT_ROW: row r at in + r
// in_stride.  MDCT_FRAME: frame v = v0 + r = i nframes + f at in + i in_stride + f M.  WIDE: 16-byte accesses of the input.
template <typename T, int LOAD, bool WIDE>
__global__ void mdct_fold_kernel(const T* __restrict__ in, size_t in_stride, size_t nframes, const T* __restrict__ window, T* __restrict__ X,
                                 const cx<T>* __restrict__ tab_a, size_t v0, size_t count, unsigned M) {
    const unsigned upr = M / 8;
    const size_t units = count * upr;
    for (size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x; x < units; x += (size_t)gridDim.x * blockDim.x) {
        const size_t r = x / upr;
        const unsigned c = (unsigned)(x - r * upr), cm = M / 4 - 1 - c;
        const T* src;
        if constexpr (LOAD == MDCT_ROW) src = in + (v0 + r) * in_stride;
        else {
            const size_t v = v0 + r, i = v / nframes, f = v - i * nframes;
            src = in + i * in_stride + f * M;
        }
        const Quad<T> ua = mdct_u4<T, LOAD, WIDE>(src, window, c, M), ub = mdct_u4<T, LOAD, WIDE>(src, window, cm, M);
        const Duo<cx<T>> aa = *reinterpret_cast<const Duo<cx<T>>*>(tab_a + 2 * c);
        const Duo<cx<T>> ab = *reinterpret_cast<const Duo<cx<T>>*>(tab_a + 2 * cm);
        const cx<T> z0 = mdct_mul(mk<T>(ua.v[0], ub.v[3]), aa.v[0]), z1 = mdct_mul(mk<T>(ua.v[2], ub.v[1]), aa.v[1]);
        const cx<T> z2 = mdct_mul(mk<T>(ub.v[0], ua.v[3]), ab.v[0]), z3 = mdct_mul(mk<T>(ub.v[2], ua.v[1]), ab.v[1]);
        Quad<T> o0, o1;
        o0.v[0] = z0.x; o0.v[1] = z0.y; o0.v[2] = z1.x; o0.v[3] = z1.y;
        o1.v[0] = z2.x; o1.v[1] = z2.y; o1.v[2] = z3.x; o1.v[3] = z3.y;
        T* dst = X + r * M;
        *reinterpret_cast<Quad<T>*>(dst + 4 * c) = o0;
        *reinterpret_cast<Quad<T>*>(dst + 4 * cm) = o1;
    }
}

// the transformed scratch rows -> rows of `out` (pitch out_stride): y_k = Z_k b_k, out[2k] = gain Re y_k, out[M-1-2k] = gain (-Im y_k).
// One thread per chunk pair (c, M/4-1-c): it reads and writes the same two chunk positions, so out may be the scratch itself.
template <typename T, bool WIDE>
__global__ void mdct_post_kernel(const T* X, T* out, size_t out_stride, const cx<T>* __restrict__ tab_b, T gain, size_t count, unsigned M) {
    const unsigned upr = M / 8;
    const size_t units = count * upr;
    for (size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x; x < units; x += (size_t)gridDim.x * blockDim.x) {
        const size_t r = x / upr;
        const unsigned c = (unsigned)(x - r * upr), cm = M / 4 - 1 - c;
        const T* src = X + r * M;
        const Quad<T> za = *reinterpret_cast<const Quad<T>*>(src + 4 * c), zb = *reinterpret_cast<const Quad<T>*>(src + 4 * cm);
        const Duo<cx<T>> ba = *reinterpret_cast<const Duo<cx<T>>*>(tab_b + 2 * c);
        const Duo<cx<T>> bb = *reinterpret_cast<const Duo<cx<T>>*>(tab_b + 2 * cm);
        const cx<T> y0 = mdct_mul(mk<T>(za.v[0], za.v[1]), ba.v[0]), y1 = mdct_mul(mk<T>(za.v[2], za.v[3]), ba.v[1]);
        const cx<T> y2 = mdct_mul(mk<T>(zb.v[0], zb.v[1]), bb.v[0]), y3 = mdct_mul(mk<T>(zb.v[2], zb.v[3]), bb.v[1]);
        Quad<T> o0, o1;
        o0.v[0] = gain * y0.x; o0.v[1] = gain * (-y3.y); o0.v[2] = gain * y1.x; o0.v[3] = gain * (-y2.y);
        o1.v[0] = gain * y2.x; o1.v[1] = gain * (-y1.y); o1.v[2] = gain * y3.x; o1.v[3] = gain * (-y0.y);
        T* dst = out + r * out_stride;
        mdct_st4<T, WIDE>(dst + 4 * c, o0);
        mdct_st4<T, WIDE>(dst + 4 * cm, o1);
    }
}

// overlap-add as a GATHER with a fixed order: sample s of signal i, s0 <= s < s1, is
//   scaling * ( sum over f ascending, 0 <= s - f M < 2M, of  window[s - f M] * y_f[s - f M] ),   y_f the unfold of v_f = C4(X_f),
// each product and each addition rounded once, the sum started from its first term.  `V` holds v of the frames fbase ... of every signal
// as dense rows (`fpitch` rows per signal).  One thread per four consecutive samples (they share a quarter frame); WIDE: one 16-byte
// store, else four scalar stores of the same values.
template <typename T, bool WIDE>
__global__ void mdct_ola_kernel(const T* __restrict__ V, size_t fbase, size_t fpitch, size_t nframes, unsigned M, const T* __restrict__ window,
                                T scaling, T* __restrict__ signal, size_t signal_stride, size_t nsignals, size_t s0, size_t s1) {
    const unsigned h = M / 2;
    const size_t per = (s1 - s0) / 4, total = nsignals * per;
    for (size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (size_t)gridDim.x * blockDim.x) {
        const size_t i = x / per, s = s0 + 4 * (x - i * per);
        const size_t fq = s / M;   // the frames that cover s: fq - 1 (second half) and fq (first half)
        Quad<T> acc = {};
        bool first = true;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (k == 0 ? fq < 1 : fq >= nframes) continue;
            const size_t f = k == 0 ? fq - 1 : fq;
            const unsigned j = (unsigned)(s - f * M), q = j / h, r = j - q * h;
            const T* v = V + (i * fpitch + (f - fbase)) * M;
            // q = 0: v[h + r + e];  1: -v[M-1-r-e];  2: -v[h-1-r-e];  3: -v[r + e]
            const bool rev = q == 1 || q == 2;
            const unsigned at = q == 0 ? h + r : q == 1 ? M - 4 - r : q == 2 ? h - 4 - r : r;
            const Quad<T> c = *reinterpret_cast<const Quad<T>*>(v + at);
            Quad<T> term;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const T y = rev ? c.v[3 - e] : c.v[e];
                term.v[e] = q == 0 ? y : -y;
            }
            if (window) {
                const Quad<T> wv = *reinterpret_cast<const Quad<T>*>(window + j);
#pragma unroll
                for (int e = 0; e < 4; ++e) term.v[e] = wv.v[e] * term.v[e];
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) acc.v[e] = first ? term.v[e] : acc.v[e] + term.v[e];
            first = false;
        }
        Quad<T> o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o.v[e] = first ? (T)0 : scaling * acc.v[e];
        mdct_st4<T, WIDE>(signal + i * signal_stride + s, o);
    }
}

}  // namespace pf
