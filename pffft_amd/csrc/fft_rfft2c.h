// Batched 2-D spectral convolution of REAL images on the rfft2 handle (include/pffft_hip.h: pffft[d]_hip_rfft2_convolve_batch):
//     out = s rows cols irfft2( rfft2(in) . G ),  G = H or conj(H),
// of dense row-major images of rows x cols reals, H a half-spectrum of rows x (cols / 2 + 1) interleaved complex values in natural order
// (one for every image of the batch, or one per image), irfft2 with numpy's rule: only the Hermitian part along u of the product's
// columns 0 and cols / 2 counts.  The COMPOSED route is host code (rfft2_tu.hip): the handle's forward transform into a scratch of
// half-spectra, fft2conv_product_kernel of fft_fft2c.h in place there, the handle's backward transform.  This file holds
//   fft_rfft2conv_kernel   the FUSED route (float, broadcast H, rows in {16, 32, 64}, cols in {32, 64}): fft_rfft2_kernel's persistent
//                          loop (the hand-out of pf_handout.h, inactive slots, chunked 16-byte loads and stores;
//                          the launch is loop_launch with CONV_ONESHOT) on Rfft2Cfg / Rfft2Layout as they are, ONE HBM read and ONE HBM
//                          write of 4 rows cols bytes per image.
// The routes run different butterfly networks: each is held to the float64 truth at the convolution bar, not to the other bit for bit.
//
// The fused kernel, per image (H = cols / 2, HP the pitch of a half line):
//   load       as fft_rfft2_kernel forward: rows 2 l and 2 l + 1 are the real and imaginary parts of line l.
//   rows       forward over rows / 2 lines, fft2_axis as it is (a 64-point line ends in base-8 digit-reversed positions).
//   untangle   as fft_rfft2_kernel forward: rows half lines of H points in NATURAL order, position 0 the packed column
//              Q = col_0 + j col_H (both real sequences along the rows).
//   columns    rfft2conv_columns, the H columns at pitch HP: forward, x G, backward, in the manner of fft2conv_columns of fft_fft2c.h.
//              R < 64: a column is one thread's registers, ONE LDS round trip.  R = 64: forward half pass, a barrier, the second forward
//              half pass leaves X[k1 + 8 k2] in register k2 of group k1, x G, then the transposed 8 x 8 network (fft2_half_t2): the rows
//              come out at natural positions.  G[u][v] is read at the natural v: the untangling step undid the digit reversal.
//   rebuild    Z = A + j B of the backward direction of fft_rfft2_kernel, reading the half lines 2 l and 2 l + 1 at NATURAL positions.
//   rows       backward over rows / 2 lines (fft2_axis; a 64-point line ends digit-reversed, which the store undoes as the backward
//              store of fft_rfft2_kernel does).
//   store      the real parts are row 2 l, the imaginary parts row 2 l + 1, times s (one product per component; s = 1 changes no bit).
//
// THE PACKED COLUMN.  With FQ the forward transform of Q along the rows and u' = (rows - u) mod rows,
//     X0[u] = (FQ[u] + conj FQ[u']) / 2,   XH[u] = (FQ[u] - conj FQ[u']) / (2 j)
// are the columns 0 and H of the image's half-spectrum; X0[u'] = conj X0[u] and XH[u'] = conj XH[u] hold bit for bit.  What goes into the
// backward transform is  Y[u] = Herm(X0 G[.][0])[u] + j Herm(XH G[.][H])[u],  Herm(P)[u] = (P[u] + conj P[u']) / 2 - numpy's rule - with
// every product through fft2conv_mul_g.  A thread forms it from FQ[u], FQ[u'] and the four values G[u][0], G[u'][0], G[u][H], G[u'][H],
// which it reads from H (L2) in every form: HREG 1 keeps only the interior columns' values in registers.
//   R < 64   u and u' sit in the registers of the one thread that owns column position 0; it forms Y[u] and Y[u'] together.
//   R = 64   X[k1 + 8 k2] and its partner sit in the groups k1 and (8 - k1) mod 8 (other waves for 64 x 64).  CHOICE: an exchange through
//            the spare positions of the half lines (HP > H; the forward direction leaves them unused): the eight threads of column 0
//            write FQ[k1 + 8 k2] to (row position 8 k1 + k2, H + x(k1)), ONE extra barrier per image, then read FQ[u'] from
//            (8 k1' + k2', H + x(k1')), k1' = (8 - k1) mod 8, k2' = (8 - k2) mod 8 where k1 = 0, else 7 - k2.  x(k1) = k1 / 4 where a half
//            line has two spare positions (64 x 32: the groups k1 and k1 + 4 would meet on one bank pair, 2.2-way with the other slot),
//            else 0.  Nothing else touches those positions, so no second barrier is needed before the column's results are written.  Carrying the two columns unpacked instead would make H + 1
//            columns, which the thread groups do not divide.
//
// G.  HREG 1: the values of a thread's columns are loaded once per workgroup and stay in registers across the loop (conjugation applied);
// HREG 0: re-read per group from L2 at the same indices (H is at most 16.5 KiB and every workgroup reads all of it).  PF: the next
// group's chunks are requested before the column step (1) or behind the store (0).  The resource table of every form is
// tools/rfft2_resources.py's; the RFFT2CONV_FORM table below follows from it.
// IN PLACE (in == out): an image is wholly in LDS or registers before any of it is stored, and images do not overlap.
//
// LDS banks (tools/rfft2_lds.py, the layouts of fft_rfft2.h untouched): no access is worse than 2-way.
//
// Out of scope: an accumulate form, linear (zero-padded) convolution and cropping, two images that both change per call, a fused
// per-image-H path, fused double, cols = 16, shapes beyond 64, strided images.
#pragma once
#include "fft_fft2c.h"
#include "fft_rfft2.h"
#include "pf_handout.h"

namespace pf {

// The form per shape, (rows, cols, PF, HREG), from the resource remarks of all four forms of every shape (tools/rfft2_resources.py; the
// table of DESIGN.md §3.30): a form qualifies with no scratch and waves per SIMD not below what the LDS images allow anyway.  Four
// shapes have one qualifying form, PF 0 HREG 0.  The others were timed on the device at 64 MiB of images: in 16 x 32 PF 0 beats PF 1 by
// 4 us of 58 and HREG makes no difference; in 64 x 32 PF 1 HREG 0 and PF 0 HREG 0 cannot be told apart, and the one with fewer
// registers stays.
template <int R, int C> struct Rfft2ConvForm;
#define RFFT2CONV_FORM(R_, C_, PF_, HREG_) \
    template <> struct Rfft2ConvForm<R_, C_> { static constexpr int PF = PF_, HREG = HREG_; };
RFFT2CONV_FORM(16, 32, 0, 0)
RFFT2CONV_FORM(16, 64, 0, 0)
RFFT2CONV_FORM(32, 32, 0, 0)
RFFT2CONV_FORM(32, 64, 0, 0)
RFFT2CONV_FORM(64, 32, 0, 0)
RFFT2CONV_FORM(64, 64, 0, 0)
#undef RFFT2CONV_FORM

// values of G a thread holds (HREG 1): g[0 ... PT - 1], in the order its column step meets them.  The values of column 0 are loaded
// like the others and never read: the packed column reads H.
template <int R, int C>
__device__ __forceinline__ void rfft2conv_load_g(cx<float>* g, const cx<float>* __restrict__ H, int t, int conj_h) {
    typedef Rfft2Cfg<R, C> Cf;
    constexpr int T = Cf::T, NC = Cf::H, BINS = Cf::BINS;
    if constexpr (R < 64) {
#pragma unroll
        for (int i = 0; i < NC / T; ++i) {
            const int v = t + T * i;
#pragma unroll
            for (int u = 0; u < R; ++u) g[i * R + u] = fft2conv_conj(H[u * BINS + v], conj_h);
        }
    } else {
        constexpr int G = T / 8;
        const int k1 = t / G, l0 = t % G;
#pragma unroll
        for (int i = 0; i < NC / G; ++i) {
            const int v = l0 + G * i;
#pragma unroll
            for (int k2 = 0; k2 < 8; ++k2) g[i * 8 + k2] = fft2conv_conj(H[(k1 + 8 * k2) * BINS + v], conj_h);
        }
    }
}

// Y[u] of the packed column from a = FQ[u], b = FQ[u'] and the rows gu, gp of H at u and u' (BINS values each); see THE PACKED COLUMN.
// Y[u'] = conj Herm(X0 G0)[u] + j conj Herm(XH GH)[u] comes out with it.
template <int NC>
__device__ __forceinline__ void rfft2conv_packed(const cx<float> a, const cx<float> b, const cx<float>* __restrict__ gu,
                                                 const cx<float>* __restrict__ gp, int conj_h, cx<float>& yu, cx<float>& yp) {
    typedef cx<float> CX;
    const CX x0 = mk<float>(0.5f * (a.x + b.x), 0.5f * (a.y - b.y)), xh = mk<float>(0.5f * (a.y + b.y), 0.5f * (b.x - a.x));
    const CX p0 = fft2conv_mul_g(x0, fft2conv_conj(gu[0], conj_h)), q0 = fft2conv_mul_g(mk<float>(x0.x, -x0.y), fft2conv_conj(gp[0], conj_h));
    const CX ph = fft2conv_mul_g(xh, fft2conv_conj(gu[NC], conj_h)), qh = fft2conv_mul_g(mk<float>(xh.x, -xh.y), fft2conv_conj(gp[NC], conj_h));
    const CX h0 = mk<float>(0.5f * (p0.x + q0.x), 0.5f * (p0.y - q0.y)), hh = mk<float>(0.5f * (ph.x + qh.x), 0.5f * (ph.y - qh.y));
    yu = mk<float>(h0.x - hh.y, h0.y + hh.x);
    yp = mk<float>(h0.x + hh.y, hh.x - h0.y);
}

// The column step: forward over the H columns of the half lines, x G, backward; rows at natural positions in and out.
template <int R, int C, int HREG>
__device__ __forceinline__ void rfft2conv_columns(cx<float>* img, int t, const cx<float> (&w)[8], const cx<float>* g, const cx<float>* __restrict__ H,
                                                  int conj_h) {
    typedef Rfft2Cfg<R, C> Cf;
    constexpr int T = Cf::T, HP = Cf::HP, NC = Cf::H, BINS = Cf::BINS;
    if constexpr (R < 64) {
        static_assert(NC % T == 0, "whole columns per thread");
#pragma unroll
        for (int i = 0; i < NC / T; ++i) {
            const int v = t + T * i;
            cx<float>* p = img + v;
            cx<float> a[R];
#pragma unroll
            for (int q = 0; q < R; ++q) a[q] = p[q * HP];
            dftR<R, FWD>(a);
            if (i == 0 && t == 0) {   // the packed column
#pragma unroll
                for (int u = 0; u <= R / 2; ++u) {
                    const int up = (R - u) & (R - 1);
                    cx<float> yu, yp;
                    rfft2conv_packed<NC>(a[u], a[up], H + u * BINS, H + up * BINS, conj_h, yu, yp);
                    a[u] = yu;
                    if (up != u) a[up] = yp;
                }
            } else {
#pragma unroll
                for (int u = 0; u < R; ++u) a[u] = fft2conv_mul_g(a[u], HREG ? g[i * R + u] : fft2conv_conj(H[u * BINS + v], conj_h));
            }
            dftR<R, BWD>(a);
#pragma unroll
            for (int q = 0; q < R; ++q) p[q * HP] = a[q];
        }
    } else {
        constexpr int G = T / 8;
        constexpr int SP = HP - NC >= 2 ? 2 : 1;   // spare positions the exchange spreads over: groups k1 and k1 + 4 share their banks at one
        static_assert(T % 8 == 0 && NC % G == 0, "eight thread groups, whole columns per thread");
        const int j = t / G, l0 = t % G;   // j in the first half pass, k1 in the second
#pragma unroll
        for (int i = 0; i < NC / G; ++i) {
            cx<float>* p = img + (l0 + G * i) + j * HP;
            cx<float> a[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) a[q] = p[8 * q * HP];
            dft8<FWD>(a);
#pragma unroll
            for (int k = 1; k < 8; ++k) a[k] = twmul<FWD>(a[k], w[k]);
#pragma unroll
            for (int k = 0; k < 8; ++k) p[8 * k * HP] = a[k];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NC / G; ++i) {
            const int v = l0 + G * i;
            cx<float>* p = img + v + 8 * j * HP;
            cx<float> a[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) a[q] = p[q * HP];
            dft8<FWD>(a);                                                    // a[k2] = X[k1 + 8 k2]
            if (i == 0) {
                // the packed column's exchange through the spare position H: uniform barrier, eight threads of an image take part
                if (l0 == 0) {
#pragma unroll
                    for (int k2 = 0; k2 < 8; ++k2) p[k2 * HP + NC + (j >> 2) % SP] = a[k2];
                }
                __syncthreads();
            }
            if (i == 0 && l0 == 0) {
                const int kp = (8 - j) & 7;
#pragma unroll
                for (int k2 = 0; k2 < 8; ++k2) {
                    const int k2p = j == 0 ? (8 - k2) & 7 : 7 - k2;
                    const int u = j + 8 * k2, up = kp + 8 * k2p;
                    const cx<float> b = img[(8 * kp + k2p) * HP + NC + (kp >> 2) % SP];
                    cx<float> yu, yp;
                    rfft2conv_packed<NC>(a[k2], b, H + u * BINS, H + up * BINS, conj_h, yu, yp);
                    a[k2] = yu;
                }
            } else {
#pragma unroll
                for (int k2 = 0; k2 < 8; ++k2)
                    a[k2] = fft2conv_mul_g(a[k2], HREG ? g[i * 8 + k2] : fft2conv_conj(H[(j + 8 * k2) * BINS + v], conj_h));
            }
            dft8<BWD>(a);                                                    // k2 -> j
#pragma unroll
            for (int k = 1; k < 8; ++k) a[k] = twmul<BWD>(a[k], w[k]);
#pragma unroll
            for (int k = 0; k < 8; ++k) p[k * HP] = a[k];
        }
        __syncthreads();
        fft2_half_t2<NC, 1, HP, T>(img, t);
    }
}

// waves per SIMD the LDS images allow (a workgroup is four waves, one per SIMD; 160 KiB of LDS per CU): the register budget asked of the
// compiler, which otherwise spends up to 512 registers per lane on overlapping the unrolled columns
template <int R, int C> constexpr int rfft2conv_waves() {
    constexpr int by_lds = (int)((size_t)160 * 1024 / Rfft2Cfg<R, C>::LDS_BYTES);
    return by_lds < 8 ? by_lds : 8;
}

template <int R, int C, int PF, int HREG>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(rfft2conv_waves<R, C>())))
fft_rfft2conv_kernel(const float* in, const cx<float>* __restrict__ H, float* out, unsigned batch, float s, int conj_h,
                     const cx<float>* __restrict__ tw64, unsigned* ctr) {
    typedef Rfft2Cfg<R, C> Cf;
    typedef cx<float> CX;
    typedef vec4<float> chunk;
    constexpr int T = Cf::T, HF = Cf::H, HP = Cf::HP, PITCH = Cf::PITCH, SLOTS = Cf::SLOTS, NPAIR = Cf::NPAIR, NI = Cf::NI_REAL;
    constexpr size_t IMAGE = (size_t)R * C;   // scalars of one image
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int slot = threadIdx.x / T, t = threadIdx.x % T;
    CX* img = reinterpret_cast<CX*>(smem_raw) + (size_t)slot * Cf::IMG;
    float* imgf = reinterpret_cast<float*>(img);
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
    if constexpr (HREG) rfft2conv_load_g<R, C>(g_, H, t, conj_h);

    const bool dyn = ctr != nullptr;
    unsigned g = blockIdx.x;
    unsigned pend = blockIdx.x + gridDim.x;   // hand-out: pf_handout.h
    const size_t last = (size_t)batch - 1;
    chunk raw[NI];
    auto load = [&](size_t image) {
        const chunk* src = reinterpret_cast<const chunk*>(in + image * IMAGE);
        int tl = t;
        asm volatile("" : "+v"(tl));   // (as tt in the loop below)
#pragma unroll
        for (int i = 0; i < NI; ++i) raw[i] = __builtin_nontemporal_load(src + tl + T * i);
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
        // tt is t made opaque once per pass: the LDS addresses of a pass are then formed next to their use.  Left to itself the compiler
        // hoists every one of them out of the persistent loop and, at the register budget of rfft2conv_waves, spills them.
        int tt = t;
        asm volatile("" : "+v"(tt));
        // ---- the image into LDS (free: the previous pass ended with a barrier behind its last read)
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int e = 4 * (tt + T * i), r = e / C, c = e % C;
            float* p = imgf + 2 * ((r >> 1) * PITCH + c) + (r & 1);
            // the four reals in an order rotated by tt / 4, as in fft_rfft2_kernel
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int jj = (j + (tt >> 2)) & 3;
                p[2 * jj] = jj == 0 ? raw[i].x : jj == 1 ? raw[i].y : jj == 2 ? raw[i].z : raw[i].w;
            }
        }
        __syncthreads();  // publishes s_next
        const unsigned gn = handout_next(dyn, s_next, it, g);
        // the next image's index is formed where its chunks are requested: one register (gn) crosses the pass, not a 64-bit index
        auto next_image = [&]() {
            const size_t tn = (size_t)gn * SLOTS + slot;
            return tn < last ? tn : last;
        };
        // ---- rows forward: R / 2 lines of C points, 1 apart, PITCH from line to line
        fft2_axis<C, R / 2, PITCH, 1, T, FWD>(img, tt, w);
        __syncthreads();
        // ---- untangle the two rows of every line, into half lines in natural order
        {
            CX za[NPAIR], zb[NPAIR];
#pragma unroll
            for (int i = 0; i < NPAIR; ++i) {
                const int k = tt + T * i, l = k / HF, v = k % HF;
                const CX* p = img + l * PITCH;
                za[i] = p[fft2_pos<C>(v)];
                zb[i] = p[fft2_pos<C>(v == 0 ? HF : C - v)];
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < NPAIR; ++i) {
                const int k = tt + T * i, l = k / HF, v = k % HF;
                const CX a = za[i], b = zb[i];
                CX A = mk<float>(0.5f * (a.x + b.x), 0.5f * (a.y - b.y)), B = mk<float>(0.5f * (a.y + b.y), 0.5f * (b.x - a.x));
                if (v == 0) { A = mk<float>(a.x, b.x); B = mk<float>(a.y, b.y); }   // the packed column: A[0] + j A[H], B[0] + j B[H]
                img[(2 * l) * HP + v] = A;
                img[(2 * l + 1) * HP + v] = B;
            }
        }
        __syncthreads();
        if constexpr (PF) load(next_image());
        // ---- columns: forward, x G, backward; natural positions out
        rfft2conv_columns<R, C, HREG>(img, tt, w, g_, H, conj_h);
        __syncthreads();
        // ---- rebuild the lines Z = A + j B of two rows each, natural order
        {
            CX qa[NPAIR], qb[NPAIR];
#pragma unroll
            for (int i = 0; i < NPAIR; ++i) {
                const int k = tt + T * i, l = k / HF, v = k % HF;
                qa[i] = img[(2 * l) * HP + v];
                qb[i] = img[(2 * l + 1) * HP + v];
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < NPAIR; ++i) {
                const int k = tt + T * i, l = k / HF, v = k % HF;
                const CX A = qa[i], B = qb[i];
                CX* p = img + l * PITCH;
                if (v == 0) {   // the packed column: A[0] = Re, A[H] = Im
                    p[0] = mk<float>(A.x, B.x);
                    p[HF] = mk<float>(A.y, B.y);
                } else {
                    p[v] = mk<float>(A.x - B.y, A.y + B.x);
                    p[C - v] = mk<float>(A.x + B.y, B.x - A.y);
                }
            }
        }
        __syncthreads();
        // ---- rows backward: R / 2 lines of C points
        fft2_axis<C, R / 2, PITCH, 1, T, BWD>(img, tt, w);
        __syncthreads();
        // ---- store: the real parts are row 2 l, the imaginary parts row 2 l + 1
        if (active) {
            chunk* dst = reinterpret_cast<chunk*>(out + dv * IMAGE);
            asm volatile("" : "+v"(tt));
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int e = 4 * (tt + T * i), r = e / C, c = e % C;
                const float* p = imgf + 2 * ((r >> 1) * PITCH) + (r & 1);
                chunk o;
                o.x = s * p[2 * fft2_pos<C>(c)]; o.y = s * p[2 * fft2_pos<C>(c + 1)];
                o.z = s * p[2 * fft2_pos<C>(c + 2)]; o.w = s * p[2 * fft2_pos<C>(c + 3)];
                __builtin_nontemporal_store(o, dst + tt + T * i);
            }
        }
        __syncthreads();
        if constexpr (!PF) load(next_image());
        g = gn;
    }
    if (dyn && threadIdx.x == 0) handout_rearm(ctr);
}

}  // namespace pf
