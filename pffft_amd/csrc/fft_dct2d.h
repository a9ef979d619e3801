// Batched 2-D cosine / sine transforms of types II and III (include/pffft_hip.h: pffft[d]_hip_dct2d_*): the 1-D transform of the header's
// DCT definitions along the columns index (every row), then along the rows index, of dense row-major images of rows x cols reals -
// scipy.fft.dctn / dstn over the last two axes.  This file holds
//   fft_dct2d_kernel         the FUSED route (float; rows, cols in {32, 64}; all four kinds): whole images live in LDS, ONE HBM read and ONE
//                            HBM write of 4 R C bytes per image, on the persistent loop of the fused family exactly as fft_rfft2_kernel
//                            runs it (the hand-out of pf_handout.h, inactive slots; the launch is loop_launch with CONV_ONESHOT).
//   dct2d_transpose_kernel   the COMPOSED route's kernel around the two pffft[d]_hip_dct_transform_batch calls (dct2d_tu.hip): per image
//                            [rows][cols] -> [cols][rows] of REAL elements through padded 32 x 32 LDS tiles, 64-bit indices, edge tiles
//                            predicated.  The complex twin is fft2_transpose_kernel (fft_fft2.h), which keeps its code.
// The routes run different networks (one complex transform of C points for TWO real rows here, one real transform per row there): they
// agree at the accuracy bar, not bit for bit.
//
// The fused kernel is Makhoul's algorithm on both axes, two real lines riding one complex line (fft_rfft2.h).  H = C / 2, G = R / 2.
// T = R C / (2 PT) threads own one image (PT = 32 points per thread where a length is 32, else 16); a 256-thread workgroup holds 256 / T
// images ("slots").  The LDS image is R x C floats: R / 2 lines of C complex points, PITCH = 2 HP complex elements apart, ALSO read as R real
// rows of C floats (H complex points), HP complex elements apart (real row p starts at p HP).  p_N(i) = i / 2 (i even), N - 1 - (i - 1) / 2
// (i odd) is Makhoul's permutation.  Type II, per image:
//   load     R C / 4 chunks of 16 bytes (four reals of one row), chunk k = t + T i: linear across the lanes, unpredicated.  Element c of row r
//            goes to position p_C(c) of line r / 2, even rows to the real parts, odd rows to the imaginary parts (4-byte LDS writes).
//            Requested one group ahead.
//   row pass   R / 2 complex forward transforms of C points in place (fft2_axis of fft_fft2.h).
//   untangle and table, along the rows   with Z the transform of line l:  A[k] = (Z[k] + conj Z[C - k]) / 2 is the real transform of row
//            2 l, B[k] = (Z[k] - conj Z[C - k]) / (2 j) that of row 2 l + 1.  Every thread reads its PT / 2 pairs (Z[k], Z[C - k]), k < H, a
//            barrier, then z = dct_mul(A[k], t_k): Re z is output k, -Im z output C - k of row 2 l (k = 0: the two real ends, plain
//            products, outputs 0 and H), likewise B for row 2 l + 1, each written as a scalar into real row p_R(r) of the same image.
//            That is the row-axis permutation of the second pass, and the columns 2 q, 2 q + 1 are the real and imaginary parts of the
//            complex column q.  k = t mod H is the same for every pair of a thread: ONE table value in registers.
//   column pass   H complex columns of R points, HP apart.
//   untangle and table, along the columns   the same step with t_u of length R on the pairs (Z[u], Z[R - u]) of column q, u = t mod G:
//            outputs (u, 2 q), (u, 2 q + 1) are one complex write into real row u, natural order, and so are (R - u, 2 q), (R - u, 2 q + 1).
//   store    16-byte chunks of four reals, linear across the lanes; inactive slots skip it.
// Type III is the mirror, the rows index first: natural load; table product and packing Z[u] = Va[u] + j Vb[u], Z[R - u] = conj Va[u] +
// j conj Vb[u] of column q, in place (a thread reads and writes its own two positions); backward column pass; the same packing along the
// rows from real rows read at the positions the column pass left them, p_R undone (read, barrier, write); backward row pass; the store
// reads position p_C(c) of line r / 2 (64 columns: the four reals of a chunk in an order rotated by t).  The sine forms are the cosine
// forms with (-1)^(r + c) on the input (II) / output (III) and both indices reversed on the output (II) / input (III): signs and index
// maps of the load and the store, no table of their own.
// Both tables are the 1-D handles' device tables, read once before the loop.  IN PLACE (in == out) needs no extra care: an image is
// wholly in LDS (or in its threads' registers) before any of it is stored.
//
// The LDS image and its banks: HP and the slot stride IMG come from DCT2D_LAYOUT below, chosen by tools/dct2d_lds.py --search (the
// pitches it finds are those of fft_rfft2.h, whose two passes are the same accesses; the slot strides are its own) and verified by
// tools/dct2d_lds.py, which forms every LDS address of the kernel from this table and runs it through tools/lds_sim.py.  No access is
// worse than 2-way.
//
// Out of scope: lengths below 32, types I and IV, a different kind per axis, transforms along one axis only, strided images, a fused
// double kernel, fused lengths beyond 64.
#pragma once
#include "fft_dct.h"
#include "fft_fft2.h"
#include "pf_handout.h"

namespace pf {

// (rows, cols, HP, IMG) in complex elements: chosen by tools/dct2d_lds.py --search, verified by tools/dct2d_lds.py
template <int R, int C> struct Dct2dLayout;
#define DCT2D_LAYOUT(R_, C_, P_, I_) \
    template <> struct Dct2dLayout<R_, C_> { static constexpr int HP = P_, IMG = I_; };
DCT2D_LAYOUT(32, 32, 17, 560)
DCT2D_LAYOUT(32, 64, 35, 1120)
DCT2D_LAYOUT(64, 32, 19, 1216)
DCT2D_LAYOUT(64, 64, 33, 2112)
#undef DCT2D_LAYOUT

constexpr bool dct2d_fused_shape(int rows, int cols) { return (rows == 32 || rows == 64) && (cols == 32 || cols == 64); }

template <int R_, int C_>
struct Dct2dCfg {
    static constexpr int R = R_, C = C_, H = C / 2, G = R / 2;
    static_assert(dct2d_fused_shape(R, C), "rows, cols 32 / 64");
    static constexpr int PT = (R == 32 || C == 32) ? 32 : 16;   // points per thread
    static constexpr int T = R * C / 2 / PT;                    // threads per image
    static constexpr int WG = 256, SLOTS = WG / T;
    static constexpr int HP = Dct2dLayout<R, C>::HP, PITCH = 2 * HP, IMG = Dct2dLayout<R, C>::IMG;
    static constexpr int NI = R * C / 4 / T;                    // 16-byte chunks per thread
    static constexpr int NPAIR = G * H / T;                     // pairs of either untangling step per thread
    static constexpr size_t LDS_BYTES = (size_t)SLOTS * IMG * sizeof(cx<float>) + 16;   // + s_next[2]
    static_assert(T >= 16 && T <= WG && WG % T == 0, "whole slots");
    static_assert((R * C / 4) % T == 0 && (G * H) % T == 0, "whole chunks and pairs per thread");
    static_assert(T % H == 0 && T % G == 0, "one table value per thread and axis");
    static_assert(HP >= H && IMG >= R * HP, "the padded image holds every element");
};

// PF 1: the next group's chunks are requested before the second pass (they are live next to its points); PF 0: behind the store.
template <int R, int C, int KIND, int PF>
__global__ void __launch_bounds__(256)
fft_dct2d_kernel(const float* in, float* out, unsigned batch, const cx<float>* __restrict__ tabc, const cx<float>* __restrict__ tabr,
                 const cx<float>* __restrict__ tw64, unsigned* ctr) {
    typedef Dct2dCfg<R, C> Cf;
    typedef cx<float> CX;
    typedef vec4<float> chunk;
    constexpr bool III = dct_type3(KIND), SINE = dct_sine(KIND);
    constexpr int T = Cf::T, H = Cf::H, G = Cf::G, HP = Cf::HP, PITCH = Cf::PITCH, SLOTS = Cf::SLOTS, NPAIR = Cf::NPAIR, NI = Cf::NI;
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
    // t_k of the thread's own bins, either axis (they depend on the thread index only); bin 0 packs the two real ends
    const int kc = t % H, ur = t % G;
    const bool ec = kc == 0, er = ur == 0;
    const CX tc = ec ? mk<float>(tabc[0].x, tabc[H].x) : tabc[kc];
    const CX tr = er ? mk<float>(tabr[0].x, tabr[G].x) : tabr[ur];
    const int kc2 = ec ? H : C - kc, ur2 = er ? G : R - ur;   // the partner bin

    const bool dyn = ctr != nullptr;
    unsigned g = blockIdx.x;
    unsigned pend = blockIdx.x + gridDim.x;   // hand-out: pf_handout.h
    const size_t last = (size_t)batch - 1;
    chunk raw[NI];
    auto load = [&](size_t image) {
        const chunk* src = reinterpret_cast<const chunk*>(in + image * IMAGE);
#pragma unroll
        for (int i = 0; i < NI; ++i) raw[i] = __builtin_nontemporal_load(src + t + T * i);
    };
    {
        const size_t t0 = (size_t)g * SLOTS + slot;
        load(t0 < last ? t0 : last);
    }
    for (unsigned it = 0; (size_t)g * SLOTS < batch; ++it) {
        if (dyn && threadIdx.x == 0) pend = handout_grab(s_next, it, pend, ctr);
        const size_t tr_ = (size_t)g * SLOTS + slot;
        const bool active = tr_ < batch;  // inactive slots recompute the last image and never store
        const size_t dv = active ? tr_ : last;
        // ---- the image into LDS (free: the previous pass ended with a barrier behind its last read)
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int e = 4 * (t + T * i), r = e / C, c = e % C, h = c >> 1;   // c is a multiple of 4: h is even
            if constexpr (!III) {
                // (x0, x1, x2, x3) -> positions h, C - 1 - h, h + 1, C - 2 - h; the sine form negates where r + c is odd
                float* p = imgf + 2 * ((r >> 1) * PITCH) + (r & 1);
                const bool neg = SINE && (r & 1);
                p[2 * h] = neg ? -raw[i].x : raw[i].x;
                p[2 * (C - 1 - h)] = (SINE && !neg) ? -raw[i].y : raw[i].y;
                p[2 * (h + 1)] = neg ? -raw[i].z : raw[i].z;
                p[2 * (C - 2 - h)] = (SINE && !neg) ? -raw[i].w : raw[i].w;
            } else if constexpr (!SINE) {
                CX* p = img + r * HP + h;
                p[0] = mk<float>(raw[i].x, raw[i].y);
                p[1] = mk<float>(raw[i].z, raw[i].w);
            } else {   // both indices reversed
                CX* p = img + (R - 1 - r) * HP + (H - 1 - h);
                p[0] = mk<float>(raw[i].y, raw[i].x);
                p[-1] = mk<float>(raw[i].w, raw[i].z);
            }
        }
        __syncthreads();  // publishes s_next
        const unsigned gn = handout_next(dyn, s_next, it, g);
        const size_t tn = (size_t)gn * SLOTS + slot, nv = tn < last ? tn : last;
        if constexpr (!III) {
            // ---- rows: R / 2 lines of C points, 1 apart, PITCH from line to line
            fft2_axis<C, G, PITCH, 1, T, 0>(img, t, w);
            __syncthreads();
            // ---- untangle the two rows of every line, times t_k of length C, into real rows at their second-pass positions
            CX za[NPAIR], zb[NPAIR];
#pragma unroll
            for (int i = 0; i < NPAIR; ++i) {
                const CX* p = img + ((t + T * i) / H) * PITCH;
                za[i] = p[fft2_pos<C>(kc)];
                zb[i] = p[fft2_pos<C>(kc2)];
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < NPAIR; ++i) {
                const int l = (t + T * i) / H;
                const CX a = za[i], b = zb[i];
                CX A = mk<float>(0.5f * (a.x + b.x), 0.5f * (a.y - b.y)), B = mk<float>(0.5f * (a.y + b.y), 0.5f * (b.x - a.x));
                if (ec) { A = mk<float>(a.x, b.x); B = mk<float>(a.y, b.y); }   // the two real ends of either row
                const CX ya = dct_mul<false>(A, tc, ec), yb = dct_mul<false>(B, tc, ec);
                float* pa = imgf + 2 * (l * HP);              // real row p_R(2 l) = l
                float* pb = imgf + 2 * ((R - 1 - l) * HP);    // real row p_R(2 l + 1) = R - 1 - l
                pa[kc] = ya.x; pa[kc2] = ec ? ya.y : -ya.y;
                pb[kc] = yb.x; pb[kc2] = ec ? yb.y : -yb.y;
            }
            __syncthreads();
            if constexpr (PF) load(nv);
            // ---- columns: H complex columns of R points, HP apart, 1 from column to column
            fft2_axis<R, H, 1, HP, T, 0>(img, t, w);
            __syncthreads();
            // ---- untangle the two real columns of every complex column, times t_u of length R, into real rows in natural order
#pragma unroll
            for (int i = 0; i < NPAIR; ++i) {
                const CX* p = img + (t + T * i) / G;
                za[i] = p[fft2_pos<R>(ur) * HP];
                zb[i] = p[fft2_pos<R>(ur2) * HP];
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < NPAIR; ++i) {
                const int q = (t + T * i) / G;
                const CX a = za[i], b = zb[i];
                CX A = mk<float>(0.5f * (a.x + b.x), 0.5f * (a.y - b.y)), B = mk<float>(0.5f * (a.y + b.y), 0.5f * (b.x - a.x));
                if (er) { A = mk<float>(a.x, b.x); B = mk<float>(a.y, b.y); }
                const CX ya = dct_mul<false>(A, tr, er), yb = dct_mul<false>(B, tr, er);
                const float a2 = er ? ya.y : -ya.y, b2 = er ? yb.y : -yb.y;
                if constexpr (!SINE) {
                    img[ur * HP + q] = mk<float>(ya.x, yb.x);
                    img[ur2 * HP + q] = mk<float>(a2, b2);
                } else {   // output (R - 1 - u, C - 1 - v): the two columns of a pair change places
                    img[(R - 1 - ur) * HP + (H - 1 - q)] = mk<float>(yb.x, ya.x);
                    img[(R - 1 - ur2) * HP + (H - 1 - q)] = mk<float>(b2, a2);
                }
            }
            __syncthreads();
            // ---- store
            if (active) {
                chunk* dst = reinterpret_cast<chunk*>(out + dv * IMAGE);
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    const int e = 4 * (t + T * i);
                    const CX* p = img + (e / C) * HP + ((e % C) >> 1);
                    const CX a = p[0], b = p[1];
                    chunk o;
                    o.x = a.x; o.y = a.y; o.z = b.x; o.w = b.y;
                    __builtin_nontemporal_store(o, dst + t + T * i);
                }
            }
        } else {
            // ---- the columns' table product and packing Z = Va + j Vb, in place: a thread owns (u, q) and (R - u, q)
#pragma unroll
            for (int i = 0; i < NPAIR; ++i) {
                CX* p = img + (t + T * i) / G;
                const CX a = p[ur * HP], b = p[ur2 * HP];   // (X[u][2q], X[u][2q+1]), (X[R-u][2q], X[R-u][2q+1])
                const CX va = dct_mul<true>(mk<float>(a.x, er ? b.x : -b.x), tr, er), vb = dct_mul<true>(mk<float>(a.y, er ? b.y : -b.y), tr, er);
                p[ur * HP] = er ? mk<float>(va.x, vb.x) : mk<float>(va.x - vb.y, va.y + vb.x);
                p[ur2 * HP] = er ? mk<float>(va.y, vb.y) : mk<float>(va.x + vb.y, vb.x - va.y);
            }
            __syncthreads();
            // ---- columns: H complex columns of R points, backward
            fft2_axis<R, H, 1, HP, T, 1>(img, t, w);
            __syncthreads();
            // ---- the rows' table product and packing: real row r sits where the column pass left sample p_R(r)
            float xa[NPAIR], xa2[NPAIR], xb[NPAIR], xb2[NPAIR];
#pragma unroll
            for (int i = 0; i < NPAIR; ++i) {
                const int l = (t + T * i) / H;
                const float* pa = imgf + 2 * (fft2_pos<R>(l) * HP);
                const float* pb = imgf + 2 * (fft2_pos<R>(R - 1 - l) * HP);
                xa[i] = pa[kc]; xa2[i] = pa[kc2];
                xb[i] = pb[kc]; xb2[i] = pb[kc2];
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < NPAIR; ++i) {
                CX* p = img + ((t + T * i) / H) * PITCH;
                const CX va = dct_mul<true>(mk<float>(xa[i], ec ? xa2[i] : -xa2[i]), tc, ec);
                const CX vb = dct_mul<true>(mk<float>(xb[i], ec ? xb2[i] : -xb2[i]), tc, ec);
                p[kc] = ec ? mk<float>(va.x, vb.x) : mk<float>(va.x - vb.y, va.y + vb.x);
                p[kc2] = ec ? mk<float>(va.y, vb.y) : mk<float>(va.x + vb.y, vb.x - va.y);
            }
            __syncthreads();
            if constexpr (PF) load(nv);
            // ---- rows: R / 2 lines of C points, backward
            fft2_axis<C, G, PITCH, 1, T, 1>(img, t, w);
            __syncthreads();
            // ---- store: the real parts are row 2 l, the imaginary parts row 2 l + 1; sample c sits at position p_C(c)
            if (active) {
                chunk* dst = reinterpret_cast<chunk*>(out + dv * IMAGE);
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    const int e = 4 * (t + T * i), r = e / C, h = (e % C) >> 1;
                    const float* p = imgf + 2 * ((r >> 1) * PITCH) + (r & 1);
                    const bool neg = SINE && (r & 1);
                    // 64 columns: the four reals in an order rotated by t - the lanes whose digit-reversed positions fall on one bank take different ones
                    float x0 = 0.0f, x1 = 0.0f, x2 = 0.0f, x3 = 0.0f;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int jj = C == 64 ? (j + t) & 3 : j;
                        const int pos = jj == 0 ? h : jj == 1 ? C - 1 - h : jj == 2 ? h + 1 : C - 2 - h;
                        const float v = p[2 * fft2_pos<C>(pos)];
                        x0 = jj == 0 ? v : x0; x1 = jj == 1 ? v : x1; x2 = jj == 2 ? v : x2; x3 = jj == 3 ? v : x3;
                    }
                    chunk o;
                    o.x = neg ? -x0 : x0; o.y = (SINE && !neg) ? -x1 : x1; o.z = neg ? -x2 : x2; o.w = (SINE && !neg) ? -x3 : x3;
                    __builtin_nontemporal_store(o, dst + t + T * i);
                }
            }
        }
        __syncthreads();
        if constexpr (!PF) load(nv);
        g = gn;
    }
    if (dyn && threadIdx.x == 0) handout_rearm(ctr);
}

// ------------------------------------------------------------------------------------------------ composed route
// Per image [rows][cols] -> [cols][rows].  Tiles of 32 x 32 elements through a [32][33] LDS tile (the column read walks a pitch of 33
// elements: the 32 lanes of a row of the thread block fall on 32 different banks in float, on 32 different bank pairs in double),
// 256 threads as 32 x 8, tiles on a grid stride with 64-bit indices; lengths that are no multiple of 32 have predicated edge tiles.
// src != dst.
template <typename T>
__global__ void __launch_bounds__(256)
dct2d_transpose_kernel(const T* __restrict__ src, T* __restrict__ dst, size_t images, unsigned rows, unsigned cols) {
    __shared__ T tile[32][33];
    const unsigned tr = (rows + 31) / 32, tc = (cols + 31) / 32;
    const size_t per = (size_t)tr * tc, total = images * per, plane = (size_t)rows * cols;
    const unsigned x = threadIdx.x & 31, y = threadIdx.x >> 5;
    for (size_t id = blockIdx.x; id < total; id += gridDim.x) {
        const size_t im = id / per;
        const unsigned rem = (unsigned)(id - im * per), r0 = (rem / tc) * 32, c0 = (rem % tc) * 32;
        const T* a = src + im * plane;
        T* b = dst + im * plane;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned r = r0 + y + 8 * k, c = c0 + x;
            if (r < rows && c < cols) tile[y + 8 * k][x] = a[(size_t)r * cols + c];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned c = c0 + y + 8 * k, r = r0 + x;
            if (r < rows && c < cols) b[(size_t)c * rows + r] = tile[x][y + 8 * k];
        }
        __syncthreads();
    }
}

}  // namespace pf
