// Batched 2-D real transforms (include/pffft_hip.h: pffft[d]_hip_rfft2_*): forward rows x cols reals -> rows x bins interleaved complex
// values, bins = cols / 2 + 1 (numpy.fft.rfft2 times s); backward the half-spectrum -> rows x cols reals (numpy.fft.irfft2 times
// rows cols s, with numpy's rule for a half-spectrum that is not Hermitian: only the Hermitian part (X[u] + conj X[rows - u]) / 2 of the
// columns 0 and cols / 2 counts).  Dense row-major images, natural order in and out.  This file holds
//   fft_rfft2_kernel     the FUSED route (float; rows in {16, 32, 64}, cols in {32, 64}): whole images live in LDS, ONE HBM read and ONE
//                        HBM write per image (4 R C bytes on the real side, 8 R bins on the spectrum side), on the persistent loop of the
//                        fused family exactly as fft_fft2_kernel runs it (the hand-out of pf_handout.h, inactive slots; the launch is
//                        loop_launch with CONV_ONESHOT).
//   rfft2_unpack_kernel, rfft2_pack_kernel   the COMPOSED route's kernels between the real transform_batch over the rows and the complex
//                        one over the columns (rfft2_tu.hip): canonical packed real spectra [rows][cols] (element 0 DC, element 1 Nyquist,
//                        then re / im pairs) <-> [bins][rows] complex, through padded 32 x 32 LDS tiles like fft2_transpose_kernel.
// The routes run different butterfly networks: they agree at the accuracy bar, not bit for bit.
//
// The fused kernel does half the work of the complex one and needs no twiddles beyond W_64.  H = cols / 2.  T = rows cols / (2 PT) threads
// own one image (PT = 32 points per thread where a length is 32, else 16); a 256-thread workgroup holds 256 / T images ("slots").
// The LDS image is rows / 2 lines of cols complex points, PITCH = 2 HP elements apart; it is ALSO read as rows half lines of H points,
// HP apart (half line r starts at r HP: line l holds the half lines 2 l and 2 l + 1).  Forward, per image:
//   load     rows cols / 4 chunks of 16 bytes (four reals of one row), chunk k = t + T i: linear across the lanes, unpredicated.  Real row
//            2 l goes to the real parts of line l, row 2 l + 1 to its imaginary parts (4-byte LDS writes).  Requested one group ahead.
//   row pass   rows / 2 complex transforms of cols points in place (fft2_axis of fft_fft2.h: dft16 / dft32 per line, or 8 x 8 with W_64).
//   untangle   with Z the transform of line l:  A[v] = (Z[v] + conj Z[cols - v]) / 2 is the spectrum of row 2 l, B[v] = (Z[v] - conj Z[cols -
//            v]) / (2 j) that of row 2 l + 1.  Every thread reads its PT / 2 pairs (Z[v], Z[cols - v]), v < H, a barrier, then it writes
//            A[v] to half line 2 l and B[v] to half line 2 l + 1, position v - natural order, which undoes the digit reversal of a 64-point
//            row.  A[0], A[H], B[0], B[H] are real: column 0 and column H of a row travel as ONE complex column A[0] + j A[H] at v = 0.
//   column pass   H complex columns of rows points, HP apart: a power of two, no ragged thread mapping.
//   store    chunk k of the rows x bins half-spectrum (two complex bins, 16 bytes, linear across the lanes; bins is odd, so chunks straddle
//            row ends and the last iteration is predicated): bin (u, v), 0 < v < H, is read from (p(u), v); with Q the packed column,
//            bin (u, 0) = (Q[u] + conj Q[rows - u]) / 2 and bin (u, H) = (Q[u] - conj Q[rows - u]) / (2 j).  Times s, one product per
//            component (s = 1 changes no bit).
// Backward is the mirror: the chunks of the half-spectrum go to half line u, position v (bin H to the spare position H: HP > H); the
// Hermitian parts of the columns 0 and H along u are formed and packed into position 0 (without this step a non-Hermitian column leaks
// into the result; one thread owns u and rows - u); backward column pass; Z[v] = A[v] + j B[v], Z[cols - v] = conj A[v] + j conj B[v] are
// rebuilt (read, barrier, write) with A[0] = Re Q, A[H] = Im Q of the packed column; backward row pass of rows / 2 lines; the real parts
// are row 2 l, the imaginary parts row 2 l + 1, stored times s as 16-byte chunks of four reals.
//
// The LDS image and its banks: HP, the slot stride IMG and the order of a half-spectrum chunk's two bins come from RFFT2_LAYOUT below, chosen by tools/rfft2_lds.py --search and verified
// by tools/rfft2_lds.py, which forms every LDS address of the kernel from this table and runs it through tools/lds_sim.py.  No access is
// worse than 2-way.
//
// Out of scope: padded or strided rows (and therefore in place), cols = 16, a fused double kernel, fused lengths beyond 64 and mixed-radix
// tiles, transforms along one axis only, multi-device shards of one setup, 3-D.
#pragma once
#include "fft_fft2.h"
#include "pf_handout.h"

namespace pf {

// (rows, cols, HP, IMG, LSW, SSW): HP and IMG in complex elements; LSW / SSW 1: odd threads take the two bins of a half-spectrum chunk in
// the other order when the backward kernel writes them to LDS (LSW) / when the forward kernel reads them for the store (SSW).  The rows
// of a half-spectrum have an odd length, so a chunk's bins walk across row ends; where the radix-8 half passes ask for a pitch at which
// that walk is 3-way, the alternating order brings it to 2-way.  Chosen by tools/rfft2_lds.py --search, verified by tools/rfft2_lds.py.
template <int R, int C> struct Rfft2Layout;
#define RFFT2_LAYOUT(R_, C_, P_, I_, L_, S_) \
    template <> struct Rfft2Layout<R_, C_> { static constexpr int HP = P_, IMG = I_, LSW = L_, SSW = S_; };
RFFT2_LAYOUT(16, 32, 26, 423, 0, 0)
RFFT2_LAYOUT(16, 64, 35, 560, 1, 1)
RFFT2_LAYOUT(32, 32, 17, 547, 0, 0)
RFFT2_LAYOUT(32, 64, 35, 1121, 1, 1)
RFFT2_LAYOUT(64, 32, 19, 1217, 1, 0)
RFFT2_LAYOUT(64, 64, 33, 2112, 0, 0)
#undef RFFT2_LAYOUT

constexpr bool rfft2_fused_shape(int rows, int cols) { return fft2_fused_len(rows) && (cols == 32 || cols == 64); }

template <int R_, int C_>
struct Rfft2Cfg {
    static constexpr int R = R_, C = C_, H = C / 2, BINS = H + 1;
    static_assert(rfft2_fused_shape(R, C), "rows 16 / 32 / 64, cols 32 / 64");
    static constexpr int PT = (R == 32 || C == 32) ? 32 : 16;   // points per thread
    static constexpr int T = R * C / 2 / PT;                    // threads per image
    static constexpr int WG = 256, SLOTS = WG / T;
    static constexpr int HP = Rfft2Layout<R, C>::HP, PITCH = 2 * HP, IMG = Rfft2Layout<R, C>::IMG;
    static constexpr int CH_REAL = R * C / 4, CH_SPEC = R * BINS / 2;               // 16-byte chunks of an image, either side
    static constexpr int NI_REAL = CH_REAL / T, NI_SPEC = (CH_SPEC + T - 1) / T;    // ... per thread (the last of NI_SPEC predicated)
    static constexpr int NPAIR = R * H / 2 / T;                                     // (Z[v], Z[cols - v]) pairs per thread
    static constexpr size_t LDS_BYTES = (size_t)SLOTS * IMG * sizeof(cx<float>) + 16;   // + s_next[2]
    static_assert(T >= 8 && T <= WG && WG % T == 0, "whole slots");
    static_assert(CH_REAL % T == 0 && (R * H / 2) % T == 0, "whole chunks and pairs per thread");
    static_assert(HP >= H + 1 && IMG >= R * HP, "the padded image holds every element, and bin H next to its half line");
};

template <int R, int C, int DIR, int PF>
__global__ void __launch_bounds__(256)
fft_rfft2_kernel(const float* in, float* out, unsigned batch, float s, const cx<float>* __restrict__ tw64, unsigned* ctr) {
    typedef Rfft2Cfg<R, C> Cf;
    typedef cx<float> CX;
    typedef vec4<float> chunk;
    constexpr int T = Cf::T, H = Cf::H, BINS = Cf::BINS, HP = Cf::HP, PITCH = Cf::PITCH, SLOTS = Cf::SLOTS, NPAIR = Cf::NPAIR;
    constexpr size_t REAL_IMAGE = (size_t)R * C, SPEC_IMAGE = (size_t)R * BINS * 2;   // scalars of one image, either side
    constexpr size_t IN_IMAGE = DIR ? SPEC_IMAGE : REAL_IMAGE, OUT_IMAGE = DIR ? REAL_IMAGE : SPEC_IMAGE;
    constexpr int NI_IN = DIR ? Cf::NI_SPEC : Cf::NI_REAL, CH_IN = DIR ? Cf::CH_SPEC : Cf::CH_REAL;
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

    const bool dyn = ctr != nullptr;
    unsigned g = blockIdx.x;
    unsigned pend = blockIdx.x + gridDim.x;   // hand-out: pf_handout.h
    const size_t last = (size_t)batch - 1;
    chunk raw[NI_IN];
#pragma unroll
    for (int i = 0; i < NI_IN; ++i) raw[i].x = raw[i].y = raw[i].z = raw[i].w = 0.0f;
    // chunk t + T i of an image exists: always, but in the last iteration of a count that is no multiple of T
    auto has = [&](int i, int chunks) { return chunks % T == 0 || i < (chunks + T - 1) / T - 1 || t + T * i < chunks; };
    auto load = [&](size_t image) {
        const chunk* src = reinterpret_cast<const chunk*>(in + image * IN_IMAGE);
#pragma unroll
        for (int i = 0; i < NI_IN; ++i)
            if (has(i, CH_IN)) raw[i] = __builtin_nontemporal_load(src + t + T * i);
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
        for (int i = 0; i < NI_IN; ++i) {
            if (!has(i, CH_IN)) continue;
            if constexpr (!DIR) {
                const int e = 4 * (t + T * i), r = e / C, c = e % C;
                float* p = imgf + 2 * ((r >> 1) * PITCH + c) + (r & 1);
                // the four reals in an order rotated by t / 4: lanes 4 apart, whose chunks start 32 dwords apart, take different banks
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int jj = (j + (t >> 2)) & 3;
                    p[2 * jj] = jj == 0 ? raw[i].x : jj == 1 ? raw[i].y : jj == 2 ? raw[i].z : raw[i].w;
                }
            } else {
                const int odd = Rfft2Layout<R, C>::LSW ? (t & 1) : 0;
                const int e0 = 2 * (t + T * i) + odd, e1 = 2 * (t + T * i) + 1 - odd;
                const CX lo = mk<float>(raw[i].x, raw[i].y), hi = mk<float>(raw[i].z, raw[i].w);
                img[(e0 / BINS) * HP + e0 % BINS] = odd ? hi : lo;
                img[(e1 / BINS) * HP + e1 % BINS] = odd ? lo : hi;
            }
        }
        __syncthreads();  // publishes s_next
        const unsigned gn = handout_next(dyn, s_next, it, g);
        const size_t tn = (size_t)gn * SLOTS + slot, nv = tn < last ? tn : last;
        if constexpr (!DIR) {
            // ---- rows: R / 2 lines of C points, 1 apart, PITCH from line to line
            fft2_axis<C, R / 2, PITCH, 1, T, 0>(img, t, w);
            __syncthreads();
            // ---- untangle the two rows of every line, into half lines in natural order
            CX za[NPAIR], zb[NPAIR];
#pragma unroll
            for (int i = 0; i < NPAIR; ++i) {
                const int k = t + T * i, l = k / H, v = k % H;
                const CX* p = img + l * PITCH;
                za[i] = p[fft2_pos<C>(v)];
                zb[i] = p[fft2_pos<C>(v == 0 ? H : C - v)];
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < NPAIR; ++i) {
                const int k = t + T * i, l = k / H, v = k % H;
                const CX a = za[i], b = zb[i];
                CX A = mk<float>(0.5f * (a.x + b.x), 0.5f * (a.y - b.y)), B = mk<float>(0.5f * (a.y + b.y), 0.5f * (b.x - a.x));
                if (v == 0) { A = mk<float>(a.x, b.x); B = mk<float>(a.y, b.y); }   // the packed column: A[0] + j A[H], B[0] + j B[H]
                img[(2 * l) * HP + v] = A;
                img[(2 * l + 1) * HP + v] = B;
            }
            __syncthreads();
            if constexpr (PF) load(nv);
            // ---- columns: H lines of R points, HP apart, 1 from line to line
            fft2_axis<R, H, 1, HP, T, 0>(img, t, w);
            __syncthreads();
            // ---- store
            if (active) {
                auto bin = [&](int e) {
                    const int u = e / BINS, v = e % BINS;
                    const CX* p = img + fft2_pos<R>(u) * HP;
                    if (v != 0 && v != H) return p[v];
                    const CX a = p[0], b = img[fft2_pos<R>((R - u) & (R - 1)) * HP];
                    return v == 0 ? mk<float>(0.5f * (a.x + b.x), 0.5f * (a.y - b.y)) : mk<float>(0.5f * (a.y + b.y), 0.5f * (b.x - a.x));
                };
                chunk* dst = reinterpret_cast<chunk*>(out + dv * OUT_IMAGE);
#pragma unroll
                for (int i = 0; i < Cf::NI_SPEC; ++i) {
                    if (!has(i, Cf::CH_SPEC)) continue;
                    const int e = 2 * (t + T * i), odd = Rfft2Layout<R, C>::SSW ? (t & 1) : 0;
                    const CX p = bin(e + odd), q = bin(e + 1 - odd);
                    const CX a = odd ? q : p, b = odd ? p : q;
                    chunk o;
                    o.x = s * a.x; o.y = s * a.y; o.z = s * b.x; o.w = s * b.y;
                    __builtin_nontemporal_store(o, dst + t + T * i);
                }
            }
        } else {
            // ---- the Hermitian parts of the columns 0 and H along u, packed into position 0: one thread owns u and R - u
            for (int u = t; u <= R / 2; u += T) {
                const int ur = (R - u) & (R - 1);
                const CX a = img[u * HP], a2 = img[ur * HP], b = img[u * HP + H], b2 = img[ur * HP + H];
                const CX h0 = mk<float>(0.5f * (a.x + a2.x), 0.5f * (a.y - a2.y)), hh = mk<float>(0.5f * (b.x + b2.x), 0.5f * (b.y - b2.y));
                img[u * HP] = mk<float>(h0.x - hh.y, h0.y + hh.x);
                img[ur * HP] = mk<float>(h0.x + hh.y, hh.x - h0.y);
            }
            __syncthreads();
            // ---- columns: H lines of R points, HP apart
            fft2_axis<R, H, 1, HP, T, 1>(img, t, w);
            __syncthreads();
            // ---- rebuild the lines Z = A + j B of two rows each, natural order
            CX qa[NPAIR], qb[NPAIR];
#pragma unroll
            for (int i = 0; i < NPAIR; ++i) {
                const int k = t + T * i, l = k / H, v = k % H;
                qa[i] = img[fft2_pos<R>(2 * l) * HP + v];
                qb[i] = img[fft2_pos<R>(2 * l + 1) * HP + v];
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < NPAIR; ++i) {
                const int k = t + T * i, l = k / H, v = k % H;
                const CX A = qa[i], B = qb[i];
                CX* p = img + l * PITCH;
                if (v == 0) {   // the packed column: A[0] = Re, A[H] = Im
                    p[0] = mk<float>(A.x, B.x);
                    p[H] = mk<float>(A.y, B.y);
                } else {
                    p[v] = mk<float>(A.x - B.y, A.y + B.x);
                    p[C - v] = mk<float>(A.x + B.y, B.x - A.y);
                }
            }
            __syncthreads();
            if constexpr (PF) load(nv);
            // ---- rows: R / 2 lines of C points
            fft2_axis<C, R / 2, PITCH, 1, T, 1>(img, t, w);
            __syncthreads();
            // ---- store: the real parts are row 2 l, the imaginary parts row 2 l + 1
            if (active) {
                chunk* dst = reinterpret_cast<chunk*>(out + dv * OUT_IMAGE);
#pragma unroll
                for (int i = 0; i < Cf::NI_REAL; ++i) {
                    const int e = 4 * (t + T * i), r = e / C, c = e % C;
                    const float* p = imgf + 2 * ((r >> 1) * PITCH) + (r & 1);
                    chunk o;
                    o.x = s * p[2 * fft2_pos<C>(c)]; o.y = s * p[2 * fft2_pos<C>(c + 1)];
                    o.z = s * p[2 * fft2_pos<C>(c + 2)]; o.w = s * p[2 * fft2_pos<C>(c + 3)];
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
// Per image: canonical packed real spectra [rows][2 half scalars] (element 0 of a row is (DC, Nyquist), element v the bin v) ->
// [half + 1][rows] complex, the imaginary parts of the bins 0 and half a +0.  Tiles of 32 x 32 elements through a [32][33] LDS tile,
// 256 threads as 32 x 8, tiles on a grid stride with 64-bit indices, edge tiles predicated (the bin count is odd).  src != dst.
template <typename T>
__global__ void __launch_bounds__(256)
rfft2_unpack_kernel(const cx<T>* src, cx<T>* dst, size_t images, unsigned rows, unsigned half) {
    __shared__ cx<T> tile[32][33];
    const unsigned bins = half + 1, tr = (rows + 31) / 32, tc = (bins + 31) / 32;
    const size_t per = (size_t)tr * tc, total = images * per;
    const unsigned x = threadIdx.x & 31, y = threadIdx.x >> 5;
    for (size_t id = blockIdx.x; id < total; id += gridDim.x) {
        const size_t im = id / per;
        const unsigned rem = (unsigned)(id - im * per), r0 = (rem / tc) * 32, c0 = (rem % tc) * 32;
        const cx<T>* a = src + im * ((size_t)rows * half);
        cx<T>* b = dst + im * ((size_t)bins * rows);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned r = r0 + y + 8 * k, c = c0 + x;
            if (r < rows && c < bins) {
                cx<T> v = a[(size_t)r * half + (c < half ? c : 0)];
                if (c == 0) v = mk<T>(v.x, (T)0);
                else if (c == half) v = mk<T>(v.y, (T)0);
                tile[y + 8 * k][x] = v;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned c = c0 + y + 8 * k, r = r0 + x;
            if (r < rows && c < bins) b[(size_t)c * rows + r] = tile[x][y + 8 * k];
        }
        __syncthreads();
    }
}

// The way back: [half + 1][rows] complex -> canonical packed real spectra [rows][2 half scalars], times s (one product per stored
// component).  Element 0 of a row takes the REAL parts of the bins 0 and half; their imaginary parts are dropped, which is numpy's rule for
// a half-spectrum that is not Hermitian.  src != dst.
template <typename T>
__global__ void __launch_bounds__(256)
rfft2_pack_kernel(const cx<T>* src, cx<T>* dst, size_t images, unsigned rows, unsigned half, T s) {
    __shared__ cx<T> tile[32][33];
    const unsigned bins = half + 1, tv = (half + 31) / 32, tc = (rows + 31) / 32;
    const size_t per = (size_t)tv * tc, total = images * per;
    const unsigned x = threadIdx.x & 31, y = threadIdx.x >> 5;
    for (size_t id = blockIdx.x; id < total; id += gridDim.x) {
        const size_t im = id / per;
        const unsigned rem = (unsigned)(id - im * per), v0 = (rem / tc) * 32, r0 = (rem % tc) * 32;
        const cx<T>* a = src + im * ((size_t)bins * rows);
        cx<T>* b = dst + im * ((size_t)rows * half);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned v = v0 + y + 8 * k, r = r0 + x;
            if (v < half && r < rows) {
                cx<T> e = a[(size_t)v * rows + r];
                if (v == 0) e = mk<T>(e.x, a[(size_t)half * rows + r].x);
                tile[y + 8 * k][x] = e;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned r = r0 + y + 8 * k, v = v0 + x;
            if (v < half && r < rows) {
                const cx<T> e = tile[x][y + 8 * k];
                b[(size_t)r * half + v] = mk<T>(s * e.x, s * e.y);
            }
        }
        __syncthreads();
    }
}

}  // namespace pf
