// Batched 2-D complex transforms (include/pffft_hip.h: pffft[d]_hip_fft2_*):  out[u][v] = s sum_r sum_c in[r][c] exp(-/+ 2 pi j (u r / rows +
// v c / cols)) of dense row-major images of rows x cols interleaved complex values, natural order in and out.  This file holds
//   fft_fft2_kernel      the FUSED route (float; rows, cols in {16, 32, 64}): whole images live in LDS, ONE HBM read and ONE HBM write per
//                        image, on the persistent loop of the fused family (the hand-out of pf_handout.h, inactive slots; the launch is
//                        loop_launch with CONV_ONESHOT).  All nine shapes loop: none runs in dispatch order only.
//   fft2_transpose_kernel  the COMPOSED route's kernel around two ordered transform_batch calls (fft2_tu.hip): per image
//                        [rows][cols] -> [cols][rows] through padded 32 x 32 LDS tiles, 64-bit indices, edge tiles predicated; the second
//                        launch carries the scaling.
// The routes run different butterfly networks (one in-register dft16 / dft32 per line or 8 x 8 with W_64 twiddles here, whatever
// transform_batch picks there): they agree at the accuracy bar, not bit for bit.
//
// The fused kernel.  T = rows cols / PT threads own one image (PT = 32 points per thread where a length is 32, else 16); a 256-thread
// workgroup holds 256 / T images ("slots").  Per image:
//   load     NCH = PT / 2 chunks of 16 bytes per thread, chunk k = t + T i of the image's dense run: linear across the lanes, unpredicated
//            (an inactive slot reads the batch's last image).  They are requested one group ahead, before the previous group's column pass,
//            and wait in registers.  A chunk holds two neighbours of one row: two 8-byte LDS writes.
//   row pass   every row through a length-`cols` transform IN PLACE in the LDS image; column pass: every column through a length-`rows`
//            one.  A line of 16 / 32 points is one thread's dftR in registers, natural order.  A line of 64 points takes two half passes of
//            radix 8 with a barrier between them: thread group j reads x[j + 8 q], transforms over q, multiplies by W_64^(j k1) (seven
//            values of the inner setup's table of length 64, held in registers across the loop: j depends on the thread only) and writes
//            position j + 8 k1; then group k1 reads positions 8 k1 ... 8 k1 + 7, transforms over j and writes X[k1 + 8 k2] to position
//            8 k1 + k2.  A 64-point axis therefore stays in base-8 digit-reversed positions; the other axis' pass does not care.
//   store    chunk k again: bin (u, v) and its neighbour are read from positions (p(u), p(v)), (p(u), p(v + 1)) - p undoes the digit
//            reversal - multiplied by s (one product per component; s = 1 changes no bit) and stored with one 16-byte access, linear
//            across the lanes; inactive slots skip it.
// IN PLACE (in == out) needs no extra care: an image is wholly in LDS (or in its threads' registers) before any of it is stored, and images
// do not overlap.  The one read that can see a stored result is an inactive slot's load of the last image, whose result is never stored.
//
// The LDS image and its banks.  Element (r, c) sits at complex index r PITCH + c of its slot, slots IMG elements apart (FFT2_LAYOUT
// below).  Nothing walks an axis at the natural pitch of cols 8 = 128 / 256 / 512 bytes: PITCH is cols + 1 (+ 3 or + 5 for three shapes), so
// that the lanes of a row pass - one row each, 32 consecutive rows per half wave - fall r PITCH mod 32 apart, on 32 different 8-byte bank
// pairs of the 64 banks a ds_read_b64 sees, and column passes have their lanes along c, consecutive elements at any pitch.  Where a half
// wave spans two slots (16 x 16) IMG = 16 mod 32 interleaves them.  Writes bank on (a / 4) mod 32 in groups of 16 lanes, so the same
// argument holds for 16 consecutive rows.  What is left is 2-way and is listed per shape and access by tools/fft2_lds.py, which forms the
// kernel's addresses from this table and runs them through tools/lds_sim.py: the writes of a 32 / 64-wide row's chunks (16 lanes, even
// elements of ONE row: two lanes per bank pair), the row passes of a thread group that spans 8 rows x 4 j (16 x 64, 32 x 64), and the
// digit-reversed reads of the store.  No access is worse than 2-way.
//
// Real input with half-spectrum columns is fft_rfft2.h (pffft[d]_hip_rfft2_*); forward x spectrum x backward in one kernel is fft_fft2c.h
// (pffft[d]_hip_fft2_convolve_batch).  Out of scope: strided or padded images, transforms along one axis only, a fused double
// kernel, fused shapes beyond 64 (128 x 128 = 128 KiB is one image per CU) and mixed-radix tiles, multi-device shards of one setup, 3-D.
#pragma once
#include "cxmath.h"
#include "pf_handout.h"

namespace pf {

// (rows, cols, PITCH, IMG) in complex elements: chosen by tools/fft2_lds.py --search, verified by tools/fft2_lds.py
template <int R, int C> struct Fft2Layout;
#define FFT2_LAYOUT(R_, C_, P_, I_) \
    template <> struct Fft2Layout<R_, C_> { static constexpr int PITCH = P_, IMG = I_; };
FFT2_LAYOUT(16, 16, 17, 272)
FFT2_LAYOUT(16, 32, 33, 528)
FFT2_LAYOUT(16, 64, 67, 1072)
FFT2_LAYOUT(32, 16, 17, 560)
FFT2_LAYOUT(32, 32, 33, 1056)
FFT2_LAYOUT(32, 64, 67, 2144)
FFT2_LAYOUT(64, 16, 17, 1088)
FFT2_LAYOUT(64, 32, 37, 2368)
FFT2_LAYOUT(64, 64, 65, 4160)
#undef FFT2_LAYOUT

constexpr bool fft2_fused_len(int n) { return n == 16 || n == 32 || n == 64; }

template <int R_, int C_>
struct Fft2Cfg {
    static constexpr int R = R_, C = C_;
    static_assert(fft2_fused_len(R) && fft2_fused_len(C), "lengths 16 / 32 / 64");
    static constexpr int PT = (R == 32 || C == 32) ? 32 : 16;   // points per thread
    static constexpr int T = R * C / PT;                        // threads per image
    static constexpr int WG = 256, SLOTS = WG / T, NCH = PT / 2;
    static constexpr int PITCH = Fft2Layout<R, C>::PITCH, IMG = Fft2Layout<R, C>::IMG;
    static constexpr size_t LDS_BYTES = (size_t)SLOTS * IMG * sizeof(cx<float>) + 16;   // + s_next[2]
    static_assert(T >= 16 && T <= WG && WG % T == 0, "whole slots");
    static_assert(PITCH >= C && IMG >= R * PITCH, "the padded image holds every element");
    static_assert(R % 16 == 0 && C % 2 == 0, "a 16-byte chunk holds two neighbours of one row");
};

// position of bin u of a line of L points in the LDS image
template <int L> __device__ __forceinline__ int fft2_pos(int u) { return L == 64 ? 8 * (u & 7) + (u >> 3) : u; }

// NL lines of L points through a transform in place: line l starts at img + l LS, its elements are ES apart.  w: W_64^(j k), k < 8, of
// the thread's j = t / (T / 8) (read for L = 64 only).
template <int L, int NL, int LS, int ES, int T, int DIR>
__device__ __forceinline__ void fft2_axis(cx<float>* img, int t, const cx<float> (&w)[8]) {
    if constexpr (L < 64) {
        static_assert(NL % T == 0, "whole lines per thread");
#pragma unroll
        for (int i = 0; i < NL / T; ++i) {
            cx<float>* p = img + (t + T * i) * LS;
            cx<float> a[L];
#pragma unroll
            for (int q = 0; q < L; ++q) a[q] = p[q * ES];
            dftR<L, DIR>(a);
#pragma unroll
            for (int q = 0; q < L; ++q) p[q * ES] = a[q];
        }
    } else {
        constexpr int G = T / 8;
        static_assert(T % 8 == 0 && NL % G == 0, "eight thread groups, whole lines per thread");
        const int j = t / G, l0 = t % G;
#pragma unroll
        for (int i = 0; i < NL / G; ++i) {
            cx<float>* p = img + (l0 + G * i) * LS + j * ES;
            cx<float> a[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) a[q] = p[8 * q * ES];
            dft8<DIR>(a);
#pragma unroll
            for (int k = 1; k < 8; ++k) a[k] = twmul<DIR>(a[k], w[k]);
#pragma unroll
            for (int k = 0; k < 8; ++k) p[8 * k * ES] = a[k];
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NL / G; ++i) {
            cx<float>* p = img + (l0 + G * i) * LS + 8 * j * ES;
            cx<float> a[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) a[q] = p[q * ES];
            dft8<DIR>(a);
#pragma unroll
            for (int q = 0; q < 8; ++q) p[q * ES] = a[q];
        }
    }
}

// PF 1: the next group's chunks are requested before the column pass (they are live next to its points); PF 0: behind the store.
template <int R, int C, int DIR, int PF>
__global__ void __launch_bounds__(256)
fft_fft2_kernel(const float* in, float* out, unsigned batch, float s, const cx<float>* __restrict__ tw64, unsigned* ctr) {
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
        // ---- rows: lines of C points, 1 apart, PITCH from line to line
        fft2_axis<C, R, PITCH, 1, T, DIR>(img, t, w);
        __syncthreads();
        if constexpr (PF) load(nv);
        // ---- columns: lines of R points, PITCH apart, 1 from line to line
        fft2_axis<R, C, 1, PITCH, T, DIR>(img, t, w);
        __syncthreads();
        // ---- store
        if (active) {
            chunk* dst = reinterpret_cast<chunk*>(out + dv * IMAGE);
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int e = 2 * (t + T * i);
                const CX* p = img + fft2_pos<R>(e / C) * PITCH;
                const CX a = p[fft2_pos<C>(e % C)], b = p[fft2_pos<C>(e % C + 1)];
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

// ------------------------------------------------------------------------------------------------ composed route
// Per image [rows][cols] -> [cols][rows], times s where SCALE (one product per stored component).  Tiles of 32 x 32 elements through a
// [32][33] LDS tile (the column read walks a pitch of 33 elements: no two lanes of a half wave on one bank pair), 256 threads as 32 x 8,
// tiles on a grid stride with 64-bit indices; lengths that are no multiple of 32 have predicated edge tiles.  src != dst.
template <typename T, int SCALE>
__global__ void __launch_bounds__(256)
fft2_transpose_kernel(const cx<T>* src, cx<T>* dst, size_t images, unsigned rows, unsigned cols, T s) {
    __shared__ cx<T> tile[32][33];
    const unsigned tr = (rows + 31) / 32, tc = (cols + 31) / 32;
    const size_t per = (size_t)tr * tc, total = images * per, plane = (size_t)rows * cols;
    const unsigned x = threadIdx.x & 31, y = threadIdx.x >> 5;
    for (size_t id = blockIdx.x; id < total; id += gridDim.x) {
        const size_t im = id / per;
        const unsigned rem = (unsigned)(id - im * per), r0 = (rem / tc) * 32, c0 = (rem % tc) * 32;
        const cx<T>* a = src + im * plane;
        cx<T>* b = dst + im * plane;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned r = r0 + y + 8 * k, c = c0 + x;
            if (r < rows && c < cols) tile[y + 8 * k][x] = a[(size_t)r * cols + c];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned c = c0 + y + 8 * k, r = r0 + x;
            if (r < rows && c < cols) {
                cx<T> v = tile[x][y + 8 * k];
                if constexpr (SCALE) v = mk<T>(s * v.x, s * v.y);
                b[(size_t)c * rows + r] = v;
            }
        }
        __syncthreads();
    }
}

}  // namespace pf
