// Polyphase filter bank (pffft_hip_pfb_transform_batch, pffft_hip_pfb_synthesis_batch): the kernels.
//
// ANALYSIS
//   u_f[j] = sum over p < taps, p ascending, of  h[p N + j] * x[f hop + p N + j]     (every product and every addition rounded once,
//                                                                                     the sum started from its first term)
//   out_f  = forward transform of u_f
//
//   fft_pfb_c1024_kernel   the FUSED route, complex float N = 1024: the persistent in-order loop of c1024_dyn_body (fft_c1024.h) with a
//                          folding loader.  Lane L's chunk j of tap p is the 16 bytes at frame + (p 512 + 64 j + L) chunks; its two
//                          prototype values are h[p N + 128 j + 2L + e].  The fold fills raw[8], then the SAME c1024_part_a /
//                          c1024_part_b as transform_batch run: the spectra equal transform_batch of the materialised folded frames
//                          bit for bit (tests/test_gpu_pfb.py).  It is a kernel of its own: fft_c1024.h keeps its text.
//                          PROTOTYPE: copied once per workgroup into an LDS table behind the exchange images (4 KiB per tap) and read
//                          with 8-byte accesses - consecutive lanes read consecutive 8 bytes, conflict-free -, so the vector-memory
//                          queue carries signal chunks only.
//                          LOADS IN FLIGHT: PFB_SLOTS taps (8 x 16 bytes per lane each) rotate through register slots: the slot a tap
//                          is folded from is at once refilled with tap p + PFB_SLOTS of the same frame, and after part A the slots take
//                          the first PFB_SLOTS taps of the NEXT frame, which are in flight while part B finishes this one.
//   pfb_fold_kernel        the streaming kernel of the COMPOSED route: folded frames -> dense rows of the frame matrix.  Rows are
//                          mapped to groups of threads of a workgroup (one division per row and thread, not per unit), units of U scalars.
//
// SYNTHESIS
//   signal[s] = scaling * ( sum over f ascending, 0 <= s - f hop < taps N, of  g[s - f hop] * y_f[(s - f hop) mod N] )
//                                                                                    (every product and every addition rounded once,
//                                                                                     the sum started from its first term; 0 where no
//                                                                                     frame covers s)
//   pfb_syn_kernel         the output-stationary gather behind the backward transforms: a thread owns units of U scalars of the output
//                          and loops over the covering frames.  WIDE form (U = 16 bytes) where every offset allows 16-byte accesses,
//                          SCALAR form (U = 1) for everything else; the arithmetic of a scalar is the same in both.  XCD = 1 maps every
//                          eighth of a sweep of the grid's tiles to one XCD (xcd_local of fft_fir.h); XCD = 0 is the plain grid stride.
#pragma once
#include "fft_c1024.h"
#include "fft_frames.h"
#include "fft_fir.h"
#include "pf_handout.h"

namespace pf {

constexpr int PFB_FUSED_MAX_TAPS = 16;          // = PFFFT_HIP_PFB_FUSED_MAX_TAPS (include/pffft_hip.h): 64 KiB of LDS table
constexpr int PFB_SLOTS = 2;                    // taps of one frame in flight per lane (32 VGPRs each)
constexpr size_t PFB_TABLE_OFFSET = (size_t)C1024_LDS_BYTES;   // the table starts behind the images and the counter slot (16-byte aligned)
constexpr size_t pfb_c1024_lds_bytes(size_t taps) { return PFB_TABLE_OFFSET + taps * 1024 * sizeof(float); }
static_assert(PFB_TABLE_OFFSET % 16 == 0, "table alignment");
static_assert(pfb_c1024_lds_bytes(PFB_FUSED_MAX_TAPS) <= 160 * 1024, "one workgroup per CU must fit with the largest table");

// the 8 chunks of tap p of the frame at `frame` (plain loads: a sample is read by taps N / hop frames, most of them of this workgroup)
__device__ __forceinline__ void pfb_load_tap(C1024V4 (&x)[8], const float* frame, unsigned p, int L) {
    const C1024V4* src = reinterpret_cast<const C1024V4*>(frame) + (size_t)p * 512 + L;
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = src[64 * j];
}

// raw = first ? x h : raw + x h, one rounding per product and per addition (the library is built with -ffp-contract=off)
__device__ __forceinline__ void pfb_fold_tap(C1024V4 (&raw)[8], const C1024V4 (&x)[8], const vec2<float>* htab, unsigned p, int L,
                                             bool first) {
    const vec2<float>* hp = htab + (size_t)p * 512 + L;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const vec2<float> h = hp[64 * j];
        C1024V4 t;
        t.x = x[j].x * h.x; t.y = x[j].y * h.x; t.z = x[j].z * h.y; t.w = x[j].w * h.y;
        if (first) raw[j] = t;
        else { raw[j].x = raw[j].x + t.x; raw[j].y = raw[j].y + t.y; raw[j].z = raw[j].z + t.z; raw[j].w = raw[j].w + t.w; }
    }
}

// ctr: the {next, done} pair of take_counters.  batch = nsignals nframes < 2^32; every offset is 64-bit.
template <int OUT_INTERNAL>
__global__ void __launch_bounds__(C1024_WAVES * 64, 1)
fft_pfb_c1024_kernel(const float* signal, size_t signal_stride, unsigned nframes, size_t hop2, const float* __restrict__ prototype,
                     unsigned taps, float* out, size_t out_stride, unsigned batch, const cx<float>* __restrict__ twg, unsigned* ctr) {
    typedef cx<float> C;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int wave = threadIdx.x >> 6, L = threadIdx.x & 63;
    char* wbase = smem_raw + wave * C1024_WAVE_BYTES;
    C* wl = reinterpret_cast<C*>(wbase);
    float* wf = reinterpret_cast<float*>(wbase);
    unsigned* s_next = reinterpret_cast<unsigned*>(smem_raw + C1024_WAVES * C1024_WAVE_BYTES);
    vec2<float>* htab = reinterpret_cast<vec2<float>*>(smem_raw + PFB_TABLE_OFFSET);

    C w1[7][2], w2[15];
    c1024_load_twiddles(twg, L, w1, w2);
    for (unsigned i = threadIdx.x; i < taps * 512u; i += C1024_WAVES * 64) htab[i] = reinterpret_cast<const vec2<float>*>(prototype)[i];
    unsigned pend = blockIdx.x + gridDim.x;   // hand-out: pf_handout.h
    __syncthreads();
    unsigned g = blockIdx.x;
    const size_t last = (size_t)batch - 1;
    // frame v = i nframes + f starts at signal + i signal_stride + f hop2 floats (hop2 = 2 hop); clamped: always a valid address
    auto frame_of = [&](size_t t) -> const float* {
        const unsigned v = (unsigned)(t < last ? t : last);
        const unsigned i = v / nframes, f = v - i * nframes;
        return signal + (size_t)i * signal_stride + (size_t)f * hop2;
    };
    C1024V4 slot[PFB_SLOTS][8];
    const float* cur = frame_of((size_t)g * C1024_WAVES + wave);
#pragma unroll
    for (int q = 0; q < PFB_SLOTS; ++q)
        if ((unsigned)q < taps) pfb_load_tap(slot[q], cur, q, L);
    for (unsigned it = 0; (size_t)g * C1024_WAVES < batch; ++it) {
        if (threadIdx.x == 0) pend = handout_grab(s_next, it, pend, ctr);
        const size_t t = (size_t)g * C1024_WAVES + wave;
        const bool active = t < batch;  // wave-uniform
        // ---- the fold: slot q holds tap p0 + q; a consumed slot is refilled with tap p + PFB_SLOTS of the same frame
        C1024V4 raw[8];
        for (unsigned p0 = 0; p0 < taps; p0 += PFB_SLOTS) {
#pragma unroll
            for (int q = 0; q < PFB_SLOTS; ++q) {
                const unsigned p = p0 + q;
                if (p < taps) {
                    pfb_fold_tap(raw, slot[q], htab, p, L, q == 0 && p0 == 0);
                    if (p + PFB_SLOTS < taps) pfb_load_tap(slot[q], cur, p + PFB_SLOTS, L);
                }
            }
        }
        c1024_part_a<FWD, 0>(raw, wl, wf, w1, L);
        __syncthreads();
        const unsigned gn = s_next[(it + 1) & 1];   // hand-out: pf_handout.h, kept inline: handout_next(true, ..) changes this kernel
        cur = frame_of((size_t)gn * C1024_WAVES + wave);
#pragma unroll
        for (int q = 0; q < PFB_SLOTS; ++q)
            if ((unsigned)q < taps) pfb_load_tap(slot[q], cur, q, L);   // in flight while this transform finishes
        if (active) c1024_part_b<FWD, OUT_INTERNAL>(out + t * out_stride, 0, wl, wf, w2, L);
        g = gn;
    }
    if (threadIdx.x == 0) handout_rearm(ctr);
}

// ------------------------------------------------------------------------------------------------ composed route
// folded frames v0 ... v0 + count - 1 (v = i nframes + f) -> dense rows of `row` = N spp scalars.  A workgroup of 256 threads works on
// 256 / lpr rows at a time, lpr (a power of two <= 256) threads per row, each on units of U scalars (U = 4 / 2 where the offsets allow
// 16-byte accesses, else 1): the frame's source is computed once per row and thread.  spp scalars per sample share one prototype value.
template <typename T, int U>
__global__ void __launch_bounds__(256)
pfb_fold_kernel(const T* __restrict__ signal, size_t signal_stride, size_t nframes, size_t hop, int spp, const T* __restrict__ prototype,
                unsigned taps, T* __restrict__ dst, size_t v0, size_t count, unsigned row, unsigned lpr) {
    const unsigned upr = row / U, rpb = 256 / lpr;
    const unsigned lr = threadIdx.x / lpr, u0 = threadIdx.x - lr * lpr;
    const unsigned N = row / (unsigned)spp;
    for (size_t r = (size_t)blockIdx.x * rpb + lr; r < count; r += (size_t)gridDim.x * rpb) {
        const size_t v = v0 + r, i = v / nframes, f = v - i * nframes;
        const T* src = signal + i * signal_stride + f * hop;
        T* d = dst + r * row;
        for (unsigned u = u0; u < upr; u += lpr) {
            const unsigned j = u * U;
            T acc[U];
            for (unsigned p = 0; p < taps; ++p) {
                const T* sp = src + (size_t)p * row + j;
                const T* hp = prototype + (size_t)p * N;
                T a[U];
                if constexpr (U == 1) a[0] = sp[0];
                else {
                    const vec4<float> c = *reinterpret_cast<const vec4<float>*>(sp);
                    __builtin_memcpy(a, &c, 16);
                }
#pragma unroll
                for (int k = 0; k < U; ++k) {
                    const T t = a[k] * hp[(j + k) / (unsigned)spp];
                    acc[k] = p == 0 ? t : acc[k] + t;
                }
            }
            if constexpr (U == 1) d[j] = acc[0];
            else {
                vec4<float> c;
                __builtin_memcpy(&c, acc, 16);
                *reinterpret_cast<vec4<float>*>(d + j) = c;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ synthesis
// a / b and the remainder: 32-bit division wherever both fit (the common case), 64-bit otherwise
__device__ __forceinline__ size_t pfb_udiv(size_t a, size_t b, size_t& rem) {
    if (((a | b) >> 32) == 0) {
        const unsigned q = (unsigned)a / (unsigned)b;
        rem = (unsigned)a - q * (unsigned)b;
        return q;
    }
    const size_t q = a / b;
    rem = a - q * b;
    return q;
}

// U consecutive scalars as ONE access (16 bytes: U = 4 floats / 2 doubles; 8 bytes: 2 floats), or one scalar
template <typename T, int U>
__device__ __forceinline__ void pfb_load(T (&a)[U], const T* p) {
    if constexpr (U == 1) a[0] = p[0];
    else if constexpr (sizeof(T) * U == 16) {
        const vec4<float> c = *reinterpret_cast<const vec4<float>*>(p);
        __builtin_memcpy(a, &c, 16);
    } else {
        static_assert(sizeof(T) * U == 8, "8- and 16-byte units only");
        const vec2<float> c = *reinterpret_cast<const vec2<float>*>(p);
        __builtin_memcpy(a, &c, 8);
    }
}

// Scalars s0 spp ... s1 spp - 1 of every signal, as units of U scalars (the wide form's conditions are the host's: hop spp, signal_stride
// and row are multiples of U and every pointer is aligned, so that the scalars of a unit share their frames and neither a frame's edge nor
// the wrap at N falls inside a unit).  `y` holds the backward-transformed frames fbase ... of every signal as dense rows (`fpitch` rows per
// signal); frames f < nframes exist.  span = taps N samples, hop_mod = (hop spp) mod (N spp).  Per unit: the divisions that split the unit
// index and find the first and the last covering frame; inside the f loop the position in the prototype falls by hop and the position in
// the row is carried modulo N with one compare - no division.
template <typename T, int U, int SPP, int XCD>
__global__ void __launch_bounds__(256)
pfb_syn_kernel(const T* __restrict__ y, size_t fbase, size_t fpitch, size_t nframes, size_t hop, unsigned N, size_t span, unsigned hop_mod,
               const T* __restrict__ g, T scaling, T* __restrict__ signal, size_t signal_stride, size_t nsignals, size_t s0, size_t s1) {
    constexpr int GU = U >= SPP ? U / SPP : 1;    // prototype values per unit
    const unsigned row = N * SPP;
    const size_t hop_s = hop * SPP;
    const size_t ups = (s1 - s0) * SPP / U, units = nsignals * ups;
    const size_t tiles = (units + 255) / 256;
    const unsigned pos = XCD ? xcd_local(blockIdx.x, gridDim.x) : blockIdx.x;
    for (size_t t0 = 0; t0 < tiles; t0 += gridDim.x) {
        const size_t x = (t0 + pos) * 256 + threadIdx.x;
        if (x >= units) continue;
        size_t u;
        const size_t i = pfb_udiv(x, ups, u);
        const size_t e = s0 * SPP + u * U, s = e / SPP;
        size_t r;
        size_t fhi = pfb_udiv(s, hop, r);
        if (fhi > nframes - 1) fhi = nframes - 1;
        const size_t flo = s < span ? 0 : pfb_udiv(s - span, hop, r) + 1;
        T acc[U];
#pragma unroll
        for (int k = 0; k < U; ++k) acc[k] = (T)0;
        bool first = true;
        if (flo <= fhi) {
            size_t m = e - flo * hop_s;     // scalars from the start of frame flo: < span SPP
            size_t jr;
            pfb_udiv(m, row, jr);
            unsigned j = (unsigned)jr;      // ... modulo the row
            const T* yp = y + (i * fpitch + (flo - fbase)) * row;
            for (size_t f = flo; f <= fhi; ++f) {
                T yv[U], gv[GU];
                pfb_load<T, U>(yv, yp + j);
                pfb_load<T, GU>(gv, g + m / SPP);
#pragma unroll
                for (int k = 0; k < U; ++k) {
                    const T term = gv[U >= SPP ? k / SPP : 0] * yv[k];
                    acc[k] = first ? term : acc[k] + term;
                }
                first = false;
                m -= hop_s;
                j = j >= hop_mod ? j - hop_mod : j + (row - hop_mod);
                yp += row;
            }
        }
        T o[U];
#pragma unroll
        for (int k = 0; k < U; ++k) o[k] = first ? (T)0 : scaling * acc[k];
        T* dst = signal + i * signal_stride + e;
        if constexpr (U == 1) __builtin_nontemporal_store(o[0], dst);
        else {
            vec4<float> c;
            __builtin_memcpy(&c, o, 16);
            __builtin_nontemporal_store(c, reinterpret_cast<vec4<float>*>(dst));
        }
    }
}

}  // namespace pf
