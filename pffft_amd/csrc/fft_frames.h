// Windowed overlapping-frame transforms (pffft_hip_frames_transform_batch / pffft_hip_frames_overlap_add_batch): the kernels.
//
//   fft_frames_kernel   the FUSED analysis route - the register-tiled real forward transform of fft_tiled.h with a framed loader: the
//                       source of transform v = i nframes + f is  signal + i signal_stride + f hop  instead of  in + v N, the raw
//                       16-byte chunks are multiplied by the window values of the thread's own positions (they depend on the thread
//                       index only, like its twiddles), and the spectrum is stored with a row pitch - or as |X|^2, taken from the
//                       registers that hold the canonical spectrum, so that the write is half a spectrum.  It is a kernel of its own
//                       built from the Tiled<> helpers: fft_tiled_kernel keeps its code.  The arithmetic after the one rounded
//                       product is the sequence of fft_tiled_kernel<C, FWD, 1>, so the result equals transform_batch of the
//                       materialised frames bit for bit (tests/test_gpu_frames.py).
//   frames_gather_kernel, frames_rows_kernel, frames_ola_kernel
//                       the streaming kernels of the COMPOSED routes: frames x window -> dense scratch, scratch rows -> pitched rows
//                       or |X|^2, and the fixed-order overlap-add gather of the synthesis.
#pragma once
#include "fft_tiled.h"
#include "pf_handout.h"

namespace pf {

enum { FR_INTERNAL = 0, FR_ORDERED = 1, FR_POWER = 2 };

// WMODE: 0 = no window (no multiplication at all), 1 = the thread's window values resident in registers (2E scalars),
//        2 = the window in an LDS table behind the images, read with 16-byte accesses where it is used
template <class C, int OUT, int WMODE>
__global__ void __launch_bounds__(C::WG_THREADS, C::OCC)
fft_frames_kernel(const float* signal, size_t signal_stride, unsigned nframes, size_t hop, const float* __restrict__ window,
                  float* out, size_t out_stride, unsigned batch, const cx<float>* __restrict__ twg,
                  const cx<float>* __restrict__ twrg, unsigned* ctr) {
    typedef float T;
    typedef cx<T> CX;
    typedef Tiled<C, FWD, 1> K;
    typedef typename K::S0 S0;
    typedef typename K::SL SL;
    constexpr int n = C::n, E = C::E, TPT = C::TPT, CH = C::CH, NCH = C::NCH;
    constexpr int R0 = K::R0, RL = K::RL;
    static_assert(sizeof(typename C::real_t) == 4 && C::VEC == 2 && S0::PAIR && SL::PAIR, "float configurations only");
    static_assert(C::TWMODE == 0 || C::TWMODE == 3, "register twiddles only");
    static_assert(((n / RL) % 64 == 0 && (n / R0) % 64 == 0) || C::PADN == 0, "pad period vs operand stride");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int slot = threadIdx.x / TPT, t = threadIdx.x % TPT;
    CX* img = reinterpret_cast<CX*>(smem_raw) + (size_t)slot * C::IMG;
    T* imgs = reinterpret_cast<T*>(img);
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

        // ------------------------------------------------------------------ output
        K::pair_regs(v, t, w);   // v[u RL + d] = bin jm(t, u) + d n/RL of the half-complex spectrum; bin 0 = (DC, Nyquist)
        if constexpr (OUT == FR_POWER) {
            // |X|^2 straight from the registers: N/2 + 1 scalars per frame, 4-byte stores that consecutive threads coalesce
            if (active) {
#pragma unroll
                for (int u = 0; u < SL::B; ++u)
#pragma unroll
                    for (int d = 0; d < RL; ++d) {
                        const int k = K::template jm<C::NS - 1>(t, u) + d * (n / RL);
                        const CX x = v[u * RL + d];
                        if (k == 0) {
                            __builtin_nontemporal_store(x.x * x.x, dst);
                            __builtin_nontemporal_store(x.y * x.y, dst + n);
                        } else {
                            __builtin_nontemporal_store(x.x * x.x + x.y * x.y, dst + k);
                        }
                    }
            }
        } else if constexpr (OUT == FR_INTERNAL) {
#pragma unroll
            for (int u = 0; u < SL::B; ++u)
#pragma unroll
                for (int d = 0; d < RL; ++d) {
                    const int ip = K::template ipos<RL>(K::template jm<C::NS - 1>(t, u), d);
                    imgs[ip] = v[u * RL + d].x;
                    imgs[ip + 4] = v[u * RL + d].y;
                }
            K::xsync();
            const chunk16* im16 = reinterpret_cast<const chunk16*>(imgs);
            chunk16* d16o = reinterpret_cast<chunk16*>(dst);
            constexpr int CPB = 32 / CH;
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int c = t + TPT * i;
                const chunk16 o = im16[(c / CPB) * (C::IBS / CH) + (c % CPB)];
                if (active) __builtin_nontemporal_store(o, d16o + c);
            }
            K::xsync();
        } else {
#pragma unroll
            for (int u = 0; u < SL::B; ++u)
#pragma unroll
                for (int d = 0; d < RL; ++d) {
                    const int j = K::template jm<C::NS - 1>(t, u);
                    lds_st(img + j + C::PADN * (j >> 6) + K::nat_off(d * (n / RL)), v[u * RL + d]);
                }
            K::xsync();
            chunk16* d16 = reinterpret_cast<chunk16*>(dst);
#pragma unroll
            for (int i = 0; i < NCH; ++i) {
                const int c = tl + TPT * i;
                const CX a = lds_ld(img + phys_nat<C>(2 * c)), b = lds_ld(img + phys_nat<C>(2 * c + 1));
                chunk16 o;
                o.x = a.x; o.y = a.y; o.z = b.x; o.w = b.y;
                if (active) __builtin_nontemporal_store(o, d16 + c);
            }
            K::xsync();
        }
        if constexpr (!C::PREFETCH) K::load_raw(raw, src_of((size_t)gn * C::T_PER_WG + slot), t, true);
        g = gn;
    }
    if (dyn && threadIdx.x == 0) handout_rearm(ctr);
}

// LDS of fft_frames_kernel: the images and the counter slot of fft_tiled_kernel (these configurations have no twiddle table) + the window
template <class C> constexpr size_t frames_lds_bytes(int wmode) {
    return (size_t)C::T_PER_WG * C::IMG * 2 * sizeof(float) + 16 + (wmode == 2 ? (size_t)C::n * 2 * sizeof(float) : 0);
}

// ------------------------------------------------------------------------------------------------ composed routes
// frames v0 ... v0 + count - 1 (v = i nframes + f) x window -> dense rows of `row` scalars.  One thread per UNIT of U scalars (U = 4 / 2
// where the offsets allow 16-byte accesses, else 1); spp scalars per sample share one window value.
template <typename T, int U>
__global__ void frames_gather_kernel(const T* __restrict__ signal, size_t signal_stride, size_t nframes, size_t hop, int spp,
                                     const T* __restrict__ window, T* __restrict__ dst, size_t v0, size_t count, unsigned row) {
    const unsigned upr = row / U;
    const size_t units = count * upr;
    for (size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x; x < units; x += (size_t)gridDim.x * blockDim.x) {
        const size_t r = x / upr;
        const unsigned j = (unsigned)(x - r * upr) * U;
        const size_t v = v0 + r, i = v / nframes, f = v - i * nframes;
        const T* src = signal + i * signal_stride + f * hop + j;
        T a[U];
        if constexpr (U == 1) a[0] = src[0];
        else if constexpr (sizeof(T) * U == 16) {
            const vec4<float> c = *reinterpret_cast<const vec4<float>*>(src);
            __builtin_memcpy(a, &c, 16);
        }
        if (window) {
#pragma unroll
            for (int k = 0; k < U; ++k) a[k] = a[k] * window[(j + k) / spp];
        }
        if constexpr (U == 1) dst[r * row + j] = a[0];
        else {
            vec4<float> c;
            __builtin_memcpy(&c, a, 16);
            *reinterpret_cast<vec4<float>*>(dst + r * row + j) = c;
        }
    }
}

// dense rows (`row` scalars) -> rows with a pitch, one scalar per thread.  MODE 0: a copy (either side may be the pitched one);
// MODE 1: |X|^2 of a canonical REAL spectrum (row = N: bins 0 ... N/2, DC and Nyquist unpacked, N/2 + 1 scalars out);
// MODE 2: |X|^2 of a canonical complex spectrum (row = 2N -> N scalars out)
template <typename T, int MODE>
__global__ void frames_rows_kernel(const T* __restrict__ src, size_t src_stride, T* __restrict__ dst, size_t dst_stride, size_t count,
                                   unsigned row) {
    const unsigned per = MODE == 0 ? row : MODE == 1 ? row / 2 + 1 : row / 2;
    const size_t total = count * per;
    for (size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (size_t)gridDim.x * blockDim.x) {
        const size_t r = x / per;
        const unsigned k = (unsigned)(x - r * per);
        const T* s = src + r * src_stride;
        T o;
        if constexpr (MODE == 0) o = s[k];
        else if constexpr (MODE == 2) o = s[2 * k] * s[2 * k] + s[2 * k + 1] * s[2 * k + 1];
        else {
            if (k == 0) o = s[0] * s[0];
            else if (k == row / 2) o = s[1] * s[1];
            else o = s[2 * k] * s[2 * k] + s[2 * k + 1] * s[2 * k + 1];
        }
        dst[r * dst_stride + k] = o;
    }
}

// overlap-add as a GATHER with a fixed order: scalar e (sample s = e / spp) of signal i, s0 <= s < s1, is
//   scaling * ( sum over f ascending, 0 <= s - f hop < N, of  window[s - f hop] * y_f[e - f hop spp] ),
// each product and each addition rounded once, the sum started from its first term; 0 where no frame covers s.  `y` holds the
// backward-transformed frames fbase ... of every signal as dense rows (`fpitch` rows per signal).
template <typename T>
__global__ void frames_ola_kernel(const T* __restrict__ y, size_t fbase, size_t fpitch, size_t nframes, size_t hop, unsigned N, int spp,
                                  const T* __restrict__ window, T scaling, T* __restrict__ signal, size_t signal_stride, size_t nsignals,
                                  size_t s0, size_t s1) {
    const size_t per = (s1 - s0) * spp, total = nsignals * per;
    const size_t row = (size_t)N * spp;
    for (size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (size_t)gridDim.x * blockDim.x) {
        const size_t i = x / per, e = s0 * spp + (x - i * per), s = e / spp;
        const unsigned c = (unsigned)(e - s * spp);
        const size_t flo = s < N ? 0 : (s - N) / hop + 1;
        size_t fhi = s / hop;
        if (fhi > nframes - 1) fhi = nframes - 1;
        T acc = (T)0;
        bool first = true;
        for (size_t f = flo; f <= fhi; ++f) {
            const size_t j = s - f * hop;
            T term = y[(i * fpitch + (f - fbase)) * row + j * spp + c];
            if (window) term = window[j] * term;
            acc = first ? term : acc + term;
            first = false;
        }
        signal[i * signal_stride + e] = first ? (T)0 : scaling * acc;
    }
}

}  // namespace pf
