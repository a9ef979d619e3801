// Averaged power spectra over overlapping frames (pffft_hip_frames_psd_batch, Welch's method): the kernels.
//
//   fft_psd_kernel    the FUSED route - the framed, windowing loader and the stage sequence of fft_frames_kernel<C, FR_POWER, WMODE>, with a
//                     RUN of up to PSD_RUN consecutive frames of one average as the unit of work instead of a frame: a workgroup slot steps
//                     through its run's frames in order, forms |X|^2 in the registers that hold the canonical spectrum exactly as the POWER
//                     branch does, adds it into E + 1 accumulator registers per thread and stores ONCE per run.  It is a kernel of its own
//                     built from the Tiled<> helpers: fft_frames_kernel keeps its code.
//   psd_runs_kernel   the COMPOSED route's accumulation: one thread per (run, bin) walks the run's spectrum rows of the frame matrix in
//                     ascending order with the |X|^2 expressions of frames_rows_kernel MODE 1 / 2.
//   psd_reduce_kernel adds the run partials of every group in ascending order and scales (averages longer than one run).
//
// The order is the contract (include/pffft_hip.h): a run's partial is p_f0 + p_f1 + ... with f ascending, started from the first term, every
// addition rounded once; a group's value is the sum of its run partials, run ascending, started from the first; one product by `scaling`.
// No atomics, no FMA (the library is built with -ffp-contract=off), so both routes give the same bits.
#pragma once
#include "fft_frames.h"
#include "pf_handout.h"

namespace pf {

constexpr unsigned PSD_RUN = 32;   // PFFFT_HIP_PSD_RUN of include/pffft_hip.h

// Run r (r < nruns; runs per group rpg = ceil(navg / PSD_RUN)) of this launch is run j = r mod rpg of output row row0 + r div rpg; row
// v = i G + gg is group gg of signal i: frames gg navg + j PSD_RUN ... of that signal, min(PSD_RUN, navg - j PSD_RUN) of them.  The run's
// result, times `scale`, is stored at out + r out_stride (the caller passes the output rows and its scaling where rpg == 1, the partial
// buffer and 1 otherwise).  Runs and the frames of one average are counted in 32 bits, offsets in 64.
template <class C, int WMODE>
__global__ void __launch_bounds__(C::WG_THREADS, C::OCC)
fft_psd_kernel(const float* signal, size_t signal_stride, unsigned G, unsigned navg, size_t hop, const float* __restrict__ window,
               float* out, size_t out_stride, size_t row0, unsigned nruns, float scale, const cx<float>* __restrict__ twg,
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
    const unsigned rpg = (navg + PSD_RUN - 1) / PSD_RUN;
    const size_t last = (size_t)nruns - 1;
    // first frame and length of a run (indices past the end name the last run: such slots recompute it and never store)
    auto len_of = [&](size_t r) -> unsigned {
        const unsigned j = (unsigned)(r < last ? r : last) % rpg;
        const unsigned left = navg - j * PSD_RUN;
        return left < PSD_RUN ? left : PSD_RUN;
    };
    auto src_of = [&](size_t r) -> const T* {
        const unsigned rr = (unsigned)(r < last ? r : last);
        const unsigned q = rr / rpg, j = rr - q * rpg;
        const size_t v = row0 + q, i = v / G, gg = v - i * G;
        return signal + i * signal_stride + (gg * navg + (size_t)j * PSD_RUN) * hop;
    };
    // the slots of a workgroup share its barriers: every slot steps through as many frames as the longest run of the group has
    auto bound_of = [&](size_t grp) -> unsigned {
        unsigned m = 1;
        for (int sl = 0; sl < C::T_PER_WG; ++sl) {
            const size_t r = grp * C::T_PER_WG + sl;
            if (r < nruns) { const unsigned l = len_of(r); m = l > m ? l : m; }
        }
        return m;
    };
    const T* base = src_of((size_t)g * C::T_PER_WG + slot);
    unsigned len = len_of((size_t)g * C::T_PER_WG + slot);
    unsigned bound = bound_of(g);
    chunk16 raw[NCH];
    K::load_raw(raw, base, t, true);
    for (unsigned it = 0; (size_t)g * C::T_PER_WG < nruns; ++it) {
        if (dyn && threadIdx.x == 0) pend = handout_grab(s_next, it, pend, ctr);
        const size_t tr = (size_t)g * C::T_PER_WG + slot;
        const bool active = tr < nruns;
        unsigned gn = 0;
        const T* nbase = base;
        T acc[E], nyq = (T)0;
#pragma unroll
        for (int i = 0; i < E; ++i) acc[i] = (T)0;
        for (unsigned fi = 0; fi < bound; ++fi) {
            CX v[E];
            int tl = t;
            asm volatile("" : "+v"(tl));

            // -------------------------------------------------------------- input: raw chunk x window, ONE rounding per scalar
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

            // -------------------------------------------------------------- transform (the sequence of fft_tiled_kernel)
            K::template butterflies<0>(v, t, w, twt);
            if constexpr (C::NS > 1) K::template xwrite<0>(v, t, img);
            __syncthreads();  // publishes s_next; first half of exchange 0
            if (fi == 0) gn = handout_next(dyn, s_next, it, g);
            // what follows: the run's next frame (a shorter run repeats its last one), after the group's last pass the next run's first
            const T* nsrc;
            if (fi + 1 < bound) nsrc = base + (size_t)(fi + 1 < len ? fi + 1 : len - 1) * hop;
            else nsrc = nbase = src_of((size_t)gn * C::T_PER_WG + slot);
            if constexpr (C::PREFETCH) K::load_raw(raw, nsrc, t, true);
            if constexpr (C::NS > 1) { K::template xread<0>(v, t, img); K::xsync(); K::template butterflies<1>(v, t, w, twt); }
            if constexpr (C::NS > 2) { K::template xwrite<1>(v, t, img); K::xsync(); K::template xread<1>(v, t, img); K::xsync(); K::template butterflies<2>(v, t, w, twt); }
            if constexpr (C::NS > 3) { K::template xwrite<2>(v, t, img); K::xsync(); K::template xread<2>(v, t, img); K::xsync(); K::template butterflies<3>(v, t, w, twt); }
            if constexpr (C::NS > 4) { K::template xwrite<3>(v, t, img); K::xsync(); K::template xread<3>(v, t, img); K::xsync(); K::template butterflies<4>(v, t, w, twt); }

            // -------------------------------------------------------------- |X|^2 as the POWER branch forms it, into the accumulators
            K::pair_regs(v, t, w);   // v[u RL + d] = bin jm(t, u) + d n/RL of the half-complex spectrum; bin 0 = (DC, Nyquist)
            const bool take = fi < len, first = fi == 0;
#pragma unroll
            for (int u = 0; u < SL::B; ++u)
#pragma unroll
                for (int d = 0; d < RL; ++d) {
                    const int k = K::template jm<C::NS - 1>(t, u) + d * (n / RL);
                    const CX x = v[u * RL + d];
                    T p;
                    if (k == 0) {
                        p = x.x * x.x;
                        const T q = x.y * x.y;
                        if (take) nyq = first ? q : nyq + q;
                    } else {
                        p = x.x * x.x + x.y * x.y;
                    }
                    if (take) acc[u * RL + d] = first ? p : acc[u * RL + d] + p;
                }
            if constexpr (!C::PREFETCH) K::load_raw(raw, nsrc, t, true);
        }
        // ------------------------------------------------------------------ one store per run: 4-byte stores that consecutive threads coalesce
        if (active) {
            T* dst = out + tr * out_stride;
#pragma unroll
            for (int u = 0; u < SL::B; ++u)
#pragma unroll
                for (int d = 0; d < RL; ++d) {
                    const int k = K::template jm<C::NS - 1>(t, u) + d * (n / RL);
                    __builtin_nontemporal_store(scale * acc[u * RL + d], dst + k);
                    if (k == 0) __builtin_nontemporal_store(scale * nyq, dst + n);
                }
        }
        g = gn;
        base = nbase;
        len = len_of((size_t)g * C::T_PER_WG + slot);
        bound = bound_of(g);
    }
    if (dyn && threadIdx.x == 0) handout_rearm(ctr);
}

// ------------------------------------------------------------------------------------------------ composed route
// Runs r0 ... r0 + count - 1 of the whole call (run r: run j = r mod rpg of output row r div rpg, so its frames follow those of run r - 1 in
// the numbering v = i nframes + f) over canonical spectra in dense rows of `row` scalars; X holds the frames from the first frame of run
// r0 on.  One thread per (run, bin).  REAL: |X|^2 of a canonical real spectrum (row = N: bins 0 ... N/2, DC and Nyquist unpacked), else of a
// canonical complex one (row = 2N) - the expressions of frames_rows_kernel MODE 1 / 2.  scale * partial -> dst + (r - r0) dst_stride.
template <typename T, int REAL>
__global__ void psd_runs_kernel(const T* __restrict__ X, unsigned row, size_t r0, size_t count, size_t navg, size_t rpg, T* __restrict__ dst,
                                size_t dst_stride, T scale) {
    const unsigned per = REAL ? row / 2 + 1 : row / 2;
    const size_t total = count * per;
    const size_t f00 = (r0 / rpg) * navg + (r0 % rpg) * PSD_RUN;
    for (size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (size_t)gridDim.x * blockDim.x) {
        const size_t rl = x / per, r = r0 + rl;
        const unsigned k = (unsigned)(x - rl * per);
        const size_t q = r / rpg, j = r - q * rpg;
        const size_t left = navg - j * PSD_RUN, len = left < PSD_RUN ? left : PSD_RUN;
        const T* s = X + (q * navg + j * PSD_RUN - f00) * row;
        T acc = (T)0;
        for (size_t f = 0; f < len; ++f, s += row) {
            T o;
            if constexpr (!REAL) o = s[2 * k] * s[2 * k] + s[2 * k + 1] * s[2 * k + 1];
            else {
                if (k == 0) o = s[0] * s[0];
                else if (k == row / 2) o = s[1] * s[1];
                else o = s[2 * k] * s[2 * k] + s[2 * k + 1] * s[2 * k + 1];
            }
            acc = f == 0 ? o : acc + o;
        }
        dst[rl * dst_stride + k] = scale * acc;
    }
}

// partial rows (P scalars each, rpg per output row, dense) -> out rows: the partials of a row added in ascending order, started from the
// first, times `scale`.  Grid stride, one scalar per thread.
template <typename T>
__global__ void psd_reduce_kernel(const T* __restrict__ part, size_t rpg, unsigned P, size_t rows, T scale, T* __restrict__ out,
                                  size_t out_stride) {
    const size_t total = rows * P;
    for (size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (size_t)gridDim.x * blockDim.x) {
        const size_t v = x / P;
        const unsigned k = (unsigned)(x - v * P);
        const T* s = part + v * rpg * P + k;
        T acc = s[0];
        for (size_t j = 1; j < rpg; ++j) acc = acc + s[j * P];
        out[v * out_stride + k] = scale * acc;
    }
}

}  // namespace pf
