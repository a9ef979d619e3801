// Averaged cross-spectra and coherence of two signals over overlapping frames (pffft_hip_frames_csd_batch, Welch's method): the kernels.
//
//   fft_csd_kernel              the FUSED route - fft_psd_kernel's run loop (a workgroup slot steps through the consecutive frames of ONE
//                               run, stores once per run) with the stage sequence run TWICE per frame: first on the x frame, whose E
//                               canonical bins stay in registers, then on the y frame, after which conj(X) Y (and |X|^2, |Y|^2) go into
//                               the accumulators.  One raw[] set: the y frame is requested after the first barrier of the x pass, the
//                               next x frame after the first barrier of the y pass.  A kernel of its own built from the Tiled<> helpers.
//                               XPF 0 requests the next x frame behind the products instead: 32 registers fewer during the y pass.
//   csd_runs_kernel             the COMPOSED route's accumulation: one thread per (run, bin) walks the run's rows of BOTH spectrum sets of
//                               the frame matrix in ascending order.
//   csd_coherence_reduce_kernel adds the four run partials of every group in ascending order and forms the ratio (coherence of averages
//                               longer than one run).  Cross and all-four rows of longer averages are plain sums of partial rows: they go
//                               through psd_reduce_kernel with the row length of their partials.
//
// The order is the contract (include/pffft_hip.h): per frame and bin  c_re = Xr Yr + Xi Yi,  c_im = Xr Yi - Xi Yr  (conj(X) Y), every
// product and every sum rounded once; the two real-only bins of a real setup give (X Y, +0); pxx and pyy are the POWER expressions of the
// frame entry.  Each of the four sums is accumulated as fft_psd.h accumulates: runs of PSD_RUN frames, f ascending, started from the first
// term, then the run partials ascending.  No atomics, no FMA (-ffp-contract=off), so every route gives the same bits.
#pragma once
#include "fft_psd.h"
#include "pf_handout.h"

namespace pf {

// PFFFT_HIP_CSD_* of include/pffft_hip.h
enum { CSD_CROSS = 0, CSD_ALL = 1, CSD_COHERENCE = 2 };

// scalars of one output row and of one run's partial row, P bins.  CROSS: (re, im) interleaved; ALL: Pxx[P] | Pyy[P] | Pxy[2P]; COHERENCE: P
// ratios - its partials are ALL rows, unscaled (the kernels of a longer coherence average are the ALL ones with scale 1).
constexpr size_t csd_row(int what, size_t P) { return what == CSD_CROSS ? 2 * P : what == CSD_ALL ? 4 * P : P; }
constexpr size_t csd_part_row(int what, size_t P) { return what == CSD_CROSS ? 2 * P : 4 * P; }

// The run numbering, the partial / output addressing and `scale` are fft_psd_kernel's: run r of this launch is run r mod rpg of output row
// row0 + r div rpg, row v = i G + gg is group gg of signal i, and the run's row goes to out + r out_stride.  WHAT = CSD_COHERENCE stores
// the ratio of the run's own sums (`scale` is not read): the caller launches it only where a group is one run.
template <class C, int WMODE, int WHAT, int XPF>
__global__ void __launch_bounds__(C::WG_THREADS, C::OCC)
fft_csd_kernel(const float* xsig, size_t x_stride, const float* ysig, size_t y_stride, unsigned G, unsigned navg, size_t hop,
               const float* __restrict__ window, float* out, size_t out_stride, size_t row0, unsigned nruns, float scale,
               const cx<float>* __restrict__ twg, const cx<float>* __restrict__ twrg, unsigned* ctr) {
    typedef float T;
    typedef cx<T> CX;
    typedef Tiled<C, FWD, 1> K;
    typedef typename K::S0 S0;
    typedef typename K::SL SL;
    constexpr int n = C::n, E = C::E, TPT = C::TPT, NCH = C::NCH;
    constexpr int R0 = K::R0, RL = K::RL;
    constexpr bool POW = WHAT != CSD_CROSS;   // |X|^2 and |Y|^2 next to the cross term
    constexpr int EP = POW ? E : 1;
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
    // length and first frame of a run (indices past the end name the last run: such slots recompute it and never store)
    auto len_of = [&](size_t r) -> unsigned {
        const unsigned j = (unsigned)(r < last ? r : last) % rpg;
        const unsigned left = navg - j * PSD_RUN;
        return left < PSD_RUN ? left : PSD_RUN;
    };
    auto src_of = [&](size_t r, const T*& xb, const T*& yb) {
        const unsigned rr = (unsigned)(r < last ? r : last);
        const unsigned q = rr / rpg, j = rr - q * rpg;
        const size_t v = row0 + q, i = v / G, gg = v - i * G;
        const size_t fo = (gg * navg + (size_t)j * PSD_RUN) * hop;
        xb = xsig + i * x_stride + fo;
        yb = ysig + i * y_stride + fo;
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
    const T *xbase, *ybase;
    src_of((size_t)g * C::T_PER_WG + slot, xbase, ybase);
    unsigned len = len_of((size_t)g * C::T_PER_WG + slot);
    unsigned bound = bound_of(g);
    chunk16 raw[NCH];
    K::load_raw(raw, xbase, t, true);
    for (unsigned it = 0; (size_t)g * C::T_PER_WG < nruns; ++it) {
        if (dyn && threadIdx.x == 0) pend = handout_grab(s_next, it, pend, ctr);
        const size_t tr = (size_t)g * C::T_PER_WG + slot;
        const bool active = tr < nruns;
        unsigned gn = 0;
        const T *nxbase = xbase, *nybase = ybase;
        // acc_im[j] of the real-only bin 0 carries the Nyquist product, as the spectrum packs it; likewise nxx / nyy next to pxx / pyy
        T acc_re[E], acc_im[E], pxx[EP], pyy[EP], nxx = (T)0, nyy = (T)0;
#pragma unroll
        for (int i = 0; i < E; ++i) { acc_re[i] = (T)0; acc_im[i] = (T)0; }
#pragma unroll
        for (int i = 0; i < EP; ++i) { pxx[i] = (T)0; pyy[i] = (T)0; }
        for (unsigned fi = 0; fi < bound; ++fi) {
            CX v[E], xs[E];
            int tl = t;
            asm volatile("" : "+v"(tl));
            // raw chunk x window, ONE rounding per scalar: the frame entry's input step
            auto take_raw = [&]() {
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
            };
            // the stages behind the first barrier (the sequence of fft_tiled_kernel), then the canonical bins in v
            auto finish_pass = [&]() {
                if constexpr (C::NS > 1) { K::template xread<0>(v, t, img); K::xsync(); K::template butterflies<1>(v, t, w, twt); }
                if constexpr (C::NS > 2) { K::template xwrite<1>(v, t, img); K::xsync(); K::template xread<1>(v, t, img); K::xsync(); K::template butterflies<2>(v, t, w, twt); }
                if constexpr (C::NS > 3) { K::template xwrite<2>(v, t, img); K::xsync(); K::template xread<2>(v, t, img); K::xsync(); K::template butterflies<3>(v, t, w, twt); }
                if constexpr (C::NS > 4) { K::template xwrite<3>(v, t, img); K::xsync(); K::template xread<3>(v, t, img); K::xsync(); K::template butterflies<4>(v, t, w, twt); }
                K::pair_regs(v, t, w);   // v[u RL + d] = bin jm(t, u) + d n/RL of the half-complex spectrum; bin 0 = (DC, Nyquist)
            };

            // -------------------------------------------------------------- the x frame
            take_raw();
            K::template butterflies<0>(v, t, w, twt);
            if constexpr (C::NS > 1) K::template xwrite<0>(v, t, img);
            __syncthreads();  // publishes s_next; first half of exchange 0
            if (fi == 0) gn = handout_next(dyn, s_next, it, g);
            // the y frame of this step (a shorter run repeats its last one)
            const T* ysrc = ybase + (size_t)(fi < len ? fi : len - 1) * hop;
            if constexpr (C::PREFETCH) K::load_raw(raw, ysrc, t, true);
            finish_pass();
#pragma unroll
            for (int i = 0; i < E; ++i) xs[i] = v[i];
            if constexpr (!C::PREFETCH) K::load_raw(raw, ysrc, t, true);

            // -------------------------------------------------------------- the y frame
            take_raw();
            K::template butterflies<0>(v, t, w, twt);
            if constexpr (C::NS > 1) K::template xwrite<0>(v, t, img);
            __syncthreads();
            // what follows: the run's next x frame, after the group's last step the next run's first
            const T* nsrc;
            if (fi + 1 < bound) nsrc = xbase + (size_t)(fi + 1 < len ? fi + 1 : len - 1) * hop;
            else { src_of((size_t)gn * C::T_PER_WG + slot, nxbase, nybase); nsrc = nxbase; }
            if constexpr (C::PREFETCH && XPF) K::load_raw(raw, nsrc, t, true);
            finish_pass();

            // -------------------------------------------------------------- conj(X) Y, |X|^2, |Y|^2 into the accumulators
            const bool take = fi < len, first = fi == 0;
#pragma unroll
            for (int u = 0; u < SL::B; ++u)
#pragma unroll
                for (int d = 0; d < RL; ++d) {
                    const int k = K::template jm<C::NS - 1>(t, u) + d * (n / RL), j = u * RL + d;
                    const CX a = xs[j], b = v[j];
                    T cre, cim;
                    if (k == 0) { cre = a.x * b.x; cim = a.y * b.y; }
                    else { cre = a.x * b.x + a.y * b.y; cim = a.x * b.y - a.y * b.x; }
                    if (take) {
                        acc_re[j] = first ? cre : acc_re[j] + cre;
                        acc_im[j] = first ? cim : acc_im[j] + cim;
                    }
                    if constexpr (POW) {
                        T px, py;
                        if (k == 0) {
                            px = a.x * a.x; py = b.x * b.x;
                            const T qx = a.y * a.y, qy = b.y * b.y;
                            if (take) { nxx = first ? qx : nxx + qx; nyy = first ? qy : nyy + qy; }
                        } else {
                            px = a.x * a.x + a.y * a.y; py = b.x * b.x + b.y * b.y;
                        }
                        if (take) { pxx[j] = first ? px : pxx[j] + px; pyy[j] = first ? py : pyy[j] + py; }
                    }
                }
            if constexpr (!(C::PREFETCH && XPF)) K::load_raw(raw, nsrc, t, true);
        }
        // ------------------------------------------------------------------ one store per run: 4-byte stores (out needs scalar alignment only)
        if (active) {
            T* dst = out + tr * out_stride;
            constexpr int P = n + 1;
#pragma unroll
            for (int u = 0; u < SL::B; ++u)
#pragma unroll
                for (int d = 0; d < RL; ++d) {
                    const int k = K::template jm<C::NS - 1>(t, u) + d * (n / RL), j = u * RL + d;
                    const bool edge = k == 0;
                    const T im = edge ? (T)0 : acc_im[j];
                    if constexpr (WHAT == CSD_COHERENCE) {
                        __builtin_nontemporal_store(coherence_ratio(acc_re[j], im, pxx[j], pyy[j]), dst + k);
                        if (edge) __builtin_nontemporal_store(coherence_ratio(acc_im[j], (T)0, nxx, nyy), dst + n);
                    } else {
                        T* c = dst + (WHAT == CSD_ALL ? 2 * P : 0);
                        __builtin_nontemporal_store(scale * acc_re[j], c + 2 * k);
                        __builtin_nontemporal_store(scale * im, c + 2 * k + 1);
                        if (edge) {
                            __builtin_nontemporal_store(scale * acc_im[j], c + 2 * n);
                            __builtin_nontemporal_store(scale * (T)0, c + 2 * n + 1);
                        }
                        if constexpr (WHAT == CSD_ALL) {
                            __builtin_nontemporal_store(scale * pxx[j], dst + k);
                            __builtin_nontemporal_store(scale * pyy[j], dst + P + k);
                            if (edge) {
                                __builtin_nontemporal_store(scale * nxx, dst + n);
                                __builtin_nontemporal_store(scale * nyy, dst + P + n);
                            }
                        }
                    }
                }
        }
        g = gn;
        xbase = nxbase;
        ybase = nybase;
        len = len_of((size_t)g * C::T_PER_WG + slot);
        bound = bound_of(g);
    }
    if (dyn && threadIdx.x == 0) handout_rearm(ctr);
}

// ------------------------------------------------------------------------------------------------ composed route
// psd_runs_kernel over TWO sets of canonical spectra: X and Y hold the x and the y frames from the first frame of run r0 on, in dense rows
// of `row` scalars.  One thread per (run, bin).  CROSS and ALL store scale * partial in the row layout of csd_row; COHERENCE stores the
// ratio of the run's own sums.
template <typename T, int REAL, int WHAT>
__global__ void csd_runs_kernel(const T* __restrict__ X, const T* __restrict__ Y, unsigned row, size_t r0, size_t count, size_t navg,
                                size_t rpg, T* __restrict__ dst, size_t dst_stride, T scale) {
    const unsigned P = REAL ? row / 2 + 1 : row / 2;
    const size_t total = count * P;
    const size_t f00 = (r0 / rpg) * navg + (r0 % rpg) * PSD_RUN;
    for (size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (size_t)gridDim.x * blockDim.x) {
        const size_t rl = x / P, r = r0 + rl;
        const unsigned k = (unsigned)(x - rl * P);
        const size_t q = r / rpg, j = r - q * rpg;
        const size_t left = navg - j * PSD_RUN, len = left < PSD_RUN ? left : PSD_RUN;
        const size_t off = (q * navg + j * PSD_RUN - f00) * row;
        const T *s = X + off, *u = Y + off;
        const bool edge = REAL && (k == 0 || k == row / 2);          // the two real-only bins: s[0] and s[1] of a canonical real spectrum
        const unsigned e = REAL && k == row / 2 ? 1 : 2 * k;
        T are = (T)0, aim = (T)0, axx = (T)0, ayy = (T)0;
        for (size_t f = 0; f < len; ++f, s += row, u += row) {
            T cre, cim, px, py;
            if (edge) {
                cre = s[e] * u[e]; cim = (T)0; px = s[e] * s[e]; py = u[e] * u[e];
            } else {
                const T xr = s[e], xi = s[e + 1], yr = u[e], yi = u[e + 1];
                cre = xr * yr + xi * yi; cim = xr * yi - xi * yr;
                px = xr * xr + xi * xi; py = yr * yr + yi * yi;
            }
            are = f == 0 ? cre : are + cre;
            aim = f == 0 ? cim : aim + cim;
            if constexpr (WHAT != CSD_CROSS) { axx = f == 0 ? px : axx + px; ayy = f == 0 ? py : ayy + py; }
        }
        T* d = dst + rl * dst_stride;
        if constexpr (WHAT == CSD_COHERENCE) d[k] = coherence_ratio(are, aim, axx, ayy);
        else {
            T* c = d + (WHAT == CSD_ALL ? 2 * (size_t)P : 0);
            c[2 * k] = scale * are;
            c[2 * k + 1] = scale * aim;
            if constexpr (WHAT == CSD_ALL) { d[k] = scale * axx; d[P + k] = scale * ayy; }
        }
    }
}

// partial rows of ALL layout (4P scalars each, rpg per output row, dense, unscaled) -> coherence rows: each of the four sums added in
// ascending order, started from the first, then the ratio.  Grid stride, one bin per thread.
template <typename T>
__global__ void csd_coherence_reduce_kernel(const T* __restrict__ part, size_t rpg, unsigned P, size_t rows, T* __restrict__ out,
                                            size_t out_stride) {
    const size_t total = rows * P, W = 4 * (size_t)P;
    for (size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (size_t)gridDim.x * blockDim.x) {
        const size_t v = x / P;
        const unsigned k = (unsigned)(x - v * P);
        const T* s = part + v * rpg * W;
        T axx = s[k], ayy = s[P + k], are = s[2 * (size_t)P + 2 * k], aim = s[2 * (size_t)P + 2 * k + 1];
        for (size_t j = 1; j < rpg; ++j) {
            s += W;
            axx = axx + s[k]; ayy = ayy + s[P + k]; are = are + s[2 * (size_t)P + 2 * k]; aim = aim + s[2 * (size_t)P + 2 * k + 1];
        }
        out[v * out_stride + k] = coherence_ratio(are, aim, axx, ayy);
    }
}

}  // namespace pf
