// libpffft_hip.so, translation unit of the polyphase filter bank (include/pffft_hip.h: pffft_hip_pfb_transform_batch,
// pffft_hip_pfb_route, pffft_hip_pfb_synthesis_batch): validation, route decision, the fused complex N = 1024 kernel's launch and the
// composed routes through the per-stream frame matrix (pf::Setup::frames and its helpers: pf_compose.h, shared with the frame entries of
// frames_tu.hip).  Kernels: fft_pfb.h.
#include "pf_compose.h"
#include "fft_pfb.h"

static_assert(pf::PFB_FUSED_MAX_TAPS == PFFFT_HIP_PFB_FUSED_MAX_TAPS, "the header's constant is the kernel's");

namespace pf {

static bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// ------------------------------------------------------------------------------------------------ route
// The fused kernel runs part A / part B of fft_c1024.h: its bits are transform_batch's only where transform_batch runs that family for
// the same layout, which is read from the setup's stored route.
static bool pfb_fusable_setup(const Setup* s, int output) {
    if (s->is_double || s->transform != PFFFT_COMPLEX || s->N != 1024 || s->kernel != K_C1024_F32) return false;
    if (output != FR_INTERNAL && output != FR_ORDERED) return false;
    return s->route[PFFFT_FORWARD][output == FR_INTERNAL ? 0 : 1].fam == FAM_C1024;
}

// (taps, hop) cells where the fused kernel is the default: only where it beat the composed route by more than the spread of identical
// runs in tools/pfb_bench.py on the MI355X.  A cell that is not listed stays composed and reachable through
// AB_PFB_FUSED.  Measured: taps 1 / 4 / 8 x hop N/2 / N, fused 2.1-3.5 x faster in all six against a spread below 1 %.  Exactly those
// cells are listed - none is listed by interpolation or on the byte model.
static bool pfb_fused_default(size_t taps, size_t hop) {
    return (taps == 1 || taps == 4 || taps == 8) && (hop == 512 || hop == 1024);
}

// the route of a call whose pointers are aligned (signal / out 16 bytes, prototype 8): true = fused
static bool pfb_route_fused(const Setup* s, size_t hop, size_t taps, size_t signal_stride, size_t out_stride, int output, const AbSel& sel) {
    if (sel.is(AB_PFB_COMPOSED)) return false;
    if (!pfb_fusable_setup(s, output)) return false;
    // 16-byte loads of every tap of every frame of every signal, 16-byte stores of every spectrum row; the LDS table holds the prototype
    if (hop % 2 || signal_stride % 4 || out_stride % 4 || taps > (size_t)PFB_FUSED_MAX_TAPS) return false;
    if (sel.is(AB_PFB_FUSED)) return true;
    // (any other selector may move transform_batch off the family this kernel shares its bits with: composed follows it)
    return !sel.any() && pfb_fused_default(taps, hop);
}

static int launch_pfb_c1024(Setup* s, const float* signal, size_t signal_stride, size_t nframes, size_t hop, const float* prototype,
                            size_t taps, float* out, size_t out_stride, size_t batch, int output, hipStream_t st) {
    // launched as launch_c1024 launches the persistent loop: ONE 8-wavefront workgroup per CU
    const size_t groups = (batch + C1024_WAVES - 1) / C1024_WAVES;
    const unsigned grid = (unsigned)std::min<size_t>((size_t)num_cus(), groups);
    const size_t lds = pfb_c1024_lds_bytes(taps);
    auto k = output == FR_INTERNAL ? fft_pfb_c1024_kernel<1> : fft_pfb_c1024_kernel<0>;
    int rc = allow_big_lds(k, lds);
    if (rc) return rc;
    unsigned* ctr = take_counters(s, st);
    hipLaunchKernelGGL(k, dim3(grid), dim3(C1024_WAVES * 64), lds, st, signal, signal_stride, (unsigned)nframes, 2 * hop, prototype,
                       (unsigned)taps, out, out_stride, (unsigned)batch, s->d_tw.as<cx<float>>(), ctr);
    PF_CHECK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------ composed pieces (pf_compose.h: the
// frame matrix, the row kernel's launch)
template <typename T, int U>
static int launch_fold(const T* signal, size_t signal_stride, size_t nframes, size_t hop_s, int spp, const T* prototype, size_t taps, T* X,
                       size_t v0, size_t cnt, size_t row, hipStream_t st) {
    const size_t upr = row / U;
    unsigned lpr = 1;
    while (lpr < 256 && lpr < upr) lpr *= 2;
    const size_t rpb = 256 / lpr;
    // eight resident workgroups of 256 threads per CU, each striding over the rows
    const size_t grid = std::max<size_t>(1, std::min<size_t>((cnt + rpb - 1) / rpb, (size_t)num_cus() * 8));
    hipLaunchKernelGGL((pfb_fold_kernel<T, U>), dim3((unsigned)grid), dim3(256), 0, st, signal, signal_stride, nframes, hop_s, spp, prototype,
                       (unsigned)taps, X, v0, cnt, (unsigned)row, lpr);
    PF_CHECK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------ the entry
template <typename T>
static int pfb_transform_batch(Setup* s, const T* signal, size_t signal_stride, size_t nsignals, size_t nframes, size_t hop,
                               const T* prototype, size_t taps, T* out, size_t out_stride, int output, hipStream_t st) {
    AnalysisArgs a;
    if (int rc = analysis_args<T>("pfb: ", s, signal, &signal_stride, nsignals, nframes, hop, out, &out_stride, output, &a, &taps, prototype))
        return rc == ARGS_EMPTY ? 0 : rc;

    s = for_device(s);
    if (int rc = ensure_device_any(s, st)) return rc;
    const AbSel sel = ab();
    if constexpr (sizeof(T) == 4) {
        // (the kernel counts frames in 32 bits: longer batches of ONE signal go out in slices; several signals that long are composed)
        if (pfb_route_fused(s, hop, taps, signal_stride, out_stride, output, sel) && aligned_to(signal, 16) && aligned_to(out, 16) &&
            aligned_to(prototype, 8) && (a.batch <= ROW_SLICE || nsignals == 1))
            return for_slices(a.batch, [&](size_t b0, size_t nb) {
                return launch_pfb_c1024(s, signal + b0 * a.hop_s, signal_stride, nsignals == 1 ? nb : nframes, hop, prototype, taps,
                                        out + b0 * out_stride, out_stride, nb, output, st);
            });
    }
    constexpr int U = 16 / (int)sizeof(T);
    const bool wide = aligned_to(signal, 16) && signal_stride % U == 0 && a.hop_s % U == 0 && a.row % U == 0;
    return analysis_composed<T>(s, a, out, out_stride, output, st, [&](T* X, size_t v0, size_t cnt) {
        return wide ? launch_fold<T, U>(signal, signal_stride, nframes, a.hop_s, (int)a.spp, prototype, taps, X, v0, cnt, a.row, st)
                    : launch_fold<T, 1>(signal, signal_stride, nframes, a.hop_s, (int)a.spp, prototype, taps, X, v0, cnt, a.row, st);
    });
}

// ------------------------------------------------------------------------------------------------ synthesis
// Mapping of the gather's tiles onto workgroups where no selector asks for one: the plain grid stride (false) or XCD-contiguous sweeps
// (true) - whichever tools/pfb_synth_bench.py measured faster on the MI355X.
constexpr bool PFB_SYN_XCD_DEFAULT = false;

template <typename T, int U, int SPP>
static int launch_syn_form(bool xcd, const T* y, size_t fbase, size_t fpitch, size_t nframes, size_t hop, size_t N, size_t span,
                           const T* g, T scaling, T* signal, size_t signal_stride, size_t nsignals, size_t s0, size_t s1, hipStream_t st) {
    const size_t units = nsignals * ((s1 - s0) * SPP / U);
    if (units == 0) return 0;
    const unsigned hop_mod = (unsigned)((hop * SPP) % (N * SPP));
    auto k = xcd ? pfb_syn_kernel<T, U, SPP, 1> : pfb_syn_kernel<T, U, SPP, 0>;
    return stream_launch(k, units, st, y, fbase, fpitch, nframes, hop, (unsigned)N, span, hop_mod, g, scaling, signal, signal_stride, nsignals, s0, s1);
}

struct SynForm { bool wide, xcd; };

template <typename T>
static int launch_syn(SynForm form, size_t spp, const T* y, size_t fbase, size_t fpitch, size_t nframes, size_t hop, size_t N, size_t span,
                      const T* g, T scaling, T* signal, size_t signal_stride, size_t nsignals, size_t s0, size_t s1, hipStream_t st) {
    constexpr int U = 16 / (int)sizeof(T);
#define PF_SYN(UU, SS) launch_syn_form<T, UU, SS>(form.xcd, y, fbase, fpitch, nframes, hop, N, span, g, scaling, signal, signal_stride, nsignals, s0, s1, st)
    if (spp == 1) return form.wide ? PF_SYN(U, 1) : PF_SYN(1, 1);
    return form.wide ? PF_SYN(U, 2) : PF_SYN(1, 2);
#undef PF_SYN
}

template <typename T>
static int pfb_synthesis_batch(Setup* s, const T* spectra, size_t spectra_stride, size_t nsignals, size_t nframes, size_t hop,
                               const T* prototype, size_t taps, T scaling, T* signal, size_t signal_stride, int ordered, hipStream_t st) {
    if (int rc = check_setup<T>(s)) return rc;
    if (hop == 0) return bad("pfb synthesis: hop == 0");
    if (taps == 0) return bad("pfb synthesis: taps == 0");
    if (!prototype) return bad("pfb synthesis: NULL prototype");
    if (nsignals == 0 || nframes == 0) return 0;
    const bool real = s->transform == PFFFT_REAL;
    const size_t spp = real ? 1 : 2, N = (size_t)s->N, row = s->vec_scalars, span = taps * N;
    if (spectra_stride == 0) spectra_stride = row;
    if (spectra_stride < row) return bad("pfb synthesis: spectra_stride smaller than one spectrum");
    const size_t samples = (nframes - 1) * hop + span;
    if (nsignals > 1 && signal_stride < samples * spp) return bad("pfb synthesis: signal_stride smaller than one signal's samples");
    if (!spectra || !signal) return bad("pfb synthesis: NULL spectra / signal");
    if (nsignals == 1) signal_stride = 0;   // (one signal: the stride is not read)

    const AbSel sel = ab();
    constexpr size_t U = 16 / sizeof(T);
    SynForm form;
    // wide: every unit of 16 bytes lies inside one frame's span and one period of it, and every access is aligned (the frame matrix is an
    // allocation of its own); the prototype is read GU = U / spp values at a time
    form.wide = !sel.is(AB_PFB_SYN_SCALAR) && (hop * spp) % U == 0 && signal_stride % U == 0 && row % U == 0 && aligned_to(signal, 16) &&
                aligned_to(prototype, real ? 16 : sizeof(T) * (U / 2));
    form.xcd = sel.is(AB_PFB_SYN_XCD) || (PFB_SYN_XCD_DEFAULT && !sel.is(AB_PFB_SYN_PLAIN));
    return synthesis_runs<T>(s, spectra, spectra_stride, nsignals, nframes, hop, span, synth_reach(span, hop), ordered, signal, signal_stride, st,
                             [&](const T* X, size_t fbase, size_t fpitch, size_t fend, T* sig, size_t sig_stride, size_t nsig, size_t s0, size_t s1) {
                                 return launch_syn<T>(form, spp, X, fbase, fpitch, fend, hop, N, span, prototype, scaling, sig, sig_stride, nsig, s0, s1, st);
                             });
}

}  // namespace pf

PF_EXPORT int pffft_hip_pfb_transform_batch(PFFFT_Setup* s, const float* signal, size_t signal_stride, size_t nsignals, size_t nframes,
                                            size_t hop, const float* prototype, size_t taps, float* out, size_t out_stride, int output,
                                            void* stream) {
    return pf::pfb_transform_batch<float>(s, signal, signal_stride, nsignals, nframes, hop, prototype, taps, out, out_stride, output,
                                          (hipStream_t)stream);
}
PF_EXPORT int pffftd_hip_pfb_transform_batch(PFFFTD_Setup* s, const double* signal, size_t signal_stride, size_t nsignals, size_t nframes,
                                             size_t hop, const double* prototype, size_t taps, double* out, size_t out_stride, int output,
                                             void* stream) {
    return pf::pfb_transform_batch<double>(s, signal, signal_stride, nsignals, nframes, hop, prototype, taps, out, out_stride, output,
                                           (hipStream_t)stream);
}

PF_EXPORT const char* pffft_hip_pfb_route(const void* setup, size_t hop, size_t taps, size_t signal_stride, size_t out_stride, int output) {
    const pf::Setup* s = pf::route_setup(setup, hop);
    if (!s || taps == 0 || output < 0 || output > 2) return "";
    if (out_stride == 0) out_stride = pf::frame_dims(s, output).out_row;
    return pf::pfb_route_fused(s, hop, taps, signal_stride, out_stride, output, pf::ab()) ? "fused" : "composed";
}

PF_EXPORT int pffft_hip_pfb_synthesis_batch(PFFFT_Setup* s, const float* spectra, size_t spectra_stride, size_t nsignals, size_t nframes,
                                            size_t hop, const float* prototype, size_t taps, float scaling, float* signal,
                                            size_t signal_stride, int ordered, void* stream) {
    return pf::pfb_synthesis_batch<float>(s, spectra, spectra_stride, nsignals, nframes, hop, prototype, taps, scaling, signal, signal_stride,
                                          ordered, (hipStream_t)stream);
}
PF_EXPORT int pffftd_hip_pfb_synthesis_batch(PFFFTD_Setup* s, const double* spectra, size_t spectra_stride, size_t nsignals, size_t nframes,
                                             size_t hop, const double* prototype, size_t taps, double scaling, double* signal,
                                             size_t signal_stride, int ordered, void* stream) {
    return pf::pfb_synthesis_batch<double>(s, spectra, spectra_stride, nsignals, nframes, hop, prototype, taps, scaling, signal, signal_stride,
                                           ordered, (hipStream_t)stream);
}
