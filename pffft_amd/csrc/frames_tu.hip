// libpffft_hip.so, translation unit of the windowed overlapping-frame entries (include/pffft_hip.h: pffft_hip_frames_transform_batch,
// pffft_hip_frames_overlap_add_batch, pffft_hip_frames_route): validation, route decision, the fused kernel's instantiations and the
// composed routes through the per-stream frame matrix.  Kernels: fft_frames.h; the frame matrix and its helpers: pf_compose.h.
#include "pf_compose.h"

namespace pf {

// ------------------------------------------------------------------------------------------------ fused analysis
typedef void (*FramesFn)(const float*, size_t, unsigned, size_t, const float*, float*, size_t, unsigned, const cx<float>*,
                         const cx<float>*, unsigned*);
typedef KernelSel<FramesFn> FramesSel;

// Window values: resident in registers (WMODE 1; 32 VGPRs) - the resource remarks of the three configurations show no scratch and the
// occupancy of the unframed kernel with them.  WMODE 2 (LDS table) is the twin kept for configurations where they would not.
constexpr int FRAMES_WMODE = 1;

template <class C>
static FramesSel frames_sel(int output, bool windowed) {
    FramesSel e;
    e.wg = C::WG_THREADS; e.t_per_wg = C::T_PER_WG;
    e.lds = frames_lds_bytes<C>(windowed ? FRAMES_WMODE : 0);
    if (windowed) {
        e.fn = output == FR_POWER ? fft_frames_kernel<C, FR_POWER, FRAMES_WMODE>
               : output == FR_ORDERED ? fft_frames_kernel<C, FR_ORDERED, FRAMES_WMODE> : fft_frames_kernel<C, FR_INTERNAL, FRAMES_WMODE>;
    } else {
        e.fn = output == FR_POWER ? fft_frames_kernel<C, FR_POWER, 0>
               : output == FR_ORDERED ? fft_frames_kernel<C, FR_ORDERED, 0> : fft_frames_kernel<C, FR_INTERNAL, 0>;
    }
    return e;
}

// The framed kernel runs on the configuration of the forward route of the same layout (visit_tiled_cfg); everything else has none.
static const Route& frames_route(const Setup* s, int output) { return s->route[PFFFT_FORWARD][output == FR_INTERNAL ? 0 : 1]; }

static bool frames_fusable_setup(const Setup* s, int output, FramesSel* e, bool windowed) {
    return visit_tiled_cfg(s, frames_route(s, output), [&](auto tag) {
        if (e) *e = frames_sel<typename decltype(tag)::type>(output, windowed);
    });
}

// (size, output) cells where the fused kernel is the default: fused wherever it beat the composed route by more than the spread of
// identical runs in tools/frames_bench.py on the MI355X - all of them (2.2-4.5 x against a spread below 2 %).  A cell
// that loses on a later measurement returns false here and stays reachable through AB_FRAMES_FUSED.
static bool frames_fused_default(int n, int output) {
    (void)n; (void)output;
    return true;
}

// the route of an analysis call whose pointers are 16-byte aligned: true = fused
static bool frames_route_fused(const Setup* s, size_t hop, size_t signal_stride, size_t out_stride, int output, const AbSel& sel) {
    if (sel.is(AB_FRAMES_COMPOSED)) return false;
    if (!frames_fusable_setup(s, output, nullptr, true)) return false;
    // 16-byte loads of every frame and every signal; 16-byte stores of every spectrum row (|X|^2 rows are stored scalar by scalar)
    if (hop % 4 || signal_stride % 4) return false;
    if (output != FR_POWER && out_stride % 4) return false;
    return sel.is(AB_FRAMES_FUSED) || frames_fused_default(s->n, output);
}

// The launch rule of the transform kernel: the `oneshot` of the stored route whose configuration `e` was read from.  It equals
// env().oneshot for every setup that has a framed kernel today (real float, n = 512 to 2048); the PSD and DCT entries do the same.
static int launch_frames_fused(Setup* s, const FramesSel& e, int oneshot, const float* signal, size_t signal_stride, size_t nframes, size_t hop,
                               const float* window, float* out, size_t out_stride, size_t batch, hipStream_t st) {
    LoopLaunch ll;
    if (int rc = loop_launch(s, st, e.fn, e.wg, e.lds, (batch + e.t_per_wg - 1) / e.t_per_wg, oneshot, &ll)) return rc;
    hipLaunchKernelGGL(e.fn, dim3(ll.grid), dim3(e.wg), e.lds, st, signal, signal_stride, (unsigned)nframes, hop, window, out,
                       out_stride, (unsigned)batch, s->d_tw.as<cx<float>>(), s->d_twr.as<cx<float>>(), ll.ctr);
    PF_CHECK(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------ analysis
template <typename T>
static int frames_transform_batch(Setup* s, const T* signal, size_t signal_stride, size_t nsignals, size_t nframes, size_t hop,
                                  const T* window, T* out, size_t out_stride, int output, hipStream_t st) {
    AnalysisArgs a;
    if (int rc = analysis_args<T>("frames: ", s, signal, &signal_stride, nsignals, nframes, hop, out, &out_stride, output, &a))
        return rc == ARGS_EMPTY ? 0 : rc;

    s = for_device(s);
    if (int rc = ensure_device_any(s, st)) return rc;
    const AbSel sel = ab();
    if constexpr (sizeof(T) == 4) {
        FramesSel e;
        // (the kernel counts frames in 32 bits: longer batches of ONE signal go out in slices; several signals that long are composed)
        if (frames_route_fused(s, hop, signal_stride, out_stride, output, sel) && aligned16(signal) && (!window || aligned16(window)) &&
            (output == FR_POWER || aligned16(out)) && frames_fusable_setup(s, output, &e, window != nullptr) &&
            (a.batch <= ROW_SLICE || nsignals == 1)) {
            const int oneshot = frames_route(s, output).oneshot;
            return for_slices(a.batch, [&](size_t b0, size_t nb) {
                return launch_frames_fused(s, e, oneshot, signal + b0 * a.hop_s, signal_stride, nsignals == 1 ? nb : nframes, a.hop_s, window,
                                           out + b0 * out_stride, out_stride, nb, st);
            });
        }
    }
    return analysis_composed<T>(s, a, out, out_stride, output, st, [&](T* X, size_t v0, size_t cnt) {
        return launch_gather<T>(signal, signal_stride, nframes, a.hop_s, a.spp, window, X, v0, cnt, a.row, st);
    });
}

// ------------------------------------------------------------------------------------------------ synthesis
template <typename T>
static int launch_ola(const T* y, size_t fbase, size_t fpitch, size_t nframes, size_t hop, size_t N, size_t spp, const T* window, T scaling,
                      T* signal, size_t signal_stride, size_t nsignals, size_t s0, size_t s1, hipStream_t st) {
    return stream_launch(frames_ola_kernel<T>, nsignals * (s1 - s0) * spp, st, y, fbase, fpitch, nframes, hop, (unsigned)N, (int)spp, window, scaling,
                         signal, signal_stride, nsignals, s0, s1);
}

template <typename T>
static int frames_overlap_add_batch(Setup* s, const T* spectra, size_t spectra_stride, size_t nsignals, size_t nframes, size_t hop,
                                    const T* window, T scaling, T* signal, size_t signal_stride, int ordered, hipStream_t st) {
    if (int rc = check_setup<T>(s)) return rc;
    if (hop == 0) return bad("frames: hop == 0");
    if (nsignals == 0 || nframes == 0) return 0;
    const size_t spp = s->transform == PFFFT_REAL ? 1 : 2, N = (size_t)s->N, row = s->vec_scalars;
    if (spectra_stride == 0) spectra_stride = row;
    if (spectra_stride < row) return bad("frames: spectra_stride smaller than one spectrum");
    if (nsignals > 1 && signal_stride < ((nframes - 1) * hop + N) * spp) return bad("frames: signal_stride smaller than one signal's samples");
    if (!spectra || !signal) return bad("frames: NULL spectra / signal");
    return synthesis_runs<T>(s, spectra, spectra_stride, nsignals, nframes, hop, N, 0, ordered, signal, signal_stride, st,
                             [&](const T* X, size_t fbase, size_t fpitch, size_t fend, T* sig, size_t sig_stride, size_t nsig, size_t s0, size_t s1) {
                                 return launch_ola<T>(X, fbase, fpitch, fend, hop, N, spp, window, scaling, sig, sig_stride, nsig, s0, s1, st);
                             });
}

}  // namespace pf

PF_EXPORT int pffft_hip_frames_transform_batch(PFFFT_Setup* s, const float* signal, size_t signal_stride, size_t nsignals, size_t nframes,
                                               size_t hop, const float* window, float* out, size_t out_stride, int output, void* stream) {
    return pf::frames_transform_batch<float>(s, signal, signal_stride, nsignals, nframes, hop, window, out, out_stride, output,
                                             (hipStream_t)stream);
}
PF_EXPORT int pffftd_hip_frames_transform_batch(PFFFTD_Setup* s, const double* signal, size_t signal_stride, size_t nsignals, size_t nframes,
                                                size_t hop, const double* window, double* out, size_t out_stride, int output, void* stream) {
    return pf::frames_transform_batch<double>(s, signal, signal_stride, nsignals, nframes, hop, window, out, out_stride, output,
                                              (hipStream_t)stream);
}
PF_EXPORT int pffft_hip_frames_overlap_add_batch(PFFFT_Setup* s, const float* spectra, size_t spectra_stride, size_t nsignals, size_t nframes,
                                                 size_t hop, const float* window, float scaling, float* signal, size_t signal_stride,
                                                 int ordered, void* stream) {
    return pf::frames_overlap_add_batch<float>(s, spectra, spectra_stride, nsignals, nframes, hop, window, scaling, signal, signal_stride,
                                               ordered, (hipStream_t)stream);
}
PF_EXPORT int pffftd_hip_frames_overlap_add_batch(PFFFTD_Setup* s, const double* spectra, size_t spectra_stride, size_t nsignals,
                                                  size_t nframes, size_t hop, const double* window, double scaling, double* signal,
                                                  size_t signal_stride, int ordered, void* stream) {
    return pf::frames_overlap_add_batch<double>(s, spectra, spectra_stride, nsignals, nframes, hop, window, scaling, signal, signal_stride,
                                                ordered, (hipStream_t)stream);
}

PF_EXPORT const char* pffft_hip_frames_route(const void* setup, size_t hop, size_t signal_stride, size_t out_stride, int output) {
    const pf::Setup* s = pf::route_setup(setup, hop);
    if (!s || output < 0 || output > 2) return "";
    if (out_stride == 0) out_stride = pf::frame_dims(s, output).out_row;
    return pf::frames_route_fused(s, hop, signal_stride, out_stride, output, pf::ab()) ? "fused" : "composed";
}
