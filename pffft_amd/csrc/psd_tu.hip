// libpffft_hip.so, translation unit of the averaged-power-spectrum entries (include/pffft_hip.h: pffft_hip_frames_psd_batch,
// pffft_hip_frames_psd_route): validation, route decision, the fused kernel's instantiations and the composed route through the per-stream
// frame matrix.  Kernels: fft_psd.h; the frame matrix and the framing kernel: pf_compose.h / fft_frames.h.
#include "pf_compose.h"
#include "fft_psd.h"

static_assert(pf::PSD_RUN == PFFFT_HIP_PSD_RUN && pf::AVG_RUN == pf::PSD_RUN, "the run length is part of the contract");

namespace pf {

// ------------------------------------------------------------------------------------------------ fused
typedef void (*PsdFn)(const float*, size_t, unsigned, unsigned, size_t, const float*, float*, size_t, size_t, unsigned, float,
                      const cx<float>*, const cx<float>*, unsigned*);
typedef KernelSel<PsdFn> PsdSel;

// Window values: resident in registers (WMODE 1), as in the frame kernel.  With the E + 1 accumulators on top of them the resource remarks
// of the three configurations still show no scratch and the occupancy of fft_frames_kernel<C, FR_POWER, 1>, so the LDS
// twin (WMODE 2) is not needed.
constexpr int PSD_WMODE = 1;

template <class C>
static PsdSel psd_sel(bool windowed) {
    PsdSel e;
    e.wg = C::WG_THREADS; e.t_per_wg = C::T_PER_WG;
    e.lds = frames_lds_bytes<C>(windowed ? PSD_WMODE : 0);
    e.fn = windowed ? fft_psd_kernel<C, PSD_WMODE> : fft_psd_kernel<C, 0>;
    return e;
}

// The frame entry's rule: p_f equals the POWER output of pffft_hip_frames_transform_batch bit for bit only on the configuration
// transform_batch(ordered = 1) runs on, so that is read from the setup's stored route.
static bool psd_fusable_setup(const Setup* s, PsdSel* e, bool windowed) {
    return visit_tiled_cfg(s, s->route[PFFFT_FORWARD][1], [&](auto tag) {
        if (e) *e = psd_sel<typename decltype(tag)::type>(windowed);
    });
}

// sizes where the fused kernel is the default: all three until a measurement says otherwise (tests/test_gpu_psd.py times every cell; a size
// that loses returns false here and stays reachable through AB_PSD_FUSED)
static bool psd_fused_default(int n) {
    (void)n;
    return true;
}

// the route of a call whose pointers are 16-byte aligned: true = fused (the rows are stored scalar by scalar: no rule for out_stride)
static bool psd_route_fused(const Setup* s, size_t hop, size_t signal_stride, size_t navg, const AbSel& sel) {
    return averaged_route_fused(sel, AB_PSD_COMPOSED, AB_PSD_FUSED, [&] { return psd_fusable_setup(s, nullptr, true); }, hop, signal_stride, 0, navg,
                                psd_fused_default(s->n));
}

template <typename T>
static int psd_batch(Setup* s, const T* signal, size_t signal_stride, size_t nsignals, size_t nframes, size_t hop, const T* window,
                     size_t navg, T scaling, T* out, size_t out_stride, hipStream_t st) {
    AnalysisArgs a;
    int rc = analysis_args<T>("psd: ", s, signal, &signal_stride, nsignals, nframes, hop, out, &out_stride, FR_POWER, &a, nullptr, nullptr, &navg);
    if (rc) return rc == ARGS_EMPTY ? 0 : rc;
    const size_t spp = a.spp, row = a.row, P = a.out_row, hop_s = a.hop_s;
    const size_t G = nframes / navg, V = nsignals * G;     // V output rows; row v = i G + g
    s = for_device(s);
    if ((rc = ensure_device_any(s, st))) return rc;
    PsdSel e;
    bool fused = false;
    if constexpr (sizeof(T) == 4)
        fused = psd_route_fused(s, hop, signal_stride, navg, ab()) && aligned16(signal) && (!window || aligned16(window)) && G <= 0xffffffffull &&
                psd_fusable_setup(s, &e, window != nullptr);
    const AvgPlan p = avg_plan(V, navg, P * sizeof(T), row * sizeof(T), fused);
    return averaged_runs<T>(s, st, p, P, row, out, out_stride, scaling,
        [&](T* dst, size_t dstride, size_t row0, size_t nruns, T scale) {
            if constexpr (sizeof(T) == 4) {
                // the launch rule of the transform kernel: the `oneshot` of the stored route that psd_fusable_setup read `e` from (frames_tu.hip)
                LoopLaunch ll;
                if ((rc = loop_launch(s, st, e.fn, e.wg, e.lds, (nruns + e.t_per_wg - 1) / e.t_per_wg, s->route[PFFFT_FORWARD][1].oneshot, &ll))) return rc;
                hipLaunchKernelGGL(e.fn, dim3(ll.grid), dim3(e.wg), e.lds, st, signal, signal_stride, (unsigned)G, (unsigned)navg, hop_s, window, dst,
                                   dstride, row0, (unsigned)nruns, scale, s->d_tw.as<cx<float>>(), s->d_twr.as<cx<float>>(), ll.ctr);
                PF_CHECK(hipGetLastError());
            }
            return 0;
        },
        [&](T* X, size_t r, size_t cnt, size_t fa, size_t nfr, T* dst, size_t dstride, T scale) {
            if ((rc = launch_gather<T>(signal, signal_stride, nframes, hop_s, spp, window, X, fa, nfr, row, st))) return rc;
            if ((rc = transform_batch_any(s, X, X, nfr, PFFFT_FORWARD, 1, st))) return rc;
            return with_flag(a.real, [&](auto R) {
                return stream_launch(psd_runs_kernel<T, decltype(R)::value>, cnt * P, st, X, (unsigned)row, r, cnt, navg, p.rpg, dst, dstride, scale);
            });
        },
        [&](T* part, size_t rows, T* out_rows) {
            return stream_launch(psd_reduce_kernel<T>, rows * P, st, part, p.rpg, (unsigned)P, rows, scaling, out_rows, out_stride);
        });
}

}  // namespace pf

PF_EXPORT int pffft_hip_frames_psd_batch(PFFFT_Setup* s, const float* signal, size_t signal_stride, size_t nsignals, size_t nframes, size_t hop,
                                         const float* window, size_t navg, float scaling, float* out, size_t out_stride, void* stream) {
    return pf::psd_batch<float>(s, signal, signal_stride, nsignals, nframes, hop, window, navg, scaling, out, out_stride, (hipStream_t)stream);
}
PF_EXPORT int pffftd_hip_frames_psd_batch(PFFFTD_Setup* s, const double* signal, size_t signal_stride, size_t nsignals, size_t nframes,
                                          size_t hop, const double* window, size_t navg, double scaling, double* out, size_t out_stride,
                                          void* stream) {
    return pf::psd_batch<double>(s, signal, signal_stride, nsignals, nframes, hop, window, navg, scaling, out, out_stride, (hipStream_t)stream);
}

PF_EXPORT const char* pffft_hip_frames_psd_route(const void* setup, size_t hop, size_t signal_stride, size_t navg) {
    const pf::Setup* s = pf::route_setup(setup, hop);
    if (!s) return "";
    return pf::psd_route_fused(s, hop, signal_stride, navg, pf::ab()) ? "fused" : "composed";
}
