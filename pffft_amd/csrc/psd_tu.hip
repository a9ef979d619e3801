// libpffft_hip.so, translation unit of the averaged-power-spectrum entries (include/pffft_hip.h: pffft_hip_frames_psd_batch,
// pffft_hip_frames_psd_route): validation, route decision, the fused kernel's instantiations and the composed route through the per-stream
// frame matrix.  Kernels: fft_psd.h; the frame matrix and the framing kernel: pf_compose.h / fft_frames.h.
#include "pf_compose.h"
#include "fft_psd.h"

static_assert(pf::PSD_RUN == PFFFT_HIP_PSD_RUN, "the run length is part of the contract");

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

// the route of a call whose pointers are 16-byte aligned: true = fused
static bool psd_route_fused(const Setup* s, size_t hop, size_t signal_stride, size_t navg, const AbSel& sel) {
    if (sel.is(AB_PSD_COMPOSED)) return false;
    if (!psd_fusable_setup(s, nullptr, true)) return false;
    if (hop % 4 || signal_stride % 4) return false;       // 16-byte loads of every frame and every signal; the rows are stored scalar by scalar
    if (navg > 0xffffffffull) return false;               // (the kernel counts the frames of one average in 32 bits)
    return sel.is(AB_PSD_FUSED) || psd_fused_default(s->n);
}

static int launch_psd_fused(Setup* s, const PsdSel& e, const float* signal, size_t signal_stride, size_t G, size_t navg, size_t hop,
                            const float* window, float* dst, size_t dst_stride, size_t row0, size_t nruns, float scale, hipStream_t st) {
    // the launch rule of the transform kernel: the `oneshot` of the stored route that psd_fusable_setup read `e` from (frames_tu.hip)
    LoopLaunch ll;
    if (int rc = loop_launch(s, st, e.fn, e.wg, e.lds, (nruns + e.t_per_wg - 1) / e.t_per_wg, s->route[PFFFT_FORWARD][1].oneshot, &ll)) return rc;
    hipLaunchKernelGGL(e.fn, dim3(ll.grid), dim3(e.wg), e.lds, st, signal, signal_stride, (unsigned)G, (unsigned)navg, hop, window, dst,
                       dst_stride, row0, (unsigned)nruns, scale, s->d_tw.as<cx<float>>(), s->d_twr.as<cx<float>>(), ll.ctr);
    PF_CHECK(hipGetLastError());
    return 0;
}

template <typename T>
static int psd_batch(Setup* s, const T* signal, size_t signal_stride, size_t nsignals, size_t nframes, size_t hop, const T* window,
                     size_t navg, T scaling, T* out, size_t out_stride, hipStream_t st) {
    AnalysisArgs a;
    int rc = analysis_args<T>("psd: ", s, signal, &signal_stride, nsignals, nframes, hop, out, &out_stride, FR_POWER, &a, nullptr, nullptr, &navg);
    if (rc) return rc == ARGS_EMPTY ? 0 : rc;
    const bool real = a.real;
    const size_t spp = a.spp, row = a.row, P = a.out_row, hop_s = a.hop_s;
    const size_t G = nframes / navg, V = nsignals * G;     // V output rows; row v = i G + g
    const size_t rpg = (navg + PSD_RUN - 1) / PSD_RUN;     // runs per group
    s = for_device(s);
    if ((rc = ensure_device_any(s))) return rc;
    const AbSel sel = ab();
    PsdSel e;
    bool fused = false;
    if constexpr (sizeof(T) == 4)
        fused = psd_route_fused(s, hop, signal_stride, navg, sel) && aligned16(signal) && (!window || aligned16(window)) && G <= 0xffffffffull &&
                psd_fusable_setup(s, &e, window != nullptr);

    // Averages of one run are scaled and stored by the run itself.  Longer ones go through the partial buffer in whole groups: `vstep`
    // output rows per pass, then the reduction of those rows.
    size_t vstep = V;
    if (rpg > 1) vstep = cap_rows(rpg * P * sizeof(T));
    if (fused) vstep = std::min(vstep, std::max<size_t>(1, ROW_SLICE / rpg));   // (the kernel counts the runs of a launch in 32 bits)
    vstep = std::min(vstep, V);
    // composed: the frames of whole runs through the frame matrix (as large as one run needs where a run exceeds the cap)
    const size_t lfull = std::min<size_t>(navg, PSD_RUN);
    const size_t crun = std::max<size_t>(1, cap_rows(row * sizeof(T)) / lfull);
    auto first_frame = [&](size_t r) { return (r / rpg) * navg + (r % rpg) * PSD_RUN; };   // in the numbering v = i nframes + f

    std::unique_lock<std::mutex> lkp(s->psd.mu, std::defer_lock), lkf(s->frames.mu, std::defer_lock);
    void* buf = nullptr;
    T* part = nullptr;
    T* X = nullptr;
    if (rpg > 1) {
        lkp.lock();
        if ((rc = scratch_buffer(s->psd, st, vstep * rpg * P * sizeof(T), "the partial buffer", &buf))) return rc;
        part = (T*)buf;
    }
    if (!fused) {
        lkf.lock();
        const size_t rows_x = std::min(V * navg, std::min(crun, vstep * rpg) * lfull);
        if ((rc = scratch_buffer(s->frames, st, rows_x * row * sizeof(T), "the frame matrix", &buf))) return rc;
        X = (T*)buf;
    }
    for (size_t v0 = 0; v0 < V; v0 += vstep) {
        const size_t rows = std::min(V - v0, vstep), ra = v0 * rpg, rb = (v0 + rows) * rpg;
        T* dst = rpg == 1 ? out + v0 * out_stride : part;
        const size_t dstride = rpg == 1 ? out_stride : P;
        const T scale = rpg == 1 ? scaling : (T)1;
        if (fused) {
            if constexpr (sizeof(T) == 4)
                if ((rc = launch_psd_fused(s, e, signal, signal_stride, G, navg, hop_s, window, dst, dstride, v0, rb - ra, scale, st))) return rc;
        } else {
            for (size_t r = ra; r < rb; r += crun) {
                const size_t cnt = std::min(rb - r, crun), fa = first_frame(r), nfr = first_frame(r + cnt) - fa;
                if ((rc = launch_gather<T>(signal, signal_stride, nframes, hop_s, spp, window, X, fa, nfr, row, st))) return rc;
                if ((rc = transform_batch_any(s, X, X, nfr, PFFFT_FORWARD, 1, st))) return rc;
                if (real)
                    hipLaunchKernelGGL((psd_runs_kernel<T, 1>), dim3(stream_grid(cnt * P)), dim3(256), 0, st, X, (unsigned)row, r, cnt, navg, rpg,
                                       dst + (r - ra) * dstride, dstride, scale);
                else
                    hipLaunchKernelGGL((psd_runs_kernel<T, 0>), dim3(stream_grid(cnt * P)), dim3(256), 0, st, X, (unsigned)row, r, cnt, navg, rpg,
                                       dst + (r - ra) * dstride, dstride, scale);
                PF_CHECK(hipGetLastError());
            }
        }
        if (rpg > 1) {
            hipLaunchKernelGGL((psd_reduce_kernel<T>), dim3(stream_grid(rows * P)), dim3(256), 0, st, part, rpg, (unsigned)P, rows, scaling,
                               out + v0 * out_stride, out_stride);
            PF_CHECK(hipGetLastError());
        }
    }
    return 0;
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
    const pf::Setup* s = static_cast<const pf::Setup*>(setup);
    if (!s || s->magic != pf::MAGIC || hop == 0) return "";
    return pf::psd_route_fused(s, hop, signal_stride, navg, pf::ab()) ? "fused" : "composed";
}
