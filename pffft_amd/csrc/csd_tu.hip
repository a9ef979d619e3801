// libpffft_hip.so, translation unit of the averaged-cross-spectrum entries (include/pffft_hip.h: pffft_hip_frames_csd_batch,
// pffft_hip_frames_csd_route): validation, route decision, the fused kernel's instantiations and the composed route through the two halves
// of the per-stream frame matrix.  Kernels: fft_csd.h; the frame matrix, the framing kernel and the argument rules: pf_compose.h.
#include "pf_compose.h"
#include "fft_csd.h"

static_assert(pf::CSD_CROSS == PFFFT_HIP_CSD_CROSS && pf::CSD_ALL == PFFFT_HIP_CSD_ALL && pf::CSD_COHERENCE == PFFFT_HIP_CSD_COHERENCE,
              "the selectors of `what` are part of the contract");

namespace pf {

// ------------------------------------------------------------------------------------------------ fused
typedef void (*CsdFn)(const float*, size_t, const float*, size_t, unsigned, unsigned, size_t, const float*, float*, size_t, size_t, unsigned,
                      float, const cx<float>*, const cx<float>*, unsigned*);
typedef KernelSel<CsdFn> CsdSel;

// Which variant of a cell (configuration, windowed, what) is adopted - arithmetic on the resource remarks of every instantiation
// (-Rpass-analysis=kernel-resource-usage; the table of DESIGN.md §3.22), not a measurement: the first that builds with NO scratch among
//   window in registers (WMODE 1), next x frame requested after the first barrier of the y pass (XPF 1);
//   window in LDS (WMODE 2), XPF 1;
//   window in LDS, next x frame requested behind the products (XPF 0: its 32 registers are free during the y pass);
// wmode < 0: no such variant, the cell stays composed.  The x spectrum and the complex accumulator on top of the PSD kernel's registers
// leave no room for resident window values in any configuration; CROSS fits with the late request (N = 1024 also with the early one); the
// four sums of ALL / COHERENCE spill in every variant of every configuration.
struct CsdVariant { int wmode, xpf; };
template <class C> constexpr CsdVariant csd_variant(bool windowed, int what) {
    if (what != CSD_CROSS) return {-1, 0};
    return {windowed ? 2 : 0, C::n == 512 ? 1 : 0};
}

template <class C, int WHAT>
static bool csd_sel_what(bool windowed, CsdSel* e) {
    constexpr CsdVariant VW = csd_variant<C>(true, WHAT), V0 = csd_variant<C>(false, WHAT);
    if ((windowed ? VW.wmode : V0.wmode) < 0) return false;
    if (!e) return true;
    e->wg = C::WG_THREADS; e->t_per_wg = C::T_PER_WG;
    if (windowed) {
        if constexpr (VW.wmode >= 0) { e->lds = frames_lds_bytes<C>(VW.wmode); e->fn = fft_csd_kernel<C, VW.wmode, WHAT, VW.xpf>; }
    } else {
        if constexpr (V0.wmode >= 0) { e->lds = frames_lds_bytes<C>(0); e->fn = fft_csd_kernel<C, 0, WHAT, V0.xpf>; }
    }
    return true;
}
template <class C>
static bool csd_sel(bool windowed, int what, CsdSel* e) {
    return what == CSD_CROSS ? csd_sel_what<C, CSD_CROSS>(windowed, e) : what == CSD_ALL ? csd_sel_what<C, CSD_ALL>(windowed, e)
                                                                                           : csd_sel_what<C, CSD_COHERENCE>(windowed, e);
}

// The PSD entry's rule: X_f and Y_f equal the ordered spectra of transform_batch bit for bit only on the configuration
// transform_batch(ordered = 1) runs on, so that is read from the setup's stored route.  `kwhat`: the WHAT of the kernel to launch.
static bool csd_fusable_setup(const Setup* s, CsdSel* e, bool windowed, int kwhat) {
    bool ok = false;
    return visit_tiled_cfg(s, s->route[PFFFT_FORWARD][1], [&](auto tag) { ok = csd_sel<typename decltype(tag)::type>(windowed, kwhat, e); }) && ok;
}

// the kernel a (what, runs per group) runs: a coherence average longer than one run leaves ALL partials
static int csd_kernel_what(int what, size_t navg) { return what == CSD_COHERENCE && navg > PSD_RUN ? CSD_ALL : what; }

// cells where the fused kernel is the default: those tests/test_gpu_csd.py timed ahead of the composed route by more than the spread of
// identical rounds; the others stay reachable through AB_CSD_FUSED
static bool csd_fused_default(int n, int what) {
    (void)n; (void)what;
    return true;
}

// the route of a call whose pointers are 16-byte aligned: true = fused.  navg == 0 (every frame of a signal, length unknown here) is
// answered for the windowed kernels of a long average.
static bool csd_route_fused(const Setup* s, size_t hop, size_t x_stride, size_t y_stride, size_t navg, int what, const AbSel& sel) {
    if (sel.is(AB_CSD_COMPOSED)) return false;
    const int kw = csd_kernel_what(what, navg == 0 ? PSD_RUN + 1 : navg);
    if (!csd_fusable_setup(s, nullptr, true, kw) || !csd_fusable_setup(s, nullptr, false, kw)) return false;
    if (hop % 4 || x_stride % 4 || y_stride % 4) return false;   // 16-byte loads of every frame of either signal
    if (navg > 0xffffffffull) return false;                      // (the kernel counts the frames of one average in 32 bits)
    return sel.is(AB_CSD_FUSED) || csd_fused_default(s->n, what);
}

static int launch_csd_fused(Setup* s, const CsdSel& e, const float* x, size_t x_stride, const float* y, size_t y_stride, size_t G,
                            size_t navg, size_t hop, const float* window, float* dst, size_t dst_stride, size_t row0, size_t nruns,
                            float scale, hipStream_t st) {
    LoopLaunch ll;
    if (int rc = loop_launch(s, st, e.fn, e.wg, e.lds, (nruns + e.t_per_wg - 1) / e.t_per_wg, s->route[PFFFT_FORWARD][1].oneshot, &ll)) return rc;
    hipLaunchKernelGGL(e.fn, dim3(ll.grid), dim3(e.wg), e.lds, st, x, x_stride, y, y_stride, (unsigned)G, (unsigned)navg, hop, window, dst,
                       dst_stride, row0, (unsigned)nruns, scale, s->d_tw.as<cx<float>>(), s->d_twr.as<cx<float>>(), ll.ctr);
    PF_CHECK(hipGetLastError());
    return 0;
}

template <typename T, int REAL>
static void launch_csd_runs(int kwhat, const T* X, const T* Y, size_t row, size_t P, size_t r, size_t cnt, size_t navg, size_t rpg, T* dst,
                            size_t dstride, T scale, hipStream_t st) {
    const dim3 grid(stream_grid(cnt * P)), block(256);
    if (kwhat == CSD_CROSS)
        hipLaunchKernelGGL((csd_runs_kernel<T, REAL, CSD_CROSS>), grid, block, 0, st, X, Y, (unsigned)row, r, cnt, navg, rpg, dst, dstride, scale);
    else if (kwhat == CSD_ALL)
        hipLaunchKernelGGL((csd_runs_kernel<T, REAL, CSD_ALL>), grid, block, 0, st, X, Y, (unsigned)row, r, cnt, navg, rpg, dst, dstride, scale);
    else
        hipLaunchKernelGGL((csd_runs_kernel<T, REAL, CSD_COHERENCE>), grid, block, 0, st, X, Y, (unsigned)row, r, cnt, navg, rpg, dst, dstride, scale);
}

template <typename T>
static int csd_batch(Setup* s, const T* x, size_t x_stride, const T* y, size_t y_stride, size_t nsignals, size_t nframes, size_t hop,
                     const T* window, size_t navg, T scaling, int what, T* out, size_t out_stride, hipStream_t st) {
    const char* PRE = "csd: ";
    int rc = check_setup<T>(s);
    if (rc) return rc;
    if (hop == 0) return bad_in(PRE, "hop == 0");
    if (what != CSD_CROSS && what != CSD_ALL && what != CSD_COHERENCE) return bad_in(PRE, "unknown what");
    AnalysisArgs a;
    // the shared rules on x; the output row depends on `what` and is checked below, so the rule for a power row sees a stride that fits
    size_t any_stride = ~(size_t)0;
    rc = analysis_args<T>(PRE, s, x, &x_stride, nsignals, nframes, hop, out, &any_stride, FR_POWER, &a, nullptr, nullptr, &navg);
    if (rc) return rc == ARGS_EMPTY ? 0 : rc;
    const bool real = a.real;
    const size_t spp = a.spp, row = a.row, P = a.out_row, hop_s = a.hop_s;
    const size_t orow = csd_row(what, P);
    if (out_stride == 0) out_stride = orow;
    if (out_stride < orow) return bad_in(PRE, "out_stride smaller than one output row");
    if (nsignals > 1 && y_stride < ((nframes - 1) * hop + a.N) * spp) return bad_in(PRE, "y_stride smaller than one signal's samples");
    if (!y) return bad_in(PRE, "NULL y");
    if (nsignals == 1) y_stride = 0;
    const size_t G = nframes / navg, V = nsignals * G;     // V output rows; row v = i G + g
    const size_t rpg = (navg + PSD_RUN - 1) / PSD_RUN;     // runs per group
    const int kwhat = csd_kernel_what(what, navg);         // what the run kernels store
    const size_t W = csd_part_row(what, P);                // scalars of one run's partial row
    s = for_device(s);
    if ((rc = ensure_device_any(s))) return rc;
    const AbSel sel = ab();
    CsdSel e;
    bool fused = false;
    if constexpr (sizeof(T) == 4)
        fused = csd_route_fused(s, hop, x_stride, y_stride, navg, what, sel) && aligned16(x) && aligned16(y) && (!window || aligned16(window)) &&
                G <= 0xffffffffull && csd_fusable_setup(s, &e, window != nullptr, kwhat);

    // As in the PSD entry: averages of one run are finished by the run itself; longer ones go through the partial buffer in whole groups,
    // `vstep` output rows per pass, then the reduction of those rows.
    size_t vstep = V;
    if (rpg > 1) vstep = cap_rows(rpg * W * sizeof(T));
    if (fused) vstep = std::min(vstep, std::max<size_t>(1, ROW_SLICE / rpg));   // (the kernel counts the runs of a launch in 32 bits)
    vstep = std::min(vstep, V);
    // composed: the x and the y frames of whole runs in the two halves of the frame matrix - the cap holds for both together
    const size_t lfull = std::min<size_t>(navg, PSD_RUN);
    const size_t crun = std::max<size_t>(1, cap_rows(2 * row * sizeof(T)) / lfull);
    auto first_frame = [&](size_t r) { return (r / rpg) * navg + (r % rpg) * PSD_RUN; };   // in the numbering v = i nframes + f

    std::unique_lock<std::mutex> lkp(s->psd.mu, std::defer_lock), lkf(s->frames.mu, std::defer_lock);
    void* buf = nullptr;
    T* part = nullptr;
    T* X = nullptr;
    size_t half = 0;                                       // rows of one half of the frame matrix
    if (rpg > 1) {
        lkp.lock();
        if ((rc = scratch_buffer(s->psd, st, vstep * rpg * W * sizeof(T), "the partial buffer", &buf))) return rc;
        part = (T*)buf;
    }
    if (!fused) {
        lkf.lock();
        half = std::min(V * navg, std::min(crun, vstep * rpg) * lfull);
        if ((rc = scratch_buffer(s->frames, st, 2 * half * row * sizeof(T), "the frame matrix", &buf))) return rc;
        X = (T*)buf;
    }
    for (size_t v0 = 0; v0 < V; v0 += vstep) {
        const size_t rows = std::min(V - v0, vstep), ra = v0 * rpg, rb = (v0 + rows) * rpg;
        T* dst = rpg == 1 ? out + v0 * out_stride : part;
        const size_t dstride = rpg == 1 ? out_stride : W;
        const T scale = rpg == 1 ? scaling : (T)1;
        if (fused) {
            if constexpr (sizeof(T) == 4)
                if ((rc = launch_csd_fused(s, e, x, x_stride, y, y_stride, G, navg, hop_s, window, dst, dstride, v0, rb - ra, scale, st))) return rc;
        } else {
            for (size_t r = ra; r < rb; r += crun) {
                const size_t cnt = std::min(rb - r, crun), fa = first_frame(r), nfr = first_frame(r + cnt) - fa;
                T* Y = X + nfr * row;                      // (dense behind the x rows: ONE transform_batch over both)
                if ((rc = launch_gather<T>(x, x_stride, nframes, hop_s, spp, window, X, fa, nfr, row, st))) return rc;
                if ((rc = launch_gather<T>(y, y_stride, nframes, hop_s, spp, window, Y, fa, nfr, row, st))) return rc;
                if ((rc = transform_batch_any(s, X, X, 2 * nfr, PFFFT_FORWARD, 1, st))) return rc;
                if (real) launch_csd_runs<T, 1>(kwhat, X, Y, row, P, r, cnt, navg, rpg, dst + (r - ra) * dstride, dstride, scale, st);
                else launch_csd_runs<T, 0>(kwhat, X, Y, row, P, r, cnt, navg, rpg, dst + (r - ra) * dstride, dstride, scale, st);
                PF_CHECK(hipGetLastError());
            }
        }
        if (rpg > 1) {
            if (what == CSD_COHERENCE)
                hipLaunchKernelGGL((csd_coherence_reduce_kernel<T>), dim3(stream_grid(rows * P)), dim3(256), 0, st, part, rpg, (unsigned)P, rows,
                                   out + v0 * out_stride, out_stride);
            else   // cross and all-four rows: the sum of the partial rows, scalar by scalar
                hipLaunchKernelGGL((psd_reduce_kernel<T>), dim3(stream_grid(rows * W)), dim3(256), 0, st, part, rpg, (unsigned)W, rows, scaling,
                                   out + v0 * out_stride, out_stride);
            PF_CHECK(hipGetLastError());
        }
    }
    return 0;
}

}  // namespace pf

PF_EXPORT int pffft_hip_frames_csd_batch(PFFFT_Setup* s, const float* x, size_t x_stride, const float* y, size_t y_stride, size_t nsignals,
                                         size_t nframes, size_t hop, const float* window, size_t navg, float scaling, int what, float* out,
                                         size_t out_stride, void* stream) {
    return pf::csd_batch<float>(s, x, x_stride, y, y_stride, nsignals, nframes, hop, window, navg, scaling, what, out, out_stride,
                                (hipStream_t)stream);
}
PF_EXPORT int pffftd_hip_frames_csd_batch(PFFFTD_Setup* s, const double* x, size_t x_stride, const double* y, size_t y_stride, size_t nsignals,
                                          size_t nframes, size_t hop, const double* window, size_t navg, double scaling, int what, double* out,
                                          size_t out_stride, void* stream) {
    return pf::csd_batch<double>(s, x, x_stride, y, y_stride, nsignals, nframes, hop, window, navg, scaling, what, out, out_stride,
                                 (hipStream_t)stream);
}

PF_EXPORT const char* pffft_hip_frames_csd_route(const void* setup, size_t hop, size_t x_stride, size_t y_stride, size_t navg, int what) {
    const pf::Setup* s = static_cast<const pf::Setup*>(setup);
    if (!s || s->magic != pf::MAGIC || hop == 0) return "";
    if (what != pf::CSD_CROSS && what != pf::CSD_ALL && what != pf::CSD_COHERENCE) return "";
    return pf::csd_route_fused(s, hop, x_stride, y_stride, navg, what, pf::ab()) ? "fused" : "composed";
}
