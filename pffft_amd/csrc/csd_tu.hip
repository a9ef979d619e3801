// libpffft_hip.so, translation unit of the averaged-cross-spectrum entries (include/pffft_hip.h: pffft_hip_frames_csd_batch,
// pffft_hip_frames_csd_route): validation, route decision, the fused kernel's instantiations and the composed route through the two halves
// of the per-stream frame matrix.  Kernels: fft_csd.h; the frame matrix, the framing kernel and the argument rules: pf_compose.h.
#include "pf_compose.h"
#include "fft_csd.h"

static_assert(pf::CSD_CROSS == PFFFT_HIP_CSD_CROSS && pf::CSD_ALL == PFFFT_HIP_CSD_ALL && pf::CSD_COHERENCE == PFFFT_HIP_CSD_COHERENCE,
              "the selectors of `what` are part of the contract");
static_assert(pf::AVG_RUN == pf::PSD_RUN, "the plan of pf_compose.h and the kernels count the same runs");

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
template <class F>
static auto with_what(int what, F&& f) { return with_one_of<CSD_CROSS, CSD_ALL, CSD_COHERENCE>(what, f); }
template <class C>
static bool csd_sel(bool windowed, int what, CsdSel* e) {
    return with_what(what, [&](auto W) { return csd_sel_what<C, decltype(W)::value>(windowed, e); });
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
    const int kw = csd_kernel_what(what, navg == 0 ? PSD_RUN + 1 : navg);
    return averaged_route_fused(sel, AB_CSD_COMPOSED, AB_CSD_FUSED,
                                [&] { return csd_fusable_setup(s, nullptr, true, kw) && csd_fusable_setup(s, nullptr, false, kw); }, hop, x_stride,
                                y_stride, navg, csd_fused_default(s->n, what));
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
    const size_t spp = a.spp, row = a.row, P = a.out_row, hop_s = a.hop_s;
    const size_t orow = csd_row(what, P);
    if (out_stride == 0) out_stride = orow;
    if (out_stride < orow) return bad_in(PRE, "out_stride smaller than one output row");
    if (nsignals > 1 && y_stride < ((nframes - 1) * hop + a.N) * spp) return bad_in(PRE, "y_stride smaller than one signal's samples");
    if (!y) return bad_in(PRE, "NULL y");
    if (nsignals == 1) y_stride = 0;
    const size_t G = nframes / navg, V = nsignals * G;     // V output rows; row v = i G + g
    const int kwhat = csd_kernel_what(what, navg);         // what the run kernels store
    const size_t W = csd_part_row(what, P);                // scalars of one run's partial row
    s = for_device(s);
    if ((rc = ensure_device_any(s, st))) return rc;
    CsdSel e;
    bool fused = false;
    if constexpr (sizeof(T) == 4)
        fused = csd_route_fused(s, hop, x_stride, y_stride, navg, what, ab()) && aligned16(x) && aligned16(y) && (!window || aligned16(window)) &&
                G <= 0xffffffffull && csd_fusable_setup(s, &e, window != nullptr, kwhat);
    // the x and the y frames of whole runs in the two halves of the frame matrix: the cap holds for both together
    const AvgPlan p = avg_plan(V, navg, W * sizeof(T), 2 * row * sizeof(T), fused);
    return averaged_runs<T>(s, st, p, W, 2 * row, out, out_stride, scaling,
        [&](T* dst, size_t dstride, size_t row0, size_t nruns, T scale) {
            if constexpr (sizeof(T) == 4) {
                LoopLaunch ll;   // (the launch rule of the PSD entry)
                if ((rc = loop_launch(s, st, e.fn, e.wg, e.lds, (nruns + e.t_per_wg - 1) / e.t_per_wg, s->route[PFFFT_FORWARD][1].oneshot, &ll))) return rc;
                hipLaunchKernelGGL(e.fn, dim3(ll.grid), dim3(e.wg), e.lds, st, x, x_stride, y, y_stride, (unsigned)G, (unsigned)navg, hop_s, window, dst,
                                   dstride, row0, (unsigned)nruns, scale, s->d_tw.as<cx<float>>(), s->d_twr.as<cx<float>>(), ll.ctr);
                PF_CHECK(hipGetLastError());
            }
            return 0;
        },
        [&](T* X, size_t r, size_t cnt, size_t fa, size_t nfr, T* dst, size_t dstride, T scale) {
            T* Y = X + nfr * row;                          // (dense behind the x rows: ONE transform_batch over both)
            if ((rc = launch_gather<T>(x, x_stride, nframes, hop_s, spp, window, X, fa, nfr, row, st))) return rc;
            if ((rc = launch_gather<T>(y, y_stride, nframes, hop_s, spp, window, Y, fa, nfr, row, st))) return rc;
            if ((rc = transform_batch_any(s, X, X, 2 * nfr, PFFFT_FORWARD, 1, st))) return rc;
            return with_flag(a.real, [&](auto R) {
                return with_what(kwhat, [&](auto K) {
                    return stream_launch(csd_runs_kernel<T, decltype(R)::value, decltype(K)::value>, cnt * P, st, X, Y, (unsigned)row, r, cnt, navg, p.rpg,
                                         dst, dstride, scale);
                });
            });
        },
        [&](T* part, size_t rows, T* out_rows) {
            if (what == CSD_COHERENCE)
                return stream_launch(csd_coherence_reduce_kernel<T>, rows * P, st, part, p.rpg, (unsigned)P, rows, out_rows, out_stride);
            // cross and all-four rows: the sum of the partial rows, scalar by scalar
            return stream_launch(psd_reduce_kernel<T>, rows * W, st, part, p.rpg, (unsigned)W, rows, scaling, out_rows, out_stride);
        });
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
    const pf::Setup* s = pf::route_setup(setup, hop);
    if (!s) return "";
    if (what != pf::CSD_CROSS && what != pf::CSD_ALL && what != pf::CSD_COHERENCE) return "";
    return pf::csd_route_fused(s, hop, x_stride, y_stride, navg, what, pf::ab()) ? "fused" : "composed";
}
