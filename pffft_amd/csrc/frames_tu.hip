// libpffft_hip.so, translation unit of the windowed overlapping-frame entries (include/pffft_hip.h: pffft_hip_frames_transform_batch,
// pffft_hip_frames_overlap_add_batch, pffft_hip_frames_route): validation, route decision, the fused kernel's instantiations and the
// composed routes through the per-stream frame matrix.  Kernels: fft_frames.h; the frame matrix and its helpers: frames_host.h.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/pffft_hip.h"
#include "frames_host.h"

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

// The configuration the framed kernel runs on must be the one transform_batch runs on for the same (direction, layout) - the results are
// equal bit for bit only then -, so it is read from the setup's stored route: real float forward on TiledPick C512 / C1024 / C2048
// (N = 1024 / 2048 / 4096).  Everything else has no framed kernel.
static const Route& frames_route(const Setup* s, int output) { return s->route[PFFFT_FORWARD][output == FR_INTERNAL ? 0 : 1]; }

static bool frames_fusable_setup(const Setup* s, int output, FramesSel* e, bool windowed) {
    if (s->is_double || s->transform != PFFFT_REAL || s->kernel != K_TILED) return false;
    const Route& r = frames_route(s, output);
    if (r.fam != FAM_TILED) return false;
    const std::string cfg = r.tiled.cfg;
    if (s->n == 512 && cfg == "TiledPick::C512") { if (e) *e = frames_sel<TiledPick<float>::C512>(output, windowed); return true; }
    if (s->n == 1024 && cfg == "TiledPick::C1024") { if (e) *e = frames_sel<TiledPick<float>::C1024>(output, windowed); return true; }
    if (s->n == 2048 && cfg == "TiledPick::C2048") { if (e) *e = frames_sel<TiledPick<float>::C2048>(output, windowed); return true; }
    return false;
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
    int rc = check_setup<T>(s);
    if (rc) return rc;
    if (hop == 0) return bad("frames: hop == 0");
    if (output != FR_INTERNAL && output != FR_ORDERED && output != FR_POWER) return bad("frames: unknown output");
    if (nsignals == 0 || nframes == 0) return 0;
    const bool real = s->transform == PFFFT_REAL;
    const size_t spp = real ? 1 : 2, N = (size_t)s->N, row = s->vec_scalars;
    const size_t out_row = output == FR_POWER ? (real ? N / 2 + 1 : N) : row;
    if (out_stride == 0) out_stride = out_row;
    if (out_stride < out_row) return bad("frames: out_stride smaller than one output row");
    const size_t sig_scalars = ((nframes - 1) * hop + N) * spp;
    if (nsignals > 1 && signal_stride < sig_scalars) return bad("frames: signal_stride smaller than one signal's samples");
    if (!signal || !out) return bad("frames: NULL signal / out");
    const size_t hop_s = hop * spp, batch = nsignals * nframes;
    if (nsignals == 1) signal_stride = 0;   // (one signal: the stride is not read)

    s = for_device(s);
    if ((rc = ensure_device_any(s))) return rc;
    const AbSel sel = ab();
    if constexpr (sizeof(T) == 4) {
        FramesSel e;
        if (frames_route_fused(s, hop, signal_stride, out_stride, output, sel) && aligned16(signal) && (!window || aligned16(window)) &&
            (output == FR_POWER || aligned16(out)) && frames_fusable_setup(s, output, &e, window != nullptr)) {
            // (the kernel counts frames in 32 bits: longer batches of ONE signal go out in slices; several signals that long are composed)
            constexpr size_t SLICE = (size_t)3 << 30;
            const int oneshot = frames_route(s, output).oneshot;
            if (batch <= SLICE)
                return launch_frames_fused(s, e, oneshot, signal, signal_stride, nframes, hop_s, window, out, out_stride, batch, st);
            if (nsignals == 1) {
                for (size_t b0 = 0; b0 < batch; b0 += SLICE) {
                    const size_t nb = std::min(batch - b0, SLICE);
                    if ((rc = launch_frames_fused(s, e, oneshot, signal + b0 * hop_s, 0, nb, hop_s, window, out + b0 * out_stride, out_stride, nb, st))) return rc;
                }
                return 0;
            }
        }
    }

    // composed: frames x window -> frame matrix (chunks of at most FRAMES_CAP_BYTES), transform_batch, then rows -> out where `out` is not
    // the dense spectrum
    const size_t chunk = std::max<size_t>(1, std::min(batch, FRAMES_CAP_BYTES / (row * sizeof(T))));
    const bool direct = output != FR_POWER && out_stride == row;
    std::lock_guard<std::mutex> lk(s->frames.mu);
    void* buf = nullptr;
    if ((rc = frames_buffer(s, st, chunk * row * sizeof(T), &buf))) return rc;
    T* X = (T*)buf;
    constexpr int U = 16 / (int)sizeof(T);
    const bool wide = aligned16(signal) && signal_stride % U == 0 && hop_s % U == 0;
    for (size_t v0 = 0; v0 < batch; v0 += chunk) {
        const size_t cnt = std::min(batch - v0, chunk);
        if (wide)
            hipLaunchKernelGGL((frames_gather_kernel<T, U>), dim3(stream_grid(cnt * row / U)), dim3(256), 0, st, signal, signal_stride, nframes,
                               hop_s, (int)spp, window, X, v0, cnt, (unsigned)row);
        else
            hipLaunchKernelGGL((frames_gather_kernel<T, 1>), dim3(stream_grid(cnt * row)), dim3(256), 0, st, signal, signal_stride, nframes,
                               hop_s, (int)spp, window, X, v0, cnt, (unsigned)row);
        PF_CHECK(hipGetLastError());
        T* dst = out + v0 * out_stride;
        if ((rc = transform_batch_any(s, X, direct ? dst : X, cnt, PFFFT_FORWARD, output == FR_INTERNAL ? 0 : 1, st))) return rc;
        if (direct) continue;
        if (output != FR_POWER) rc = launch_rows<T, 0>(X, row, dst, out_stride, cnt, row, st);
        else if (real) rc = launch_rows<T, 1>(X, row, dst, out_stride, cnt, row, st);
        else rc = launch_rows<T, 2>(X, row, dst, out_stride, cnt, row, st);
        if (rc) return rc;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------ synthesis
template <typename T>
static int launch_ola(const T* y, size_t fbase, size_t fpitch, size_t nframes, size_t hop, size_t N, size_t spp, const T* window, T scaling,
                      T* signal, size_t signal_stride, size_t nsignals, size_t s0, size_t s1, hipStream_t st) {
    hipLaunchKernelGGL((frames_ola_kernel<T>), dim3(stream_grid(nsignals * (s1 - s0) * spp)), dim3(256), 0, st, y, fbase, fpitch, nframes, hop,
                       (unsigned)N, (int)spp, window, scaling, signal, signal_stride, nsignals, s0, s1);
    PF_CHECK(hipGetLastError());
    return 0;
}

template <typename T>
static int frames_overlap_add_batch(Setup* s, const T* spectra, size_t spectra_stride, size_t nsignals, size_t nframes, size_t hop,
                                    const T* window, T scaling, T* signal, size_t signal_stride, int ordered, hipStream_t st) {
    int rc = check_setup<T>(s);
    if (rc) return rc;
    if (hop == 0) return bad("frames: hop == 0");
    if (nsignals == 0 || nframes == 0) return 0;
    const bool real = s->transform == PFFFT_REAL;
    const size_t spp = real ? 1 : 2, N = (size_t)s->N, row = s->vec_scalars;
    if (spectra_stride == 0) spectra_stride = row;
    if (spectra_stride < row) return bad("frames: spectra_stride smaller than one spectrum");
    const size_t samples = (nframes - 1) * hop + N;
    if (nsignals > 1 && signal_stride < samples * spp) return bad("frames: signal_stride smaller than one signal's samples");
    if (!spectra || !signal) return bad("frames: NULL spectra / signal");

    s = for_device(s);
    if ((rc = ensure_device_any(s))) return rc;
    const size_t batch = nsignals * nframes, cap_rows = std::max<size_t>(1, FRAMES_CAP_BYTES / (row * sizeof(T)));
    std::lock_guard<std::mutex> lk(s->frames.mu);
    void* buf = nullptr;
    if (batch <= cap_rows) {   // every frame at once, one gather
        if ((rc = frames_buffer(s, st, batch * row * sizeof(T), &buf))) return rc;
        T* X = (T*)buf;
        if ((rc = frames_backward<T>(s, spectra, spectra_stride, 0, batch, X, ordered, st))) return rc;
        return launch_ola<T>(X, 0, nframes, nframes, hop, N, spp, window, scaling, signal, signal_stride, nsignals, 0, samples, st);
    }
    // beyond the cap: signal by signal, each in runs of frames.  A run owns the samples from its first frame's start to the next run's
    // first frame's start (the last run: to the end) and re-transforms the up to ceil(N / hop) - 1 earlier frames that reach into them.
    const size_t reach = (N + hop - 1) / hop - 1;
    const size_t run = std::max<size_t>(cap_rows > reach ? cap_rows - reach : 1, 1);
    if ((rc = frames_buffer(s, st, std::min(nframes, run + reach) * row * sizeof(T), &buf))) return rc;
    T* X = (T*)buf;
    for (size_t i = 0; i < nsignals; ++i)
        for (size_t fa = 0; fa < nframes; fa += run) {
            const size_t fb = std::min(nframes, fa + run), f0 = fa > reach ? fa - reach : 0;
            if ((rc = frames_backward<T>(s, spectra, spectra_stride, i * nframes + f0, fb - f0, X, ordered, st))) return rc;
            const size_t s0 = fa * hop, s1 = fb == nframes ? samples : fb * hop;
            if ((rc = launch_ola<T>(X, f0, 0, fb, hop, N, spp, window, scaling, signal + i * signal_stride, 0, 1, s0, s1, st))) return rc;
        }
    return 0;
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
    const pf::Setup* s = static_cast<const pf::Setup*>(setup);
    if (!s || s->magic != pf::MAGIC || hop == 0 || output < 0 || output > 2) return "";
    const bool real = s->transform == PFFFT_REAL;
    if (out_stride == 0) out_stride = output == pf::FR_POWER ? (real ? (size_t)s->N / 2 + 1 : (size_t)s->N) : s->vec_scalars;
    return pf::frames_route_fused(s, hop, signal_stride, out_stride, output, pf::ab()) ? "fused" : "composed";
}
