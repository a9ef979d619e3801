// libpffft_hip.so, translation unit of the polyphase filter-bank analysis (include/pffft_hip.h: pffft_hip_pfb_transform_batch,
// pffft_hip_pfb_route): validation, route decision, the fused complex N = 1024 kernel's launch and the composed route through the
// per-stream frame matrix (pf::Setup::frames, shared with the frame entries of frames_tu.hip).  Kernels: fft_pfb.h.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/pffft_hip.h"
#include "pf_host.h"
#include "fft_pfb.h"

struct PFFFT_Setup : pf::Setup {};
struct PFFFTD_Setup : pf::Setup {};

#define PF_EXPORT extern "C" __attribute__((visibility("default")))

static_assert(pf::PFB_FUSED_MAX_TAPS == PFFFT_HIP_PFB_FUSED_MAX_TAPS, "the header's constant is the kernel's");

namespace pf {

// the cap of the frame matrix of one composed launch sequence (include/pffft_hip.h; the value of the frame entries)
constexpr size_t PFB_CAP_BYTES = (size_t)256 << 20;

static int bad(const char* what, hipError_t e = hipErrorInvalidValue) {
    g_last_error = std::string("pffft_hip: ") + what;
    return (int)e;
}

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

// ------------------------------------------------------------------------------------------------ composed pieces
// the frame matrix of `st` (frames.mu held by the caller), grown to `bytes`: outside graph capture only
static int pfb_buffer(Setup* s, hipStream_t st, size_t bytes, void** buf) {
    StreamScratch::Entry& sc = s->frames.acquire(st);
    if (sc.buf[0].bytes() < bytes && stream_capturing(st))
        return bad("the frame matrix of this stream would have to grow during graph capture: run the call once on this stream before capturing",
                   hipErrorStreamCaptureUnsupported);
    if (int rc = s->frames.grow(sc, 0, bytes)) return rc;
    *buf = sc.buf[0].get();
    return 0;
}

template <typename T, int MODE>
static int launch_rows(const T* src, size_t src_stride, T* dst, size_t dst_stride, size_t count, size_t row, hipStream_t st) {
    const size_t per = MODE == 0 ? row : MODE == 1 ? row / 2 + 1 : row / 2;
    const size_t grid = std::max<size_t>(1, std::min<size_t>((count * per + 255) / 256, (size_t)num_cus() * 16));
    hipLaunchKernelGGL((frames_rows_kernel<T, MODE>), dim3((unsigned)grid), dim3(256), 0, st, src, src_stride, dst, dst_stride, count,
                       (unsigned)row);
    PF_CHECK(hipGetLastError());
    return 0;
}

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
    if (!s || s->magic != MAGIC || s->is_double != (sizeof(T) == 8)) {
        g_last_error = "pffft_hip: bad setup handle";
        return (int)hipErrorInvalidHandle;
    }
    if (hop == 0) return bad("pfb: hop == 0");
    if (taps == 0) return bad("pfb: taps == 0");
    if (!prototype) return bad("pfb: NULL prototype");
    if (output != FR_INTERNAL && output != FR_ORDERED && output != FR_POWER) return bad("pfb: unknown output");
    if (nsignals == 0 || nframes == 0) return 0;
    const bool real = s->transform == PFFFT_REAL;
    const size_t spp = real ? 1 : 2, N = (size_t)s->N, row = s->vec_scalars;
    const size_t out_row = output == FR_POWER ? (real ? N / 2 + 1 : N) : row;
    if (out_stride == 0) out_stride = out_row;
    if (out_stride < out_row) return bad("pfb: out_stride smaller than one output row");
    const size_t sig_scalars = ((nframes - 1) * hop + taps * N) * spp;
    if (nsignals > 1 && signal_stride < sig_scalars) return bad("pfb: signal_stride smaller than one signal's samples");
    if (!signal || !out) return bad("pfb: NULL signal / out");
    const size_t hop_s = hop * spp, batch = nsignals * nframes;
    if (nsignals == 1) signal_stride = 0;   // (one signal: the stride is not read)

    s = for_device(s);
    int rc = ensure_device_any(s);
    if (rc) return rc;
    const AbSel sel = ab();
    if constexpr (sizeof(T) == 4) {
        if (pfb_route_fused(s, hop, taps, signal_stride, out_stride, output, sel) && aligned_to(signal, 16) && aligned_to(out, 16) &&
            aligned_to(prototype, 8)) {
            // (the kernel counts frames in 32 bits: longer batches of ONE signal go out in slices; several signals that long are composed)
            constexpr size_t SLICE = (size_t)3 << 30;
            if (batch <= SLICE)
                return launch_pfb_c1024(s, signal, signal_stride, nframes, hop, prototype, taps, out, out_stride, batch, output, st);
            if (nsignals == 1) {
                for (size_t b0 = 0; b0 < batch; b0 += SLICE) {
                    const size_t nb = std::min(batch - b0, SLICE);
                    if ((rc = launch_pfb_c1024(s, signal + b0 * hop_s, 0, nb, hop, prototype, taps, out + b0 * out_stride, out_stride, nb,
                                               output, st)))
                        return rc;
                }
                return 0;
            }
        }
    }

    // composed: folded frames -> frame matrix (chunks of at most PFB_CAP_BYTES), transform_batch, then rows -> out where `out` is not the
    // dense spectrum
    const size_t chunk = std::max<size_t>(1, std::min(batch, PFB_CAP_BYTES / (row * sizeof(T))));
    const bool direct = output != FR_POWER && out_stride == row;
    std::lock_guard<std::mutex> lk(s->frames.mu);
    void* buf = nullptr;
    if ((rc = pfb_buffer(s, st, chunk * row * sizeof(T), &buf))) return rc;
    T* X = (T*)buf;
    constexpr int U = 16 / (int)sizeof(T);
    const bool wide = aligned_to(signal, 16) && signal_stride % U == 0 && hop_s % U == 0 && row % U == 0;
    for (size_t v0 = 0; v0 < batch; v0 += chunk) {
        const size_t cnt = std::min(batch - v0, chunk);
        rc = wide ? launch_fold<T, U>(signal, signal_stride, nframes, hop_s, (int)spp, prototype, taps, X, v0, cnt, row, st)
                  : launch_fold<T, 1>(signal, signal_stride, nframes, hop_s, (int)spp, prototype, taps, X, v0, cnt, row, st);
        if (rc) return rc;
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
    const pf::Setup* s = static_cast<const pf::Setup*>(setup);
    if (!s || s->magic != pf::MAGIC || hop == 0 || taps == 0 || output < 0 || output > 2) return "";
    const bool real = s->transform == PFFFT_REAL;
    if (out_stride == 0) out_stride = output == pf::FR_POWER ? (real ? (size_t)s->N / 2 + 1 : (size_t)s->N) : s->vec_scalars;
    return pf::pfb_route_fused(s, hop, taps, signal_stride, out_stride, output, pf::ab()) ? "fused" : "composed";
}
