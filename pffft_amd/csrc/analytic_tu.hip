// libpffft_hip.so, translation unit of the analytic signals (include/pffft_hip.h: pffft[d]_hip_analytic_*): z = IDFT(H . DFT(x)) of real
// rows, its imaginary part (the Hilbert transform) and its modulus (the envelope), on the library's own convolution.  The handle owns a
// complex setup of N and the GIVEN filter spectrum H = c_k gain[k]; the fused kernel's launch (one kernel per call) and the composed
// route (widening kernel, convolve_batch, narrowing kernel).  Kernels: fft_analytic.h.
#include <memory>

#include "bluestein_host.h"
#include "fft_analytic.h"

namespace pf {

constexpr uint32_t ANALYTIC_MAGIC = 0x5046414Eu;   // "PFAN"

// The owned inner setup: a complex one of N.  One setup serves ONE device (bind_device_once).
struct AnalyticSetup : InnerOwner<ANALYTIC_MAGIC> {
    static constexpr const char* KIND = "analytic";
    int N = 0;
    bool fusable = false;          // float and N = 512 / 1024 / 2048 / 4096
    std::vector<double> gain;      // N/2 + 1 values (float gains widened: exact); empty: all ones
    DeviceBinding bound;
    DevBuf d_H;                    // H as N complex values (imaginary parts zero) in the inner setup's internal layout
    StreamScratch pad;             // batch x N complex image of the composed real outputs: one per stream, pad.mu held while a call enqueues
};

// ------------------------------------------------------------------------------------------------ plan
static bool analytic_fused_len(int N) { return N == 512 || N == 1024 || N == 2048 || N == 4096; }

// (size, output) cells where the fused kernel is the default: a cell is in it where tests/test_gpu_analytic.py test_default_cells holds
// the fused kernel faster than selector 144 on the device by more than the spread of identical rounds.  A cell that
// loses on a later measurement returns false here and stays reachable through AB_ANALYTIC_FUSED.
static bool analytic_fused_default(int N, int what) {
    (void)N; (void)what;
    return true;
}

static bool analytic_fused_now(const AnalyticSetup* z, int what, const AbSel& sel) {
    return fused_selected(sel, AB_ANALYTIC_COMPOSED, AB_ANALYTIC_FUSED, z->fusable, analytic_fused_default(z->N, what));
}

template <typename G>
static AnalyticSetup* analytic_new_setup(int N, const G* gain, int is_double) {
    if (N < 1) return nullptr;
    std::unique_ptr<AnalyticSetup> z(new AnalyticSetup);
    z->N = N;
    z->fusable = !is_double && analytic_fused_len(N);
    if (!z->new_inner(N, PFFFT_COMPLEX, is_double)) return nullptr;   // (every legal N is even)
    if (gain) z->gain.assign(gain, gain + (size_t)N / 2 + 1);
    return z.release();
}

// ------------------------------------------------------------------------------------------------ the filter spectrum
// H[k] = c_k gain[k], k <= N/2 (c_0 = c_{N/2} = 1, else 2), zero above: the product in double (exact for float gains), rounded once
template <typename T>
static T analytic_h_value(const AnalyticSetup* z, size_t k) {
    const size_t half = (size_t)z->N / 2;
    if (k > half) return (T)0;
    const double c = (k == 0 || k == half) ? 1.0 : 2.0;
    return (T)(c * (z->gain.empty() ? 1.0 : z->gain[k]));
}

// No transform: the spectrum is given.  The permutation into the internal layout is exact (as in bluestein_filter_spectrum).
template <typename T>
static int analytic_build_tables(AnalyticSetup* z) {
    const size_t N = (size_t)z->N;
    std::vector<cx<T>> h(N);
    for (size_t k = 0; k < N; ++k) h[k] = mk<T>(analytic_h_value<T>(z, k), (T)0);
    DevBuf tmp;
    int rc = upload_table(tmp, h);
    if (!rc) rc = z->d_H.grow(N * sizeof(cx<T>));
    if (rc) return rc;
    rc = inner_zreorder_batch<T>(z->inner, tmp.as<T>(), z->d_H.as<T>(), 1, PFFFT_BACKWARD, nullptr);
    const hipError_t e = hipStreamSynchronize(nullptr);   // (the permutation reads tmp: it has finished before the temporary goes)
    if (rc) return rc;
    return e == hipSuccess ? 0 : fail(e, "the filter spectrum of an analytic setup");
}

template <typename T>
static int analytic_ensure(AnalyticSetup* z, hipStream_t st) {
    return bind_device_once(z->bound, "analytic: ", st, [&] { return analytic_build_tables<T>(z); });
}

// ------------------------------------------------------------------------------------------------ the routes
template <int WHAT>
static int analytic_fused(AnalyticSetup* z, const float* in, float* out, size_t batch, hipStream_t st) {
    const size_t N = (size_t)z->N, rout = WHAT == AN_ANALYTIC ? 2 * N : N;
    return bluestein_fused(z->inner, z->N, batch, st, [&](auto tag, size_t b0, size_t nb) {
        typedef typename decltype(tag)::type C;
        const AnalyticIO<C, WHAT> io{in + b0 * N, out + b0 * rout};
        return bluestein_fused_launch<C>(z->inner, io, (const float*)z->d_H.as<float>(), nb, z->N, st);
    });
}

template <typename T>
static int analytic_widen(const T* in, cx<T>* X, size_t total, hipStream_t st) {
    return stream_launch(analytic_widen_kernel<T>, total, st, in, X, total);
}

// ANALYTIC: (x, 0) straight into out, the convolution in place there - no scratch of this handle's
template <typename T>
static int analytic_composed_complex(AnalyticSetup* z, const T* in, T* out, size_t batch, hipStream_t st) {
    const size_t N = (size_t)z->N;
    const T scaling = (T)1 / (T)N;
    if (int rc = analytic_widen<T>(in, reinterpret_cast<cx<T>*>(out), batch * N, st)) return rc;
    return inner_convolve_batch<T>(z->inner, out, z->d_H.as<T>(), out, scaling, batch, st);
}

// HILBERT / ENVELOPE: through the chunked scratch image
template <typename T, int WHAT>
static int analytic_composed_real(AnalyticSetup* z, const T* in, T* out, size_t batch, hipStream_t st) {
    const size_t N = (size_t)z->N;
    return bluestein_composed<T>(
        z->inner, z->pad, (const T*)z->d_H.as<T>(), N, batch, st,
        [&](cx<T>* X, size_t v0, size_t cnt) { return analytic_widen<T>(in + v0 * N, X, cnt * N, st); },
        [&](cx<T>* X, size_t v0, size_t cnt) { return stream_launch(analytic_narrow_kernel<T, WHAT>, cnt * N, st, (const cx<T>*)X, out + v0 * N, cnt * N); });
}

// ------------------------------------------------------------------------------------------------ the entry
template <typename T>
static int analytic_transform_batch(void* setup, const T* in, T* out, size_t batch, int what, hipStream_t st) {
    AnalyticSetup* z = typed_handle<AnalyticSetup, T>(setup);
    if (!z) return (int)hipErrorInvalidHandle;
    if (what != AN_ANALYTIC && what != AN_HILBERT && what != AN_ENVELOPE) return bad("analytic: unknown output");
    if (batch && (!in || !out)) return bad("analytic: NULL in / out");
    const bool cplx = what == AN_ANALYTIC;
    if (((uintptr_t)in & 7) || ((uintptr_t)out & (cplx ? 15 : 7)))
        return bad("analytic: in / out not aligned to 8 bytes (real rows) / 16 bytes (complex rows)");
    if (batch && (cplx || in != out)) {   // the real outputs: the same rows in place, or rows that do not overlap
        const size_t in_bytes = batch * (size_t)z->N * sizeof(T);
        if (ranges_overlap((uintptr_t)in, in_bytes, (uintptr_t)out, in_bytes * (cplx ? 2 : 1))) return bad(cplx ? "analytic: in and out overlap" : "analytic: in and out overlap without being equal");
    }
    int rc = analytic_ensure<T>(z, st);
    if (rc || batch == 0) return rc;
    if constexpr (sizeof(T) == 4) {
        if (analytic_fused_now(z, what, ab()))
            return what == AN_ANALYTIC  ? analytic_fused<AN_ANALYTIC>(z, in, out, batch, st)
                   : what == AN_HILBERT ? analytic_fused<AN_HILBERT>(z, in, out, batch, st)
                                        : analytic_fused<AN_ENVELOPE>(z, in, out, batch, st);
    }
    if (cplx) return analytic_composed_complex<T>(z, in, out, batch, st);
    return what == AN_HILBERT ? analytic_composed_real<T, AN_HILBERT>(z, in, out, batch, st)
                              : analytic_composed_real<T, AN_ENVELOPE>(z, in, out, batch, st);
}

}  // namespace pf

static_assert((int)PFFFT_HIP_ANALYTIC == pf::AN_ANALYTIC && (int)PFFFT_HIP_HILBERT == pf::AN_HILBERT && (int)PFFFT_HIP_ENVELOPE == pf::AN_ENVELOPE,
              "pffft_hip_analytic_what_t is the kernels' WHAT");

PF_EXPORT PFFFT_HIP_AnalyticSetup* pffft_hip_analytic_new_setup(int N, const float* gain) {
    return reinterpret_cast<PFFFT_HIP_AnalyticSetup*>(pf::analytic_new_setup(N, gain, 0));
}
PF_EXPORT PFFFTD_HIP_AnalyticSetup* pffftd_hip_analytic_new_setup(int N, const double* gain) {
    return reinterpret_cast<PFFFTD_HIP_AnalyticSetup*>(pf::analytic_new_setup(N, gain, 1));
}
PF_EXPORT void pffft_hip_analytic_destroy_setup(PFFFT_HIP_AnalyticSetup* s) { pf::destroy_handle<pf::AnalyticSetup>(s); }
PF_EXPORT void pffftd_hip_analytic_destroy_setup(PFFFTD_HIP_AnalyticSetup* s) { pf::destroy_handle<pf::AnalyticSetup>(s); }
PF_EXPORT int pffft_hip_analytic_transform_batch(PFFFT_HIP_AnalyticSetup* s, const float* in, float* out, size_t batch,
                                                 pffft_hip_analytic_what_t what, void* stream) {
    return pf::analytic_transform_batch<float>(s, in, out, batch, (int)what, (hipStream_t)stream);
}
PF_EXPORT int pffftd_hip_analytic_transform_batch(PFFFTD_HIP_AnalyticSetup* s, const double* in, double* out, size_t batch,
                                                  pffft_hip_analytic_what_t what, void* stream) {
    return pf::analytic_transform_batch<double>(s, in, out, batch, (int)what, (hipStream_t)stream);
}
PF_EXPORT const char* pffft_hip_analytic_route(const void* setup, int what) {
    const pf::AnalyticSetup* z = pf::checked_handle<pf::AnalyticSetup>(setup);
    if (!z || what < pf::AN_ANALYTIC || what > pf::AN_ENVELOPE) return "";
    return pf::analytic_fused_now(z, what, pf::ab()) ? "fused" : "composed";
}
PF_EXPORT int pffft_hip_analytic_table(const void* setup, size_t first, size_t count, void* host_out) {
    const pf::AnalyticSetup* z = pf::checked_handle<pf::AnalyticSetup>(setup);
    if (!z || !host_out) {
        pf::g_last_error = "pffft_hip: bad analytic setup handle / NULL output";
        return (int)hipErrorInvalidValue;
    }
    const size_t len = (size_t)z->N;
    if (first > len || count > len - first) {
        pf::g_last_error = "pffft_hip: analytic table range beyond the table";
        return (int)hipErrorInvalidValue;
    }
    for (size_t i = 0; i < count; ++i) {
        if (z->is_double) static_cast<double*>(host_out)[i] = pf::analytic_h_value<double>(z, first + i);
        else static_cast<float*>(host_out)[i] = pf::analytic_h_value<float>(z, first + i);
    }
    return 0;
}
