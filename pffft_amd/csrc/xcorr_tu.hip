// libpffft_hip.so, translation unit of the correlations (include/pffft_hip.h: pffft[d]_hip_xcorr_*): r = IDFT(W(conj(DFT x) DFT y)) of two
// row sets that both change per call, plain or PHAT-weighted, a window of lags stored.  The handle owns a complex setup of N and no tables;
// the fused kernel's launch (one kernel per call) and the composed route (pad kernel, transform_batch over both halves of the scratch
// image, product kernel, transform_batch back, crop kernel - in the ORDERED layout).  Kernels: fft_xcorr.h.
#include <memory>

#include "bluestein_host.h"
#include "fft_xcorr.h"

namespace pf {

constexpr uint32_t XCORR_MAGIC = 0x50465843u;   // "PFXC"

// The owned inner setup: a complex one of N.  One setup serves ONE device (bind_device_once).
struct XcorrSetup : InnerOwner<XCORR_MAGIC> {
    static constexpr const char* KIND = "xcorr";
    int N = 0, real = 0, len_x = 0, len_y = 0, lag0 = 0, nlags = 0;
    unsigned m0 = 0;               // lag0 mod N
    bool fusable = false;          // float and N = 512 / 1024 / 2048 / 4096
    DeviceBinding bound;
    StreamScratch pad;             // the composed route's image: one per stream, pad.mu held while a call enqueues
};

// ------------------------------------------------------------------------------------------------ plan
static bool xcorr_fused_len(int N) { return N == 512 || N == 1024 || N == 2048 || N == 4096; }

// Which request point of the next x row a cross cell takes - arithmetic on the resource remarks of every instantiation
// (tools/xcorr_resources.py; the table of DESIGN.md §3.25), not a measurement: XPF 1 where it keeps the waves per SIMD of XPF 0.  No form
// has scratch.  Cross: N = 512 / 1024 lose a wave with the early request (2 against 3), N = 2048 / 4096 hold 2 either way.  Auto: the early
// request costs a wave everywhere but on real rows of N = 2048 / 4096 (3 either way).
template <class C> constexpr int xcorr_xpf(bool real, bool is_auto) { return C::n >= 2048 && (!is_auto || real) ? 1 : 0; }

// (N, kind, weight, auto) cells where the fused kernel is the default: a cell is in it where tests/test_gpu_xcorr.py test_default_cells
// holds the fused kernel faster than selector 146 on the device by more than the spread of identical rounds.  A cell
// that loses returns false here and stays reachable through AB_XCORR_FUSED.
static bool xcorr_fused_default(int N, int real, int weight, int is_auto) {
    (void)N; (void)real; (void)weight; (void)is_auto;
    return true;
}

static bool xcorr_fused_now(const XcorrSetup* z, int weight, int is_auto, const AbSel& sel) {
    return fused_selected(sel, AB_XCORR_COMPOSED, AB_XCORR_FUSED, z->fusable, xcorr_fused_default(z->N, z->real, weight, is_auto));
}

static XcorrSetup* xcorr_new_setup(int N, int real_rows, int len_x, int len_y, int lag0, int nlags, int is_double) {
    if (N < 1 || len_x < 1 || len_x > N || len_y < 1 || len_y > N || lag0 <= -N || lag0 >= N || nlags < 1 || nlags > N) return nullptr;
    std::unique_ptr<XcorrSetup> z(new XcorrSetup);
    z->N = N; z->real = real_rows ? 1 : 0; z->len_x = len_x; z->len_y = len_y; z->lag0 = lag0; z->nlags = nlags;
    z->m0 = (unsigned)(lag0 < 0 ? lag0 + N : lag0);
    z->fusable = !is_double && xcorr_fused_len(N);
    if (!z->new_inner(N, PFFFT_COMPLEX, is_double)) return nullptr;
    return z.release();
}

// ------------------------------------------------------------------------------------------------ the routes
template <class C, int REAL, int AUTO>
static int xcorr_fused_launch(Setup* s, const XcorrIO<C, REAL>& io, size_t batch, int weight, hipStream_t st) {
    auto k = fft_xcorr_kernel<C, XcorrIO<C, REAL>, AUTO, xcorr_xpf<C>(REAL != 0, AUTO != 0)>;
    const cx<float>* tw = s->d_tw.as<cx<float>>();
    return loop_launch_last(s, st, k, C::WG_THREADS, C::LDS_BYTES, (batch + C::T_PER_WG - 1) / C::T_PER_WG, CONV_ONESHOT, io, (unsigned)batch, weight, tw, tw);
}

template <int REAL, int AUTO>
static int xcorr_fused(XcorrSetup* z, const float* x, const float* y, float* out, size_t batch, int weight, float s, hipStream_t st) {
    const size_t spp = REAL ? 1 : 2;
    return bluestein_fused(z->inner, z->N, batch, st, [&](auto tag, size_t b0, size_t nb) {
        typedef typename decltype(tag)::type C;
        const XcorrIO<C, REAL> io{x + b0 * (size_t)z->len_x * spp, y + b0 * (size_t)z->len_y * spp, out + b0 * (size_t)z->nlags * spp,
                                  (unsigned)z->len_x, (unsigned)z->len_y, z->m0, (unsigned)z->nlags, s};
        return xcorr_fused_launch<C, REAL, AUTO>(z->inner, io, nb, weight, st);
    });
}

// Two N-point complex rows of the image per row pair (one for the autocorrelation), the cap holds for both together
template <typename T, int REAL>
static int xcorr_composed(XcorrSetup* z, const T* x, const T* y, T* out, size_t batch, int weight, bool is_auto, T s, hipStream_t st) {
    const size_t N = (size_t)z->N, spp = REAL ? 1 : 2, lx = (size_t)z->len_x, ly = (size_t)z->len_y, nl = (size_t)z->nlags;
    const int sets = is_auto ? 1 : 2;
    return chunked_scratch<cx<T>>(z->pad, st, batch, (size_t)sets * N * sizeof(cx<T>), "the scratch image", [&](cx<T>* X, size_t v0, size_t cnt) {
        cx<T>* Y = is_auto ? X : X + cnt * N;   // (dense behind the x rows: ONE forward transform_batch over both)
        if (int rc = stream_launch(xcorr_pad_kernel<T, REAL>, cnt * N * sets, st, x + v0 * lx * spp, y + v0 * ly * spp, X, cnt, N, lx, ly, sets)) return rc;
        if (int rc = inner_transform_batch<T>(z->inner, (const T*)X, (T*)X, cnt * sets, PFFFT_FORWARD, 1, st)) return rc;
        if (int rc = stream_launch(xcorr_product_kernel<T>, cnt * N, st, (const cx<T>*)X, Y, cnt * N, weight)) return rc;
        if (int rc = inner_transform_batch<T>(z->inner, (const T*)Y, (T*)Y, cnt, PFFFT_BACKWARD, 1, st)) return rc;
        return stream_launch(xcorr_crop_kernel<T, REAL>, cnt * nl, st, (const cx<T>*)Y, out + v0 * nl * spp, cnt, N, (size_t)z->m0, nl, s);
    });
}

// ------------------------------------------------------------------------------------------------ the entry
template <typename T>
static int xcorr_batch(void* setup, const T* x, const T* y, T* out, size_t batch, int weight, T scaling, hipStream_t st) {
    XcorrSetup* z = typed_handle<XcorrSetup, T>(setup);
    if (!z) return (int)hipErrorInvalidHandle;
    if (weight != XC_PLAIN && weight != XC_PHAT) return bad("xcorr: unknown weight");
    if (batch && (!x || !y || !out)) return bad("xcorr: NULL x / y / out");
    const bool is_auto = x == y;
    if (batch && is_auto && z->len_x != z->len_y) return bad("xcorr: y == x (the autocorrelation) needs a setup with len_x == len_y");
    const size_t el = (z->real ? 1 : 2) * sizeof(T);
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)out) & (el - 1)) return bad("xcorr: x / y / out not aligned to one element");
    if (batch) {
        const uintptr_t o0 = (uintptr_t)out;
        const size_t olen = batch * (size_t)z->nlags * el;
        if (ranges_overlap((uintptr_t)x, batch * (size_t)z->len_x * el, o0, olen) || ranges_overlap((uintptr_t)y, batch * (size_t)z->len_y * el, o0, olen))
            return bad("xcorr: out overlaps x or y");
    }
    int rc = bind_device_once(z->bound, "xcorr: ", st, [] { return 0; });   // (no tables: nothing is built beyond the binding)
    if (rc || batch == 0) return rc;
    const T s = (T)((double)scaling / (double)z->N);
    if constexpr (sizeof(T) == 4) {
        if (xcorr_fused_now(z, weight, is_auto, ab()))
            return with_flag(z->real != 0, [&](auto R) {
                return with_flag(is_auto, [&](auto A) { return xcorr_fused<decltype(R)::value, decltype(A)::value>(z, x, y, out, batch, weight, s, st); });
            });
    }
    return with_flag(z->real != 0, [&](auto R) { return xcorr_composed<T, decltype(R)::value>(z, x, y, out, batch, weight, is_auto, s, st); });
}

}  // namespace pf

static_assert((int)PFFFT_HIP_XCORR_PLAIN == pf::XC_PLAIN && (int)PFFFT_HIP_XCORR_PHAT == pf::XC_PHAT, "pffft_hip_xcorr_weight_t is the kernels' weight");

PF_EXPORT PFFFT_HIP_XcorrSetup* pffft_hip_xcorr_new_setup(int N, int real_rows, int len_x, int len_y, int lag0, int nlags) {
    return reinterpret_cast<PFFFT_HIP_XcorrSetup*>(pf::xcorr_new_setup(N, real_rows, len_x, len_y, lag0, nlags, 0));
}
PF_EXPORT PFFFTD_HIP_XcorrSetup* pffftd_hip_xcorr_new_setup(int N, int real_rows, int len_x, int len_y, int lag0, int nlags) {
    return reinterpret_cast<PFFFTD_HIP_XcorrSetup*>(pf::xcorr_new_setup(N, real_rows, len_x, len_y, lag0, nlags, 1));
}
PF_EXPORT void pffft_hip_xcorr_destroy_setup(PFFFT_HIP_XcorrSetup* s) { pf::destroy_handle<pf::XcorrSetup>(s); }
PF_EXPORT void pffftd_hip_xcorr_destroy_setup(PFFFTD_HIP_XcorrSetup* s) { pf::destroy_handle<pf::XcorrSetup>(s); }
PF_EXPORT int pffft_hip_xcorr_batch(PFFFT_HIP_XcorrSetup* s, const float* x, const float* y, float* out, size_t batch, pffft_hip_xcorr_weight_t w,
                                    float scaling, void* stream) {
    return pf::xcorr_batch<float>(s, x, y, out, batch, (int)w, scaling, (hipStream_t)stream);
}
PF_EXPORT int pffftd_hip_xcorr_batch(PFFFTD_HIP_XcorrSetup* s, const double* x, const double* y, double* out, size_t batch,
                                     pffft_hip_xcorr_weight_t w, double scaling, void* stream) {
    return pf::xcorr_batch<double>(s, x, y, out, batch, (int)w, scaling, (hipStream_t)stream);
}
PF_EXPORT const char* pffft_hip_xcorr_route(const void* setup, int weight, int is_auto) {
    const pf::XcorrSetup* z = pf::checked_handle<pf::XcorrSetup>(setup);
    if (!z || (weight != pf::XC_PLAIN && weight != pf::XC_PHAT)) return "";
    return pf::xcorr_fused_now(z, weight, is_auto ? 1 : 0, pf::ab()) ? "fused" : "composed";
}
