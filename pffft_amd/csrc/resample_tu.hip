// libpffft_hip.so, translation unit of the Fourier resampling of rows (include/pffft_hip.h: pffft[d]_hip_resample_*): N samples in, M
// samples out over the same span, out = s IDFT_M(crop / zero-fill(DFT_N x)).  The handle owns a complex setup of N and one of M (one where
// N == M) and no tables; the fused kernel's launch (one kernel per call) and the composed route (widening kernel, transform_batch at N,
// map kernel, transform_batch at M, narrowing kernel - in the ORDERED layout).  Kernels: fft_resample.h.
#include <memory>

#include "bluestein_host.h"
#include "fft_resample.h"

namespace pf {

constexpr uint32_t RESAMPLE_MAGIC = 0x50465253u;   // "PFRS"

// The owned inner setups: complex ones of N and of M.  One setup serves ONE device (bind_device_once).
struct ResampleSetup : InnerOwner<RESAMPLE_MAGIC> {
    static constexpr const char* KIND = "resample";
    int N = 0, M = 0, real = 0;
    Setup* inner_m = nullptr;      // the setup of M (== inner where N == M)
    bool fusable = false;          // float, N != M, both from 512 / 1024 / 2048 / 4096
    DeviceBinding bound;
    StreamScratch pad;             // the composed route's spectra: one buffer per stream, pad.mu held while a call enqueues
};

// ------------------------------------------------------------------------------------------------ plan
static bool resample_fused_len(int n) { return n == 512 || n == 1024 || n == 2048 || n == 4096; }

// Where the next group's first loads are requested - arithmetic on the resource remarks of every instantiation (tools/resample_resources.py;
// the table of DESIGN.md §3.32), not a measurement: behind the first barrier (PF 1) where that keeps the waves per SIMD of PF 0.  No form
// has scratch.  Up: the early request costs the fourth wave (the second workgroup of a CU) in every cell - PF 0.  Down: 3 waves either
// way - PF 1.
constexpr int resample_pf(bool up) { return up ? 0 : 1; }

// (N, M, kind) cells where the fused kernel is the default: a cell is in it where tests/test_gpu_resample.py test_default_cells holds the
// fused kernel faster than selector 156 on the device by more than the spread of identical rounds.  A cell that loses
// returns false here and stays reachable through AB_RESAMPLE_FUSED.
static bool resample_fused_default(int N, int M, int real) {
    (void)N; (void)M; (void)real;
    return true;
}

static bool resample_fused_now(const ResampleSetup* z, const AbSel& sel) {
    return fused_selected(sel, AB_RESAMPLE_COMPOSED, AB_RESAMPLE_FUSED, z->fusable, resample_fused_default(z->N, z->M, z->real));
}

static ResampleSetup* resample_new_setup(int N, int M, int real_rows, int is_double) {
    if (N < 1 || M < 1) return nullptr;
    std::unique_ptr<ResampleSetup> z(new ResampleSetup);
    z->N = N; z->M = M; z->real = real_rows ? 1 : 0;
    z->fusable = !is_double && N != M && resample_fused_len(N) && resample_fused_len(M);
    if (!z->new_inner(N, PFFFT_COMPLEX, is_double)) return nullptr;
    z->inner_m = N == M ? z->inner : z->add_inner(M, PFFFT_COMPLEX);
    if (!z->inner_m) return nullptr;
    return z.release();
}

// ------------------------------------------------------------------------------------------------ the routes
template <class F>
static int resample_with_cfg(int n, F&& f) {
    typedef ConvPick<float> P;
    switch (n) {
        case 512: return f(CfgTag<P::C512>());
        case 1024: return f(CfgTag<P::C1024>());
        case 2048: return f(CfgTag<P::C2048>());
        case 4096: return f(CfgTag<P::C4096>());
        default: return bad("no fused kernel for this resampling length");
    }
}

template <class CS, class CB, int UP, int REAL>
static int resample_fused_launch(ResampleSetup* z, const float* in, float* out, size_t batch, float s, hipStream_t st) {
    auto k = fft_resample_kernel<CS, CB, UP, REAL, resample_pf(UP != 0)>;
    Setup* small = UP ? z->inner : z->inner_m;
    Setup* big = UP ? z->inner_m : z->inner;
    constexpr size_t G = 512 / CS::TPT;   // rows of one group
    return loop_launch_last(z->inner, st, k, 512, CB::LDS_BYTES, (batch + G - 1) / G, CONV_ONESHOT, in, out, (unsigned)batch, s,
                            small->d_tw.as<cx<float>>(), big->d_tw.as<cx<float>>());
}

template <int REAL>
static int resample_fused(ResampleSetup* z, const float* in, float* out, size_t batch, float s, hipStream_t st) {
    const size_t spp = REAL ? 1 : 2;
    if (int rc = inner_on_device(z->inner, st)) return rc;
    if (int rc = inner_on_device(z->inner_m, st)) return rc;
    return for_slices(batch, [&](size_t b0, size_t nb) {
        const float* src = in + b0 * (size_t)z->N * spp;
        float* dst = out + b0 * (size_t)z->M * spp;
        return resample_with_cfg(z->N, [&](auto tn) {
            return resample_with_cfg(z->M, [&](auto tm) {
                typedef typename decltype(tn)::type CN;
                typedef typename decltype(tm)::type CM;
                if constexpr (CN::n < CM::n) return resample_fused_launch<CN, CM, 1, REAL>(z, src, dst, nb, s, st);
                else if constexpr (CN::n > CM::n) return resample_fused_launch<CM, CN, 0, REAL>(z, src, dst, nb, s, st);
                else return bad("no fused kernel for N == M");
            });
        });
    });
}

// N + M complex values of scratch per row: the spectrum of N, then the spectrum of M; the cap holds for both together
template <typename T, int REAL>
static int resample_composed(ResampleSetup* z, const T* in, T* out, size_t batch, T s, hipStream_t st) {
    const size_t N = (size_t)z->N, M = (size_t)z->M;
    return chunked_scratch<cx<T>>(z->pad, st, batch, (N + M) * sizeof(cx<T>), "the scratch image", [&](cx<T>* X, size_t v0, size_t cnt) {
        cx<T>* Y = X + cnt * N;
        const T* src = in + v0 * N * 2;
        if constexpr (REAL) {
            if (int rc = stream_launch(resample_widen_kernel<T>, cnt * N, st, in + v0 * N, X, cnt * N)) return rc;
            src = (const T*)X;
        }
        if (int rc = inner_transform_batch<T>(z->inner, src, (T*)X, cnt, PFFFT_FORWARD, 1, st)) return rc;
        if (int rc = stream_launch(resample_map_kernel<T>, cnt * M, st, (const cx<T>*)X, Y, cnt, N, M, s)) return rc;
        T* dst = REAL ? (T*)Y : out + v0 * M * 2;   // the complex kind: straight into out
        if (int rc = inner_transform_batch<T>(z->inner_m, (const T*)Y, dst, cnt, PFFFT_BACKWARD, 1, st)) return rc;
        if constexpr (REAL) return stream_launch(resample_narrow_kernel<T>, cnt * M, st, (const cx<T>*)Y, out + v0 * M, cnt * M);
        else return 0;
    });
}

// ------------------------------------------------------------------------------------------------ the entry
template <typename T>
static int resample_batch(void* setup, const T* in, T* out, size_t batch, T scaling, hipStream_t st) {
    ResampleSetup* z = typed_handle<ResampleSetup, T>(setup);
    if (!z) return (int)hipErrorInvalidHandle;
    if (batch && (!in || !out)) return bad("resample: NULL in / out");
    const size_t el = (z->real ? 1 : 2) * sizeof(T);
    if (((uintptr_t)in | (uintptr_t)out) & (el - 1)) return bad("resample: in / out not aligned to one element");
    if (batch && ranges_overlap((uintptr_t)in, batch * (size_t)z->N * el, (uintptr_t)out, batch * (size_t)z->M * el))
        return bad("resample: out overlaps in (there is no in-place form)");
    int rc = bind_device_once(z->bound, "resample: ", st, [] { return 0; });   // (no tables: nothing is built beyond the binding)
    if (rc || batch == 0) return rc;
    const T s = (T)((double)scaling / (double)z->N);
    if constexpr (sizeof(T) == 4) {
        if (resample_fused_now(z, ab()))
            return with_flag(z->real != 0, [&](auto R) { return resample_fused<decltype(R)::value>(z, in, out, batch, s, st); });
    }
    return with_flag(z->real != 0, [&](auto R) { return resample_composed<T, decltype(R)::value>(z, in, out, batch, s, st); });
}

}  // namespace pf

PF_EXPORT PFFFT_HIP_ResampleSetup* pffft_hip_resample_new_setup(int N, int M, int real_rows) {
    return reinterpret_cast<PFFFT_HIP_ResampleSetup*>(pf::resample_new_setup(N, M, real_rows, 0));
}
PF_EXPORT PFFFTD_HIP_ResampleSetup* pffftd_hip_resample_new_setup(int N, int M, int real_rows) {
    return reinterpret_cast<PFFFTD_HIP_ResampleSetup*>(pf::resample_new_setup(N, M, real_rows, 1));
}
PF_EXPORT void pffft_hip_resample_destroy_setup(PFFFT_HIP_ResampleSetup* s) { pf::destroy_handle<pf::ResampleSetup>(s); }
PF_EXPORT void pffftd_hip_resample_destroy_setup(PFFFTD_HIP_ResampleSetup* s) { pf::destroy_handle<pf::ResampleSetup>(s); }
PF_EXPORT int pffft_hip_resample_batch(PFFFT_HIP_ResampleSetup* s, const float* in, float* out, size_t batch, float scaling, void* stream) {
    return pf::resample_batch<float>(s, in, out, batch, scaling, (hipStream_t)stream);
}
PF_EXPORT int pffftd_hip_resample_batch(PFFFTD_HIP_ResampleSetup* s, const double* in, double* out, size_t batch, double scaling, void* stream) {
    return pf::resample_batch<double>(s, in, out, batch, scaling, (hipStream_t)stream);
}
PF_EXPORT const char* pffft_hip_resample_route(const void* setup) {
    const pf::ResampleSetup* z = pf::checked_handle<pf::ResampleSetup>(setup);
    if (!z) return "";
    return pf::resample_fused_now(z, pf::ab()) ? "fused" : "composed";
}
