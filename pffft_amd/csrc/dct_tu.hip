// libpffft_hip.so, translation unit of the cosine / sine transforms (include/pffft_hip.h: pffft[d]_hip_dct_*): types II and III by
// Makhoul's algorithm on ONE real transform of the same length.  The handle owns an ordinary real setup of N and the folded table t_k;
// the fused kernel's instantiations and launch, and the composed route through a per-stream scratch image.  Kernels: fft_dct.h.
#include <cmath>
#include <memory>

#include "pf_compose.h"
#include "dct_host.h"
#include "fft_dct.h"

namespace pf {

constexpr uint32_t DCT_MAGIC = 0x50464443u;   // "PFDC"

struct DctSetup : InnerOwner<DCT_MAGIC> {   // the owned inner setup: a real one of N
    static constexpr const char* KIND = "dct";
    int N = 0, kind = 0, norm = 0;
    std::mutex mu;                 // guards the lazy tables
    // t_k, k = 0 ... N/2, per object that holds the inner setup's device state (for_device): one table per device the setup is used on
    std::map<const Setup*, DevBuf> d_tab;
    StreamScratch scratch;         // batch x N image of the composed route: one per stream, scratch.mu held while a call enqueues
};

// ------------------------------------------------------------------------------------------------ the folded table
// t_k = 2 s_k w_k (type II) / s'_k conj(w_k) (type III), w_k = exp(-j pi k / 2N) = W_{4N}^k; norm none: s = s' = 1; ortho:
// s_0 = 1/sqrt(4N), s'_0 = 1/sqrt(N), s_k = s'_k = 1/sqrt(2N).  The sine forms run the cosine form on a reversed index, so their end
// factors sit at the same k of the table.  Scale and root are multiplied in long double and rounded once (pf_devmem.h).
template <typename T>
static cx<T> dct_table_value(const DctSetup* z, size_t k) {
    const bool t3 = dct_type3(z->kind);
    long double s = 1.0L;
    if (z->norm == PFFFT_HIP_DCT_NORM_ORTHO)
        s = 1.0L / sqrtl(k == 0 ? (t3 ? (long double)z->N : 4.0L * (long double)z->N) : 2.0L * (long double)z->N);
    return scaled_unit_root<T>((long long)k, 4ll * z->N, t3 ? s : 2.0L * s, t3);
}

template <typename T>
static int dct_table(DctSetup* z, const Setup* s, hipStream_t st, const cx<T>** tab) {
    std::lock_guard<std::mutex> lk(z->mu);
    auto it = z->d_tab.find(s);
    if (it == z->d_tab.end()) {
        if (stream_capturing(st))
            return bad("dct: the table of this setup would have to be built during graph capture: run the call once before capturing",
                       hipErrorStreamCaptureUnsupported);
        std::vector<cx<T>> h((size_t)z->N / 2 + 1);
        for (size_t k = 0; k < h.size(); ++k) h[k] = dct_table_value<T>(z, k);
        DevBuf d;
        if (int rc = upload_table(d, h)) return rc;
        it = z->d_tab.emplace(s, std::move(d)).first;
    }
    *tab = it->second.as<cx<T>>();
    return 0;
}

// ------------------------------------------------------------------------------------------------ plan
typedef void (*DctFn)(const float*, float*, unsigned, const cx<float>*, const cx<float>*, const cx<float>*, unsigned*);
typedef KernelSel<DctFn> DctSel;

template <class C>
static DctSel dct_sel(int kind) {
    DctSel e;
    e.wg = C::WG_THREADS; e.t_per_wg = C::T_PER_WG; e.lds = dct_lds_bytes<C>();
    e.fn = kind == DCT_2 ? fft_dct_kernel<C, DCT_2> : kind == DCT_3 ? fft_dct_kernel<C, DCT_3>
           : kind == DST_2 ? fft_dct_kernel<C, DST_2> : fft_dct_kernel<C, DST_3>;
    return e;
}

// The fused kernel runs on the configuration of the inner setup's route in the canonical layout (visit_tiled_cfg), forward for type II,
// backward for type III.  Everything else has no fused kernel.
static const Route& dct_route(const Setup* s, int kind) { return s->route[dct_type3(kind) ? PFFFT_BACKWARD : PFFFT_FORWARD][1]; }

static bool dct_fusable(const DctSetup* z, DctSel* e) {
    return visit_tiled_cfg(z->inner, dct_route(z->inner, z->kind), [&](auto tag) {
        if (e) *e = dct_sel<typename decltype(tag)::type>(z->kind);
    });
}

// (size, kind) cells where the fused kernel is the default: a cell is in it where tools/dct_bench.py holds the fused kernel faster than
// selector 138 on the device by more than the spread of identical runs - all twelve (0.30-0.38 of the composed time against a spread
// below 2.2 %).  A cell that loses on a later measurement returns false here and stays reachable through AB_DCT_FUSED.
static bool dct_fused_default(int N, int kind) {
    (void)N; (void)kind;
    return true;
}

static bool dct_fused_now(const DctSetup* z, const AbSel& sel) {
    return fused_selected(sel, AB_DCT_COMPOSED, AB_DCT_FUSED, dct_fusable(z, nullptr), dct_fused_default(z->N, z->kind));
}

static DctSetup* dct_new_setup(int N, int kind, int norm, int is_double) {
    if (N < 1 || kind < PFFFT_HIP_DCT2 || kind > PFFFT_HIP_DST3 || (norm != PFFFT_HIP_DCT_NORM_NONE && norm != PFFFT_HIP_DCT_NORM_ORTHO))
        return nullptr;
    std::unique_ptr<DctSetup> z(new DctSetup);
    z->N = N; z->kind = kind; z->norm = norm;
    return z->new_inner(N, PFFFT_REAL, is_double) ? z.release() : nullptr;
}

// ------------------------------------------------------------------------------------------------ the two routes
// (oneshot: the launch rule of the transform kernel - of the stored route that dct_fusable read `e` from, frames_tu.hip)
static int dct_fused(Setup* s, const DctSel& e, int oneshot, const float* in, float* out, size_t batch, const cx<float>* tab, hipStream_t st) {
    size_t resident = 0;
    if (int rc = loop_resident(e.fn, e.wg, e.lds, &resident)) return rc;
    const size_t N = (size_t)s->N;
    return for_slices(batch, [&](size_t b0, size_t nb) {
        const LoopLaunch ll = loop_take(s, st, resident, (nb + e.t_per_wg - 1) / e.t_per_wg, oneshot);
        hipLaunchKernelGGL(e.fn, dim3(ll.grid), dim3(e.wg), e.lds, st, in + b0 * N, out + b0 * N, (unsigned)nb, tab,
                           s->d_tw.as<cx<float>>(), s->d_twr.as<cx<float>>(), ll.ctr);
        PF_CHECK(hipGetLastError());
        return 0;
    });
}

template <typename T, int KIND>
static int dct_composed_kind(DctSetup* z, Setup* s, const T* in, T* out, size_t batch, const cx<T>* tab, hipStream_t st) {
    constexpr bool III = dct_type3(KIND);
    const size_t N = (size_t)z->N;
    return chunked_scratch<T>(z->scratch, st, batch, N * sizeof(T), "dct: the scratch image", [&](T* X, size_t v0, size_t cnt) {
        if (int rc = stream_launch(dct_pre_kernel<T, KIND>, cnt * (III ? N / 8 : N / 4), st, in + v0 * N, X, tab, cnt, (unsigned)N)) return rc;
        if (int rc = transform_batch_any(s, X, X, cnt, III ? PFFFT_BACKWARD : PFFFT_FORWARD, 1, st)) return rc;
        return stream_launch(dct_post_kernel<T, KIND>, cnt * (III ? N / 4 : N / 8), st, (const T*)X, out + v0 * N, tab, cnt, (unsigned)N);
    });
}

template <typename T>
static int dct_composed(DctSetup* z, Setup* s, const T* in, T* out, size_t batch, const cx<T>* tab, hipStream_t st) {
    switch (z->kind) {
        case DCT_2: return dct_composed_kind<T, DCT_2>(z, s, in, out, batch, tab, st);
        case DCT_3: return dct_composed_kind<T, DCT_3>(z, s, in, out, batch, tab, st);
        case DST_2: return dct_composed_kind<T, DST_2>(z, s, in, out, batch, tab, st);
        default: return dct_composed_kind<T, DST_3>(z, s, in, out, batch, tab, st);
    }
}

// ------------------------------------------------------------------------------------------------ the entry
template <typename T>
static int dct_transform_batch(void* setup, const T* in, T* out, size_t batch, hipStream_t st) {
    DctSetup* z = typed_handle<DctSetup, T>(setup);
    if (!z) return (int)hipErrorInvalidHandle;
    if (batch == 0) return 0;
    if (!in || !out) return bad("dct: NULL in / out");
    if (((uintptr_t)in | (uintptr_t)out) & 15) return bad("dct: in / out not aligned to 16 bytes");
    const size_t len = batch * (size_t)z->N * sizeof(T);   // the same rows in place, or rows that do not overlap
    if (in != out && ranges_overlap((uintptr_t)in, len, (uintptr_t)out, len)) return bad("dct: in and out overlap without being equal");
    Setup* s = for_device(z->inner);   // the object that holds the inner setup's tables on the calling thread's device
    int rc = ensure_device_any(s, st);
    if (rc) return rc;
    const cx<T>* tab = nullptr;
    if ((rc = dct_table<T>(z, s, st, &tab))) return rc;
    if constexpr (sizeof(T) == 4) {
        DctSel e;
        if (dct_fused_now(z, ab()) && dct_fusable(z, &e)) return dct_fused(s, e, dct_route(z->inner, z->kind).oneshot, in, out, batch, tab, st);
    }
    return dct_composed<T>(z, s, in, out, batch, tab, st);
}

// (dct_host.h) for the fused 2-D kernel of dct2d_tu.hip
int dct_device_table(void* setup, hipStream_t st, const cx<float>** tab) {
    DctSetup* z = typed_handle<DctSetup, float>(setup);
    if (!z) return (int)hipErrorInvalidHandle;
    Setup* s = for_device(z->inner);
    if (int rc = ensure_device_any(s, st)) return rc;
    return dct_table<float>(z, s, st, tab);
}

}  // namespace pf

PF_EXPORT PFFFT_HIP_DctSetup* pffft_hip_dct_new_setup(int N, pffft_hip_dct_kind_t kind, pffft_hip_dct_norm_t norm) {
    return reinterpret_cast<PFFFT_HIP_DctSetup*>(pf::dct_new_setup(N, (int)kind, (int)norm, 0));
}
PF_EXPORT PFFFTD_HIP_DctSetup* pffftd_hip_dct_new_setup(int N, pffft_hip_dct_kind_t kind, pffft_hip_dct_norm_t norm) {
    return reinterpret_cast<PFFFTD_HIP_DctSetup*>(pf::dct_new_setup(N, (int)kind, (int)norm, 1));
}
PF_EXPORT void pffft_hip_dct_destroy_setup(PFFFT_HIP_DctSetup* s) { pf::destroy_handle<pf::DctSetup>(s); }
PF_EXPORT void pffftd_hip_dct_destroy_setup(PFFFTD_HIP_DctSetup* s) { pf::destroy_handle<pf::DctSetup>(s); }
PF_EXPORT int pffft_hip_dct_transform_batch(PFFFT_HIP_DctSetup* s, const float* in, float* out, size_t batch, void* stream) {
    return pf::dct_transform_batch<float>(s, in, out, batch, (hipStream_t)stream);
}
PF_EXPORT int pffftd_hip_dct_transform_batch(PFFFTD_HIP_DctSetup* s, const double* in, double* out, size_t batch, void* stream) {
    return pf::dct_transform_batch<double>(s, in, out, batch, (hipStream_t)stream);
}
PF_EXPORT const char* pffft_hip_dct_route(const void* setup) {
    const pf::DctSetup* z = pf::checked_handle<pf::DctSetup>(setup);
    if (!z) return "";
    return pf::dct_fused_now(z, pf::ab()) ? "fused" : "composed";
}
PF_EXPORT int pffft_hip_dct_table(const void* setup, size_t first, size_t count, void* host_out) {
    const pf::DctSetup* z = pf::checked_handle<pf::DctSetup>(setup);
    if (!z || !host_out) {
        pf::g_last_error = "pffft_hip: bad dct setup handle / NULL output";
        return (int)hipErrorInvalidValue;
    }
    const size_t len = (size_t)z->N / 2 + 1;
    if (first > len || count > len - first) {
        pf::g_last_error = "pffft_hip: dct table range beyond the table";
        return (int)hipErrorInvalidValue;
    }
    for (size_t i = 0; i < count; ++i) {
        if (z->is_double) static_cast<pf::cx<double>*>(host_out)[i] = pf::dct_table_value<double>(z, first + i);
        else static_cast<pf::cx<float>*>(host_out)[i] = pf::dct_table_value<float>(z, first + i);
    }
    return 0;
}
