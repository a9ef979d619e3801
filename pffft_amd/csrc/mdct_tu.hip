// libpffft_hip.so, translation unit of the MDCT / IMDCT frames and the type-IV cosine transform (include/pffft_hip.h:
// pffft[d]_hip_mdct_*): the type-IV cosine sum of M reals on ONE complex transform of M/2.  The handle owns an ordinary complex setup of
// M/2 and the two tables a_m, b_k; the fused kernel's instantiations and launch, and the composed routes through a per-stream scratch
// image.  Kernels: fft_mdct.h.
#include <memory>

#include "pf_compose.h"
#include "fft_mdct.h"

namespace pf {

constexpr uint32_t MDCT_MAGIC = 0x50464d44u;   // "PFMD"
enum { MDCT_DCT4 = 0, MDCT_FORWARD = 1, MDCT_OLA = 2 };   // `what` of pffft_hip_mdct_route

struct MdctSetup : InnerOwner<MDCT_MAGIC> {   // the owned inner setup: a complex one of M/2
    static constexpr const char* KIND = "mdct";
    int M = 0;
    std::mutex mu;                 // guards the lazy tables
    // a_m then b_k, m, k < M/2, per object that holds the inner setup's device state (for_device): one table per device the setup is used on
    std::map<const Setup*, DevBuf> d_tab;
    StreamScratch scratch;         // rows x M image of the composed routes and of the overlap-add: one per stream, scratch.mu held while a call enqueues
};

// ------------------------------------------------------------------------------------------------ the tables
// a_m = exp(-j pi (4m+1) / 4M) = W_{8M}^(4m+1), b_k = exp(-j pi k / M) = W_{2M}^k: integer phases below the denominator, the angle in
// long double, rounded once (pf_devmem.h)
template <typename T>
static cx<T> mdct_table_value(const MdctSetup* z, int which, size_t k) {
    return which == 0 ? unit_root<T>(4ll * (long long)k + 1, 8ll * z->M) : unit_root<T>((long long)k, 2ll * z->M);
}

template <typename T>
static int mdct_tables(MdctSetup* z, const Setup* s, hipStream_t st, const cx<T>** ta, const cx<T>** tb) {
    std::lock_guard<std::mutex> lk(z->mu);
    auto it = z->d_tab.find(s);
    const size_t n = (size_t)z->M / 2;
    if (it == z->d_tab.end()) {
        if (stream_capturing(st))
            return bad("mdct: the tables of this setup would have to be built during graph capture: run the call once before capturing",
                       hipErrorStreamCaptureUnsupported);
        std::vector<cx<T>> h(2 * n);
        for (size_t k = 0; k < n; ++k) { h[k] = mdct_table_value<T>(z, 0, k); h[n + k] = mdct_table_value<T>(z, 1, k); }
        DevBuf d;
        if (int rc = upload_table(d, h)) return rc;
        it = z->d_tab.emplace(s, std::move(d)).first;
    }
    *ta = it->second.as<cx<T>>();
    *tb = *ta + n;
    return 0;
}

// ------------------------------------------------------------------------------------------------ plan
typedef void (*MdctFn)(const float*, size_t, unsigned, const float*, float*, size_t, unsigned, float, const cx<float>*, const cx<float>*,
                       const cx<float>*, unsigned*);
typedef KernelSel<MdctFn> MdctSel;

template <class C>
static MdctSel mdct_sel(int load) {
    MdctSel e;
    e.wg = C::WG_THREADS; e.t_per_wg = C::T_PER_WG; e.lds = mdct_lds_bytes<C>(load);
    e.fn = load == MDCT_FRAME ? fft_mdct_kernel<C, MDCT_FRAME> : fft_mdct_kernel<C, MDCT_ROW>;
    return e;
}

// The fused kernel runs on the configuration of the inner setup's forward route in the canonical layout (visit_tiled_cfg_complex).
static const Route& mdct_route(const Setup* s) { return s->route[PFFFT_FORWARD][1]; }

static bool mdct_fusable(const MdctSetup* z, int load, MdctSel* e) {
    return visit_tiled_cfg_complex(z->inner, mdct_route(z->inner), [&](auto tag) {
        if (e) *e = mdct_sel<typename decltype(tag)::type>(load);
    });
}

// (M, what) cells where the fused kernel is the default: a cell is in it where tools/mdct_bench.py holds the fused kernel faster than
// selector 140 on the device by more than the spread of identical rounds - all six (dct4 0.35-0.41, forward 0.43-0.50, overlap-add
// 0.54-0.63 of the composed time against a spread below 3 %).  A cell that loses on a later measurement returns false
// here and stays reachable through AB_MDCT_FUSED.
static bool mdct_fused_default(int M, int what) {
    (void)M; (void)what;
    return true;
}

static bool mdct_fused_now(const MdctSetup* z, int what, const AbSel& sel) {
    return fused_selected(sel, AB_MDCT_COMPOSED, AB_MDCT_FUSED, mdct_fusable(z, MDCT_ROW, nullptr), mdct_fused_default(z->M, what));
}

static MdctSetup* mdct_new_setup(int M, int is_double) {
    if (M < 32 || M % 32) return nullptr;
    std::unique_ptr<MdctSetup> z(new MdctSetup);
    z->M = M;
    return z->new_inner(M / 2, PFFFT_COMPLEX, is_double) ? z.release() : nullptr;
}

// ------------------------------------------------------------------------------------------------ the core on either route
struct MdctTabs { const void *a, *b; };

// `count` rows (nframes == 0; consecutive rows in_stride apart) or frames (of nframes per signal; consecutive frames M apart) -> rows of
// `out`, one fused launch per slice
static int mdct_fused(Setup* s, const MdctSel& e, const float* in, size_t in_stride, size_t nframes, const float* window, float* out,
                      size_t out_stride, size_t count, float gain, const MdctTabs& tb, hipStream_t st) {
    const size_t row_step = nframes ? (size_t)s->N * 2 : in_stride;
    size_t resident = 0;
    if (int rc = loop_resident(e.fn, e.wg, e.lds, &resident)) return rc;
    const int oneshot = mdct_route(s).oneshot;   // the launch rule of the transform kernel whose configuration `e` was read from
    return for_slices(count, [&](size_t b0, size_t nb) {
        const LoopLaunch ll = loop_take(s, st, resident, (nb + e.t_per_wg - 1) / e.t_per_wg, oneshot);
        // (a frame call longer than one slice has one signal - mdct_transform_batch -, so its slices start at frame b0)
        hipLaunchKernelGGL(e.fn, dim3(ll.grid), dim3(e.wg), e.lds, st, in + b0 * row_step, in_stride, (unsigned)std::min(nframes, nb), window,
                           out + b0 * out_stride, out_stride, (unsigned)nb, gain, static_cast<const cx<float>*>(tb.a),
                           static_cast<const cx<float>*>(tb.b), s->d_tw.as<cx<float>>(), ll.ctr);
        PF_CHECK(hipGetLastError());
        return 0;
    });
}

// `cnt` rows (LOAD = MDCT_ROW: row v0 + r at in + (v0 + r) in_stride) or frames (MDCT_FRAME: v = v0 + r = i nframes + f) through the
// scratch rows X: fold, transform_batch in place, table product and scatter into rows of `out` (pitch out_stride; out may be X)
template <typename T, int LOAD>
static int mdct_composed_rows(MdctSetup* z, Setup* s, const T* in, size_t in_stride, size_t nframes, const T* window, T* X, T* out,
                              size_t out_stride, size_t v0, size_t cnt, T gain, const MdctTabs& tb, hipStream_t st) {
    constexpr size_t U = 16 / sizeof(T);
    const size_t M = (size_t)z->M;
    const cx<T>*ta = static_cast<const cx<T>*>(tb.a), *tbb = static_cast<const cx<T>*>(tb.b);
    const size_t items = cnt * (M / 8);
    if (int rc = stream_launch(in_stride % U == 0 ? mdct_fold_kernel<T, LOAD, true> : mdct_fold_kernel<T, LOAD, false>, items, st, in, in_stride, nframes,
                               window, X, ta, v0, cnt, (unsigned)M))
        return rc;
    if (int rc = transform_batch_any(s, X, X, cnt, PFFFT_FORWARD, 1, st)) return rc;
    return stream_launch(out_stride % U == 0 ? mdct_post_kernel<T, true> : mdct_post_kernel<T, false>, items, st, (const T*)X, out, out_stride, tbb, gain,
                         cnt, (unsigned)M);
}

// the object that holds the inner setup's tables on the calling thread's device, and the handle's own tables there
template <typename T>
static int mdct_open(MdctSetup* z, hipStream_t st, Setup** s, MdctTabs* tb) {
    *s = for_device(z->inner);
    if (int rc = ensure_device_any(*s, st)) return rc;
    const cx<T>*a = nullptr, *b = nullptr;
    if (int rc = mdct_tables<T>(z, *s, st, &a, &b)) return rc;
    tb->a = a; tb->b = b;
    return 0;
}

// ------------------------------------------------------------------------------------------------ dct4
template <typename T>
static int mdct_dct4_batch(void* setup, const T* in, T* out, size_t rows, hipStream_t st) {
    MdctSetup* z = typed_handle<MdctSetup, T>(setup);
    if (!z) return (int)hipErrorInvalidHandle;
    if (rows == 0) return 0;
    if (!in || !out) return bad("mdct: NULL in / out");
    if (((uintptr_t)in | (uintptr_t)out) & 15) return bad("mdct: in / out not aligned to 16 bytes");
    const size_t M = (size_t)z->M;
    const size_t len = rows * M * sizeof(T);   // the same rows in place, or rows that do not overlap
    if (in != out && ranges_overlap((uintptr_t)in, len, (uintptr_t)out, len)) return bad("mdct: in and out overlap without being equal");
    Setup* s = nullptr;
    MdctTabs tb;
    if (int rc = mdct_open<T>(z, st, &s, &tb)) return rc;
    if constexpr (sizeof(T) == 4) {
        MdctSel e;
        if (mdct_fused_now(z, MDCT_DCT4, ab()) && mdct_fusable(z, MDCT_ROW, &e))
            return mdct_fused(s, e, in, M, 0, nullptr, out, M, rows, 2.0f, tb, st);
    }
    return chunked_scratch<T>(z->scratch, st, rows, M * sizeof(T), "mdct: the scratch image", [&](T* X, size_t v0, size_t cnt) {
        return mdct_composed_rows<T, MDCT_ROW>(z, s, in, M, 0, nullptr, X, out + v0 * M, M, v0, cnt, (T)2, tb, st);
    });
}

// ------------------------------------------------------------------------------------------------ forward and overlap-add
// what the two frame entries check alike, in this order; ARGS_EMPTY for a call without signals (the entry returns 0)
template <typename T>
static int mdct_frame_args(const MdctSetup* z, const T* signal, size_t* signal_stride, size_t nsignals, size_t nframes, const T* window,
                           const T* coefs, size_t* coefs_stride) {
    if (nsignals == 0) return ARGS_EMPTY;
    if (nframes == 0) return bad("mdct: nframes == 0");
    const size_t M = (size_t)z->M;
    if (*coefs_stride == 0) *coefs_stride = M;
    if (*coefs_stride < M) return bad("mdct: coefs_stride smaller than one row of coefficients");
    if (nsignals > 1 && *signal_stride < (nframes + 1) * M) return bad("mdct: signal_stride smaller than one signal's samples");
    if (!signal || !coefs) return bad("mdct: NULL signal / coefs");
    if (((uintptr_t)signal | (uintptr_t)coefs | (uintptr_t)window) & 15) return bad("mdct: signal / window / coefs not aligned to 16 bytes");
    if (nsignals == 1) *signal_stride = 0;   // (one signal: the stride is not read)
    return 0;
}

template <typename T>
static int mdct_transform_batch(void* setup, const T* signal, size_t signal_stride, size_t nsignals, size_t nframes, const T* window,
                                T* coefs, size_t coefs_stride, hipStream_t st) {
    MdctSetup* z = typed_handle<MdctSetup, T>(setup);
    if (!z) return (int)hipErrorInvalidHandle;
    if (int rc = mdct_frame_args<T>(z, signal, &signal_stride, nsignals, nframes, window, coefs, &coefs_stride)) return rc == ARGS_EMPTY ? 0 : rc;
    Setup* s = nullptr;
    MdctTabs tb;
    if (int rc = mdct_open<T>(z, st, &s, &tb)) return rc;
    const size_t M = (size_t)z->M, batch = nsignals * nframes;
    if constexpr (sizeof(T) == 4) {
        MdctSel e;
        // 16-byte loads of every frame of every signal, 16-byte stores of every row; the kernel counts frames in 32 bits: longer batches
        // of ONE signal go out in slices, several signals that long are composed
        if (mdct_fused_now(z, MDCT_FORWARD, ab()) && signal_stride % 4 == 0 && coefs_stride % 4 == 0 && (batch <= ROW_SLICE || nsignals == 1) &&
            mdct_fusable(z, MDCT_FRAME, &e))
            return mdct_fused(s, e, signal, signal_stride, nframes, window, coefs, coefs_stride, batch, 1.0f, tb, st);
    }
    return chunked_scratch<T>(z->scratch, st, batch, M * sizeof(T), "mdct: the scratch image", [&](T* X, size_t v0, size_t cnt) {
        return mdct_composed_rows<T, MDCT_FRAME>(z, s, signal, signal_stride, nframes, window, X, coefs + v0 * coefs_stride, coefs_stride, v0, cnt,
                                                 (T)1, tb, st);
    });
}

template <typename T>
static int mdct_overlap_add_batch(void* setup, const T* coefs, size_t coefs_stride, size_t nsignals, size_t nframes, const T* window, T scaling,
                                  T* signal, size_t signal_stride, hipStream_t st) {
    MdctSetup* z = typed_handle<MdctSetup, T>(setup);
    if (!z) return (int)hipErrorInvalidHandle;
    if (int rc = mdct_frame_args<T>(z, signal, &signal_stride, nsignals, nframes, window, coefs, &coefs_stride)) return rc == ARGS_EMPTY ? 0 : rc;
    Setup* s = nullptr;
    MdctTabs tb;
    if (int rc = mdct_open<T>(z, st, &s, &tb)) return rc;
    constexpr size_t U = 16 / sizeof(T);
    const size_t M = (size_t)z->M, batch = nsignals * nframes, samples = (nframes + 1) * M, cap = cap_rows(M * sizeof(T));
    MdctSel e;
    bool fused = false;
    if constexpr (sizeof(T) == 4) fused = mdct_fused_now(z, MDCT_OLA, ab()) && coefs_stride % 4 == 0 && mdct_fusable(z, MDCT_ROW, &e);
    // v = C4 of the rows r0 ... r0 + cnt - 1 of coefs -> dense rows of V
    auto core = [&](size_t r0, size_t cnt, T* V) {
        if constexpr (sizeof(T) == 4)
            if (fused) return mdct_fused(s, e, coefs + r0 * coefs_stride, coefs_stride, 0, nullptr, V, M, cnt, 1.0f, tb, st);
        return mdct_composed_rows<T, MDCT_ROW>(z, s, coefs, coefs_stride, 0, nullptr, V, V, M, r0, cnt, (T)1, tb, st);
    };
    auto gather = [&](const T* V, size_t fbase, size_t fpitch, size_t fend, T* sig, size_t sig_stride, size_t nsig, size_t s0, size_t s1) {
        return stream_launch(aligned16(sig) && sig_stride % U == 0 ? mdct_ola_kernel<T, true> : mdct_ola_kernel<T, false>, nsig * (s1 - s0) / 4, st, V,
                             fbase, fpitch, fend, (unsigned)M, window, scaling, sig, sig_stride, nsig, s0, s1);
    };
    std::lock_guard<std::mutex> lk(z->scratch.mu);
    void* buf = nullptr;
    if (batch <= cap) {   // every frame at once, one gather
        if (int rc = scratch_buffer(z->scratch, st, batch * M * sizeof(T), "mdct: the scratch image", &buf)) return rc;
        if (int rc = core(0, batch, (T*)buf)) return rc;
        return gather((const T*)buf, 0, nframes, nframes, signal, signal_stride, nsignals, 0, samples);
    }
    // beyond the cap: signal by signal in runs of frames, each run re-transforming the one earlier frame that reaches into its samples
    const size_t reach = synth_reach(2 * M, M);
    const RunPlan p = synth_plan(nframes, cap, reach, 0);
    if (int rc = scratch_buffer(z->scratch, st, p.buffer_rows * M * sizeof(T), "mdct: the scratch image", &buf)) return rc;
    for (size_t i = 0; i < nsignals; ++i)
        for (size_t fa = 0; fa < nframes; fa += p.run) {
            const size_t fb = std::min(nframes, fa + p.run), f0 = fa > reach ? fa - reach : 0;
            if (int rc = core(i * nframes + f0, fb - f0, (T*)buf)) return rc;
            if (int rc = gather((const T*)buf, f0, 0, fb, signal + i * signal_stride, 0, 1, fa * M, fb == nframes ? samples : fb * M)) return rc;
        }
    return 0;
}

}  // namespace pf

PF_EXPORT PFFFT_HIP_MdctSetup* pffft_hip_mdct_new_setup(int M) { return reinterpret_cast<PFFFT_HIP_MdctSetup*>(pf::mdct_new_setup(M, 0)); }
PF_EXPORT PFFFTD_HIP_MdctSetup* pffftd_hip_mdct_new_setup(int M) { return reinterpret_cast<PFFFTD_HIP_MdctSetup*>(pf::mdct_new_setup(M, 1)); }
PF_EXPORT void pffft_hip_mdct_destroy_setup(PFFFT_HIP_MdctSetup* s) { pf::destroy_handle<pf::MdctSetup>(s); }
PF_EXPORT void pffftd_hip_mdct_destroy_setup(PFFFTD_HIP_MdctSetup* s) { pf::destroy_handle<pf::MdctSetup>(s); }
PF_EXPORT int pffft_hip_mdct_dct4_batch(PFFFT_HIP_MdctSetup* s, const float* in, float* out, size_t rows, void* stream) {
    return pf::mdct_dct4_batch<float>(s, in, out, rows, (hipStream_t)stream);
}
PF_EXPORT int pffftd_hip_mdct_dct4_batch(PFFFTD_HIP_MdctSetup* s, const double* in, double* out, size_t rows, void* stream) {
    return pf::mdct_dct4_batch<double>(s, in, out, rows, (hipStream_t)stream);
}
PF_EXPORT int pffft_hip_mdct_transform_batch(PFFFT_HIP_MdctSetup* s, const float* signal, size_t signal_stride, size_t nsignals, size_t nframes,
                                             const float* window, float* coefs, size_t coefs_stride, void* stream) {
    return pf::mdct_transform_batch<float>(s, signal, signal_stride, nsignals, nframes, window, coefs, coefs_stride, (hipStream_t)stream);
}
PF_EXPORT int pffftd_hip_mdct_transform_batch(PFFFTD_HIP_MdctSetup* s, const double* signal, size_t signal_stride, size_t nsignals,
                                              size_t nframes, const double* window, double* coefs, size_t coefs_stride, void* stream) {
    return pf::mdct_transform_batch<double>(s, signal, signal_stride, nsignals, nframes, window, coefs, coefs_stride, (hipStream_t)stream);
}
PF_EXPORT int pffft_hip_mdct_overlap_add_batch(PFFFT_HIP_MdctSetup* s, const float* coefs, size_t coefs_stride, size_t nsignals, size_t nframes,
                                               const float* window, float scaling, float* signal, size_t signal_stride, void* stream) {
    return pf::mdct_overlap_add_batch<float>(s, coefs, coefs_stride, nsignals, nframes, window, scaling, signal, signal_stride,
                                             (hipStream_t)stream);
}
PF_EXPORT int pffftd_hip_mdct_overlap_add_batch(PFFFTD_HIP_MdctSetup* s, const double* coefs, size_t coefs_stride, size_t nsignals,
                                                size_t nframes, const double* window, double scaling, double* signal, size_t signal_stride,
                                                void* stream) {
    return pf::mdct_overlap_add_batch<double>(s, coefs, coefs_stride, nsignals, nframes, window, scaling, signal, signal_stride,
                                              (hipStream_t)stream);
}
PF_EXPORT const char* pffft_hip_mdct_route(const void* setup, int what) {
    const pf::MdctSetup* z = pf::checked_handle<pf::MdctSetup>(setup);
    if (!z || what < pf::MDCT_DCT4 || what > pf::MDCT_OLA) return "";
    return pf::mdct_fused_now(z, what, pf::ab()) ? "fused" : "composed";
}
PF_EXPORT int pffft_hip_mdct_table(const void* setup, int which, size_t first, size_t count, void* host_out) {
    const pf::MdctSetup* z = pf::checked_handle<pf::MdctSetup>(setup);
    if (!z || !host_out || which < 0 || which > 1) {
        pf::g_last_error = "pffft_hip: bad mdct setup handle / table / NULL output";
        return (int)hipErrorInvalidValue;
    }
    const size_t len = (size_t)z->M / 2;
    if (first > len || count > len - first) {
        pf::g_last_error = "pffft_hip: mdct table range beyond the table";
        return (int)hipErrorInvalidValue;
    }
    for (size_t i = 0; i < count; ++i) {
        if (z->is_double) static_cast<pf::cx<double>*>(host_out)[i] = pf::mdct_table_value<double>(z, which, first + i);
        else static_cast<pf::cx<float>*>(host_out)[i] = pf::mdct_table_value<float>(z, which, first + i);
    }
    return 0;
}
