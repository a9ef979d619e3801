// libpffft_hip.so, translation unit of the band-energy entries (include/pffft_hip.h: pffft[d]_hip_bands_*): the handle with its host copy
// of the bank, validation, route decision, the fused kernel's instantiations and the composed route (the inner setup's own frame entry
// into a handle-owned scratch of |X|^2 rows, then the row kernel).  Kernels: fft_bands.h; framing rules and planners: pf_compose.h.
#include <cmath>
#include <memory>

#include "pf_compose.h"
#include "fft_bands.h"

static_assert(pf::BANDS_SEG == PFFFT_HIP_BANDS_SEG, "the segment length is part of the contract");
static_assert(pf::BANDS_ENERGY == PFFFT_HIP_BANDS_ENERGY && pf::BANDS_LOG == PFFFT_HIP_BANDS_LOG, "the values of `what`");

namespace pf {

constexpr uint32_t BANDS_MAGIC = 0x5046424eu;   // "PFBN"

// The owned inner setup: one of length N, real or complex.  One setup serves ONE device (bind_device_once builds the device tables).
struct BandsSetup : InnerOwner<BANDS_MAGIC> {
    static constexpr const char* KIND = "bands";
    unsigned nbands = 0, P = 0;
    unsigned long long nsegs = 0;      // segments of the whole bank: sum of ceil(count[b] / PFFFT_HIP_BANDS_SEG)
    std::vector<BandDesc> bank;        // host copy: (first, count, first segment, offset into the weights) per band
    std::vector<float> wf;             // host copy of the weights (the precision of the handle)
    std::vector<double> wd;
    DeviceBinding bound;
    DevBuf d_bank, d_segs, d_w;        // (d_segs: the segment list of the fused kernel, built from `bank` at the first call)
    StreamScratch rows;                // |X|^2 rows of the composed route: one buffer per stream, rows.mu held while a call enqueues
    template <typename T> std::vector<T>& w() {
        if constexpr (sizeof(T) == 8) return wd;
        else return wf;
    }
};

static void* bands_refuse(const char* what) {
    bad_in("bands: ", what);
    return nullptr;
}

template <typename T>
static void* bands_new_setup(int N, int transform, unsigned nbands, const unsigned* first, const unsigned* count, const T* weights) {
    constexpr int dbl = sizeof(T) == 8;
    if (transform != PFFFT_REAL && transform != PFFFT_COMPLEX) return bands_refuse("unknown transform");
    if (N < 1 || !(dbl ? pffftd_is_valid_size(N, (pffft_transform_t)transform) : pffft_is_valid_size(N, (pffft_transform_t)transform)))
        return bands_refuse("N is no length of this transform");
    if (nbands == 0) return bands_refuse("nbands == 0");
    if (!first || !count || !weights) return bands_refuse("NULL first / count / weights");
    const unsigned P = transform == PFFFT_REAL ? (unsigned)N / 2 + 1 : (unsigned)N;
    std::unique_ptr<BandsSetup> z(new BandsSetup);
    z->nbands = nbands; z->P = P;
    z->bank.resize(nbands);
    unsigned long long total = 0;
    for (unsigned b = 0; b < nbands; ++b) {
        if ((unsigned long long)first[b] + count[b] > P) return bands_refuse("first[b] + count[b] exceeds the bins of a row");
        z->bank[b] = BandDesc{first[b], count[b], (unsigned)std::min<unsigned long long>(z->nsegs, 0xffffffffull), 0, total};
        total += count[b];
        z->nsegs += (count[b] + BANDS_SEG - 1) / BANDS_SEG;
    }
    for (unsigned long long j = 0; j < total; ++j)
        if (!std::isfinite(weights[j])) return bands_refuse("a weight is not finite");
    z->template w<T>().assign(weights, weights + total);
    if (!z->new_inner(N, transform, dbl)) return bands_refuse("the inner setup could not be created");
    return z.release();
}

// ------------------------------------------------------------------------------------------------ fused
typedef void (*BandsFn)(const float*, size_t, unsigned, size_t, const float*, float*, size_t, unsigned, const BandDesc*, const SegDesc*,
                        const float*, unsigned, unsigned, float, float, const cx<float>*, const cx<float>*, unsigned*);
struct BandsSel : KernelSel<BandsFn> { unsigned seg_cap = 0; };   // (seg_cap: the segments the configuration's image has room for)

// Window values: resident in registers (WMODE 1), as in the frame kernel: the resource remarks of the twelve instantiations show no scratch
// and the waves of fft_frames_kernel<C, FR_POWER, 1> (tools/bands_resources.py).
constexpr int BANDS_WMODE = 1;

template <class C>
static BandsSel bands_sel(bool windowed, int what) {
    BandsSel e;
    e.wg = C::WG_THREADS; e.t_per_wg = C::T_PER_WG;
    e.lds = frames_lds_bytes<C>(windowed ? BANDS_WMODE : 0);
    e.seg_cap = bands_seg_cap<C>();
    if (windowed) e.fn = what == BANDS_LOG ? fft_bands_kernel<C, BANDS_WMODE, BANDS_LOG> : fft_bands_kernel<C, BANDS_WMODE, BANDS_ENERGY>;
    else e.fn = what == BANDS_LOG ? fft_bands_kernel<C, 0, BANDS_LOG> : fft_bands_kernel<C, 0, BANDS_ENERGY>;
    return e;
}

// The frame entry's rule: p[k] equals the POWER output of pffft_hip_frames_transform_batch bit for bit only on the configuration
// transform_batch(ordered = 1) runs on, so that is read from the inner setup's stored route.
static bool bands_fusable_setup(const Setup* s, BandsSel* e, bool windowed, int what) {
    return visit_tiled_cfg(s, s->route[PFFFT_FORWARD][1], [&](auto tag) {
        if (e) *e = bands_sel<typename decltype(tag)::type>(windowed, what);
    });
}

// Sizes where the fused kernel is the default: where tools/bands_bench.py held selector 161 faster than selector 160 on the device by more
// than the spread of the round-bests (tests/test_gpu_bands.py test_default_cells holds the ordering).  A size that loses
// returns false here and stays reachable through AB_BANDS_FUSED.
static bool bands_fused_default(int N) {
    (void)N;
    return true;
}

// the route of a call whose pointers are 16-byte aligned: true = fused.  Descriptors and weights are read through L2, so nbands and the
// sum of the counts have no cap; the partials of the bank's segments live in the slot's image, so their number has one (include/pffft_hip.h:
// 658 / 1298 / 2578 at N = 1024 / 2048 / 4096).  The rows are stored scalar by scalar: no rule for out_stride.
static bool bands_route_fused(const BandsSetup* z, size_t hop, size_t signal_stride, const AbSel& sel) {
    if (hop % 4 || signal_stride % 4) return false;
    BandsSel e;
    const bool fusable = bands_fusable_setup(z->inner, &e, true, 0) && z->nsegs <= e.seg_cap;
    return fused_selected(sel, AB_BANDS_COMPOSED, AB_BANDS_FUSED, fusable, bands_fused_default(z->inner->N));
}
static_assert(bands_seg_cap<TiledPick<float>::C512>() == 658 && bands_seg_cap<TiledPick<float>::C1024>() == 1298 &&
              bands_seg_cap<TiledPick<float>::C2048>() == 2578, "the caps stated in include/pffft_hip.h");

// ------------------------------------------------------------------------------------------------ composed
template <typename T>
static int inner_frames_power(Setup* inner, const T* signal, size_t signal_stride, size_t nsignals, size_t nframes, size_t hop, const T* window,
                              T* out, hipStream_t st) {
    if constexpr (sizeof(T) == 8)
        return pffftd_hip_frames_transform_batch(static_cast<PFFFTD_Setup*>(inner), signal, signal_stride, nsignals, nframes, hop, window, out, 0,
                                                 PFFFT_HIP_FRAMES_POWER, st);
    else
        return pffft_hip_frames_transform_batch(static_cast<PFFFT_Setup*>(inner), signal, signal_stride, nsignals, nframes, hop, window, out, 0,
                                                PFFFT_HIP_FRAMES_POWER, st);
}

// How the composed route cuts nsignals x nframes frames into chunks of at most `cap` rows: whole signals where one signal's rows fit, else
// runs of frames of one signal.
struct BandsChunks { size_t sigs, frames; };   // signals per chunk (frames == nframes), or frames per chunk of one signal (sigs == 1)
constexpr BandsChunks bands_chunks(size_t nsignals, size_t nframes, size_t cap) {
    if (nframes <= cap) return {std::min(nsignals, cap / nframes), nframes};
    return {1, cap};
}
static_assert(bands_chunks(3, 5, 100).sigs == 3 && bands_chunks(3, 5, 100).frames == 5, "a batch under the cap: one chunk");
static_assert(bands_chunks(30, 40, 100).sigs == 2 && bands_chunks(30, 40, 100).frames == 40, "whole signals");
static_assert(bands_chunks(3, 102, 100).sigs == 1 && bands_chunks(3, 102, 100).frames == 100, "one signal beyond the cap: runs of frames");
static_assert(bands_chunks(3, 100, 100).sigs == 1 && bands_chunks(3, 100, 100).frames == 100, "one signal exactly at the cap");

template <typename T>
static int bands_composed(BandsSetup* z, const AnalysisArgs& a, const T* signal, size_t signal_stride, size_t nsignals, size_t nframes, size_t hop,
                          const T* window, T scaling, T floor, int what, T* out, size_t out_stride, hipStream_t st) {
    const size_t P = z->P;
    const BandsChunks c = bands_chunks(nsignals, nframes, cap_rows(P * sizeof(T)));
    std::lock_guard<std::mutex> lk(z->rows.mu);
    void* buf = nullptr;
    if (int rc = scratch_buffer(z->rows, st, c.sigs * c.frames * P * sizeof(T), "the band scratch", &buf)) return rc;
    T* X = static_cast<T*>(buf);
    const BandDesc* bank = z->d_bank.as<BandDesc>();
    const T* w = z->d_w.as<T>();
    auto reduce = [&](size_t v0, size_t rows) {
        T* dst = out + v0 * out_stride;
        return what == BANDS_LOG ? stream_launch(bands_rows_kernel<T, BANDS_LOG>, rows * z->nbands, st, (const T*)X, (unsigned)P, rows, bank, w, z->nbands, scaling, floor, dst, out_stride)
                                 : stream_launch(bands_rows_kernel<T, BANDS_ENERGY>, rows * z->nbands, st, (const T*)X, (unsigned)P, rows, bank, w, z->nbands, scaling, floor, dst, out_stride);
    };
    if (c.frames == nframes) {
        for (size_t i0 = 0; i0 < nsignals; i0 += c.sigs) {
            const size_t ns = std::min(nsignals - i0, c.sigs);
            if (int rc = inner_frames_power<T>(z->inner, signal + i0 * signal_stride, signal_stride, ns, nframes, hop, window, X, st)) return rc;
            if (int rc = reduce(i0 * nframes, ns * nframes)) return rc;
        }
        return 0;
    }
    for (size_t i = 0; i < nsignals; ++i)
        for (size_t f0 = 0; f0 < nframes; f0 += c.frames) {
            const size_t nf = std::min(nframes - f0, c.frames);
            if (int rc = inner_frames_power<T>(z->inner, signal + i * signal_stride + f0 * a.hop_s, 0, 1, nf, hop, window, X, st)) return rc;
            if (int rc = reduce(i * nframes + f0, nf)) return rc;
        }
    return 0;
}

// ------------------------------------------------------------------------------------------------ the entry
template <typename T>
static int bands_batch(void* setup, const T* signal, size_t signal_stride, size_t nsignals, size_t nframes, size_t hop, const T* window,
                       T scaling, T floor, int what, T* out, size_t out_stride, hipStream_t st) {
    BandsSetup* z = typed_handle<BandsSetup, T>(setup);
    if (!z) return (int)hipErrorInvalidHandle;
    if (what != BANDS_ENERGY && what != BANDS_LOG) return bad("bands: unknown what");
    if (what == BANDS_LOG && !(std::isfinite(floor) && floor > (T)0)) return bad("bands: the floor of LOG must be finite and > 0");
    if (what == BANDS_ENERGY) floor = (T)0;   // (not read)
    AnalysisArgs a;
    size_t power_stride = 0;   // the |X|^2 rows are the route's own: dense
    if (int rc = analysis_args<T>("bands: ", z->inner, signal, &signal_stride, nsignals, nframes, hop, out, &power_stride, FR_POWER, &a))
        return rc == ARGS_EMPTY ? 0 : rc;
    if (out_stride == 0) out_stride = z->nbands;
    if (out_stride < z->nbands) return bad("bands: out_stride smaller than one output row");
    if (int rc = bind_device_once(z->bound, "bands: ", st, [&] {
            if (int rc = upload_table(z->d_bank, z->bank)) return rc;
            BandsSel cfg;
            if (sizeof(T) == 4 && z->nsegs && bands_fusable_setup(z->inner, &cfg, true, 0) && z->nsegs <= cfg.seg_cap) {   // (where fused can run)
                std::vector<SegDesc> segs;
                for (const BandDesc& bd : z->bank)
                    for (unsigned s0 = 0; s0 < bd.count; s0 += BANDS_SEG)
                        segs.push_back(SegDesc{bd.first + s0, std::min(bd.count - s0, BANDS_SEG), bd.off + s0});
                if (int rc = upload_table(z->d_segs, segs)) return rc;
            }
            return z->template w<T>().empty() ? 0 : upload_table(z->d_w, z->template w<T>());
        }))
        return rc;
    if constexpr (sizeof(T) == 4) {
        BandsSel e;
        // (the kernel counts frames in 32 bits: longer batches of ONE signal go out in slices; several signals that long are composed)
        if (bands_route_fused(z, hop, signal_stride, ab()) && aligned16(signal) && (!window || aligned16(window)) &&
            bands_fusable_setup(z->inner, &e, window != nullptr, what) && (a.batch <= ROW_SLICE || nsignals == 1)) {
            if (int rc = inner_on_device(z->inner, st)) return rc;
            Setup* s = z->inner;
            const int oneshot = s->route[PFFFT_FORWARD][1].oneshot;
            return for_slices(a.batch, [&](size_t b0, size_t nb) {
                LoopLaunch ll;
                if (int rc = loop_launch(s, st, e.fn, e.wg, e.lds, (nb + e.t_per_wg - 1) / e.t_per_wg, oneshot, &ll)) return rc;
                hipLaunchKernelGGL(e.fn, dim3(ll.grid), dim3(e.wg), e.lds, st, signal + b0 * a.hop_s, signal_stride,
                                   (unsigned)(nsignals == 1 ? nb : nframes), a.hop_s, window, out + b0 * out_stride, out_stride, (unsigned)nb,
                                   z->d_bank.as<BandDesc>(), z->d_segs.as<SegDesc>(), z->d_w.as<float>(), z->nbands, (unsigned)z->nsegs, scaling, floor, s->d_tw.as<cx<float>>(),
                                   s->d_twr.as<cx<float>>(), ll.ctr);
                PF_CHECK(hipGetLastError());
                return 0;
            });
        }
    }
    return bands_composed<T>(z, a, signal, signal_stride, nsignals, nframes, hop, window, scaling, floor, what, out, out_stride, st);
}

}  // namespace pf

PF_EXPORT PFFFT_HIP_Bands_Setup* pffft_hip_bands_new_setup(int N, pffft_transform_t transform, unsigned nbands, const unsigned* first,
                                                           const unsigned* count, const float* weights) {
    return reinterpret_cast<PFFFT_HIP_Bands_Setup*>(pf::bands_new_setup<float>(N, (int)transform, nbands, first, count, weights));
}
PF_EXPORT PFFFTD_HIP_Bands_Setup* pffftd_hip_bands_new_setup(int N, pffft_transform_t transform, unsigned nbands, const unsigned* first,
                                                             const unsigned* count, const double* weights) {
    return reinterpret_cast<PFFFTD_HIP_Bands_Setup*>(pf::bands_new_setup<double>(N, (int)transform, nbands, first, count, weights));
}
PF_EXPORT void pffft_hip_bands_destroy_setup(PFFFT_HIP_Bands_Setup* s) { pf::destroy_handle<pf::BandsSetup>(s); }
PF_EXPORT void pffftd_hip_bands_destroy_setup(PFFFTD_HIP_Bands_Setup* s) { pf::destroy_handle<pf::BandsSetup>(s); }
PF_EXPORT int pffft_hip_bands_batch(PFFFT_HIP_Bands_Setup* s, const float* signal, size_t signal_stride, size_t nsignals, size_t nframes, size_t hop,
                                    const float* window, float scaling, float floor, int what, float* out, size_t out_stride, void* stream) {
    return pf::bands_batch<float>(s, signal, signal_stride, nsignals, nframes, hop, window, scaling, floor, what, out, out_stride, (hipStream_t)stream);
}
PF_EXPORT int pffftd_hip_bands_batch(PFFFTD_HIP_Bands_Setup* s, const double* signal, size_t signal_stride, size_t nsignals, size_t nframes,
                                     size_t hop, const double* window, double scaling, double floor, int what, double* out, size_t out_stride,
                                     void* stream) {
    return pf::bands_batch<double>(s, signal, signal_stride, nsignals, nframes, hop, window, scaling, floor, what, out, out_stride, (hipStream_t)stream);
}
PF_EXPORT const char* pffft_hip_bands_route(const void* setup, size_t hop, size_t signal_stride) {
    const pf::BandsSetup* z = pf::checked_handle<pf::BandsSetup>(setup);
    if (!z || hop == 0) return "";
    return pf::bands_route_fused(z, hop, signal_stride, pf::ab()) ? "fused" : "composed";
}
PF_EXPORT unsigned pffft_hip_bands_count(const void* setup) {
    const pf::BandsSetup* z = pf::checked_handle<pf::BandsSetup>(setup);
    return z ? z->nbands : 0;
}
PF_EXPORT unsigned pffft_hip_bands_bins(const void* setup) {
    const pf::BandsSetup* z = pf::checked_handle<pf::BandsSetup>(setup);
    return z ? z->P : 0;
}
