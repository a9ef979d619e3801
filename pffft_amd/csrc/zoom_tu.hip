// libpffft_hip.so, translation unit of the zoom transforms (include/pffft_hip.h: pffft[d]_hip_zoom_*): K spectral lines from f0 in steps
// of df, by Bluestein's algorithm on the library's own convolution.  Plan (route, convolution length) at setup, tables on first use from
// exactly reduced phases, the fused kernel's launch and the composed route through a per-stream scratch image.  Kernels: fft_zoom.h.
#include <cmath>
#include <memory>

#include "bluestein_host.h"
#include "fft_zoom.h"

namespace pf {

constexpr uint32_t ZOOM_MAGIC = 0x50465A4Du;   // "PFZM"
constexpr long long ZOOM_MAX_CONV = 1ll << 26;  // N + K - 1 <= 2^26, the library's largest setup

// ------------------------------------------------------------------------------------------------ exact phases
// frac(n f0 + n^2 df / 2) from the exact rational value of the doubles.  A finite double is m 2^e with |m| < 2^53, and n^2 m < 2^105 for
// n < 2^26: every term is a 128-bit integer times a power of two.  The terms are added modulo 1 in a fixed-point fraction of W 64-bit
// words (W covers the lowest bit of either term: at most 17 words for the smallest subnormal), the sum is moved to (-1/2, 1/2] and rounded
// ONCE, to nearest even, to the 64 significant bits of long double.
struct Dyadic {
    unsigned long long m = 0;   // |x| = m 2^e
    int e = 0, neg = 0;
};
static Dyadic dyadic(double x) {
    Dyadic d;
    if (x == 0) return d;
    int ex = 0;
    const double f = frexp(fabs(x), &ex);            // |x| = f 2^ex, 1/2 <= f < 1
    d.m = (unsigned long long)ldexp(f, 53);          // exact: 53 bits
    d.e = ex - 53;
    d.neg = x < 0;
    while (!(d.m & 1)) { d.m >>= 1; ++d.e; }         // (fewer words for round values)
    return d;
}

constexpr int PH_WORDS = 18;
struct Phase {
    int W = 2;             // words in use
    Dyadic f0, hdf;        // f0 and df / 2
    void plan(double f0_, double df_) {
        f0 = dyadic(f0_);
        hdf = dyadic(df_);
        if (hdf.m) hdf.e -= 1;
        const int need = std::max(std::max(-f0.e, -hdf.e), 0);
        W = std::min(PH_WORDS, std::max(2, (need + 63) / 64));
    }
    // acc (little-endian words: value = acc / 2^(64 W)) += sign . I . 2^e  modulo 1
    void add(unsigned long long* acc, unsigned __int128 I, const Dyadic& d) const {
        if (!I) return;
        const long long sh = (long long)d.e + 64ll * W;   // >= 0 by plan()
        if (sh >= 64ll * W) return;                       // an integer: nothing below the point
        unsigned long long t[PH_WORDS];
        for (int i = 0; i < W; ++i) t[i] = 0;
        const int w0 = (int)(sh / 64), b = (int)(sh % 64);
        const unsigned long long lo = (unsigned long long)I, hi = (unsigned long long)(I >> 64);
        const unsigned long long part[3] = {lo << b, b ? (lo >> (64 - b)) | (hi << b) : hi, b ? hi >> (64 - b) : 0ull};
        for (int i = 0; i < 3; ++i)
            if (w0 + i < W) t[w0 + i] = part[i];
        if (d.neg) {   // two's complement: -t modulo 2^(64 W)
            unsigned long long c = 1;
            for (int i = 0; i < W; ++i) { t[i] = ~t[i] + c; c = (c && t[i] == 0) ? 1 : 0; }
        }
        unsigned long long c = 0;
        for (int i = 0; i < W; ++i) {
            const unsigned long long s = acc[i] + t[i], s2 = s + c;
            c = (s < acc[i]) || (s2 < s) ? 1 : 0;
            acc[i] = s2;
        }
    }
    // the reduced phase of index n, in (-1/2, 1/2], rounded once
    long double reduced(unsigned long long n, bool with_f0) const {
        unsigned long long acc[PH_WORDS];
        for (int i = 0; i < W; ++i) acc[i] = 0;
        if (with_f0) add(acc, (unsigned __int128)n * f0.m, f0);
        add(acc, (unsigned __int128)(n * n) * hdf.m, hdf);   // (n < 2^26: n^2 < 2^52)
        // above one half: the phase is acc - 1
        bool low = false;
        for (int i = 0; i + 1 < W; ++i) low |= acc[i] != 0;
        const unsigned long long top = 1ull << 63;
        const bool negative = acc[W - 1] > top || (acc[W - 1] == top && low);
        if (negative) {
            unsigned long long c = 1;
            for (int i = 0; i < W; ++i) { acc[i] = ~acc[i] + c; c = (c && acc[i] == 0) ? 1 : 0; }
        }
        int hw = W - 1;
        while (hw >= 0 && !acc[hw]) --hw;
        if (hw < 0) return 0.0L;
        const int hb = 64 * hw + 63 - __builtin_clzll(acc[hw]);   // the highest set bit
        unsigned long long mant;
        int lsb = hb - 63;                                          // weight of mant's lowest bit: 2^(lsb - 64 W)
        if (lsb <= 0) {
            mant = acc[0];                                          // (hw == 0: fewer than 65 bits, exact)
            lsb = 0;
        } else {
            const int w = lsb / 64, b = lsb % 64;
            mant = b ? (acc[w] >> b) | (acc[w + 1] << (64 - b)) : acc[w];
            // round to nearest even on the bits below lsb
            const int rb = lsb - 1, rw = rb / 64, rbit = rb % 64;
            const bool round = (acc[rw] >> rbit) & 1;
            bool sticky = (acc[rw] & ((1ull << rbit) - 1)) != 0;
            for (int i = 0; i < rw; ++i) sticky |= acc[i] != 0;
            if (round && (sticky || (mant & 1))) {
                if (++mant == 0) { mant = top; ++lsb; }
            }
        }
        const long double p = ldexpl((long double)mant, lsb - 64 * W);
        return negative ? -p : p;
    }
    // exp(-2 pi j p): the angle in long double, cos and sin rounded once to T
    template <typename T>
    cx<T> value(unsigned long long n, bool with_f0) const {
        const long double ang = (2.0L * 3.14159265358979323846264338327950288L) * reduced(n, with_f0);
        cx<T> w;
        w.x = (T)cosl(ang); w.y = (T)(-sinl(ang));
        return w;
    }
};

// ------------------------------------------------------------------------------------------------ the setup
// The owned inner setup has length M.  One setup serves ONE device, like the any-length setups (bind_device_once).
struct ZoomSetup : InnerOwner<ZOOM_MAGIC> {
    static constexpr const char* KIND = "zoom";
    int N = 0, K = 0;
    double f0 = 0, df = 0;
    Phase ph;
    bool fusable = false;          // float and M in the fused set: both routes exist, on the same M
    int M = 0;                     // convolution length
    DeviceBinding bound;
    DevBuf d_a;                    // a[n], n < N (fusable: M entries, zero from N on)
    DevBuf d_c;                    // c[k], k < K (fusable: M entries, zero from K on)
    DevBuf d_H;                    // spectrum of the filter b in the inner setup's internal layout
    StreamScratch pad;             // batch x M image of the composed route: one per stream, pad.mu held while a call enqueues
};

// ------------------------------------------------------------------------------------------------ plan
// The fused kernel exists for float and these convolution lengths (M2 = next power of two >= N + K - 1).  Per row it moves 8 (N + K)
// bytes in one launch where the composed route moves 8 (N + K) + 4 M 8 in three.  Which lengths RUN fused by default is the table
// zoom_fused_default: a length is in it where tests/test_gpu_zoom.py holds the fused kernel faster than selector 136 on the device by
// more than the spread of the composed route's rounds (0.37 / 0.38 / 0.51 / 0.64 of the composed time at M = 512 / 1024 / 2048 / 4096;
// DESIGN.md §3.15 has the table).  Selectors 136 / 137 pin either route.
static bool zoom_fused_len(int M) { return M == 512 || M == 1024 || M == 2048 || M == 4096; }
static bool zoom_fused_default(int M) {
    switch (M) {
        case 512: return true;
        case 1024: return true;
        case 2048: return true;
        case 4096: return true;
        default: return false;
    }
}

static ZoomSetup* zoom_new_setup(int N, int K, double f0, double df, int is_double) {
    if (N < 1 || K < 1 || (long long)N + K - 1 > ZOOM_MAX_CONV || !std::isfinite(f0) || !std::isfinite(df)) return nullptr;
    std::unique_ptr<ZoomSetup> z(new ZoomSetup);
    z->N = N; z->K = K; z->f0 = f0; z->df = df;
    z->ph.plan(f0, df);
    const long long need = (long long)N + K - 1;
    long long p2 = 16;
    while (p2 < need) p2 *= 2;
    z->fusable = !is_double && zoom_fused_len((int)p2);
    // (a setup that can run fused runs BOTH routes on M2: one filter spectrum, one answer to pffft_hip_zoom_conv_size)
    z->M = z->fusable ? (int)p2 : pffft_nearest_transform_size((int)need, PFFFT_COMPLEX, 1);
    return z->new_inner(z->M, PFFFT_COMPLEX, is_double) ? z.release() : nullptr;
}

// the route of a call under the calling thread's selector
static bool zoom_fused_now(const ZoomSetup* z, const AbSel& sel) {
    return fused_selected(sel, AB_ZOOM_COMPOSED, AB_ZOOM_FUSED, z->fusable, zoom_fused_default(z->M));
}

// ------------------------------------------------------------------------------------------------ tables
template <typename T>
static int zoom_build_tables(ZoomSetup* z) {
    const size_t N = (size_t)z->N, K = (size_t)z->K, M = (size_t)z->M;
    std::vector<cx<T>> w(z->fusable ? M : N);
    for (size_t n = 0; n < N; ++n) w[n] = z->ph.value<T>(n, true);
    for (size_t n = N; n < w.size(); ++n) w[n] = mk<T>(0, 0);
    int rc = upload_table(z->d_a, w);
    if (rc) return rc;
    w.assign(z->fusable ? M : K, mk<T>(0, 0));
    for (size_t k = 0; k < K; ++k) w[k] = z->ph.value<T>(k, false);
    if ((rc = upload_table(z->d_c, w))) return rc;
    // b[m] = conj(c[|m|]) for -(N-1) <= m <= K-1 (negative m at M + m), zero elsewhere - in double whatever the setup's type
    std::vector<cx<double>> b(M);
    for (size_t m = 0; m < M; ++m) b[m] = mk<double>(0, 0);
    for (size_t m = 0; m < std::max(N, K); ++m) {
        const cx<double> c = z->ph.value<double>(m, false);
        if (m < K) b[m] = mk<double>(c.x, -c.y);
        if (m && m < N) b[M - m] = mk<double>(c.x, -c.y);
    }
    return bluestein_filter_spectrum<T>(z->inner, M, b, z->d_H);
}

template <typename T>
static int zoom_ensure(ZoomSetup* z, hipStream_t st) {
    return bind_device_once(z->bound, "zoom: ", st, [&] { return zoom_build_tables<T>(z); });
}

// ------------------------------------------------------------------------------------------------ the two routes (bluestein_host.h)
static int zoom_fused(ZoomSetup* z, const float* in, float* out, size_t batch, int cj, hipStream_t st) {
    return bluestein_fused(z->inner, z->M, batch, st, [&](auto tag, size_t b0, size_t nb) {
        typedef typename decltype(tag)::type C;
        const ZoomIO<C, ZoomHold<C>::value> io{in + b0 * 2 * (size_t)z->N, out + b0 * 2 * (size_t)z->K, z->d_a.as<cx<float>>(),
                                               z->d_c.as<cx<float>>(), (unsigned)z->N, (unsigned)z->K, cj};
        return bluestein_fused_launch<C>(z->inner, io, (const float*)z->d_H.as<float>(), nb, z->M, st);
    });
}

template <typename T>
static int zoom_composed(ZoomSetup* z, const T* in, T* out, size_t batch, int cj, hipStream_t st) {
    const size_t N = (size_t)z->N, K = (size_t)z->K, M = (size_t)z->M;
    return bluestein_composed<T>(
        z->inner, z->pad, (const T*)z->d_H.as<T>(), M, batch, st,
        [&](cx<T>* X, size_t v0, size_t cnt) {
            return stream_launch(zoom_pad_kernel<T>, cnt * M, st, reinterpret_cast<const cx<T>*>(in) + v0 * N, X, z->d_a.as<cx<T>>(), cnt, N, M, cj);
        },
        [&](cx<T>* X, size_t v0, size_t cnt) {
            return stream_launch(zoom_crop_kernel<T>, cnt * K, st, (const cx<T>*)X, reinterpret_cast<cx<T>*>(out) + v0 * K, z->d_c.as<cx<T>>(), cnt, K, M,
                                 cj);
        });
}

// ------------------------------------------------------------------------------------------------ the entry
template <typename T>
static int zoom_transform_batch(void* setup, const T* in, T* out, size_t batch, int dir, hipStream_t st) {
    ZoomSetup* z = typed_handle<ZoomSetup, T>(setup);
    if (!z) return (int)hipErrorInvalidHandle;
    if (dir != PFFFT_FORWARD && dir != PFFFT_BACKWARD) return bad("zoom: bad direction");
    if (batch && (!in || !out)) return bad("zoom: NULL in / out");
    if (((uintptr_t)in | (uintptr_t)out) & (2 * sizeof(T) - 1)) return bad("zoom: in / out not aligned to one complex value");
    // rows of N in, rows of K out: the two must not overlap
    if (batch && ranges_overlap((uintptr_t)in, batch * (size_t)z->N * 2 * sizeof(T), (uintptr_t)out, batch * (size_t)z->K * 2 * sizeof(T)))
        return bad("zoom: in and out overlap");
    int rc = zoom_ensure<T>(z, st);
    if (rc || batch == 0) return rc;
    const int cj = dir == PFFFT_BACKWARD;
    if constexpr (sizeof(T) == 4)
        if (zoom_fused_now(z, ab())) return zoom_fused(z, in, out, batch, cj, st);
    return zoom_composed<T>(z, in, out, batch, cj, st);
}

template <typename T>
static void zoom_table_fill(const ZoomSetup* z, int which, size_t first, size_t count, void* host_out) {
    cx<T>* o = static_cast<cx<T>*>(host_out);
    for (size_t i = 0; i < count; ++i) o[i] = z->ph.value<T>(first + i, which == 0);
}

}  // namespace pf

PF_EXPORT PFFFT_HIP_ZoomSetup* pffft_hip_zoom_new_setup(int N, int K, double f0, double df) {
    return reinterpret_cast<PFFFT_HIP_ZoomSetup*>(pf::zoom_new_setup(N, K, f0, df, 0));
}
PF_EXPORT PFFFTD_HIP_ZoomSetup* pffftd_hip_zoom_new_setup(int N, int K, double f0, double df) {
    return reinterpret_cast<PFFFTD_HIP_ZoomSetup*>(pf::zoom_new_setup(N, K, f0, df, 1));
}
PF_EXPORT void pffft_hip_zoom_destroy_setup(PFFFT_HIP_ZoomSetup* s) { pf::destroy_handle<pf::ZoomSetup>(s); }
PF_EXPORT void pffftd_hip_zoom_destroy_setup(PFFFTD_HIP_ZoomSetup* s) { pf::destroy_handle<pf::ZoomSetup>(s); }
PF_EXPORT int pffft_hip_zoom_transform_batch(PFFFT_HIP_ZoomSetup* s, const float* in, float* out, size_t batch, pffft_direction_t d, void* stream) {
    return pf::zoom_transform_batch<float>(s, in, out, batch, (int)d, (hipStream_t)stream);
}
PF_EXPORT int pffftd_hip_zoom_transform_batch(PFFFTD_HIP_ZoomSetup* s, const double* in, double* out, size_t batch, pffft_direction_t d,
                                              void* stream) {
    return pf::zoom_transform_batch<double>(s, in, out, batch, (int)d, (hipStream_t)stream);
}
PF_EXPORT int pffft_hip_zoom_conv_size(const void* setup) {
    const pf::ZoomSetup* z = pf::checked_handle<pf::ZoomSetup>(setup);
    return z ? z->M : -1;
}
PF_EXPORT const char* pffft_hip_zoom_route(const void* setup) {
    const pf::ZoomSetup* z = pf::checked_handle<pf::ZoomSetup>(setup);
    if (!z) return "";
    return pf::zoom_fused_now(z, pf::ab()) ? "fused" : "composed";
}
PF_EXPORT int pffft_hip_zoom_table(const void* setup, int which, size_t first, size_t count, void* host_out) {
    const pf::ZoomSetup* z = pf::checked_handle<pf::ZoomSetup>(setup);
    if (!z || !host_out || (which != 0 && which != 1)) {
        pf::g_last_error = "pffft_hip: bad zoom setup handle / table / NULL output";
        return (int)hipErrorInvalidValue;
    }
    const size_t len = which == 0 ? (size_t)z->N : (size_t)std::max(z->N, z->K);
    if (first > len || count > len - first) {
        pf::g_last_error = "pffft_hip: zoom table range beyond the table";
        return (int)hipErrorInvalidValue;
    }
    if (z->is_double) pf::zoom_table_fill<double>(z, which, first, count, host_out);
    else pf::zoom_table_fill<float>(z, which, first, count, host_out);
    return 0;
}
