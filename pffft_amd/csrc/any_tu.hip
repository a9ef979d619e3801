// libpffft_hip.so, translation unit of the any-length transforms, complex and real (include/pffft_hip.h: pffft[d]_hip_any_*): Bluestein's
// algorithm on the library's own convolution.  Plan (route, convolution length) at setup, tables on first use, the fused kernel's launch and the
// composed route through a per-stream scratch image.  Kernels: fft_any.h.
#include <memory>

#include "bluestein_host.h"
#include "fft_any.h"

namespace pf {

constexpr uint32_t ANY_MAGIC = 0x50464159u;   // "PFAY"
constexpr int ANY_MAX_N = 1 << 25;             // M <= 2^26, the library's largest setup

enum AnyRoute { ANY_DIRECT = 0, ANY_FUSED = 1, ANY_COMPOSED = 2 };

// The owned inner setup has length N (direct) or M.  One setup serves ONE device (bind_device_once).
struct AnySetup : InnerOwner<ANY_MAGIC> {
    static constexpr const char* KIND = "any-length";
    int N = 0;
    int is_real = 0;               // pffft[d]_hip_any_new_real_setup: rows of N reals <-> H = N/2 + 1 complex bins
    AnyRoute route = ANY_DIRECT;   // the default route, fixed at setup
    int M = 0;                     // convolution length; 0 on the direct route
    DeviceBinding bound;
    DevBuf d_chirp;                // w[n], n < N (where the fused kernel is legal: M entries, zero from N on)
    DevBuf d_H;                    // spectrum of the filter b in the inner setup's internal layout (real setups: of b_f, the forward one)
    DevBuf d_Hr;                   // real setups: spectrum of b_r, the backward filter (the index reversal of b_f)
    StreamScratch pad;             // batch x M image of the composed route (real direct route: batch x N canonical spectra): one per
                                   // stream, pad.mu held while a call enqueues
    int bins() const { return is_real ? N / 2 + 1 : N; }
};

// ------------------------------------------------------------------------------------------------ plan
// The fused kernel exists for float and these convolution lengths (M2 = next power of two >= 2N - 1), and it is the default in all of
// them: per vector it moves 2 N 8 bytes in one launch where the composed route moves 2 N 8 + 4 M 8 in three (the pad image written, read
// and rewritten by the convolution, read by the crop).  tests/test_gpu_any.py holds it faster than selector 132 in every cell on the
// device; DESIGN.md §3.12 has the figures.
static bool any_fused_len(int M) { return M == 512 || M == 1024 || M == 2048 || M == 4096; }

// Complex setups: k - n runs over [-(N-1), N-1], so the convolution needs M >= 2N - 1.  Real setups: the bins k < H = N/2 + 1 only, so
// k - n runs over [-(N-1), N/2] and M >= N + N/2 suffices; the fused cells are then N = 172 ... 2731 (M2 = 512 ... 4096).  The composed
// route takes the nearest legal size at or above that (M <= 2^26 for N <= 2^25); a setup that can run fused runs BOTH routes on M2, the
// next power of two: one filter spectrum, one answer to pffft_hip_any_conv_size.
static AnySetup* any_new_setup(int N, int transform, int is_double, int is_real) {
    if (transform != (is_real ? PFFFT_REAL : PFFFT_COMPLEX) || N < 1 || N > ANY_MAX_N) return nullptr;
    std::unique_ptr<AnySetup> a(new AnySetup);
    a->N = N; a->is_real = is_real;
    int len = N;
    if (pffft_is_valid_size(N, (pffft_transform_t)transform)) {
        a->route = ANY_DIRECT;
    } else {
        const long long need = is_real ? (long long)N + N / 2 : 2ll * N - 1;
        long long p2 = 16;
        while (p2 < need) p2 *= 2;
        const bool fused = !is_double && any_fused_len((int)p2);
        a->M = len = fused ? (int)p2 : pffft_nearest_transform_size((int)need, PFFFT_COMPLEX, 1);
        a->route = fused ? ANY_FUSED : ANY_COMPOSED;
        transform = PFFFT_COMPLEX;
    }
    return a->new_inner(len, transform, is_double) ? a.release() : nullptr;
}

// the route of a call under the calling thread's selector
static AnyRoute any_route_now(const AnySetup* a, const AbSel& sel) {
    if (a->route == ANY_FUSED && sel.is(AB_ANY_COMPOSED)) return ANY_COMPOSED;
    return a->route;   // (AB_ANY_FUSED: every legal cell is fused by default today - the selector pins that against a later cell list)
}

// ------------------------------------------------------------------------------------------------ tables
// w[n] = exp(-j pi (n^2 mod 2N) / N): the reduction in 64-bit integers (n < 2^25: n^2 < 2^50), the angle in extended precision, rounded once
template <typename T>
static cx<T> chirp_value(unsigned long long n, unsigned long long N) {
    const unsigned long long r = (n * n) % (2 * N);
    const long double a = -3.14159265358979323846264338327950288L * (long double)r / (long double)N;
    cx<T> w;
    w.x = (T)cosl(a); w.y = (T)sinl(a);
    return w;
}

// the spectrum of one filter b (M values, double whatever the setup's type) in the inner setup's internal layout, into `dst`
// (bluestein_host.h: shared with the zoom transforms)
template <typename T>
static int any_filter_spectrum(AnySetup* a, std::vector<cx<double>>& b, DevBuf& dst) {
    return bluestein_filter_spectrum<T>(a->inner, (size_t)a->M, b, dst);
}

// b[m] = conj(w[|m|]) for -(neg - 1) <= m <= pos - 1 (negative m at M + m), zero elsewhere
static std::vector<cx<double>> any_filter(size_t N, size_t M, size_t pos, size_t neg) {
    std::vector<cx<double>> b(M);
    for (size_t m = 0; m < M; ++m) b[m] = mk<double>(0, 0);
    for (size_t m = 0; m < std::max(pos, neg); ++m) {
        const cx<double> c = chirp_value<double>(m, N);
        if (m < pos) b[m] = mk<double>(c.x, -c.y);
        if (m && m < neg) b[M - m] = mk<double>(c.x, -c.y);
    }
    return b;
}

template <typename T>
static int any_build_tables(AnySetup* a) {
    const size_t N = (size_t)a->N, M = (size_t)a->M;
    std::vector<cx<T>> w(a->route == ANY_FUSED ? M : N);
    for (size_t n = 0; n < N; ++n) w[n] = chirp_value<T>(n, N);
    for (size_t n = N; n < w.size(); ++n) w[n] = mk<T>(0, 0);
    int rc = upload_table(a->d_chirp, w);
    if (rc) return rc;
    if (!a->is_real) {
        // b[m] = conj(w[m]), m < N; b[M - m] = b[m]; zero elsewhere - in double whatever the setup's type
        std::vector<cx<double>> b = any_filter(N, M, N, N);
        return any_filter_spectrum<T>(a, b, a->d_H);
    }
    // real: b_f on [-(N-1), H-1], b_r on [-(H-1), N-1]
    const size_t H = (size_t)a->bins();
    std::vector<cx<double>> b = any_filter(N, M, H, N);
    if ((rc = any_filter_spectrum<T>(a, b, a->d_H))) return rc;
    b = any_filter(N, M, N, H);
    return any_filter_spectrum<T>(a, b, a->d_Hr);
}

template <typename T>
static int any_ensure(AnySetup* a, hipStream_t st) {
    return bind_device_once(a->bound, "any: ", st, [&] { return a->route != ANY_DIRECT ? any_build_tables<T>(a) : 0; });
}

// ------------------------------------------------------------------------------------------------ the two routes (bluestein_host.h)
static int any_fused(AnySetup* a, const float* in, float* out, size_t batch, int cj, hipStream_t st) {
    return bluestein_fused(a->inner, a->M, batch, st, [&](auto tag, size_t b0, size_t nb) {
        typedef typename decltype(tag)::type C;
        const AnyChirpIO<C, AnyHold<C>::value> io{in + b0 * 2 * (size_t)a->N, out + b0 * 2 * (size_t)a->N, a->d_chirp.as<cx<float>>(),
                                                  (unsigned)a->N, cj};
        return bluestein_fused_launch<C>(a->inner, io, (const float*)a->d_H.as<float>(), nb, a->M, st);
    });
}

template <typename T>
static int any_composed(AnySetup* a, const T* in, T* out, size_t batch, int cj, hipStream_t st) {
    const size_t N = (size_t)a->N, M = (size_t)a->M;
    const cx<T>* w = a->d_chirp.as<cx<T>>();
    return bluestein_composed<T>(
        a->inner, a->pad, (const T*)a->d_H.as<T>(), M, batch, st,
        [&](cx<T>* X, size_t v0, size_t cnt) {
            return stream_launch(any_pad_kernel<T>, cnt * M, st, reinterpret_cast<const cx<T>*>(in) + v0 * N, X, w, cnt, N, M, cj);
        },
        [&](cx<T>* X, size_t v0, size_t cnt) {
            return stream_launch(any_crop_kernel<T>, cnt * N, st, (const cx<T>*)X, reinterpret_cast<cx<T>*>(out) + v0 * N, w, cnt, N, M, cj);
        });
}

// ------------------------------------------------------------------------------------------------ real setups
template <int DIRN>
static int any_real_fused(AnySetup* a, const float* in, float* out, size_t batch, hipStream_t st) {
    const size_t rin = DIRN == FWD ? (size_t)a->N : 2 * (size_t)a->bins(), rout = DIRN == FWD ? 2 * (size_t)a->bins() : (size_t)a->N;
    const DevBuf& Hs = DIRN == FWD ? a->d_H : a->d_Hr;
    return bluestein_fused(a->inner, a->M, batch, st, [&](auto tag, size_t b0, size_t nb) {
        typedef typename decltype(tag)::type C;
        const AnyRealIO<C, AnyHold<C>::value, DIRN> io{in + b0 * rin, out + b0 * rout, a->d_chirp.as<cx<float>>(), (unsigned)a->N,
                                                       (unsigned)a->bins()};
        return bluestein_fused_launch<C>(a->inner, io, (const float*)Hs.as<float>(), nb, a->M, st);
    });
}

template <typename T>
static int any_real_composed(AnySetup* a, const T* in, T* out, size_t batch, int back, hipStream_t st) {
    const size_t N = (size_t)a->N, M = (size_t)a->M, H = (size_t)a->bins();
    const size_t rin = back ? 2 * H : N, rout = back ? N : 2 * H;
    const cx<T>* w = a->d_chirp.as<cx<T>>();
    return bluestein_composed<T>(
        a->inner, a->pad, (const T*)(back ? a->d_Hr : a->d_H).template as<T>(), M, batch, st,
        [&](cx<T>* X, size_t v0, size_t cnt) { return stream_launch(any_real_pad_kernel<T>, cnt * M, st, in + v0 * rin, X, w, cnt, N, H, M, back); },
        [&](cx<T>* X, size_t v0, size_t cnt) {
            return stream_launch(any_real_crop_kernel<T>, cnt * (back ? N : H), st, (const cx<T>*)X, out + v0 * rout, w, cnt, N, H, M, back);
        });
}

// direct route: the inner REAL setup's ordered transform, its canonical spectrum (DC, Nyquist, then bins 1 ... N/2 - 1) staged per stream
template <typename T>
static int any_real_direct(AnySetup* a, const T* in, T* out, size_t batch, int back, hipStream_t st) {
    const size_t N = (size_t)a->N, H = (size_t)a->bins();
    return chunked_scratch<T>(a->pad, st, batch, N * sizeof(T), "the scratch image", [&](T* S, size_t v0, size_t cnt) {
        if (!back) {
            if (int rc = transform_batch_any(a->inner, in + v0 * N, S, cnt, PFFFT_FORWARD, 1, st)) return rc;
            return stream_launch(any_real_unpack_kernel<T>, cnt * H, st, (const T*)S, reinterpret_cast<cx<T>*>(out) + v0 * H, cnt, N);
        }
        if (int rc = stream_launch(any_real_pack_kernel<T>, cnt * H, st, reinterpret_cast<const cx<T>*>(in) + v0 * H, S, cnt, N)) return rc;
        return transform_batch_any(a->inner, S, out + v0 * N, cnt, PFFFT_BACKWARD, 1, st);
    });
}

template <typename T>
static int any_real_transform_batch(AnySetup* a, const T* in, T* out, size_t batch, int dir, hipStream_t st) {
    const int back = dir == PFFFT_BACKWARD;
    // (direct: transform_batch's 16- / 32-byte rule; otherwise one scalar on the real side, one complex value on the complex side)
    const uintptr_t ar = a->route == ANY_DIRECT ? 4 * sizeof(T) : sizeof(T), ac = a->route == ANY_DIRECT ? 4 * sizeof(T) : 2 * sizeof(T);
    if (((uintptr_t)in & ((back ? ac : ar) - 1)) || ((uintptr_t)out & ((back ? ar : ac) - 1)))
        return bad(a->route == ANY_DIRECT ? "any: in / out not 16-byte (float) / 32-byte (double) aligned"
                                          : "any: in / out not aligned to one scalar (real rows) / one complex value (spectra)");
    int rc = any_ensure<T>(a, st);
    if (rc || batch == 0) return rc;
    const AnyRoute r = any_route_now(a, ab());
    if (r == ANY_DIRECT) return any_real_direct<T>(a, in, out, batch, back, st);
    if constexpr (sizeof(T) == 4)
        if (r == ANY_FUSED) return back ? any_real_fused<BWD>(a, in, out, batch, st) : any_real_fused<FWD>(a, in, out, batch, st);
    return any_real_composed<T>(a, in, out, batch, back, st);
}

// ------------------------------------------------------------------------------------------------ the entry
template <typename T>
static int any_transform_batch(void* setup, const T* in, T* out, size_t batch, int dir, hipStream_t st) {
    AnySetup* a = typed_handle<AnySetup, T>(setup);
    if (!a) return (int)hipErrorInvalidHandle;
    if (dir != PFFFT_FORWARD && dir != PFFFT_BACKWARD) return bad("any: bad direction");
    if (batch && (!in || !out)) return bad("any: NULL in / out");
    if (a->is_real) return any_real_transform_batch<T>(a, in, out, batch, dir, st);
    // (the direct route is transform_batch: its 16- / 32-byte rule; the other routes access one complex value at a time)
    const uintptr_t align = a->route == ANY_DIRECT ? 4 * sizeof(T) : 2 * sizeof(T);
    if (((uintptr_t)in | (uintptr_t)out) & (align - 1))
        return bad(a->route == ANY_DIRECT ? "any: in / out not 16-byte (float) / 32-byte (double) aligned" : "any: in / out not aligned to one complex value");
    int rc = any_ensure<T>(a, st);
    if (rc || batch == 0) return rc;
    const AnyRoute r = any_route_now(a, ab());
    if (r == ANY_DIRECT) return transform_batch_any(a->inner, in, out, batch, dir, 1, st);
    const int cj = dir == PFFFT_BACKWARD;
    if constexpr (sizeof(T) == 4)
        if (r == ANY_FUSED) return any_fused(a, in, out, batch, cj, st);
    return any_composed<T>(a, in, out, batch, cj, st);
}

}  // namespace pf

PF_EXPORT PFFFT_HIP_AnySetup* pffft_hip_any_new_setup(int N, pffft_transform_t tr) {
    return reinterpret_cast<PFFFT_HIP_AnySetup*>(pf::any_new_setup(N, (int)tr, 0, 0));
}
PF_EXPORT PFFFTD_HIP_AnySetup* pffftd_hip_any_new_setup(int N, pffft_transform_t tr) {
    return reinterpret_cast<PFFFTD_HIP_AnySetup*>(pf::any_new_setup(N, (int)tr, 1, 0));
}
PF_EXPORT PFFFT_HIP_AnySetup* pffft_hip_any_new_real_setup(int N) {
    return reinterpret_cast<PFFFT_HIP_AnySetup*>(pf::any_new_setup(N, PFFFT_REAL, 0, 1));
}
PF_EXPORT PFFFTD_HIP_AnySetup* pffftd_hip_any_new_real_setup(int N) {
    return reinterpret_cast<PFFFTD_HIP_AnySetup*>(pf::any_new_setup(N, PFFFT_REAL, 1, 1));
}
PF_EXPORT void pffft_hip_any_destroy_setup(PFFFT_HIP_AnySetup* s) { pf::destroy_handle<pf::AnySetup>(s); }
PF_EXPORT void pffftd_hip_any_destroy_setup(PFFFTD_HIP_AnySetup* s) { pf::destroy_handle<pf::AnySetup>(s); }
PF_EXPORT int pffft_hip_any_transform_batch(PFFFT_HIP_AnySetup* s, const float* in, float* out, size_t batch, pffft_direction_t d, void* stream) {
    return pf::any_transform_batch<float>(s, in, out, batch, (int)d, (hipStream_t)stream);
}
PF_EXPORT int pffftd_hip_any_transform_batch(PFFFTD_HIP_AnySetup* s, const double* in, double* out, size_t batch, pffft_direction_t d,
                                             void* stream) {
    return pf::any_transform_batch<double>(s, in, out, batch, (int)d, (hipStream_t)stream);
}
PF_EXPORT int pffft_hip_any_conv_size(const void* setup) {
    const pf::AnySetup* a = pf::checked_handle<pf::AnySetup>(setup);
    return a ? a->M : -1;
}
PF_EXPORT int pffft_hip_any_is_real(const void* setup) {
    const pf::AnySetup* a = pf::checked_handle<pf::AnySetup>(setup);
    return a ? a->is_real : -1;
}
PF_EXPORT int pffft_hip_any_bins(const void* setup) {
    const pf::AnySetup* a = pf::checked_handle<pf::AnySetup>(setup);
    return a ? a->bins() : -1;
}
PF_EXPORT const char* pffft_hip_any_route(const void* setup) {
    const pf::AnySetup* a = pf::checked_handle<pf::AnySetup>(setup);
    if (!a) return "";
    switch (pf::any_route_now(a, pf::ab())) {
        case pf::ANY_DIRECT: return "direct";
        case pf::ANY_FUSED: return "fused";
        default: return "composed";
    }
}
PF_EXPORT int pffft_hip_any_chirp(const void* setup, void* host_out) {
    const pf::AnySetup* a = pf::checked_handle<pf::AnySetup>(setup);
    if (!a || !host_out) { pf::g_last_error = "pffft_hip: bad any-length setup handle / NULL output"; return (int)hipErrorInvalidValue; }
    const unsigned long long N = (unsigned long long)a->N;
    if (a->is_double) {
        pf::cx<double>* o = static_cast<pf::cx<double>*>(host_out);
        for (unsigned long long n = 0; n < N; ++n) o[n] = pf::chirp_value<double>(n, N);
    } else {
        pf::cx<float>* o = static_cast<pf::cx<float>*>(host_out);
        for (unsigned long long n = 0; n < N; ++n) o[n] = pf::chirp_value<float>(n, N);
    }
    return 0;
}
