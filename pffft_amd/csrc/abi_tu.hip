// libpffft_hip.so, translation unit of the C ABI (include/pffft_hip.h; each entry cites the reference line it replaces): the legacy
// single-vector entries with their host-pointer staging and fail-soft layer, the batched entries as thin exports of the typed
// functions of pf_host.h, the multi-device entry and the small getters.  No kernel lives here.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "../../include/pffft_hip.h"
#include "pf_host.h"

namespace pf {

// Legacy void entries have no error channel (include/pffft/pffft.h:159).  A drop-in must not kill its caller where the
// reference could not fail: the default is FAIL-SOFT — one line on stderr (the first 8 failures per process, then every
// 2^k-th: a long-running caller never goes fully silent), the text in pffft_hip_last_error(), the failure counted in
// pffft_hip_error_count(), and the output vector filled with NaN (all-ones bytes; host or device memory alike) so that a
// failed call can never be mistaken for a spectrum.  A call on an INVALID HANDLE (null, destroyed, wrong precision) writes
// nothing: the vector length would have to be read from the very object that failed validation.
// PFFFT_HIP_ABORT=1 restores fail-fast (abort()).
static std::atomic<unsigned> g_error_count{0};
static bool abort_on_error() { return env().abort_on_error; }
void legacy_fatal(int code, const char* entry, void* out, size_t out_bytes, bool out_is_host) {
    const unsigned nth = g_error_count.fetch_add(1);
    const unsigned seq = nth + 1;
    if (nth < 8 || (seq & (seq - 1)) == 0 || abort_on_error())
        fprintf(stderr, "%s: HIP path failed (%d) [failure #%u of this process]: %s%s\n", entry, code, seq, g_last_error.c_str(),
                abort_on_error() ? "" : (out && out_bytes) ? " -- output filled with NaN (PFFFT_HIP_ABORT=1 aborts instead)"
                                                          : " -- output left untouched (PFFFT_HIP_ABORT=1 aborts instead)");
    if (abort_on_error()) abort();
    if (out && out_bytes) {
        if (out_is_host) memset(out, 0xFF, out_bytes);  // all-ones = NaN pattern
        else if (hipMemset(out, 0xFF, out_bytes) != hipSuccess) (void)hipGetLastError();
    }
}

// ------------------------------------------------------------------------------------------------
// legacy single-vector entries: host pointers are staged, device pointers are used in place
// ------------------------------------------------------------------------------------------------
bool is_device_ptr(const void* p) {
    hipPointerAttribute_t attr;
    hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) { (void)hipGetLastError(); return false; }
    return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

// Host-pointer calls on small vectors: no DMA copies at all.  The vector is copied (CPU memcpy, < 1 us) into a pinned host
// image that the kernel reads over PCIe directly, the kernel writes its result into another pinned image, one stream
// synchronisation, CPU memcpy out: one launch + one sync per call instead of two synchronous hipMemcpy around them
// (measured: tools/legacy_bench.py).  Vectors above ZC_LIMIT keep the device staging (kernels there may sweep `out`
// more than once).  PFFFT_HIP_NO_ZEROCOPY=1 switches it off (A/B).
constexpr size_t ZC_LIMIT = 256 * 1024;
bool zero_copy_enabled() { return env().zero_copy; }

// run `fn(d_in..., d_out)` with up to 3 inputs + 1 output vector of `bytes` bytes each
template <typename T, typename F>
static int legacy_run(Setup* s, const T* const* ins, int nin, T* out, bool out_is_inout, F&& fn) {
    if (int rc = check_setup<T>(s)) return rc;
    s = for_device(s);        // (the staging buffers of the calling thread's device)
    const size_t bytes = s->vec_scalars * sizeof(T);
    // the staging buffers belong to the setup; the mutex keeps concurrent callers correct
    // (the reference allows a setup to be shared between threads, include/pffft/pffft.h:102-105)
    std::lock_guard<std::mutex> lk(s->stage_mu);
    if (bytes <= ZC_LIMIT && zero_copy_enabled() && s->kernel != K_BIG) {
        bool any_dev = is_device_ptr(out);
        for (int i = 0; i < nin && !any_dev; ++i) any_dev = is_device_ptr(ins[i]);
        // the pinned images are allocated up front; if the host cannot pin memory the device staging below still works
        bool pinned_ok = !any_dev;
        for (int k = 0; k <= nin && pinned_ok; ++k) pinned_ok = s->h_stage[k].grow(bytes) == 0;
        if (!any_dev && pinned_ok) {
            const T* h_in[3] = {nullptr, nullptr, nullptr};
            T* h_out = s->h_stage[0].as<T>();
            bool out_loaded = false;
            if (out_is_inout) { memcpy(h_out, out, bytes); out_loaded = true; }
            int slot = 1;
            for (int i = 0; i < nin; ++i) {
                if (ins[i] == out) { if (!out_loaded) { memcpy(h_out, out, bytes); out_loaded = true; } h_in[i] = h_out; continue; }
                bool dup = false;
                for (int j = 0; j < i; ++j) if (ins[j] == ins[i]) { h_in[i] = h_in[j]; dup = true; break; }
                if (dup) continue;
                void* p = s->h_stage[slot++].get();
                memcpy(p, ins[i], bytes);
                h_in[i] = (const T*)p;
            }
            int rc = fn(h_in, h_out);
            if (rc) return rc;
            PF_CHECK(hipStreamSynchronize(nullptr));
            memcpy(out, h_out, bytes);
            return 0;
        }
    }
    const T* d_in[3] = {nullptr, nullptr, nullptr};
    T* d_out = nullptr;
    const bool out_dev = is_device_ptr(out);
    int slot = 0;
    if (out_dev) d_out = out;
    else {
        int rc = s->d_stage[slot].grow(bytes); if (rc) return rc;
        d_out = s->d_stage[slot++].as<T>();
        if (out_is_inout) PF_CHECK(hipMemcpy(d_out, out, bytes, hipMemcpyHostToDevice));
    }
    for (int i = 0; i < nin; ++i) {
        if (ins[i] == out) { d_in[i] = d_out; if (!out_dev && !out_is_inout) PF_CHECK(hipMemcpy(d_out, out, bytes, hipMemcpyHostToDevice)); continue; }
        bool dup = false;
        for (int j = 0; j < i; ++j) if (ins[j] == ins[i]) { d_in[i] = d_in[j]; dup = true; break; }
        if (dup) continue;
        if (is_device_ptr(ins[i])) d_in[i] = ins[i];
        else {
            int rc = s->d_stage[slot].grow(bytes); if (rc) return rc;
            void* p = s->d_stage[slot++].get();
            PF_CHECK(hipMemcpy(p, ins[i], bytes, hipMemcpyHostToDevice));
            d_in[i] = (const T*)p;
        }
    }
    int rc = fn(d_in, d_out);
    if (rc) return rc;
    if (!out_dev) PF_CHECK(hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost));
    else PF_CHECK(hipStreamSynchronize(nullptr));
    return 0;
}

// bytes of the caller's output vector the fail-soft path may overwrite: none unless the handle itself is valid
template <typename T>
static size_t legacy_out_bytes(const Setup* s) {
    return (s && s->magic == MAGIC && s->is_double == (sizeof(T) == 8)) ? s->vec_scalars * sizeof(T) : 0;
}

template <typename T>
static void legacy_transform(Setup* s, const T* in, T* out, int dir, int ordered, const char* name) {
    const T* ins[1] = {in};
    int rc = legacy_run<T>(s, ins, 1, out, false, [&](const T* const* di, T* dout) {
        return transform_batch<T>(s, di[0], dout, 1, dir, ordered, nullptr);
    });
    if (rc) legacy_fatal(rc, name, out, legacy_out_bytes<T>(s), !is_device_ptr(out));
}

template <typename T>
static void legacy_zreorder(Setup* s, const T* in, T* out, int dir, const char* name) {
    const T* ins[1] = {in};
    int rc = legacy_run<T>(s, ins, 1, out, false, [&](const T* const* di, T* dout) {
        return zreorder_batch<T>(s, di[0], dout, 1, dir, nullptr);
    });
    if (rc) legacy_fatal(rc, name, out, legacy_out_bytes<T>(s), !is_device_ptr(out));
}

template <typename T>
static void legacy_zconvolve(Setup* s, const T* a, const T* b, T* ab, T scaling, int accumulate, const char* name) {
    const T* ins[2] = {a, b};
    int rc = legacy_run<T>(s, ins, 2, ab, accumulate != 0, [&](const T* const* di, T* dout) {
        return zconvolve_batch<T>(s, di[0], di[1], dout, scaling, 1, accumulate, 0, nullptr);
    });
    if (rc) legacy_fatal(rc, name, ab, legacy_out_bytes<T>(s), !is_device_ptr(ab));
}

}  // namespace pf

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
#define PF_DEFINE_API(PFX, SETUP, T, ISD, ARCHSTR)                                                                  \
    PF_EXPORT SETUP* PFX##_new_setup(int N, pffft_transform_t tr) {                                                 \
        return static_cast<SETUP*>(pf::new_setup(N, (int)tr, ISD));                                                 \
    }                                                                                                               \
    PF_EXPORT void PFX##_destroy_setup(SETUP* s) { pf::destroy_setup(s); }                                          \
    PF_EXPORT void PFX##_transform(SETUP* s, const T* in, T* out, T* work, pffft_direction_t d) {                   \
        (void)work; pf::legacy_transform<T>(s, in, out, (int)d, 0, #PFX "_transform");                              \
    }                                                                                                               \
    PF_EXPORT void PFX##_transform_ordered(SETUP* s, const T* in, T* out, T* work, pffft_direction_t d) {           \
        (void)work; pf::legacy_transform<T>(s, in, out, (int)d, 1, #PFX "_transform_ordered");                      \
    }                                                                                                               \
    PF_EXPORT void PFX##_zreorder(SETUP* s, const T* in, T* out, pffft_direction_t d) {                             \
        pf::legacy_zreorder<T>(s, in, out, (int)d, #PFX "_zreorder");                                               \
    }                                                                                                               \
    PF_EXPORT void PFX##_zconvolve_accumulate(SETUP* s, const T* a, const T* b, T* ab, T sc) {                      \
        pf::legacy_zconvolve<T>(s, a, b, ab, sc, 1, #PFX "_zconvolve_accumulate");                                  \
    }                                                                                                               \
    PF_EXPORT void PFX##_zconvolve_no_accu(SETUP* s, const T* a, const T* b, T* ab, T sc) {                         \
        pf::legacy_zconvolve<T>(s, a, b, ab, sc, 0, #PFX "_zconvolve_no_accu");                                     \
    }                                                                                                               \
    PF_EXPORT int PFX##_simd_size(void) { return pf::SIMD; }                                                        \
    PF_EXPORT const char* PFX##_simd_arch(void) { return ARCHSTR; }                                                 \
    PF_EXPORT int PFX##_min_fft_size(pffft_transform_t tr) { return pf::min_fft_size((int)tr); }                    \
    PF_EXPORT int PFX##_is_valid_size(int N, pffft_transform_t tr) { return pf::is_valid_size(N, (int)tr); }        \
    PF_EXPORT int PFX##_nearest_transform_size(int N, pffft_transform_t tr, int higher) {                           \
        return pf::nearest_size(N, (int)tr, higher);                                                                \
    }                                                                                                               \
    PF_EXPORT int PFX##_next_power_of_two(int N) { return pf::next_pow2(N); }                                       \
    PF_EXPORT int PFX##_is_power_of_two(int N) { return pf::is_pow2(N); }                                           \
    PF_EXPORT void* PFX##_aligned_malloc(size_t nb) { return pf::aligned_malloc64(nb); }                            \
    PF_EXPORT void PFX##_aligned_free(void* p) { pf::aligned_free64(p); }                                           \
    PF_EXPORT int validate_##PFX##_simd_ex(void* dbg) { return pf::validate_layout((FILE*)dbg); }                   \
    PF_EXPORT int validate_##PFX##_simd(void) { return pf::validate_layout(nullptr); }                              \
    PF_EXPORT int PFX##_hip_transform_batch(SETUP* s, const T* in, T* out, size_t batch, pffft_direction_t d,       \
                                            int ordered, void* stream) {                                            \
        return pf::transform_batch<T>(s, in, out, batch, (int)d, ordered, (hipStream_t)stream);                     \
    }                                                                                                               \
    PF_EXPORT int PFX##_hip_zreorder_batch(SETUP* s, const T* in, T* out, size_t batch, pffft_direction_t d,        \
                                           void* stream) {                                                          \
        return pf::zreorder_batch<T>(s, in, out, batch, (int)d, (hipStream_t)stream);                               \
    }                                                                                                               \
    PF_EXPORT int PFX##_hip_zconvolve_batch(SETUP* s, const T* a, const T* b, T* ab, T sc, size_t batch,            \
                                            int accumulate, int b_broadcast, void* stream) {                        \
        return pf::zconvolve_batch<T>(s, a, b, ab, sc, batch, accumulate, b_broadcast, (hipStream_t)stream);        \
    }                                                                                                               \
    PF_EXPORT int PFX##_hip_convolve_batch(SETUP* s, const T* in, const T* H, T* out, T sc, size_t batch,           \
                                           int accumulate, int h_broadcast, void* stream) {                         \
        return pf::convolve_batch<T>(s, in, H, out, sc, batch, accumulate, h_broadcast, (hipStream_t)stream);       \
    }

// Batch shards over several devices from ONE host thread (independent units, no exchange step): part p is transformed by
// setups[p] on devices[p] - hipSetDevice, then the batched entry on streams[p] (NULL: that device's default stream); every launch is
// asynchronous, so the devices run concurrently.  The caller's current device is restored.  Round 6: setups[p] may be the SAME setup in
// every slot (for_device: a setup holds device state per device it is used on) or a setup of its own per part, as before.  Returns the
// first error (0 = all enqueued).
template <typename T, typename SETUP>
static int transform_batch_multi(int nparts, const int* devices, SETUP* const* setups, const T* const* in, T* const* out, const size_t* batches,
                                 int dir, int ordered, void* const* streams) {
    if (nparts < 0 || (nparts > 0 && (!devices || !setups || !in || !out || !batches))) {
        pf::g_last_error = "pffft_hip: transform_batch_multi needs devices, setups, in, out and batches";
        return (int)hipErrorInvalidValue;
    }
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); prev = -1; }
    int rc = 0;
    for (int p = 0; p < nparts && !rc; ++p) {
        hipError_t e = hipSetDevice(devices[p]);
        if (e != hipSuccess) { (void)hipGetLastError(); rc = pf::fail(e, "hipSetDevice"); break; }   // (the runtime's sticky error is consumed here: the next launch checks it)
        rc = pf::transform_batch<T>(setups[p], in[p], out[p], batches[p], dir, ordered, (hipStream_t)(streams ? streams[p] : nullptr));
    }
    if (prev >= 0) (void)hipSetDevice(prev);
    return rc;
}
PF_EXPORT int pffft_hip_transform_batch_multi(int nparts, const int* devices, PFFFT_Setup* const* setups, const float* const* in, float* const* out,
                                              const size_t* batches, pffft_direction_t d, int ordered, void* const* streams) {
    return transform_batch_multi<float, PFFFT_Setup>(nparts, devices, setups, in, out, batches, (int)d, ordered, streams);
}
PF_EXPORT int pffftd_hip_transform_batch_multi(int nparts, const int* devices, PFFFTD_Setup* const* setups, const double* const* in, double* const* out,
                                               const size_t* batches, pffft_direction_t d, int ordered, void* const* streams) {
    return transform_batch_multi<double, PFFFTD_Setup>(nparts, devices, setups, in, out, batches, (int)d, ordered, streams);
}

PF_DEFINE_API(pffft, PFFFT_Setup, float, 0, "HIP-gfx950")
PF_DEFINE_API(pffftd, PFFFTD_Setup, double, 1, "HIP-gfx950")

PF_EXPORT int pffft_hip_shift_transform_batch(PFFFT_Setup* s, const float* in, float* out, size_t batch, int ordered,
                                              double rate, double phase_rad, void* stream) {
    return pf::shift_transform_batch(reinterpret_cast<pf::Setup*>(s), in, out, batch, ordered, rate, phase_rad,
                                     (hipStream_t)stream);
}

PF_EXPORT const char* pffft_hip_kernel_name(const void* setup) {
    const pf::Setup* s = static_cast<const pf::Setup*>(setup);
    if (!s || s->magic != pf::MAGIC) return "invalid";
    return pf::setup_family(s);
}
PF_EXPORT int pffft_hip_describe(const void* setup, char* buf, size_t len) {
    const pf::Setup* s = static_cast<const pf::Setup*>(setup);
    if (!s || s->magic != pf::MAGIC) { if (buf && len) buf[0] = 0; return -1; }
    return pf::describe_setup(s, buf, len);
}
PF_EXPORT int pffft_hip_tile_plan(long long n, int is_double, int deep, int lengths[3]) {
    if (!lengths) return 0;
    return pf::tile_plan_lengths(n, is_double != 0, deep < 0 || deep > 2 ? 1 : deep, lengths);
}
PF_EXPORT int pffft_hip_tile_candidates(long long n, int is_double, int* out, int max) {
    return (out && max > 0) ? pf::tile_plan_candidates(n, is_double != 0, out, max) : 0;
}
PF_EXPORT int pffft_hip_tile_override(long long n, int is_double, int l1, int g1, int l2, int g2) {
    return pf::tile_plan_override(n, is_double != 0, l1, g1, l2, g2);
}
PF_EXPORT const char* pffft_hip_last_error(void) { return pf::g_last_error.c_str(); }
PF_EXPORT unsigned pffft_hip_error_count(void) { return pf::g_error_count.load(); }
// devices the setup holds tables / counters / scratch on right now (the device it bound to first, then its replicas; a key >= 64 is the
// test hook AB_FAKE_DEVICE); fills out[0 .. max), returns the count
PF_EXPORT int pffft_hip_setup_devices(const void* setup, int* out, int max) {
    return pf::setup_devices(const_cast<pf::Setup*>(static_cast<const pf::Setup*>(setup)), out, max < 0 ? 0 : max);
}
PF_EXPORT int pffft_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}
PF_EXPORT void pffft_hip_set_variant(int v) { pf::g_ab_raw = v; }
PF_EXPORT int pffft_hip_has_variants(void) {
#ifdef PFFFT_HIP_VARIANTS
    return 1;
#else
    return 0;
#endif
}
