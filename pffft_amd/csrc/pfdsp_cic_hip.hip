// libpfdsp_cic_hip.so — the PFDSP carriers (reference: src/pf_carrier.cpp, API include/pffft/pf_carrier.h:72-85) and
// CIC decimating down-converter (src/pf_cic.cpp, include/pffft/pf_cic.h) for MI355X.  ABI: include/pfdsp_cic_hip.h.
//
// A companion of libpfdsp_hip.so (the mixers): the reference builds its PFDSP library from pf_mixer.cpp, pf_carrier.cpp and
// pf_cic.cpp; here the mixers keep their library and exported set, and these 17 entries plus the bank entry live in this one.
// The CIC kernels are in pfdsp_cic.h.  Legacy entries follow the mixers' pointer and failure rules (fail soft: one stderr
// line, NaN-filled output, counted in pfdsp_hip_cic_error_count(); PFFFT_HIP_ABORT=1 aborts).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/pfdsp_cic_hip.h"
#include "pfdsp_cic.h"

#define PD_EXPORT extern "C" __attribute__((visibility("default")))

namespace pdc {

static thread_local std::string g_last_error;

static int fail(hipError_t e, const char* what) {
    char buf[512];
    snprintf(buf, sizeof buf, "pfdsp_cic_hip: %s failed: %s (%d)", what, hipGetErrorString(e), (int)e);
    g_last_error = buf;
    return (int)e;
}
#define PD_CHECK(expr)                                   \
    do {                                                 \
        hipError_t _e = (expr);                          \
        if (_e != hipSuccess) return fail(_e, #expr);    \
    } while (0)

static bool is_device_ptr(const void* p) {
    if (!p) return false;
    hipPointerAttribute_t attr;
    hipError_t e = hipPointerGetAttributes(&attr, p);
    if (e != hipSuccess) { (void)hipGetLastError(); return false; }
    return attr.type == hipMemoryTypeDevice || attr.type == hipMemoryTypeManaged;
}

// the legacy entries cannot fail in the reference: here they fail soft (the first 8 per process on stderr)
static std::atomic<unsigned> g_error_count{0};
static void legacy_fatal(int code, const char* entry, void* out, size_t bytes) {
    static const bool fail_fast = [] { const char* e = getenv("PFFFT_HIP_ABORT"); return e && e[0] == '1'; }();
    const unsigned nth = g_error_count.fetch_add(1);
    if (nth < 8 || fail_fast)
        fprintf(stderr, "%s: HIP path failed (%d): %s%s\n", entry, code, g_last_error.c_str(),
                fail_fast ? "" : " -- output filled with NaN (PFFFT_HIP_ABORT=1 aborts instead)");
    if (fail_fast) abort();
    if (out && bytes) {
        if (!is_device_ptr(out)) memset(out, 0xFF, bytes);
        else if (hipMemset(out, 0xFF, bytes) != hipSuccess) (void)hipGetLastError();
    }
}

// ------------------------------------------------------------------------------------------------
// CIC down-converter (src/pf_cic.cpp) and carriers (src/pf_carrier.cpp): kernels in pfdsp_cic.h
// ------------------------------------------------------------------------------------------------
// The state block is private to the library (the reference's is too): factor, gain and the packed table on the host;
// the integrators, combs, phase and partial records in device memory, bound at the first call to that call's device.
struct CicHost {
    int factor;
    float gain;
    int device;                         // -1 until the first call
    char* dev;                          // pfcic::CIC_DEV_BYTES on `device`
    uint32_t table[pfcic::CIC_TABLE];   // sin | cos << 16, the reference's int16 table (src/pf_cic.cpp:70-75)
};

// freq = rate * ((float)(1ULL << 63) * 2) (src/pf_cic.cpp:95): a float product converted to uint64.  The conversion is
// undefined in C outside [0, 2^64); this is what the reference's x86-64 object does there (include/pfdsp_hip.h).
static uint64_t cic_freq(float rate) {
    const float p = rate * ((float)(1ULL << 63) * 2);
    const float two63 = (float)(1ULL << 63);
    if (p >= 2 * two63) return 0;                                           // rate >= 1
    if (p >= two63) return (uint64_t)(int64_t)(p - two63) ^ (1ULL << 63);   // [0.5, 1)
    if (p >= -two63) return (uint64_t)(int64_t)p;                           // [-0.5, 0.5): two's complement
    return 1ULL << 63;                                                      // below -0.5 (and NaN)
}

static int cic_sample_bytes(int fmt) { return fmt == pfcic::FMT_CS16 ? 4 : 2; }

static int g_cic_cus[64];
static int cic_cus(int dev) {
    if (dev < 0 || dev >= 64) return 256;
    if (!g_cic_cus[dev]) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
            (void)hipGetLastError();
            n = 256;
        }
        g_cic_cus[dev] = n;
    }
    return g_cic_cus[dev];
}

static std::mutex g_cic_bind_mu;
// binds the state to the calling thread's current device at its first call: zeroed state, table uploaded
static int cic_bind(CicHost* s) {
    int d = 0;
    PD_CHECK(hipGetDevice(&d));
    std::lock_guard<std::mutex> lk(g_cic_bind_mu);
    if (s->dev) {
        if (s->device != d) {
            g_last_error = "pfdsp_hip: CIC state is bound to device " + std::to_string(s->device) + ", called on device " +
                           std::to_string(d);
            return (int)hipErrorInvalidDevice;
        }
        return 0;
    }
    void* p = nullptr;
    PD_CHECK(hipMalloc(&p, pfcic::CIC_DEV_BYTES));
    hipError_t e = hipMemset(p, 0, pfcic::CIC_TABLE_OFF);
    if (e == hipSuccess) e = hipMemcpy((char*)p + pfcic::CIC_TABLE_OFF, s->table, sizeof s->table, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        (void)hipFree(p);
        return fail(e, "CIC state allocation");
    }
    s->dev = (char*)p;
    s->device = d;
    return 0;
}

// main kernel + finisher for up to CIC_MAXCH channels of one factor over one device input
static int cic_launch(CicHost* const* st, const uint64_t* freq, int nch, int fmt, const void* d_in, size_t K, float2* d_out,
                      size_t out_stride, hipStream_t stream) {
    const int R = st[0]->factor;
    int nseg = 1;
    while (nseg < 64 && (size_t)nseg * pfcic::CIC_TCH < (size_t)R) nseg <<= 1;   // <= 16 samples per lane up to R = 1024
    const size_t bpp = pfcic::CIC_THREADS / nseg;
    size_t nwg = (K + bpp - 1) / bpp;
    // three workgroups fit a CU (52 KiB of LDS): one round of them; every workgroup keeps >= 2 blocks (cic_finish_kernel)
    nwg = std::min(nwg, (size_t)std::min(pfcic::CIC_MAXWG, 3 * cic_cus(st[0]->device)));
    nwg = std::max<size_t>(1, std::min(nwg, K / 2));
    for (int c0 = 0; c0 < nch; c0 += pfcic::CIC_MAXCH) {
        pfcic::CicArgs a;
        memset(&a, 0, sizeof a);
        a.in = d_in; a.K = K; a.R = R; a.nseg = nseg; a.nwg = (int)nwg;
        a.nch = std::min(pfcic::CIC_MAXCH, nch - c0);
        a.gain = st[0]->gain;
        for (int c = 0; c < a.nch; ++c) {
            a.ch[c].dev = st[c0 + c]->dev;
            a.ch[c].freq = freq[c0 + c];
            a.ch[c].out = d_out + (size_t)(c0 + c) * out_stride;
        }
        if (fmt == pfcic::FMT_S16)
            hipLaunchKernelGGL(pfcic::cic_main_kernel<pfcic::FMT_S16>, dim3((unsigned)nwg), dim3(pfcic::CIC_THREADS), 0, stream, a);
        else if (fmt == pfcic::FMT_CS16)
            hipLaunchKernelGGL(pfcic::cic_main_kernel<pfcic::FMT_CS16>, dim3((unsigned)nwg), dim3(pfcic::CIC_THREADS), 0, stream, a);
        else
            hipLaunchKernelGGL(pfcic::cic_main_kernel<pfcic::FMT_CU8>, dim3((unsigned)nwg), dim3(pfcic::CIC_THREADS), 0, stream, a);
        PD_CHECK(hipGetLastError());
        hipLaunchKernelGGL(pfcic::cic_finish_kernel, dim3((unsigned)a.nch), dim3(pfcic::CIC_THREADS), 0, stream, a);
        PD_CHECK(hipGetLastError());
    }
    return 0;
}

// legacy entries: host pointers staged through grow-only device buffers (input and output differ in type and length),
// null stream, return after synchronising
static std::mutex g_cic_stage_mu;
static void* g_cic_in = nullptr;
static size_t g_cic_in_bytes = 0;
static void* g_cic_out = nullptr;
static size_t g_cic_out_bytes = 0;

static int grow(void*& buf, size_t& have, size_t need) {
    if (have >= need) return 0;
    if (buf) (void)hipFree(buf);
    buf = nullptr; have = 0;
    PD_CHECK(hipMalloc(&buf, need));
    have = need;
    return 0;
}

static int cic_legacy(CicHost* s, int fmt, const void* in, complexf* out, size_t K, float rate) {
    int rc = cic_bind(s);
    if (rc) return rc;
    const uint64_t freq = cic_freq(rate);
    const size_t in_bytes = K * (size_t)s->factor * cic_sample_bytes(fmt), out_bytes = K * sizeof(complexf);
    const bool in_dev = is_device_ptr(in), out_dev = is_device_ptr(out);
    std::unique_lock<std::mutex> lk(g_cic_stage_mu, std::defer_lock);
    const void* d_in = in;
    float2* d_out = reinterpret_cast<float2*>(out);
    if (!in_dev || !out_dev) lk.lock();
    if (!in_dev) {
        if ((rc = grow(g_cic_in, g_cic_in_bytes, in_bytes))) return rc;
        PD_CHECK(hipMemcpy(g_cic_in, in, in_bytes, hipMemcpyHostToDevice));
        d_in = g_cic_in;
    }
    if (!out_dev) {
        if ((rc = grow(g_cic_out, g_cic_out_bytes, out_bytes))) return rc;
        d_out = reinterpret_cast<float2*>(g_cic_out);
    }
    if ((rc = cic_launch(&s, &freq, 1, fmt, d_in, K, d_out, K, nullptr))) return rc;
    if (!out_dev) PD_CHECK(hipMemcpy(out, d_out, out_bytes, hipMemcpyDeviceToHost));
    else PD_CHECK(hipStreamSynchronize(nullptr));
    return 0;
}

static void cic_or_die(const char* entry, void* state, int fmt, const void* in, complexf* out, int outsize, float rate) {
    if (!state || outsize <= 0) return;   // cicddc_init returns NULL for factor < 1
    int rc = cic_legacy(static_cast<CicHost*>(state), fmt, in, out, (size_t)outsize, rate);
    if (rc) legacy_fatal(rc, entry, out, (size_t)outsize * sizeof(complexf));
}

// carriers: four complex samples repeated; `size` samples written, a size that is not a multiple of 4 truncates the pattern
template <typename S>
static void carrier(const char* entry, S* out, int size, const S (&pat)[8]) {
    if (!out || size <= 0) return;
    const size_t n = 2 * (size_t)size;
    if (!is_device_ptr(out)) {
        for (size_t i = 0; i < n; ++i) out[i] = pat[i & 7];
        return;
    }
    const unsigned blocks = (unsigned)std::min<size_t>((n + pfcic::CIC_THREADS - 1) / pfcic::CIC_THREADS, 4096);
    hipLaunchKernelGGL(pfcic::carrier_fill_kernel<S>, dim3(blocks), dim3(pfcic::CIC_THREADS), 0, nullptr, out, (unsigned long long)n,
                       pat[0], pat[1], pat[2], pat[3], pat[4], pat[5], pat[6], pat[7]);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) {
        fail(e, "carrier fill kernel");
        legacy_fatal((int)e, entry, out, n * sizeof(S));
    }
}

}  // namespace pdc

using namespace pdc;

// ---- CIC down-converter (src/pf_cic.cpp) ----
PD_EXPORT void* cicddc_init(int factor) {   // :60-77
    if (factor < 1) return nullptr;          // the reference divides by zero in its gain
    CicHost* s = new (std::nothrow) CicHost;
    if (!s) return nullptr;
    s->factor = factor;
    s->gain = 1.0f / SHRT_MAX / 32767.0f / factor / factor / factor;
    s->device = -1;
    s->dev = nullptr;
    int16_t t[pfcic::CIC_TABLE * 5 / 4];
    const double f = 2.0 * M_PI / (double)pfcic::CIC_TABLE;
    for (int i = 0; i < pfcic::CIC_TABLE * 5 / 4; ++i) t[i] = (int16_t)(32767.0f * cos(f * i));
    for (int i = 0; i < pfcic::CIC_TABLE; ++i) s->table[i] = (uint16_t)t[i] | (uint32_t)(uint16_t)t[i + pfcic::CIC_TABLE / 4] << 16;
    return s;
}
PD_EXPORT void cicddc_free(void* state) {
    CicHost* s = static_cast<CicHost*>(state);
    if (!s) return;
    if (s->dev && hipFree(s->dev) != hipSuccess) (void)hipGetLastError();
    delete s;
}
PD_EXPORT void cicddc_s16_c(void* state, int16_t* input, complexf* output, int outsize, float rate) {
    cic_or_die("cicddc_s16_c", state, pfcic::FMT_S16, input, output, outsize, rate);
}
PD_EXPORT void cicddc_cs16_c(void* state, int16_t* input, complexf* output, int outsize, float rate) {
    cic_or_die("cicddc_cs16_c", state, pfcic::FMT_CS16, input, output, outsize, rate);
}
PD_EXPORT void cicddc_cu8_c(void* state, uint8_t* input, complexf* output, int outsize, float rate) {
    cic_or_die("cicddc_cu8_c", state, pfcic::FMT_CU8, input, output, outsize, rate);
}

// ---- carriers (src/pf_carrier.cpp) ----
static constexpr float CA = 127.0F / 128.0F;
static constexpr short CM = SHRT_MAX, CH = SHRT_MAX / 2;
PD_EXPORT void generate_dc_f(float* o, int n) { carrier<float>("generate_dc_f", o, n, {CA, 0, CA, 0, CA, 0, CA, 0}); }
PD_EXPORT void generate_dc_s16(short* o, int n) { carrier<short>("generate_dc_s16", o, n, {CM, 0, CM, 0, CM, 0, CM, 0}); }
PD_EXPORT void generate_pos_fs4_f(float* o, int n) { carrier<float>("generate_pos_fs4_f", o, n, {CA, 0, 0, CA, -CA, 0, 0, -CA}); }
PD_EXPORT void generate_pos_fs4_s16(short* o, int n) { carrier<short>("generate_pos_fs4_s16", o, n, {CM, 0, 0, CM, -CM, 0, 0, -CM}); }
PD_EXPORT void generate_neg_fs4_f(float* o, int n) { carrier<float>("generate_neg_fs4_f", o, n, {CA, 0, 0, -CA, -CA, 0, 0, CA}); }
PD_EXPORT void generate_neg_fs4_s16(short* o, int n) { carrier<short>("generate_neg_fs4_s16", o, n, {CM, 0, 0, -CM, -CM, 0, 0, CM}); }
PD_EXPORT void generate_dc_pos_fs4_s16(short* o, int n) {
    carrier<short>("generate_dc_pos_fs4_s16", o, n, {2 * CH, 0, CH, CH, 0, 0, CH, -CH});
}
PD_EXPORT void generate_dc_neg_fs4_s16(short* o, int n) {
    carrier<short>("generate_dc_neg_fs4_s16", o, n, {2 * CH, 0, CH, -CH, 0, 0, CH, CH});
}
PD_EXPORT void generate_pos_neg_fs4_s16(short* o, int n) {
    carrier<short>("generate_pos_neg_fs4_s16", o, n, {CH, -CH, -CH, CH, -CH, CH, CH, -CH});
}
PD_EXPORT void generate_dc_pos_neg_fs4_s16(short* o, int n) {
    carrier<short>("generate_dc_pos_neg_fs4_s16", o, n, {2 * CH, -CH, 0, CH, 0, CH, 2 * CH, -CH});
}
PD_EXPORT void generate_pos_neg_fs2_s16(short* o, int n) {
    carrier<short>("generate_pos_neg_fs2_s16", o, n, {CH, 0, -CH, 0, CH, 0, -CH, 0});
}
PD_EXPORT void generate_dc_pos_neg_fs2_s16(short* o, int n) {
    carrier<short>("generate_dc_pos_neg_fs2_s16", o, n, {CH, CH, -CH, CH, CH, CH, -CH, CH});
}

// ---- the bank entry ----
PD_EXPORT int pfdsp_hip_cicddc_device(void* const* states, const float* rates, int nch, int format, const void* d_input,
                                      size_t outsize, complexf* d_output, size_t out_stride, void* stream) {
    auto bad = [](const char* why) { pdc::g_last_error = std::string("pfdsp_hip_cicddc_device: ") + why; return (int)hipErrorInvalidValue; };
    if (!states || !rates || nch < 1) return bad("states, rates and nch >= 1 are required");
    if (format < pfcic::FMT_S16 || format > pfcic::FMT_CU8) return bad("format must be PFDSP_HIP_CIC_S16, _CS16 or _CU8");
    if (out_stride < outsize) return bad("out_stride < outsize");
    if (outsize && (!d_input || !d_output)) return bad("NULL device pointer");
    std::vector<CicHost*> st((size_t)nch);
    std::vector<uint64_t> freq((size_t)nch);
    for (int c = 0; c < nch; ++c) {
        st[c] = static_cast<CicHost*>(states[c]);
        if (!st[c]) return bad("NULL state");
        if (st[c]->factor != st[0]->factor) return bad("states of different factors");
        freq[c] = cic_freq(rates[c]);
    }
    std::vector<CicHost*> sorted(st);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return bad("the same state twice");
    for (int c = 0; c < nch; ++c)
        if (int rc = cic_bind(st[c])) return rc;
    if (!outsize) return 0;   // binds the states: a call with outsize 0 before a stream capture
    return cic_launch(st.data(), freq.data(), nch, format, d_input, outsize, reinterpret_cast<float2*>(d_output), out_stride,
                      (hipStream_t)stream);
}
PD_EXPORT const char* pfdsp_hip_cic_last_error(void) { return pdc::g_last_error.c_str(); }
PD_EXPORT unsigned pfdsp_hip_cic_error_count(void) { return pdc::g_error_count.load(); }
