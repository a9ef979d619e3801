// Host-side declarations shared by the translation units of libpffft_hip.so: the plan ("PFFFT_Setup":
// src/pffft_priv_impl.h:1051-1060), error plumbing and launch helpers, and what each unit offers the others.  The planner is
// plan_tu.hip, the device state and the LDS-resident launchers pffft_hip.hip, the C ABI abi_tu.hip; every kernel family beyond those
// has a *_tu.hip of its own.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include <map>
#include <mutex>
#include <string>

#include "fft_generic.h"
#include "fft_big.h"
#include "stock_plan.h"
#include "pf_route.h"
#include "pf_devmem.h"

namespace pf {

#ifdef PFFFT_HIP_VARIANTS
constexpr bool PF_HAS_VARIANTS = true;
#else
constexpr bool PF_HAS_VARIANTS = false;
#endif

extern thread_local std::string g_last_error;
extern thread_local int g_ab_raw;   // pffft_hip_set_variant(): ab() decodes it (pf_route.h)
int fail(hipError_t e, const char* what);
#define PF_CHECK(expr)                                   \
    do {                                                 \
        hipError_t _e = (expr);                          \
        if (_e != hipSuccess) return fail(_e, #expr);    \
    } while (0)

// a refused argument / state: the text behind pffft_hip_last_error(), the code the entry returns
inline int bad(const char* what, hipError_t e = hipErrorInvalidValue) {
    g_last_error = std::string("pffft_hip: ") + what;
    return (int)e;
}
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the C ABI of include/pffft_hip.h (exports.map lists the names)
#define PF_EXPORT extern "C" __attribute__((visibility("default")))

int num_cus();

// is `st` recording into a HIP graph right now (hipStreamIsCapturing; errors read as "no")
bool stream_capturing(hipStream_t st);

// opt-in to more than 64 KiB of dynamic LDS: once per (kernel, size) - the attribute call sat on every launch
int allow_big_lds_impl(const void* kernel, size_t bytes);
template <typename K>
static int allow_big_lds(K kernel, size_t bytes) {
    if (bytes > 64 * 1024) return allow_big_lds_impl(reinterpret_cast<const void*>(kernel), bytes);
    return 0;
}

// hipOccupancyMaxActiveBlocksPerMultiprocessor is constant per (kernel, threads, LDS bytes): asked once, then served from a table
// (it sat on the launch path of every tile pass and FIR call: pure host latency for the one-vector legacy entries)
int cached_occupancy(const void* kernel, int threads, size_t lds, int* per_cu);

// the class a SIZE is built for: K_STOCK its mixed-radix Stockham plan (fft_stock.h), K_BIG beyond LDS (streaming / tile passes, fft_one.h)
enum Kernel { K_STOCK = 0, K_C1024_F32 = 1, K_TILED = 2, K_BIG = 3 };
constexpr size_t LDS_MAX = 160 * 1024;
constexpr unsigned CTR_RING = 4096;
constexpr unsigned CTR_CAPTURED = 512;   // counter pairs set aside for launches recorded into a HIP graph (take_counters)

struct Setup {
    uint32_t magic;
    int N, transform, is_double;
    int n;           // complex length of the device transform
    size_t vec_scalars;  // scalars per vector: N (real) / 2N (complex)
    Kernel kernel;
    // what runs for [direction][ordered], decided at pffft_new_setup (plan_routes); pffft_hip_describe() prints it
    Route route[2][2];
    // mixed-radix Stockham plans (fft_stock.h): [0] forward order, [1] backward order of the same radices
    StockPlan sk[2], skw[2];          // workgroup-phase plans; wave-local plans (small n)
    int sk_threads = 0, skw_threads = 0;
    bool sk_ok = false, skw_ok = false;
    // single-image plan (fft_one.h, round 6): the sizes that fill LDS once but not twice - [0] forward, [1] backward
    StockPlan one[3];          // [2]: the float complex backward transform from the internal layout (fft_one.h NARROW: no two-trip middle stages)
    bool one_ok = false;
    DevBuf d_one_tw2;          // compact twiddles of one[2]
    // device state (lazy: creating a setup never touches the GPU)
    std::mutex mu;        // guards the lazy device initialisation
    std::mutex stage_mu;  // guards the staging buffers of the legacy host-pointer entries
    bool dev_ready = false;
    // The device the tables / counters / scratch of THIS object live on: bound at first use.  A call from a thread whose current device is
    // another one is served by a replica of the plan with device state of its own (for_device; round 6): one PFFFT_Setup may be shared by
    // threads on different devices like the reference's immutable setup (include/pffft/pffft.h:102-105)
    std::atomic<int> device{-1};
    std::map<int, Setup*> replicas;   // (under mu) device key -> replica; owned, destroyed with the setup
    bool is_replica = false;
    // (every table, scratch and staging buffer below is a DevBuf / PinnedBuf / StreamScratch of pf_devmem.h: freed with the object)
    DevBuf d_tw;      // W_n^j, j < n
    DevBuf d_twr;     // W_N^k, k <= n/2 (real only)
    DevBuf d_twc[2];  // compact per-stage base twiddles of the Stockham plans (forward / backward order)
    DevBuf d_ctr;     // ring of {next, done} work counters for the dynamic kernels (+ the captured region behind it)
    std::atomic<unsigned> ctr_slot{0}, cap_slot{0};
    // sizes beyond LDS with a small factor (fft_big.h, three streaming passes): n = bigR x sub->n
    int bigR = 0;
    Setup* sub = nullptr;
    // sizes beyond LDS (K_BIG): n = bigN[0] x bigN[1], one strided plan + twiddle table per factor
    StridedPlan bigp[2];
    DevBuf d_bigtw[2];
    // HBM work buffers of the beyond-LDS path: one pair per stream, big.mu held while a call enqueues its passes (launch_big)
    StreamScratch big;
    // spectrum image of the composed pffft_hip_convolve_batch route: one per stream, conv.mu held while a call enqueues
    StreamScratch conv;
    // frame matrix of the composed pffft_hip_frames_* routes (frames_tu.hip): one per stream, frames.mu held while a call enqueues
    StreamScratch frames;
    // run partials of pffft_hip_frames_psd_batch for averages longer than one run (psd_tu.hip): one per stream, psd.mu held while a call
    // enqueues (taken BEFORE frames.mu where a call needs both)
    StreamScratch psd;
    DevBuf d_stage[3];     // staging for host-pointer legacy calls
    PinnedBuf h_stage[4];  // pinned host images the kernels read / write directly (small vectors)
};
constexpr uint32_t MAGIC = 0x50464654u;  // "PFFT"

// The {next, done} work-counter pairs of ONE launch of an in-order kernel (`pairs` consecutive pairs: the per-XCD kernels take five).  A
// direct launch takes the next slot of the setup's ring: reused CTR_RING launches later, i.e. at most CTR_RING launches of one setup in
// flight at once (include/pffft_hip.h).  A launch that is being RECORDED INTO A GRAPH freezes its counter address for every replay: it gets
// a slot of a region of its own, outside the ring, so that no later direct launch can share counters with a replay running on another
// stream (tiles skipped or run twice).  CTR_CAPTURED captured launches per setup have private counters; beyond that the region wraps, which
// is safe as long as the launches that share a slot do not run concurrently (nodes of one graph on one stream never do).
struct Setup;
unsigned* take_counters(Setup* s, hipStream_t st, unsigned pairs = 1);

// The object that holds `s`'s device state for the calling thread's CURRENT device: `s` itself on the device it is bound to (or binds to
// now), else the replica of that device, created on first use.  Every entry that takes a setup resolves it first; the launchers that read
// device pointers of a setup (d_tw, counters) are handed the resolved object.  NULL / foreign handles pass through (the entry reports them).
Setup* for_device(Setup* s);
// devices `s` holds state on right now (its own binding first): fills out[0 .. max), returns the count (pffft_hip_setup_devices)
int setup_devices(Setup* s, int* out, int max);

// every entry that takes a setup of the scalar type T checks the handle first
template <typename T>
static int check_setup(const Setup* s) {
    if (!s || s->magic != MAGIC || s->is_double != (sizeof(T) == 8)) {
        g_last_error = "pffft_hip: bad setup handle";
        return (int)hipErrorInvalidHandle;
    }
    return 0;
}

// Buffer 0 of `pool`'s entry for `st` (pool.mu held by the caller), at least `bytes`.  It never grows while the stream records a HIP
// graph: a replay would run on the pointer it froze.  `what` names the buffer in the error text ("the frame matrix").
inline int scratch_buffer(StreamScratch& pool, hipStream_t st, size_t bytes, const char* what, void** buf) {
    StreamScratch::Entry& sc = pool.acquire(st);
    if (sc.buf[0].bytes() < bytes && stream_capturing(st))
        return bad((std::string(what) + " of this stream would have to grow during graph capture: run the call once on this stream before "
                    "capturing").c_str(), hipErrorStreamCaptureUnsupported);
    if (int rc = pool.grow(sc, 0, bytes)) return rc;
    *buf = sc.buf[0].get();
    return 0;
}

// ---- formulas more than one unit uses
constexpr int SIMD = 4;  // the internal layout is the reference's SIMD_SZ == 4 layout (SURVEY.md finding 2)

// radix schedule of the in-place DIF stages (fft_generic.h stage, the strided plans of fft_big.h): 5s, 3s, then 4s, then at most one 2
constexpr int radix_schedule(int n, unsigned char* radix) {
    int ns = 0;
    while (n % 5 == 0) { radix[ns++] = 5; n /= 5; }
    while (n % 3 == 0) { radix[ns++] = 3; n /= 3; }
    while (n % 4 == 0) { radix[ns++] = 4; n /= 4; }
    if (n % 2 == 0) { radix[ns++] = 2; n /= 2; }
    return ns;
}
constexpr bool radix_schedule_is(int n, int ns, int r0, int r1, int r2, int r3) {
    unsigned char r[MAX_STAGES] = {};
    return radix_schedule(n, r) == ns && r[0] == r0 && r[1] == r1 && r[2] == r2 && r[3] == r3;
}
static_assert(radix_schedule_is(240, 4, 5, 3, 4, 4), "240 = 5 x 3 x 4 x 4");
static_assert(radix_schedule_is(32, 3, 4, 4, 2, 0) && radix_schedule_is(1, 0, 0, 0, 0, 0), "one 2 at the end; nothing for 1");

// bytes of an LDS image of `points` elements with one pad element per 32 (fft_generic.h gpad) and two spare
constexpr size_t padded_image_bytes(size_t points, size_t elem_bytes) { return (points + (points >> 5) + 2) * elem_bytes; }
static_assert(padded_image_bytes(2048, 8) == 16912 && padded_image_bytes(20480, 8) == 168976, "n + n / 32 + 2 elements");

// workgroup threads of the strided kernels (fft_big.h): points / 8, rounded up to wavefronts, within 64 .. 1024
constexpr int strided_threads(size_t points) {
    const int th = (int)((points / 8 + 63) / 64 * 64);
    return th < 64 ? 64 : (th > 1024 ? 1024 : th);
}
static_assert(strided_threads(256) == 64 && strided_threads(640) == 128 && strided_threads(4096) == 512 && strided_threads(100000) == 1024, "");

// power-of-two n with a register-tiled kernel (fft_tiled.h): 16 .. 16384 points and at most 128 KiB per vector
constexpr bool is_pow2_tiled(int n, size_t elem_bytes) {
    return (n & (n - 1)) == 0 && n >= 16 && n <= 16384 && (size_t)n * elem_bytes <= 128 * 1024;
}
static_assert(is_pow2_tiled(16384, 8) && !is_pow2_tiled(16384, 16) && is_pow2_tiled(8192, 16), "float to 16384, double to 8192");
static_assert(!is_pow2_tiled(8, 8) && !is_pow2_tiled(48, 8) && is_pow2_tiled(16, 16), "powers of two from 16");

// resident wavefronts per CU of the N = 1024 short-launch kernel: 4 workgroups x C1024_ONCE_W wavefronts (35 KiB of LDS and 84 VGPRs each)
constexpr int C1024_ONCE_W = 4, C1024_ONCE_RESIDENT = 16;

// ---- plan_tu.hip: sizes, setups, routes and their text.  Nothing here launches.
int min_fft_size(int transform);
int is_valid_size(int N, int transform);
int nearest_size(int N, int transform, int higher);
int next_pow2(int N);
int is_pow2(int N);
void* aligned_malloc64(size_t nb);
void aligned_free64(void* p);
Setup* new_setup(int N, int transform, int is_double);
void destroy_setup(Setup* s);
int current_device_key(int* key);   // the key the calling thread's current device goes by (AB_FAKE_DEVICE: a key of its own)
// the route of a (direction, layout) under a selector, planned as new_setup plans the stored ones (transform_batch and describe() under set_variant)
Route plan_route(const Setup* s, int dir, int ordered, const AbSel& sel);
const char* setup_family(const Setup* s);
int describe_setup(const Setup* s, char* buf, size_t len);
int validate_layout(FILE* dbg);

// ---- pffft_hip.hip: the lazy device state, the LDS-resident launchers, the batched transform.  transform_batch / ensure_device are
// instantiated there for float and double; the *_any twins serve the composed units behind type-erased pointers.
template <typename T> int ensure_device(Setup* s, hipStream_t st);
template <typename T> int transform_batch(Setup* s, const T* in, T* out, size_t batch, int dir, int ordered, hipStream_t st);
int transform_batch_any(Setup* s, const void* in, void* out, size_t batch, int dir, int ordered, hipStream_t st);
int ensure_device_any(Setup* s, hipStream_t st);
int shift_transform_batch(Setup* s, const float* in, float* out, size_t batch, int ordered, double rate, double phase_rad, hipStream_t st);
// the measured table of the register-tiled kernels (fft_tiled.h): the one planner input that needs kernel addresses; false: no kernel for n
bool tiled_pick_any(bool is_double, int n, int dir, int real, int ordered, TiledSel* e);

// ---- big_tu.hip: the sweeps of a FAM_BIG route (fft_big.h), as plan_big planned them
int launch_big(Setup* s, const Route& r, const void* in, void* out, size_t batch, int dir, int ordered, hipStream_t st);

// ---- aux_tu.hip: pffft_zreorder / pffft_zconvolve_* / the composed convolution, batched; instantiated there for float and double
template <typename T> int zreorder_batch(Setup* s, const T* in, T* out, size_t batch, int dir, hipStream_t st);
template <typename T> int zconvolve_batch(Setup* s, const T* a, const T* b, T* ab, T scaling, size_t batch, int accumulate, int b_broadcast, hipStream_t st);
template <typename T> int convolve_batch(Setup* s, const T* in, const T* H, T* out, T scaling, size_t batch, int accumulate, int h_broadcast, hipStream_t st);

// ---- abi_tu.hip: what pffastconv_apply shares with the legacy transform entries
void legacy_fatal(int code, const char* entry, void* out, size_t out_bytes, bool out_is_host);
bool is_device_ptr(const void* p);
bool zero_copy_enabled();

struct FcBatch { int nsig; size_t xstride, ystride; };   // signals of one pffastconv call (1 for the reference entries)
// one pffastconv call on the blocks of its route (fastconv_tu.hip fir_route): what every FIR block launcher takes
struct FirCall { const float* x; float* y; int nblk, step, inputLen, lastOut; hipStream_t st; FcBatch fb; };

// dma_tu.hip, on a real setup of Nfft = 2 ps->n and its canonical filter spectrum x 1 / Nfft; a block length the kernel does not have is the
// caller's error (refused with a text), never a fall-through.  hp_cache / ab_cache: the kernel's own table, built on first use into the caller's setup
int launch_fir_dma(Setup* ps, const float* d_Hc, const FirCall& c);                              // the lock-step LDS-DMA staged block kernel (fft_dma.h)
int launch_fir_split(Setup* ps, const float* d_Hc, const FirCall& c, bool plain);                // 16384-sample blocks on the split kernel (fft_split.h)
int launch_fir32(Setup* ps, const float* d_Hc, const FirCall& c, DevBuf& hp_cache, int pref);    // ... on 256 threads with 32 points per thread (fft_fir32.h)
int launch_fir_split1(Setup* ps, const float* d_Hc, const FirCall& c, DevBuf& ab_cache);         // few blocks of 8192 / 4096 samples (fft_split.h fastconv_split1_kernel)

// tile_real_tu.hip: REAL transforms beyond LDS in two sweeps (fft_tile.h RMODE): N real points -> canonical half spectrum through a
// work buffer of tile_rfft_work_elems(N) complex elements per vector; -1: no plan for this length / direction
int launch_tile_rfft(Setup* s, const void* in, void* work, void* out, size_t batch, long long N, int dir, hipStream_t st);
bool tile_rfft_has_plan(long long N, bool is_double, bool adopted = true);   // adopted: only where it measured faster
size_t tile_rfft_work_elems(long long N, bool is_double);

// one_tu.hip: the single-image kernel (fft_one.h) - one HBM pass for the vectors between 80 and 144 KiB that have no two-image Stockham plan
bool one_build(int n, bool is_double, bool real, StockPlan out[2], size_t lds_max, bool narrow = false);
size_t one_lds_bytes(const StockPlan& p, bool is_double, bool real);
int launch_one(Setup* s, const void* in, void* out, size_t batch, int dir, int ordered, hipStream_t st);
const void* one_kernel_ptr(bool is_double, int flags);

// conv_tu.hip: forward -> x H (one filter spectrum, internal layout) -> backward in ONE kernel (fft_conv.h); -1: no fused kernel
int launch_conv_fused(Setup* s, const void* in, const void* H, void* out, size_t batch, double scaling, int accumulate, hipStream_t st);

// tile_tu.hip: power-of-two sizes beyond LDS in two / three passes (fft_tile.h); canonical complex, in -> out through `work`
// (same size, distinct from both; in may equal out).  -1 when the size has no tile plan.  layout 3 (round 6, forward only, the complex core
// of a REAL transform): the last pass carries the pair pass and stores the canonical half-complex spectrum.  layout 1 (forward only): the
// spectrum is stored in the pffft-internal layout by the last pass; layout 2 (backward only): it is read from that layout
// by the first pass.
// (n complex points; -1 = no tile plan for n.  tile_has_plan: the same answer without launching)
// deep: the streaming route of this n would take five sweeps - three tile passes are allowed
int launch_tile_fft(Setup* s, const void* in, void* work, void* out, size_t batch, long long n, int dir, hipStream_t st, int layout = 0, int mode = 0);
bool tile_has_plan(long long n, bool is_double, int mode = 0);
bool tile_real_rows_plan(long long n, bool is_double, int mode);   // layout 3 of launch_tile_fft: real forward, the pair pass inside the last (row) pass   // mode: 0 complex / three streaming sweeps, 1 five (deep), 2 real core / three
int tile_plan_lengths(long long n, bool is_double, int mode, int lengths[3]);
int tile_plan_candidates(long long n, bool is_double, int* out, int max);   // every legal pair {L1, gen1, L2, gen2, model cost}
int tile_plan_override(long long n, bool is_double, int l1, int g1, int l2, int g2);   // the tuner's hook (tools/tune_tile_plans.py)
int tile_plan_layouts(long long n, bool is_double, int mode);   // bit 0: internal layout out of the last pass, bit 1: into the first   // 0 / 2 / 3 passes (pffft_hip_tile_plan)

}  // namespace pf

// the opaque handles of include/pffft_hip.h
struct PFFFT_Setup : pf::Setup {};
struct PFFFTD_Setup : pf::Setup {};
