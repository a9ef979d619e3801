// libpffft_hip.so, translation unit of the planner: what a setup is and what runs for each of its (direction, layout) - sizes, plans,
// routes, their text (pffft_hip_describe) and the per-device replicas.  It launches nothing and instantiates no kernel: the one planner
// input that needs kernel addresses, the register-tiled table, is asked through tiled_pick_any (pffft_hip.hip), the compile-time
// Stockham plans through stock_ct_lookup (stock_ct.h).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/pffft_hip.h"
#include "pf_host.h"
#include "fft_stock.h"
#include "stock_plan.h"
#include "stock_ct.h"
#include "stock_df_gen.h"
#include "stock_grid_gen.h"

namespace pf {

// ------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------
thread_local std::string g_last_error;
thread_local int g_ab_raw = 0;   // pffft_hip_set_variant(): per calling thread
AbSel ab() { AbSel a; a.raw = g_ab_raw; return a; }

// every environment switch of the product build, read once (pf_route.h)
const Env& env() {
    static const Env e = [] {
        auto num = [](const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; };
        Env r;
        r.abort_on_error = num("PFFFT_HIP_ABORT", 0) == 1;
        r.zero_copy = num("PFFFT_HIP_NO_ZEROCOPY", 0) != 1;
        r.oneshot = num("PFFFT_HIP_ONESHOT", 4);
        r.c1024_rounds = num("PFFFT_HIP_C1024_ONCE", 4);
        r.tile_plans = num("PFFFT_HIP_TILE_PLANS", 1);
        r.tile_force = getenv("PFFFT_HIP_TILE_FORCE");
        r.fir_nfft = num("PFFASTCONV_HIP_NFFT", -1);
        r.fir_xcd = num("PFFASTCONV_HIP_XCD", 1);
        if (r.oneshot < 0) r.oneshot = 0;
        if (r.c1024_rounds < 0) r.c1024_rounds = 0;
        return r;
    }();
    return e;
}

int fail(hipError_t e, const char* what) {
    char buf[512];
    snprintf(buf, sizeof buf, "pffft_hip: %s failed: %s (%d)", what, hipGetErrorString(e), (int)e);
    g_last_error = buf;
    return (int)e;
}

// ------------------------------------------------------------------------------------------------
// size helpers — semantics of src/pffft_priv_impl.h:76-116 and src/pffft_common.c:25-43
// ------------------------------------------------------------------------------------------------
int min_fft_size(int transform) {
    if (transform == PFFFT_REAL) return 2 * SIMD * SIMD;
    if (transform == PFFFT_COMPLEX) return SIMD * SIMD;
    return 1;
}
int is_valid_size(int N, int transform) {
    const int nmin = min_fft_size(transform);
    int r = N;
    while (r >= 5 * nmin && r % 5 == 0) r /= 5;
    while (r >= 3 * nmin && r % 3 == 0) r /= 3;
    while (r >= 2 * nmin && r % 2 == 0) r /= 2;
    return r == nmin;
}
int nearest_size(int N, int transform, int higher) {
    const int nmin = min_fft_size(transform);
    if (N < nmin) N = nmin;
    const int d = higher ? nmin : -nmin;
    N = higher ? nmin * ((N + nmin - 1) / nmin) : nmin * (N / nmin);
    for (;; N += d)
        if (is_valid_size(N, transform)) return N;
}
int next_pow2(int N) {
    unsigned v = (unsigned)N;
    v--;
    v |= v >> 1; v |= v >> 2; v |= v >> 4; v |= v >> 8; v |= v >> 16;
    return (int)(v + 1);
}
int is_pow2(int N) { return N && !(N & (N - 1)); }

void* aligned_malloc64(size_t nb) {  // src/pffft_common.c:12-22: 64-byte aligned, raw pointer kept at p[-1]
    void* p0 = malloc(nb + 63 + sizeof(void*));
    if (!p0) return nullptr;
    uintptr_t p = ((uintptr_t)p0 + 63 + sizeof(void*)) & ~(uintptr_t)63;
    ((void**)p)[-1] = p0;
    return (void*)p;
}
void aligned_free64(void* p) {
    if (p) free(((void**)p)[-1]);
}

// ------------------------------------------------------------------------------------------------
// the plan ("PFFFT_Setup": src/pffft_priv_impl.h:1051-1060)
// ------------------------------------------------------------------------------------------------

static void plan_routes(Setup* s);

// does the canonical forward transform of this (sub-)setup run on one of the fast kernels: register-tiled power-of-two
// sizes, or a Stockham plan that exists as a compile-time constant (the run-time-plan twin runs at 0.3)
static bool sub_is_fast(const Setup* q) {
    if (q->kernel == K_TILED || q->kernel == K_C1024_F32) return true;
    if (q->kernel != K_STOCK) return false;
    const int flags = layout_flags(PFFFT_FORWARD, 1, q->transform == PFFFT_REAL);   // forward, canonical layouts (fft_stock.h)
    // (the product build instantiates ONE of the two variants of a plan - deposit or direct first stage, bit 4 -, see
    //  tools/gen_stock_plans.hip: a plan exists when either is there)
    auto has = [&](const StockPlan& p, bool wl) {
        if (q->is_double) return stock_ct_lookup(p, flags, wl, (const double*)nullptr) || stock_ct_lookup(p, flags | 16, wl, (const double*)nullptr);
        return stock_ct_lookup(p, flags, wl, (const float*)nullptr) || stock_ct_lookup(p, flags | 16, wl, (const float*)nullptr);
    };
    return (q->skw_ok && has(q->skw[0], true)) || (q->sk_ok && has(q->sk[0], false));
}

// ---- new_setup, step by step -------------------------------------------------------------------------------------------------
// validation: src/pffft_priv_impl.h:1066-1078 and :1105-1109
static bool setup_args_ok(int N, int transform) {
    if (N <= 0 || N > (1 << 26)) return false;
    if (transform != PFFFT_REAL && transform != PFFFT_COMPLEX) return false;
    const int mult = transform == PFFFT_REAL ? 2 * SIMD * SIMD : SIMD * SIMD;
    if (N % mult) return false;
    // N / SIMD must factor into 2, 3, 5 (what decompose() + the product check enforce)
    int r = N / SIMD;
    for (int f : {2, 3, 5}) while (r % f == 0) r /= f;
    return r == 1;
}

// mixed-radix Stockham plans (fft_stock.h) for every size whose two exchange images fit LDS
static void build_resident_plans(Setup* s) {
    const bool real = s->transform == PFFFT_REAL;
    bool wl = false;
    s->sk_ok = sk_build(s->n, s->is_double != 0, real, s->sk, &s->sk_threads, &wl, false, LDS_MAX);
    s->skw_ok = sk_build(s->n, s->is_double != 0, real, s->skw, &s->skw_threads, &wl, true, LDS_MAX) && wl;
}

// does ONE padded image of the vector (of 2048 / n vectors below 2048 points) fit LDS, 16-byte rounded plus one unit
static bool one_image_fits(const Setup* s, size_t esz) {
    const size_t points = s->n >= 2048 ? (size_t)s->n : (size_t)(2048 / s->n) * s->n;
    return (padded_image_bytes(points, esz) + 15) / 16 * 16 + 16 <= LDS_MAX;
}

// sizes with ONE image in LDS (two do not fit: complex float n = 9600 .. 20480): as R x N2 with the rows on a fast kernel
// the three streaming passes below measure 0.17-0.24
// (the same holds for a size whose Stockham plan fits but has no compile-time twin: the run-time-plan kernel measured 0.07
//  at n = 9600)
static bool is_single_image(const Setup* s, size_t esz) {
    return one_image_fits(s, esz) && !is_pow2_tiled(s->n, esz) && !sub_is_fast(s) && s->n >= 2048;
}

// n = R x N2 with a register-sized R and an N2 the LDS-resident batched kernels take (fft_big.h)
static void choose_streaming_factor(Setup* s, size_t esz, bool single_image) {
    // (the first R whose N2 runs on a fast kernel: N = 20480 as 4 x 5120 put the rows on the run-time-plan Stockham
    //  kernel and measured 0.04 of the roofline, as 32 x 640 it has a compile-time plan)
    // (multiples of 4 first: their column pass can read the internal layout itself, big_col_int_kernel)
    for (int R : {4, 8, 12, 16, 32, 2, 3, 5, 6, 9, 10, 15, 25, 27}) {
        if (s->n % R) continue;
        const int N2 = s->n / R;
        if ((size_t)N2 * esz > 80 * 1024 || N2 % (SIMD * SIMD)) continue;   // (Stockham plans reach n = 10000 float)
        Setup* sub = new_setup(N2, PFFFT_COMPLEX, s->is_double);
        if (!sub) continue;
        if (sub->kernel == K_BIG || (sub->kernel == K_STOCK && !sub->sk_ok)) { destroy_setup(sub); continue; }
        const bool fast = sub_is_fast(sub);
        if (s->sub && !fast) { destroy_setup(sub); continue; }      // keep the first usable one as the fallback
        if (s->sub) destroy_setup(s->sub);
        s->sub = sub; s->bigR = R;
        if (fast) break;
    }
    if (single_image && !(s->sub && sub_is_fast(s->sub))) {
        // no factorisation with fast rows: the balanced two-pass strided plan below (launch_strided) - decided HERE, at setup
        // time (the in-place kernel this branch used to fall back to is gone: such a setup would have been created and then
        // failed on every transform).  No legal size reaches this today (tests/test_generated_sources.py: every size has a
        // compile-time plan); the route exists so that a gap in the generated tables costs speed, not correctness.
        if (s->sub) destroy_setup(s->sub);
        s->sub = nullptr; s->bigR = 0;
    }
    // larger still: peel the largest register-sized factor and recurse (n = R x (R' x N2')): five passes, seven, ...
    if (!s->sub) {
        for (int R : {32, 16, 15, 12, 10, 8, 6, 5, 4, 3, 2}) {
            if (s->n % R) continue;
            const int N2 = s->n / R;
            if (N2 % (SIMD * SIMD)) continue;
            Setup* sub = new_setup(N2, PFFFT_COMPLEX, s->is_double);
            if (!sub) continue;
            if (!(sub->kernel == K_BIG && sub->bigR)) { destroy_setup(sub); continue; }
            s->sub = sub; s->bigR = R;
            break;
        }
    }
}

// four-step plan: split the prime factors of n into two balanced products
static void build_strided_pair(Setup* s, size_t esz) {
    std::vector<int> f;
    int rr = s->n;
    for (int q : {5, 3, 2}) while (rr % q == 0) { f.push_back(q); rr /= q; }
    long long a = 1, b = 1;
    for (int q : f) { if (a <= b) a *= q; else b *= q; }
    const long long sub[2] = {a, b};
    for (int i = 0; i < 2; ++i) {
        StridedPlan& sp = s->bigp[i];
        memset(&sp, 0, sizeof sp);
        sp.n = (int)sub[i];
        sp.nstages = radix_schedule(sp.n, sp.radix);
        long long g = (long long)(92 * 1024) / ((long long)sp.n * (long long)esz);
        sp.G = (int)(g < 1 ? 1 : (g > 32 ? 32 : g));
        sp.vec = s->n;
    }
    // step A: columns (length N1 = sub[0], stride N2), twiddled;  step B: rows (length N2), transposed store
    s->bigp[0].count = sub[1]; s->bigp[0].estride_in = sub[1]; s->bigp[0].tstride_in = 1;
    s->bigp[0].estride_out = sub[1]; s->bigp[0].tstride_out = 1; s->bigp[0].twN = s->n;
    s->bigp[1].count = sub[0]; s->bigp[1].estride_in = 1; s->bigp[1].tstride_in = sub[1];
    s->bigp[1].estride_out = sub[0]; s->bigp[1].tstride_out = 1; s->bigp[1].twN = 0;
}

// ... of those, the vectors that fill LDS once (80-144 KiB): ONE pass on the single-image kernel (fft_one.h, round 6); the plan above stays
// as the route of the helpers (zreorder, zconvolve) and of AB_NO_ONE_IMAGE
static void build_single_image_plans(Setup* s) {
    const bool real = s->transform == PFFFT_REAL;
    s->one_ok = one_build(s->n, s->is_double != 0, real, s->one, LDS_MAX);
    if (s->one_ok) {
        StockPlan narrow[2];
        if (one_build(s->n, s->is_double != 0, real, narrow, LDS_MAX, true)) s->one[2] = narrow[1];
        else s->one_ok = false;
    }
}

// the kernel class of a size that fits LDS twice: the headline kernel, the register-tiled power-of-two kernels (fft_tiled.h), else its
// mixed-radix Stockham plan (fft_stock.h)
static Kernel resident_kernel_class(const Setup* s, size_t esz) {
    if (!s->is_double && s->transform == PFFFT_COMPLEX && s->N == 1024) return K_C1024_F32;
    if (is_pow2_tiled(s->n, esz)) return K_TILED;
    return K_STOCK;
}

// the routes of every (direction, layout); false (with the error text set): the size is refused, as the reference refuses unsupported
// sizes (NULL, src/pffft_priv_impl.h:1105-1109)
static bool plan_or_refuse(Setup* s) {
    if (s->kernel == K_STOCK && !PF_HAS_VARIANTS && !sub_is_fast(s)) {
        // product build: only compile-time Stockham plans exist.  A size without one (none today) must not yield a setup whose
        // every transform fails: refuse it here, where the reference reports unsupported sizes too (NULL, src/pffft_priv_impl.h:1105-1109)
        g_last_error = "pffft_hip: no kernel plan for this size in the product build";
        return false;
    }
    plan_routes(s);       // what runs for every (direction, layout): decided here, printed by pffft_hip_describe()
    for (int d = 0; d < 2; ++d)
        for (int o = 0; o < 2; ++o)
            if (s->route[d][o].fam == FAM_NONE) {
                g_last_error = "pffft_hip: no kernel plan for this size";
                return false;
            }
    return true;
}

Setup* new_setup(int N, int transform, int is_double) {
    if (!setup_args_ok(N, transform)) return nullptr;
    Setup* s = new Setup();
    s->magic = MAGIC;
    s->N = N; s->transform = transform; s->is_double = is_double;
    s->n = transform == PFFFT_REAL ? N / 2 : N;
    s->vec_scalars = transform == PFFFT_REAL ? (size_t)N : 2 * (size_t)N;
    s->kernel = K_STOCK;   // (what sub_is_fast judges this size as until its class is decided below)
    const size_t esz = is_double ? 16 : 8;
    build_resident_plans(s);
    const bool single_image = is_single_image(s, esz);
    if (!one_image_fits(s, esz) || single_image) {
        s->kernel = K_BIG;
        choose_streaming_factor(s, esz, single_image);
        build_strided_pair(s, esz);
        s->sk_ok = s->skw_ok = false;
        build_single_image_plans(s);
    } else {
        s->kernel = resident_kernel_class(s, esz);
    }
    if (!plan_or_refuse(s)) { destroy_setup(s); return nullptr; }
    return s;
}

void destroy_setup(Setup* s) {
    if (!s) return;
    for (auto& kv : s->replicas) destroy_setup(kv.second);
    if (s->sub) destroy_setup(s->sub);
    s->magic = 0;
    delete s;   // (the tables, scratch and staging buffers go with their owners: pf_devmem.h)
}

// The key a thread's current device goes by: the HIP device index; AB_FAKE_DEVICE moves the calling thread to a key of its own (the
// replica path on a one-GPU box).
int current_device_key(int* key) {
    int dev = -1;
    PF_CHECK(hipGetDevice(&dev));
    *key = ab().is(AB_FAKE_DEVICE) ? dev + 64 : dev;
    return 0;
}

// One setup, any device (round 6; the reference's setup is immutable and shareable, include/pffft/pffft.h:102-105).  The object binds
// to the device of its first use; every other device gets a replica of the plan - the same (N, transform, precision), hence the same
// routes - with tables, counter ring, per-stream scratch and staging of its own, built lazily under the setup's mutex and destroyed with it.
Setup* for_device(Setup* s) {
    if (!s || s->magic != MAGIC || s->is_replica) return s;
    int key = -1;
    if (current_device_key(&key)) { (void)hipGetLastError(); return s; }   // no usable device: the entry's own checks report it
    if (s->device.load(std::memory_order_acquire) == key) return s;
    std::lock_guard<std::mutex> lk(s->mu);
    int bound = s->device.load(std::memory_order_relaxed);
    if (bound < 0) { s->device.store(key, std::memory_order_release); return s; }
    if (bound == key) return s;
    auto it = s->replicas.find(key);
    if (it != s->replicas.end()) return it->second;
    Setup* r = new_setup(s->N, s->transform, s->is_double);
    if (!r) return s;                                                       // (cannot happen: the same arguments made `s`)
    r->is_replica = true;
    r->device.store(key, std::memory_order_release);
    s->replicas[key] = r;
    return r;
}

int setup_devices(Setup* s, int* out, int max) {
    if (!s || s->magic != MAGIC) return 0;
    std::lock_guard<std::mutex> lk(s->mu);
    int n = 0;
    // (a bound object whose tables were never built - its first call was refused, e.g. during a stream capture - holds nothing there)
    const int bound = s->device.load();
    if (bound >= 0 && s->dev_ready) { if (out && n < max) out[n] = bound; ++n; }
    for (auto& kv : s->replicas) {
        std::lock_guard<std::mutex> lr(kv.second->mu);
        if (!kv.second->dev_ready) continue;
        if (out && n < max) out[n] = kv.first;
        ++n;
    }
    return n;
}

// ------------------------------------------------------------------------------------------------
// mixed-radix Stockham plans (fft_stock.h): kernel twin, organisation and launch rule of a (direction, layout)
// ------------------------------------------------------------------------------------------------
// false: the product build has no kernel for this plan (a development build runs the run-time-plan kernel: r.stock.fn == nullptr)
template <typename T>
static bool plan_stock(const Setup* s, int dir, int ordered, const AbSel& sel, Route& r) {
    const bool bwd = dir == PFFFT_BACKWARD, real = s->transform == PFFFT_REAL;
    StockSel& k = r.stock;
    k.wl = s->skw_ok && !(PF_HAS_VARIANTS && sel.is(AB_STOCK_WORKGROUP));   // (workgroup plans of the small sizes have run-time twins only)
    if (!k.wl && !s->sk_ok) return false;
    const StockPlan& sp = k.wl ? s->skw[bwd ? 1 : 0] : s->sk[bwd ? 1 : 0];
    k.lds = stock_lds<T>(sp).total;
    k.flags = layout_flags(dir, ordered, real);
    // Static stride by default: these kernels sit at ~0.6-0.75 of the roofline on latency, not on the HBM access order, and the hand-over
    // of the next chunk costs more than the ordering buys (0.63 static against 0.54 in-order chunks on N = 96 .. 800).  The workgroup-phase
    // kernels of the LARGE plans - one workgroup per CU - do gain from the order (round 3, 1 GiB per launch, tools/scan_variant.py): complex
    // float n = 4320 .. 5760 +0.01 .. +0.04, n = 8192 forward 0.68 -> 0.77 / 0.80, n = 8640 0.65 -> 0.77; double n = 2160 .. 4800 +0.02 .. +0.09,
    // n = 4096 forward 0.69 -> 0.81 / 0.79; real transforms are neutral up to 64 KiB and gain 0 .. +0.04 beyond.
    const size_t vbytes = (size_t)sp.n * sizeof(cx<T>);
    bool auto_dyn = false;
    if (!k.wl) auto_dyn = real ? vbytes >= 65536 : vbytes >= (sizeof(T) == 8 ? 32u : 34u) * 1024u;
    const bool dyn = sel.is(AB_INORDER_SMALL) || (auto_dyn && !sel.is(AB_STATIC_LARGE));
    r.rule = dyn ? LR_INORDER : LR_STATIC;
    r.oneshot = dyn ? env().oneshot : 0;
    // the kernel body instantiated on this very plan as a compile-time constant; per plan, direction and layout either the deposit
    // variant or the direct first stage (operands straight from HBM into registers, fft_stock.h sk_df_body) is adopted from a measured
    // table (stock_df_gen.h, tools/tune_stock_df.py): the product build instantiates the adopted one only
    const bool rt_forced = PF_HAS_VARIANTS && sel.is(AB_STOCK_RUNTIME);
    const bool df_ok = !(k.flags & 1) && !rt_forced;
    const bool want_df = df_ok && (sel.is(AB_STOCK_DF_ON) ? true : sel.is(AB_STOCK_DF_OFF) ? false
                                   : stock_df_adopted(sizeof(T) == 8, real, sp.n, (k.flags & 2) != 0, bwd));
    auto cf = want_df ? stock_ct_lookup(sp, k.flags | 16, k.wl, (const T*)nullptr) : nullptr;
    k.df = cf != nullptr;
    if (!cf && !rt_forced) cf = stock_ct_lookup(sp, k.flags, k.wl, (const T*)nullptr);
    if (!cf && !rt_forced && df_ok) { cf = stock_ct_lookup(sp, k.flags | 16, k.wl, (const T*)nullptr); k.df = cf != nullptr; }
    k.fn = reinterpret_cast<const void*>(cf);
    k.threads = (cf && k.df) ? sk_df_threads(sp, k.flags & 15, k.wl) : (k.wl ? s->skw_threads : s->sk_threads);
    // grid of the static stride: groups per workgroup from the measured table (stock_grid_gen.h, tools/tune_stock_grid.py: 2-3 for the
    // complex plans, 3-4 for the real ones, N = 384 / 768 complex float 0.71-0.75 -> 0.78-0.80) or the size rule - 16 x the resident set
    // for vectors <= 4 KiB, 8 x up to 20 KiB, the resident set beyond (tools/stock_bench2.py: N = 96 .. 480 0.63-0.69 -> 0.71-0.77)
    k.groups_per_wg = stock_grid_its(sizeof(T) == 8, real, sp.n);
    k.grid_mul = vbytes <= 4096 ? 16 : vbytes <= 20480 ? 8 : 1;
    return cf != nullptr || PF_HAS_VARIANTS;
}

// ------------------------------------------------------------------------------------------------
// n beyond LDS: the sweeps over HBM of a (direction, layout), planned once (BigPlan), executed by launch_big
// ------------------------------------------------------------------------------------------------
static void plan_big(const Setup* s, int dir, int ordered, const AbSel& sel, BigPlan& b) {
    const bool real = s->transform == PFFFT_REAL, fwd = dir == PFFFT_FORWARD, dbl = s->is_double != 0;
    const bool strided = sel.is(AB_BIG_STRIDED), no_tiles = strided || sel.is(AB_BIG_NO_TILES);
    b = BigPlan();
    // real forward into the canonical spectrum in TWO sweeps where they measured faster (tile_real_tu.hip RMODE; AB_RFFT_THREE = always the
    // complex core + pair sweep, AB_RFFT_TWO = two sweeps wherever the length splits).  Ordered and unordered take the SAME route -
    // pffft_transform_ordered == pffft_zreorder(pffft_transform) bit for bit -: the unordered spectrum is the canonical one of the two
    // sweeps through the one-sweep permutation big_block_kernel<5>
    if (real && fwd && !sel.is(AB_RFFT_THREE) && !no_tiles && tile_rfft_has_plan(2LL * s->n, dbl, !sel.is(AB_RFFT_TWO))) {
        b.core = BIG_RFFT2;
        b.post = ordered ? -1 : 5;
        b.sweeps = ordered ? 2 : 3;
        return;
    }
    const bool blk = !sel.is(AB_BIG_SEPARATE_SWEEPS), fuse_ok = !sel.is(AB_BIG_SEPARATE_LAYOUT);
    // two (three beyond 2^20) tile passes: power-of-two n and the n whose odd part splits over two tile lengths (tile_tu.hip)
    // (deep: the row length of the streaming route is itself beyond LDS, or there is no streaming plan - five sweeps)
    const bool deep = !s->bigR || !s->sub || s->sub->kernel == K_BIG;
    b.tmode = deep ? 1 : real ? 2 : 0;
    bool tiled = !no_tiles && tile_has_plan(s->n, dbl, b.tmode);
    const int tlay = tiled ? tile_plan_layouts(s->n, dbl, b.tmode) : 0;
    // a complex plan with a run-time tile pass that cannot carry the internal layout costs two passes + a reorder sweep against the three
    // streaming passes, which fuse it (measured 0.13-0.15 against 0.18-0.24) - and ordered / unordered must run the SAME arithmetic:
    // such a plan is used for both layouts or for none; it stays where the streaming route would take five sweeps (deep)
    if (tiled && !real && !deep && s->bigR && tlay != 3) tiled = false;
    // backward from the internal layout: the first tile pass / the column pass of the streaming route (R a multiple of 4) reads it itself
    b.fuse_in = !fwd && !ordered && !real && tiled && (tlay & 2) && fuse_ok;
    b.col_in = !fwd && !ordered && !real && !tiled && s->bigR && s->bigR % 4 == 0 && !strided && fuse_ok;
    if (!b.fuse_in && !b.col_in) {
        if (!fwd && !ordered) b.pre = real ? 3 : 1;      // internal -> canonical (complex) / -> packed spectrum of the inverse (real)
        else if (!fwd && real) b.pre = 4;                // canonical half-complex spectrum -> packed spectrum
        b.pre_separate = b.pre >= 0 && !blk;
    }
    // real forward ORDERED on a two-pass plan whose row pass is a register-tiled one on 128-byte runs: the pair pass runs INSIDE that pass (mirror-
    // closed row tiles, fft_tile.h RMODE 3) - two sweeps into the canonical spectrum instead of three.  Its arithmetic is the pair sweeps' operation
    // for operation, so the unordered transform keeps its three sweeps (pair pass + internal layout in one) and pffft_transform_ordered ==
    // pffft_zreorder(pffft_transform) still holds bit for bit.  Adopted in double (0.24-0.25 -> 0.28-0.32 of the roofline); in float the exact-
    // argument W_N^k per pair (a double-precision division + sincospif) costs the small tiles more than the sweep saves - 128-point rows 0.25 ->
    // 0.23, 512-point rows 0.25 -> 0.26 - and AB_RFFT_TWO runs it.  AB_RFFT_THREE: the complex core + pair sweep (the second route of the tests)
    if (tiled && real && fwd && ordered && blk && !sel.is(AB_RFFT_THREE) && (dbl || sel.is(AB_RFFT_TWO)) && tile_real_rows_plan(s->n, dbl, b.tmode)) {
        b.core = BIG_TILES;
        b.rfuse = true;
        b.sweeps = tile_plan_lengths(s->n, dbl, b.tmode, b.lens);
        return;
    }
    if (tiled) {
        b.core = BIG_TILES;
        b.fuse_out = fwd && !ordered && !real && (tlay & 1) && fuse_ok;      // the last tile pass stores the internal layout
        b.sweeps = tile_plan_lengths(s->n, dbl, b.tmode, b.lens);
    } else if (s->bigR && !strided) {
        b.core = BIG_STREAM;
        b.fuse_out = fwd && !ordered && !real && fuse_ok;                    // the transpose pass stores it
        b.lens[0] = s->bigR; b.lens[1] = s->sub->n;
        b.sweeps = s->sub->kernel == K_BIG ? 5 : 3;
    } else {
        b.core = BIG_STRIDED;
        b.lens[0] = s->bigp[0].n; b.lens[1] = s->bigp[1].n;
        b.sweeps = 2;
    }
    if (fwd && !ordered && !b.fuse_out) { b.post = real ? 2 : 0; b.post_separate = !blk; }   // (real: pair pass +) canonical -> internal
    else if (fwd && real) b.pair_after = true;                                                 // real forward ordered: in-place pair pass
    b.sweeps += (b.pre >= 0 ? (b.pre_separate && b.pre != 1 ? 2 : 1) : 0) + (b.post >= 0 ? (b.post_separate && b.post == 2 ? 2 : 1) : 0) + (b.pair_after ? 1 : 0);
}

// ------------------------------------------------------------------------------------------------
// the planner: one Route per (direction, layout), computed at pffft_new_setup (plan_routes) - and again, into a temporary, only for a
// call made under a non-default A/B selector
// ------------------------------------------------------------------------------------------------
// power-of-two sizes where the Stockham kernel on its compile-time plan measured faster than the register-tiled one (1 GiB of vectors,
// tools/stock_ab.py, tools/route_ab.py):
//   float   complex n = 16: 0.46 vs 0.26, 32: 0.70 vs 0.59, 64: 0.70 vs 0.65, 128: 0.65 -> 0.71-0.74, 8192: 0.68-0.73 vs 0.62-0.70 (both directions since
//           the large plans are pulled in order: backward 0.78 / 0.72 -> 0.77 / 0.78); real N = 32: 0.38 vs 0.26, 64: 0.66 vs 0.60, N = 128 0.66-0.69 ->
//           0.62-0.75, N = 16384 backward 0.61-0.68 vs 0.51-0.60 (symmetric spectrum-side stage)
//   double  complex n = 16: 0.50 vs 0.26, 32: 0.70 vs 0.48, 64: 0.69 vs 0.47, 128 / 256 0.68 -> 0.75, 2048 0.70-0.72 -> 0.75-0.77, 4096 forward
//           0.70 -> 0.73 / 0.75, backward 0.71 -> 0.77; real N = 32: 0.42 vs 0.29, 64: 0.66 vs 0.55, 128 0.39-0.50 -> 0.66-0.76, N = 256 backward 0.70 ->
//           0.76, N = 512 0.70-0.73 -> 0.73-0.75, N = 4096 0.69-0.72 -> 0.71-0.75, N = 8192 forward 0.68 / 0.69 -> 0.73 / 0.70
template <typename T>
static bool pow2_prefers_stock(int n, bool cplx, bool fwd) {
    if (sizeof(T) == 4) return cplx ? (n <= 64 || n == 128 || n == 8192) : (n <= 64 || (n == 8192 && !fwd));
    return cplx ? (n <= 256 || n >= 2048) : (n <= 64 || (n == 128 && !fwd) || n == 256 || n >= 2048);
}

template <typename T>
static Route plan_route_t(const Setup* s, int dir, int ordered, const AbSel& sel) {
    Route r;
    const bool real = s->transform == PFFFT_REAL, fwd = dir == PFFFT_FORWARD;
    // n = 16 / 32: one thread per transform (fft_tiny.h), one group of 64 vectors per wavefront in dispatch order (measured faster than
    // persistent wavefronts on a static stride: 256-byte vectors 0.75-0.78 against 0.67-0.72)
    if (!sel.is(AB_NO_TINY) && (s->n == 16 || (sizeof(T) == 4 && s->n == 32))) { r.fam = FAM_TINY; r.rule = LR_DISPATCH; return r; }
    const bool stock_all = sel.is(AB_STOCK_FOR_TILED) && s->sk_ok;
    if (sizeof(T) == 4 && s->kernel == K_C1024_F32 && !stock_all) {
        r.fam = FAM_C1024; r.rule = LR_INORDER; r.oneshot = env().c1024_rounds;
        return r;
    }
    if (s->kernel == K_TILED && !stock_all) {
        const bool stock = s->sk_ok && pow2_prefers_stock<T>(s->n, !real, fwd);
        if (!stock && tiled_pick_any(sizeof(T) == 8, s->n, dir, real ? 1 : 0, ordered, &r.tiled)) {
            r.fam = FAM_TILED; r.rule = LR_INORDER;
            // (N = 4096 complex float alone prefers the dispatch order up to SIXTEEN groups per workgroup: 256 / 512 MiB 111 / 193 -> 91 / 178 us; every
            //  other size measured loses there - 4096 real 104 -> 154 us at 256 MiB, 16384 complex 217 -> 283 at 512 MiB)
            r.oneshot = (env().oneshot == 4 && sizeof(T) == 4 && s->n == 4096 && !real) ? 16 : env().oneshot;
            return r;
        }
    }
    if (s->kernel == K_BIG && s->one_ok && !sel.is(AB_NO_ONE_IMAGE)) { r.fam = FAM_ONE; r.rule = LR_INORDER; return r; }
    if (s->kernel == K_BIG) { r.fam = FAM_BIG; r.rule = LR_INORDER; plan_big(s, dir, ordered, sel, r.big); return r; }
    if ((s->sk_ok || s->skw_ok) && plan_stock<T>(s, dir, ordered, sel, r)) { r.fam = FAM_STOCK; return r; }
    r.fam = FAM_NONE;   // (every legal size is routed above: new_setup sends whatever has no Stockham plan to the streaming passes, K_BIG)
    return r;
}

Route plan_route(const Setup* s, int dir, int ordered, const AbSel& sel) {
    return s->is_double ? plan_route_t<double>(s, dir, ordered, sel) : plan_route_t<float>(s, dir, ordered, sel);
}

static void plan_routes(Setup* s) {
    // The stored routes are the DEFAULT ones whatever selector the creating thread has set: the tile planner's helpers
    // (tile_has_plan, tile_plan_lengths) read the calling thread's selector themselves (AB_BIG_NO_MR_TILES), so it is cleared for the
    // planning and restored (a setup created under set_variant(83) had the streaming route baked in as its default)
    const int keep = g_ab_raw;
    g_ab_raw = 0;
    const AbSel none;
    for (int d = 0; d < 2; ++d)
        for (int o = 0; o < 2; ++o)
            s->route[d][o] = plan_route(s, d, o, none);
    g_ab_raw = keep;
}

// ------------------------------------------------------------------------------------------------
// pffft_hip_describe: the routes of a setup as text
// ------------------------------------------------------------------------------------------------
const char* family_name(Family f) {
    switch (f) {
        case FAM_TINY: return "tiny";
        case FAM_C1024: return "c1024_f32";
        case FAM_TILED: return "tiled";
        case FAM_STOCK: return "stockham";
        case FAM_BIG: return "fourstep";
        case FAM_ONE: return "oneimage";
        default: return "none";
    }
}
const char* launch_rule_name(LaunchRule r) {
    switch (r) {
        case LR_DISPATCH: return "dispatch-order";
        case LR_STATIC: return "static-stride";
        default: return "in-order";
    }
}
static int describe_route(const Setup* s, const Route& r, int dir, int ordered, char* buf, size_t len) {
    switch (r.fam) {
        case FAM_TINY: return snprintf(buf, len, "tiny: one thread per transform, %s", launch_rule_name(r.rule));
        case FAM_C1024:
            return snprintf(buf, len, "c1024_f32: loop 8 waves/wg x 1 wg/CU %s; <= %d resident sets: once kernel %d waves/wg %s, resident set %d waves/CU",
                            launch_rule_name(r.rule), r.oneshot, C1024_ONCE_W, launch_rule_name(LR_DISPATCH), C1024_ONCE_RESIDENT);
        case FAM_TILED:
            return snprintf(buf, len, "tiled: cfg %s wg %d vec/wg %d lds %zu %s oneshot<=%d groups/wg", r.tiled.cfg, r.tiled.wg, r.tiled.t_per_wg,
                            r.tiled.lds, launch_rule_name(r.rule), r.oneshot);
        case FAM_STOCK: {
            char grid[48], once[48] = "";
            if (r.rule == LR_INORDER && r.oneshot) snprintf(once, sizeof once, " oneshot<=%d groups/wg", r.oneshot);
            if (r.stock.groups_per_wg > 0) snprintf(grid, sizeof grid, "%d groups/wg (table)", r.stock.groups_per_wg);
            else snprintf(grid, sizeof grid, "%d x resident set", r.stock.grid_mul);
            return snprintf(buf, len, "stockham: %s%s%s threads %d lds %zu %s grid %s%s", r.stock.wl ? "wave-local" : "workgroup",
                            r.stock.df ? " direct-first-stage" : " deposit", r.stock.fn ? "" : " run-time-plan", r.stock.threads, r.stock.lds,
                            launch_rule_name(r.rule), r.rule == LR_INORDER ? "resident set" : grid,
                            once);
        }
        case FAM_BIG: {
            const BigPlan& b = r.big;
            char core[96];
            switch (b.core) {
                case BIG_RFFT2: snprintf(core, sizeof core, "real two-sweep tiles"); break;
                case BIG_TILES:
                    if (b.lens[2]) snprintf(core, sizeof core, "tiles %d x %d x %d (mode %d)", b.lens[0], b.lens[1], b.lens[2], b.tmode);
                    else snprintf(core, sizeof core, "tiles %d x %d (mode %d)%s", b.lens[0], b.lens[1], b.tmode, b.rfuse ? " real-rows" : "");
                    break;
                case BIG_STREAM: snprintf(core, sizeof core, "streaming %d x %d%s", b.lens[0], b.lens[1], (s->sub && s->sub->kernel == K_BIG) ? " (rows beyond LDS)" : ""); break;
                default: snprintf(core, sizeof core, "strided %d x %d", b.lens[0], b.lens[1]); break;
            }
            return snprintf(buf, len, "fourstep: %s; pre %d%s fuse_in %d col_in %d fuse_out %d post %d%s pair_after %d; %d sweeps", core, b.pre,
                            b.pre_separate ? "(separate)" : "", (int)b.fuse_in, (int)b.col_in, (int)b.fuse_out, b.post, b.post_separate ? "(separate)" : "",
                            (int)b.pair_after, b.sweeps);
        }
        case FAM_ONE: {
            // the plan launch_one_t (one_tu.hip) runs: the float complex backward transform from the layout has one of its own
            const StockPlan& sp = s->one[one_plan_index(s->is_double != 0, layout_flags(dir, ordered, s->transform == PFFFT_REAL))];
            char rad[48] = "";
            for (int i = 0; i < sp.ns; ++i) snprintf(rad + strlen(rad), sizeof rad - strlen(rad), i ? " x %d" : "%d", sp.st[i].R);
            return snprintf(buf, len, "oneimage: one %d-thread workgroup per vector, stages %s in place, lds %zu %s; 1 sweep", sp.C, rad,
                            one_lds_bytes(sp, s->is_double != 0, s->transform == PFFFT_REAL), launch_rule_name(r.rule));
        }
        default: return snprintf(buf, len, "none");
    }
}
// the family a SIZE is built for (pffft_hip_kernel_name); a (direction, layout) of a power of two may still run its Stockham plan
const char* setup_family(const Setup* s) {
    if (!ab().is(AB_NO_TINY) && (s->n == 16 || (s->n == 32 && !s->is_double))) return "tiny";
    switch (s->kernel) {
        case K_C1024_F32: return "c1024_f32";
        case K_TILED: return "tiled";
        case K_BIG: return "fourstep";
        // "stockham_rt": the plan has no compile-time twin and runs the run-time-plan kernel (0.3 of the roofline and less)
        default: return s->sk_ok ? (sub_is_fast(s) ? "stockham" : "stockham_rt") : "none";
    }
}
int describe_setup(const Setup* s, char* buf, size_t len) {
    std::string out;
    char line[512];
    snprintf(line, sizeof line, "pffft_hip setup N=%d %s %s: core n=%d, family %s\n", s->N, s->transform == PFFFT_REAL ? "real" : "complex",
             s->is_double ? "f64" : "f32", s->n, setup_family(s));
    out += line;
    static const char* dn[2] = {"forward ", "backward"};
    static const char* on[2] = {"unordered", "ordered  "};
    // under a selector (pffft_hip_set_variant) the routes that selector runs, planned exactly as transform_batch plans them
    const AbSel sel = ab();
    for (int d = 0; d < 2; ++d)
        for (int o = 1; o >= 0; --o) {
            char body[400];
            const Route r = !sel.any() ? s->route[d][o] : plan_route(s, d, o, sel);
            describe_route(s, r, d, o, body, sizeof body);
            snprintf(line, sizeof line, "  %s %s: %s\n", dn[d], on[o], body);
            out += line;
        }
    if (buf && len) { const size_t c = out.size() < len - 1 ? out.size() : len - 1; memcpy(buf, out.data(), c); buf[c] = 0; }
    return (int)out.size();
}

// Layout self-test standing in for validate_pffft_simd_ex (src/pffft_priv_impl.h:1889-2225, which
// unit-tests the SIMD macros): checks on the host that the internal-layout map used by the kernels
// is a permutation with the documented fixed points.  Returns the number of errors.
static int host_bin_of(int v, int l, int n, int is_real) {
    int b = v >> 3, q = (v >> 1) & 3, t = 4 * b + l;
    if (!is_real) return q * (n >> 2) + t;
    switch (q) {
        case 0: return t;
        case 2: return (n >> 1) + t;
        case 1: return t ? (n >> 1) - t : (n >> 2);
        default: return t ? n - t : 3 * (n >> 2);
    }
}
int validate_layout(FILE* dbg) {
    int errors = 0;
    for (int is_real = 0; is_real < 2; ++is_real)
        for (int n : {16, 32, 48, 80, 1024}) {
            std::vector<int> seen(2 * n, 0);
            for (int v = 0; v < n / 2; ++v)
                for (int l = 0; l < 4; ++l) {
                    int idx = 2 * host_bin_of(v, l, n, is_real) + (v & 1);
                    if (idx < 0 || idx >= 2 * n || seen[idx]++) ++errors;
                }
            if (host_bin_of(0, 0, n, is_real) != 0) ++errors;
            if (dbg) fprintf(dbg, "pffft_hip layout check n=%d real=%d: errors so far %d\n", n, is_real, errors);
        }
    return errors;
}

}  // namespace pf
