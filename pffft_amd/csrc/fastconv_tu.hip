// pffastconv on the GPU: overlap-save FIR with ALL blocks of a call batched into one pass.
//
// Reference: src/pffastconv.c — setup :58-116 (Nfft choice :62-80, flipped / zero-stuffed filter image
// :99-106, one forward transform into Hf :108), apply :133-263 (block loop :207-261: copy + zero pad,
// forward rFFT, pffft_zconvolve_no_accu with scale 1/Nfft, backward rFFT, copy numOut samples).
// The reference walks the blocks one by one on one core; here every block of the call is gathered
// into a [nblk][Nfft] device image and pushed through the batched kernels in place:
//   gather -> rFFT fwd (internal layout) -> x Hf * 1/Nfft -> rFFT bwd -> scatter.
// A translation unit of libpffft_hip.so: it runs the transforms and helpers through the typed entries of pf_host.h.  In order: fir_route
// decides (integers only), fc_spectrum builds the filter tables, the launchers take one FirCall, fc_apply_device joins them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/pffft_hip.h"
#include "pf_host.h"
#include "pf_launch.h"
#include "fft_fir.h"
#include "fft_firtd.h"

namespace pf {

// what a setup fixes of every call's route: all that fir_route reads of it
struct FirGeom {
    int filterLen;  // effective length (2*len-1 for the single-FFT complex mode, src/pffastconv.c:93-94)
    int Nfft, flags, cplxFactor;
};
struct FastConv : FirGeom {
    uint32_t magic;
    PFFFT_Setup* st;
    float scale;
    std::vector<float> h_filter_image;  // time-domain image the reference builds in Xt (:99-106)
    std::mutex mu;
    bool ready = false;     // set only after EVERY step of fc_ensure_device succeeded
    int device = -1;
    // a launch of this setup was recorded into a HIP graph (on d_Hc_big / st_big: recorded_big): a replay reads the table addresses it froze, so
    // from then on nothing of them is freed before pffastconv_destroy_setup - no move to another device, no other internal block length
    bool recorded = false, recorded_big = false;
    // (device tables, work images and staging: DevBuf / PinnedBuf / StreamScratch of pf_devmem.h, freed with the setup)
    DevBuf d_Hf;
    DevBuf d_Hc;  // canonical-order filter spectrum * 1/Nfft for the fused kernel
    // throughput regime (many blocks): the same outputs through LARGER internal blocks (better overlap-save efficiency)
    PFFFT_Setup* st_big = nullptr; DevBuf d_Hc_big; int Nfft_big = 0;
    // partitioned path (fft_fir.h fastconv_part_kernel): P spectra of 1024-tap partitions on 2048-sample blocks
    PFFFT_Setup* st_part = nullptr; DevBuf d_Hp; int part_P = 0;
    std::vector<float> h_td;  // y[m] = sum_i h_td[i] x[m + i]: the filter as the time-domain kernel applies it (zero padded to 8)
    DevBuf d_td;
    DevBuf d_fir32_hp;       // thread-major filter spectrum of the 32-points-per-thread block kernel (fft_fir32.h), of d_Hc_big
    DevBuf d_fir32_hp_ref;   // ... of d_Hc (filters whose reference block length is 16384 samples itself)
    DevBuf d_split1_ab;      // folded per-bin coefficients of the few-block split kernel (fft_split.h), built on first use
    StreamScratch work;      // work image of the composed path (buf[0]): one per stream; FastConv::mu is the lock its callers hold
    DevBuf d_x, d_y;         // staging of pffastconv_apply's host pointers (large signals)
    PinnedBuf h_x, h_y;      // pinned host images the kernels read / write directly (zero copy)
};
constexpr uint32_t FC_MAGIC = 0x46434e56u;

// ---- the route of a call: integer arithmetic on FirGeom - no device, no allocation, no FastConv state ----------------------------------
enum FirKind : uint8_t { FIR_NONE, FIR_TD, FIR_WAVE, FIR_PART, FIR_FIR32, FIR_DMA, FIR_SPLIT, FIR_SPLIT1, FIR_FUSED, FIR_GATHER };
static const char* const FIR_KERNEL[] = {"", "fastconv_td_kernel", "fastconv_wave_kernel", "fastconv_part_kernel", "fastconv_fused32_kernel", "fastconv_dma_kernel",
                                         "fastconv_split_kernel", "fastconv_split1_kernel", "fastconv_fused_kernel", "fastconv_gather_kernel"};
// the filter table a route reads: d_Hc on the reference's blocks (the composed path: d_Hf), d_Hc_big on blocks of `block` samples, d_Hp, d_td
enum FirTable : uint8_t { FT_REF, FT_BIG, FT_PART, FT_TD };
enum FirFused : int { FF_C512, FF_C1024, FF_C2048, FF_C2048m, FF_C4096, FF_C4096m, FF_C8192 };   // the FirCfg of a FIR_FUSED route
static const char* const FIR_FUSED_NAME[] = {"C512", "C1024", "C2048", "C2048m", "C4096", "C4096m", "C8192"};
struct FirRoute {
    FirKind kind = FIR_NONE;
    int cfg = 0;   // TD: stride of the float stream 1 | 2; PART: partitions; FIR32: prefetch form 2 (development build: 0 | 1); SPLIT: 1 (...: plain 0); SPLIT1: wavefronts 4 | 8; FUSED: FirFused
    FirTable table = FT_REF;
    int block = 0, step = 0, blocks = 0, last = 0;   // internal block length, its valid samples, blocks per signal, outputs of the last one
    int produced = 0;                                // fc_schedule's: samples of the real stream one signal produces
};

// Block schedule of src/pffastconv.c:156-166 / :204-210.  Returns the number of time blocks and the
// number of outputs of the last one; *produced = value returned by pffastconv_apply (in real samples).
static int fc_schedule(const FirGeom& s, int inputLen, int flush, int* lastOut, int* produced) {
    const int Nfft = s.Nfft, flen = s.filterLen;
    const int step_full = s.cplxFactor == 2 ? ((Nfft - flen + 1) & ~1) : (Nfft - flen + 1);
    const long maxOff = flush ? ((long)inputLen - flen + 1) : ((long)inputLen - Nfft + 1);
    if (s.cplxFactor == 1) {
        // closed form of the loop below (it runs once per block: a million iterations for a short filter on a long signal):
        // full blocks while off + Nfft <= inputLen, then - flushing only - one partial block with the remaining outputs
        const long nfull = inputLen >= Nfft ? ((long)inputLen - Nfft) / step_full + 1 : 0;
        long off = nfull * step_full;
        int nb = (int)nfull, lst = nfull ? step_full : 0;
        if (flush && off < maxOff) { lst = (int)(inputLen - off - flen + 1); off += lst; ++nb; }
        *lastOut = lst;
        *produced = (int)off;
        return nb;
    }
    int nblk = 0, last = 0;
    long off = 0;
    while (off < maxOff) {
        long remain = inputLen - off;
        int procLen = remain >= Nfft ? Nfft : (int)remain;
        int numOut = procLen - flen + 1;
        if (s.cplxFactor == 2) { numOut &= ~1; if (!numOut) break; }
        ++nblk; last = numOut; off += numOut;
        if (numOut != step_full) break;  // a partial block is always the last one
    }
    *lastOut = last;
    *produced = (int)off;
    return nblk;
}

// filters of up to this many taps take the wave kernel (from g_fir_wave_min on, below): beyond, the 16384-sample split kernel (fft_split.h, round 4) is faster - 800 taps 0.44 / 0.465 (wave) against
// 0.41 / 0.46 (split), 900 taps 0.40 / 0.43 against 0.41 / 0.46, 1024 taps 0.37 / 0.39 against 0.40 / 0.45 (tools/fir_shapes.py)
static const int g_fir_wave_max = dev_env("PFFASTCONV_HIP_WAVE_MAX", 850);
// Filters from this many taps up take the wave kernel when a call has many blocks (PFFASTCONV_HIP_WAVE_MIN, A/B); below: time
// domain.  Measured (MI355X, tools/fir_quick.py, fraction of the 8 B / sample roofline on 2^26 samples / 256 signals of 2^20;
// time domain or partitioned kernel -> wave kernel): 8-24 taps 0.47 / 0.50-0.52 -> 0.47-0.49 / 0.56 (a tie: the time-domain
// kernel stays), 32 taps 0.45 / 0.49 -> 0.52 / 0.57, 64 taps 0.38 / 0.43 -> 0.52 / 0.55, 128 taps 0.25 / 0.30 -> 0.52 / 0.55,
// 200 taps 0.31 / 0.38 -> 0.54 / 0.54, 600 taps 0.31 / 0.38 -> 0.39 / 0.47, 800 taps -> 0.35 / 0.43, 1024 taps 0.30 / 0.37 (equal).
static const int g_fir_wave_min = dev_env("PFFASTCONV_HIP_WAVE_MIN", 32);
// the partitioned path: the filter as P partitions of PART_B taps on blocks of 2 PART_B samples (fft_fir.h); the wave kernel is its P = 1
constexpr int PART_B = 1024, PART_MAXP = 4;
constexpr long FIR_WAVE_BLOCKS_PER_CU = 8;   // the wave kernel from this many of its blocks per CU on
constexpr long FIR_REF_BLOCKS_PER_CU = 2;    // reference blocks of 16384 samples on the 16384-sample kernels from this many per CU on
constexpr int FIR_BIG_FLOOR_TAPS = 128;      // up to this many taps no longer internal blocks (the table of fc_big_nfft)

// Internal block length for the throughput regime.  What a caller can observe of the reference's blocks is only HOW MANY
// samples a call produces (fc_schedule); the values are those of the exact convolution whatever the block length, so
// when a call has many blocks the same `produced` outputs are computed with longer internal blocks: overlap-save
// efficiency (Nfft - len + 1) / Nfft goes from ~0.5 (the reference's Nfft = 2 next_pow2(len-1), src/pffastconv.c:62-63)
// to 0.75-0.94.  PFFASTCONV_HIP_NFFT=<n> forces a length (A/B), =0 switches this off.
static int fc_big_nfft(const FirGeom& s, long produced, int nsig, int cus, int forced, int wave_max) {
    if (forced == 0) return 0;
    const int taps = s.filterLen;
    // measured table (MI355X, tools/fir_quick.py with PFFASTCONV_HIP_NFFT forced; fraction of the 8 B / sample roofline on
    // 2^26 samples / on 256 signals of 2^20; r02):      Nfft   2048          4096          8192          16384
    //    200 taps (FFT route forced)                         0.12 / 0.15   0.23 / 0.30   0.26 / 0.31   0.26 / 0.30
    //    600 taps                                            0.10 / 0.12   0.22 / 0.27   0.25 / 0.30   0.27 / 0.29
    //   1024 taps                                            0.08 / 0.09   0.20 / 0.24   0.24 / 0.28   0.26 / 0.29
    //   2048 taps                                                 -        0.14 / 0.17   0.22 / 0.25   0.25 / 0.27
    //   4096 taps                                                 -             -        0.16 / 0.19   0.21 / 0.24
    // -> 16384 from 1024 taps on, 8192 below (the time-domain kernel wins up to ~128 taps).  All block kernels saturate
    // near 0.26-0.30: two 8192-point transforms per block cost ~33 k cycles per CU whatever the filter.
    const int want = forced > 0 ? forced : (taps <= wave_max ? 8192 : 16384);
    if (want <= s.Nfft || want > 16384 || (want & (want - 1)) || want < 2 * taps) return 0;
    if (want < 2048) return 0;                           // (a forced length below the block kernels': the reference's blocks)
    if (forced > 0) return want;
    if (taps <= FIR_BIG_FLOOR_TAPS) return 0;
    const long bblk = (produced + (want - taps)) / (want - taps + 1);
    return bblk * nsig >= cus ? want : 0;                // fewer blocks: latency regime, one reference-sized block per CU is faster
}

// What one call of `nsig` signals of `cplxInputLen` samples runs on a device of `cus` compute units: the first branch that holds.
static FirRoute fir_route(const FirGeom& s, int cplxInputLen, int nsig, int flush, int cus, const AbSel& sel, const Env& e, int wave_min,
                          int wave_max) {
    FirRoute r;
    const int flen = s.filterLen, Nfft = s.Nfft, cf = s.cplxFactor;
    int lastOut = 0;
    const int nbt = fc_schedule(s, cf * cplxInputLen, flush, &lastOut, &r.produced);   // :141
    if (nbt == 0) return r;
    const long produced = r.produced;
    const int mode = ((s.flags & PFFASTCONV_HIP_CPLX_INP_OUT) && cf == 1) ? 1 : 0;     // 1: two real streams per signal (fft_firtd.h)
    const bool real = mode == 0 && cf == 1;
    auto own = [&](FirKind k, int cfg, FirTable t, int block, int step, long outs) {   // blocks of the route's own over `outs` samples
        const int nb = (int)((outs + step - 1) / step);
        return FirRoute{k, cfg, t, block, step, nb, (int)(outs - (long)(nb - 1) * step), r.produced};
    };
    auto ref = [&](FirKind k, int cfg) {                                               // the reference's blocks (fc_schedule; mode 1: two per time block)
        return FirRoute{k, cfg, FT_REF, Nfft, cf == 2 ? ((Nfft - flen + 1) & ~1) : (Nfft - flen + 1), mode ? 2 * nbt : nbt, lastOut, r.produced};
    };
    // 16384-sample blocks: 256 threads, 32 points per thread, four exchanges per block (fft_fir32.h, round 6); AB_FIR_SPLIT: the split
    // kernel it replaced (fft_split.h: the second route of tests/test_gpu_round6.py: cross-wave radix 8 + wave-local 1024-point transforms).
    // Development build: AB_FIR_LOCKSTEP = the lock-step LDS-DMA kernel that one replaced, AB_FIR_SPLIT_PLAIN = without the pairwise
    // flags and the spread pieces (the product build runs the split kernel under all three)
    const bool not32 = sel.is(AB_FIR_SPLIT) || sel.is(AB_FIR_LOCKSTEP) || sel.is(AB_FIR_SPLIT_PLAIN);
    const FirKind k16 = !not32 ? FIR_FIR32 : (PF_HAS_VARIANTS && sel.is(AB_FIR_LOCKSTEP)) ? FIR_DMA : FIR_SPLIT;
    const int split_cfg = (PF_HAS_VARIANTS && sel.is(AB_FIR_SPLIT_PLAIN)) ? 0 : 1;
    if (real && !sel.any() && flen >= wave_min && flen <= PART_B && flen <= wave_max && produced > 0) {
        // many blocks of a filter of up to 1024 taps: one wavefront per 2048-sample block, step = 2048 - taps + 1 (round 3;
        // the partitioned kernel below advances 1024 samples per block whatever the filter)
        const int wstep = (2 * PART_B - flen + 1) & ~3;                                // valid samples per block, 16-byte store units
        if ((produced + wstep - 1) / wstep * nsig >= FIR_WAVE_BLOCKS_PER_CU * cus) return own(FIR_WAVE, 0, FT_PART, 2 * PART_B, wstep, produced);
    }
    if (PF_HAS_VARIANTS && real && flen > TD_MAX_TAPS / 4 && flen <= PART_B * PART_MAXP && sel.is(AB_FIR_PARTITIONED) && produced > 0) {
        // development build: the uniformly partitioned one-wavefront-per-block kernel (fft_fir.h fastconv_part_kernel, round 2;
        // AB_FIR_PARTITIONED forces it).  Measured (fraction of the 8 B / sample roofline, 2^26 samples / 256
        // signals of 2^20): one partition 0.30 / 0.37 - superseded by the wave kernel above, which advances by the samples the
        // filter leaves valid instead of 1024; two partitions (2048 taps) 0.25 / 0.26 lose to the long-block DMA kernel; three
        // and four keep their ring in > 256 registers and run one wavefront per SIMD (0.12-0.23).
        return own(FIR_PART, (flen + PART_B - 1) / PART_B, FT_PART, 2 * PART_B, PART_B, produced);
    }
    if (const int nbig = real ? fc_big_nfft(s, produced, nsig, cus, e.fir_nfft, wave_max) : 0) {
        // shorter internal blocks: the register-staged fused kernel (tools/dma_ab.py: a tie with the DMA kernel at Nfft 8192, 0.22-0.29 both)
        if (nbig != 16384) return own(FIR_FUSED, nbig == 2048 ? FF_C1024 : nbig == 4096 ? FF_C2048 : FF_C4096, FT_BIG, nbig, nbig - flen + 1, produced);
        const int pf = !PF_HAS_VARIANTS ? 2 : sel.is(AB_FIR_FUSED32_PF1) ? 1 : sel.is(AB_FIR_FUSED32_NOPF) ? 0 : 2;
        return own(k16, k16 == FIR_FIR32 ? pf : split_cfg, FT_BIG, nbig, nbig - flen + 1, produced);
    }
    const int taps = cf == 2 ? (flen + 1) / 2 : flen;   // the caller's filter length
    // short real filter: time domain, in tiles of the float stream; the complex modes are the stride-2 sum over it
    if (taps <= TD_MAX_TAPS) return own(FIR_TD, (mode == 1 || cf == 2) ? 2 : 1, FT_TD, TD_TILE, TD_TILE, mode == 1 ? 2 * produced : produced);
    if (mode == 0 && Nfft == 16384 && (long)nbt * nsig >= FIR_REF_BLOCKS_PER_CU * cus) return ref(k16, k16 == FIR_FIR32 ? 2 : split_cfg);   // many reference-sized blocks
    // few blocks of 8192 / 4096 samples: cross-wave radix 8 / 4 + wave-local 512-point transforms (fft_split.h
    // fastconv_split1_kernel, round 4); AB_FIR_FEW_LOCKSTEP = the lock-step kernel on 512 / 256 threads (the second route of
    // tests/test_gpu_round4.py), AB_FIR_FEW_16PT (development build) = on 256 / 128
    if (mode == 0 && !sel.is(AB_FIR_FEW_16PT) && !sel.is(AB_FIR_FEW_LOCKSTEP) && (Nfft == 8192 || Nfft == 4096)) return ref(FIR_SPLIT1, Nfft == 8192 ? 8 : 4);
    if (mode == 0) {  // one real stream: the fused one-kernel path when Nfft/2 has a tiled kernel
        const bool pt16 = PF_HAS_VARIANTS && sel.is(AB_FIR_FEW_16PT);
        switch (Nfft / 2) {
            case 512: return ref(FIR_FUSED, FF_C512);
            case 1024: return ref(FIR_FUSED, FF_C1024);
            // 2048 / 4096 points: twice the threads per block, eight points per thread (FirCfg::C*m, round 4): the stated C4 call
            // 10.9 -> 9.5 us, 2048 taps on 2^19 samples 8.8 -> 7.3 us; n = 8192 on 1024 threads measured slower (15.9 -> 17.9 us).
            case 2048: return ref(FIR_FUSED, pt16 ? FF_C2048 : FF_C2048m);
            case 4096: return ref(FIR_FUSED, pt16 ? FF_C4096 : FF_C4096m);
            case 8192: return ref(FIR_FUSED, FF_C8192);
        }
    }
    return ref(FIR_GATHER, 0);   // composed path (complex-I/O modes with long filters, blocks beyond the block kernels')
}

// ---- the filter tables --------------------------------------------------------------------------------------------------------------
// everything this setup holds on its device: the filter tables of every route, per-stream work images, staging (not the pinned host
// images, not the inner pffft setups - those keep state per device themselves, for_device)
static void fc_release_device(FastConv* s) {
    for (DevBuf* b : {&s->d_Hf, &s->d_Hc, &s->d_Hc_big, &s->d_Hp, &s->d_td, &s->d_split1_ab, &s->d_fir32_hp, &s->d_fir32_hp_ref, &s->d_x, &s->d_y})
        b->reset();
    s->work.clear();
    s->Nfft_big = 0; s->part_P = 0; s->ready = false;
}

// The spectrum of `count` time-domain filter images of Nfft floats (:99-108) as the block kernels read it: upload -> forward transform
// (the internal layout: kept in *keep_internal when asked) -> canonical order (pffft_zreorder) -> x scale, built on the null stream and
// COMPLETE before the caller publishes it.  A failed build leaves both buffers empty; the caller's cached length / count stays zero.
// A table that does not exist yet is built with hipMalloc, launches on the null stream and a synchronisation: never while the call's stream
// records into a HIP graph.  Refused before anything is allocated or dropped; `what` names the missing table in the text.
static int fc_refuse_capture(const char* what) {
    return bad((std::string("pffastconv: ") + what + " of this setup would have to be built during graph capture: run a call of this shape "
                "once before capturing").c_str(), hipErrorStreamCaptureUnsupported);
}

static int fc_spectrum(PFFFT_Setup* st, const float* host_images, int count, int Nfft, float scale, DevBuf& Hc, DevBuf* keep_internal) {
    const size_t bytes = sizeof(float) * (size_t)count * Nfft;
    DevBuf tmp;
    DevBuf& Hf = keep_internal ? *keep_internal : tmp;
    int rc = Hf.grow(bytes);
    if (!rc) rc = Hc.grow(bytes);
    float* const f = Hf.as<float>();
    float* const c = Hc.as<float>();
    hipError_t e = hipSuccess;
    if (!rc && (e = hipMemcpy(f, host_images, bytes, hipMemcpyHostToDevice)) != hipSuccess) rc = fail(e, "pffastconv: upload of the filter image");
    if (!rc) rc = transform_batch<float>(st, f, f, count, PFFFT_FORWARD, 0, nullptr);   // :108
    if (!rc) rc = zreorder_batch<float>(st, f, c, count, PFFFT_FORWARD, nullptr);
    if (!rc) {
        hipLaunchKernelGGL(fastconv_scale_kernel, dim3(64), dim3(256), 0, nullptr, c, c, count * Nfft, scale);
        if ((e = hipGetLastError()) == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) rc = fail(e, "fastconv_scale_kernel");
    }
    if (rc) { Hf.reset(); Hc.reset(); }
    return rc;
}

// A PFFASTCONV_Setup is used by one thread at a time (the reference's is "not shareable", include/pffft/pffastconv.h:77-80,142-143) and
// holds the filter's tables on ONE device: the calling thread's current one.  Round 6: a call from another device no longer fails - the
// tables are released and rebuilt there (the filter is kept on the host), i.e. the setup follows its user from device to device; a caller
// that alternates between devices call by call should hold one setup per device.  Once a HIP graph has recorded a launch of the setup it
// stays where it is: a replay reads the tables at the addresses it froze.  `capturing`: the call's stream records right now.
static int fc_ensure_device(FastConv* s, bool capturing) {
    int dev = -1;
    if (int rc = current_device_key(&dev)) return rc;
    if (s->ready) {
        if (dev == s->device) return 0;
        if (s->recorded)
            return bad("pffastconv: a captured graph reads the tables of this setup on the device of its first calls: they stay there until "
                       "pffastconv_destroy_setup (one setup per device)", hipErrorInvalidDevice);
        if (capturing) return fc_refuse_capture("the reference-block spectrum (on the calling thread's device)");
        fc_release_device(s);
    }
    if (capturing) return fc_refuse_capture("the reference-block spectrum");
    // (a failed build: a later call, on whatever device, starts over instead of launching on half-built tables)
    if (int rc = fc_spectrum(s->st, s->h_filter_image.data(), 1, s->Nfft, s->scale, s->d_Hc, &s->d_Hf)) return rc;
    s->device = dev;
    s->ready = true;
    return 0;
}

static int fc_ensure_big(FastConv* s, int Nfft_big, bool capturing) {
    if (s->Nfft_big == Nfft_big) return 0;
    if (capturing) return fc_refuse_capture("the big-block spectrum");
    if (s->recorded_big)
        return bad("pffastconv: a captured graph reads the big-block spectrum of this setup: a call that needs another internal block length "
                   "would free it (use a second setup for such calls)", hipErrorInvalidValue);
    if (s->st_big) { pffft_destroy_setup(s->st_big); s->st_big = nullptr; }
    s->d_Hc_big.reset(); s->d_fir32_hp.reset(); s->Nfft_big = 0;
    s->st_big = pffft_new_setup(Nfft_big, PFFFT_REAL);
    if (!s->st_big) { g_last_error = "pffastconv: internal setup failed"; return (int)hipErrorInvalidValue; }
    std::vector<float> img((size_t)Nfft_big, 0.f);
    for (int i = 0; i < s->filterLen; ++i) img[(Nfft_big - i) & (Nfft_big - 1)] = s->h_td[i];   // :100-106 with the longer block
    if (int rc = fc_spectrum(s->st_big, img.data(), 1, Nfft_big, 1.0f / (float)Nfft_big, s->d_Hc_big, nullptr)) return rc;
    s->Nfft_big = Nfft_big;
    return 0;
}

static int fc_ensure_part(FastConv* s, bool capturing) {
    const int P = (s->filterLen + PART_B - 1) / PART_B;
    if (s->part_P == P && s->d_Hp) return 0;
    if (capturing) return fc_refuse_capture("the partition spectra");
    const int Nfft = 2 * PART_B;
    if (!s->st_part) s->st_part = pffft_new_setup(Nfft, PFFFT_REAL);
    if (!s->st_part) { g_last_error = "pffastconv: internal setup failed"; return (int)hipErrorInvalidValue; }
    // correlation image of partition p (src/pffastconv.c:100-106 with the partition's taps): g[(Nfft - i) mod Nfft] = c[pB + i]
    std::vector<float> img((size_t)P * Nfft, 0.f);
    for (int i = 0; i < s->filterLen; ++i) img[(size_t)(i / PART_B) * Nfft + ((Nfft - i % PART_B) & (Nfft - 1))] = s->h_td[i];
    s->d_Hp.reset(); s->part_P = 0;
    if (int rc = fc_spectrum(s->st_part, img.data(), P, Nfft, 1.0f / (float)Nfft, s->d_Hp, nullptr)) return rc;
    s->part_P = P;
    return 0;
}

// the table a route names, built on first use
static int fc_ensure_table(FastConv* s, const FirRoute& r, bool capturing) {
    switch (r.table) {
        case FT_BIG: return fc_ensure_big(s, r.block, capturing);
        case FT_PART: return fc_ensure_part(s, capturing);
        case FT_TD:
            if (s->d_td) return 0;
            if (capturing) return fc_refuse_capture("the time-domain taps");
            if (int rc = s->d_td.grow(sizeof(float) * s->h_td.size())) return rc;
            PF_CHECK(hipMemcpy(s->d_td.get(), s->h_td.data(), sizeof(float) * s->h_td.size(), hipMemcpyHostToDevice));
            return 0;
        default: return 0;   // FT_REF: fc_ensure_device built it
    }
}

// ---- the launchers: one FirCall each (pf_host.h; those of the 16384-sample and few-block kernels: dma_tu.hip) ---------------------------
template <class C>
static int fc_launch_fused(Setup* ps, const float* d_Hc, const FirCall& c) {
    auto k = fastconv_fused_kernel<C>;
    size_t resident = 0;
    if (int rc = loop_resident(k, C::WG_THREADS, C::LDS_BYTES, &resident)) return rc;
    ps = for_device(ps);
    const LoopLaunch ll = loop_take(ps, c.st, resident, ((size_t)c.nblk * c.fb.nsig + C::T_PER_WG - 1) / C::T_PER_WG, 0);
    hipLaunchKernelGGL(k, dim3(ll.grid), dim3(C::WG_THREADS), C::LDS_BYTES, c.st, c.x, c.y, (const cx<float>*)d_Hc,
                       c.nblk, c.step, c.inputLen, c.lastOut, ps->d_tw.as<cx<float>>(), ps->d_twr.as<cx<float>>(), ll.ctr,
                       c.fb.nsig, c.fb.xstride, c.fb.ystride);
    PF_CHECK(hipGetLastError());
    return 0;
}
static int (*const FIR_FUSED_LAUNCH[])(Setup*, const float*, const FirCall&) = {   // in the order of FirFused
    fc_launch_fused<FirCfg::C512>, fc_launch_fused<FirCfg::C1024>, fc_launch_fused<FirCfg::C2048>, fc_launch_fused<FirCfg::C2048m>,
    fc_launch_fused<FirCfg::C4096>, fc_launch_fused<FirCfg::C4096m>, fc_launch_fused<FirCfg::C8192>};

// The task split of the one-wavefront-per-block kernels (fft_fir.h: wave, partitioned), on at most the resident workgroups:
// runs of consecutive output blocks per wavefront task: ~2 tasks per wavefront (measured on 2^26 samples: runs of 8-16
// blocks 0.34, 4: 0.32, 32: 0.30, 64: 0.22; on 256 signals of 2^20: 32-64 best — both ~1.3-2.7 tasks per wavefront; the
// first loads of a run are not prefetched), never so short that filling the ring (P - 1 extra forward transforms per
// run) costs more than ~10 %
struct FirTasks { int kchunk; unsigned grid; };
static FirTasks fir_wave_tasks(int per_cu, int T_PER_WG, int nblk, int nsig, long kchunk_min, long forced) {
    const long wgs = (long)num_cus() * per_cu, waves = wgs * T_PER_WG;
    long kchunk = ((long)nblk * nsig + 2 * waves - 1) / (2 * waves);
    if (kchunk < kchunk_min) kchunk = kchunk_min;
    if (forced > 0) kchunk = forced;
    if (kchunk > nblk) kchunk = nblk;
    const long ntask = ((nblk + kchunk - 1) / kchunk) * nsig;
    return {(int)kchunk, (unsigned)std::min((ntask + T_PER_WG - 1) / T_PER_WG, wgs)};
}

// one launch of such a kernel on P partitions; `step`: the block step, of the kernel that takes one (the partitioned kernel's is PART_B)
template <class K, class... Step>
static int fc_launch_waves(FastConv* s, K k, int P, const FirCall& c, long kchunk_min, long forced, Step... step) {
    typedef FirPartCfg::C1024 C;
    const size_t lds = ((size_t)C::T_PER_WG * C::IMG + (size_t)P * C::E * 2 * 64) * sizeof(cx<float>);
    int rc = allow_big_lds(k, lds), per_cu = 0;
    if (!rc) rc = cached_occupancy(reinterpret_cast<const void*>(k), C::WG_THREADS, lds, &per_cu);
    if (rc) return rc;
    const FirTasks t = fir_wave_tasks(per_cu, C::T_PER_WG, c.nblk, c.fb.nsig, kchunk_min, forced);
    Setup* ps = for_device(s->st_part);
    hipLaunchKernelGGL(k, dim3(t.grid), dim3(C::WG_THREADS), lds, c.st, c.x, c.y, s->d_Hp.as<cx<float>>(), c.nblk, step..., c.inputLen,
                       c.lastOut, t.kchunk, ps->d_tw.as<cx<float>>(), ps->d_twr.as<cx<float>>(), c.fb.nsig, c.fb.xstride, c.fb.ystride);
    PF_CHECK(hipGetLastError());
    return 0;
}
#ifdef PFFFT_HIP_VARIANTS
template <int P, int OCC>
static int fc_launch_part(FastConv* s, const FirCall& c) {
    return fc_launch_waves(s, fastconv_part_kernel<FirPartCfg::C1024, P, OCC>, P, c, std::max(10 * (P - 1), 8), dev_env("PFFASTCONV_HIP_PART_K", 0));
}
static int (*const FIR_PART_LAUNCH[])(FastConv*, const FirCall&) = {fc_launch_part<1, 3>, fc_launch_part<2, 2>, fc_launch_part<3, 1>, fc_launch_part<4, 1>};
#endif

// time domain (fft_firtd.h): the route's blocks are tiles of the float stream; stride 2 on two real streams counts the input in floats too
static int fc_launch_td(FastConv* s, const FirCall& c, int stride) {
    const int flen8 = (int)s->h_td.size();
    auto k = stride == 2 ? fastconv_td_kernel<2> : fastconv_td_kernel<1>;
    const long out_f = (long)(c.nblk - 1) * TD_TILE + c.lastOut, in_f = (stride == 2 && s->cplxFactor == 1) ? 2L * c.inputLen : c.inputLen;
    const size_t lds = sizeof(float) * (TD_TILE + stride * flen8 + 8);
    // the signal index is blockIdx.y (<= 65535): longer batches go out in slices of 65535 signals on the same stream
    for (int s0 = 0; s0 < c.fb.nsig; s0 += 65535) {
        const int ns = c.fb.nsig - s0 < 65535 ? c.fb.nsig - s0 : 65535;
        const dim3 grid((unsigned)c.nblk, (unsigned)ns);
        const float* xs = c.x + (size_t)s0 * c.fb.xstride;
        float* ys = c.y + (size_t)s0 * c.fb.ystride;
        hipLaunchKernelGGL(k, grid, dim3(TD_THREADS), lds, c.st, xs, ys, s->d_td.as<float>(), flen8, out_f, in_f, c.fb.xstride, c.fb.ystride);
    }
    PF_CHECK(hipGetLastError());
    return 0;
}

// composed path: signal by signal on the same stream through one work image
static int fc_launch_composed(FastConv* s, const FirCall& c) {
    const int Nfft = s->Nfft, nblk = c.nblk, mode = ((s->flags & PFFASTCONV_HIP_CPLX_INP_OUT) && s->cplxFactor == 1) ? 1 : 0;
    void* buf = nullptr;   // (never grown while the stream records: a replay runs on the pointer it froze; outgrown later, it is retired)
    int rc = scratch_buffer(s->work, c.st, sizeof(float) * (size_t)nblk * Nfft, "pffastconv: the work image", &buf);
    if (rc) return rc;
    float* const d_work = (float*)buf;
    const unsigned grid = (unsigned)std::min<size_t>(((size_t)nblk * Nfft + 255) / 256, (size_t)num_cus() * 16);
    for (int sig = 0; sig < c.fb.nsig; ++sig) {
        const float* xs = c.x + (size_t)sig * c.fb.xstride;
        float* ys = c.y + (size_t)sig * c.fb.ystride;
        hipLaunchKernelGGL(fastconv_gather_kernel, dim3(grid), dim3(256), 0, c.st, xs, d_work, nblk, Nfft, c.step, c.inputLen, mode);
        PF_CHECK(hipGetLastError());
        if ((rc = transform_batch<float>(s->st, d_work, d_work, nblk, PFFFT_FORWARD, 0, c.st))) return rc;                         // :235
        if ((rc = zconvolve_batch<float>(s->st, d_work, s->d_Hf.as<float>(), d_work, s->scale, nblk, 0, 1, c.st))) return rc;      // :238
        if ((rc = transform_batch<float>(s->st, d_work, d_work, nblk, PFFFT_BACKWARD, 0, c.st))) return rc;                        // :254
        hipLaunchKernelGGL(fastconv_scatter_kernel, dim3(grid), dim3(256), 0, c.st, d_work, ys, nblk, Nfft, c.step, c.lastOut, mode);
        PF_CHECK(hipGetLastError());
    }
    return 0;
}

static int fc_apply_device(FastConv* s, const float* d_x, int cplxInputLen, float* d_y, int flush, hipStream_t st,
                           int* produced_out, const FcBatch& fb = FcBatch{1, 0, 0}) {
    std::lock_guard<std::mutex> lk(s->mu);
    const bool capturing = stream_capturing(st);
    int rc = fc_ensure_device(s, capturing);
    if (rc) return rc;
    const FirRoute r = fir_route(*s, cplxInputLen, fb.nsig, flush, num_cus(), ab(), env(), g_fir_wave_min, g_fir_wave_max);
    *produced_out = r.produced / s->cplxFactor;  // :200 / :261
    if (r.kind == FIR_NONE) return 0;
    if ((rc = fc_ensure_table(s, r, capturing))) return rc;
    const FirCall c{d_x, d_y, r.blocks, r.step, s->cplxFactor * cplxInputLen, r.last, st, fb};
    const bool big = r.table == FT_BIG;
    Setup* const ps = big ? s->st_big : s->st;
    const float* const Hc = (big ? s->d_Hc_big : s->d_Hc).as<float>();
    auto launch = [&]() -> int {
        switch (r.kind) {
            case FIR_TD: return fc_launch_td(s, c, r.cfg);
            // one wavefront per 2048-sample block, step = 2048 - taps + 1 (fft_fir.h fastconv_wave_kernel): filters up to 1024 taps
            case FIR_WAVE: return fc_launch_waves(s, fastconv_wave_kernel<FirPartCfg::C1024, 3>, 1, c, 4, 0, c.step);
            case FIR_FIR32: return launch_fir32(ps, Hc, c, big ? s->d_fir32_hp : s->d_fir32_hp_ref, r.cfg);
            case FIR_SPLIT: return launch_fir_split(ps, Hc, c, r.cfg == 0);
            case FIR_SPLIT1: return launch_fir_split1(ps, Hc, c, s->d_split1_ab);
            case FIR_GATHER: return fc_launch_composed(s, c);
            case FIR_FUSED: return FIR_FUSED_LAUNCH[r.cfg](ps, Hc, c);
#ifdef PFFFT_HIP_VARIANTS
            case FIR_DMA: return launch_fir_dma(ps, Hc, c);
            case FIR_PART: return FIR_PART_LAUNCH[r.cfg - 1](s, c);
#endif
            default: break;
        }
        return bad("pffastconv: the route names a kernel this build does not have");
    };
    rc = launch();
    if (!rc && capturing) { s->recorded = true; s->recorded_big |= big; }   // (a refused call recorded nothing)
    return rc;
}

}  // namespace pf

struct PFFASTCONV_Setup : pf::FastConv {};

PF_EXPORT PFFASTCONV_Setup* pffastconv_new_setup(const float* filterCoeffs, int filterLen, int* blockLen, int flags) {
    using namespace pf;
    // src/pffastconv.c:61-82
    const int cplxFactor = ((flags & PFFASTCONV_HIP_CPLX_INP_OUT) && (flags & PFFASTCONV_HIP_CPLX_SINGLE_FFT)) ? 2 : 1;
    const int minFftLen = 2 * SIMD * SIMD;
    if (!filterCoeffs || filterLen <= 0 || !blockLen) return nullptr;
    int Nfft = 2 * next_pow2(filterLen - 1);
    if (Nfft < minFftLen) Nfft = minFftLen;
    if (flags & PFFASTCONV_HIP_CPLX_FILTER) return nullptr;  // :71-72 "not implemented yet"
    if (*blockLen > Nfft) Nfft = next_pow2(*blockLen);
    *blockLen = Nfft;
    Nfft *= cplxFactor;
    PFFFT_Setup* st = pffft_new_setup(Nfft, PFFFT_REAL);
    if (!st) return nullptr;
    PFFASTCONV_Setup* s = new PFFASTCONV_Setup();
    s->magic = FC_MAGIC;
    s->st = st;
    s->filterLen = cplxFactor == 2 ? 2 * filterLen - 1 : filterLen;
    s->Nfft = Nfft; s->flags = flags; s->cplxFactor = cplxFactor;
    s->scale = (float)(1.0 / Nfft);
    s->h_filter_image.assign(Nfft, 0.f);
    s->h_td.assign((size_t)(filterLen + 7) / 8 * 8, 0.f);
    for (int i = 0; i < filterLen; ++i) {  // :100-106
        float c = (flags & PFFASTCONV_HIP_CORRELATION) ? filterCoeffs[i] : filterCoeffs[filterLen - 1 - i];
        s->h_filter_image[(Nfft - cplxFactor * i) & (Nfft - 1)] = c;
        s->h_td[i] = c;
    }
    return s;
}

PF_EXPORT void pffastconv_destroy_setup(PFFASTCONV_Setup* s) {
    if (!s) return;
    pffft_destroy_setup(s->st);
    if (s->st_big) pffft_destroy_setup(s->st_big);
    if (s->st_part) pffft_destroy_setup(s->st_part);
    s->magic = 0;
    delete s;
}

PF_EXPORT int pffastconv_hip_apply_device(PFFASTCONV_Setup* s, const float* d_input, int inputLen, float* d_output,
                                          int applyFlush, void* stream) {
    return pffastconv_hip_apply_batch(s, d_input, inputLen, 0, d_output, 0, 1, applyFlush, stream);   // (one signal: no strides to check)
}

PF_EXPORT int pffastconv_hip_apply_batch(PFFASTCONV_Setup* s, const float* d_input, int inputLen, size_t inputStride,
                                         float* d_output, size_t outputStride, int nsignals, int applyFlush, void* stream) {
    if (!s || s->magic != pf::FC_MAGIC || nsignals < 0) return -1;
    const size_t cpl = (s->flags & PFFASTCONV_HIP_CPLX_INP_OUT) ? 2 : 1, fl = (size_t)inputLen * cpl;
    if (nsignals > 1 && (inputStride < fl || outputStride == 0)) { pf::g_last_error = "pffastconv_hip_apply_batch: stride smaller than a signal"; return -1; }
    int produced = 0;
    if (nsignals != 1) {
        int lastOut = 0;
        (void)pf::fc_schedule(*s, s->cplxFactor * inputLen, applyFlush, &lastOut, &produced);
        produced /= s->cplxFactor;
        // rows of the output must not overlap: outputStride >= the floats one signal produces
        if (nsignals > 1 && outputStride < (size_t)produced * cpl) { pf::g_last_error = "pffastconv_hip_apply_batch: outputStride smaller than the samples one signal produces"; return -1; }
        if (nsignals == 0) return produced;   // nothing to do, but the count a call would produce is still defined
    }
    int rc = pf::fc_apply_device(s, d_input, inputLen, d_output, applyFlush, (hipStream_t)stream, &produced,
                                 pf::FcBatch{nsignals, inputStride, outputStride});
    return rc ? -1 : produced;
}

PF_EXPORT int pffastconv_hip_route(const PFFASTCONV_Setup* s, int inputLen, int nsignals, int applyFlush, int cus, char* buf, size_t len) {
    using namespace pf;
    if (!s || s->magic != FC_MAGIC || !buf) return -1;
    const FirRoute r = nsignals > 0 ? fir_route(*s, inputLen, nsignals, applyFlush, cus > 0 ? cus : num_cus(), ab(), env(), g_fir_wave_min, g_fir_wave_max) : FirRoute{};
    const char* const tab = r.table == FT_BIG ? "big" : "ref";
    char text[96] = "", cfg[16] = "";
    switch (r.kind) {
        case FIR_TD: case FIR_PART: case FIR_SPLIT1: snprintf(cfg, sizeof cfg, "%s%d", r.kind == FIR_TD ? "" : r.kind == FIR_PART ? "P" : "W", r.cfg); break;
        case FIR_FIR32: snprintf(cfg, sizeof cfg, "%s%s", tab, r.cfg == 2 ? "" : r.cfg == 1 ? "-pf1" : "-nopf"); break;
        case FIR_DMA: case FIR_SPLIT: snprintf(cfg, sizeof cfg, "%s%s", tab, r.kind == FIR_SPLIT && !r.cfg ? "-plain" : ""); break;
        case FIR_FUSED: snprintf(cfg, sizeof cfg, "%s", FIR_FUSED_NAME[r.cfg]); break;
        default: break;
    }
    if (r.kind != FIR_NONE) snprintf(text, sizeof text, "%s %s %d %d %d %d", FIR_KERNEL[r.kind], cfg, r.block, r.step, r.blocks, r.last);
    const size_t n = strlen(text);
    if (n + 1 > len) return -1;
    memcpy(buf, text, n + 1);
    return (int)n;
}

// Host pointers (the reference's calling convention): up to FC_ZC_LIMIT bytes per signal there is no DMA copy — the signal
// is copied by the CPU into a pinned host image that the kernel reads over PCIe directly, the kernel writes its outputs
// into another pinned image, one stream synchronisation, CPU copy out (the same scheme as the transform entries,
// abi_tu.hip legacy_run).  Larger signals are staged through device buffers.  Failure: fail-soft like the transform
// entries (stderr, pffft_hip_last_error(), error counter) and the return value -1, abort() only under PFFFT_HIP_ABORT=1.
PF_EXPORT int pffastconv_apply(PFFASTCONV_Setup* s, const float* input, int cplxInputLen, float* output, int applyFlush) {
    using namespace pf;
    if (!s || s->magic != FC_MAGIC) {
        g_last_error = "pffastconv_apply: bad setup";
        legacy_fatal((int)hipErrorInvalidHandle, "pffastconv_apply", nullptr, 0, true);
        return -1;
    }
    constexpr size_t FC_ZC_LIMIT = (size_t)64 << 20;
    const bool in_dev = is_device_ptr(input), out_dev = is_device_ptr(output);
    const int cpl = (s->flags & PFFASTCONV_HIP_CPLX_INP_OUT) ? 2 : 1;
    const size_t in_floats = (size_t)cplxInputLen * cpl;
    const size_t stage_bytes = (in_floats ? in_floats : 1) * sizeof(float);
    const float* d_in = input; float* d_out = output;
    int rc = 0, produced = 0;
    const bool zc = zero_copy_enabled() && in_floats * sizeof(float) <= FC_ZC_LIMIT;
    bool out_pinned = false;
    do {
        if (!in_dev) {
            if (zc && s->h_x.grow(stage_bytes) == 0) {
                if (in_floats) memcpy(s->h_x.get(), input, in_floats * sizeof(float));
                d_in = s->h_x.as<float>();
            } else {
                if ((rc = s->d_x.grow(stage_bytes))) break;
                if (in_floats && hipMemcpy(s->d_x.get(), input, in_floats * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { rc = -1; break; }
                d_in = s->d_x.as<float>();
            }
        }
        if (!out_dev) {
            if (zc && s->h_y.grow(stage_bytes) == 0) { d_out = s->h_y.as<float>(); out_pinned = true; }
            else {
                if ((rc = s->d_y.grow(stage_bytes))) break;
                d_out = s->d_y.as<float>();
            }
        }
        if ((rc = fc_apply_device(s, d_in, cplxInputLen, d_out, applyFlush, nullptr, &produced))) break;
        if (!out_dev && !out_pinned) {
            if (produced > 0 && hipMemcpy(output, d_out, (size_t)produced * cpl * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) { rc = -1; break; }
        } else {
            if (hipStreamSynchronize(nullptr) != hipSuccess) { rc = -1; break; }
            if (out_pinned && produced > 0) memcpy(output, d_out, (size_t)produced * cpl * sizeof(float));
        }
    } while (0);
    if (rc) {
        // The reference cannot fail here.  Fail soft: NaN over the part of `output` the reference's contract guarantees to be
        // writable - inputLen - filterLen + 1 samples (include/pffft/pffastconv.h:159), never the whole input length - and
        // -1 as the return value: 0 would be indistinguishable from "not enough input yet" and a streaming loop waiting for
        // progress would spin forever (documented in include/pffft_hip.h).
        const int taps = s->cplxFactor == 2 ? (s->filterLen + 1) / 2 : s->filterLen;   // the caller's filter length
        const long writable = (long)cplxInputLen - taps + 1;
        legacy_fatal(rc, "pffastconv_apply", output, writable > 0 ? (size_t)writable * cpl * sizeof(float) : 0, !out_dev);
        return -1;
    }
    return produced;
}

PF_EXPORT void* pffastconv_malloc(size_t nb) { return pf::aligned_malloc64(nb); }
PF_EXPORT void pffastconv_free(void* p) { pf::aligned_free64(p); }
PF_EXPORT int pffastconv_simd_size(void) { return pf::SIMD; }
