// The planner's records: what runs for a (setup, direction, layout), decided ONCE at pffft_new_setup and stored in the setup
// (round 5: the decisions used to be re-derived per call from ~60 scattered tests of an integer selector and ~40 environment
// reads).  Three pieces:
//   Env    every environment switch of the product build, read once;
//   AbSel  the A/B selector of pffft_hip_set_variant() decoded into named flags - the alternatives that still exist because a test
//          holds two independent routes to one answer; the measured-and-lost ones are gone from the product build;
//   Route  kernel family + configuration + launch rule per (direction, layout); pffft_hip_describe() prints it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>

namespace pf {

// ------------------------------------------------------------------------------------------------ environment
// The product build reads exactly these names (once, at first use).  Development builds (-DPFFFT_HIP_VARIANTS) keep further tuning
// knobs behind dev_env(): in the product build that is a constant.
struct Env {
    bool abort_on_error;   // PFFFT_HIP_ABORT=1        legacy void entries abort() instead of failing soft
    bool zero_copy;        // PFFFT_HIP_NO_ZEROCOPY=1  host-pointer calls through device staging instead of pinned images
    int oneshot;           // PFFFT_HIP_ONESHOT=<k>    launches of up to k groups per resident workgroup run one group per workgroup in
                           //                          dispatch order instead of the persistent in-order loop (default 4, 0 = never)
    int c1024_rounds;      // PFFFT_HIP_C1024_ONCE=<r> N = 1024 float: up to r resident sets of wavefronts as one transform per wavefront (0 = never)
    int tile_plans;        // PFFFT_HIP_TILE_PLANS=0   no run-time mixed-radix tile plans (fft_tileg.h): those sizes take the streaming passes
    const char* tile_force;  // PFFFT_HIP_TILE_FORCE="L1[g],L2[g]"  the two tile lengths of the sizes they multiply to (tests)
    int fir_nfft;          // PFFASTCONV_HIP_NFFT=<n>  internal block length of the throughput regime (0 = the reference's, -1 = planner)
    int fir_xcd;           // PFFASTCONV_HIP_XCD=0     split FIR kernels without the XCD-contiguous block ranges
};
const Env& env();

#ifdef PFFFT_HIP_VARIANTS
inline int dev_env(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
#else
constexpr int dev_env(const char*, int dflt) { return dflt; }
#endif

// ------------------------------------------------------------------------------------------------ A/B selector
// pffft_hip_set_variant(v), thread-local.  0 = the planner's routes.  The values that remain select an ALTERNATIVE ROUTE to the same
// result that a parity test compares with the default one (tests/test_gpu_*.py), or a development-build twin.
enum AbValue : int {
    AB_DEFAULT = 0,
    AB_INORDER_SMALL = 42,      // Stockham / zreorder / zconvolve kernels: in-order chunks where the default is a static stride
    AB_STATIC_LARGE = 43,       // Stockham: static stride where the default pulls in order
    AB_STOCK_FOR_TILED = 50,    // the Stockham plan also for the sizes that have a register-tiled kernel (and N = 1024 float)
    AB_STOCK_WORKGROUP = 52,    // (development build) workgroup-phase Stockham kernel where the wave-local one applies
    AB_STOCK_RUNTIME = 53,      // (development build) run-time-plan Stockham kernels
    AB_STOCK_DF_ON = 54,        // (development build) direct-first-stage twin of every Stockham plan
    AB_STOCK_DF_OFF = 55,       // (development build) deposit twin of every plan
    AB_AUX_DIRECT = 60,         // zreorder / zconvolve: the direct grid-stride kernels; shift + FFT as two passes
    AB_AUX_NO_STREAM = 61,      // zreorder / zconvolve: no in-order streaming kernel
    AB_BIG_STRIDED = 80,        // beyond LDS: the balanced two-pass strided kernels
    AB_BIG_NO_TILES = 82,       // beyond LDS: never the tile passes (three / five streaming sweeps)
    AB_BIG_NO_MR_TILES = 83,    // beyond LDS: tile passes for power-of-two n only (the route the mixed-radix plans replaced)
    AB_BIG_SEPARATE_LAYOUT = 86,  // beyond LDS: the internal layout through its own sweep instead of fused into the first / last pass
    AB_BIG_SEPARATE_SWEEPS = 87,  // beyond LDS: zreorder kernel + in-place pair pass instead of the one-sweep block kernels
    AB_FIR_PARTITIONED = 88,    // (development build) uniformly partitioned FIR kernel
    AB_NO_TINY = 91,            // n = 16 / 32 on the Stockham plan instead of one thread per transform
    AB_FIR_LOCKSTEP = 97,       // (development build) 16384-sample FIR blocks on the lock-step LDS-DMA kernel
    AB_FIR_FEW_16PT = 114,      // (development build) few-block FIR: 16 points per thread
    AB_FIR_FEW_LOCKSTEP = 115,  // few-block FIR: the lock-step kernel on 512 / 256 threads instead of the split one
    AB_FIR_SPLIT_PLAIN = 116,   // (development build) split FIR kernel with plain barriers / pieces at once
    AB_FIR_FUSED32_PF1 = 117,   // (development build) 16384-sample FIR blocks, fft_fir32.h: the next block requested at once after the product
    AB_FIR_FUSED32_NOPF = 118,  // (development build) ... after the output stores
    AB_FIR_SPLIT = 119,         // 16384-sample FIR blocks on the split kernel (fft_split.h) that fft_fir32.h replaced in round 6
    AB_CONV_COMPOSED = 120,     // pffft_hip_convolve_batch as the three batched entries
    AB_RFFT_THREE = 121,        // real transforms beyond LDS: always complex core + pair sweep
    AB_RFFT_TWO = 122,          // real transforms beyond LDS: two sweeps wherever the length splits
    AB_NO_ONE_IMAGE = 123,      // the sizes of the single-image kernel (fft_one.h) on the tile / streaming passes they ran on before round 6
    AB_FRAMES_COMPOSED = 124,   // pffft_hip_frames_transform_batch: framing kernel + transform_batch through the frame matrix
    AB_FRAMES_FUSED = 125,      // ... the framed register-tiled kernel wherever it is legal, whatever the measured default of the cell is
    AB_PFB_COMPOSED = 126,      // pffft_hip_pfb_transform_batch: folding kernel + transform_batch through the frame matrix
    AB_PFB_FUSED = 127,         // ... the folding complex N = 1024 kernel wherever it is legal, whatever the measured default of the cell is
    AB_PFB_SYN_SCALAR = 128,    // pffft_hip_pfb_synthesis_batch: the scalar form of the gather also where the wide one is legal (same arithmetic)
    AB_PFB_SYN_PLAIN = 129,     // ... the gather's tiles on the plain grid stride, whatever the measured default is (same arithmetic)
    AB_PFB_SYN_XCD = 131,       // ... the gather's tiles in XCD-contiguous sweeps, whatever the measured default is (same arithmetic)
    AB_ANY_COMPOSED = 132,      // pffft_hip_any_transform_batch: never the fused chirp kernel (pad kernel + convolve_batch + crop kernel)
    AB_ANY_FUSED = 133,         // ... the fused chirp kernel wherever it is legal (today the default in every legal cell)
    AB_PSD_COMPOSED = 134,      // pffft_hip_frames_psd_batch: framing kernel + transform_batch + run kernel through the frame matrix
    AB_PSD_FUSED = 135,         // ... the accumulating framed kernel wherever it is legal, whatever the measured default of the size is
    AB_ZOOM_COMPOSED = 136,     // pffft_hip_zoom_transform_batch: never the fused zoom kernel (pad kernel + convolve_batch + crop kernel)
    AB_ZOOM_FUSED = 137,        // ... the fused zoom kernel wherever it is legal, whatever the measured default of the length is
    AB_DCT_COMPOSED = 138,      // pffft_hip_dct_transform_batch: never the fused kernel (permutation / table kernel + transform_batch + its twin)
    AB_DCT_FUSED = 139,         // ... the fused register-tiled kernel wherever it is legal, whatever the measured default of the (size, kind) is
    AB_MDCT_COMPOSED = 140,     // pffft_hip_mdct_*_batch: never the fused kernel (fold kernel + transform_batch + table / scatter kernel)
    AB_MDCT_FUSED = 141,        // ... the fused register-tiled kernel wherever it is legal, whatever the measured default of the (size, entry) is
    AB_CSD_COMPOSED = 142,      // pffft_hip_frames_csd_batch: framing kernel (x and y) + transform_batch + run kernel through the frame matrix
    AB_CSD_FUSED = 143,         // ... the two-pass accumulating framed kernel wherever it is legal, whatever the measured default of the cell is
    AB_ANALYTIC_COMPOSED = 144, // pffft_hip_analytic_transform_batch: never the fused kernel (widening kernel + convolve_batch + narrowing kernel)
    AB_ANALYTIC_FUSED = 145,    // ... the fused real-loading convolution kernel wherever it is legal, whatever the measured default of the (size, output) is
    AB_XCORR_COMPOSED = 146,    // pffft_hip_xcorr_batch: never the fused kernel (pad kernel + transform_batch + product kernel + transform_batch + crop kernel)
    AB_XCORR_FUSED = 147,       // ... the fused two-pass correlation kernel wherever it is legal, whatever the measured default of the cell is
    AB_FFT2_COMPOSED = 148,     // pffft_hip_fft2_transform_batch: never the fused kernel (transform_batch + transposing kernel + transform_batch + its twin)
    AB_FFT2_FUSED = 149,        // ... the fused LDS-resident 2-D kernel wherever it is legal, whatever the measured default of the shape is
    AB_RFFT2_COMPOSED = 150,    // pffft_hip_rfft2_transform_batch: never the fused kernel (real transform_batch + unpacking kernel + transform_batch + transposing kernel)
    AB_RFFT2_FUSED = 151,       // ... the fused LDS-resident 2-D real kernel wherever it is legal, whatever the measured default of the shape is
    AB_FFT2CONV_COMPOSED = 152, // pffft_hip_fft2_convolve_batch: never the fused kernel (the handle's forward transform + product kernel + its backward transform)
    AB_FFT2CONV_FUSED = 153,    // ... the fused LDS-resident 2-D convolution kernel wherever it is legal (float, one broadcast H), whatever the measured default of the shape is
    AB_RFFT2CONV_COMPOSED = 154, // pffft_hip_rfft2_convolve_batch: never the fused kernel (the handle's forward transform + product kernel + its backward transform)
    AB_RFFT2CONV_FUSED = 155,   // ... the fused LDS-resident 2-D real convolution kernel wherever it is legal (float, one broadcast H), whatever the measured default of the shape is
    AB_RESAMPLE_COMPOSED = 156, // pffft_hip_resample_batch: never the fused kernel (widening kernel + transform_batch at N + map kernel + transform_batch at M + narrowing kernel)
    AB_RESAMPLE_FUSED = 157,    // ... the fused two-length resampling kernel wherever it is legal (float, N != M from 512 ... 4096), whatever the measured default of the cell is
    AB_DCT2D_COMPOSED = 158,    // pffft_hip_dct2d_transform_batch: never the fused kernel (dct_transform_batch + real transposing kernel + dct_transform_batch + its twin)
    AB_DCT2D_FUSED = 159,       // ... the fused LDS-resident 2-D cosine kernel wherever it is legal (float, rows and cols 32 / 64), whatever the measured default of the (shape, kind) is
    AB_BANDS_COMPOSED = 160,    // pffft_hip_bands_batch: never the fused kernel (the inner setup's POWER rows into the handle's scratch + row kernel)
    AB_BANDS_FUSED = 161,       // ... the fused framed band kernel wherever it is legal (real float N = 1024 / 2048 / 4096), whatever the measured default of the size is
    AB_FAKE_DEVICE = 130,   // the calling thread counts as being on ANOTHER device than its current one (key + 64): exercises the per-device
                                // replicas of a shared setup on a box with one GPU (tests/test_gpu_round6.py)
};
struct AbSel {
    int raw = 0;
    bool is(AbValue v) const { return raw == (int)v; }
    bool any() const { return raw != 0; }
};
AbSel ab();   // the calling thread's selector

// ------------------------------------------------------------------------------------------------ routes
enum Family : uint8_t { FAM_NONE = 0, FAM_TINY, FAM_C1024, FAM_TILED, FAM_STOCK, FAM_BIG, FAM_ONE };
const char* family_name(Family f);

// launch rule of an LDS-resident kernel
enum LaunchRule : uint8_t {
    LR_DISPATCH,       // one group per workgroup (or wavefront), workgroups in hardware dispatch order
    LR_STATIC,         // persistent workgroups on a static stride
    LR_INORDER,        // persistent workgroups pull groups in order from a counter (first two groups static);
                       // launches of <= `oneshot` groups per resident workgroup run as LR_DISPATCH
};
const char* launch_rule_name(LaunchRule r);

// one kernel instantiation picked at run time: its pointer (type-erased over the configuration), dynamic LDS bytes, workgroup threads
// and vectors per workgroup
template <class Fn>
struct KernelSel {
    Fn fn = nullptr;
    size_t lds = 0;
    int wg = 0, t_per_wg = 0;
};

struct TiledSel : KernelSel<const void*> {   // a register-tiled configuration (fft_tiled.h), erased over the scalar type too
    const char* cfg = "";
};

struct StockSel {            // a Stockham plan on its compile-time kernel (fft_stock.h)
    const void* fn = nullptr;    // StockCtFn<T>; nullptr: run-time-plan kernel (development build) or none
    bool wl = false;             // wave-local organisation (vectors <= 4 KiB)
    bool df = false;             // direct first stage
    int threads = 0;
    size_t lds = 0;
    int flags = 0;
    int groups_per_wg = 0;       // measured table (stock_grid_gen.h); 0: the size rule (grid_mul x the resident set)
    int grid_mul = 1;
};

enum BigCore : uint8_t { BIG_TILES, BIG_RFFT2, BIG_STREAM, BIG_STRIDED };
struct BigPlan {             // n beyond LDS: the sweeps over HBM, in order
    BigCore core = BIG_STREAM;
    int tmode = 0;               // planner mode of the tile plans (tile_tu.hip): 0 complex, 1 deep, 2 core of a real transform
    int lens[3] = {0, 0, 0};     // tile lengths (BIG_TILES / BIG_RFFT2), {R, N2} (BIG_STREAM), {N1, N2} (BIG_STRIDED)
    int pre = -1;                // one-sweep block kernel BEFORE the core (fft_big.h big_block_kernel mode), -1 none:
                                 //   1 complex internal -> canonical, 3 real internal -> packed, 4 real canonical -> packed
    bool pre_separate = false;   // AB_BIG_SEPARATE_SWEEPS: zreorder kernel / copy + in-place pair pass instead
    bool fuse_in = false;        // the first tile pass reads the internal layout itself
    bool col_in = false;         // the column pass of the streaming route reads it
    bool fuse_out = false;       // the last pass (tile pass or transpose) stores the internal layout itself
    bool rfuse = false;          // real forward (round 6): the last tile pass carries the pair pass (fft_tile.h RMODE 3) - no pair sweep
    int post = -1;               // block kernel AFTER the core: 0 complex canonical -> internal, 2 real pair pass + internal, 5 permutation
    bool pair_after = false;     // real forward ordered: in-place pair pass on the result
    bool post_separate = false;  // AB_BIG_SEPARATE_SWEEPS: pair pass + zreorder kernel
    int sweeps = 0;              // passes over the whole vector set
};

// The (direction, layout, real) flag bits every LDS-resident family shares (fft_stock.h, fft_one.h, fft_tiled.h: the low two): 1 = backward
// FROM the internal layout, 2 = forward INTO it, 4 = backward, 8 = real.  dir: 0 forward, 1 backward (pffft_direction_t).
constexpr int layout_flags(int dir, int ordered, bool real) {
    return (!ordered ? (dir ? 1 : 2) : 0) | (dir ? 4 : 0) | (real ? 8 : 0);
}
static_assert(layout_flags(0, 1, false) == 0 && layout_flags(0, 0, false) == 2, "complex forward: canonical / into the layout");
static_assert(layout_flags(1, 1, false) == 4 && layout_flags(1, 0, false) == 5, "complex backward: canonical / from the layout");
static_assert(layout_flags(0, 1, true) == 8 && layout_flags(0, 0, true) == 10, "real forward");
static_assert(layout_flags(1, 1, true) == 12 && layout_flags(1, 0, true) == 13, "real backward");

// which of Setup::one[0..2] a flag set runs (fft_one.h): the float complex backward transform from the layout has a plan of its own
constexpr int one_plan_index(bool is_double, int flags) { return (flags == 5 && !is_double) ? 2 : (flags & 4) ? 1 : 0; }
static_assert(one_plan_index(false, 5) == 2 && one_plan_index(true, 5) == 1 && one_plan_index(false, 13) == 1, "the narrow plan: float complex only");
static_assert(one_plan_index(false, 2) == 0 && one_plan_index(false, 4) == 1 && one_plan_index(true, 10) == 0, "else the plan of the direction");

struct Route {
    Family fam = FAM_NONE;
    LaunchRule rule = LR_DISPATCH;
    int oneshot = 0;             // LR_INORDER: bound of the dispatch-order launch, groups per resident workgroup
    TiledSel tiled;
    StockSel stock;
    BigPlan big;
};

}  // namespace pf
