/* pffft_hip.h — C ABI of libpffft_hip.so, the MI355X (gfx950) drop-in for the pffft hot path.
 *
 * PART 1 declares, with identical names, argument meaning and error behaviour, every symbol the
 * reference exports for this path (reference headers: include/pffft/pffft.h:124-250,
 * include/pffft/pffft_double.h:124-246, include/pffft/pffastconv.h:145-180, plus the two
 * validate_* self-test entries the reference's test programs declare by hand,
 * tests/test_pffft.c:269-272).  A program compiled against the reference's own headers links
 * against libpffft_hip.so unchanged; this header exists so that the ABI is written down in this
 * repository (tests/test_abi.py checks that every name below is exported).
 *
 * PART 2 is the additive batched / device-pointer extension the throughput metric is measured on
 * (the reference API transforms one vector per call, include/pffft/pffft.h:159,168).
 *
 * Pointer rule for PART 1: `float*` / `double*` arguments may be ordinary host pointers (staged
 * through the device: correct, PCIe-bound) or device / managed pointers (used in place).  There is
 * no CPU arithmetic path in this library: without a usable HIP device (or on any HIP error) a
 * transform entry FAILS SOFT — one line on stderr, the output vector filled with NaN, the failure
 * counted in pffft_hip_error_count() and described by pffft_hip_last_error(); PFFFT_HIP_ABORT=1 in
 * the environment turns that into abort().  A call on an invalid handle (NULL, destroyed, wrong precision) writes
 * nothing.  `work` is accepted and ignored (reference: scratch of N / 2N scalars or NULL, include/pffft/pffft.h:137-142).
 *
 * COST OF THE LEGACY SINGLE-VECTOR ENTRIES.  One call = one kernel launch + one stream synchronisation: 17-29 us per call
 * with host pointers (N = 64 ... 16384; the reference's SSE path: 0.1-30 us), i.e. a program that links this library and
 * keeps calling pffft_transform() vector by vector runs 10-20 x SLOWER than on the CPU for N <= 4096.  The throughput of
 * this library is in PART 2 (batched entries on device-resident data): move the loop over vectors into `batch`.
 *
 * ACCURACY OF pffftd_* AGAINST THE REFERENCE.  The reference's double build keeps float-suffixed radix-3 / radix-5
 * constants (src/pffft_priv_impl.h:154,259-262,389,431-432,636-639 survive `#define float double`), so for every N with a
 * factor 3 or 5 the reference's own pffftd_* result is only ~1e-8 accurate.  This library uses full-precision constants:
 * for those sizes it agrees with a float64 DFT to 1e-12 and with the reference to ~1e-8 (tests: 2e-7); power-of-two sizes
 * agree with the reference to 1e-15.
 */
#ifndef PFFFT_HIP_H
#define PFFFT_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ PART 1: reference ABI ---- */

typedef struct PFFFT_Setup PFFFT_Setup;   /* include/pffft/pffft.h:106        */
typedef struct PFFFTD_Setup PFFFTD_Setup; /* include/pffft/pffft_double.h:111 */
typedef struct PFFASTCONV_Setup PFFASTCONV_Setup; /* include/pffft/pffastconv.h:81 */

#ifndef PFFFT_COMMON_ENUMS
#define PFFFT_COMMON_ENUMS
typedef enum { PFFFT_FORWARD, PFFFT_BACKWARD } pffft_direction_t; /* pffft.h:112 */
typedef enum { PFFFT_REAL, PFFFT_COMPLEX } pffft_transform_t;     /* pffft.h:115 */
#endif

/* float — src/pffft.c:101-129 maps these onto src/pffft_priv_impl.h */
PFFFT_Setup *pffft_new_setup(int N, pffft_transform_t transform);            /* impl :1062-1112; NULL on invalid N */
void pffft_destroy_setup(PFFFT_Setup *);                                     /* impl :1115-1120; NULL-safe */
void pffft_transform(PFFFT_Setup *, const float *in, float *out, float *work, pffft_direction_t);         /* :1816 */
void pffft_transform_ordered(PFFFT_Setup *, const float *in, float *out, float *work, pffft_direction_t); /* :1820 */
void pffft_zreorder(PFFFT_Setup *, const float *in, float *out, pffft_direction_t);                       /* :1158 */
void pffft_zconvolve_accumulate(PFFFT_Setup *, const float *a, const float *b, float *ab, float scaling); /* :1534 */
void pffft_zconvolve_no_accu(PFFFT_Setup *, const float *a, const float *b, float *ab, float scaling);    /* :1632 */
int pffft_simd_size(void);                                 /* :76  — always 4: selects the 4-lane internal layout */
const char *pffft_simd_arch(void);                         /* :116 — "HIP-gfx950" */
int pffft_min_fft_size(pffft_transform_t transform);       /* :78  */
int pffft_is_valid_size(int N, pffft_transform_t cplx);    /* :91  */
int pffft_nearest_transform_size(int N, pffft_transform_t cplx, int higher); /* :100 */
int pffft_next_power_of_two(int N);                        /* src/pffft_common.c:25 */
int pffft_is_power_of_two(int N);                          /* src/pffft_common.c:39 */
void *pffft_aligned_malloc(size_t nb_bytes);               /* src/pffft_common.c:12 — 64-byte aligned */
void pffft_aligned_free(void *);
int validate_pffft_simd(void);                             /* impl :2227 — layout self-test, 0 = ok */
int validate_pffft_simd_ex(void *dbg_file);                /* impl :1889 (FILE* or NULL) */

/* double — src/pffft_double.c:113-142 */
PFFFTD_Setup *pffftd_new_setup(int N, pffft_transform_t transform);
void pffftd_destroy_setup(PFFFTD_Setup *);
void pffftd_transform(PFFFTD_Setup *, const double *in, double *out, double *work, pffft_direction_t);
void pffftd_transform_ordered(PFFFTD_Setup *, const double *in, double *out, double *work, pffft_direction_t);
void pffftd_zreorder(PFFFTD_Setup *, const double *in, double *out, pffft_direction_t);
void pffftd_zconvolve_accumulate(PFFFTD_Setup *, const double *a, const double *b, double *ab, double scaling);
void pffftd_zconvolve_no_accu(PFFFTD_Setup *, const double *a, const double *b, double *ab, double scaling);
int pffftd_simd_size(void);
const char *pffftd_simd_arch(void);
int pffftd_min_fft_size(pffft_transform_t transform);
int pffftd_is_valid_size(int N, pffft_transform_t cplx);
int pffftd_nearest_transform_size(int N, pffft_transform_t cplx, int higher);
int pffftd_next_power_of_two(int N);
int pffftd_is_power_of_two(int N);
void *pffftd_aligned_malloc(size_t nb_bytes);
void pffftd_aligned_free(void *);
int validate_pffftd_simd(void);
int validate_pffftd_simd_ex(void *dbg_file);

/* fast convolution — src/pffastconv.c:58-263; flag values of include/pffft/pffastconv.h:83-134 */
enum {
  PFFASTCONV_HIP_CPLX_INP_OUT = 1, PFFASTCONV_HIP_CPLX_FILTER = 2, PFFASTCONV_HIP_DIRECT_INP = 4,
  PFFASTCONV_HIP_DIRECT_OUT = 8, PFFASTCONV_HIP_CPLX_SINGLE_FFT = 16, PFFASTCONV_HIP_SYMMETRIC = 32,
  PFFASTCONV_HIP_CORRELATION = 64
};
PFFASTCONV_Setup *pffastconv_new_setup(const float *filterCoeffs, int filterLen, int *blockLen, int flags);
void pffastconv_destroy_setup(PFFASTCONV_Setup *);
/* Returns the number of output samples produced, as the reference does (src/pffastconv.c:133-263).  ADDITION: -1 when the
 * HIP path failed (no device, HIP error, invalid setup) - the reference cannot fail here, and 0 would be indistinguishable
 * from "not enough input yet" for a streaming caller.  On failure at most inputLen - filterLen + 1 samples of `output`
 * (what include/pffft/pffastconv.h:159 guarantees to be writable) are filled with NaN. */
int pffastconv_apply(PFFASTCONV_Setup *, const float *input, int inputLen, float *output, int applyFlush);
void *pffastconv_malloc(size_t nb_bytes);
void pffastconv_free(void *);
int pffastconv_simd_size(void);

/* ------------------------------------------------- PART 2: batched / device extension -------- */
/* Concurrency bounds of the batched entries.  (i) ONE SETUP, ANY DEVICE (round 6): a PFFFT_Setup / PFFFTD_Setup is immutable and may
 * be shared by concurrent threads like the reference's (include/pffft/pffft.h:102-105) - also by threads whose current HIP devices
 * differ: the twiddle tables, work counters, per-stream scratch and staging buffers are kept per device (built on a device's first
 * call under the setup's mutex, released by destroy_setup; pffft_hip_setup_devices lists them).  The pointers of a call must be usable on
 * the calling thread's current device.  A PFFASTCONV_Setup - not shareable between threads in the reference either
 * (include/pffft/pffastconv.h:77-80) - holds its filter tables on ONE device and rebuilds them when its user's device changes.
 * (ii) Kernels that
 * pull their work in order draw a {next, done} counter pair from a ring of 4096 pairs per setup and re-arm it
 * when they retire: at most 4096 launches of ONE setup may be in flight at the same time (summed over all
 * streams).  Launches on one stream serialise, so only > 4096 concurrently RUNNING launches could collide.
 * (iii) Scratch of the sizes beyond LDS is kept per stream: the same setup may run on several streams at once.
 * (iv) STREAM CAPTURE.  A setup's device state is built at its first call on a device (hipMalloc, hipMemset, hipMemcpy): never while
 * `stream` records into a HIP graph.  A call on a capturing stream whose setup holds no state on the calling thread's device yet returns
 * hipErrorStreamCaptureUnsupported ("the tables of this setup would have to be built during graph capture") before anything is allocated
 * or launched, and leaves the setup as it was (pffft_hip_setup_devices does not list that device): run the call once before capturing,
 * per device.  The same holds for a PFFASTCONV_Setup, whose tables are per ROUTE (see pffastconv_hip_apply_batch), and once a graph has
 * recorded a launch of one, that setup no longer follows its user to another device: the graph reads its tables where they are.
 *
 * All return 0 on success, otherwise a hipError_t value (pffft_hip_last_error() has the text).
 * `in`, `out`, `a`, `b`, `ab` are DEVICE pointers to `batch` contiguous vectors (N scalars for a
 * real setup, 2N for a complex one), 16-byte (float) / 32-byte (double) aligned.  `stream` is a
 * hipStream_t (NULL = default stream).  Calls are asynchronous with respect to the host.  in == out
 * is allowed for the transforms (include/pffft/pffft.h:157) and all of a/b/ab may alias for
 * zconvolve (:194); zreorder needs in != out (:180).
 *   ordered = 0 -> pffft_transform semantics (spectrum in the internal layout)
 *   ordered = 1 -> pffft_transform_ordered semantics (canonical interleaved spectrum) */
int pffft_hip_transform_batch(PFFFT_Setup *, const float *in, float *out, size_t batch,
                              pffft_direction_t direction, int ordered, void *stream);
int pffft_hip_zreorder_batch(PFFFT_Setup *, const float *in, float *out, size_t batch,
                             pffft_direction_t direction, void *stream);
/* ab[i] (+)= a[i] * b[i or 0] * scaling; b_broadcast != 0 reuses ONE spectrum b for every vector
 * (the FIR case, src/pffastconv.c:238) */
int pffft_hip_zconvolve_batch(PFFFT_Setup *, const float *a, const float *b, float *ab, float scaling,
                              size_t batch, int accumulate, int b_broadcast, void *stream);

int pffftd_hip_transform_batch(PFFFTD_Setup *, const double *in, double *out, size_t batch,
                               pffft_direction_t direction, int ordered, void *stream);
int pffftd_hip_zreorder_batch(PFFFTD_Setup *, const double *in, double *out, size_t batch,
                              pffft_direction_t direction, void *stream);
int pffftd_hip_zconvolve_batch(PFFFTD_Setup *, const double *a, const double *b, double *ab, double scaling,
                               size_t batch, int accumulate, int b_broadcast, void *stream);

/* Batch shards over several devices from ONE host thread (round 5; SURVEY.md 8(e): the batch shards with no exchange step).  Part p -
 * batches[p] vectors at in[p] / out[p], device memory of devices[p] - is transformed by setups[p] on devices[p]: hipSetDevice, then the
 * batched entry on streams[p] (streams == NULL or streams[p] == NULL: that device's default stream).  Every launch is asynchronous, so the
 * devices work concurrently; the caller's current device is restored before the call returns.  setups[p] may be THE SAME SETUP in every
 * slot (round 6: a setup keeps its device state per device, above) or a setup per part.  Returns the first error, 0 when every part is
 * enqueued.  The reference has no counterpart: one of its setups serves any number of threads of one CPU
 * (include/pffft/pffft.h:102-105) - which is what one setup for all devices restores. */
int pffft_hip_transform_batch_multi(int nparts, const int *devices, PFFFT_Setup *const *setups, const float *const *in, float *const *out,
                                    const size_t *batches, pffft_direction_t direction, int ordered, void *const *streams);
int pffftd_hip_transform_batch_multi(int nparts, const int *devices, PFFFTD_Setup *const *setups, const double *const *in, double *const *out,
                                     const size_t *batches, pffft_direction_t direction, int ordered, void *const *streams);

/* Spectral convolution in one call (round 4):   out[i] (+)= backward( forward(in[i]) . H[i or 0] ) * scaling
 * - the sequence pffft_transform(FORWARD), pffft_zconvolve_no_accu, pffft_transform(BACKWARD) of every FFT convolution
 * (src/pffft_priv_impl.h:1465-1532, :1632-1684; src/pffastconv.c:235-254 is one instance), with `in` / `out` in the TIME domain
 * and H a spectrum in the INTERNAL layout (what pffft_transform(…, PFFFT_FORWARD) produced for the filter).  The transforms are
 * unscaled like the reference's: pass scaling = 1/N for a true circular convolution.  accumulate != 0 adds the result to `out`
 * (by linearity the same values as accumulating spectra with pffft_zconvolve_accumulate before one inverse transform).
 * h_broadcast != 0: ONE filter spectrum for the whole batch - for the power-of-two sizes up to N = 8192 complex / 16384 real
 * (float; 4096 / 8192 double) this runs as ONE kernel, one read and one write of every vector instead of seven vector passes;
 * every other case (per-vector spectra, sizes with factors 3 / 5, sizes beyond LDS) is composed from the three batched entries
 * on `stream` through a per-stream scratch image of the batch.  in == out is allowed; H must not alias out. */
int pffft_hip_convolve_batch(PFFFT_Setup *, const float *in, const float *H, float *out, float scaling, size_t batch,
                             int accumulate, int h_broadcast, void *stream);
int pffftd_hip_convolve_batch(PFFFTD_Setup *, const double *in, const double *H, double *out, double scaling, size_t batch,
                              int accumulate, int h_broadcast, void *stream);

/* Frequency shift fused into the forward transform (the mixers themselves:
 * include/pfdsp_hip.h, reference src/pf_mixer.cpp:142-165).  `in` is ONE stream of batch*N interleaved
 * complex samples; sample g is multiplied by exp(j*(phase_rad + 2*pi*rate*g)) — shift_math_cc's
 * function with an exactly reduced phase — and every N consecutive shifted samples are forward-
 * transformed as pffft_hip_transform_batch would (ordered as there).  Complex float setups only.
 * N = 1024 runs as one kernel (the shift costs no HBM traffic); other N as mixer + in-place transform. */
int pffft_hip_shift_transform_batch(PFFFT_Setup *, const float *in, float *out, size_t batch, int ordered,
                                    double rate, double phase_rad, void *stream);

/* Windowed overlapping-frame transforms: short-time analysis and overlap-add synthesis in one call each.
 * A SAMPLE is one scalar for a real setup and one interleaved complex pair for a complex one (spp = 1 / 2 scalars); `hop` and the
 * frame positions are in samples, every stride is in scalars of the setup's type.  All pointers are device pointers, the calls are
 * asynchronous on `stream`; 0, else a hipError_t with its text in pffft_hip_last_error().
 *
 * pffft_hip_frames_transform_batch.  Frame f of signal i is x[j] = signal[i*signal_stride + (f*hop + j)*spp ..] * window[j], j < N
 * (window: N real scalars; NULL = no multiplication at all); the product is ONE rounding in the setup's type.  Frame
 * v = i*nframes + f is forward-transformed exactly as pffft_hip_transform_batch transforms vector v - the result equals
 * transform_batch of the materialised frames bit for bit - and written at out + v*out_stride:
 *   PFFFT_HIP_FRAMES_INTERNAL / _ORDERED  the layouts of ordered = 0 / 1 (N scalars per frame for a real, 2N for a complex setup);
 *   PFFFT_HIP_FRAMES_POWER                re^2 + im^2 per bin: N/2 + 1 scalars per frame for a real setup (bins 0 ... N/2, DC and
 *                                         Nyquist unpacked), N for a complex one.
 * out_stride = 0: dense rows.  No centring and no padding: every signal holds (nframes-1)*hop + N samples (checked against
 * signal_stride when nsignals > 1; signal_stride is not read when nsignals == 1).  Any hop >= 1, also hop > N.  signal and out must
 * not overlap.  Real float setups of N = 1024 / 2048 / 4096 run as ONE kernel - the register-tiled transform with a framed,
 * windowing loader: (hop + N) scalars of HBM traffic per frame, |X|^2 taken from the registers - when hop, signal_stride and (for the
 * spectrum outputs) out_stride are multiples of 4 and signal, window and out are 16-byte aligned.  Every other legal size, hop,
 * alignment and precision is composed: a framing kernel into a per-stream frame matrix, pffft_hip_transform_batch, and a row kernel
 * where `out` is pitched or a power spectrum.  The frame matrix holds at most 256 MiB; longer batches go through it in chunks on
 * `stream`.  It follows the rules of the other per-stream scratch: it grows outside HIP graph capture only - a call that would have to
 * grow it while `stream` is capturing fails with hipErrorStreamCaptureUnsupported and launches nothing: run the call once on that
 * stream before capturing.
 *
 * pffft_hip_frames_overlap_add_batch.  Spectrum v = i*nframes + f (layout by `ordered`, at spectra + v*spectra_stride, 0 = dense) is
 * backward-transformed as pffft_hip_transform_batch(..., PFFFT_BACKWARD, ordered) does (UNSCALED) into y_f, and sample s of signal i,
 * for every s < (nframes-1)*hop + N, is WRITTEN (not accumulated) as
 *     signal[s] = scaling * ( sum_f window[s - f*hop] * y_f[s - f*hop] )    over the frames with 0 <= s - f*hop < N, f ascending,
 * each product and each addition rounded once, the sum started from its first term (window == NULL: the terms are y_f itself): a
 * gather in a fixed order, no atomics, so the result is deterministic.  Samples no frame covers (hop > N) are written as 0.
 * NORMALISING BY THE WINDOW'S OVERLAP SUM IS THE CALLER'S BUSINESS (`scaling`): the transforms are unscaled, so for a periodic Hann
 * window on both sides at hop = N/4 it is 1/(1.5*N).  Composed: backward transforms into the frame matrix, then the gather (beyond
 * the 256 MiB cap signal by signal in runs of frames).  spectra and signal must not overlap.
 *
 * Validation happens before any device is touched: a NULL or foreign setup, hop == 0, an unknown `output`, a stride smaller than the
 * row it has to hold, a signal_stride smaller than one signal's samples when nsignals > 1, a NULL signal / spectra / out -> non-zero,
 * nothing launched.  nsignals == 0 or nframes == 0 -> 0, nothing launched. */
enum { PFFFT_HIP_FRAMES_INTERNAL = 0, PFFFT_HIP_FRAMES_ORDERED = 1, PFFFT_HIP_FRAMES_POWER = 2 };
int pffft_hip_frames_transform_batch(PFFFT_Setup *, const float *signal, size_t signal_stride, size_t nsignals, size_t nframes,
                                     size_t hop, const float *window, float *out, size_t out_stride, int output, void *stream);
int pffftd_hip_frames_transform_batch(PFFFTD_Setup *, const double *signal, size_t signal_stride, size_t nsignals, size_t nframes,
                                      size_t hop, const double *window, double *out, size_t out_stride, int output, void *stream);
int pffft_hip_frames_overlap_add_batch(PFFFT_Setup *, const float *spectra, size_t spectra_stride, size_t nsignals, size_t nframes,
                                       size_t hop, const float *window, float scaling, float *signal, size_t signal_stride,
                                       int ordered, void *stream);
int pffftd_hip_frames_overlap_add_batch(PFFFTD_Setup *, const double *spectra, size_t spectra_stride, size_t nsignals, size_t nframes,
                                        size_t hop, const double *window, double scaling, double *signal, size_t signal_stride,
                                        int ordered, void *stream);
/* The route pffft_hip_frames_transform_batch takes for these arguments under the calling thread's selector (pffft_hip_set_variant:
 * 124 = always composed, 125 = fused wherever it is legal): "fused" or "composed"; "" for an invalid handle, hop == 0 or an unknown
 * output.  Pointer alignment is checked at the call: the query assumes 16-byte aligned pointers.  signal_stride = 0: one signal.
 * Host arithmetic only; PFFFT_Setup and PFFFTD_Setup handles. */
const char *pffft_hip_frames_route(const void *setup, size_t hop, size_t signal_stride, size_t out_stride, int output);

/* Averaged power spectra over overlapping frames (Welch's method; one row of a time-averaged spectrogram per navg frames) without the
 * nframes x P intermediate.  Framing, `window` (NULL = no product), `hop`, `signal_stride`, the sample / scalar rules and the pointer rules
 * are exactly those of pffft_hip_frames_transform_batch; real and complex setups, float and double, every legal size.
 * GROUPING.  navg == 0 means navg = nframes (one row per signal: Welch); otherwise nframes % navg must be 0.  With G = nframes / navg,
 * group g of signal i is frames g*navg ... g*navg + navg - 1, and output row v = i*G + g is written at out + v*out_stride (0 = dense).  A
 * row holds P scalars: N/2 + 1 for a real setup (bins 0 ... N/2, DC and Nyquist unpacked), N for a complex one.
 * ARITHMETIC - THE ORDER IS PART OF THE CONTRACT.  p_f[k] is the value pffft_hip_frames_transform_batch(..., PFFFT_HIP_FRAMES_POWER)
 * produces for frame f, bit for bit.  A group is cut into runs of PFFFT_HIP_PSD_RUN consecutive frames (the last run may be shorter); a
 * run's partial is the sum of its p_f[k], f ascending, started from the first term, every addition rounded once; the group's value is the
 * sum of its run partials, run ascending, started from the first; the result is multiplied ONCE by `scaling` (1/(navg * sum w^2 * fs) or
 * whatever the caller's normalisation is: the library normalises nothing).  No atomics and no FMA: the result is deterministic and equal
 * on every route.
 * Real float setups of N = 1024 / 2048 / 4096 run FUSED when hop and signal_stride are multiples of 4 and signal and window are 16-byte
 * aligned (out needs scalar alignment only): the framed kernel keeps a workgroup slot on the consecutive frames of one run, accumulates
 * |X|^2 in registers and stores once per run - hop + P / min(navg, 32) scalars of HBM traffic per frame; averages longer than one run
 * leave their run partials in a per-stream partial buffer that a small second kernel adds up.  Everything else is COMPOSED: the framing
 * kernel into the per-stream frame matrix (256 MiB cap, chunks of whole runs; as large as one run needs where a run exceeds the cap),
 * pffft_hip_transform_batch(ordered = 1), a kernel that adds the |X|^2 of each run's rows in order, and the same reduction.  The partial
 * buffer holds at most 256 MiB (one group's partials where a group needs more) and is gone through in whole groups.  Both buffers grow
 * outside HIP graph capture only: a call that would have to grow one while `stream` is capturing fails with
 * hipErrorStreamCaptureUnsupported and launches nothing.  signal and out must not overlap.
 * Validation happens before any device is touched: a NULL or foreign setup or the other precision's handle, hop == 0, nframes % navg != 0,
 * an out_stride smaller than P, a signal_stride smaller than one signal's scalars when nsignals > 1, a NULL signal / out -> non-zero,
 * nothing launched.  nsignals == 0 or nframes == 0 -> 0, nothing launched. */
#define PFFFT_HIP_PSD_RUN 32
int pffft_hip_frames_psd_batch(PFFFT_Setup *, const float *signal, size_t signal_stride, size_t nsignals, size_t nframes, size_t hop,
                               const float *window, size_t navg, float scaling, float *out, size_t out_stride, void *stream);
int pffftd_hip_frames_psd_batch(PFFFTD_Setup *, const double *signal, size_t signal_stride, size_t nsignals, size_t nframes, size_t hop,
                                const double *window, size_t navg, double scaling, double *out, size_t out_stride, void *stream);
/* The route pffft_hip_frames_psd_batch takes for these arguments under the calling thread's selector (pffft_hip_set_variant: 134 = always
 * composed, 135 = fused wherever it is legal): "fused" or "composed"; "" for an invalid handle or hop == 0.  Pointer alignment is checked
 * at the call: the query assumes 16-byte aligned pointers.  signal_stride = 0: one signal; navg = 0: every frame of a signal.
 * Host arithmetic only; PFFFT_Setup and PFFFTD_Setup handles. */
const char *pffft_hip_frames_psd_route(const void *setup, size_t hop, size_t signal_stride, size_t navg);

/* Averaged cross-spectra and coherence of TWO signals over overlapping frames (Welch's method; scipy's csd / coherence without detrending,
 * one-sided doubling or normalisation) without the two nframes x N spectrograms.  x and y are framed alike: framing, `window` (NULL = no
 * product), `hop`, the sample / scalar rules, the grouping by `navg` (0 = nframes, else nframes % navg == 0; output row v = i*G + g with
 * G = nframes / navg), P (N/2 + 1 for a real setup, N for a complex one), real and complex setups, float and double, every legal size and
 * the rules of the two per-stream buffers during HIP graph capture are exactly those of pffft_hip_frames_psd_batch.  x_stride and y_stride
 * may differ (neither is read when nsignals == 1); y == x is legal; out must not overlap x or y.
 * `what` selects the row written at out + v*out_stride (0 = dense):
 *     PFFFT_HIP_CSD_CROSS      P complex bins, (re, im) interleaved: 2P scalars - the cross-spectrum Pxy
 *     PFFFT_HIP_CSD_ALL        Pxx[P] | Pyy[P] | Pxy[2P]: 4P scalars
 *     PFFFT_HIP_CSD_COHERENCE  P scalars |Sxy|^2 / (Sxx*Syy); `scaling` is not read
 * ARITHMETIC - THE ORDER IS PART OF THE CONTRACT.  X_f and Y_f are the ordered spectra that pffft_hip_frames_transform_batch(...,
 * PFFFT_HIP_FRAMES_ORDERED) produces for frame f of x and of y, bit for bit.  Per frame and bin, every product and every sum rounded once,
 * no FMA:
 *     c_re = Xr*Yr + Xi*Yi,   c_im = Xr*Yi - Xi*Yr          (conj(X) * Y, scipy's convention)
 * and pxx, pyy are exactly the PFFFT_HIP_FRAMES_POWER expressions of x and of y.  The two real-only bins of a real setup (the packed bin 0)
 * give (X_0*Y_0, +0) and (X_{N/2}*Y_{N/2}, +0).  Each of the four sums is accumulated exactly as pffft_hip_frames_psd_batch accumulates:
 * runs of PFFFT_HIP_PSD_RUN consecutive frames, f ascending, started from the first term; then the run partials ascending, started from
 * the first.  CROSS and ALL multiply each sum ONCE by `scaling`.  COHERENCE forms (Sre*Sre + Sim*Sim) / (Sxx*Syy) from the UNSCALED group
 * sums: two squares, one sum, one product, one IEEE division, each rounded once; 0/0 = NaN.  No atomics: the result is deterministic and
 * equal on every route.  Hence: Pxx and Pyy of ALL are the bits of pffft_hip_frames_psd_batch for x and for y; csd(x, x) has those bits in
 * its real parts and a zero in every imaginary part; csd(y, x) is csd(x, y) with every non-zero imaginary part negated; coherence(x, x) is
 * exactly 1 wherever Sxx*Sxx neither overflows nor underflows.
 * ROUTES.  Everything runs COMPOSED: the framing kernel for the x frames and for the y frames of whole runs into the two halves of the
 * per-stream frame matrix (the 256 MiB cap holds for both together), ONE pffft_hip_transform_batch(ordered = 1) over both halves, a kernel
 * that walks each run's rows of both sets in order, and for averages longer than one run the partial buffer of the PSD entry (rows of 2P
 * scalars for CROSS, 4P for ALL and COHERENCE) with its reduction, which forms the coherence ratio.  The cross-spectrum of real float
 * setups of N = 1024 / 2048 / 4096 runs FUSED when hop, x_stride and y_stride are multiples of 4 and x, y and window are 16-byte aligned
 * (out needs scalar alignment only): one kernel runs the framed transform twice per frame, keeps X_f in registers while Y_f is computed,
 * accumulates the products in registers and stores once per run - 2*hop + 2P / min(navg, 32) scalars of HBM traffic per frame.  ALL and
 * COHERENCE have no fused kernel (their four sums do not fit the register file next to two spectra).
 * Validation happens before any device is touched: what the PSD entry refuses, an unknown `what`, a NULL y, a y_stride smaller than one
 * signal's scalars when nsignals > 1, an out_stride smaller than the row of `what` -> non-zero, nothing launched.  nsignals == 0 or
 * nframes == 0 -> 0, nothing launched. */
#define PFFFT_HIP_CSD_CROSS 0
#define PFFFT_HIP_CSD_ALL 1
#define PFFFT_HIP_CSD_COHERENCE 2
int pffft_hip_frames_csd_batch(PFFFT_Setup *, const float *x, size_t x_stride, const float *y, size_t y_stride, size_t nsignals,
                               size_t nframes, size_t hop, const float *window, size_t navg, float scaling, int what, float *out,
                               size_t out_stride, void *stream);
int pffftd_hip_frames_csd_batch(PFFFTD_Setup *, const double *x, size_t x_stride, const double *y, size_t y_stride, size_t nsignals,
                                size_t nframes, size_t hop, const double *window, size_t navg, double scaling, int what, double *out,
                                size_t out_stride, void *stream);
/* The route pffft_hip_frames_csd_batch takes for these arguments under the calling thread's selector (pffft_hip_set_variant: 142 = always
 * composed, 143 = fused wherever it is legal): "fused" or "composed"; "" for an invalid handle, hop == 0 or an unknown `what`.  Pointer
 * alignment is checked at the call: the query assumes 16-byte aligned pointers.  x_stride = y_stride = 0: one signal; navg = 0: every frame
 * of a signal.  Host arithmetic only; PFFFT_Setup and PFFFTD_Setup handles. */
const char *pffft_hip_frames_csd_route(const void *setup, size_t hop, size_t x_stride, size_t y_stride, size_t navg, int what);

/* Polyphase filter-bank analysis (weighted overlap-add channelizer): the framing of pffft_hip_frames_transform_batch with a prototype
 * filter of taps*N real coefficients that is folded onto N points before the transform.  For frame f of signal i
 *     u_f[j] = sum over p = 0 ... taps-1 of  prototype[p*N + j] * x_i[f*hop + p*N + j],   j < N
 * (x: real samples, or complex samples times the real coefficient), and out_f is the forward transform of u_f exactly as
 * pffft_hip_transform_batch transforms a vector.  ROUNDING IS PART OF THE CONTRACT: every product is rounded once, every addition is
 * rounded once, p ascending, the sum started from its first term (no FMA) - so the result equals transform_batch of the materialised
 * folded frames bit for bit on every route, and taps = 1 is pffft_hip_frames_transform_batch with the prototype as its window, bit for bit.
 * Every signal holds (nframes-1)*hop + taps*N samples.  There is NO circular shift and NO per-frame phase rotation: out_f[k] is the
 * length-taps*N windowed DFT of the segment that starts at sample f*hop, sampled at every taps-th bin (bin taps*k), phase-referenced
 * to the frame's FIRST sample - as the output of the frame entry is.  A caller who wants channel phases that are continuous from frame
 * to frame at a hop that is no multiple of N rotates bin k of frame f by exp(-2 pi i k f hop / N) (or circularly shifts u_f) itself.
 * Arguments, strides, `output` (PFFFT_HIP_FRAMES_INTERNAL / _ORDERED / _POWER), row sizes, out_stride = 0, the frame numbering
 * v = i*nframes + f, the 256 MiB cap of the frame matrix with chunking and its rule during HIP graph capture are those of
 * pffft_hip_frames_transform_batch.  signal, prototype and out must not overlap.
 * Complex float setups of N = 1024 run as ONE kernel for the spectrum outputs - the N = 1024 transform with a folding loader and the
 * prototype in LDS: taps*N/hop reads of a sample served by the caches, one write of the spectrum - when hop is even, signal_stride and
 * out_stride are multiples of 4 scalars, signal and out are 16-byte and prototype 8-byte aligned and
 * taps <= PFFFT_HIP_PFB_FUSED_MAX_TAPS, in the (taps, hop) cells where that kernel measured faster.  Everything else
 * - every other size, precision and transform, |X|^2, odd hops - is composed: a folding kernel into the per-stream frame matrix,
 * pffft_hip_transform_batch, and a row kernel where `out` is pitched or a power spectrum.
 * Validation happens before any device is touched: a NULL or foreign setup, hop == 0, taps == 0, prototype == NULL, an unknown `output`,
 * an out_stride smaller than a row, a signal_stride smaller than ((nframes-1)*hop + taps*N) samples when nsignals > 1, a NULL signal /
 * out -> non-zero, nothing launched.  nsignals == 0 or nframes == 0 -> 0, nothing launched. */
#define PFFFT_HIP_PFB_FUSED_MAX_TAPS 16
int pffft_hip_pfb_transform_batch(PFFFT_Setup *, const float *signal, size_t signal_stride, size_t nsignals, size_t nframes,
                                  size_t hop, const float *prototype, size_t taps, float *out, size_t out_stride, int output,
                                  void *stream);
int pffftd_hip_pfb_transform_batch(PFFFTD_Setup *, const double *signal, size_t signal_stride, size_t nsignals, size_t nframes,
                                   size_t hop, const double *prototype, size_t taps, double *out, size_t out_stride, int output,
                                   void *stream);
/* The route pffft_hip_pfb_transform_batch takes for these arguments under the calling thread's selector (pffft_hip_set_variant:
 * 126 = always composed, 127 = fused wherever it is legal): "fused" or "composed"; "" for an invalid handle, hop == 0, taps == 0 or an
 * unknown output.  Pointer alignment is checked at the call: the query assumes aligned pointers.  signal_stride = 0: one signal.
 * Host arithmetic only; PFFFT_Setup and PFFFTD_Setup handles. */
const char *pffft_hip_pfb_route(const void *setup, size_t hop, size_t taps, size_t signal_stride, size_t out_stride, int output);

/* Polyphase filter-bank synthesis (weighted overlap-add of PERIODICALLY EXTENDED backward transforms): the way back from the spectra of
 * pffft_hip_pfb_transform_batch, and pffft_hip_frames_overlap_add_batch with a prototype of taps*N real coefficients instead of a window
 * of N.  Spectrum v = i*nframes + f (layout by `ordered`, at spectra + v*spectra_stride, 0 = dense) is backward-transformed exactly as
 * pffft_hip_transform_batch(..., PFFFT_BACKWARD, ordered) does (UNSCALED) into y_f[0..N), and sample s of signal i, for every
 * s < (nframes-1)*hop + taps*N, is WRITTEN (not accumulated) as
 *     signal[s] = scaling * ( sum_f prototype[s - f*hop] * y_f[(s - f*hop) mod N] )
 *                 over the frames with 0 <= s - f*hop < taps*N, f ascending
 * (complex setups: a sample is an interleaved pair, both scalars take the same real coefficient).  ROUNDING IS PART OF THE CONTRACT:
 * every product is rounded once, every addition is rounded once, f ascending, the sum started from its first term (no FMA), and the result
 * is multiplied once by `scaling`.  Samples no frame covers (hop > taps*N) are written as 0.  A gather in a fixed order, no atomics: the
 * result is deterministic.  Every signal holds (nframes-1)*hop + taps*N samples (checked against signal_stride when nsignals > 1;
 * signal_stride is not read when nsignals == 1).  It follows that
 *   (1) taps = 1 with the same coefficients as window is pffft_hip_frames_overlap_add_batch, bit for bit;
 *   (2) the result equals the sum above evaluated in the setup's type on pffft_hip_transform_batch(BACKWARD)'s own rows, bit for bit, for
 *       every hop, alignment and kernel form;
 *   (3) in exact arithmetic the synthesis of pffft_hip_pfb_transform_batch's output (analysis prototype h) is
 *           out[s] = scaling * N * sum_r x[s + r*N] * sum_f prototype[m] * h[m + r*N],   m = s - f*hop,
 *       so perfect reconstruction needs sum_f prototype[m]*h[m] = 1/(scaling*N) and sum_f prototype[m]*h[m + r*N] = 0 for r != 0 (a two-tap
 *       paraunitary prototype at hop = N/2 with scaling = 1/N satisfies both on the interior
 *       taps*N - hop <= s < (nframes-1)*hop + hop).
 * There is NO circular shift and NO per-frame phase rotation: y_f is taken phase-referenced to the frame's FIRST sample - as the output
 * of the analysis entry is.  A caller who rotated bin k of frame f by exp(-2 pi i k f hop / N) (or circularly shifted u_f) for channel
 * phases that are continuous from frame to frame undoes that itself before this call.
 * Arguments and strides are those of pffft_hip_frames_overlap_add_batch; all pointers are device pointers, the call is asynchronous on
 * `stream`; 0, else a hipError_t with its text in pffft_hip_last_error().  spectra, prototype and signal must not overlap.
 * Composed, for every setup (real and complex, float and double, every size): backward transforms into the per-stream frame matrix
 * (pitched spectra through a row kernel first), then an output-stationary gather kernel - 16 bytes of the output per thread where hop*spp,
 * signal_stride and the row are multiples of 16 bytes and signal and prototype are aligned (16 bytes; the prototype of a complex setup: 8),
 * one scalar per thread otherwise, the same arithmetic in both.  The frame matrix, its 256 MiB cap, the mutex and the rule during HIP
 * graph capture (growth -> hipErrorStreamCaptureUnsupported, nothing launched) are those of the frame entries.  Beyond the cap the call
 * goes signal by signal in runs of frames; a run re-transforms the ceil(taps*N/hop) - 1 earlier frames that reach into its samples and is
 * never shorter than that, so where that many frames + 1 do not fit under the cap THE MATRIX IS AS LARGE AS THEY NEED (at most twice that
 * many rows).
 * Validation happens before any device is touched: a NULL or foreign setup or the other precision's handle, hop == 0, taps == 0,
 * prototype == NULL, a spectra_stride smaller than a row, a signal_stride smaller than one signal's scalars when nsignals > 1, a NULL
 * spectra / signal -> non-zero, nothing launched.  nsignals == 0 or nframes == 0 -> 0, nothing launched. */
int pffft_hip_pfb_synthesis_batch(PFFFT_Setup *, const float *spectra, size_t spectra_stride, size_t nsignals, size_t nframes,
                                  size_t hop, const float *prototype, size_t taps, float scaling,
                                  float *signal, size_t signal_stride, int ordered, void *stream);
int pffftd_hip_pfb_synthesis_batch(PFFFTD_Setup *, const double *spectra, size_t spectra_stride, size_t nsignals, size_t nframes,
                                   size_t hop, const double *prototype, size_t taps, double scaling,
                                   double *signal, size_t signal_stride, int ordered, void *stream);

/* Complex transforms of ANY length 1 <= N <= 2^25 (Bluestein's algorithm on the library's own convolution).  pffft_new_setup keeps
 * the reference's rule (N = 2^a 3^b 5^c, a multiple of 16 / 32, else NULL); padding to pffft_nearest_transform_size changes the bin
 * spacing, so it is no answer to "the DFT of these 1000, 1021 or 10007 samples".  This setup type is:
 *     out[v][k] = sum_n in[v][n] * exp(-/+ 2 pi j n k / N),   k < N     (forward / backward; UNSCALED: backward(forward(x)) = N x)
 * Rows are N interleaved complex values, dense; there is no internal layout for this setup type.  PFFFT_COMPLEX only - PFFFT_REAL is
 * reserved and returns NULL today, like N < 1 and N > 2^25.  Creating a setup touches no device.  in / out are device pointers, 16-byte
 * (float) / 32-byte (double) aligned like the other batched entries' (rows of odd N are then aligned to one complex value only, which
 * every kernel here copes with; a base pointer aligned to one complex value is accepted on the fused and composed routes).  in == out is
 * allowed; otherwise they must not overlap.  The call is asynchronous on `stream`; 0, else a hipError_t with its text in
 * pffft_hip_last_error().  Validation happens before any device is touched: a NULL or foreign handle or the other precision's, a bad
 * direction, NULL or misaligned in / out -> non-zero, nothing launched.
 * Routes, planned once at setup (pffft_hip_any_route names the one a call takes under the calling thread's selector):
 *   "direct"    N is itself a legal complex size: pffft[d]_hip_transform_batch(..., ordered = 1) on an inner setup, bit for bit.
 *   "fused"     float and M = the next power of two >= 2N - 1 is 512, 1024, 2048 or 4096 (N = 129 ... 2047): ONE kernel - the fused
 *               convolution kernel of pffft_hip_convolve_batch with a chirping, zero-padding loader and a chirping, cropping store: N
 *               samples read and N written per vector.  The default wherever it is legal.
 *   "composed"  everything else (double, N outside the fused set; selector 132 everywhere): a chirp-and-pad kernel into a per-stream scratch
 *               image of batch x M, pffft[d]_hip_convolve_batch on an inner setup of length M with one broadcast filter spectrum, a
 *               chirp-and-crop kernel.  M is pffft_nearest_transform_size(2N - 1, PFFFT_COMPLEX, higher); a setup that can run fused uses its power of two on both routes.
 * The scratch image follows the rules of the other per-stream scratch: at most 256 MiB (one row where a row is longer), longer batches go
 * through it in chunks on `stream`; it grows outside HIP graph capture only - a call that would have to grow it while `stream` is
 * capturing fails with hipErrorStreamCaptureUnsupported and launches nothing.
 * THE FIRST CALL ON A SETUP BUILDS ITS TABLES (the chirp w[n] = exp(-j pi (n^2 mod 2N) / N) - the reduction in 64-bit integers, the angle
 * in long double, rounded once - and the filter's spectrum, computed with the double transform also for float setups): it allocates and
 * synchronises the device, so like the first call on a CIC state it must happen BEFORE a stream capture (during one it fails with
 * hipErrorStreamCaptureUnsupported).  batch == 0 builds the tables, launches nothing else and returns 0.  The backward direction uses the
 * same tables (both ends conjugate).  A setup serves ONE device, like PFFASTCONV_Setup: the device that is current at the first call; a
 * call from a thread whose current device is another one fails with hipErrorInvalidDevice.  Any number of streams and threads of that
 * device may share it. */
typedef struct PFFFT_HIP_AnySetup PFFFT_HIP_AnySetup;
typedef struct PFFFTD_HIP_AnySetup PFFFTD_HIP_AnySetup;
PFFFT_HIP_AnySetup *pffft_hip_any_new_setup(int N, pffft_transform_t transform);
PFFFTD_HIP_AnySetup *pffftd_hip_any_new_setup(int N, pffft_transform_t transform);
void pffft_hip_any_destroy_setup(PFFFT_HIP_AnySetup *);     /* NULL-safe */
void pffftd_hip_any_destroy_setup(PFFFTD_HIP_AnySetup *);
int pffft_hip_any_transform_batch(PFFFT_HIP_AnySetup *, const float *in, float *out, size_t batch, pffft_direction_t direction,
                                  void *stream);
int pffftd_hip_any_transform_batch(PFFFTD_HIP_AnySetup *, const double *in, double *out, size_t batch, pffft_direction_t direction,
                                   void *stream);
/* Host arithmetic only, handles of both precisions.  pffft_hip_any_conv_size: the convolution length M; 0 on the direct route; -1 for an
 * invalid handle.  pffft_hip_any_route: "direct" / "fused" / "composed" under the calling thread's selector (pffft_hip_set_variant:
 * 132 = never fused, 133 = fused wherever it is legal); "" for an invalid handle.  pffft_hip_any_chirp: the N chirp values w[n] as
 * interleaved (re, im) pairs of the setup's type into host_out, as the device table holds them; 0, non-zero for an invalid handle or a
 * NULL host_out. */
int pffft_hip_any_conv_size(const void *setup);
const char *pffft_hip_any_route(const void *setup);
int pffft_hip_any_chirp(const void *setup, void *host_out);

/* REAL transforms of any length 1 <= N <= 2^25 with half-spectrum I/O (numpy's rfft / irfft . N).  PFFFT_REAL stays reserved in
 * pffft[d]_hip_any_new_setup; a real setup comes from its own constructor (NULL for N < 1 and N > 2^25; touches no device) and is an
 * any-length setup with a real flag: pffft[d]_hip_any_transform_batch, _any_destroy_setup, pffft_hip_any_route, _any_conv_size and
 * _any_chirp (the same N chirp values as for a complex setup of N) accept it.  With H = floor(N / 2) + 1:
 *   FORWARD   in: batch dense rows of N real scalars; out: batch dense rows of H interleaved complex bins (2H scalars),
 *             out[v][k] = sum_n in[v][n] exp(-2 pi j n k / N), k < H.  The imaginary part of bin 0, and of bin N/2 for even N, is what the
 *             arithmetic yields (a rounding-sized value) on the fused and composed routes and exactly +0 on the direct route.
 *   BACKWARD  in: rows of H complex bins; out: rows of N reals, UNSCALED (backward(forward(x)) = N x).  The imaginary parts of bin 0 and of
 *             bin N/2 (even N) are NOT part of the input: whatever they hold, NaN included, the output has the same bits.
 * in and out must not overlap (their rows differ in size).  Routes, planned once at setup:
 *   "direct"    N is a legal REAL size (pffft_is_valid_size(N, PFFFT_REAL)): transform_batch(ordered = 1) on an inner real setup through a
 *               per-stream scratch of canonical spectra, and a kernel that moves the values between that layout and the H bins, bit for
 *               bit.  in / out 16-byte (float) / 32-byte (double) aligned.  pffft_hip_any_conv_size = 0.
 *   "fused"     float and M = the next power of two >= N + floor(N / 2) is 512, 1024, 2048 or 4096 (N = 172 ... 2731): ONE kernel, the
 *               fused convolution kernel with a real loader / store policy: 4 N + 8 H bytes per row.  Only the bins k < H are wanted, so
 *               a circular length M >= N + floor(N / 2) suffices where the complex transform needs 2N - 1.
 *   "composed"  everything else (double, other N; selector 132 everywhere): pad kernel, pffft[d]_hip_convolve_batch at length
 *               M = pffft_nearest_transform_size(N + floor(N / 2), PFFFT_COMPLEX, higher), crop kernel (a setup that can run fused uses its
 *               power of two on both routes).
 * On the fused and composed routes the real-side pointer may be aligned to one scalar and the complex-side pointer to one complex value.
 * Each direction has its own filter spectrum (the two supports are mirror images); both are built with the chirp at the first call.
 * Validation before any device is touched, the first-call table build and its stream-capture rule, one setup per device, the 256 MiB
 * scratch cap with chunking: as for the complex setup above. */
PFFFT_HIP_AnySetup *pffft_hip_any_new_real_setup(int N);
PFFFTD_HIP_AnySetup *pffftd_hip_any_new_real_setup(int N);
/* Host arithmetic only, handles of both precisions.  pffft_hip_any_is_real: 1 for a real setup, 0 for a complex one.
 * pffft_hip_any_bins: complex values per spectrum row: floor(N / 2) + 1 for a real setup, N for a complex one.  Both -1 for an invalid
 * handle. */
int pffft_hip_any_is_real(const void *setup);
int pffft_hip_any_bins(const void *setup);

/* ZOOM transforms (the chirp-z transform on the unit circle, scipy's zoom_fft): K spectral lines from f0 in steps of df, both in cycles
 * per sample (finite doubles of any sign and magnitude), of rows of N samples - where the any-length setups answer "the DFT of these N
 * samples", this one answers "K lines between two frequencies at a resolution of my choosing" without padding to a long size or mixing,
 * decimating and transforming in three calls:
 *     out[v][k] = sum_{n<N} in[v][n] * exp(-/+ 2 pi j n (f0 + k df)),   k < K     (forward / backward; UNSCALED)
 * `in` holds batch dense rows of N interleaved complex values, `out` batch dense rows of K.  BACKWARD is the conjugate kernel,
 * conj(zoom(conj x)) - it is NOT an inverse.  f0 = 0, df = 1 / N, K = N is the DFT.  Real-input rows and spirals off the unit circle
 * (|w| != 1, |a| != 1 of the general chirp-z transform) are not offered.  NULL for N < 1, K < 1, N + K - 1 > 2^26 (the library's
 * largest setup) or a non-finite f0 / df.  Creating a setup touches no device.
 * Bluestein's algorithm on the library's own convolution, with n k df = (n^2 + k^2 - (k - n)^2) df / 2:
 *     a[n] = exp(-2 pi j frac(n f0 + n^2 df / 2)), n < N      c[k] = exp(-2 pi j frac(k^2 df / 2)), k < K
 *     b[m] = exp(+2 pi j frac(m^2 df / 2)), -(N-1) <= m <= K-1     out[k] = c[k] sum_n (in[n] a[n]) b[k - n]     (circular length M >= N + K - 1)
 * THE PHASE REDUCTION IS PART OF THE CONTRACT: frac is taken from the exact rational value of the doubles (a double is an integer times a
 * power of two; n^2 times a 53-bit mantissa fits 128 bits), the reduced phase in (-1/2, 1/2] is rounded once to long double and multiplied
 * by 2 pi there, cos and sin are rounded once to the table's type.  a and c are in the setup's type, the filter b always in double; its
 * spectrum comes from the double transform and is rounded once.
 * in / out are device pointers aligned to one complex value (8 / 16 bytes).  in and out MUST NOT OVERLAP (their rows differ in size):
 * overlapping ranges are refused.  The call is asynchronous on `stream`; 0, else a hipError_t with its text in pffft_hip_last_error().
 * Validation happens before any device is touched: a NULL or foreign handle or the other precision's, a bad direction, NULL, misaligned
 * or overlapping in / out -> non-zero, nothing launched.
 * Routes, planned once at setup (pffft_hip_zoom_route names the one a call takes under the calling thread's selector):
 *   "fused"     float and M2 = the next power of two >= N + K - 1 is 512, 1024, 2048 or 4096 (257 <= N + K - 1 <= 4096): ONE kernel - the
 *               fused convolution kernel of pffft_hip_convolve_batch with a loader that takes N samples times a (zeros above N) and a
 *               store that writes the first K results times c: 8 N bytes read and 8 K written per row.  The default at all four lengths: on
 *               an MI355X it takes 0.37 ... 0.64 of the composed route's time.
 *   "composed"  double, every other N + K - 1, selector 136 everywhere: a pad kernel (times a) into a per-stream scratch image of
 *               batch x M, pffft[d]_hip_convolve_batch on an inner setup of length M with one broadcast filter spectrum, a crop kernel
 *               (times c, K values).  M = pffft_nearest_transform_size(N + K - 1, PFFFT_COMPLEX, higher); a setup that can run fused
 *               uses M2 on both routes.
 * The first-call table build and its stream-capture rule, one setup per device, the 256 MiB per-stream scratch with chunking and its
 * capture rule, batch == 0 (builds the tables, launches nothing else, returns 0): as for the any-length complex setup above. */
typedef struct PFFFT_HIP_ZoomSetup PFFFT_HIP_ZoomSetup;
typedef struct PFFFTD_HIP_ZoomSetup PFFFTD_HIP_ZoomSetup;
PFFFT_HIP_ZoomSetup *pffft_hip_zoom_new_setup(int N, int K, double f0, double df);
PFFFTD_HIP_ZoomSetup *pffftd_hip_zoom_new_setup(int N, int K, double f0, double df);
void pffft_hip_zoom_destroy_setup(PFFFT_HIP_ZoomSetup *);     /* NULL-safe */
void pffftd_hip_zoom_destroy_setup(PFFFTD_HIP_ZoomSetup *);
int pffft_hip_zoom_transform_batch(PFFFT_HIP_ZoomSetup *, const float *in, float *out, size_t batch, pffft_direction_t direction,
                                   void *stream);
int pffftd_hip_zoom_transform_batch(PFFFTD_HIP_ZoomSetup *, const double *in, double *out, size_t batch, pffft_direction_t direction,
                                    void *stream);
/* Host arithmetic only, handles of both precisions.  pffft_hip_zoom_conv_size: the convolution length M; -1 for an invalid handle.
 * pffft_hip_zoom_route: "fused" / "composed" under the calling thread's selector (pffft_hip_set_variant: 136 = never fused, 137 = fused
 * wherever it is legal); "" for an invalid handle.  pffft_hip_zoom_table: the host evaluation of the phase functions above, `count` values
 * from index `first` as interleaved (re, im) pairs rounded to the setup's type into host_out: which = 0 is a (indices below N: the values
 * of the device's input table), which = 1 is c for indices below max(N, K) (below K the values of the device's output table; the filter
 * is conj(c[|m|]) in double, so the indices from K to N - 1 exist in the filter only).  0; non-zero for an invalid handle, another
 * `which`, a range beyond these counts or a NULL host_out. */
int pffft_hip_zoom_conv_size(const void *setup);
const char *pffft_hip_zoom_route(const void *setup);
int pffft_hip_zoom_table(const void *setup, int which, size_t first, size_t count, void *host_out);

/* COSINE AND SINE transforms of types II and III (scipy.fft.dct / dst with type = 2 / 3; FFTPACK's cosqb / cosqf / sinqb / sinqf are
 * 2 x DCT-II, DCT-III, 2 x DST-II, DST-III): rows of N reals in, rows of N reals out, dense.  norm = NONE (scipy's norm=None):
 *     DCT-II   X[k] = 2 sum_n x[n] cos(pi k (2n+1) / 2N)
 *     DCT-III  y[n] = X[0] + 2 sum_{k>=1} X[k] cos(pi k (2n+1) / 2N)                          DCT-III(DCT-II(x)) = 2N x
 *     DST-II   X[k] = 2 sum_n x[n] sin(pi (k+1) (2n+1) / 2N)                                  = DCT-II((-1)^n x)[N-1-k]
 *     DST-III  y[n] = (-1)^n X[N-1] + 2 sum_{k<N-1} X[k] sin(pi (k+1) (2n+1) / 2N)            = (-1)^n DCT-III(reverse X)[n]
 * norm = ORTHO is scipy's norm="ortho": the transforms are orthogonal, II and III exact inverses.  Legal N: every N pffft_new_setup(N,
 * PFFFT_REAL) takes (a multiple of 32, 2^a 3^b 5^c, up to 2^26); NULL for any other N, a kind or a norm out of range.  Creating a setup
 * touches no device; the handle owns a real setup of N, whose per-device behaviour carries over (one handle may serve several devices).
 * Makhoul's algorithm, ONE real transform of the same N (n = N/2, w_k = exp(-j pi k / 2N)):
 *     II   v[m] = x[2m], v[N-1-m] = x[2m+1];  V = forward transform of v;  z_k = V[k] t_k;  X[k] = Re z_k, X[N-k] = -Im z_k (0 < k < n),
 *          X[0] = V[0] Re t_0, X[n] = V[n] Re t_n
 *     III  V[k] = (X[k] - j X[N-k]) t_k (0 < k < n), V[0] = X[0] Re t_0, V[n] = 2 X[n] Re t_n;  v = unscaled backward transform of V;
 *          y[2m] = v[m], y[2m+1] = v[N-1-m]
 * with ONE folded table t_k, k = 0 ... n: t_k = 2 s_k w_k (II) / s'_k conj(w_k) (III); NONE: s = s' = 1; ORTHO: s_0 = 1/sqrt(4N),
 * s'_0 = 1/sqrt(N), s_k = s'_k = 1/sqrt(2N).  Each t_k is evaluated in long double and rounded once; every route forms the product with
 * the same operations (one product and one fused multiply-add per component), so the routes agree bit for bit.
 * in / out are device pointers aligned to 16 bytes.  out == in IS LEGAL on every route (any other overlap is refused).  The call is
 * asynchronous on `stream`; 0, else a hipError_t with its text in pffft_hip_last_error().  batch == 0 returns 0.
 * Routes (pffft_hip_dct_route names the one a call takes under the calling thread's selector):
 *   "fused"     float, N = 1024 / 2048 / 4096: ONE kernel - the register-tiled real transform between an input and an output round trip
 *               through its own LDS image: 4N bytes read and 4N written per row.  Which (size, kind) cells run it by default is a measured
 *               table - all twelve: on an MI355X it takes 0.30 ... 0.38 of the composed route's time;
 *               pffft_hip_set_variant(139) runs it wherever it is legal, 138 never.
 *   "composed"  every setup: a permutation / table kernel into a per-stream scratch image of batch x N, pffft[d]_hip_transform_batch in
 *               the canonical layout in place there, a table / permutation kernel into out.  The scratch holds at most 256 MiB (longer
 *               batches go through it in chunks on the stream); a call that would have to grow it - or build the table of a first call -
 *               on a capturing stream returns hipErrorStreamCaptureUnsupported before any launch: run the call once before capturing.
 * Type I, strided rows and lengths pffft_new_setup refuses are not offered (type IV: pffft[d]_hip_mdct_dct4_batch below). */
typedef enum { PFFFT_HIP_DCT2, PFFFT_HIP_DCT3, PFFFT_HIP_DST2, PFFFT_HIP_DST3 } pffft_hip_dct_kind_t;
typedef enum { PFFFT_HIP_DCT_NORM_NONE, PFFFT_HIP_DCT_NORM_ORTHO } pffft_hip_dct_norm_t;
typedef struct PFFFT_HIP_DctSetup PFFFT_HIP_DctSetup;
typedef struct PFFFTD_HIP_DctSetup PFFFTD_HIP_DctSetup;
PFFFT_HIP_DctSetup *pffft_hip_dct_new_setup(int N, pffft_hip_dct_kind_t kind, pffft_hip_dct_norm_t norm);
PFFFTD_HIP_DctSetup *pffftd_hip_dct_new_setup(int N, pffft_hip_dct_kind_t kind, pffft_hip_dct_norm_t norm);
void pffft_hip_dct_destroy_setup(PFFFT_HIP_DctSetup *);     /* NULL-safe */
void pffftd_hip_dct_destroy_setup(PFFFTD_HIP_DctSetup *);
int pffft_hip_dct_transform_batch(PFFFT_HIP_DctSetup *, const float *in, float *out, size_t batch, void *stream);
int pffftd_hip_dct_transform_batch(PFFFTD_HIP_DctSetup *, const double *in, double *out, size_t batch, void *stream);
/* Host arithmetic only, handles of both precisions.  pffft_hip_dct_route: "fused" / "composed" under the calling thread's selector; ""
 * for an invalid handle.  pffft_hip_dct_table: `count` values t_k from k = `first` (k <= N/2) as interleaved (re, im) pairs in the
 * setup's type into host_out - the values of the device's table.  0; non-zero for an invalid handle, a range beyond N/2 + 1 values or a
 * NULL host_out. */
const char *pffft_hip_dct_route(const void *setup);
int pffft_hip_dct_table(const void *setup, size_t first, size_t count, void *host_out);

/* MDCT / IMDCT FRAMES and the type-IV cosine transform (the lapped transform of audio and spectral codecs): frames of 2M samples at hop
 * M, M coefficients per frame, perfect reconstruction through time-domain alias cancellation (TDAC).  M = coefficients per frame,
 * h = n = M/2.  Legal M: M/2 is a length pffft[d]_new_setup(M/2, PFFFT_COMPLEX) takes (so M is a multiple of 32); NULL for any other M.
 * Creating a setup touches no device; the handle owns a complex setup of M/2, whose per-device behaviour carries over.
 * The core is the type-IV cosine sum without a factor, on ONE complex transform of half the length:
 *     C4(u)[k] = sum_{i<M} u[i] cos(pi (2k+1)(2i+1) / 4M)
 *     z[m] = (u[2m] + j u[M-1-2m]) a_m;  Z = the forward complex transform of length n, exactly as pffft_hip_transform_batch(...,
 *     PFFFT_FORWARD, ordered = 1) transforms a vector;  y_k = Z_k b_k;  C4[2k] = Re y_k, C4[M-1-2k] = -Im y_k
 * with a_m = exp(-j pi (4m+1) / 4M) and b_k = exp(-j pi k / M), m, k < n, evaluated in long double from exactly reduced integer phases
 * and rounded once.  Every route forms both complex products with the same operations (one product and one fused multiply-add per
 * component), so the routes agree bit for bit.
 *   pffft[d]_hip_mdct_dct4_batch: dense rows of M reals in and out, out == in IS LEGAL (any other overlap is refused).  out = 2 C4(in) -
 *     scipy.fft.dct(type=4, norm=None); the doubling is the last operation and exact.  dct4(dct4(x)) = 2M x.
 *   pffft[d]_hip_mdct_transform_batch: signal i (at signal + i signal_stride) holds (nframes + 1) M samples.  Frame f of it is
 *     p[j] = window[j] x_i[f M + j], j < 2M (window: 2M reals, NULL: no product; each product rounded once).  Fold, i < h:
 *     u[i] = (-p[3h-1-i]) - p[3h+i], u[h+i] = p[i] - p[M-1-i] (one rounded subtraction each, no fused multiply-add with the window
 *     product).  Row v = i nframes + f at coefs + v coefs_stride (0 = dense, M) is C4(u):
 *     X[k] = sum_{j<2M} p[j] cos(pi/M (j + 1/2 + M/2)(k + 1/2)), the textbook MDCT without a factor.
 *   pffft[d]_hip_mdct_overlap_add_batch: per frame v = C4(X_f), v1 = v[0..h), v2 = v[h..M), y_f = (v2, -reverse(v2), -reverse(v1), -v1)
 *     = sum_k X[k] cos(...) (2M values).  Every sample s < (nframes + 1) M is WRITTEN as scaling (sum_f window[s - f M] y_f[s - f M])
 *     over the at most two frames that cover it, f ascending, each product and each addition rounded once, the sum started from its
 *     first term (window NULL: the terms are y_f themselves).  With a Princen-Bradley window (w[j]^2 + w[j+M]^2 = 1) and scaling = 2/M
 *     the samples M ... nframes M - 1 reproduce the input; the first and the last M samples carry one aliased term.
 * All pointers are device pointers aligned to 16 bytes; signal, window and coefs must not overlap; calls are asynchronous on `stream`;
 * 0, else a hipError_t with its text in pffft_hip_last_error().  A call without rows or signals returns 0; nframes == 0 is refused.
 * Routes (pffft_hip_mdct_route names the one an entry takes under the calling thread's selector):
 *   "fused"     float, M = 512 / 1024: ONE kernel - the register-tiled complex transform of M/2 between two round trips of linear
 *               16-byte accesses through its own LDS image; the frame entry loads the four quarter frames, windows and folds them in
 *               registers.  4M bytes read from HBM and 4M written per frame or row.  The frame entry also needs signal_stride and
 *               coefs_stride to be multiples of 4 scalars, the overlap-add coefs_stride (its core runs the kernel into the scratch image,
 *               the gather follows).  Which (M, entry) cells run it by default is a measured table;
 *               pffft_hip_set_variant(141) runs it wherever it is legal, 140 never.
 *   "composed"  every setup: a fold / table kernel into a per-stream scratch image of rows x M, pffft[d]_hip_transform_batch in the
 *               canonical layout in place there, a table / scatter kernel into the result; the overlap-add gathers from the image.  The
 *               scratch holds at most 256 MiB (longer batches go through it in chunks on the stream, the overlap-add in runs of frames
 *               that re-transform the one frame reaching into a run); a call that would have to grow it - or build the tables of a first
 *               call - on a capturing stream returns hipErrorStreamCaptureUnsupported before any launch: run the call once before capturing.
 * DST-IV, type I, window-shape switching between frames, strided samples and lengths pffft_new_setup refuses are not offered. */
typedef struct PFFFT_HIP_MdctSetup PFFFT_HIP_MdctSetup;
typedef struct PFFFTD_HIP_MdctSetup PFFFTD_HIP_MdctSetup;
PFFFT_HIP_MdctSetup *pffft_hip_mdct_new_setup(int M);
PFFFTD_HIP_MdctSetup *pffftd_hip_mdct_new_setup(int M);
void pffft_hip_mdct_destroy_setup(PFFFT_HIP_MdctSetup *);     /* NULL-safe */
void pffftd_hip_mdct_destroy_setup(PFFFTD_HIP_MdctSetup *);
int pffft_hip_mdct_dct4_batch(PFFFT_HIP_MdctSetup *, const float *in, float *out, size_t rows, void *stream);
int pffftd_hip_mdct_dct4_batch(PFFFTD_HIP_MdctSetup *, const double *in, double *out, size_t rows, void *stream);
int pffft_hip_mdct_transform_batch(PFFFT_HIP_MdctSetup *, const float *signal, size_t signal_stride, size_t nsignals, size_t nframes,
                                   const float *window, float *coefs, size_t coefs_stride, void *stream);
int pffftd_hip_mdct_transform_batch(PFFFTD_HIP_MdctSetup *, const double *signal, size_t signal_stride, size_t nsignals, size_t nframes,
                                    const double *window, double *coefs, size_t coefs_stride, void *stream);
int pffft_hip_mdct_overlap_add_batch(PFFFT_HIP_MdctSetup *, const float *coefs, size_t coefs_stride, size_t nsignals, size_t nframes,
                                     const float *window, float scaling, float *signal, size_t signal_stride, void *stream);
int pffftd_hip_mdct_overlap_add_batch(PFFFTD_HIP_MdctSetup *, const double *coefs, size_t coefs_stride, size_t nsignals, size_t nframes,
                                      const double *window, double scaling, double *signal, size_t signal_stride, void *stream);
/* Host arithmetic only, handles of both precisions.  pffft_hip_mdct_route: `what` 0 = dct4, 1 = forward, 2 = overlap-add; "fused" /
 * "composed" under the calling thread's selector, "" for an invalid handle or another `what`.  pffft_hip_mdct_table: `count` values from
 * index `first` of a (which = 0) or b (which = 1), M/2 values each, as interleaved (re, im) pairs in the setup's type into host_out -
 * the values of the device's tables.  0; non-zero for an invalid handle, another `which`, a range beyond M/2 values or a NULL host_out. */
const char *pffft_hip_mdct_route(const void *setup, int what);
int pffft_hip_mdct_table(const void *setup, int which, size_t first, size_t count, void *host_out);

/* ANALYTIC SIGNALS of real rows (scipy.signal.hilbert): the step between real samples from a converter and the complex rows the mixers
 * and the channelizer work on.  With X = DFT(x) (forward, exp(-2 pi j n k / N)):
 *     Z[k] = c_k gain[k] X[k], 0 <= k <= N/2, c_0 = c_{N/2} = 1, c_k = 2 otherwise;   Z[k] = 0 above N/2;   z = IDFT(Z) / N
 * gain == NULL is all ones - exactly scipy.signal.hilbert.  A gain (N/2 + 1 host values, copied at setup) makes the call a one-sided
 * band-pass and an analytic signal in the same pass: the real -> IQ channel extraction in front of the mixers.
 *   in   batch dense rows of N reals
 *   out  PFFFT_HIP_ANALYTIC: batch dense rows of N interleaved complex values z;  PFFFT_HIP_HILBERT: rows of N reals Im z (the Hilbert
 *        transform of x);  PFFFT_HIP_ENVELOPE: rows of N reals |z|
 * Legal N: every N pffft[d]_new_setup(N, PFFFT_COMPLEX) takes; NULL for any other N.  Creating a setup touches no device; the handle
 * owns a complex setup of N.  The filter spectrum H[k] = c_k gain[k] is formed in double (exact for float gains), rounded once to the
 * setup's type and permuted into the inner setup's internal layout (exact); no transform is involved, because the spectrum is given.
 * The 1 / N rides on the convolution's scaling.  The envelope is ONE device function on every route: sqrt(fma(re, re, im im)) with the
 * correctly rounded square root and no scaling tricks - it overflows to +inf where re^2 + im^2 does and loses bits where that sum is
 * subnormal.
 * in / out are device pointers, 8-byte aligned on a real side and 16-byte aligned on the complex side.  out == in IS LEGAL for HILBERT
 * and ENVELOPE (any other overlap is refused); for ANALYTIC any overlap of in and out is refused.  The call is asynchronous on `stream`;
 * 0, else a hipError_t with its text in pffft_hip_last_error().  Validation happens before any device is touched: a NULL or foreign
 * handle or the other precision's (hipErrorInvalidHandle), another `what`, NULL, misaligned or overlapping in / out
 * (hipErrorInvalidValue) -> nothing launched.
 * Routes (pffft_hip_analytic_route names the one a call takes under the calling thread's selector):
 *   "fused"     float, N = 512 / 1024 / 2048 / 4096: ONE kernel - the fused convolution kernel of pffft_hip_convolve_batch with a loader
 *               that takes N reals (an exact zero as imaginary part) and a store that writes z, Im z or |z|: 12 N bytes per row for
 *               ANALYTIC and 8 N for the real outputs, where widening, convolve_batch and .imag / .abs() move 28 N and about 40 N.
 *               Which (N, what) cells run it by default is a measured table; pffft_hip_set_variant(145) runs it
 *               wherever it is legal, 144 never.
 *   "composed"  every setup.  ANALYTIC: a widening kernel writes (x, 0) straight into out, pffft[d]_hip_convolve_batch with the one
 *               broadcast H runs in place there - no scratch of this handle, so the call is legal on a capturing stream once the
 *               tables exist (the inner convolve_batch keeps its own rules).  HILBERT / ENVELOPE: the widening kernel into a per-stream
 *               scratch image of batch x N complex values, convolve_batch in place there, a narrowing kernel into out.  The image holds
 *               at most 256 MiB (longer batches go through it in chunks on the stream); a call that would have to grow it on a capturing
 *               stream returns hipErrorStreamCaptureUnsupported before any launch.
 * In the four fused cells convolve_batch itself runs the fused convolution kernel on the same configuration, H and scaling, and the
 * loader's zero is exact: THE ROUTES AGREE BIT FOR BIT in all three outputs.
 * THE FIRST CALL ON A SETUP BUILDS ITS TABLES: it allocates and synchronises the device, so it must happen BEFORE a stream capture (during
 * one it fails with hipErrorStreamCaptureUnsupported and launches nothing).  batch == 0 builds the tables, launches nothing else and
 * returns 0.  A setup serves ONE device, the one that is current at the first call (hipErrorInvalidDevice from another); any number of
 * streams and threads of that device may share it.
 * Two real rows per complex transform, a fused double kernel, strided rows, a down-mix fused into the store and the instantaneous phase
 * are not offered. */
typedef enum { PFFFT_HIP_ANALYTIC, PFFFT_HIP_HILBERT, PFFFT_HIP_ENVELOPE } pffft_hip_analytic_what_t;
typedef struct PFFFT_HIP_AnalyticSetup PFFFT_HIP_AnalyticSetup;
typedef struct PFFFTD_HIP_AnalyticSetup PFFFTD_HIP_AnalyticSetup;
PFFFT_HIP_AnalyticSetup *pffft_hip_analytic_new_setup(int N, const float *gain);     /* gain: NULL or N/2 + 1 host values */
PFFFTD_HIP_AnalyticSetup *pffftd_hip_analytic_new_setup(int N, const double *gain);
void pffft_hip_analytic_destroy_setup(PFFFT_HIP_AnalyticSetup *);     /* NULL-safe */
void pffftd_hip_analytic_destroy_setup(PFFFTD_HIP_AnalyticSetup *);
int pffft_hip_analytic_transform_batch(PFFFT_HIP_AnalyticSetup *, const float *in, float *out, size_t batch,
                                       pffft_hip_analytic_what_t what, void *stream);
int pffftd_hip_analytic_transform_batch(PFFFTD_HIP_AnalyticSetup *, const double *in, double *out, size_t batch,
                                        pffft_hip_analytic_what_t what, void *stream);
/* Host arithmetic only, handles of both precisions.  pffft_hip_analytic_route: "fused" / "composed" for `what` under the calling
 * thread's selector; "" for an invalid handle or another `what`.  pffft_hip_analytic_table: `count` values H[k] from k = `first` in
 * canonical order (N real scalars of the setup's type in all: c_k gain[k] up to N/2, zeros above) into host_out - the values the
 * device's spectrum holds.  0; non-zero for an invalid handle, a range beyond N values or a NULL host_out. */
const char *pffft_hip_analytic_route(const void *setup, int what);
int pffft_hip_analytic_table(const void *setup, size_t first, size_t count, void *host_out);

/* CROSS- AND AUTOCORRELATION OF ROWS (plain and PHAT-weighted): two rows that BOTH change per call, r[m] = sum_n conj(x[n]) y[n + m] -
 * delay estimation (TDOA, GCC-PHAT), burst / preamble search against a received reference, range profiles of pulse pairs, and the
 * autocorrelation (pitch, periodicity, Wiener-Khinchin).  (A FIXED template is pffft_hip_convolve_batch / pffastconv.)  A setup fixes
 *   N                     any length pffft[d]_new_setup(N, PFFFT_COMPLEX) takes
 *   real_rows             non-zero: rows of scalars in and out; zero: rows of interleaved (re, im) pairs in and out
 *   len_x, len_y          1 <= len <= N: samples per x row / y row
 *   lag0, nlags           the lag window: -N < lag0 < N, 1 <= nlags <= N
 * NULL for anything else.  Creating a setup touches no device; the handle owns a complex setup of N and has no tables.  With x and y
 * zero-extended to N samples and all indices taken mod N:
 *     X = DFT_N(x),  Y = DFT_N(y)                      (forward, unscaled)
 *     G[k] = W( conj(X[k]) Y[k] )
 *     r = IDFT_N(G)                                    (backward, unscaled)
 *     out[v][i] = s r[(lag0 + i) mod N],  i < nlags,   s = (T)(scaling / N) formed in double, rounded once
 * Real rows: len_x / len_y scalars in and nlags scalars out (Re r).  Complex rows: interleaved in and out.  With len_x + len_y - 1 <= N,
 * lag0 = -(len_x - 1), nlags = len_x + len_y - 1 this is scipy.signal.correlate(y, x, "full") (= np.correlate(y, x, "full")); with
 * len_x = len_y = nlags = N, lag0 = 0 it is the circular correlation.
 * The arithmetic between the transforms is ONE device function on every route, without fused multiply-adds in the product:
 *     c_re = Xr Yr + Xi Yi,  c_im = Xr Yi - Xi Yr      (every product and every sum rounded once)
 *     PFFFT_HIP_XCORR_PLAIN   G = (c_re, c_im)
 *     PFFFT_HIP_XCORR_PHAT    m = sqrt(fma(c_re, c_re, c_im c_im)) with the correctly rounded square root (the envelope's form),
 *                             G = (c_re / m, c_im / m) with correctly rounded divisions; m == 0 GIVES (+0, +0), never a NaN.
 * Consequences of the PHAT rule, stated rather than hidden: a bin with |c| above about 1.8e19 (float; 1.3e154 double) has m = inf and
 * comes out as ZERO; a bin whose c_re^2 + c_im^2 underflows to zero counts as EMPTY (zero); a non-finite input propagates (NaN).  The
 * multiplication by s is one product per stored component, followed by + 0: that addition is exact and only turns a -0 into +0, so that
 * A ROW WHOSE BINS ARE ALL EMPTY COMES OUT AS ALL +0 ON EVERY ROUTE (the inverse transform of an all +0 spectrum holds -0 in places on
 * some routes).
 * y == x (the same pointer; the setup must have len_x == len_y) is the AUTOCORRELATION: one load and one forward transform per row, G
 * from (X, X) through the same function.  c_im is then a - a = +0 exactly, so the result is BIT-IDENTICAL to the cross path on a copy
 * of x on the same route.  The routes themselves run different butterfly networks: they agree at the accuracy bar, not bit for bit.
 * x, y, out are device pointers, non-NULL for batch > 0, aligned to ONE ELEMENT (4 / 8 bytes real, 8 / 16 bytes complex, float /
 * double), rows dense.  out must not overlap x or y; x and y may overlap each other freely (both are only read).  batch == 0 binds the
 * device and returns 0.  The call is asynchronous on `stream`; 0, else a hipError_t with its text in pffft_hip_last_error().
 * Validation happens before any device is touched: a NULL or foreign handle or the other precision's (hipErrorInvalidHandle), an
 * unknown weight, NULL pointers, y == x with len_x != len_y, misalignment, overlap of out with an input (hipErrorInvalidValue) ->
 * nothing launched.
 * Routes (pffft_hip_xcorr_route names the one a call takes under the calling thread's selector):
 *   "fused"     float, N = 512 / 1024 / 2048 / 4096, both kinds, both weights, cross and auto: ONE kernel.  A workgroup slot runs the
 *               forward register-tiled transform on the x row, keeps its bins in registers, runs it again on the y row through the same
 *               LDS image, forms G, runs the backward transform and scatters the lag window: len_x + len_y elements read and nlags
 *               written per row pair, predicated element-sized non-temporal accesses.  Which cells run it by default is a measured
 *               table; pffft_hip_set_variant(147) runs it wherever it is legal, 146 never.
 *   "composed"  every setup: a pad kernel writes the zero-extended x rows and y rows into the two halves of a per-stream scratch image,
 *               ONE forward pffft[d]_hip_transform_batch (ordered) runs over both halves, a product kernel forms G in place on the y
 *               half, ONE backward transform_batch (ordered) runs on that half, a crop kernel stores the lag window.  The
 *               autocorrelation takes one row of the image per input row.  The image holds at most 256 MiB (longer batches go through
 *               it in chunks on the stream); a call that would have to grow it on a capturing stream returns
 *               hipErrorStreamCaptureUnsupported before any launch: run the call once before capturing.
 * A setup serves ONE device, the one that is current at the first call (hipErrorInvalidDevice from another); any number of streams and
 * threads of that device may share it.  THE FIRST CALL ON A SETUP BINDS IT (and the inner setup builds its device tables at its first
 * use): make it BEFORE a stream capture - during one it fails with hipErrorStreamCaptureUnsupported and launches nothing.
 * Two real rows packed into one complex transform, strided rows or a broadcast x, 16-byte fast paths for aligned lengths, SCOT / ML
 * weightings, normalised coefficients and a fused double or other-size kernel are not offered. */
typedef enum { PFFFT_HIP_XCORR_PLAIN = 0, PFFFT_HIP_XCORR_PHAT = 1 } pffft_hip_xcorr_weight_t;
typedef struct PFFFT_HIP_XcorrSetup PFFFT_HIP_XcorrSetup;
typedef struct PFFFTD_HIP_XcorrSetup PFFFTD_HIP_XcorrSetup;
PFFFT_HIP_XcorrSetup *pffft_hip_xcorr_new_setup(int N, int real_rows, int len_x, int len_y, int lag0, int nlags);
PFFFTD_HIP_XcorrSetup *pffftd_hip_xcorr_new_setup(int N, int real_rows, int len_x, int len_y, int lag0, int nlags);
void pffft_hip_xcorr_destroy_setup(PFFFT_HIP_XcorrSetup *);     /* NULL-safe */
void pffftd_hip_xcorr_destroy_setup(PFFFTD_HIP_XcorrSetup *);
int pffft_hip_xcorr_batch(PFFFT_HIP_XcorrSetup *, const float *x, const float *y, float *out, size_t batch, pffft_hip_xcorr_weight_t w,
                          float scaling, void *stream);
int pffftd_hip_xcorr_batch(PFFFTD_HIP_XcorrSetup *, const double *x, const double *y, double *out, size_t batch,
                           pffft_hip_xcorr_weight_t w, double scaling, void *stream);
/* Host arithmetic only, handles of both precisions: "fused" / "composed" for (weight, cross or auto) under the calling thread's
 * selector; "" for an invalid handle or another weight. */
const char *pffft_hip_xcorr_route(const void *setup, int weight, int is_auto);

/* ---- batched Fourier resampling of rows: N samples in, M samples out over the same span (scipy.signal.resample(x, M))
 * Matching a capture to the length a later setup takes, 2x / 4x / 8x interpolation before peak picking or delay estimation, decimating
 * a band-limited block.  A setup fixes
 *   N, M                  any lengths pffft[d]_new_setup(., PFFFT_COMPLEX) takes (so K = min(N, M) is even)
 *   real_rows             non-zero: rows of N scalars in and M scalars out; zero: rows of interleaved (re, im) pairs in and out
 * NULL for anything else.  Creating a setup touches no device; the handle owns a complex setup of N and one of M (one where N == M) and
 * has no tables.  With X = DFT_N(x) (forward, unscaled) and h = K / 2 the M-point spectrum Y is
 *     Y[k] = X[k], 0 <= k < h;      Y[M - k] = X[N - k], 1 <= k < h;      every other bin but those below is +0
 *     N == M: Y[h] = X[h];    M < N: Y[h] = X[h] + X[N - h] (one addition per component, no fused multiply-add);
 *     M > N: Y[h] = Y[M - h] = 0.5 X[h] (exact)
 *     out = s IDFT_M(Y) (backward, unscaled),  s = (T)(scaling / N) formed in double, rounded once, ONE product per component
 * Real rows: the real part of the same sum (the result of a real row is real in exact arithmetic).  scaling = 1 is
 * scipy.signal.resample(x, M): rows are periodic blocks, no window, no continuity between rows.
 * in, out are device pointers, non-NULL for batch > 0, aligned to ONE ELEMENT (4 / 8 bytes real, 8 / 16 bytes complex, float / double),
 * rows dense.  out must not overlap in: there is no in-place form, not even at N == M.  batch == 0 binds the device and returns 0.  The
 * call is asynchronous on `stream`; 0, else a hipError_t with its text in pffft_hip_last_error().  Validation happens before any device
 * is touched: a NULL or foreign handle or the other precision's (hipErrorInvalidHandle), NULL pointers, misalignment, overlap
 * (hipErrorInvalidValue) -> nothing launched.
 * Routes (pffft_hip_resample_route names the one a call takes under the calling thread's selector):
 *   "fused"     float, both kinds, N != M with both lengths from 512 / 1024 / 2048 / 4096: ONE kernel, 8N + 8M bytes of HBM per complex
 *               row (4N + 4M real), no scratch buffer.  Two register-tiled halves of different lengths joined in LDS: a workgroup slot
 *               of the larger length's threads takes r = max / min rows, runs the smaller transform on r sub-slots at once and the
 *               larger one r times, the cropped / zero-filled spectra crossing between them in natural order through the slot's LDS
 *               image.  Which cells run it by default is a measured table; pffft_hip_set_variant(157) runs it
 *               wherever it is legal, 156 never.
 *   "composed"  every setup: (real: a widening kernel,) a forward pffft[d]_hip_transform_batch (ordered) at N into a per-stream scratch
 *               buffer, a map kernel that writes every one of the M bins times s, a backward transform_batch (ordered) at M (complex:
 *               straight into out; real: a narrowing kernel).  N + M complex values of scratch per row, at most 256 MiB (longer
 *               batches go through it in chunks on the stream); a call that would have to grow it on a capturing stream returns
 *               hipErrorStreamCaptureUnsupported before any launch: run the call once before capturing.
 * The routes run different butterfly networks: they agree at the accuracy bar, not bit for bit.  Within a route the real kind equals
 * the real parts of the complex kind on the widened rows bit for bit.
 * A setup serves ONE device, the one that is current at the first call (hipErrorInvalidDevice from another); any number of streams and
 * threads of that device may share it.  THE FIRST CALL ON A SETUP BINDS IT (and the inner setups build their device tables at their
 * first use): make it BEFORE a stream capture - during one it fails with hipErrorStreamCaptureUnsupported and launches nothing.
 * Lengths the complex setup refuses, a spectral window, streaming continuity between rows, strided rows, two real rows per complex
 * transform, in-place operation and a fused double or other-length kernel are not offered. */
typedef struct PFFFT_HIP_ResampleSetup PFFFT_HIP_ResampleSetup;
typedef struct PFFFTD_HIP_ResampleSetup PFFFTD_HIP_ResampleSetup;
PFFFT_HIP_ResampleSetup *pffft_hip_resample_new_setup(int N, int M, int real_rows);
PFFFTD_HIP_ResampleSetup *pffftd_hip_resample_new_setup(int N, int M, int real_rows);
void pffft_hip_resample_destroy_setup(PFFFT_HIP_ResampleSetup *);     /* NULL-safe */
void pffftd_hip_resample_destroy_setup(PFFFTD_HIP_ResampleSetup *);
int pffft_hip_resample_batch(PFFFT_HIP_ResampleSetup *, const float *in, float *out, size_t batch, float scaling, void *stream);
int pffftd_hip_resample_batch(PFFFTD_HIP_ResampleSetup *, const double *in, double *out, size_t batch, double scaling, void *stream);
/* Host arithmetic only, handles of both precisions: "fused" / "composed" under the calling thread's selector; "" for an invalid handle. */
const char *pffft_hip_resample_route(const void *setup);

/* ---- batched 2-D complex transforms (numpy.fft.fft2 of a batch of images)
 * pffft[d]_hip_fft2_new_setup(rows, cols): both lengths must be ones a complex setup of that precision takes, NULL otherwise.  Creating a
 * setup touches no device; the handle owns one inner complex setup per distinct length (rows == cols shares one) and has no tables.
 * An image is rows x cols interleaved complex values, row-major and dense; `batch` images follow one another:
 *     out[u][v] = scaling * sum_r sum_c in[r][c] exp(-/+ 2 pi j (u r / rows + v c / cols))       (forward: the minus sign)
 * Forward with scaling = 1 is numpy.fft.fft2, backward is ifft2 * rows * cols.  Input and output are in natural order; there is no internal
 * layout.  `scaling` is ONE product per stored component in the last kernel of either route: scaling == 1 changes no bit.
 * in, out are device pointers, non-NULL for batch > 0, ALIGNED TO 16 BYTES (as the ordered transform_batch asks).  in == out (in place) is
 * legal on every route; any other overlap of the two ranges is refused.  `in` is never written unless it is `out`.  batch == 0 returns 0.
 * The call is asynchronous on `stream`; 0, else a hipError_t with its text in pffft_hip_last_error().  Validation happens before any device
 * is touched: a NULL or foreign handle or the other precision's (hipErrorInvalidHandle), an unknown direction, NULL pointers, misalignment,
 * partial overlap (hipErrorInvalidValue) -> nothing launched.
 * Routes (pffft_hip_fft2_route names the one a call takes under the calling thread's selector):
 *   "fused"     float, rows and cols out of 16 / 32 / 64 (nine shapes): ONE kernel.  A workgroup holds whole images in LDS: 16-byte loads
 *               of the image's dense run, a row pass and a column pass in place in a padded LDS image (one in-register 16- or 32-point
 *               transform per line, 64 points as 8 x 8 with W_64 from the inner setup's table), 16-byte stores.  One HBM read and one HBM
 *               write per image.  Which shapes run it by default is a measured table; pffft_hip_set_variant(149) runs
 *               it wherever it is legal, 148 never.
 *   "composed"  every setup: an ordered pffft[d]_hip_transform_batch of length cols over batch * rows rows from in to out, a transposing
 *               kernel [rows][cols] -> [cols][rows] per image into a per-stream scratch image, an ordered transform_batch of length rows
 *               over batch * cols rows in place there, the transposing kernel back into out, times scaling.  With scaling == 1 the result
 *               equals, bit for bit, the four steps a caller can do by hand (transform_batch, transpose, transform_batch, transpose).  The
 *               scratch holds at most 256 MiB (longer batches go through it in chunks of whole images on the stream); a call that would
 *               have to grow it on a capturing stream returns hipErrorStreamCaptureUnsupported before any launch: run the call once before
 *               capturing.
 * The two routes agree at the accuracy bar of a transform of rows * cols points, not bit for bit.
 * A setup serves ONE device, the one that is current at the first call (hipErrorInvalidDevice from another); any number of streams and
 * threads of that device may share it.  THE FIRST CALL ON A SETUP BINDS IT: make it BEFORE a stream capture - during one it fails with
 * hipErrorStreamCaptureUnsupported and launches nothing.
 * Real images with half-spectrum columns are the next entry (pffft[d]_hip_rfft2_*).  Strided or padded images, transforms along one axis
 * only, a fused double kernel, fused shapes beyond 64 and mixed-radix tiles, multi-device shards of one setup and 3-D transforms are not
 * offered.  Circular 2-D convolution / correlation of the images with a spectrum is pffft[d]_hip_fft2_convolve_batch below. */
typedef struct PFFFT_HIP_Fft2Setup PFFFT_HIP_Fft2Setup;
typedef struct PFFFTD_HIP_Fft2Setup PFFFTD_HIP_Fft2Setup;
PFFFT_HIP_Fft2Setup *pffft_hip_fft2_new_setup(int rows, int cols);
PFFFTD_HIP_Fft2Setup *pffftd_hip_fft2_new_setup(int rows, int cols);
void pffft_hip_fft2_destroy_setup(PFFFT_HIP_Fft2Setup *);     /* NULL-safe */
void pffftd_hip_fft2_destroy_setup(PFFFTD_HIP_Fft2Setup *);
int pffft_hip_fft2_transform_batch(PFFFT_HIP_Fft2Setup *, const float *in, float *out, size_t batch, pffft_direction_t direction,
                                   float scaling, void *stream);
int pffftd_hip_fft2_transform_batch(PFFFTD_HIP_Fft2Setup *, const double *in, double *out, size_t batch, pffft_direction_t direction,
                                    double scaling, void *stream);
/* Host arithmetic only, handles of both precisions: "fused" / "composed" under the calling thread's selector; "" for an invalid handle. */
const char *pffft_hip_fft2_route(const void *setup);

/* ---- batched 2-D spectral convolution on the fft2 handle (numpy: ifft2(fft2(x) * G) of a batch of images)
 *     out = scaling * IFFT2u( FFT2(in) . G ),   G = H where conj_h == 0, G = conj(H) otherwise
 * FFT2 and IFFT2u are the forward and the UNNORMALISED backward transform of pffft[d]_hip_fft2_transform_batch: scaling = 1 / (rows * cols)
 * gives numpy's ifft2(fft2(x) * G).  conj_h != 0 is the circular cross-correlation against the template whose spectrum is H.  Images are
 * those of the fft2 entry (rows x cols interleaved complex values, dense, row-major, natural order); H is a spectrum in that same natural
 * order, as fft2_transform_batch forward writes it: ONE image of it serves every image of the batch where h_broadcast != 0, `batch` images
 * of it are read otherwise.  There is no accumulate form.  The product is a.x h.x - a.y h.y, a.x h.y + a.y h.x (conj_h: a.x h.x + a.y h.y,
 * a.y h.x - a.x h.y), every product and sum rounded once, on every route; `scaling` is ONE product per stored component in the last kernel
 * of either route: scaling == 1 changes no bit.
 * in, H, out are device pointers, non-NULL for batch > 0, ALIGNED TO 16 BYTES.  in == out (in place) is legal on every route; any other
 * overlap of in and out is refused, and so is H overlapping out.  `in` and H are never written (in: unless it is out).  batch == 0 returns 0.
 * The call is asynchronous on `stream`; 0, else a hipError_t with its text in pffft_hip_last_error() (it opens with "fft2 convolve: ").
 * Validation happens before any device is touched, in this order: the handle (hipErrorInvalidHandle: NULL, foreign, the other
 * precision's), the empty call, NULL pointers, alignment, the two overlap rules (hipErrorInvalidValue) -> nothing launched.
 * Routes (pffft_hip_fft2_convolve_route names the one a call takes under the calling thread's selector):
 *   "fused"     float, h_broadcast != 0, rows and cols out of 16 / 32 / 64: ONE kernel, one HBM read and one HBM write per image.  The image
 *               stays in LDS between the transforms: row pass forward, a column step that transforms a column forward, multiplies by G and
 *               transforms it backward in registers (64 points: through the transposed 8 x 8 network, digit-reversed in, natural out), row
 *               pass backward, 16-byte stores from natural positions.  G sits in registers across a workgroup's images.  Which shapes run
 *               it by default is a measured table; pffft_hip_set_variant(153) runs it wherever it is legal, 152 never.
 *   "composed"  every setup, either h_broadcast: the handle's own forward transform from in into out with scaling 1, a product kernel in
 *               place in out, the handle's own backward transform in place in out with `scaling` - the transforms on whichever route
 *               pffft_hip_fft2_route names under the calling thread's selector.  It equals those three steps made by hand bit for bit and
 *               has no scratch of its own; what the inner transforms need (their scratch image, its capture rule) follows their rules.
 * The two routes agree at the accuracy bar of a convolution of rows * cols points, not bit for bit.
 * Device binding, first call and capture are the handle's (above): ONE device per setup, THE FIRST CALL ON A SETUP BINDS IT - make it
 * before a stream capture.
 * Real images are pffft[d]_hip_rfft2_convolve_batch on the rfft2 handle (below): half the bytes and half the arithmetic.  An accumulate
 * form, linear (zero-padded) convolution and cropping, two images that both change per call, a fused per-image H or double kernel and
 * shapes beyond 64 are not offered. */
int pffft_hip_fft2_convolve_batch(PFFFT_HIP_Fft2Setup *, const float *in, const float *H, float *out, float scaling, size_t batch, int conj_h,
                                  int h_broadcast, void *stream);
int pffftd_hip_fft2_convolve_batch(PFFFTD_HIP_Fft2Setup *, const double *in, const double *H, double *out, double scaling, size_t batch,
                                   int conj_h, int h_broadcast, void *stream);
/* Host arithmetic only, handles of both precisions: "fused" / "composed" under the calling thread's selector; "" for an invalid handle. */
const char *pffft_hip_fft2_convolve_route(const void *setup, int h_broadcast);

/* ---- batched 2-D real transforms (numpy.fft.rfft2 / irfft2 of a batch of images)
 * pffft[d]_hip_rfft2_new_setup(rows, cols): rows must be a length a COMPLEX setup of that precision takes, cols one a REAL setup takes
 * (so cols >= 32), NULL otherwise.  Creating a setup touches no device; the handle owns a real inner setup of length cols, a complex one of
 * length rows (and, for the fused row pass of cols = 64, a complex one of length 64 where rows is another length) and has no tables.
 * bins = cols / 2 + 1.  Images are dense and row-major, `batch` of them one after another:
 *   forward    rows x cols reals in, rows x bins interleaved complex values out:
 *                  out[u][v] = scaling * sum_r sum_c in[r][c] exp(-2 pi j (u r / rows + v c / cols)),  v = 0 ... cols / 2
 *              with scaling = 1 this is numpy.fft.rfft2.
 *   backward   rows x bins complex values in, rows x cols reals out: numpy.fft.irfft2(X, s = (rows, cols)) * rows * cols * scaling.
 *              A half-spectrum that is not Hermitian is read by numpy's rule: after the transform along the columns the imaginary parts
 *              of the columns 0 and cols / 2 contribute nothing - only the Hermitian part (X[u] + conj X[rows - u]) / 2 of those two
 *              columns counts.  Every route obeys it.
 * `scaling` is ONE product per stored component and scaling == 1 changes no bit: forward in the last kernel of either route; backward in
 * the store of the fused kernel, and on the composed route in the packing kernel AHEAD of the last transform_batch (which has no scaling
 * argument) - so there a power of two reproduces the product of the unscaled result bit for bit, any other factor to rounding.
 * in, out are device pointers, non-NULL for batch > 0, ALIGNED TO 16 BYTES (every image then starts on 16 bytes too: rows is a multiple of
 * 16).  The two sides differ in size (4 rows cols against 8 rows bins bytes in float), so there is NO in-place form: in == out and every
 * partial overlap of the two ranges, each with its own byte count for the direction, are refused.  `in` is never written.  batch == 0
 * returns 0.  The call is asynchronous on `stream`; 0, else a hipError_t with its text in pffft_hip_last_error().  Validation happens before
 * any device is touched, in this order: a NULL or foreign handle or the other precision's (hipErrorInvalidHandle), an unknown direction,
 * the empty call, NULL pointers, misalignment, overlap (hipErrorInvalidValue) -> nothing launched.
 * Routes (pffft_hip_rfft2_route names the one a call takes under the calling thread's selector):
 *   "fused"     float, rows out of 16 / 32 / 64 and cols out of 32 / 64 (six shapes): ONE kernel, no scratch.  A workgroup holds whole
 *               images in LDS: 16-byte loads of the image's dense run, the rows 2 l and 2 l + 1 as the real and imaginary parts of one
 *               complex line, a row pass of rows / 2 lines, an untangling step, a column pass of cols / 2 columns (columns 0 and cols / 2
 *               travel as one), 16-byte stores.  One HBM read and one HBM write per image.  Which shapes run it by default is a measured
 *               table; pffft_hip_set_variant(151) runs it wherever it is legal, 150 never.
 *   "composed"  every setup.  Forward: an ordered real pffft[d]_hip_transform_batch of length cols over batch * rows rows, an unpacking and
 *               transposing kernel [rows][cols packed] -> [bins][rows] into a per-stream scratch image, an ordered complex
 *               transform_batch of length rows over batch * bins rows in place there, a transposing kernel into out, times scaling.
 *               Backward: the transposing kernel [rows][bins] -> [bins][rows] into the scratch, the complex transform_batch there, a
 *               transposing and packing kernel into canonical packed real spectra in out, times scaling (it drops the imaginary parts of
 *               the columns 0 and cols / 2: numpy's rule), the ordered real transform_batch in place in out.  With scaling == 1 either
 *               direction equals, bit for bit, the same steps done by hand.  The scratch holds at most 256 MiB (longer batches go through
 *               it in chunks of whole images on the stream); a call that would have to grow it on a capturing stream returns
 *               hipErrorStreamCaptureUnsupported before any launch: run the call once before capturing.
 * The two routes agree at the accuracy bar of a transform of rows * cols points, not bit for bit.
 * A setup serves ONE device, the one that is current at the first call (hipErrorInvalidDevice from another); any number of streams and
 * threads of that device may share it.  THE FIRST CALL ON A SETUP BINDS IT: make it BEFORE a stream capture - during one it fails with
 * hipErrorStreamCaptureUnsupported and launches nothing.
 * Padded or strided rows (and therefore in place), cols = 16, a fused double kernel, fused lengths beyond 64 and mixed-radix tiles,
 * transforms along one axis only, multi-device shards of one setup and 3-D transforms are not offered. */
typedef struct PFFFT_HIP_Rfft2Setup PFFFT_HIP_Rfft2Setup;
typedef struct PFFFTD_HIP_Rfft2Setup PFFFTD_HIP_Rfft2Setup;
PFFFT_HIP_Rfft2Setup *pffft_hip_rfft2_new_setup(int rows, int cols);
PFFFTD_HIP_Rfft2Setup *pffftd_hip_rfft2_new_setup(int rows, int cols);
void pffft_hip_rfft2_destroy_setup(PFFFT_HIP_Rfft2Setup *);     /* NULL-safe */
void pffftd_hip_rfft2_destroy_setup(PFFFTD_HIP_Rfft2Setup *);
int pffft_hip_rfft2_transform_batch(PFFFT_HIP_Rfft2Setup *, const float *in, float *out, size_t batch, pffft_direction_t direction,
                                    float scaling, void *stream);
int pffftd_hip_rfft2_transform_batch(PFFFTD_HIP_Rfft2Setup *, const double *in, double *out, size_t batch, pffft_direction_t direction,
                                     double scaling, void *stream);
/* Host arithmetic only, handles of both precisions: "fused" / "composed" under the calling thread's selector; "" for an invalid handle. */
const char *pffft_hip_rfft2_route(const void *setup);

/* ---- batched 2-D spectral convolution of real images on the rfft2 handle (numpy: irfft2(rfft2(x) * G, s = (rows, cols)) of a batch)
 *     out = scaling * rows * cols * numpy.fft.irfft2( numpy.fft.rfft2(in) . G, s = (rows, cols) ),   G = H where conj_h == 0, else conj(H)
 * in and out are `batch` dense row-major images of rows x cols reals, as the rfft2 entry takes them; H is a half-spectrum of rows x bins
 * interleaved complex values (bins = cols / 2 + 1) in natural order, as rfft2_transform_batch forward writes it: ONE of it serves every
 * image of the batch where h_broadcast != 0, `batch` of them are read otherwise.  scaling = 1 / (rows * cols) gives numpy's
 * irfft2(rfft2(x) * G); conj_h != 0 is the circular cross-correlation against the real template whose half-spectrum is H.  There is no
 * accumulate form.
 * H NEED NOT BE HERMITIAN in the columns 0 and cols / 2: the result is what numpy's irfft2 makes of the product - only the Hermitian part
 * (Y[u] + conj Y[rows - u]) / 2 along u of those two product columns counts (the backward rule of the rfft2 entry).  Every route obeys it.
 * The product is a.x h.x - a.y h.y, a.x h.y + a.y h.x (conj_h: a.x h.x + a.y h.y, a.y h.x - a.x h.y), every product and sum rounded
 * once, on every route.  `scaling` follows the backward transform's rule above: ONE product per stored component, scaling == 1 changes
 * no bit; in the store of the fused kernel, and on the composed route where the backward transform of the handle applies it (composed
 * inner transform: ahead of its last transform_batch, so there a power of two reproduces the product of the unscaled result bit for bit,
 * any other factor to rounding).
 * in, H, out are device pointers, non-NULL for batch > 0, ALIGNED TO 16 BYTES.  The two sides have the same size, so in == out (in place)
 * is legal on every route; any other overlap of in and out is refused, and so is H (one half-spectrum where it is broadcast, `batch` of
 * them otherwise) overlapping out.  `in` and H are never written (in: unless it is out).  batch == 0 returns 0.  The call is asynchronous
 * on `stream`; 0, else a hipError_t with its text in pffft_hip_last_error() (it opens with "rfft2 convolve: ").  Validation happens before
 * any device is touched, in this order: the handle (hipErrorInvalidHandle: NULL, foreign, the other precision's), the empty call, NULL
 * pointers, alignment, the two overlap rules (hipErrorInvalidValue) -> nothing launched.
 * Routes (pffft_hip_rfft2_convolve_route names the one a call takes under the calling thread's selector):
 *   "fused"     float, h_broadcast != 0, the six fused shapes of the rfft2 entry (rows 16 / 32 / 64, cols 32 / 64): ONE kernel, one HBM read
 *               and one HBM write of 4 rows cols bytes per image.  The image stays in LDS: the real-side load, a row pass over rows / 2
 *               lines, the untangling step, a column step that transforms a column forward, multiplies by G and transforms it backward
 *               (64 rows: through the transposed 8 x 8 network), the rebuilding step, the backward row pass, the real-side store.  The
 *               columns 0 and cols / 2 travel as one packed column, whose product takes the Hermitian parts named above.  Which shapes run
 *               it by default is a measured table; pffft_hip_set_variant(155) runs it wherever it is legal, 154 never.
 *   "composed"  every setup, either h_broadcast.  Per chunk of whole images through a second per-stream scratch of the handle, which holds
 *               the half-spectra (at most 256 MiB; longer batches go through it in chunks on the stream): the handle's own forward
 *               transform from in into the scratch with scaling 1, a product kernel in place there, the handle's own backward transform
 *               into out with `scaling` - the transforms on whichever route pffft_hip_rfft2_route names under the calling thread's
 *               selector.  It equals those three calls made by hand bit for bit.  A call that would have to grow either scratch (this one,
 *               or the scratch image of a composed inner transform) on a capturing stream returns hipErrorStreamCaptureUnsupported before
 *               anything is launched: run the call once on the stream before capturing.
 * The two routes agree at the accuracy bar of a convolution of rows * cols points, not bit for bit.
 * Device binding, first call and capture are the handle's (above): ONE device per setup, THE FIRST CALL ON A SETUP BINDS IT - make it
 * before a stream capture.
 * An accumulate form, linear (zero-padded) convolution and valid-region cropping, two images that both change per call (2-D correlation
 * of image pairs, PHAT), a fused per-image H or double kernel, cols = 16, shapes beyond 64 and strided images are not offered. */
int pffft_hip_rfft2_convolve_batch(PFFFT_HIP_Rfft2Setup *, const float *in, const float *H, float *out, float scaling, size_t batch, int conj_h,
                                   int h_broadcast, void *stream);
int pffftd_hip_rfft2_convolve_batch(PFFFTD_HIP_Rfft2Setup *, const double *in, const double *H, double *out, double scaling, size_t batch,
                                    int conj_h, int h_broadcast, void *stream);
/* Host arithmetic only, handles of both precisions: "fused" / "composed" under the calling thread's selector; "" for an invalid handle. */
const char *pffft_hip_rfft2_convolve_route(const void *setup, int h_broadcast);

/* ---- batched 2-D cosine / sine transforms of types II and III (scipy.fft.dctn / idctn, dstn / idstn of a batch of real tiles)
 * pffft[d]_hip_dct2d_new_setup(rows, cols, kind, norm): both lengths must be ones pffft_new_setup(N, PFFFT_REAL) of that precision takes
 * (a multiple of 32, 2^a 3^b 5^c: at least 32); NULL, with the text in pffft_hip_last_error(), for any other length and for a kind or a
 * norm out of range.  Creating a setup touches no device.  The handle owns two pffft[d]_hip_dct_* handles, one of length cols and one of
 * length rows (one where they are equal): the tables t_k and the product are the 1-D entry's.
 * in and out are `batch` dense row-major images of rows x cols reals.  out is the 1-D transform of the DCT definitions above (kind, norm)
 * applied along the columns index (every row of an image), then along the rows index - kind and norm are the same on both axes:
 *     scipy.fft.dctn / dstn(x, type = 2 | 3, norm = None | "ortho") over the last two axes.
 * There is no scaling argument, as in the 1-D entry.  Unnormalised, type III after type II returns 4 rows cols x; with ORTHO it returns x.
 * in, out are device pointers, non-NULL for batch > 0, ALIGNED TO 16 BYTES.  in == out (in place) IS LEGAL; any partial overlap of the two
 * ranges of batch * rows * cols scalars is refused.  `in` is never written unless it is out.  batch == 0 returns 0.  The call is
 * asynchronous on `stream`; 0, else a hipError_t with its text in pffft_hip_last_error() (it opens with "pffft_hip: dct2d: ").  Validation happens
 * before any device is touched, in this order: a NULL or foreign handle (a 1-D dct handle is one) or the other precision's
 * (hipErrorInvalidHandle), the empty call, NULL pointers, misalignment, overlap (hipErrorInvalidValue) -> nothing launched.
 * Routes (pffft_hip_dct2d_route names the one a call takes under the calling thread's selector):
 *   "fused"     float, rows and cols out of 32 / 64 (four shapes, all four kinds): ONE kernel, no scratch.  A workgroup holds whole images
 *               in LDS: 16-byte loads of the image's dense run, Makhoul's permutation in the load's index map, the rows 2 l and 2 l + 1 as
 *               the real and imaginary parts of one complex line, a row pass of rows / 2 lines, an untangling step that multiplies by t_k
 *               of length cols and leaves two real columns per complex column, a column pass of cols / 2 columns, the same step with
 *               t_k of length rows, 16-byte stores (type III the mirror).  One HBM read and one HBM write of 4 rows cols bytes per
 *               image.  Both tables are the 1-D handles' device tables.  Which (shape, kind) cells run it by default is a measured table
 *               (DESIGN.md §3.33); pffft_hip_set_variant(159) runs it wherever it is legal, 158 never.
 *   "composed"  every setup: pffft[d]_hip_dct_transform_batch of length cols over batch * rows rows from in into out, a real transposing
 *               kernel [rows][cols] -> [cols][rows] into a per-stream scratch image, dct_transform_batch of length rows over batch * cols
 *               rows in place there, the transposing kernel back into out.  The inner calls take whichever 1-D route
 *               pffft_hip_dct_route names under the calling thread's selector.  The result equals, bit for bit, the same four steps done
 *               by hand.  The scratch holds at most 256 MiB (longer batches go through it in chunks of whole images on the stream); a
 *               call that would have to grow it on a capturing stream returns hipErrorStreamCaptureUnsupported before any launch: run
 *               the call once on the stream before capturing.
 * The two routes run different networks: they agree at the accuracy bar of a transform of rows * cols points, not bit for bit.
 * A setup serves ONE device, the one that is current at the first call (hipErrorInvalidDevice from another); any number of streams and
 * threads of that device may share it.  THE FIRST CALL ON A SETUP BINDS IT: make it BEFORE a stream capture - during one it fails with
 * hipErrorStreamCaptureUnsupported and launches nothing.
 * Lengths below 32 (8 x 8 and 16 x 16 codec blocks), types I and IV, a different kind per axis, transforms along one axis only,
 * strided images, a fused double kernel and fused lengths beyond 64 are not offered. */
typedef struct PFFFT_HIP_Dct2dSetup PFFFT_HIP_Dct2dSetup;
typedef struct PFFFTD_HIP_Dct2dSetup PFFFTD_HIP_Dct2dSetup;
PFFFT_HIP_Dct2dSetup *pffft_hip_dct2d_new_setup(int rows, int cols, pffft_hip_dct_kind_t kind, pffft_hip_dct_norm_t norm);
PFFFTD_HIP_Dct2dSetup *pffftd_hip_dct2d_new_setup(int rows, int cols, pffft_hip_dct_kind_t kind, pffft_hip_dct_norm_t norm);
void pffft_hip_dct2d_destroy_setup(PFFFT_HIP_Dct2dSetup *);     /* NULL-safe */
void pffftd_hip_dct2d_destroy_setup(PFFFTD_HIP_Dct2dSetup *);
int pffft_hip_dct2d_transform_batch(PFFFT_HIP_Dct2dSetup *, const float *in, float *out, size_t batch, void *stream);
int pffftd_hip_dct2d_transform_batch(PFFFTD_HIP_Dct2dSetup *, const double *in, double *out, size_t batch, void *stream);
/* Host arithmetic only, handles of both precisions: "fused" / "composed" under the calling thread's selector; "" for an invalid handle. */
const char *pffft_hip_dct2d_route(const void *setup);

/* ---- batched band energies of framed transforms: mel / Bark / ERB / octave bands, channel powers, rebinned spectrograms
 *
 * Row v of `out` is the |X|^2 row of frame v reduced along frequency by a sparse bank of weighted bands, without the nframes x P
 * intermediate and without a dense matrix product.
 *
 * pffft[d]_hip_bands_new_setup(N, transform, nbands, first, count, weights).  The handle owns one inner setup of length N (real or complex)
 * and a host copy of the bank; the arrays are HOST arrays and are copied.  P = N/2 + 1 bins for a real setup, N for a complex one
 * (pffft_hip_bands_bins; pffft_hip_bands_count returns nbands).  `weights` holds sum(count[b]) values, band after band: entry j of band b
 * multiplies bin first[b] + j.  Bands may overlap, repeat and come in any order; count[b] == 0 and negative weights are legal.  NULL, with
 * a text in pffft_hip_last_error() (it opens with "pffft_hip: bands: ") and no device touched, for: an N that is no length of that
 * transform, nbands == 0, a NULL array, first[b] + count[b] > P, a weight that is not finite.  A handle serves ONE device: the first call
 * binds it to the current device and uploads the bank (not during a stream capture: run the call once before capturing).
 *
 * pffft[d]_hip_bands_batch.  Framing, `window` (NULL = no product), `hop`, `signal_stride`, the frame numbering v = i*nframes + f, the
 * sample / scalar rules and the pointer rules are exactly those of pffft_hip_frames_transform_batch.  Row v holds nbands scalars at
 * out + v*out_stride (0 = dense); out needs scalar alignment only and must not overlap signal.
 * ARITHMETIC - THE ORDER IS PART OF THE CONTRACT.  p[k] is the value pffft_hip_frames_transform_batch(..., PFFFT_HIP_FRAMES_POWER) produces
 * for that frame, bit for bit (DC and Nyquist as that output forms them).  Band b's entries are cut into segments of PFFFT_HIP_BANDS_SEG
 * consecutive entries, counted from the band's first entry (the last segment may be shorter).  A segment's partial is the sum of
 * fl(w_j * p[first + j]), j ascending, started from its first term; the band's value e_b is the sum of its segment partials, segment
 * ascending, started from the first.  Every product and every addition is rounded once: no FMA, no atomics.  An empty band gives +0.
 *     PFFFT_HIP_BANDS_ENERGY  stores fl(scaling * e_b); `floor` is not read
 *     PFFFT_HIP_BANDS_LOG     stores log(max(fl(scaling * e_b), floor)), the natural logarithm of the device's math library (a NaN passes
 *                             through the maximum); floor must be finite and > 0
 * Up to 16 entries the order is the plain left-to-right sum.  The result is deterministic and equal on every route, LOG included.
 * ROUTES (pffft_hip_bands_route names the one a call takes under the calling thread's selector, pffft_hip_set_variant: 160 = always
 * composed, 161 = fused wherever it is legal; it assumes 16-byte aligned pointers; signal_stride = 0: one signal; "" for an invalid handle
 * or hop == 0; host arithmetic only).  Real float setups of N = 1024 / 2048 / 4096 run FUSED when hop and signal_stride are multiples of 4
 * and signal and window are 16-byte aligned: the framed kernel leaves the |X|^2 values of a frame in LDS, forms the band sums there and
 * stores nbands scalars per frame - hop + nbands scalars of HBM traffic per frame.  Descriptors and weights are read through L2, so the
 * fused route puts no cap on nbands or on sum(count); it keeps one partial per segment of the bank in LDS, so the bank may hold at most
 * 658 / 1298 / 2578 segments, sum over b of ceil(count[b] / 16), at N = 1024 / 2048 / 4096 (an 80-band mel bank has 104 / 162 / 286).
 * Banks beyond that run composed, and pffft_hip_bands_route says so.
 * Everything else - double, complex, other sizes, hops and alignments - is COMPOSED: the |X|^2 rows of
 * whole chunks of frames go into a scratch of the handle (one buffer per stream, at most 256 MiB), produced by the inner setup's own
 * pffft_hip_frames_transform_batch, and a row kernel reduces them.  A chunk is whole signals; where one signal's rows exceed the cap, runs
 * of frames of one signal.  The scratch grows outside HIP graph capture only: a call that would have to grow it while `stream` is
 * capturing fails with hipErrorStreamCaptureUnsupported and launches nothing.
 * Validation happens before any device is touched: a NULL or foreign handle or the other precision's handle, an unknown `what`, a floor
 * that is not finite or not > 0 for LOG, what pffft_hip_frames_transform_batch refuses (hop == 0, a signal_stride smaller than one
 * signal's scalars when nsignals > 1, a NULL signal / out), an out_stride smaller than nbands -> non-zero, nothing launched.
 * nsignals == 0 or nframes == 0 -> 0, nothing launched. */
enum { PFFFT_HIP_BANDS_ENERGY = 0, PFFFT_HIP_BANDS_LOG = 1 };
#define PFFFT_HIP_BANDS_SEG 16
typedef struct PFFFT_HIP_Bands_Setup PFFFT_HIP_Bands_Setup;
typedef struct PFFFTD_HIP_Bands_Setup PFFFTD_HIP_Bands_Setup;
PFFFT_HIP_Bands_Setup *pffft_hip_bands_new_setup(int N, pffft_transform_t transform, unsigned nbands, const unsigned *first,
                                                 const unsigned *count, const float *weights);
PFFFTD_HIP_Bands_Setup *pffftd_hip_bands_new_setup(int N, pffft_transform_t transform, unsigned nbands, const unsigned *first,
                                                   const unsigned *count, const double *weights);
void pffft_hip_bands_destroy_setup(PFFFT_HIP_Bands_Setup *);     /* NULL-safe */
void pffftd_hip_bands_destroy_setup(PFFFTD_HIP_Bands_Setup *);
int pffft_hip_bands_batch(PFFFT_HIP_Bands_Setup *, const float *signal, size_t signal_stride, size_t nsignals, size_t nframes, size_t hop,
                          const float *window, float scaling, float floor, int what, float *out, size_t out_stride, void *stream);
int pffftd_hip_bands_batch(PFFFTD_HIP_Bands_Setup *, const double *signal, size_t signal_stride, size_t nsignals, size_t nframes, size_t hop,
                           const double *window, double scaling, double floor, int what, double *out, size_t out_stride, void *stream);
const char *pffft_hip_bands_route(const void *setup, size_t hop, size_t signal_stride);
unsigned pffft_hip_bands_count(const void *setup);   /* nbands; 0 for an invalid handle */
unsigned pffft_hip_bands_bins(const void *setup);    /* P; 0 for an invalid handle */

/* Overlap-save FIR on device-resident signal/output (same block schedule as pffastconv_apply,
 * src/pffastconv.c:204-261): returns the number of output samples written, or -1 on error. */
int pffastconv_hip_apply_device(PFFASTCONV_Setup *, const float *d_input, int inputLen, float *d_output,
                                int applyFlush, void *stream);
/* The same filter over `nsignals` independent signals of `inputLen` samples each (complex I/O: complex samples), signal
 * i at d_input + i*inputStride and its output at d_output + i*outputStride (strides in floats; inputStride >= the signal's
 * floats, outputStride >= the floats one signal produces - both checked, -1 otherwise; any nsignals).
 * Every signal is processed exactly as one pffastconv_hip_apply_device call would (src/pffastconv.c:133-263 per signal,
 * same block schedule, same number of outputs — the return value, per signal); all blocks of all signals share one
 * launch so that reference-sized calls (BASELINE configs[3]: 255 blocks) fill the chip.  -1 on error.
 * STREAM CAPTURE: the filter tables are built on first use PER ROUTE (pffastconv_hip_route: the reference-block spectrum at the first call
 * of all, then the big-block spectrum, the partition spectra, the time-domain taps, the coefficient table of the fused32 / split1 kernel,
 * the work image of the composed path per stream and size) with allocations and a synchronisation of the null stream.  A call on a
 * capturing stream that lacks one of them returns -1, launches nothing, changes nothing, and pffft_hip_last_error() names "graph capture"
 * and the missing table: run a call of the SAME shape (signals x length: the route depends on both) once before capturing - a warm-up on
 * a short signal takes another route.  After a capture has recorded a launch of the setup, nothing it reads is freed before
 * pffastconv_destroy_setup: a call from another device, and a call whose route needs big blocks of another length than the recorded
 * one, are refused (-1, with a text) instead of rebuilding the tables; a work image that is outgrown later is kept beside the new one. */
int pffastconv_hip_apply_batch(PFFASTCONV_Setup *, const float *d_input, int inputLen, size_t inputStride,
                               float *d_output, size_t outputStride, int nsignals, int applyFlush, void *stream);
/* Host arithmetic only.  pffastconv_hip_route: the route a pffastconv_hip_apply_batch call of `nsignals` signals of `inputLen` samples
 * takes under the calling thread's selector (pffft_hip_set_variant) and the process environment, written into buf as
 * "<kernel short name> <cfg> <block> <step> <blocks> <last>": the kernel that takes the call's blocks, its configuration (the stride of
 * fastconv_td_kernel, "big" / "ref" = which filter table a 16384-sample kernel reads, "W4" / "W8" wavefronts of fastconv_split1_kernel,
 * the FirCfg of fastconv_fused_kernel, "" where a kernel has one form), the internal block length, its valid samples, the blocks per
 * signal and the outputs of the last one (the time-domain kernel: tiles of the float stream); "" for a call that launches nothing.
 * `cus` > 0 is taken as the device's number of compute units and no device is touched; `cus` <= 0 asks the current device.  Returns the
 * length of the text, -1 for an invalid handle or a buffer too small for the text and its terminating 0. */
int pffastconv_hip_route(const PFFASTCONV_Setup *, int inputLen, int nsignals, int applyFlush, int cus, char *buf, size_t len);

/* Name of the kernel family a setup dispatches to ("c1024_f32", "tiled", "tiny", "stockham", "stockham_rt" = the same kernel on a
 * run-time plan because the size has no generated compile-time plan (no legal size today), "fourstep" = tile / streaming
 * passes beyond LDS): for tests/bench. */
const char *pffft_hip_kernel_name(const void *setup);
/* The routes of a setup as text: one line for the setup and one per (direction, layout) with the kernel family, its configuration,
 * the launch rule (dispatch order / static stride / in-order loop and the bound below which a launch runs in dispatch order) and,
 * beyond LDS, the sweeps over HBM (tile lengths, which pass reads / stores the internal layout).  Decided once, at pffft_new_setup
 * (reference: the ifac[] / twiddle plan of struct PFFFT_Setup, src/pffft_priv_impl.h:1051-1060, is fixed at setup time too).  Writes at
 * most len - 1 characters + a terminating 0 into buf and returns the length of the whole text (snprintf convention), -1 for an
 * invalid handle.  Works for PFFFT_Setup and PFFFTD_Setup handles; no device needed.  When the calling thread has set a selector
 * (pffft_hip_set_variant, tests), the lines show the routes the transforms run under that selector instead of the stored ones. */
int pffft_hip_describe(const void *setup, char *buf, size_t len);
/* The devices a setup holds tables / counters / scratch on right now: the device it was first used on, then one entry per further
 * device (HIP device indices; values >= 64 belong to the test hook pffft_hip_set_variant(130)).  Fills devices[0 .. max) and returns the
 * count (which may exceed max); 0 for a setup no transform has run on, or an invalid handle.  PFFFT_Setup and PFFFTD_Setup handles. */
int pffft_hip_setup_devices(const void *setup, int *devices, int max);
/* Resident workgroups per CU of the kernel a (direction, layout) of an LDS-resident setup runs on, as the launcher sizes its grid (the
 * runtime's occupancy query for the route's kernel, workgroup size and LDS bytes); 0 for routes without one persistent kernel (beyond
 * LDS, the minimum sizes), -1 on error.  Needs a device.  For tests and tools. */
int pffft_hip_route_occupancy(const void *setup, int direction, int ordered);
/* The tile plan of a complex core transform of n points beyond LDS (n = N for complex setups, N / 2 for real ones): returns the
 * number of tile passes over HBM — 2 or 3 — and their tile lengths in `lengths` (column pass(es) first, the row pass last), or 0
 * when the size runs on the streaming passes (or is LDS-resident: the planner is not consulted then).  `deep` = 1: the size's
 * streaming route would take five sweeps (its row length is itself beyond LDS), which admits costlier tile plans; 0: it takes three
 * and n is a complex transform; 2: it takes three and n is the core of a real transform of 2n points (the plans of 0 minus those
 * that pay only for complex transforms).  Pure host arithmetic, no device needed: for tests and for callers that want to know what
 * a size costs. */
int pffft_hip_tile_plan(long long n, int is_double, int deep, int lengths[3]);
/* The planner's tuning interface (tools/tune_tile_plans.py writes pffft_amd/csrc/tile_plan_gen.h with it).  pffft_hip_tile_candidates: every
 * legal pair of tile lengths of n, out[5 i ..] = {L1, gen1, L2, gen2, cost of the model}, returns the count (may exceed max).
 * pffft_hip_tile_override: from now on setups of n are planned with this pair (l1 > 0; -1 when it is not a legal pair), with no tile plan
 * (l1 == 0: the streaming passes) or by the tables again (l1 < 0).  Process-wide.  Call it while NO setup of n exists and destroy the setups
 * of n before changing it again: a setup's route is fixed at pffft_new_setup for the lengths of that moment, the passes read the lengths
 * per launch. */
int pffft_hip_tile_candidates(long long n, int is_double, int *out, int max);
int pffft_hip_tile_override(long long n, int is_double, int l1, int g1, int l2, int g2);
const char *pffft_hip_last_error(void);
/* Number of legacy (void) entries that failed in this process so far.  The legacy entries have no error channel
 * (include/pffft/pffft.h:159); a failed call — no device, HIP error — prints one line on stderr, fills its output
 * vector with NaN (all-ones bytes) and increments this counter.  PFFFT_HIP_ABORT=1 makes it abort() instead. */
unsigned pffft_hip_error_count(void);
int pffft_hip_device_count(void);
/* 0 = the planner's routes; the other values (enum AbValue, pffft_amd/csrc/pf_route.h) select an ALTERNATIVE ROUTE to the same
 * result - the streaming passes instead of the tile passes beyond LDS, the composed convolution instead of the fused kernel ... -
 * which the parity tests hold to the same bar as the default one; a development build (-DPFFFT_HIP_VARIANTS) knows a few more.  A
 * value the build does not know runs the default route.  The selector is THREAD-LOCAL: it affects only calls made by the thread
 * that set it. */
void pffft_hip_set_variant(int variant);
/* 1 when the library was built with -DPFFFT_HIP_VARIANTS (development build: both variants of every Stockham plan are
 * instantiated for A/B measurements), 0 for the product build (the adopted variant only; a selector that asks for the
 * other one gets the same arithmetic from the kernel that exists). */
int pffft_hip_has_variants(void);

#ifdef __cplusplus
}
#endif
#endif /* PFFFT_HIP_H */
