/* pfdsp_cic_hip.h — C ABI of libpfdsp_cic_hip.so: the PFDSP carrier generators and CIC decimating
 * down-converter on MI355X (gfx950), the companion of libpfdsp_hip.so (the mixers, include/pfdsp_hip.h).
 *
 * PART 1 declares, with identical names and argument meaning, the reference's carrier generators
 * (include/pffft/pf_carrier.h:72-85, src/pf_carrier.cpp) and CIC down-converter (include/pffft/pf_cic.h,
 * src/pf_cic.cpp).  A program written against the reference's PFDSP library (-lpfdsp) links against
 * -lpfdsp_hip -lpfdsp_cic_hip unchanged.  Unlike the mixers, these outputs ARE bit-identical to the
 * reference's.  PART 2 is the additive device / stream entry for a bank of channels.
 * With both headers in one translation unit, include pfdsp_hip.h first: it defines complexf.
 */
#ifndef PFDSP_CIC_HIP_H
#define PFDSP_CIC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ PART 1: reference ABI ---- */

#if !defined(PFDSP_HIP_NO_COMPLEXF) && !defined(PFDSP_HIP_H)
typedef struct complexf_s { float i; float q; } complexf;      /* include/pffft/pf_cplx.h:44 */
#endif

/* ---- carriers (include/pffft/pf_carrier.h:72-85, src/pf_carrier.cpp) ----
 * Each writes a fixed pattern of four complex samples, repeated: amplitude 127.0f/128 (float) or SHRT_MAX,
 * SHRT_MAX/2 (int16) -- the values the reference's code writes, not its comments.  `size` is in complex
 * samples.  DEVIATION: every entry writes exactly `size` samples, and a size that is not a multiple of 4
 * truncates the pattern (the reference asserts size % 4 == 0 for the fs/4 and fs/2 variants, and without
 * NDEBUG writes past the end otherwise).  Host pointers are written on the host; device / managed pointers by
 * a fill kernel on the null stream, returning after it finished. */
void generate_dc_f(float *output, int size);
void generate_dc_s16(short *output, int size);
void generate_pos_fs4_f(float *output, int size);
void generate_pos_fs4_s16(short *output, int size);
void generate_neg_fs4_f(float *output, int size);
void generate_neg_fs4_s16(short *output, int size);
void generate_dc_pos_fs4_s16(short *output, int size);
void generate_dc_neg_fs4_s16(short *output, int size);
void generate_pos_neg_fs4_s16(short *output, int size);
void generate_dc_pos_neg_fs4_s16(short *output, int size);
void generate_pos_neg_fs2_s16(short *output, int size);
void generate_dc_pos_neg_fs2_s16(short *output, int size);

/* ---- CIC decimating down-converter (include/pffft/pf_cic.h, src/pf_cic.cpp) ----
 * One call mixes outsize*factor input samples with the reference's int16 cosine table (phase += freq per
 * sample, freq = (uint64)(rate * 2^64) formed in float), runs them through three int64 integrators and two
 * combs, and writes outsize outputs (float)out * gain, gain = 1/SHRT_MAX/32767/factor^3.  Outputs and the
 * chained state are BIT-IDENTICAL to the reference's: the GPU regroups the int64 recurrence exactly (block
 * moments).  s16: real int16 input; cs16: interleaved int16 I/Q; cu8: interleaved uint8 I/Q
 * (offset 127.4).
 * rate outside [-0.5, 1): the reference's float-to-uint64 conversion is undefined in C; reproduced is what its
 * x86-64 object does: rate in [-0.5, 1] -> (rate*2^64) mod 2^64, rate below -0.5 -> 2^63, above 1 -> 0.
 * The state is opaque.  cicddc_init / cicddc_free are pure host code and work without a GPU; the first call
 * binds the state (integrators, combs, phase, table in device memory) to the calling thread's current device,
 * and a call on another device fails.  Pointer rule and failures as for the mixers (include/pfdsp_hip.h): host
 * pointers staged, device / managed pointers used in place, null stream, return after synchronising; a
 * failing call leaves NaN in the output and the state unchanged and counts in pfdsp_hip_cic_error_count().
 * DEVIATION: factor < 1 (the reference divides by zero) -> cicddc_init returns NULL, and every entry ignores
 * a NULL state. */
void *cicddc_init(int factor);
void cicddc_free(void *state);
void cicddc_s16_c(void *state, int16_t *input, complexf *output, int outsize, float rate);
void cicddc_cs16_c(void *state, int16_t *input, complexf *output, int outsize, float rate);
void cicddc_cu8_c(void *state, uint8_t *input, complexf *output, int outsize, float rate);

/* ------------------------------------------------- PART 2: device / stream extension --------- */
/* CIC bank: nch states (same factor, distinct), one rate per channel for this call, one DEVICE input of
 * outsize*factor samples in `format`; channel c writes outsize outputs at d_output + c*out_stride (complexf
 * units, out_stride >= outsize).  The input is read from memory once per 64 channels.  Asynchronous on `stream`; calls on
 * one state are ordered by the stream, and each call advances every state (a replayed graph too).  No
 * allocation and no host synchronisation, except at the first call of a state, which binds it: make that call
 * (outsize 0 binds and returns) before a stream capture.  64-bit sample indices: outsize*factor may exceed 2^31.
 * Returns 0 or a hipError_t value (pfdsp_hip_cic_last_error() has the text); invalid arguments (NULL /
 * duplicate states, mixed factors, unknown format, out_stride < outsize) return an error and write nothing. */
enum { PFDSP_HIP_CIC_S16 = 0, PFDSP_HIP_CIC_CS16 = 1, PFDSP_HIP_CIC_CU8 = 2 };
int pfdsp_hip_cicddc_device(void *const *states, const float *rates, int nch, int format,
                            const void *d_input, size_t outsize, complexf *d_output,
                            size_t out_stride, void *stream);
const char *pfdsp_hip_cic_last_error(void);
/* number of legacy entries of this library that failed soft (no device / HIP error: stderr line, NaN-filled output) */
unsigned pfdsp_hip_cic_error_count(void);

#ifdef __cplusplus
}
#endif
#endif /* PFDSP_CIC_HIP_H */
