// pffastconv kernels that are no block kernel of fft_fir.h: the gather / scatter pair of the composed path and the time-domain kernel of
// short filters.  Included by fastconv_tu.hip only: the gather / scatter kernels are plain (non-template) symbols of that unit.
#pragma once
#include <cstdint>
#include "cxmath.h"

namespace pf {

// mode 0: real stream (also the single-FFT complex mode, which is a real stream of 2x length)
// mode 1: interleaved complex input processed as two real streams (part = block & 1)
__global__ void fastconv_gather_kernel(const float* __restrict__ x, float* __restrict__ blocks, int nblk, int Nfft,
                                       int step, int inputLen, int mode) {
    const size_t total = (size_t)nblk * Nfft;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        int b = (int)(i / Nfft), j = (int)(i - (size_t)b * Nfft);
        float v = 0.f;
        if (mode == 0) {
            long src = (long)b * step + j;
            if (src < inputLen) v = x[src];
        } else {
            int part = b & 1;
            long src = (long)(b >> 1) * step + j;
            if (src < inputLen) v = x[2 * src + part];
        }
        blocks[i] = v;
    }
}

__global__ void fastconv_scatter_kernel(const float* __restrict__ blocks, float* __restrict__ y, int nblk, int Nfft,
                                        int step, int lastOut, int mode) {
    const int nb_time = mode == 0 ? nblk : nblk >> 1;
    const size_t total = (size_t)nblk * step;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        int b = (int)(i / step), j = (int)(i - (size_t)b * step);
        int tb = mode == 0 ? b : (b >> 1);
        int numOut = (tb == nb_time - 1) ? lastOut : step;
        if (j >= numOut) continue;
        float v = blocks[(size_t)b * Nfft + j];
        if (mode == 0) y[(size_t)tb * step + j] = v;
        else y[2 * ((size_t)tb * step + j) + (b & 1)] = v;
    }
}

// ---- short filters: time domain ------------------------------------------------------------------------------------
// The reference always goes through Nfft = max(32, 2 next_pow2(len - 1)) transforms.  For <= TD_MAX_TAPS taps that is two
// transforms per (Nfft - len + 1) outputs of a kernel family that is latency-bound at these sizes (64 taps: 36
// Gsamples/s, 512 taps: 77; this kernel: 378 and 84 - the crossover is near 550 taps); the same outputs  y[m] = sum_i c_i x[m + i]  (the circular product of :99-108 and :238-255 written
// out: c_i = filter[len-1-i], or filter[i] with PFFASTCONV_CORRELATION) cost len FMAs each.  A workgroup stages
// 2048 + len inputs in LDS, a thread owns 8 consecutive outputs and slides a 16-value register window over them, 8 taps
// per step (two 16-byte LDS reads for 64 FMAs), the taps come through scalar loads.  The block schedule the caller can
// observe (how many samples a call produces, src/pffastconv.c:156-166,204-210) is computed as before.
constexpr int TD_THREADS = 256, TD_PER = 8, TD_TILE = TD_THREADS * TD_PER, TD_MAX_TAPS = 512;

// STRIDE 2: interleaved complex samples filtered by a real filter = the same sum over every second float,
// y[f] = sum_i c_i x[f + 2 i] — both complex modes of the reference (two real transforms per block, or one transform with
// the zero-stuffed filter, src/pffastconv.c:84-106) are this on the float stream; they differ in the block schedule only.
template <int STRIDE>
__global__ void __launch_bounds__(TD_THREADS)
fastconv_td_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ c, int flen8, long produced,
                   long inputLen, size_t xstride, size_t ystride) {
    extern __shared__ __attribute__((aligned(16))) float sx[];
    x += (size_t)blockIdx.y * xstride;   // blockIdx.y = signal of a batch (pffastconv_hip_apply_batch)
    y += (size_t)blockIdx.y * ystride;
    const int tid = threadIdx.x;
    const long o0 = (long)blockIdx.x * TD_TILE;
    const int outs = (produced - o0) < TD_TILE ? (int)(produced - o0) : TD_TILE;
    const int need = outs + STRIDE * (flen8 - 1);      // produced + STRIDE (len - 1) <= inputLen (fc_schedule); the zero taps of
    for (int i = tid; i < TD_TILE + STRIDE * flen8 + 8; i += TD_THREADS)   // the padding may point past the input: guarded
        sx[i] = (i < need && o0 + i < inputLen) ? x[o0 + i] : 0.f;
    __syncthreads();
    const float* w = sx + tid * TD_PER;
    float acc[TD_PER];
#pragma unroll
    for (int k = 0; k < TD_PER; ++k) acc[k] = 0.f;
    vec4<float> lo0 = *reinterpret_cast<const vec4<float>*>(w), lo1 = *reinterpret_cast<const vec4<float>*>(w + 4);
    constexpr int TAPS_PER_STEP = 8 / STRIDE;          // the window advances 8 floats per step
    for (int j = 0, wo = 8; j < flen8; j += TAPS_PER_STEP, wo += 8) {
        const vec4<float> hi0 = *reinterpret_cast<const vec4<float>*>(w + wo);
        const vec4<float> hi1 = *reinterpret_cast<const vec4<float>*>(w + wo + 4);
        const float win[16] = {lo0.x, lo0.y, lo0.z, lo0.w, lo1.x, lo1.y, lo1.z, lo1.w,
                               hi0.x, hi0.y, hi0.z, hi0.w, hi1.x, hi1.y, hi1.z, hi1.w};
#pragma unroll
        for (int jj = 0; jj < TAPS_PER_STEP; ++jj) {
            const float cj = c[j + jj];                // wave-uniform: scalar load
#pragma unroll
            for (int k = 0; k < TD_PER; ++k) acc[k] = __builtin_fmaf(cj, win[STRIDE * jj + k], acc[k]);
        }
        lo0 = hi0; lo1 = hi1;
    }
    const int m0 = tid * TD_PER;
    float* dst = y + o0 + m0;
    if (m0 + TD_PER <= outs && (((uintptr_t)dst) & 15) == 0) {
        vec4<float> a, b;
        a.x = acc[0]; a.y = acc[1]; a.z = acc[2]; a.w = acc[3]; b.x = acc[4]; b.y = acc[5]; b.z = acc[6]; b.w = acc[7];
        *reinterpret_cast<vec4<float>*>(dst) = a;
        *reinterpret_cast<vec4<float>*>(dst + 4) = b;
    } else {
#pragma unroll
        for (int k = 0; k < TD_PER; ++k) if (m0 + k < outs) dst[k] = acc[k];
    }
}

}  // namespace pf
