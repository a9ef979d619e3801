// Host code shared by the translation units of the 2-D transforms (fft2_tu.hip, rfft2_tu.hip): what both entries check first, the device
// binding of a handle without tables, the tile grid and launch of the transposing kernels, and the fused launch in slices.  Each unit
// keeps its handle, its shape rule and *_pf table, its overlap rule and text, its composed sequence and its exports.  The handle base, the
// inner setups' device test and typed entries, the slices and the chunked scratch are pf_compose.h's.
#pragma once
#include "pf_compose.h"
#include "fft_fft2.h"

namespace pf {

// What both entries check alike after the handle, in their order; `prefix` ("fft2: ") opens every text.  ARGS_EMPTY for a call without
// images (the entry returns 0).
inline int fft2d_args(const char* prefix, const void* in, const void* out, size_t batch, int dir) {
    if (dir != PFFFT_FORWARD && dir != PFFFT_BACKWARD) return bad_in(prefix, "unknown direction");
    if (batch == 0) return ARGS_EMPTY;
    if (!in || !out) return bad_in(prefix, "NULL in / out");
    if (!aligned16(in) || !aligned16(out)) return bad_in(prefix, "in / out not aligned to 16 bytes");
    return 0;
}

// One setup serves ONE device; the handles have no tables, so nothing is built beyond the binding
inline int fft2d_bind(DeviceBinding& b, const char* prefix, hipStream_t st) {
    return bind_device_once(b, prefix, st, [] { return 0; });
}

// A kernel of 256 threads that walks the 32 x 32 tiles of `images` a x b planes with a grid stride
static unsigned fft2d_tile_grid(size_t images, size_t a, size_t b) {
    const size_t tiles = images * ((a + 31) / 32) * ((b + 31) / 32);
    return (unsigned)std::max<size_t>(1, std::min<size_t>(tiles, (size_t)num_cus() * 32));
}
template <typename K, typename... Args>
static int fft2d_tile_launch(K kernel, size_t images, size_t a, size_t b, hipStream_t st, const Args&... args) {
    hipLaunchKernelGGL(kernel, dim3(fft2d_tile_grid(images, a, b)), dim3(256), 0, st, args...);
    PF_CHECK(hipGetLastError());
    return 0;
}
// [a][b] -> [b][a] per image, times s where SCALE
template <typename T, int SCALE>
static int fft2d_transpose(const cx<T>* src, cx<T>* dst, size_t images, size_t a, size_t b, T s, hipStream_t st) {
    return fft2d_tile_launch(fft2_transpose_kernel<T, SCALE>, images, a, b, st, src, dst, images, (unsigned)a, (unsigned)b, s);
}

// The fused route: the batch goes out in slices on the same stream (the kernels count images in 32 bits); launch(in, out, images) picks
// the instantiation of a slice and hands it to fft2d_fused_launch, which runs it on the configuration Cf (WG threads, LDS_BYTES, SLOTS
// images per workgroup) under the launch rule of the convolution kernel.  `s` gives the counters, tw64 is W_64^j or NULL.
template <class Launch>
static int fft2d_fused(const float* in, size_t in_image, float* out, size_t out_image, size_t batch, Launch&& launch) {
    return for_slices(batch, [&](size_t b0, size_t nb) { return launch(in + b0 * in_image, out + b0 * out_image, nb); });
}
template <class Cf, typename K>
static int fft2d_fused_launch(Setup* s, K kernel, const cx<float>* tw64, const float* in, float* out, size_t batch, float scaling, hipStream_t st) {
    return loop_launch_last(s, st, kernel, Cf::WG, Cf::LDS_BYTES, (batch + Cf::SLOTS - 1) / Cf::SLOTS, CONV_ONESHOT, in, out, (unsigned)batch, scaling, tw64);
}
// ... its sibling for the spectral convolution kernel (fft_fft2c.h), which also takes the spectrum H and conj_h
template <class Cf, typename K>
static int fft2d_fused_conv_launch(Setup* s, K kernel, const cx<float>* tw64, const float* in, const cx<float>* H, float* out, size_t batch,
                                   float scaling, int conj_h, hipStream_t st) {
    return loop_launch_last(s, st, kernel, Cf::WG, Cf::LDS_BYTES, (batch + Cf::SLOTS - 1) / Cf::SLOTS, CONV_ONESHOT, in, H, out, (unsigned)batch, scaling,
                            conj_h, tw64);
}

// The product kernel of the composed convolutions (fft_fft2c.h fft2conv_product_kernel): X[i] = X[i] . G[i mod himage] in place on `st`.
// Defined and instantiated for float and double in fft2_tu.hip, so that the library holds the kernel once; rfft2_tu.hip calls it too.
template <typename T>
int fft2conv_product(cx<T>* X, const cx<T>* H, size_t total, size_t himage, int conj_h, hipStream_t st);

}  // namespace pf
