// Host pieces shared by the translation units that go through the per-stream frame matrix (pf::Setup::frames): frames_tu.hip (the frame
// entries) and pfb_tu.hip (filter-bank analysis and synthesis).  Every function is internal to the unit that includes it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/pffft_hip.h"
#include "pf_launch.h"
#include "fft_frames.h"

namespace pf {

// The frame matrix of one composed launch sequence holds at most this many bytes (include/pffft_hip.h): longer batches go through it in
// chunks on the stream.
constexpr size_t FRAMES_CAP_BYTES = (size_t)256 << 20;

static unsigned stream_grid(size_t items) {
    return (unsigned)std::max<size_t>(1, std::min<size_t>((items + 255) / 256, (size_t)num_cus() * 16));
}

// the frame matrix of `st` (frames.mu held by the caller), grown to `bytes`: outside graph capture only
static int frames_buffer(Setup* s, hipStream_t st, size_t bytes, void** buf) {
    return scratch_buffer(s->frames, st, bytes, "the frame matrix", buf);
}

template <typename T, int MODE>
static int launch_rows(const T* src, size_t src_stride, T* dst, size_t dst_stride, size_t count, size_t row, hipStream_t st) {
    const size_t per = MODE == 0 ? row : MODE == 1 ? row / 2 + 1 : row / 2;
    hipLaunchKernelGGL((frames_rows_kernel<T, MODE>), dim3(stream_grid(count * per)), dim3(256), 0, st, src, src_stride, dst, dst_stride,
                       count, (unsigned)row);
    PF_CHECK(hipGetLastError());
    return 0;
}

// spectra rows r0 ... r0 + cnt - 1 -> backward-transformed dense rows in X
template <typename T>
static int frames_backward(Setup* s, const T* spectra, size_t spectra_stride, size_t r0, size_t cnt, T* X, int ordered, hipStream_t st) {
    const size_t row = s->vec_scalars;
    const T* src = spectra + r0 * spectra_stride;
    if (spectra_stride != row) {
        int rc = launch_rows<T, 0>(src, spectra_stride, X, row, cnt, row, st);
        if (rc) return rc;
        src = X;
    }
    return transform_batch_any(s, src, X, cnt, PFFFT_BACKWARD, ordered ? 1 : 0, st);
}

}  // namespace pf
