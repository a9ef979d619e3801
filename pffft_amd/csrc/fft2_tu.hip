// libpffft_hip.so, translation unit of the 2-D transforms (include/pffft_hip.h: pffft[d]_hip_fft2_*): batched complex transforms of dense
// rows x cols images, natural order in and out.  The handle owns one inner complex setup per distinct length and no tables; the fused
// kernel's launch (one kernel per call, float, lengths 16 / 32 / 64) and the composed route (ordered transform_batch over the rows, a
// transposing kernel into a chunked scratch image, transform_batch over the columns, the transposing kernel back, times the scaling).
// Kernels: fft_fft2.h.
#include <memory>

#include "pf_compose.h"
#include "fft_fft2.h"

namespace pf {

constexpr uint32_t FFT2_MAGIC = 0x50463244u;   // "PF2D"

// The owned inner setups: `inner` transforms the rows (length cols), `inner_rows` the columns (length rows); rows == cols shares one.
// One setup serves ONE device (bind_device_once).
struct Fft2Setup : InnerOwner<FFT2_MAGIC> {
    static constexpr const char* KIND = "fft2";
    int rows = 0, cols = 0;
    bool fusable = false;          // float and both lengths out of 16 / 32 / 64
    Setup* inner_rows = nullptr;
    bool own_rows = false;
    DeviceBinding bound;
    StreamScratch pad;             // the composed route's image: one per stream, pad.mu held while a call enqueues
    ~Fft2Setup() {
        if (own_rows && inner_rows) {
            if (is_double) pffftd_destroy_setup(static_cast<PFFFTD_Setup*>(inner_rows));
            else pffft_destroy_setup(static_cast<PFFFT_Setup*>(inner_rows));
        }
    }
};

// ------------------------------------------------------------------------------------------------ plan
// Whether the next group's chunks are requested before the column pass (1) or behind the store (0) - arithmetic on the resource remarks of
// every instantiation (tools/fft2_resources.py; the table of DESIGN.md §3.26), not a measurement: 1 where it keeps the waves per SIMD the
// LDS images allow anyway and has no scratch.
template <int R, int C> constexpr int fft2_pf() { return 1; }

// Shapes where the fused kernel is the default: a shape is in it where tests/test_gpu_fft2.py test_default_cells holds the fused kernel
// faster than selector 148 on the device by more than the spread of identical rounds.  A shape that loses returns false
// here and stays reachable through AB_FFT2_FUSED.  Measured on an MI355X at 64 MiB of images: fused wins all nine shapes, 3.4 x (32 x 64)
// to 5.7 x (16 x 16), against a spread of the composed rounds of at most 1.02.
static bool fft2_fused_default(int rows, int cols) {
    (void)rows; (void)cols;
    return true;
}

static bool fft2_fused_now(const Fft2Setup* z, const AbSel& sel) {
    if (!z->fusable || sel.is(AB_FFT2_COMPOSED)) return false;
    return sel.is(AB_FFT2_FUSED) || fft2_fused_default(z->rows, z->cols);
}

static Fft2Setup* fft2_new_setup(int rows, int cols, int is_double) {
    if (rows < 1 || cols < 1) return nullptr;
    std::unique_ptr<Fft2Setup> z(new Fft2Setup);
    z->rows = rows; z->cols = cols;
    z->fusable = !is_double && fft2_fused_len(rows) && fft2_fused_len(cols);
    if (!z->new_inner(cols, PFFFT_COMPLEX, is_double)) return nullptr;
    if (rows == cols) {
        z->inner_rows = z->inner;
    } else {
        z->inner_rows = is_double ? static_cast<Setup*>(pffftd_new_setup(rows, PFFFT_COMPLEX)) : static_cast<Setup*>(pffft_new_setup(rows, PFFFT_COMPLEX));
        if (!z->inner_rows) return nullptr;
        z->own_rows = true;
    }
    return z.release();
}

// ------------------------------------------------------------------------------------------------ the routes
template <int R, int C, int DIR>
static int fft2_fused_launch(Setup* s, const cx<float>* tw64, const float* in, float* out, size_t batch, float scaling, hipStream_t st) {
    typedef Fft2Cfg<R, C> Cf;
    auto k = fft_fft2_kernel<R, C, DIR, fft2_pf<R, C>()>;
    LoopLaunch ll;
    if (int rc = loop_launch(s, st, k, Cf::WG, Cf::LDS_BYTES, (batch + Cf::SLOTS - 1) / Cf::SLOTS, CONV_ONESHOT, &ll)) return rc;
    hipLaunchKernelGGL(k, dim3(ll.grid), dim3(Cf::WG), Cf::LDS_BYTES, st, in, out, (unsigned)batch, scaling, tw64, ll.ctr);
    PF_CHECK(hipGetLastError());
    return 0;
}

// the inner setup with its tables on the calling thread's device
static int fft2_inner_ready(Setup* inner) {
    if (for_device(inner) != inner) {
        g_last_error = "pffft_hip: this setup holds its tables on another device";
        return (int)hipErrorInvalidDevice;
    }
    return ensure_device_any(inner);
}

// The counters come from the rows' inner setup; the W_64 values from the table W_64^j of whichever inner setup has length 64.  The batch
// goes out in slices on the same stream (for_slices): the kernel counts images in 32 bits.
static int fft2_fused(Fft2Setup* z, const float* in, float* out, size_t batch, int dir, float scaling, hipStream_t st) {
    if (int rc = fft2_inner_ready(z->inner)) return rc;
    if (z->own_rows)
        if (int rc = fft2_inner_ready(z->inner_rows)) return rc;
    Setup* s64 = z->cols == 64 ? z->inner : z->rows == 64 ? z->inner_rows : nullptr;
    const cx<float>* tw64 = s64 ? s64->d_tw.as<cx<float>>() : nullptr;
    const size_t image = (size_t)z->rows * z->cols * 2;
    return for_slices(batch, [&](size_t b0, size_t nb) {
        const float* pi = in + b0 * image;
        float* po = out + b0 * image;
        return with_one_of<16, 32, 64>(z->rows, [&](auto R) {
            return with_one_of<16, 32, 64>(z->cols, [&](auto C) {
                return with_flag(dir == PFFFT_BACKWARD, [&](auto D) {
                    return fft2_fused_launch<decltype(R)::value, decltype(C)::value, decltype(D)::value>(z->inner, tw64, pi, po, nb, scaling, st);
                });
            });
        });
    });
}

template <typename T>
static int fft2_transform(Setup* inner, const T* in, T* out, size_t lines, int dir, hipStream_t st) {
    if constexpr (sizeof(T) == 8)
        return pffftd_hip_transform_batch(static_cast<PFFFTD_Setup*>(inner), in, out, lines, (pffft_direction_t)dir, 1, st);
    else
        return pffft_hip_transform_batch(static_cast<PFFFT_Setup*>(inner), in, out, lines, (pffft_direction_t)dir, 1, st);
}

template <typename T, int SCALE>
static int fft2_transpose(const cx<T>* src, cx<T>* dst, size_t images, size_t rows, size_t cols, T s, hipStream_t st) {
    const size_t tiles = images * ((rows + 31) / 32) * ((cols + 31) / 32);
    const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>(tiles, (size_t)num_cus() * 32));
    hipLaunchKernelGGL((fft2_transpose_kernel<T, SCALE>), dim3(grid), dim3(256), 0, st, src, dst, images, (unsigned)rows, (unsigned)cols, s);
    PF_CHECK(hipGetLastError());
    return 0;
}

// One image of the scratch per image of a chunk; `in` is read by the first transform only and written only where it is `out`
template <typename T>
static int fft2_composed(Fft2Setup* z, const T* in, T* out, size_t batch, int dir, T s, hipStream_t st) {
    const size_t R = (size_t)z->rows, C = (size_t)z->cols, plane = R * C;
    return chunked_scratch<cx<T>>(z->pad, st, batch, plane * sizeof(cx<T>), "the scratch image", [&](cx<T>* X, size_t v0, size_t cnt) {
        const T* src = in + v0 * plane * 2;
        T* dst = out + v0 * plane * 2;
        if (int rc = fft2_transform<T>(z->inner, src, dst, cnt * R, dir, st)) return rc;
        if (int rc = fft2_transpose<T, 0>(reinterpret_cast<const cx<T>*>(dst), X, cnt, R, C, (T)1, st)) return rc;
        if (int rc = fft2_transform<T>(z->inner_rows, (const T*)X, (T*)X, cnt * C, dir, st)) return rc;
        return fft2_transpose<T, 1>(X, reinterpret_cast<cx<T>*>(dst), cnt, C, R, s, st);
    });
}

// ------------------------------------------------------------------------------------------------ the entry
template <typename T>
static int fft2_batch(void* setup, const T* in, T* out, size_t batch, int dir, T scaling, hipStream_t st) {
    Fft2Setup* z = typed_handle<Fft2Setup, T>(setup);
    if (!z) return (int)hipErrorInvalidHandle;
    if (dir != PFFFT_FORWARD && dir != PFFFT_BACKWARD) return bad("fft2: unknown direction");
    if (batch == 0) return 0;
    if (!in || !out) return bad("fft2: NULL in / out");
    if (!aligned16(in) || !aligned16(out)) return bad("fft2: in / out not aligned to 16 bytes");
    if (in != out) {
        const size_t bytes = batch * (size_t)z->rows * (size_t)z->cols * 2 * sizeof(T);
        const uintptr_t i0 = (uintptr_t)in, o0 = (uintptr_t)out;
        if (i0 < o0 + bytes && o0 < i0 + bytes) return bad("fft2: out overlaps in (in == out, in place, is the one legal overlap)");
    }
    if (int rc = bind_device_once(z->bound, "fft2: ", st, [] { return 0; })) return rc;   // (no tables: nothing is built beyond the binding)
    if constexpr (sizeof(T) == 4) {
        if (fft2_fused_now(z, ab())) return fft2_fused(z, in, out, batch, dir, scaling, st);
    }
    return fft2_composed<T>(z, in, out, batch, dir, scaling, st);
}

}  // namespace pf

PF_EXPORT PFFFT_HIP_Fft2Setup* pffft_hip_fft2_new_setup(int rows, int cols) {
    return reinterpret_cast<PFFFT_HIP_Fft2Setup*>(pf::fft2_new_setup(rows, cols, 0));
}
PF_EXPORT PFFFTD_HIP_Fft2Setup* pffftd_hip_fft2_new_setup(int rows, int cols) {
    return reinterpret_cast<PFFFTD_HIP_Fft2Setup*>(pf::fft2_new_setup(rows, cols, 1));
}
PF_EXPORT void pffft_hip_fft2_destroy_setup(PFFFT_HIP_Fft2Setup* s) { pf::destroy_handle<pf::Fft2Setup>(s); }
PF_EXPORT void pffftd_hip_fft2_destroy_setup(PFFFTD_HIP_Fft2Setup* s) { pf::destroy_handle<pf::Fft2Setup>(s); }
PF_EXPORT int pffft_hip_fft2_transform_batch(PFFFT_HIP_Fft2Setup* s, const float* in, float* out, size_t batch, pffft_direction_t direction,
                                             float scaling, void* stream) {
    return pf::fft2_batch<float>(s, in, out, batch, (int)direction, scaling, (hipStream_t)stream);
}
PF_EXPORT int pffftd_hip_fft2_transform_batch(PFFFTD_HIP_Fft2Setup* s, const double* in, double* out, size_t batch, pffft_direction_t direction,
                                              double scaling, void* stream) {
    return pf::fft2_batch<double>(s, in, out, batch, (int)direction, scaling, (hipStream_t)stream);
}
PF_EXPORT const char* pffft_hip_fft2_route(const void* setup) {
    const pf::Fft2Setup* z = pf::checked_handle<pf::Fft2Setup>(setup);
    if (!z) return "";
    return pf::fft2_fused_now(z, pf::ab()) ? "fused" : "composed";
}
