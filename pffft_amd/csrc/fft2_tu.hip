// libpffft_hip.so, translation unit of the 2-D transforms (include/pffft_hip.h: pffft[d]_hip_fft2_*): batched complex transforms of dense
// rows x cols images, natural order in and out.  The handle owns one inner complex setup per distinct length and no tables; the fused
// kernel's launch (one kernel per call, float, lengths 16 / 32 / 64) and the composed route (ordered transform_batch over the rows, a
// transposing kernel into a chunked scratch image, transform_batch over the columns, the transposing kernel back, times the scaling).
// Kernels: fft_fft2.h.  On the same handle the spectral convolution out = s IFFT2u(FFT2(in) . G) (pffft[d]_hip_fft2_convolve_batch): its
// fused kernel's launch and the composed route on the handle's own transforms around a product kernel.  Kernels: fft_fft2c.h.
#include <memory>

#include "fft2d_host.h"
#include "fft_fft2c.h"

namespace pf {

constexpr uint32_t FFT2_MAGIC = 0x50463244u;   // "PF2D"

// The owned inner setups: `inner` transforms the rows (length cols), `inner_rows` the columns (length rows); rows == cols shares one.
// One setup serves ONE device (bind_device_once).
struct Fft2Setup : InnerOwner<FFT2_MAGIC> {
    static constexpr const char* KIND = "fft2";
    int rows = 0, cols = 0;
    bool fusable = false;          // float and both lengths out of 16 / 32 / 64
    Setup* inner_rows = nullptr;
    DeviceBinding bound;
    StreamScratch pad;             // the composed route's image: one per stream, pad.mu held while a call enqueues
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
    return fused_selected(sel, AB_FFT2_COMPOSED, AB_FFT2_FUSED, z->fusable, fft2_fused_default(z->rows, z->cols));
}

static Fft2Setup* fft2_new_setup(int rows, int cols, int is_double) {
    if (rows < 1 || cols < 1) return nullptr;
    std::unique_ptr<Fft2Setup> z(new Fft2Setup);
    z->rows = rows; z->cols = cols;
    z->fusable = !is_double && fft2_fused_len(rows) && fft2_fused_len(cols);
    if (!z->new_inner(cols, PFFFT_COMPLEX, is_double)) return nullptr;
    if (!(z->inner_rows = rows == cols ? z->inner : z->add_inner(rows, PFFFT_COMPLEX))) return nullptr;
    return z.release();
}

// ------------------------------------------------------------------------------------------------ the routes
// The counters come from the rows' inner setup; the W_64 values from the table W_64^j of whichever inner setup has length 64.
static int fft2_fused(Fft2Setup* z, const float* in, float* out, size_t batch, int dir, float scaling, hipStream_t st) {
    if (int rc = inner_on_device(z->inner, st)) return rc;
    if (z->inner_rows != z->inner)
        if (int rc = inner_on_device(z->inner_rows, st)) return rc;
    Setup* s64 = z->cols == 64 ? z->inner : z->rows == 64 ? z->inner_rows : nullptr;
    const cx<float>* tw64 = s64 ? s64->d_tw.as<cx<float>>() : nullptr;
    const size_t image = (size_t)z->rows * z->cols * 2;
    return fft2d_fused(in, image, out, image, batch, [&](const float* pi, float* po, size_t nb) {
        return with_one_of<16, 32, 64>(z->rows, [&](auto R) {
            return with_one_of<16, 32, 64>(z->cols, [&](auto C) {
                return with_flag(dir == PFFFT_BACKWARD, [&](auto D) {
                    constexpr int r = decltype(R)::value, c = decltype(C)::value;
                    return fft2d_fused_launch<Fft2Cfg<r, c>>(z->inner, fft_fft2_kernel<r, c, decltype(D)::value, fft2_pf<r, c>()>, tw64, pi, po, nb,
                                                            scaling, st);
                });
            });
        });
    });
}

// One image of the scratch per image of a chunk; `in` is read by the first transform only and written only where it is `out`
template <typename T>
static int fft2_composed(Fft2Setup* z, const T* in, T* out, size_t batch, int dir, T s, hipStream_t st) {
    const size_t R = (size_t)z->rows, C = (size_t)z->cols, plane = R * C;
    return chunked_scratch<cx<T>>(z->pad, st, batch, plane * sizeof(cx<T>), "the scratch image", [&](cx<T>* X, size_t v0, size_t cnt) {
        const T* src = in + v0 * plane * 2;
        T* dst = out + v0 * plane * 2;
        if (int rc = inner_transform_batch<T>(z->inner, src, dst, cnt * R, dir, 1, st)) return rc;
        if (int rc = fft2d_transpose<T, 0>(reinterpret_cast<const cx<T>*>(dst), X, cnt, R, C, (T)1, st)) return rc;
        if (int rc = inner_transform_batch<T>(z->inner_rows, (const T*)X, (T*)X, cnt * C, dir, 1, st)) return rc;
        return fft2d_transpose<T, 1>(X, reinterpret_cast<cx<T>*>(dst), cnt, C, R, s, st);
    });
}

// ------------------------------------------------------------------------------------------------ the entry
// a validated call on a bound handle: the route of the calling thread's selector
template <typename T>
static int fft2_run(Fft2Setup* z, const T* in, T* out, size_t batch, int dir, T scaling, hipStream_t st) {
    if constexpr (sizeof(T) == 4) {
        if (fft2_fused_now(z, ab())) return fft2_fused(z, in, out, batch, dir, scaling, st);
    }
    return fft2_composed<T>(z, in, out, batch, dir, scaling, st);
}

template <typename T>
static int fft2_batch(void* setup, const T* in, T* out, size_t batch, int dir, T scaling, hipStream_t st) {
    Fft2Setup* z = typed_handle<Fft2Setup, T>(setup);
    if (!z) return (int)hipErrorInvalidHandle;
    if (int rc = fft2d_args("fft2: ", in, out, batch, dir)) return rc == ARGS_EMPTY ? 0 : rc;
    const size_t bytes = batch * (size_t)z->rows * (size_t)z->cols * 2 * sizeof(T);
    if (in != out && ranges_overlap((uintptr_t)in, bytes, (uintptr_t)out, bytes))
        return bad("fft2: out overlaps in (in == out, in place, is the one legal overlap)");
    if (int rc = fft2d_bind(z->bound, "fft2: ", st)) return rc;
    return fft2_run<T>(z, in, out, batch, dir, scaling, st);
}

// ------------------------------------------------------------------------------------------------ spectral convolution
// Shapes where the fused convolution kernel is the default for one broadcast H: a shape is in it where tests/test_gpu_fft2conv.py
// test_default_cells holds selector 153 faster than selector 152 on the device by more than the spread of identical rounds (DESIGN.md
// §3.29).  A shape that loses returns false here and stays reachable through AB_FFT2CONV_FUSED.
static bool fft2conv_fused_default(int rows, int cols) {
    (void)rows; (void)cols;
    return true;
}

// the fused kernel takes float images of the nine shapes and ONE spectrum; per-image H is always composed
static bool fft2conv_fused_now(const Fft2Setup* z, int h_broadcast, const AbSel& sel) {
    return fused_selected(sel, AB_FFT2CONV_COMPOSED, AB_FFT2CONV_FUSED, z->fusable && h_broadcast != 0, fft2conv_fused_default(z->rows, z->cols));
}

static int fft2conv_fused(Fft2Setup* z, const float* in, const float* H, float* out, float scaling, size_t batch, int conj_h, hipStream_t st) {
    if (int rc = inner_on_device(z->inner, st)) return rc;
    if (z->inner_rows != z->inner)
        if (int rc = inner_on_device(z->inner_rows, st)) return rc;
    Setup* s64 = z->cols == 64 ? z->inner : z->rows == 64 ? z->inner_rows : nullptr;
    const cx<float>* tw64 = s64 ? s64->d_tw.as<cx<float>>() : nullptr;
    const cx<float>* G = reinterpret_cast<const cx<float>*>(H);
    const size_t image = (size_t)z->rows * z->cols * 2;
    return fft2d_fused(in, image, out, image, batch, [&](const float* pi, float* po, size_t nb) {
        return with_one_of<16, 32, 64>(z->rows, [&](auto R) {
            return with_one_of<16, 32, 64>(z->cols, [&](auto C) {
                constexpr int r = decltype(R)::value, c = decltype(C)::value;
                typedef Fft2ConvForm<r, c> Form;
                return fft2d_fused_conv_launch<Fft2Cfg<r, c>>(z->inner, fft_fft2conv_kernel<r, c, Form::PF, Form::HREG>, tw64, pi, G, po, nb, scaling,
                                                             conj_h, st);
            });
        });
    });
}

template <typename T>
int fft2conv_product(cx<T>* X, const cx<T>* H, size_t total, size_t himage, int conj_h, hipStream_t st) {
    return stream_launch(fft2conv_product_kernel<T>, total, st, X, H, total, himage, conj_h);
}
template int fft2conv_product<float>(cx<float>*, const cx<float>*, size_t, size_t, int, hipStream_t);
template int fft2conv_product<double>(cx<double>*, const cx<double>*, size_t, size_t, int, hipStream_t);

// The handle's own forward transform from in into out, the product in place there, the handle's own backward transform in place with the
// scaling: the transforms take whichever route pffft_hip_fft2_route names under the calling thread's selector.  No scratch of its own.
template <typename T>
static int fft2conv_composed(Fft2Setup* z, const T* in, const T* H, T* out, T scaling, size_t batch, int conj_h, int h_broadcast, hipStream_t st) {
    const size_t plane = (size_t)z->rows * (size_t)z->cols, total = batch * plane;
    if (int rc = fft2_run<T>(z, in, out, batch, PFFFT_FORWARD, (T)1, st)) return rc;
    if (int rc = fft2conv_product<T>(reinterpret_cast<cx<T>*>(out), reinterpret_cast<const cx<T>*>(H), total, h_broadcast ? plane : total, conj_h, st))
        return rc;
    return fft2_run<T>(z, out, out, batch, PFFFT_BACKWARD, scaling, st);
}

template <typename T>
static int fft2conv_batch(void* setup, const T* in, const T* H, T* out, T scaling, size_t batch, int conj_h, int h_broadcast, hipStream_t st) {
    const char* pre = "fft2 convolve: ";
    Fft2Setup* z = typed_handle<Fft2Setup, T>(setup);
    if (!z) return (int)hipErrorInvalidHandle;
    if (batch == 0) return 0;
    if (!in || !H || !out) return bad_in(pre, "NULL in / H / out");
    if (!aligned16(in) || !aligned16(H) || !aligned16(out)) return bad_in(pre, "in / H / out not aligned to 16 bytes");
    const size_t image = (size_t)z->rows * (size_t)z->cols * 2 * sizeof(T), bytes = batch * image;
    if (in != out && ranges_overlap((uintptr_t)in, bytes, (uintptr_t)out, bytes))
        return bad_in(pre, "out overlaps in (in == out, in place, is the one legal overlap)");
    if (ranges_overlap((uintptr_t)H, h_broadcast ? image : bytes, (uintptr_t)out, bytes)) return bad_in(pre, "H overlaps out");
    if (int rc = fft2d_bind(z->bound, pre, st)) return rc;
    if constexpr (sizeof(T) == 4) {
        if (fft2conv_fused_now(z, h_broadcast, ab())) return fft2conv_fused(z, in, H, out, scaling, batch, conj_h != 0, st);
    }
    return fft2conv_composed<T>(z, in, H, out, scaling, batch, conj_h != 0, h_broadcast, st);
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
PF_EXPORT int pffft_hip_fft2_convolve_batch(PFFFT_HIP_Fft2Setup* s, const float* in, const float* H, float* out, float scaling, size_t batch,
                                            int conj_h, int h_broadcast, void* stream) {
    return pf::fft2conv_batch<float>(s, in, H, out, scaling, batch, conj_h, h_broadcast, (hipStream_t)stream);
}
PF_EXPORT int pffftd_hip_fft2_convolve_batch(PFFFTD_HIP_Fft2Setup* s, const double* in, const double* H, double* out, double scaling, size_t batch,
                                             int conj_h, int h_broadcast, void* stream) {
    return pf::fft2conv_batch<double>(s, in, H, out, scaling, batch, conj_h, h_broadcast, (hipStream_t)stream);
}
PF_EXPORT const char* pffft_hip_fft2_convolve_route(const void* setup, int h_broadcast) {
    const pf::Fft2Setup* z = pf::checked_handle<pf::Fft2Setup>(setup);
    if (!z) return "";
    return pf::fft2conv_fused_now(z, h_broadcast, pf::ab()) ? "fused" : "composed";
}
