// libpffft_hip.so, translation unit of the 2-D real transforms (include/pffft_hip.h: pffft[d]_hip_rfft2_*): batched transforms of dense
// rows x cols real images to rows x (cols / 2 + 1) half-spectra and back, natural order.  The handle owns a real inner setup of length cols,
// a complex one of length rows and no tables; the fused kernel's launch (one kernel per call, float, rows 16 / 32 / 64, cols 32 / 64) and
// the composed route (ordered real transform_batch over the rows, an unpacking + transposing kernel into a chunked scratch image,
// transform_batch over the columns, the transposing kernel of fft_fft2.h back, times the scaling; backward the mirror).
// Kernels: fft_rfft2.h.  On the same handle the spectral convolution of real images out = s rows cols irfft2(rfft2(in) . G)
// (pffft[d]_hip_rfft2_convolve_batch): its fused kernel's launch and the composed route on the handle's own transforms around the product
// kernel of fft_fft2c.h, through a second scratch for the half-spectra.  Kernels: fft_rfft2c.h.
#include <memory>

#include "fft2d_host.h"
#include "fft_rfft2c.h"

namespace pf {

constexpr uint32_t RFFT2_MAGIC = 0x50465232u;   // "PFR2"

// The owned inner setups: `inner` (real, length cols) transforms the rows, `inner_rows` (complex, length rows) the columns.  The fused row
// pass of cols = 64 reads the table W_64^j of a COMPLEX setup of length 64, which the real inner setup's table is not: `inner64` is that
// setup where the shape is fusable, cols is 64 and inner_rows has another length.  One setup serves ONE device (bind_device_once).
struct Rfft2Setup : InnerOwner<RFFT2_MAGIC> {
    static constexpr const char* KIND = "rfft2";
    int rows = 0, cols = 0;
    bool fusable = false;          // float and rfft2_fused_shape
    Setup* inner_rows = nullptr;
    Setup* inner64 = nullptr;
    DeviceBinding bound;
    StreamScratch pad;             // the composed route's image: one per stream, pad.mu held while a call enqueues
    StreamScratch spec;            // the composed convolution's half-spectra: one per stream, spec.mu held (outside pad.mu) while a call enqueues
};

// ------------------------------------------------------------------------------------------------ plan
// Whether the next group's chunks are requested before the last pass (1) or behind the store (0) - arithmetic on the resource remarks of
// every instantiation (tools/rfft2_resources.py; the table of DESIGN.md §3.27), not a measurement: 1 where it keeps the waves per SIMD that
// PF 0 has (no form has scratch).  Three forms lose a wave per SIMD to the chunks held across the last pass and take PF 0: 32 x 32 and
// 32 x 64 forward, 64 x 32 backward.
template <int R, int C, int DIR> constexpr int rfft2_pf() { return !((R == 32 && DIR == 0) || (R == 64 && C == 32 && DIR == 1)); }

// Shapes where the fused kernel is the default: a shape is in it where tests/test_gpu_rfft2.py test_default_cells holds the fused kernel
// faster than selector 150 on the device by more than the spread of identical rounds.  A shape that is not returns false
// here and stays reachable through AB_RFFT2_FUSED.  Measured on an MI355X at 64 MiB of half-spectra, both directions: fused wins all six
// shapes, 1.8 x (64 x 32 forward) to 4.8 x (16 x 64 forward), against a spread of the composed rounds of at most 1.01.
static bool rfft2_fused_default(int rows, int cols) {
    (void)rows; (void)cols;
    return true;
}

static bool rfft2_fused_now(const Rfft2Setup* z, const AbSel& sel) {
    return fused_selected(sel, AB_RFFT2_COMPOSED, AB_RFFT2_FUSED, z->fusable, rfft2_fused_default(z->rows, z->cols));
}

static Rfft2Setup* rfft2_new_setup(int rows, int cols, int is_double) {
    if (rows < 1 || cols < 1) return nullptr;
    std::unique_ptr<Rfft2Setup> z(new Rfft2Setup);
    z->rows = rows; z->cols = cols;
    z->fusable = !is_double && rfft2_fused_shape(rows, cols);
    if (!z->new_inner(cols, PFFFT_REAL, is_double)) return nullptr;
    if (!(z->inner_rows = z->add_inner(rows, PFFFT_COMPLEX))) return nullptr;
    if (z->fusable && cols == 64 && rows != 64)
        if (!(z->inner64 = z->add_inner(64, PFFFT_COMPLEX))) return nullptr;
    return z.release();
}

// ------------------------------------------------------------------------------------------------ the routes
// The counters come from the columns' inner setup; the W_64 values from the table W_64^j of whichever complex setup has length 64.
static int rfft2_fused(Rfft2Setup* z, const float* in, float* out, size_t batch, int dir, float scaling, hipStream_t st) {
    if (int rc = inner_on_device(z->inner_rows, st)) return rc;
    if (z->inner64)
        if (int rc = inner_on_device(z->inner64, st)) return rc;
    Setup* s64 = z->rows == 64 ? z->inner_rows : z->inner64;
    const cx<float>* tw64 = s64 ? s64->d_tw.as<cx<float>>() : nullptr;
    const size_t real_image = (size_t)z->rows * z->cols, spec_image = (size_t)z->rows * (z->cols / 2 + 1) * 2;
    const bool back = dir == PFFFT_BACKWARD;
    return fft2d_fused(in, back ? spec_image : real_image, out, back ? real_image : spec_image, batch, [&](const float* pi, float* po, size_t nb) {
        return with_one_of<16, 32, 64>(z->rows, [&](auto R) {
            return with_flag(z->cols == 64, [&](auto W) {
                return with_flag(back, [&](auto D) {
                    constexpr int r = decltype(R)::value, c = decltype(W)::value ? 64 : 32, d = decltype(D)::value;
                    return fft2d_fused_launch<Rfft2Cfg<r, c>>(z->inner_rows, fft_rfft2_kernel<r, c, d, rfft2_pf<r, c, d>()>, tw64, pi, po, nb, scaling, st);
                });
            });
        });
    });
}

// One image of rows x bins complex values of the scratch per image of a chunk; `in` is read only.  Forward, the packed row spectra wait in
// the front of the chunk's part of `out` (rows cols of its 2 rows bins scalars per image) until the unpacking kernel has read them.
// Backward, the packed spectra are written into `out` and transformed in place there.
template <typename T>
static int rfft2_composed(Rfft2Setup* z, const T* in, T* out, size_t batch, int dir, T s, hipStream_t st) {
    const size_t R = (size_t)z->rows, C = (size_t)z->cols, H = C / 2, bins = H + 1;
    return chunked_scratch<cx<T>>(z->pad, st, batch, R * bins * sizeof(cx<T>), "the scratch image", [&](cx<T>* X, size_t v0, size_t cnt) {
        if (dir == PFFFT_FORWARD) {
            const T* src = in + v0 * R * C;
            T* dst = out + v0 * R * bins * 2;
            if (int rc = inner_transform_batch<T>(z->inner, src, dst, cnt * R, dir, 1, st)) return rc;
            if (int rc = fft2d_tile_launch(rfft2_unpack_kernel<T>, cnt, R, bins, st, reinterpret_cast<const cx<T>*>(dst), X, cnt, (unsigned)R, (unsigned)H))
                return rc;
            if (int rc = inner_transform_batch<T>(z->inner_rows, (const T*)X, (T*)X, cnt * bins, dir, 1, st)) return rc;
            return fft2d_transpose<T, 1>(X, reinterpret_cast<cx<T>*>(dst), cnt, bins, R, s, st);
        }
        const T* src = in + v0 * R * bins * 2;
        T* dst = out + v0 * R * C;
        if (int rc = fft2d_transpose<T, 0>(reinterpret_cast<const cx<T>*>(src), X, cnt, R, bins, (T)1, st)) return rc;
        if (int rc = inner_transform_batch<T>(z->inner_rows, (const T*)X, (T*)X, cnt * bins, dir, 1, st)) return rc;
        if (int rc = fft2d_tile_launch(rfft2_pack_kernel<T>, cnt, H, R, st, X, reinterpret_cast<cx<T>*>(dst), cnt, (unsigned)R, (unsigned)H, s)) return rc;
        return inner_transform_batch<T>(z->inner, dst, dst, cnt * R, dir, 1, st);
    });
}

// ------------------------------------------------------------------------------------------------ the entry
// a validated call on a bound handle: the route of the calling thread's selector
template <typename T>
static int rfft2_run(Rfft2Setup* z, const T* in, T* out, size_t batch, int dir, T scaling, hipStream_t st) {
    if constexpr (sizeof(T) == 4) {
        if (rfft2_fused_now(z, ab())) return rfft2_fused(z, in, out, batch, dir, scaling, st);
    }
    return rfft2_composed<T>(z, in, out, batch, dir, scaling, st);
}

template <typename T>
static int rfft2_batch(void* setup, const T* in, T* out, size_t batch, int dir, T scaling, hipStream_t st) {
    Rfft2Setup* z = typed_handle<Rfft2Setup, T>(setup);
    if (!z) return (int)hipErrorInvalidHandle;
    if (int rc = fft2d_args("rfft2: ", in, out, batch, dir)) return rc == ARGS_EMPTY ? 0 : rc;
    const size_t real_bytes = batch * (size_t)z->rows * (size_t)z->cols * sizeof(T);
    const size_t spec_bytes = batch * (size_t)z->rows * (size_t)(z->cols / 2 + 1) * 2 * sizeof(T);
    const bool fwd = dir == PFFFT_FORWARD;
    if (ranges_overlap((uintptr_t)in, fwd ? real_bytes : spec_bytes, (uintptr_t)out, fwd ? spec_bytes : real_bytes))
        return bad("rfft2: out overlaps in (the two sides differ in size: there is no in-place form)");
    if (int rc = fft2d_bind(z->bound, "rfft2: ", st)) return rc;
    return rfft2_run<T>(z, in, out, batch, dir, scaling, st);
}

// ------------------------------------------------------------------------------------------------ spectral convolution of real images
// Shapes where the fused convolution kernel is the default for one broadcast H: a shape is in it where tests/test_gpu_rfft2conv.py
// test_default_cells holds selector 155 faster than selector 154 on the device by more than the spread of the composed route's
// round-bests.  A shape that loses returns false here and stays reachable through AB_RFFT2CONV_FUSED.  Measured on an
// MI355X at 64 MiB of images: fused wins all six shapes, 1.86 x (32 x 64) to 2.24 x (64 x 64), against a spread of the composed
// route's round-bests of at most 1.01.
static bool rfft2conv_fused_default(int rows, int cols) {
    (void)rows; (void)cols;
    return true;
}

// the fused kernel takes float images of the six shapes and ONE half-spectrum; per-image H is always composed
static bool rfft2conv_fused_now(const Rfft2Setup* z, int h_broadcast, const AbSel& sel) {
    return fused_selected(sel, AB_RFFT2CONV_COMPOSED, AB_RFFT2CONV_FUSED, z->fusable && h_broadcast != 0, rfft2conv_fused_default(z->rows, z->cols));
}

static int rfft2conv_fused(Rfft2Setup* z, const float* in, const float* H, float* out, float scaling, size_t batch, int conj_h, hipStream_t st) {
    if (int rc = inner_on_device(z->inner_rows, st)) return rc;
    if (z->inner64)
        if (int rc = inner_on_device(z->inner64, st)) return rc;
    Setup* s64 = z->rows == 64 ? z->inner_rows : z->inner64;
    const cx<float>* tw64 = s64 ? s64->d_tw.as<cx<float>>() : nullptr;
    const cx<float>* G = reinterpret_cast<const cx<float>*>(H);
    const size_t image = (size_t)z->rows * z->cols;
    return fft2d_fused(in, image, out, image, batch, [&](const float* pi, float* po, size_t nb) {
        return with_one_of<16, 32, 64>(z->rows, [&](auto R) {
            return with_flag(z->cols == 64, [&](auto W) {
                constexpr int r = decltype(R)::value, c = decltype(W)::value ? 64 : 32;
                typedef Rfft2ConvForm<r, c> Form;
                return fft2d_fused_conv_launch<Rfft2Cfg<r, c>>(z->inner_rows, fft_rfft2conv_kernel<r, c, Form::PF, Form::HREG>, tw64, pi, G, po, nb,
                                                              scaling, conj_h, st);
            });
        });
    });
}

// Per chunk of whole images through the half-spectrum scratch: the handle's own forward transform from in into the scratch, the product
// in place there (H modulo one half-spectrum where it is broadcast, offset by the chunk where it is per image), the handle's own
// backward transform into out with the scaling.  The transforms take whichever route pffft_hip_rfft2_route names under the calling
// thread's selector; composed, each takes the handle's scratch image (pad) inside, and refuses to grow it during a capture before it
// launches anything - the forward transform of the first chunk is the first launch of the call.
template <typename T>
static int rfft2conv_composed(Rfft2Setup* z, const T* in, const T* H, T* out, T scaling, size_t batch, int conj_h, int h_broadcast, hipStream_t st) {
    const size_t real_image = (size_t)z->rows * (size_t)z->cols, half = (size_t)z->rows * (size_t)(z->cols / 2 + 1);
    return chunked_scratch<cx<T>>(z->spec, st, batch, half * sizeof(cx<T>), "the half-spectrum scratch", [&](cx<T>* X, size_t v0, size_t cnt) {
        if (int rc = rfft2_run<T>(z, in + v0 * real_image, reinterpret_cast<T*>(X), cnt, PFFFT_FORWARD, (T)1, st)) return rc;
        const cx<T>* G = reinterpret_cast<const cx<T>*>(H) + (h_broadcast ? 0 : v0 * half);
        if (int rc = fft2conv_product<T>(X, G, cnt * half, h_broadcast ? half : cnt * half, conj_h, st)) return rc;
        return rfft2_run<T>(z, reinterpret_cast<const T*>(X), out + v0 * real_image, cnt, PFFFT_BACKWARD, scaling, st);
    });
}

template <typename T>
static int rfft2conv_batch(void* setup, const T* in, const T* H, T* out, T scaling, size_t batch, int conj_h, int h_broadcast, hipStream_t st) {
    const char* pre = "rfft2 convolve: ";
    Rfft2Setup* z = typed_handle<Rfft2Setup, T>(setup);
    if (!z) return (int)hipErrorInvalidHandle;
    if (batch == 0) return 0;
    if (!in || !H || !out) return bad_in(pre, "NULL in / H / out");
    if (!aligned16(in) || !aligned16(H) || !aligned16(out)) return bad_in(pre, "in / H / out not aligned to 16 bytes");
    const size_t bytes = batch * (size_t)z->rows * (size_t)z->cols * sizeof(T);
    const size_t himage = (size_t)z->rows * (size_t)(z->cols / 2 + 1) * 2 * sizeof(T);
    if (in != out && ranges_overlap((uintptr_t)in, bytes, (uintptr_t)out, bytes))
        return bad_in(pre, "out overlaps in (in == out, in place, is the one legal overlap)");
    if (ranges_overlap((uintptr_t)H, h_broadcast ? himage : batch * himage, (uintptr_t)out, bytes)) return bad_in(pre, "H overlaps out");
    if (int rc = fft2d_bind(z->bound, pre, st)) return rc;
    if constexpr (sizeof(T) == 4) {
        if (rfft2conv_fused_now(z, h_broadcast, ab())) return rfft2conv_fused(z, in, H, out, scaling, batch, conj_h != 0, st);
    }
    return rfft2conv_composed<T>(z, in, H, out, scaling, batch, conj_h != 0, h_broadcast, st);
}

}  // namespace pf

PF_EXPORT PFFFT_HIP_Rfft2Setup* pffft_hip_rfft2_new_setup(int rows, int cols) {
    return reinterpret_cast<PFFFT_HIP_Rfft2Setup*>(pf::rfft2_new_setup(rows, cols, 0));
}
PF_EXPORT PFFFTD_HIP_Rfft2Setup* pffftd_hip_rfft2_new_setup(int rows, int cols) {
    return reinterpret_cast<PFFFTD_HIP_Rfft2Setup*>(pf::rfft2_new_setup(rows, cols, 1));
}
PF_EXPORT void pffft_hip_rfft2_destroy_setup(PFFFT_HIP_Rfft2Setup* s) { pf::destroy_handle<pf::Rfft2Setup>(s); }
PF_EXPORT void pffftd_hip_rfft2_destroy_setup(PFFFTD_HIP_Rfft2Setup* s) { pf::destroy_handle<pf::Rfft2Setup>(s); }
PF_EXPORT int pffft_hip_rfft2_transform_batch(PFFFT_HIP_Rfft2Setup* s, const float* in, float* out, size_t batch, pffft_direction_t direction,
                                              float scaling, void* stream) {
    return pf::rfft2_batch<float>(s, in, out, batch, (int)direction, scaling, (hipStream_t)stream);
}
PF_EXPORT int pffftd_hip_rfft2_transform_batch(PFFFTD_HIP_Rfft2Setup* s, const double* in, double* out, size_t batch, pffft_direction_t direction,
                                               double scaling, void* stream) {
    return pf::rfft2_batch<double>(s, in, out, batch, (int)direction, scaling, (hipStream_t)stream);
}
PF_EXPORT const char* pffft_hip_rfft2_route(const void* setup) {
    const pf::Rfft2Setup* z = pf::checked_handle<pf::Rfft2Setup>(setup);
    if (!z) return "";
    return pf::rfft2_fused_now(z, pf::ab()) ? "fused" : "composed";
}
PF_EXPORT int pffft_hip_rfft2_convolve_batch(PFFFT_HIP_Rfft2Setup* s, const float* in, const float* H, float* out, float scaling, size_t batch,
                                             int conj_h, int h_broadcast, void* stream) {
    return pf::rfft2conv_batch<float>(s, in, H, out, scaling, batch, conj_h, h_broadcast, (hipStream_t)stream);
}
PF_EXPORT int pffftd_hip_rfft2_convolve_batch(PFFFTD_HIP_Rfft2Setup* s, const double* in, const double* H, double* out, double scaling, size_t batch,
                                              int conj_h, int h_broadcast, void* stream) {
    return pf::rfft2conv_batch<double>(s, in, H, out, scaling, batch, conj_h, h_broadcast, (hipStream_t)stream);
}
PF_EXPORT const char* pffft_hip_rfft2_convolve_route(const void* setup, int h_broadcast) {
    const pf::Rfft2Setup* z = pf::checked_handle<pf::Rfft2Setup>(setup);
    if (!z) return "";
    return pf::rfft2conv_fused_now(z, h_broadcast, pf::ab()) ? "fused" : "composed";
}
