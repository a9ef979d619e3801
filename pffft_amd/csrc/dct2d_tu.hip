// libpffft_hip.so, translation unit of the 2-D cosine / sine transforms (include/pffft_hip.h: pffft[d]_hip_dct2d_*): types II and III of
// dense rows x cols real images, the 1-D transform of pffft[d]_hip_dct_* along the columns index and then along the rows index.  The
// handle owns two 1-D dct handles (one where rows == cols) and no tables: t_k and the product dct_mul are the 1-D entry's.  The fused
// kernel's launch (one kernel per call, float, rows and cols 32 / 64) and the composed route: dct_transform_batch over the rows, a real
// transposing kernel into a chunked scratch image, dct_transform_batch over the columns in place there, the transposing kernel back.
// Kernels: fft_dct2d.h.
#include <memory>

#include "dct_host.h"
#include "fft2d_host.h"
#include "fft_dct2d.h"

namespace pf {

constexpr uint32_t DCT2D_MAGIC = 0x50464432u;   // "PFD2"

// The owned 1-D handles (public ones, through the C ABI): `along_cols` of length cols transforms the rows of an image, `along_rows` of
// length rows its columns; they are one handle where rows == cols.  A fusable handle also owns `inner` (the base's), a COMPLEX setup of
// length 64: its table W_64^j serves the 64-point passes of the fused kernel, and its counters every fused launch.  One setup serves ONE
// device (bind_device_once).
struct Dct2dSetup : InnerOwner<DCT2D_MAGIC> {
    static constexpr const char* KIND = "dct2d";
    int rows = 0, cols = 0, kind = 0, norm = 0;
    bool fusable = false;          // float and dct2d_fused_shape
    void* along_cols = nullptr;
    void* along_rows = nullptr;
    DeviceBinding bound;
    StreamScratch pad;             // the composed route's transposed image: one per stream, pad.mu held while a call enqueues
    ~Dct2dSetup() {
        if (along_rows != along_cols) drop(along_rows);
        drop(along_cols);
    }
    void* make(int N) const {
        return is_double ? (void*)pffftd_hip_dct_new_setup(N, (pffft_hip_dct_kind_t)kind, (pffft_hip_dct_norm_t)norm)
                         : (void*)pffft_hip_dct_new_setup(N, (pffft_hip_dct_kind_t)kind, (pffft_hip_dct_norm_t)norm);
    }
    void drop(void* h) const {
        if (is_double) pffftd_hip_dct_destroy_setup(static_cast<PFFFTD_HIP_DctSetup*>(h));
        else pffft_hip_dct_destroy_setup(static_cast<PFFFT_HIP_DctSetup*>(h));
    }
};

// ------------------------------------------------------------------------------------------------ plan
// Whether the next group's chunks are requested before the last pass (1) or behind the store (0), per shape and kind (dct2, dct3, dst2,
// dst3) - arithmetic on the resource remarks of every instantiation (tools/dct2d_resources.py, which reads this table),
// not a measurement: 1 where it keeps the waves per SIMD that PF 0 has (no form has scratch or spills).  The four kinds of 64 x 32 and
// type III of 64 x 64 lose a wave per SIMD to the chunks held across the last pass and take PF 0.
template <int R, int C> struct Dct2dPf;
#define DCT2D_PF(R_, C_, K0_, K1_, K2_, K3_) \
    template <> struct Dct2dPf<R_, C_> { static constexpr int PF[4] = {K0_, K1_, K2_, K3_}; };
DCT2D_PF(32, 32, 1, 1, 1, 1)
DCT2D_PF(32, 64, 1, 1, 1, 1)
DCT2D_PF(64, 32, 0, 0, 0, 0)
DCT2D_PF(64, 64, 1, 0, 1, 0)
#undef DCT2D_PF
template <int R, int C, int KIND> constexpr int dct2d_pf() { return Dct2dPf<R, C>::PF[KIND]; }

// (shape, kind) cells where the fused kernel is the default: a cell is in it where tests/test_gpu_dct2d.py test_default_cells holds the
// fused kernel faster than selector 158 on the device by more than the spread of identical rounds.  A cell that is not
// returns false here and stays reachable through AB_DCT2D_FUSED.
static bool dct2d_fused_default(int rows, int cols, int kind) {
    (void)rows; (void)cols; (void)kind;
    return true;
}

static bool dct2d_fused_now(const Dct2dSetup* z, const AbSel& sel) {
    return fused_selected(sel, AB_DCT2D_COMPOSED, AB_DCT2D_FUSED, z->fusable, dct2d_fused_default(z->rows, z->cols, z->kind));
}

static Dct2dSetup* dct2d_new_setup(int rows, int cols, int kind, int norm, int is_double) {
    const char* pre = "dct2d: ";
    if (kind < PFFFT_HIP_DCT2 || kind > PFFFT_HIP_DST3) return bad_in(pre, "kind out of range"), nullptr;
    if (norm != PFFFT_HIP_DCT_NORM_NONE && norm != PFFFT_HIP_DCT_NORM_ORTHO) return bad_in(pre, "norm out of range"), nullptr;
    std::unique_ptr<Dct2dSetup> z(new Dct2dSetup);
    z->is_double = is_double;
    z->rows = rows; z->cols = cols; z->kind = kind; z->norm = norm;
    if (!(z->along_cols = z->make(cols))) return bad_in(pre, "cols is no length a real setup of this precision takes"), nullptr;
    z->along_rows = rows == cols ? z->along_cols : z->make(rows);
    if (!z->along_rows) return bad_in(pre, "rows is no length a real setup of this precision takes"), nullptr;
    z->fusable = !is_double && dct2d_fused_shape(rows, cols);
    if (z->fusable && !z->new_inner(64, PFFFT_COMPLEX, 0)) return nullptr;
    return z.release();
}

// ------------------------------------------------------------------------------------------------ the fused route
template <int R, int C, int KIND>
static int dct2d_fused_launch(Dct2dSetup* z, const cx<float>* tabc, const cx<float>* tabr, const float* in, float* out, size_t batch, hipStream_t st) {
    typedef Dct2dCfg<R, C> Cf;
    return loop_launch_last(z->inner, st, fft_dct2d_kernel<R, C, KIND, dct2d_pf<R, C, KIND>()>, Cf::WG, Cf::LDS_BYTES, (batch + Cf::SLOTS - 1) / Cf::SLOTS,
                            CONV_ONESHOT, in, out, (unsigned)batch, tabc, tabr, z->inner->d_tw.as<cx<float>>());
}

// The tables come from the two 1-D handles (built at their first use: not during a capture), W_64 and the counters from `inner`.
static int dct2d_fused(Dct2dSetup* z, const float* in, float* out, size_t batch, hipStream_t st) {
    if (int rc = inner_on_device(z->inner, st)) return rc;
    const cx<float>*tabc = nullptr, *tabr = nullptr;
    if (int rc = dct_device_table(z->along_cols, st, &tabc)) return rc;
    if (int rc = dct_device_table(z->along_rows, st, &tabr)) return rc;
    const size_t image = (size_t)z->rows * z->cols;
    return fft2d_fused(in, image, out, image, batch, [&](const float* pi, float* po, size_t nb) {
        return with_flag(z->rows == 64, [&](auto RW) {
            return with_flag(z->cols == 64, [&](auto CW) {
                constexpr int r = decltype(RW)::value ? 64 : 32, c = decltype(CW)::value ? 64 : 32;
                switch (z->kind) {
                    case DCT_2: return dct2d_fused_launch<r, c, DCT_2>(z, tabc, tabr, pi, po, nb, st);
                    case DCT_3: return dct2d_fused_launch<r, c, DCT_3>(z, tabc, tabr, pi, po, nb, st);
                    case DST_2: return dct2d_fused_launch<r, c, DST_2>(z, tabc, tabr, pi, po, nb, st);
                    default: return dct2d_fused_launch<r, c, DST_3>(z, tabc, tabr, pi, po, nb, st);
                }
            });
        });
    });
}

// ------------------------------------------------------------------------------------------------ the composed route
// The public 1-D entry (it validates, resolves the device and takes the 1-D route of the calling thread's selector)
template <typename T>
static int dct1d_batch(void* h, const T* in, T* out, size_t batch, hipStream_t st) {
    if constexpr (sizeof(T) == 8) return pffftd_hip_dct_transform_batch(static_cast<PFFFTD_HIP_DctSetup*>(h), in, out, batch, st);
    else return pffft_hip_dct_transform_batch(static_cast<PFFFT_HIP_DctSetup*>(h), in, out, batch, st);
}

template <typename T>
static int dct2d_transpose(const T* src, T* dst, size_t images, size_t a, size_t b, hipStream_t st) {
    return fft2d_tile_launch(dct2d_transpose_kernel<T>, images, a, b, st, src, dst, images, (unsigned)a, (unsigned)b);
}

// One image of cols x rows reals of the scratch per image of a chunk.  `in` is read by the first step only, which may run in place.
template <typename T>
static int dct2d_composed(Dct2dSetup* z, const T* in, T* out, size_t batch, hipStream_t st) {
    const size_t R = (size_t)z->rows, C = (size_t)z->cols;
    return chunked_scratch<T>(z->pad, st, batch, R * C * sizeof(T), "the scratch image", [&](T* X, size_t v0, size_t cnt) {
        const T* src = in + v0 * R * C;
        T* dst = out + v0 * R * C;
        if (int rc = dct1d_batch<T>(z->along_cols, src, dst, cnt * R, st)) return rc;
        if (int rc = dct2d_transpose<T>(dst, X, cnt, R, C, st)) return rc;
        if (int rc = dct1d_batch<T>(z->along_rows, X, X, cnt * C, st)) return rc;
        return dct2d_transpose<T>(X, dst, cnt, C, R, st);
    });
}

// ------------------------------------------------------------------------------------------------ the entry
template <typename T>
static int dct2d_batch(void* setup, const T* in, T* out, size_t batch, hipStream_t st) {
    const char* pre = "dct2d: ";
    Dct2dSetup* z = typed_handle<Dct2dSetup, T>(setup);
    if (!z) return (int)hipErrorInvalidHandle;
    if (int rc = fft2d_args(pre, in, out, batch, PFFFT_FORWARD)) return rc == ARGS_EMPTY ? 0 : rc;
    const size_t bytes = batch * (size_t)z->rows * (size_t)z->cols * sizeof(T);
    if (in != out && ranges_overlap((uintptr_t)in, bytes, (uintptr_t)out, bytes))
        return bad_in(pre, "out overlaps in (in == out, in place, is the one legal overlap)");
    if (int rc = fft2d_bind(z->bound, pre, st)) return rc;
    if constexpr (sizeof(T) == 4) {
        if (dct2d_fused_now(z, ab())) return dct2d_fused(z, in, out, batch, st);
    }
    return dct2d_composed<T>(z, in, out, batch, st);
}

}  // namespace pf

PF_EXPORT PFFFT_HIP_Dct2dSetup* pffft_hip_dct2d_new_setup(int rows, int cols, pffft_hip_dct_kind_t kind, pffft_hip_dct_norm_t norm) {
    return reinterpret_cast<PFFFT_HIP_Dct2dSetup*>(pf::dct2d_new_setup(rows, cols, (int)kind, (int)norm, 0));
}
PF_EXPORT PFFFTD_HIP_Dct2dSetup* pffftd_hip_dct2d_new_setup(int rows, int cols, pffft_hip_dct_kind_t kind, pffft_hip_dct_norm_t norm) {
    return reinterpret_cast<PFFFTD_HIP_Dct2dSetup*>(pf::dct2d_new_setup(rows, cols, (int)kind, (int)norm, 1));
}
PF_EXPORT void pffft_hip_dct2d_destroy_setup(PFFFT_HIP_Dct2dSetup* s) { pf::destroy_handle<pf::Dct2dSetup>(s); }
PF_EXPORT void pffftd_hip_dct2d_destroy_setup(PFFFTD_HIP_Dct2dSetup* s) { pf::destroy_handle<pf::Dct2dSetup>(s); }
PF_EXPORT int pffft_hip_dct2d_transform_batch(PFFFT_HIP_Dct2dSetup* s, const float* in, float* out, size_t batch, void* stream) {
    return pf::dct2d_batch<float>(s, in, out, batch, (hipStream_t)stream);
}
PF_EXPORT int pffftd_hip_dct2d_transform_batch(PFFFTD_HIP_Dct2dSetup* s, const double* in, double* out, size_t batch, void* stream) {
    return pf::dct2d_batch<double>(s, in, out, batch, (hipStream_t)stream);
}
PF_EXPORT const char* pffft_hip_dct2d_route(const void* setup) {
    const pf::Dct2dSetup* z = pf::checked_handle<pf::Dct2dSetup>(setup);
    if (!z) return "";
    return pf::dct2d_fused_now(z, pf::ab()) ? "fused" : "composed";
}
