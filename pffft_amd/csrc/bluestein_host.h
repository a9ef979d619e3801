// Host code shared by the translation units that put a loader / store policy around the library's own convolution: Bluestein's algorithm
// (any_tu.hip, zoom_tu.hip), the analytic signals (analytic_tu.hip) and, for the walk of the fused lengths alone, the correlations
// (xcorr_tu.hip).  The spectrum of the fixed filter, the launch of fft_conv_kernel with a policy (the fused route) and the pad ->
// convolve_batch -> crop sequence through a per-stream scratch image (the composed route).  The handle base, the inner setup's device
// test and typed entries, the slices and the chunked scratch are pf_compose.h's.
#pragma once
#include <vector>

#include "pf_compose.h"
#include "fft_conv.h"

namespace pf {

// the spectrum of one filter b (M values, double whatever the setup's type; overwritten) in the internal layout of `inner` (a complex
// PFFFT_Setup / PFFFTD_Setup of length M in the type T), into `dst`
template <typename T>
static int bluestein_filter_spectrum(Setup* inner, size_t M, std::vector<cx<double>>& b, DevBuf& dst) {
    int rc = dst.grow(M * sizeof(cx<T>));
    if (rc) return rc;
    if constexpr (sizeof(T) == 8) {
        PF_CHECK(hipMemcpy(dst.get(), b.data(), M * sizeof(cx<double>), hipMemcpyHostToDevice));
        if ((rc = inner_transform_batch<T>(inner, dst.as<T>(), dst.as<T>(), 1, PFFFT_FORWARD, 0, nullptr))) return rc;
    } else {
        // float: the filter spectrum from the DOUBLE transform, rounded once (a float transform of b would add its error to every output);
        // the permutation into the internal layout is exact
        PFFFTD_Setup* sd = pffftd_new_setup((int)M, PFFFT_COMPLEX);
        if (!sd) {
            g_last_error = "pffft_hip: no double setup for the filter spectrum";
            return (int)hipErrorInvalidValue;
        }
        DevBuf tmp, tmpf;
        rc = tmp.grow(M * sizeof(cx<double>));
        if (!rc) rc = tmpf.grow(M * sizeof(cx<float>));
        hipError_t e = hipSuccess;
        if (!rc) e = hipMemcpy(tmp.get(), b.data(), M * sizeof(cx<double>), hipMemcpyHostToDevice);
        if (!rc && e == hipSuccess) rc = pffftd_hip_transform_batch(sd, tmp.as<double>(), tmp.as<double>(), 1, PFFFT_FORWARD, 1, nullptr);
        if (!rc && e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (!rc && e == hipSuccess) e = hipMemcpy(b.data(), tmp.get(), M * sizeof(cx<double>), hipMemcpyDeviceToHost);
        pffftd_destroy_setup(sd);
        if (rc) return rc;
        if (e != hipSuccess) return fail(e, "the filter spectrum of a Bluestein setup");
        std::vector<cx<float>> bf(M);
        for (size_t m = 0; m < M; ++m) bf[m] = mk<float>((float)b[m].x, (float)b[m].y);
        PF_CHECK(hipMemcpy(tmpf.get(), bf.data(), M * sizeof(cx<float>), hipMemcpyHostToDevice));
        rc = inner_zreorder_batch<float>(inner, tmpf.as<float>(), dst.as<float>(), 1, PFFFT_BACKWARD, nullptr);
        e = hipStreamSynchronize(nullptr);   // (the permutation reads tmpf: it has finished before the temporaries go)
        if (rc) return rc;
        if (e != hipSuccess) return fail(e, "the filter spectrum of a Bluestein setup");
        return 0;
    }
    PF_CHECK(hipStreamSynchronize(nullptr));
    return 0;
}

// ------------------------------------------------------------------------------------------------ the fused route
// fft_conv_kernel<C, 0, IO> on `batch` rows under the launch rule of the convolution kernel (conv_tu.hip); `s` is the resolved inner
// setup of length M, H the filter spectrum in its internal layout
template <class C, class IO>
static int bluestein_fused_launch(Setup* s, const IO& io, const float* H, size_t batch, int M, hipStream_t st) {
    const cx<float>* tw = s->d_tw.as<cx<float>>();
    return loop_launch_last(s, st, fft_conv_kernel<C, 0, IO>, C::WG_THREADS, C::LDS_BYTES, (batch + C::T_PER_WG - 1) / C::T_PER_WG, CONV_ONESHOT, io, H,
                            (unsigned)batch, 1.0f / (float)M, tw, tw);
}

// The fused route of a float setup whose convolution length M is one of the fused lengths: the inner setup must hold its tables on the
// calling thread's device; the batch goes out in slices on the same stream (for_slices).  launch(CfgTag<C>(), first row, rows) forms the
// policy object of that slice and calls bluestein_fused_launch<C>.
template <class F>
static int bluestein_fused(Setup* inner, int M, size_t batch, hipStream_t st, F&& launch) {
    typedef ConvPick<float> P;
    if (int rc = inner_on_device(inner, st)) return rc;
    return for_slices(batch, [&](size_t b0, size_t nb) {
        switch (M) {
            case 512: return launch(CfgTag<P::C512>(), b0, nb);
            case 1024: return launch(CfgTag<P::C1024>(), b0, nb);
            case 2048: return launch(CfgTag<P::C2048>(), b0, nb);
            case 4096: return launch(CfgTag<P::C4096>(), b0, nb);
            default: return bad("no fused kernel for this convolution length");
        }
    });
}

// ------------------------------------------------------------------------------------------------ the composed route
// pad kernel -> pffft[d]_hip_convolve_batch on `inner` (length M, one broadcast filter spectrum H, scaled by 1 / M) -> crop kernel, in
// chunks of at most SCRATCH_CAP_BYTES of scratch (one row where a row is longer).  pad_k(X, first row, rows) and crop_k(X, first row, rows)
// launch the two ends on `st` and return 0 or an error.
template <typename T, class PadK, class CropK>
static int bluestein_composed(Setup* inner, StreamScratch& pad, const T* H, size_t M, size_t batch, hipStream_t st, PadK&& pad_k, CropK&& crop_k) {
    const T scaling = (T)1 / (T)M;
    return chunked_scratch<cx<T>>(pad, st, batch, M * sizeof(cx<T>), "the scratch image", [&](cx<T>* X, size_t v0, size_t cnt) {
        if (int rc = pad_k(X, v0, cnt)) return rc;
        if (int rc = inner_convolve_batch<T>(inner, (const T*)X, H, (T*)X, scaling, cnt, st)) return rc;
        return crop_k(X, v0, cnt);
    });
}

}  // namespace pf
