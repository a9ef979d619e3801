"""ctypes binding of libpffft_hip.so.  Mirrors the reference's operator interface:

    reference (C)                                  here
    pffft_new_setup(N, PFFFT_COMPLEX)              Setup(N, COMPLEX, dtype=np.float32)
    pffft_transform(s, in, out, work, dir)         s.transform(x, direction)            (internal layout)
    pffft_transform_ordered(...)                   s.transform_ordered(x, direction)
    pffft_zreorder(s, in, out, dir)                s.zreorder(x, direction)
    pffft_zconvolve_accumulate / _no_accu          s.zconvolve(a, b, ab, scaling, accumulate=...)
    pffastconv_new_setup / _apply                  FastConv(h, block_len, flags).apply(x, flush)

numpy arrays go through the legacy single-vector entries (host pointers, staged by the library);
torch CUDA tensors go through the batched device entries (`*_hip_*_batch`) on the current stream.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

FORWARD, BACKWARD = 0, 1
REAL, COMPLEX = 0, 1

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


def lib_path() -> str:
    return os.path.join(_HERE, "libpffft_hip.so")


def lib():
    """Load the C-ABI library; fails loudly when it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    p = lib_path()
    if not os.path.exists(p):
        raise RuntimeError(f"{p} is missing — build it with `python -m pffft_amd.build` "
                           "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    # One HIP runtime per process: PyTorch bundles its own libamdhip64.so.7 and hands us its streams
    # and device pointers, so when torch is installed it must be loaded FIRST — the dynamic loader then
    # binds libpffft_hip.so's NEEDED libamdhip64.so.7 to that same instance (matching SONAME).  Loading
    # in the other order gives two runtimes in one process; the second one finds no device.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(p, mode=getattr(os, "RTLD_LOCAL", 0))
    for pfx, ct in (("pffft", C.c_float), ("pffftd", C.c_double)):
        g = lambda n: getattr(L, f"{pfx}_{n}")
        g("new_setup").restype = C.c_void_p; g("new_setup").argtypes = [C.c_int, C.c_int]
        g("destroy_setup").restype = None; g("destroy_setup").argtypes = [C.c_void_p]
        for n in ("transform", "transform_ordered"):
            g(n).restype = None; g(n).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        g("zreorder").restype = None; g("zreorder").argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        for n in ("zconvolve_accumulate", "zconvolve_no_accu"):
            g(n).restype = None; g(n).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, ct]
        g("simd_size").restype = C.c_int; g("simd_size").argtypes = []
        g("simd_arch").restype = C.c_char_p; g("simd_arch").argtypes = []
        g("min_fft_size").restype = C.c_int; g("min_fft_size").argtypes = [C.c_int]
        g("is_valid_size").restype = C.c_int; g("is_valid_size").argtypes = [C.c_int, C.c_int]
        g("nearest_transform_size").restype = C.c_int
        g("nearest_transform_size").argtypes = [C.c_int, C.c_int, C.c_int]
        g("next_power_of_two").restype = C.c_int; g("next_power_of_two").argtypes = [C.c_int]
        g("is_power_of_two").restype = C.c_int; g("is_power_of_two").argtypes = [C.c_int]
        g("aligned_malloc").restype = C.c_void_p; g("aligned_malloc").argtypes = [C.c_size_t]
        g("aligned_free").restype = None; g("aligned_free").argtypes = [C.c_void_p]
        g("hip_transform_batch").restype = C.c_int
        g("hip_transform_batch").argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int,
                                             C.c_int, C.c_void_p]
        g("hip_zreorder_batch").restype = C.c_int
        g("hip_zreorder_batch").argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        g("hip_zconvolve_batch").restype = C.c_int
        g("hip_zconvolve_batch").argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, ct, C.c_size_t,
                                             C.c_int, C.c_int, C.c_void_p]
        g("hip_convolve_batch").restype = C.c_int
        g("hip_convolve_batch").argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, ct, C.c_size_t,
                                            C.c_int, C.c_int, C.c_void_p]
        g("hip_frames_transform_batch").restype = C.c_int
        g("hip_frames_transform_batch").argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                                                    C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        g("hip_frames_psd_batch").restype = C.c_int
        g("hip_frames_psd_batch").argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p,
                                              C.c_size_t, ct, C.c_void_p, C.c_size_t, C.c_void_p]
        g("hip_frames_csd_batch").restype = C.c_int
        g("hip_frames_csd_batch").argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                                              C.c_void_p, C.c_size_t, ct, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
        g("hip_pfb_transform_batch").restype = C.c_int
        g("hip_pfb_transform_batch").argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                                                 C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        g("hip_frames_overlap_add_batch").restype = C.c_int
        g("hip_frames_overlap_add_batch").argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                                                      C.c_void_p, ct, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        g("hip_pfb_synthesis_batch").restype = C.c_int
        g("hip_pfb_synthesis_batch").argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t,
                                                 C.c_void_p, C.c_size_t, ct, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        g("hip_any_new_setup").restype = C.c_void_p; g("hip_any_new_setup").argtypes = [C.c_int, C.c_int]
        g("hip_any_new_real_setup").restype = C.c_void_p; g("hip_any_new_real_setup").argtypes = [C.c_int]
        g("hip_any_destroy_setup").restype = None; g("hip_any_destroy_setup").argtypes = [C.c_void_p]
        g("hip_any_transform_batch").restype = C.c_int
        g("hip_any_transform_batch").argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        g("hip_zoom_new_setup").restype = C.c_void_p; g("hip_zoom_new_setup").argtypes = [C.c_int, C.c_int, C.c_double, C.c_double]
        g("hip_zoom_destroy_setup").restype = None; g("hip_zoom_destroy_setup").argtypes = [C.c_void_p]
        g("hip_zoom_transform_batch").restype = C.c_int
        g("hip_zoom_transform_batch").argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        g("hip_dct_new_setup").restype = C.c_void_p; g("hip_dct_new_setup").argtypes = [C.c_int, C.c_int, C.c_int]
        g("hip_dct_destroy_setup").restype = None; g("hip_dct_destroy_setup").argtypes = [C.c_void_p]
        g("hip_dct_transform_batch").restype = C.c_int
        g("hip_dct_transform_batch").argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        g("hip_mdct_new_setup").restype = C.c_void_p; g("hip_mdct_new_setup").argtypes = [C.c_int]
        g("hip_mdct_destroy_setup").restype = None; g("hip_mdct_destroy_setup").argtypes = [C.c_void_p]
        g("hip_mdct_dct4_batch").restype = C.c_int
        g("hip_mdct_dct4_batch").argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        g("hip_mdct_transform_batch").restype = C.c_int
        g("hip_mdct_transform_batch").argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p,
                                                  C.c_size_t, C.c_void_p]
        g("hip_mdct_overlap_add_batch").restype = C.c_int
        g("hip_mdct_overlap_add_batch").argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, ct, C.c_void_p,
                                                    C.c_size_t, C.c_void_p]
        g("hip_analytic_new_setup").restype = C.c_void_p; g("hip_analytic_new_setup").argtypes = [C.c_int, C.c_void_p]
        g("hip_analytic_destroy_setup").restype = None; g("hip_analytic_destroy_setup").argtypes = [C.c_void_p]
        g("hip_analytic_transform_batch").restype = C.c_int
        g("hip_analytic_transform_batch").argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        g("hip_xcorr_new_setup").restype = C.c_void_p; g("hip_xcorr_new_setup").argtypes = [C.c_int] * 6
        g("hip_xcorr_destroy_setup").restype = None; g("hip_xcorr_destroy_setup").argtypes = [C.c_void_p]
        g("hip_xcorr_batch").restype = C.c_int
        g("hip_xcorr_batch").argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, ct, C.c_void_p]
        g("hip_resample_new_setup").restype = C.c_void_p; g("hip_resample_new_setup").argtypes = [C.c_int] * 3
        g("hip_resample_destroy_setup").restype = None; g("hip_resample_destroy_setup").argtypes = [C.c_void_p]
        g("hip_resample_batch").restype = C.c_int
        g("hip_resample_batch").argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, ct, C.c_void_p]
        g("hip_fft2_new_setup").restype = C.c_void_p; g("hip_fft2_new_setup").argtypes = [C.c_int, C.c_int]
        g("hip_fft2_destroy_setup").restype = None; g("hip_fft2_destroy_setup").argtypes = [C.c_void_p]
        g("hip_fft2_transform_batch").restype = C.c_int
        g("hip_fft2_transform_batch").argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, ct, C.c_void_p]
        g("hip_fft2_convolve_batch").restype = C.c_int
        g("hip_fft2_convolve_batch").argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, ct, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
        g("hip_rfft2_new_setup").restype = C.c_void_p; g("hip_rfft2_new_setup").argtypes = [C.c_int, C.c_int]
        g("hip_rfft2_destroy_setup").restype = None; g("hip_rfft2_destroy_setup").argtypes = [C.c_void_p]
        g("hip_rfft2_transform_batch").restype = C.c_int
        g("hip_rfft2_transform_batch").argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, ct, C.c_void_p]
        g("hip_rfft2_convolve_batch").restype = C.c_int
        g("hip_rfft2_convolve_batch").argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, ct, C.c_size_t, C.c_int, C.c_int, C.c_void_p]
        g("hip_dct2d_new_setup").restype = C.c_void_p; g("hip_dct2d_new_setup").argtypes = [C.c_int] * 4
        g("hip_dct2d_destroy_setup").restype = None; g("hip_dct2d_destroy_setup").argtypes = [C.c_void_p]
        g("hip_dct2d_transform_batch").restype = C.c_int
        g("hip_dct2d_transform_batch").argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        g("hip_bands_new_setup").restype = C.c_void_p
        g("hip_bands_new_setup").argtypes = [C.c_int, C.c_int, C.c_uint, C.c_void_p, C.c_void_p, C.c_void_p]
        g("hip_bands_destroy_setup").restype = None; g("hip_bands_destroy_setup").argtypes = [C.c_void_p]
        g("hip_bands_batch").restype = C.c_int
        g("hip_bands_batch").argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, ct, ct, C.c_int,
                                         C.c_void_p, C.c_size_t, C.c_void_p]
        getattr(L, f"validate_{pfx}_simd").restype = C.c_int
        getattr(L, f"validate_{pfx}_simd_ex").restype = C.c_int
        getattr(L, f"validate_{pfx}_simd_ex").argtypes = [C.c_void_p]
    L.pffastconv_new_setup.restype = C.c_void_p
    L.pffastconv_new_setup.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_int]
    L.pffastconv_destroy_setup.restype = None; L.pffastconv_destroy_setup.argtypes = [C.c_void_p]
    L.pffastconv_apply.restype = C.c_int
    L.pffastconv_apply.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.pffastconv_hip_apply_device.restype = C.c_int
    L.pffastconv_hip_apply_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    L.pffastconv_hip_apply_batch.restype = C.c_int
    L.pffastconv_hip_apply_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int,
                                             C.c_int, C.c_void_p]
    L.pffastconv_hip_route.restype = C.c_int
    L.pffastconv_hip_route.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_size_t]
    L.pffft_hip_error_count.restype = C.c_uint
    L.pffastconv_simd_size.restype = C.c_int
    L.pffft_hip_shift_transform_batch.restype = C.c_int
    L.pffft_hip_shift_transform_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_double,
                                                  C.c_double, C.c_void_p]
    L.pffft_hip_frames_route.restype = C.c_char_p
    L.pffft_hip_frames_route.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
    L.pffft_hip_frames_psd_route.restype = C.c_char_p
    L.pffft_hip_frames_psd_route.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t]
    L.pffft_hip_frames_csd_route.restype = C.c_char_p
    L.pffft_hip_frames_csd_route.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
    L.pffft_hip_pfb_route.restype = C.c_char_p
    L.pffft_hip_pfb_route.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
    L.pffft_hip_any_conv_size.restype = C.c_int; L.pffft_hip_any_conv_size.argtypes = [C.c_void_p]
    L.pffft_hip_any_route.restype = C.c_char_p; L.pffft_hip_any_route.argtypes = [C.c_void_p]
    L.pffft_hip_any_chirp.restype = C.c_int; L.pffft_hip_any_chirp.argtypes = [C.c_void_p, C.c_void_p]
    L.pffft_hip_any_is_real.restype = C.c_int; L.pffft_hip_any_is_real.argtypes = [C.c_void_p]
    L.pffft_hip_any_bins.restype = C.c_int; L.pffft_hip_any_bins.argtypes = [C.c_void_p]
    L.pffft_hip_zoom_conv_size.restype = C.c_int; L.pffft_hip_zoom_conv_size.argtypes = [C.c_void_p]
    L.pffft_hip_zoom_route.restype = C.c_char_p; L.pffft_hip_zoom_route.argtypes = [C.c_void_p]
    L.pffft_hip_zoom_table.restype = C.c_int
    L.pffft_hip_zoom_table.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p]
    L.pffft_hip_dct_route.restype = C.c_char_p; L.pffft_hip_dct_route.argtypes = [C.c_void_p]
    L.pffft_hip_dct_table.restype = C.c_int
    L.pffft_hip_dct_table.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    L.pffft_hip_mdct_route.restype = C.c_char_p; L.pffft_hip_mdct_route.argtypes = [C.c_void_p, C.c_int]
    L.pffft_hip_mdct_table.restype = C.c_int
    L.pffft_hip_mdct_table.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_size_t, C.c_void_p]
    L.pffft_hip_analytic_route.restype = C.c_char_p; L.pffft_hip_analytic_route.argtypes = [C.c_void_p, C.c_int]
    L.pffft_hip_analytic_table.restype = C.c_int
    L.pffft_hip_analytic_table.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
    L.pffft_hip_xcorr_route.restype = C.c_char_p; L.pffft_hip_xcorr_route.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.pffft_hip_resample_route.restype = C.c_char_p; L.pffft_hip_resample_route.argtypes = [C.c_void_p]
    L.pffft_hip_fft2_route.restype = C.c_char_p; L.pffft_hip_fft2_route.argtypes = [C.c_void_p]
    L.pffft_hip_fft2_convolve_route.restype = C.c_char_p; L.pffft_hip_fft2_convolve_route.argtypes = [C.c_void_p, C.c_int]
    L.pffft_hip_rfft2_route.restype = C.c_char_p; L.pffft_hip_rfft2_route.argtypes = [C.c_void_p]
    L.pffft_hip_rfft2_convolve_route.restype = C.c_char_p; L.pffft_hip_rfft2_convolve_route.argtypes = [C.c_void_p, C.c_int]
    L.pffft_hip_dct2d_route.restype = C.c_char_p; L.pffft_hip_dct2d_route.argtypes = [C.c_void_p]
    L.pffft_hip_bands_route.restype = C.c_char_p; L.pffft_hip_bands_route.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t]
    L.pffft_hip_bands_count.restype = C.c_uint; L.pffft_hip_bands_count.argtypes = [C.c_void_p]
    L.pffft_hip_bands_bins.restype = C.c_uint; L.pffft_hip_bands_bins.argtypes = [C.c_void_p]
    L.pffft_hip_kernel_name.restype = C.c_char_p; L.pffft_hip_kernel_name.argtypes = [C.c_void_p]
    L.pffft_hip_describe.restype = C.c_int; L.pffft_hip_describe.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.pffft_hip_route_occupancy.restype = C.c_int; L.pffft_hip_route_occupancy.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.pffft_hip_setup_devices.restype = C.c_int; L.pffft_hip_setup_devices.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int]
    L.pffft_hip_last_error.restype = C.c_char_p
    L.pffft_hip_device_count.restype = C.c_int
    L.pffft_hip_set_variant.restype = None; L.pffft_hip_set_variant.argtypes = [C.c_int]
    L.pffft_hip_has_variants.restype = C.c_int; L.pffft_hip_has_variants.argtypes = []
    L.pffft_hip_tile_plan.restype = C.c_int
    L.pffft_hip_tile_plan.argtypes = [C.c_longlong, C.c_int, C.c_int, C.POINTER(C.c_int)]
    _LIB = L
    return L


def _pfx(dtype) -> str:
    return "pffftd" if np.dtype(dtype) == np.float64 else "pffft"


def device_count() -> int:
    return lib().pffft_hip_device_count()


def simd_size(dtype=np.float32) -> int:
    return getattr(lib(), f"{_pfx(dtype)}_simd_size")()


def simd_arch(dtype=np.float32) -> str:
    return getattr(lib(), f"{_pfx(dtype)}_simd_arch")().decode()


def min_fft_size(transform, dtype=np.float32) -> int:
    return getattr(lib(), f"{_pfx(dtype)}_min_fft_size")(transform)


def is_valid_size(N, transform, dtype=np.float32) -> bool:
    return bool(getattr(lib(), f"{_pfx(dtype)}_is_valid_size")(N, transform))


def nearest_transform_size(N, transform, higher, dtype=np.float32) -> int:
    return getattr(lib(), f"{_pfx(dtype)}_nearest_transform_size")(N, transform, int(bool(higher)))


def error_count() -> int:
    """Legacy (void) entries that failed soft in this process (include/pffft_hip.h)."""
    return int(lib().pffft_hip_error_count())


def last_error() -> str:
    return lib().pffft_hip_last_error().decode()


def set_variant(v: int) -> None:
    lib().pffft_hip_set_variant(int(v))


def has_variants() -> bool:
    """True for a development build (PFFFT_HIP_VARIANTS=1): both variants of every Stockham plan are instantiated."""
    return bool(lib().pffft_hip_has_variants())


def tile_plan(n, is_double=False, deep=False):
    """Tile lengths of the passes over HBM of a complex core transform of n points beyond LDS ([] = streaming passes / not planned
    by the tile planner): include/pffft_hip.h pffft_hip_tile_plan.  Host arithmetic only."""
    buf = (C.c_int * 3)()
    k = lib().pffft_hip_tile_plan(int(n), int(bool(is_double)), int(deep), buf)
    return [int(buf[i]) for i in range(k)]


def kernel_name(setup: "Setup") -> str:
    return lib().pffft_hip_kernel_name(setup.handle).decode()


def describe(setup: "Setup") -> str:
    """pffft_hip_describe: the routes the planner chose for this setup, one line per (direction, layout) - under set_variant(v), the
    routes that selector runs."""
    buf = C.create_string_buffer(4096)
    n = lib().pffft_hip_describe(setup.handle, buf, len(buf))
    if n < 0:
        raise ValueError("pffft_hip_describe: invalid handle")
    return buf.value.decode()


def route_occupancy(setup: "Setup", direction, ordered) -> int:
    """pffft_hip_route_occupancy: resident workgroups per CU of the LDS-resident kernel a (direction, layout) runs on, as its launcher sees
    them; 0 where the route has no single persistent kernel of the tiled / Stockham / single-image families.  Needs a device."""
    n = lib().pffft_hip_route_occupancy(setup.handle, int(direction), int(bool(ordered)))
    if n < 0:
        raise RuntimeError("pffft_hip_route_occupancy failed: " + lib().pffft_hip_last_error().decode())
    return n


def setup_devices(setup: "Setup"):
    """pffft_hip_setup_devices: the devices this setup holds tables / counters / scratch on (first-use device first)."""
    buf = (C.c_int * 80)()
    n = lib().pffft_hip_setup_devices(setup.handle, buf, 80)
    return [buf[i] for i in range(min(n, 80))]


FRAMES_OUTPUTS = {"internal": 0, "ordered": 1, "power": 2}


def frames_route(setup: "Setup", hop, signal_stride=0, out_stride=0, output="ordered") -> str:
    """pffft_hip_frames_route: "fused" / "composed" for an analysis call with 16-byte aligned pointers, under the calling
    thread's selector.  Host arithmetic only."""
    return lib().pffft_hip_frames_route(setup.handle, int(hop), int(signal_stride), int(out_stride),
                                        FRAMES_OUTPUTS[output]).decode()


PSD_RUN = 32   # PFFFT_HIP_PSD_RUN of include/pffft_hip.h


def frames_psd_route(setup: "Setup", hop, signal_stride=0, navg=0) -> str:
    """pffft_hip_frames_psd_route: "fused" / "composed" for an averaged-power call with 16-byte aligned pointers, under the calling
    thread's selector.  Host arithmetic only."""
    return lib().pffft_hip_frames_psd_route(setup.handle, int(hop), int(signal_stride), int(navg)).decode()


CSD_WHAT = {"cross": 0, "all": 1, "coherence": 2}   # PFFFT_HIP_CSD_* of include/pffft_hip.h


def frames_csd_route(setup: "Setup", hop, x_stride=0, y_stride=0, navg=0, what="cross") -> str:
    """pffft_hip_frames_csd_route: "fused" / "composed" for an averaged cross-spectrum call with 16-byte aligned pointers, under the
    calling thread's selector.  Host arithmetic only."""
    return lib().pffft_hip_frames_csd_route(setup.handle, int(hop), int(x_stride), int(y_stride), int(navg), CSD_WHAT[what]).decode()


PFB_FUSED_MAX_TAPS = 16   # PFFFT_HIP_PFB_FUSED_MAX_TAPS of include/pffft_hip.h


def pfb_route(setup: "Setup", hop, taps, signal_stride=0, out_stride=0, output="ordered") -> str:
    """pffft_hip_pfb_route: "fused" / "composed" for a filter-bank call with aligned pointers, under the calling thread's
    selector.  Host arithmetic only."""
    return lib().pffft_hip_pfb_route(setup.handle, int(hop), int(taps), int(signal_stride), int(out_stride),
                                     FRAMES_OUTPUTS[output]).decode()


def any_route(setup) -> str:
    """pffft_hip_any_route: "direct" / "fused" / "composed" for an any-length setup (AnySetup or AnyRealSetup) under the calling thread's
    selector.  Host arithmetic only."""
    return lib().pffft_hip_any_route(setup.handle).decode()


def zoom_route(setup) -> str:
    """pffft_hip_zoom_route: "fused" / "composed" for a ZoomSetup under the calling thread's selector.  Host arithmetic only."""
    return lib().pffft_hip_zoom_route(setup.handle).decode()


ANALYTIC_WHAT = {"analytic": 0, "hilbert": 1, "envelope": 2}   # pffft_hip_analytic_what_t


def analytic_route(setup, what="analytic") -> str:
    """pffft_hip_analytic_route: "fused" / "composed" for an AnalyticSetup and one of its outputs under the calling thread's selector; ""
    for another `what`.  Host arithmetic only."""
    return lib().pffft_hip_analytic_route(setup.handle, ANALYTIC_WHAT[what] if what in ANALYTIC_WHAT else int(what)).decode()


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what} failed ({rc}): {lib().pffft_hip_last_error().decode()}")


def _aligned_empty(n, dtype):
    dtype = np.dtype(dtype)
    raw = np.empty(n * dtype.itemsize + 64, dtype=np.uint8)
    off = (-raw.ctypes.data) % 64
    return raw[off:off + n * dtype.itemsize].view(dtype)


def _aligned(a, dtype):
    a = np.asarray(a, dtype=dtype).ravel()
    if a.ctypes.data % 64 == 0 and a.flags.c_contiguous:
        return a
    out = _aligned_empty(a.size, dtype)
    out[:] = a
    return out


class _Handle:
    """What the handle classes share: the library, the precision prefix of its entries, one constructor tail, close() / __del__, and the
    checks of torch arguments.  A class names its C constructor and destructor (after the prefix) in _new / _destroy."""

    _new = _destroy = ""
    handle = None

    def _fn(self, name):
        return getattr(self._L, f"{self._pfx}_{name}")

    def _open(self, pfx, *args, shown):
        """handle = <pfx>_<_new>(*args); `shown` is the call as the ValueError words it where the library returns NULL."""
        self._pfx, self._L = pfx, lib()
        self.handle = self._fn(self._new)(*args)
        if not self.handle:
            raise ValueError(f"{shown} returned NULL")

    def close(self):
        if getattr(self, "handle", None):
            self._fn(self._destroy)(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _stream():
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def _torch_dtype(self):
        import torch
        return torch.float64 if self.dtype == np.float64 else torch.float32

    def _whole_rows(self, t, row):
        """The batch of a dense tensor of rows of `row` scalars."""
        assert t.is_cuda and t.dtype == self._torch_dtype() and t.is_contiguous() and t.numel() % row == 0, \
            "need a contiguous CUDA tensor of the setup dtype holding whole rows"
        return t.numel() // row

    def _dense_out(self, out, x, batch, row):
        """out (None: a new [batch, row] tensor next to x), dense and of that size."""
        import torch
        if out is None:
            out = torch.empty((batch, row), dtype=x.dtype, device=x.device)
        assert out.is_cuda and out.dtype == x.dtype and out.is_contiguous() and out.numel() == batch * row
        return out

    def _complex_table(self, fn, *index_args, count, detail=True):
        """`count` complex values of the setup's precision from the table reader fn(handle, *index_args, out) (host arithmetic only)."""
        out = np.empty(2 * max(int(count), 0), dtype=self.dtype)
        rc = getattr(self._L, fn)(self.handle, *index_args, out.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"{fn} failed ({rc})" + (f": {self._L.pffft_hip_last_error().decode()}" if detail else ""))
        return out.view(np.complex128 if self.dtype == np.float64 else np.complex64)


class Setup(_Handle):
    """PFFFT_Setup / PFFFTD_Setup.  Raises ValueError where pffft_new_setup returns NULL
    (src/pffft_priv_impl.h:1066-1078,1105-1109)."""

    _new, _destroy = "new_setup", "destroy_setup"

    def __init__(self, N: int, transform: int, dtype=np.float32):
        self.N, self.transform_type, self.dtype = int(N), int(transform), np.dtype(dtype)
        self._open(_pfx(dtype), self.N, self.transform_type, shown=f"pffft_new_setup({N}, {transform})")
        self.vec_scalars = self.N * (2 if transform == COMPLEX else 1)

    # ---------------- device (torch CUDA tensors): batched entries ----------------
    def _tcheck(self, t):
        assert t.is_cuda and t.dtype == self._torch_dtype() and t.is_contiguous(), "need contiguous CUDA tensor of the setup dtype"
        assert t.numel() % self.vec_scalars == 0
        return t.numel() // self.vec_scalars

    def transform_batch(self, x, out=None, direction=FORWARD, ordered=False):
        """x: CUDA tensor holding `batch` contiguous vectors.  out may be x (in place)."""
        import torch
        batch = self._tcheck(x)
        if out is None:
            out = torch.empty_like(x)
        assert self._tcheck(out) == batch
        _check(self._fn("hip_transform_batch")(self.handle, x.data_ptr(), out.data_ptr(), batch, direction, int(bool(ordered)),
                                               self._stream()), "hip_transform_batch")
        return out

    def shift_transform_batch(self, x, rate, phase_rad=0.0, out=None, ordered=False):
        """pffft_hip_shift_transform_batch: x is ONE stream of batch*N complex samples; sample g is multiplied by
        exp(j (phase_rad + 2 pi rate g)) (src/pf_mixer.cpp:142-165) and every N samples are forward-transformed."""
        import torch
        assert self.transform_type == COMPLEX and self.dtype == np.float32
        batch = self._tcheck(x)
        if out is None:
            out = torch.empty_like(x)
        _check(self._L.pffft_hip_shift_transform_batch(self.handle, x.data_ptr(), out.data_ptr(), batch,
                                                       int(bool(ordered)), float(rate), float(phase_rad), self._stream()),
               "hip_shift_transform_batch")
        return out

    def zreorder_batch(self, x, out=None, direction=FORWARD):
        import torch
        batch = self._tcheck(x)
        if out is None:
            out = torch.empty_like(x)
        _check(self._fn("hip_zreorder_batch")(self.handle, x.data_ptr(), out.data_ptr(), batch, direction, self._stream()),
               "hip_zreorder_batch")
        return out

    def zconvolve_batch(self, a, b, ab, scaling, accumulate=True, b_broadcast=False):
        batch = self._tcheck(a)
        self._tcheck(ab)
        _check(self._fn("hip_zconvolve_batch")(self.handle, a.data_ptr(), b.data_ptr(), ab.data_ptr(), scaling, batch,
                                               int(bool(accumulate)), int(bool(b_broadcast)), self._stream()), "hip_zconvolve_batch")
        return ab

    def convolve_batch(self, x, H, out=None, scaling=1.0, accumulate=False):
        """pffft_hip_convolve_batch: out (+)= backward(forward(x) . H) * scaling; H = ONE spectrum in the internal layout
        (1-D tensor, broadcast) or one per vector (same shape as x)."""
        import torch
        batch = self._tcheck(x)
        if out is None:
            assert not accumulate
            out = torch.empty_like(x)
        self._tcheck(out)
        bc = H.numel() == self.vec_scalars
        assert bc or H.numel() == x.numel()
        assert H.is_cuda and H.dtype == x.dtype and H.is_contiguous()
        _check(self._fn("hip_convolve_batch")(self.handle, x.data_ptr(), H.data_ptr(), out.data_ptr(), scaling, batch,
                                              int(bool(accumulate)), int(bc), self._stream()), "hip_convolve_batch")
        return out

    # the frame family: analysis = signal rows -> output rows at a pitch, synthesis = spectrum rows at a pitch -> signal rows
    def _frames_rows(self, t, what):
        """(nsignals, row stride in scalars, scalars per row) of a 1-D signal / 2-D [nsignals, scalars] tensor."""
        assert t.is_cuda and t.dtype == self._torch_dtype() and t.dim() in (1, 2) and t.stride(-1) == 1, \
            f"{what}: 1-D or 2-D CUDA tensor of the setup dtype with unit stride along the samples"
        if t.dim() == 1:
            return 1, 0, t.shape[0]
        return t.shape[0], (t.stride(0) if t.shape[0] > 1 else 0), t.shape[1]

    def _spp(self) -> int:
        return 2 if self.transform_type == COMPLEX else 1

    def _analysis_in(self, signal, hop, nframes, span):
        """(nsignals, signal stride, nframes) of frames of `span` samples every `hop`; nframes None = what the signal holds."""
        nsig, sstride, scalars = self._frames_rows(signal, "signal")
        samples = scalars // self._spp()
        if nframes is None:
            assert samples >= span, "the signal holds no frame"
            nframes = (samples - span) // hop + 1
        assert nframes == 0 or (nframes - 1) * hop + span <= samples, "the signal is shorter than its frames"
        return nsig, sstride, nframes

    @staticmethod
    def _rows_out(out, signal, nsig, rows, row, name):
        """(out, its row pitch): out [nsignals,] rows, row] next to `signal` (allocated when None), row v of `name` at v * pitch."""
        import torch
        if out is None:
            out = torch.empty((nsig, rows, row) if signal.dim() == 2 else (rows, row), dtype=signal.dtype, device=signal.device)
        assert out.dtype == signal.dtype and out.is_cuda and out.stride(-1) == 1 and out.shape[-1] == row and out.shape[-2] == rows
        assert out.dim() == 2 or (out.dim() == 3 and out.shape[0] == nsig)
        pitch = out.stride(-2) if rows > 1 else (out.stride(0) if out.dim() == 3 and nsig > 1 else row)
        assert out.dim() == 2 or nsig == 1 or out.stride(0) == rows * pitch, f"{name} is written at v * pitch"
        return out, pitch

    def _synthesis_in(self, spectra):
        """(nsignals, nframes, row pitch) of spectra [nsignals,] nframes, N or 2N scalars]."""
        assert spectra.is_cuda and spectra.dim() in (2, 3) and spectra.stride(-1) == 1 and spectra.shape[-1] == self.vec_scalars
        nframes = spectra.shape[-2]
        nsig = spectra.shape[0] if spectra.dim() == 3 else 1
        pitch = spectra.stride(-2) if nframes > 1 else (spectra.stride(0) if spectra.dim() == 3 and nsig > 1 else self.vec_scalars)
        assert spectra.dim() == 2 or nsig == 1 or spectra.stride(0) == nframes * pitch
        return nsig, nframes, pitch

    def _signal_out(self, out, spectra, nsig, scalars):
        """(out, its signal stride): out [nsignals,] >= scalars] next to `spectra` (allocated when None)."""
        import torch
        if out is None:
            out = torch.empty((nsig, scalars) if spectra.dim() == 3 else (scalars,), dtype=spectra.dtype, device=spectra.device)
        osig, ostride, oscalars = self._frames_rows(out, "out")
        assert osig == nsig and oscalars >= scalars
        return out, ostride

    def _window_ptr(self, window, like):
        if window is None:
            return None
        assert window.is_cuda and window.dtype == like.dtype and window.is_contiguous() and window.numel() == self.N
        return window.data_ptr()

    def _taps(self, prototype, like):
        assert prototype.is_cuda and prototype.dtype == like.dtype and prototype.is_contiguous() and prototype.dim() == 1
        taps = prototype.numel() // self.N
        assert taps >= 1 and taps * self.N == prototype.numel(), "the prototype holds taps * N coefficients"
        return taps

    def frames_out_row(self, output="internal") -> int:
        """Scalars per output row of frames_transform_batch."""
        if output == "power":
            return self.N // 2 + 1 if self.transform_type == REAL else self.N
        return self.vec_scalars

    def frames_transform_batch(self, signal, hop, nframes=None, window=None, out=None, output="internal"):
        """pffft_hip_frames_transform_batch: frames of N samples every `hop` samples of `signal` (1-D, or 2-D [nsignals, scalars] with
        the row stride taken from the tensor; complex setups: interleaved pairs), times `window` (N scalars, None = none), forward
        transformed.  Returns [nsignals,] nframes, row]; `out` may have padded rows (its stride(-2) is the row pitch)."""
        nsig, sstride, nframes = self._analysis_in(signal, hop, nframes, self.N)
        out, pitch = self._rows_out(out, signal, nsig, nframes, self.frames_out_row(output), "frame v = i nframes + f")
        _check(self._fn("hip_frames_transform_batch")(self.handle, signal.data_ptr(), sstride, nsig, nframes, hop,
                                                      self._window_ptr(window, signal), out.data_ptr(), pitch, FRAMES_OUTPUTS[output],
                                                      self._stream()), "hip_frames_transform_batch")
        return out

    @staticmethod
    def _groups(nframes, navg):
        """Groups of `navg` consecutive frames (0 = every frame of a signal) in `nframes` frames of a signal."""
        per = navg if navg else nframes
        assert nframes == 0 or nframes % per == 0, "nframes must be a multiple of navg"
        return nframes // per if nframes else 0

    def frames_psd_batch(self, signal, hop, nframes=None, window=None, navg=0, scaling=1.0, out=None):
        """pffft_hip_frames_psd_batch: |X|^2 of the frames of frames_transform_batch, averaged over groups of `navg` consecutive frames
        (0 = every frame of a signal: Welch) in the documented order and multiplied once by `scaling`.  Returns [nsignals,] nframes / navg,
        P]; `out` may have padded rows (its stride(-2) is the row pitch)."""
        nsig, sstride, nframes = self._analysis_in(signal, hop, nframes, self.N)
        groups = self._groups(nframes, navg)
        out, pitch = self._rows_out(out, signal, nsig, groups, self.frames_out_row("power"), "row v = i groups + g")
        _check(self._fn("hip_frames_psd_batch")(self.handle, signal.data_ptr(), sstride, nsig, nframes, hop,
                                                self._window_ptr(window, signal), int(navg), float(scaling), out.data_ptr(), pitch,
                                                self._stream()), "hip_frames_psd_batch")
        return out

    def frames_csd_row(self, what="cross") -> int:
        """Scalars per output row of frames_csd_batch: 2P (re, im interleaved), 4P (Pxx | Pyy | Pxy) or P."""
        return {"cross": 2, "all": 4, "coherence": 1}[what] * self.frames_out_row("power")

    def frames_csd_batch(self, x, y, hop, nframes=None, window=None, navg=0, scaling=1.0, what="cross", out=None):
        """pffft_hip_frames_csd_batch: conj(X) Y of the frames of x and y (tensors of one shape; their row strides may differ), averaged
        over groups of `navg` consecutive frames (0 = every frame of a signal: Welch) in the documented order.  what = "cross": the
        cross-spectrum times `scaling`, (re, im) interleaved; "all": Pxx | Pyy | Pxy, each times `scaling`; "coherence": |Sxy|^2 / (Sxx Syy).
        Returns [nsignals,] nframes / navg, frames_csd_row(what)]; `out` may have padded rows (its stride(-2) is the row pitch)."""
        nsig, xstride, nframes = self._analysis_in(x, hop, nframes, self.N)
        ysig, ystride, _ = self._analysis_in(y, hop, nframes, self.N)
        assert ysig == nsig and y.dim() == x.dim() and y.dtype == x.dtype, "x and y hold the same number of signals"
        groups = self._groups(nframes, navg)
        out, pitch = self._rows_out(out, x, nsig, groups, self.frames_csd_row(what), "row v = i groups + g")
        _check(self._fn("hip_frames_csd_batch")(self.handle, x.data_ptr(), xstride, y.data_ptr(), ystride, nsig, nframes, hop,
                                                self._window_ptr(window, x), int(navg), float(scaling), CSD_WHAT[what], out.data_ptr(),
                                                pitch, self._stream()), "hip_frames_csd_batch")
        return out

    def pfb_transform_batch(self, signal, hop, prototype, nframes=None, out=None, output="internal"):
        """pffft_hip_pfb_transform_batch: polyphase filter-bank analysis.  `prototype` holds taps * N coefficients; frame f folds the
        taps * N samples from f * hop on onto N points (u[j] = sum_p prototype[p N + j] x[f hop + p N + j]) and forward-transforms them.
        Tensor conventions of frames_transform_batch: returns [nsignals,] nframes, row]; `out` may have padded rows."""
        self._frames_rows(signal, "signal")                 # the signal is checked ahead of the prototype
        taps = self._taps(prototype, signal)
        nsig, sstride, nframes = self._analysis_in(signal, hop, nframes, taps * self.N)
        out, pitch = self._rows_out(out, signal, nsig, nframes, self.frames_out_row(output), "frame v = i nframes + f")
        _check(self._fn("hip_pfb_transform_batch")(self.handle, signal.data_ptr(), sstride, nsig, nframes, hop, prototype.data_ptr(), taps,
                                                   out.data_ptr(), pitch, FRAMES_OUTPUTS[output], self._stream()),
               "hip_pfb_transform_batch")
        return out

    def frames_overlap_add_batch(self, spectra, hop, window=None, scaling=1.0, out=None, ordered=False):
        """pffft_hip_frames_overlap_add_batch: spectra [nsignals,] nframes, N or 2N scalars] (stride(-2) = row pitch) are backward
        transformed (unscaled) and overlap-added every `hop` samples: out[s] = scaling * sum_f window[s - f hop] y_f[s - f hop].
        Returns [nsignals,] (nframes - 1) hop + N samples]; normalising by the window's overlap sum is the caller's `scaling`."""
        nsig, nframes, pitch = self._synthesis_in(spectra)
        out, ostride = self._signal_out(out, spectra, nsig, ((nframes - 1) * hop + self.N) * self._spp() if nframes else 0)
        _check(self._fn("hip_frames_overlap_add_batch")(self.handle, spectra.data_ptr(), pitch, nsig, nframes, hop,
                                                        self._window_ptr(window, spectra), float(scaling), out.data_ptr(), ostride,
                                                        int(bool(ordered)), self._stream()), "hip_frames_overlap_add_batch")
        return out

    def pfb_synthesis_batch(self, spectra, hop, prototype, scaling=1.0, out=None, ordered=False):
        """pffft_hip_pfb_synthesis_batch: polyphase filter-bank synthesis.  spectra [nsignals,] nframes, N or 2N scalars] (stride(-2) = row
        pitch) are backward transformed (unscaled), periodically extended over the taps * N coefficients of `prototype` and overlap-added
        every `hop` samples: out[s] = scaling * sum_f prototype[s - f hop] y_f[(s - f hop) mod N].  Tensor conventions of
        frames_overlap_add_batch: returns [nsignals,] ((nframes - 1) hop + taps N) spp scalars]; `out` may have a padded row stride."""
        nsig, nframes, pitch = self._synthesis_in(spectra)
        taps = self._taps(prototype, spectra)
        out, ostride = self._signal_out(out, spectra, nsig, ((nframes - 1) * hop + taps * self.N) * self._spp() if nframes else 0)
        _check(self._fn("hip_pfb_synthesis_batch")(self.handle, spectra.data_ptr(), pitch, nsig, nframes, hop, prototype.data_ptr(), taps,
                                                   float(scaling), out.data_ptr(), ostride, int(bool(ordered)), self._stream()),
               "hip_pfb_synthesis_batch")
        return out

    # ---------------- host (numpy): the legacy single-vector entries ----------------
    def _legacy(self, name, x, direction):
        xin = _aligned(x, self.dtype)
        assert xin.size == self.vec_scalars
        out = _aligned_empty(self.vec_scalars, self.dtype)
        getattr(self._L, f"{self._pfx}_{name}")(self.handle, xin.ctypes.data, out.ctypes.data, None, direction)
        return out

    def transform(self, x, direction=FORWARD):
        if _is_torch(x):
            return self.transform_batch(x, None, direction, ordered=False)
        return self._legacy("transform", x, direction)

    def transform_ordered(self, x, direction=FORWARD):
        if _is_torch(x):
            return self.transform_batch(x, None, direction, ordered=True)
        return self._legacy("transform_ordered", x, direction)

    def transform_inplace(self, buf: np.ndarray, direction=FORWARD, ordered=False):
        """input and output alias (allowed: include/pffft/pffft.h:157)."""
        assert buf.dtype == self.dtype and buf.size == self.vec_scalars and buf.ctypes.data % 32 == 0
        name = "transform_ordered" if ordered else "transform"
        getattr(self._L, f"{self._pfx}_{name}")(self.handle, buf.ctypes.data, buf.ctypes.data, None, direction)
        return buf

    def zreorder(self, x, direction=FORWARD):
        if _is_torch(x):
            return self.zreorder_batch(x, None, direction)
        xin = _aligned(x, self.dtype)
        out = _aligned_empty(self.vec_scalars, self.dtype)
        getattr(self._L, f"{self._pfx}_zreorder")(self.handle, xin.ctypes.data, out.ctypes.data, direction)
        return out

    def zconvolve(self, a, b, ab, scaling, accumulate=True):
        if _is_torch(a):
            return self.zconvolve_batch(a, b, ab, scaling, accumulate)
        pa, pb = _aligned(a, self.dtype), _aligned(b, self.dtype)
        pab = _aligned_empty(self.vec_scalars, self.dtype)
        pab[:] = np.asarray(ab, dtype=self.dtype).ravel()
        name = "zconvolve_accumulate" if accumulate else "zconvolve_no_accu"
        getattr(self._L, f"{self._pfx}_{name}")(self.handle, pa.ctypes.data, pb.ctypes.data, pab.ctypes.data,
                                                 self.dtype.type(scaling))
        return pab


class _AnyHandle(_Handle):
    """What AnySetup and AnyRealSetup share: the destroy entry, the convolution length, the route and the chirp."""

    _destroy = "hip_any_destroy_setup"

    @property
    def conv_size(self) -> int:
        """The convolution length M (0 on the direct route)."""
        return int(self._L.pffft_hip_any_conv_size(self.handle))

    @property
    def route(self) -> str:
        return any_route(self)

    def _chirp(self) -> np.ndarray:
        return self._complex_table("pffft_hip_any_chirp", count=self.N, detail=False)

    def _run(self, x, out, batch, direction):
        _check(self._fn("hip_any_transform_batch")(self.handle, x.data_ptr(), out.data_ptr(), batch, direction, self._stream()),
               "hip_any_transform_batch")
        return out


class AnySetup(_AnyHandle):
    """PFFFT_HIP_AnySetup / PFFFTD_HIP_AnySetup: complex transforms of any length 1 <= N <= 2^25 (include/pffft_hip.h).  Raises ValueError
    where pffft_hip_any_new_setup returns NULL.  Rows are N interleaved complex values (2N scalars), dense."""

    _new = "hip_any_new_setup"

    def __init__(self, N: int, transform: int = COMPLEX, dtype=np.float32):
        self.N, self.transform_type, self.dtype = int(N), int(transform), np.dtype(dtype)
        self._open(_pfx(dtype), self.N, self.transform_type, shown=f"pffft_hip_any_new_setup({N}, {transform})")
        self.vec_scalars = 2 * self.N

    def chirp(self) -> np.ndarray:
        """pffft_hip_any_chirp: w[n] = exp(-j pi (n^2 mod 2N) / N) as a complex array of the setup's precision (host arithmetic only)."""
        return self._chirp()

    def transform_batch(self, x, out=None, direction=FORWARD):
        """x: CUDA tensor of the setup's dtype holding `batch` rows of 2N scalars; only the extent has to be dense (a view that starts
        anywhere on the grid of complex values is accepted).  out may be x (in place)."""
        import torch
        batch = self._whole_rows(x, self.vec_scalars)
        if out is None:
            out = torch.empty_like(x)
        return self._run(x, self._dense_out(out, x, batch, self.vec_scalars), batch, direction)


class AnyRealSetup(_AnyHandle):
    """pffft[d]_hip_any_new_real_setup: real transforms of any length 1 <= N <= 2^25 with half-spectrum I/O (include/pffft_hip.h).  FORWARD
    takes rows of N reals to rows of bins = N // 2 + 1 interleaved complex values (numpy's rfft), BACKWARD the reverse, unscaled (irfft . N).
    Raises ValueError where the constructor returns NULL."""

    _new = "hip_any_new_real_setup"

    def __init__(self, N: int, dtype=np.float32):
        self.N, self.dtype = int(N), np.dtype(dtype)
        self._open(_pfx(dtype), self.N, shown=f"pffft_hip_any_new_real_setup({N})")
        self.bins = int(self._L.pffft_hip_any_bins(self.handle))

    def chirp(self) -> np.ndarray:
        """pffft_hip_any_chirp: the N chirp values, as for a complex setup of the same N."""
        return self._chirp()

    def transform_batch(self, x, out=None, direction=FORWARD):
        """x: contiguous CUDA tensor of the setup's dtype holding `batch` rows of N scalars (FORWARD) or 2 * bins scalars (BACKWARD); the
        result has `batch` rows of 2 * bins (FORWARD) or N (BACKWARD) scalars.  out must not overlap x."""
        rin, rout = (self.N, 2 * self.bins) if direction == FORWARD else (2 * self.bins, self.N)
        batch = self._whole_rows(x, rin)
        return self._run(x, self._dense_out(out, x, batch, rout), batch, direction)


class ZoomSetup(_Handle):
    """PFFFT_HIP_ZoomSetup / PFFFTD_HIP_ZoomSetup: K spectral lines from f0 in steps of df (cycles per sample) of rows of N complex samples
    (include/pffft_hip.h).  Raises ValueError where pffft_hip_zoom_new_setup returns NULL.  Rows of N interleaved complex values in, rows of
    K out, dense."""

    _new, _destroy = "hip_zoom_new_setup", "hip_zoom_destroy_setup"

    def __init__(self, N: int, K: int, f0: float, df: float, dtype=np.float32):
        self.N, self.K, self.f0, self.df, self.dtype = int(N), int(K), float(f0), float(df), np.dtype(dtype)
        self._open(_pfx(dtype), self.N, self.K, self.f0, self.df, shown=f"pffft_hip_zoom_new_setup({N}, {K}, {f0}, {df})")

    @property
    def conv_size(self) -> int:
        """The convolution length M."""
        return int(self._L.pffft_hip_zoom_conv_size(self.handle))

    @property
    def route(self) -> str:
        return zoom_route(self)

    def table(self, which: int, first: int = 0, count=None) -> np.ndarray:
        """pffft_hip_zoom_table: `count` values from index `first` of the input table a (which = 0, N entries) or the output table c
        (which = 1, max(N, K) entries) as a complex array of the setup's precision (host arithmetic only)."""
        if count is None:
            count = (self.N if which == 0 else max(self.N, self.K)) - first
        return self._complex_table("pffft_hip_zoom_table", int(which), int(first), int(count), count=count)

    def transform_batch(self, x, out=None, direction=FORWARD):
        """x: contiguous CUDA tensor of the setup's dtype holding `batch` rows of 2N scalars; the result has `batch` rows of 2K scalars.
        out must not overlap x."""
        batch = self._whole_rows(x, 2 * self.N)
        out = self._dense_out(out, x, batch, 2 * self.K)
        _check(self._fn("hip_zoom_transform_batch")(self.handle, x.data_ptr(), out.data_ptr(), batch, direction, self._stream()),
               "hip_zoom_transform_batch")
        return out


DCT_KINDS = {"dct2": 0, "dct3": 1, "dst2": 2, "dst3": 3}      # pffft_hip_dct_kind_t
DCT_NORMS = {None: 0, "none": 0, "ortho": 1}                  # pffft_hip_dct_norm_t


class DctSetup(_Handle):
    """PFFFT_HIP_DctSetup / PFFFTD_HIP_DctSetup: cosine / sine transforms of type II / III of rows of N reals (include/pffft_hip.h;
    scipy.fft.dct / dst with type = 2 / 3).  kind: "dct2" / "dct3" / "dst2" / "dst3" (or the enum value), norm: None / "ortho".  Raises
    ValueError where pffft_hip_dct_new_setup returns NULL."""

    _new, _destroy = "hip_dct_new_setup", "hip_dct_destroy_setup"

    def __init__(self, N: int, kind, norm=None, dtype=np.float32):
        self.N, self.dtype = int(N), np.dtype(dtype)
        self.kind = DCT_KINDS[kind] if kind in DCT_KINDS else int(kind)
        self.norm = DCT_NORMS[norm] if norm in DCT_NORMS else int(norm)
        self._open(_pfx(dtype), self.N, self.kind, self.norm, shown=f"pffft_hip_dct_new_setup({N}, {kind}, {norm})")

    @property
    def route(self) -> str:
        """pffft_hip_dct_route: "fused" / "composed" under the calling thread's selector.  Host arithmetic only."""
        return self._L.pffft_hip_dct_route(self.handle).decode()

    def table(self, first: int = 0, count=None) -> np.ndarray:
        """pffft_hip_dct_table: the folded table t_k, k = first ... (N/2 + 1 values in all), as a complex array of the setup's precision
        (host arithmetic only)."""
        if count is None:
            count = self.N // 2 + 1 - first
        return self._complex_table("pffft_hip_dct_table", int(first), int(count), count=count)

    def transform_batch(self, x, out=None):
        """x: contiguous CUDA tensor of the setup's dtype holding `batch` rows of N scalars; the result has the same shape.  out may be x."""
        batch = self._whole_rows(x, self.N)
        out = self._dense_out(out, x, batch, self.N)
        _check(self._fn("hip_dct_transform_batch")(self.handle, x.data_ptr(), out.data_ptr(), batch, self._stream()),
               "hip_dct_transform_batch")
        return out


class AnalyticSetup(_Handle):
    """PFFFT_HIP_AnalyticSetup / PFFFTD_HIP_AnalyticSetup: the analytic signal z = x + j H{x} of rows of N reals (scipy.signal.hilbert),
    its imaginary part and its envelope |z| (include/pffft_hip.h).  gain: None, or N/2 + 1 values that weight the bins 0 ... N/2 (a
    one-sided band-pass in the same pass).  Raises ValueError where pffft_hip_analytic_new_setup returns NULL."""

    _new, _destroy = "hip_analytic_new_setup", "hip_analytic_destroy_setup"

    def __init__(self, N: int, gain=None, dtype=np.float32):
        self.N, self.dtype = int(N), np.dtype(dtype)
        g = None
        if gain is not None:
            g = np.ascontiguousarray(gain, dtype=self.dtype).ravel()
            if g.size != self.N // 2 + 1:
                raise ValueError(f"gain holds {g.size} values, N/2 + 1 = {self.N // 2 + 1} wanted")
        self._open(_pfx(dtype), self.N, g.ctypes.data if g is not None else None,
                   shown=f"pffft_hip_analytic_new_setup({N}, {'NULL' if g is None else 'gain'})")

    def route(self, what="analytic") -> str:
        """pffft_hip_analytic_route: "fused" / "composed" for this output under the calling thread's selector.  Host arithmetic only."""
        return analytic_route(self, what)

    def table(self, first: int = 0, count=None) -> np.ndarray:
        """pffft_hip_analytic_table: the filter spectrum H[k] = c_k gain[k], k = first ... (N values in all, zeros above N/2), as a real
        array of the setup's precision (host arithmetic only)."""
        if count is None:
            count = self.N - first
        out = np.empty(max(int(count), 0), dtype=self.dtype)
        rc = self._L.pffft_hip_analytic_table(self.handle, int(first), int(count), out.ctypes.data)
        if rc != 0:
            raise RuntimeError(f"pffft_hip_analytic_table failed ({rc}): {self._L.pffft_hip_last_error().decode()}")
        return out

    def transform_batch(self, x, out=None, what="analytic"):
        """x: contiguous CUDA tensor of the setup's dtype holding `batch` rows of N scalars.  what = "analytic": the result has `batch` rows
        of 2N scalars (interleaved complex) and must not overlap x; "hilbert" / "envelope": rows of N scalars, out may be x."""
        w = ANALYTIC_WHAT[what] if what in ANALYTIC_WHAT else int(what)
        batch = self._whole_rows(x, self.N)
        out = self._dense_out(out, x, batch, 2 * self.N if w == 0 else self.N)
        _check(self._fn("hip_analytic_transform_batch")(self.handle, x.data_ptr(), out.data_ptr(), batch, w, self._stream()),
               "hip_analytic_transform_batch")
        return out


XCORR_WEIGHT = {"plain": 0, "phat": 1}              # pffft_hip_xcorr_weight_t


class XcorrSetup(_Handle):
    """PFFFT_HIP_XcorrSetup / PFFFTD_HIP_XcorrSetup: cross- and autocorrelation r[m] = sum_n conj(x[n]) y[n + m] of rows through transforms
    of length N, plain or PHAT-weighted, the lags lag0 ... lag0 + nlags - 1 (mod N) stored (include/pffft_hip.h).  real = True: rows of
    scalars in and out; else interleaved complex rows.  len_x / len_y default to N, nlags to N.  Raises ValueError where
    pffft_hip_xcorr_new_setup returns NULL."""

    _new, _destroy = "hip_xcorr_new_setup", "hip_xcorr_destroy_setup"

    def __init__(self, N: int, len_x=None, len_y=None, lag0: int = 0, nlags=None, real: bool = False, dtype=np.float32):
        self.N, self.dtype, self.real = int(N), np.dtype(dtype), bool(real)
        self.len_x = self.N if len_x is None else int(len_x)
        self.len_y = self.N if len_y is None else int(len_y)
        self.lag0 = int(lag0)
        self.nlags = self.N if nlags is None else int(nlags)
        self.spp = 1 if self.real else 2
        self._open(_pfx(dtype), self.N, int(self.real), self.len_x, self.len_y, self.lag0, self.nlags,
                   shown=f"pffft_hip_xcorr_new_setup({N}, {int(self.real)}, {self.len_x}, {self.len_y}, {self.lag0}, {self.nlags})")

    def route(self, weighting="plain", auto: bool = False) -> str:
        """pffft_hip_xcorr_route: "fused" / "composed" for (weighting, cross or auto) under the calling thread's selector; "" for another
        weighting.  Host arithmetic only."""
        w = XCORR_WEIGHT[weighting] if weighting in XCORR_WEIGHT else int(weighting)
        return self._L.pffft_hip_xcorr_route(self.handle, w, int(bool(auto))).decode()

    def correlate_batch(self, x, y=None, out=None, weighting="plain", scaling=1.0):
        """x, y: contiguous CUDA tensors of the setup's dtype holding `batch` rows of len_x / len_y elements (scalars, or interleaved
        complex pairs).  y = None (or y is x) is the autocorrelation.  The result has `batch` rows of nlags elements and must not overlap
        x or y."""
        w = XCORR_WEIGHT[weighting] if weighting in XCORR_WEIGHT else int(weighting)
        batch = self._whole_rows(x, self.len_x * self.spp)
        if y is None:
            y = x
        assert self._whole_rows(y, self.len_y * self.spp) == batch, "x and y hold different numbers of rows"
        out = self._dense_out(out, x, batch, self.nlags * self.spp)
        _check(self._fn("hip_xcorr_batch")(self.handle, x.data_ptr(), y.data_ptr(), out.data_ptr(), batch, w, float(scaling), self._stream()),
               "hip_xcorr_batch")
        return out


class ResampleSetup(_Handle):
    """PFFFT_HIP_ResampleSetup / PFFFTD_HIP_ResampleSetup: Fourier resampling of rows, N samples in and M samples out over the same span
    (include/pffft_hip.h); scaling = 1 is scipy.signal.resample(x, M).  real = True: rows of scalars in and out; else interleaved complex
    rows.  Raises ValueError where pffft_hip_resample_new_setup returns NULL (a length no complex setup of the precision takes)."""

    _new, _destroy = "hip_resample_new_setup", "hip_resample_destroy_setup"

    def __init__(self, N: int, M: int, real: bool = False, dtype=np.float32):
        self.N, self.M, self.dtype, self.real = int(N), int(M), np.dtype(dtype), bool(real)
        self.spp = 1 if self.real else 2
        self._open(_pfx(dtype), self.N, self.M, int(self.real), shown=f"pffft_hip_resample_new_setup({N}, {M}, {int(self.real)})")

    def route(self) -> str:
        """pffft_hip_resample_route: "fused" / "composed" under the calling thread's selector.  Host arithmetic only."""
        return self._L.pffft_hip_resample_route(self.handle).decode()

    def resample_batch(self, x, out=None, scaling=1.0):
        """x: contiguous CUDA tensor of the setup's dtype holding `batch` rows of N elements (scalars, or interleaved complex pairs).  The
        result has `batch` rows of M elements and must not overlap x (there is no in-place form)."""
        batch = self._whole_rows(x, self.N * self.spp)
        out = self._dense_out(out, x, batch, self.M * self.spp)
        _check(self._fn("hip_resample_batch")(self.handle, x.data_ptr(), out.data_ptr(), batch, float(scaling), self._stream()),
               "hip_resample_batch")
        return out


class Fft2Setup(_Handle):
    """PFFFT_HIP_Fft2Setup / PFFFTD_HIP_Fft2Setup: batched 2-D complex transforms of dense row-major images of rows x cols interleaved
    complex values, natural order in and out (include/pffft_hip.h): forward with scaling 1 is numpy.fft.fft2, backward ifft2 * rows * cols.
    Raises ValueError where pffft_hip_fft2_new_setup returns NULL (a length no complex setup of the precision takes)."""

    _new, _destroy = "hip_fft2_new_setup", "hip_fft2_destroy_setup"

    def __init__(self, rows: int, cols: int, dtype=np.float32):
        self.rows, self.cols, self.dtype = int(rows), int(cols), np.dtype(dtype)
        self.image_scalars = 2 * self.rows * self.cols
        self._open(_pfx(dtype), self.rows, self.cols, shown=f"pffft_hip_fft2_new_setup({rows}, {cols})")

    def route(self) -> str:
        """pffft_hip_fft2_route: "fused" / "composed" under the calling thread's selector.  Host arithmetic only."""
        return self._L.pffft_hip_fft2_route(self.handle).decode()

    def transform_batch(self, x, out=None, direction=FORWARD, scaling=1.0):
        """x: contiguous CUDA tensor of the setup's dtype holding whole images (of any shape, such as [batch, rows, 2 cols]).  out: None
        (a new tensor shaped like x), another such tensor, or x itself (in place).  direction: FORWARD / BACKWARD or "forward" /
        "backward"."""
        import torch
        d = {"forward": FORWARD, "backward": BACKWARD}.get(direction, direction)
        batch = self._whole_rows(x, self.image_scalars)
        if out is None:
            out = torch.empty_like(x)
        assert self._whole_rows(out, self.image_scalars) == batch, "x and out hold different numbers of images"
        _check(self._fn("hip_fft2_transform_batch")(self.handle, x.data_ptr(), out.data_ptr(), batch, int(d), float(scaling), self._stream()),
               "hip_fft2_transform_batch")
        return out

    def convolve_route(self, h_broadcast=True) -> str:
        """pffft_hip_fft2_convolve_route: "fused" / "composed" under the calling thread's selector.  Host arithmetic only."""
        return self._L.pffft_hip_fft2_convolve_route(self.handle, int(bool(h_broadcast))).decode()

    def convolve_batch(self, x, H, out=None, scaling=1.0, conj_h=False):
        """out = scaling * IFFT2u(FFT2(x) . G), G = H or conj(H) (conj_h), IFFT2u the unnormalised backward transform: scaling =
        1 / (rows cols) is numpy's ifft2(fft2(x) * G).  x, out as in transform_batch (out may be x).  H: contiguous CUDA tensor of the
        setup's dtype holding a spectrum in natural order, ONE image of it (broadcast over the batch) or as many images as x; any other
        size raises ValueError."""
        import torch
        batch = self._whole_rows(x, self.image_scalars)
        images = self._whole_rows(H, self.image_scalars)
        if images != 1 and images != batch:
            raise ValueError(f"H holds {images} images: it must hold 1 (broadcast) or as many as x ({batch})")
        if out is None:
            out = torch.empty_like(x)
        assert self._whole_rows(out, self.image_scalars) == batch, "x and out hold different numbers of images"
        _check(self._fn("hip_fft2_convolve_batch")(self.handle, x.data_ptr(), H.data_ptr(), out.data_ptr(), float(scaling), batch,
                                                   int(bool(conj_h)), int(images == 1), self._stream()), "hip_fft2_convolve_batch")
        return out


class Rfft2Setup(_Handle):
    """PFFFT_HIP_Rfft2Setup / PFFFTD_HIP_Rfft2Setup: batched 2-D real transforms of dense row-major images (include/pffft_hip.h): forward
    rows x cols reals -> rows x bins interleaved complex values, bins = cols / 2 + 1 (numpy.fft.rfft2 with scaling 1); backward the
    half-spectrum -> rows x cols reals (numpy.fft.irfft2 * rows * cols).  There is no in-place form.  Raises ValueError where
    pffft_hip_rfft2_new_setup returns NULL (rows: a length no complex setup of the precision takes; cols: one no real setup takes)."""

    _new, _destroy = "hip_rfft2_new_setup", "hip_rfft2_destroy_setup"

    def __init__(self, rows: int, cols: int, dtype=np.float32):
        self.rows, self.cols, self.dtype = int(rows), int(cols), np.dtype(dtype)
        self.bins = self.cols // 2 + 1
        self.image_scalars = self.rows * self.cols
        self.spectrum_scalars = 2 * self.rows * self.bins
        self._open(_pfx(dtype), self.rows, self.cols, shown=f"pffft_hip_rfft2_new_setup({rows}, {cols})")

    def route(self) -> str:
        """pffft_hip_rfft2_route: "fused" / "composed" under the calling thread's selector.  Host arithmetic only."""
        return self._L.pffft_hip_rfft2_route(self.handle).decode()

    def transform_batch(self, x, out=None, direction=FORWARD, scaling=1.0):
        """x: contiguous CUDA tensor of the setup's dtype holding whole images of the direction's input side (forward: image_scalars reals
        each; backward: spectrum_scalars each).  out: None (a new [batch, scalars of the other side] tensor) or such a tensor that does not
        overlap x.  direction: FORWARD / BACKWARD or "forward" / "backward"."""
        d = {"forward": FORWARD, "backward": BACKWARD}.get(direction, direction)
        row_in, row_out = (self.spectrum_scalars, self.image_scalars) if d == BACKWARD else (self.image_scalars, self.spectrum_scalars)
        batch = self._whole_rows(x, row_in)
        if out is None:
            out = self._dense_out(None, x, batch, row_out)
        assert self._whole_rows(out, row_out) == batch, "x and out hold different numbers of images"
        _check(self._fn("hip_rfft2_transform_batch")(self.handle, x.data_ptr(), out.data_ptr(), batch, int(d), float(scaling), self._stream()),
               "hip_rfft2_transform_batch")
        return out

    def convolve_route(self, h_broadcast=True) -> str:
        """pffft_hip_rfft2_convolve_route: "fused" / "composed" under the calling thread's selector.  Host arithmetic only."""
        return self._L.pffft_hip_rfft2_convolve_route(self.handle, int(bool(h_broadcast))).decode()

    def convolve_batch(self, x, H, out=None, scaling=1.0, conj_h=False):
        """out = scaling * rows * cols * irfft2(rfft2(x) . G), G = H or conj(H) (conj_h): scaling = 1 / (rows cols) is numpy's
        irfft2(rfft2(x) * G, s=(rows, cols)).  x: contiguous CUDA tensor of the setup's dtype holding whole real images (image_scalars
        each); out: None (a new tensor shaped like x), another such tensor, or x itself (in place).  H: contiguous CUDA tensor of the
        setup's dtype holding half-spectra in natural order (spectrum_scalars each, as transform_batch forward writes them), ONE of them
        (broadcast over the batch) or as many as x holds images; any other size raises ValueError."""
        import torch
        batch = self._whole_rows(x, self.image_scalars)
        images = self._whole_rows(H, self.spectrum_scalars)
        if images != 1 and images != batch:
            raise ValueError(f"H holds {images} half-spectra: it must hold 1 (broadcast) or as many as x ({batch})")
        if out is None:
            out = torch.empty_like(x)
        assert self._whole_rows(out, self.image_scalars) == batch, "x and out hold different numbers of images"
        _check(self._fn("hip_rfft2_convolve_batch")(self.handle, x.data_ptr(), H.data_ptr(), out.data_ptr(), float(scaling), batch,
                                                    int(bool(conj_h)), int(images == 1), self._stream()), "hip_rfft2_convolve_batch")
        return out


class Dct2dSetup(_Handle):
    """PFFFT_HIP_Dct2dSetup / PFFFTD_HIP_Dct2dSetup: batched 2-D cosine / sine transforms of type II / III of dense row-major images of
    rows x cols reals (include/pffft_hip.h; scipy.fft.dctn / dstn with type = 2 / 3 over the last two axes).  kind: "dct2" / "dct3" /
    "dst2" / "dst3" (or the enum value), norm: None / "ortho", the same on both axes.  Raises ValueError where pffft_hip_dct2d_new_setup
    returns NULL (a length no real setup of the precision takes, a kind or a norm out of range)."""

    _new, _destroy = "hip_dct2d_new_setup", "hip_dct2d_destroy_setup"

    def __init__(self, rows: int, cols: int, kind, norm=None, dtype=np.float32):
        self.rows, self.cols, self.dtype = int(rows), int(cols), np.dtype(dtype)
        self.kind = DCT_KINDS[kind] if kind in DCT_KINDS else int(kind)
        self.norm = DCT_NORMS[norm] if norm in DCT_NORMS else int(norm)
        self.image_scalars = self.rows * self.cols
        self._open(_pfx(dtype), self.rows, self.cols, self.kind, self.norm, shown=f"pffft_hip_dct2d_new_setup({rows}, {cols}, {kind}, {norm})")

    def route(self) -> str:
        """pffft_hip_dct2d_route: "fused" / "composed" under the calling thread's selector.  Host arithmetic only."""
        return self._L.pffft_hip_dct2d_route(self.handle).decode()

    def transform_batch(self, x, out=None):
        """x: contiguous CUDA tensor of the setup's dtype holding whole images (of any shape, such as [batch, rows, cols]).  out: None (a
        new tensor shaped like x), another such tensor, or x itself (in place)."""
        import torch
        batch = self._whole_rows(x, self.image_scalars)
        if out is None:
            out = torch.empty_like(x)
        assert self._whole_rows(out, self.image_scalars) == batch, "x and out hold different numbers of images"
        _check(self._fn("hip_dct2d_transform_batch")(self.handle, x.data_ptr(), out.data_ptr(), batch, self._stream()),
               "hip_dct2d_transform_batch")
        return out


BANDS_WHAT = {"energy": 0, "log": 1}   # PFFFT_HIP_BANDS_* of include/pffft_hip.h
BANDS_SEG = 16                          # PFFFT_HIP_BANDS_SEG


def _hz_to_mel(f, scale):
    f = np.asarray(f, dtype=np.float64)
    if scale == "htk":
        return 2595.0 * np.log10(1.0 + f / 700.0)
    # Slaney's Auditory Toolbox: linear below 1 kHz (200/3 Hz per mel), logarithmic above (27 steps per factor 6.4)
    lin = f / (200.0 / 3.0)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1000.0) / 1000.0) / (np.log(6.4) / 27.0), lin)


def _mel_to_hz(m, scale):
    m = np.asarray(m, dtype=np.float64)
    if scale == "htk":
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (np.maximum(m, 15.0) - 15.0)), (200.0 / 3.0) * m)


def mel_bank(N, nbands, fs, fmin=0.0, fmax=None, scale="htk", norm=None, dtype=np.float32):
    """A triangular mel filter bank over the N/2 + 1 bins of a real transform of N samples at the rate `fs`, for BandsSetup: returns
    (first, count, weights).  nbands + 2 edges are equally spaced on the mel scale ("htk": 2595 log10(1 + f / 700); "slaney": linear below
    1 kHz, logarithmic above) between fmin and fmax (None: fs / 2); band b rises from edge b to 1 at edge b + 1 and falls to 0 at edge
    b + 2, evaluated at the bin frequencies k fs / N.  norm = "slaney" divides band b by half its width in Hz (equal area).  The triangles
    are computed in float64 and rounded to `dtype`; first[b], count[b] span the non-zero support of band b (count 0 where no bin falls
    inside).  Host arithmetic only."""
    assert scale in ("htk", "slaney") and norm in (None, "slaney") and nbands >= 1 and N >= 2
    fmax = fs / 2.0 if fmax is None else float(fmax)
    assert 0.0 <= fmin < fmax <= fs / 2.0
    edges = _mel_to_hz(np.linspace(_hz_to_mel(fmin, scale), _hz_to_mel(fmax, scale), nbands + 2), scale)
    edges[0], edges[-1] = fmin, fmax                      # (exactly: a bin at fmin or fmax lies on the edge, outside the support)
    f = np.arange(N // 2 + 1, dtype=np.float64) * float(fs) / N
    first, count, weights = np.zeros(nbands, np.uint32), np.zeros(nbands, np.uint32), []
    for b in range(nbands):
        lo, c, hi = edges[b], edges[b + 1], edges[b + 2]
        tri = np.maximum(0.0, np.minimum((f - lo) / (c - lo), (hi - f) / (hi - c)))
        if norm == "slaney":
            tri = tri * (2.0 / (hi - lo))
        nz = np.nonzero(tri)[0]
        if nz.size:
            first[b], count[b] = nz[0], nz[-1] - nz[0] + 1
            weights.append(tri[nz[0]:nz[-1] + 1])
    w = np.concatenate(weights) if weights else np.zeros(0)
    return first, count, w.astype(dtype)


def bands_route(setup: "BandsSetup", hop, signal_stride=0) -> str:
    """pffft_hip_bands_route: "fused" / "composed" for a band-energy call with 16-byte aligned pointers, under the calling thread's
    selector.  Host arithmetic only."""
    return lib().pffft_hip_bands_route(setup.handle, int(hop), int(signal_stride)).decode()


class BandsSetup(_Handle):
    """PFFFT_HIP_Bands_Setup / PFFFTD_HIP_Bands_Setup: band energies (mel / Bark / octave bands, rebinned spectrograms) of the |X|^2 rows
    of framed transforms (include/pffft_hip.h).  first, count: nbands unsigned values; weights: sum(count) values, band after band (entry j
    of band b multiplies bin first[b] + j).  Raises ValueError where pffft_hip_bands_new_setup returns NULL (the text is in last_error())."""

    _new, _destroy = "hip_bands_new_setup", "hip_bands_destroy_setup"

    def __init__(self, N: int, first, count, weights, transform=REAL, dtype=np.float32):
        self.N, self.transform_type, self.dtype = int(N), int(transform), np.dtype(dtype)
        first = np.ascontiguousarray(first, dtype=np.uint32).ravel()
        count = np.ascontiguousarray(count, dtype=np.uint32).ravel()
        weights = np.ascontiguousarray(weights, dtype=self.dtype).ravel()
        assert first.size == count.size and weights.size == int(count.astype(np.uint64).sum()), "weights holds sum(count) values"
        self._open(_pfx(dtype), self.N, self.transform_type, first.size, first.ctypes.data, count.ctypes.data, weights.ctypes.data,
                   shown=f"pffft_hip_bands_new_setup({N}, {transform}, {first.size} bands)")

    @property
    def nbands(self) -> int:
        return int(self._L.pffft_hip_bands_count(self.handle))

    @property
    def bins(self) -> int:
        return int(self._L.pffft_hip_bands_bins(self.handle))

    # the framing arguments are those of Setup.frames_transform_batch
    _frames_rows, _spp, _analysis_in, _window_ptr = Setup._frames_rows, Setup._spp, Setup._analysis_in, Setup._window_ptr
    _rows_out = staticmethod(Setup._rows_out)

    def bands_batch(self, signal, hop, nframes=None, window=None, scaling=1.0, what="energy", floor=None, out=None):
        """pffft_hip_bands_batch: the band sums of the |X|^2 row of every frame of frames_transform_batch, in the documented order, times
        `scaling`; what = "log": log(max(., floor)), floor > 0 required.  Returns [nsignals,] nframes, nbands]; `out` may have padded rows
        (its stride(-2) is the row pitch)."""
        nsig, sstride, nframes = self._analysis_in(signal, hop, nframes, self.N)
        out, pitch = self._rows_out(out, signal, nsig, nframes, self.nbands, "row v = i nframes + f")
        w = BANDS_WHAT[what] if what in BANDS_WHAT else int(what)
        if floor is None:
            if w == BANDS_WHAT["log"]:
                raise ValueError("what = 'log' needs a floor > 0")
            floor = 0.0
        _check(self._fn("hip_bands_batch")(self.handle, signal.data_ptr(), sstride, nsig, nframes, hop, self._window_ptr(window, signal),
                                           float(scaling), float(floor), w, out.data_ptr(), pitch, self._stream()), "hip_bands_batch")
        return out


MDCT_WHAT = {"dct4": 0, "mdct": 1, "imdct": 2}      # `what` of pffft_hip_mdct_route


class MdctSetup(_Handle):
    """PFFFT_HIP_MdctSetup / PFFFTD_HIP_MdctSetup: MDCT / IMDCT frames of 2M samples at hop M (M coefficients per frame) and the type-IV
    cosine transform of rows of M reals (include/pffft_hip.h).  Raises ValueError where pffft_hip_mdct_new_setup returns NULL.  Every
    method takes CUDA tensors of the setup's dtype (and returns one), or numpy arrays, which go through the device (and return an array)."""

    _new, _destroy = "hip_mdct_new_setup", "hip_mdct_destroy_setup"

    def __init__(self, M: int, dtype=np.float32):
        self.M, self.dtype = int(M), np.dtype(dtype)
        self._open(_pfx(dtype), self.M, shown=f"pffft_hip_mdct_new_setup({M})")

    def route(self, what) -> str:
        """pffft_hip_mdct_route: "fused" / "composed" for what = 0 / "dct4", 1 / "mdct", 2 / "imdct" under the calling thread's selector
        ("" for another `what`).  Host arithmetic only."""
        return self._L.pffft_hip_mdct_route(self.handle, MDCT_WHAT[what] if what in MDCT_WHAT else int(what)).decode()

    def table(self, which: int, first: int = 0, count=None) -> np.ndarray:
        """pffft_hip_mdct_table: a_m (which = 0) or b_k (which = 1), M/2 values each, as a complex array of the setup's precision (host
        arithmetic only)."""
        if count is None:
            count = self.M // 2 - first
        return self._complex_table("pffft_hip_mdct_table", int(which), int(first), int(count), count=count)

    def _dev(self, x):
        """(CUDA tensor of x, x was a numpy array)"""
        import torch
        if x is None:
            return None, False
        if _is_torch(x):
            assert x.is_cuda and x.dtype == self._torch_dtype(), "need a CUDA tensor of the setup dtype"
            return x, False
        return torch.from_numpy(np.ascontiguousarray(x, dtype=self.dtype)).cuda(), True

    def dct4(self, rows, out=None):
        """rows: `rows` x M scalars, contiguous; the result (2 C4(rows): scipy.fft.dct(type=4)) has the same shape.  out may be rows."""
        import torch
        x, host = self._dev(rows)
        assert x.is_contiguous() and x.numel() % self.M == 0, "need contiguous whole rows"
        if out is None:
            out = torch.empty_like(x)
        assert out.is_cuda and out.dtype == x.dtype and out.is_contiguous() and out.numel() == x.numel()
        _check(self._fn("hip_mdct_dct4_batch")(self.handle, x.data_ptr(), out.data_ptr(), x.numel() // self.M, self._stream()), "hip_mdct_dct4_batch")
        return out.cpu().numpy() if host else out

    def mdct(self, signal, window=None, nframes=None, out=None):
        """signal: [(nframes + 1) M] or [nsignals, >= (nframes + 1) M] with unit stride along the samples (rows may be pitched); window:
        2M values or None.  nframes defaults to what the samples hold.  Returns coefficients [nsignals, nframes, M] (out: the same shape, rows may be pitched)."""
        import torch
        x, host = self._dev(signal)
        w, _ = self._dev(window)
        one = x.dim() == 1
        if one:
            x = x.unsqueeze(0)
        assert x.dim() == 2 and x.stride(1) == 1, "need samples with unit stride"
        nsig = x.shape[0]
        if nframes is None:
            nframes = x.shape[1] // self.M - 1
        nframes = int(nframes)
        assert nframes >= 0 and x.shape[1] >= (nframes + 1) * self.M, "a signal holds (nframes + 1) M samples"
        assert w is None or (w.is_contiguous() and w.numel() == 2 * self.M), "the window has 2M values"
        if out is None:
            out = torch.empty((nsig, nframes, self.M), dtype=x.dtype, device=x.device)
        o3 = out.unsqueeze(0) if out.dim() == 2 else out
        assert o3.is_cuda and o3.dtype == x.dtype and tuple(o3.shape) == (nsig, nframes, self.M) and o3.stride(2) == 1
        cstride = o3.stride(1) if nframes > 1 else self.M
        assert nsig == 1 or o3.stride(0) == nframes * cstride, "rows at one pitch"
        _check(self._fn("hip_mdct_transform_batch")(self.handle, x.data_ptr(), x.stride(0) if nsig > 1 else 0, nsig, nframes, w.data_ptr() if w is not None else None,
                  o3.data_ptr(), cstride, self._stream()), "hip_mdct_transform_batch")
        res = o3[0] if one else o3
        return res.cpu().numpy() if host else res

    def imdct(self, coefs, window=None, scaling=1.0, out=None):
        """coefs: [nframes, M] or [nsignals, nframes, M], unit stride along a row (rows may be pitched).  Returns the overlap-added signals
        [nsignals, (nframes + 1) M] (out: rows may be pitched); scaling = 2 / M with a Princen-Bradley window reconstructs the interior."""
        import torch
        X, host = self._dev(coefs)
        w, _ = self._dev(window)
        one = X.dim() == 2
        if one:
            X = X.unsqueeze(0)
        assert X.dim() == 3 and X.shape[2] == self.M and X.stride(2) == 1, "need rows of M coefficients with unit stride"
        nsig, nframes = X.shape[0], X.shape[1]
        cstride = X.stride(1) if nframes > 1 else self.M
        assert nsig == 1 or X.stride(0) == nframes * cstride, "rows at one pitch"
        assert w is None or (w.is_contiguous() and w.numel() == 2 * self.M), "the window has 2M values"
        samples = (nframes + 1) * self.M
        if out is None:
            out = torch.empty((nsig, samples), dtype=X.dtype, device=X.device)
        o2 = out.unsqueeze(0) if out.dim() == 1 else out
        assert o2.is_cuda and o2.dtype == X.dtype and o2.dim() == 2 and o2.shape[0] == nsig and o2.shape[1] >= samples and o2.stride(1) == 1
        _check(self._fn("hip_mdct_overlap_add_batch")(self.handle, X.data_ptr(), cstride, nsig, nframes, w.data_ptr() if w is not None else None, float(scaling),
                  o2.data_ptr(), o2.stride(0) if nsig > 1 else 0, self._stream()), "hip_mdct_overlap_add_batch")
        res = o2[0, :samples] if one else o2[:, :samples]
        return res.cpu().numpy() if host else res


class FastConv(_Handle):
    """PFFASTCONV_Setup (src/pffastconv.c:58-116); `block_len` is updated like *blockLen."""

    _new, _destroy = "new_setup", "destroy_setup"

    def __init__(self, taps, block_len: int = 0, flags: int = 0):
        h = _aligned(taps, np.float32)
        self.filter_len = h.size
        bl = C.c_int(block_len)
        self._open("pffastconv", h.ctypes.data, h.size, C.byref(bl), flags, shown="pffastconv_new_setup")
        self.block_len, self.flags = bl.value, flags

    def route(self, L, nsig=1, flush=True, cus=0):
        """pffastconv_hip_route: (kernel, cfg, block, step, blocks, last) of an apply_batch call of nsig signals of L samples under the calling
        thread's selector - the kernel's short name (None: the call launches nothing), its configuration, the internal block length, its
        valid samples, the blocks per signal and the last block's outputs.  Host arithmetic only; cus > 0 stands for the device's compute
        units, so that no device is touched."""
        buf = C.create_string_buffer(128)
        if self._L.pffastconv_hip_route(self.handle, int(L), int(nsig), int(bool(flush)), int(cus), buf, len(buf)) < 0:
            raise RuntimeError("pffastconv_hip_route failed")
        f = buf.value.decode().split(" ")
        return (f[0], f[1]) + tuple(int(v) for v in f[2:]) if f[0] else (None, "", 0, 0, 0, 0)

    def apply(self, x, flush: bool = True, out=None):
        """Returns (y[:n_out], n_out) like pffastconv_apply (src/pffastconv.c:133-263)."""
        cpl = 2 if (self.flags & 1) else 1
        if _is_torch(x):
            import torch
            assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
            n_in = x.numel() // cpl
            y = out if out is not None else torch.empty_like(x)
            n = self._L.pffastconv_hip_apply_device(self.handle, x.data_ptr(), n_in, y.data_ptr(), int(bool(flush)), self._stream())
            if n < 0:
                raise RuntimeError("pffastconv_hip_apply_device failed: " + self._L.pffft_hip_last_error().decode())
            return y[:n * cpl], n
        xin = _aligned(x, np.float32)
        n_in = xin.size // cpl
        y = _aligned_empty(max(xin.size, 1), np.float32)
        n = self._L.pffastconv_apply(self.handle, xin.ctypes.data, n_in, y.ctypes.data, int(bool(flush)))
        if n < 0:   # the drop-in's failure value (include/pffft_hip.h): the C entry has already failed soft, the mirror returns it as is
            return y[:0].copy(), n
        return y[:n * cpl].copy(), n

    def apply_batch(self, x, flush: bool = True, out=None):
        """pffastconv_hip_apply_batch: x is a [nsignals, floats-per-signal] CUDA tensor of independent signals; every row
        is filtered exactly as apply() would.  Returns (y[:, :n_out*cpl], n_out); n_out is per signal."""
        import torch
        cpl = 2 if (self.flags & 1) else 1
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.stride(1) == 1
        nsig, fl = x.shape
        y = out if out is not None else torch.empty_like(x)
        assert y.dim() == 2 and y.shape[0] == nsig and y.stride(1) == 1
        n = self._L.pffastconv_hip_apply_batch(self.handle, x.data_ptr(), fl // cpl, x.stride(0) if nsig > 1 else fl,
                                               y.data_ptr(), y.stride(0) if nsig > 1 else fl, nsig, int(bool(flush)), self._stream())
        if n < 0:
            raise RuntimeError("pffastconv_hip_apply_batch failed: " + self._L.pffft_hip_last_error().decode())
        return y[:, :n * cpl], n
