// What the units of the cosine / sine transforms share on the host: dct_tu.hip owns the 1-D handle type and defines, dct2d_tu.hip (which
// owns 1-D handles and runs a fused kernel on their tables) calls.
#pragma once
#include <hip/hip_runtime.h>

#include "cxmath.h"

namespace pf {

// t_k, k = 0 ... N/2, of a FLOAT 1-D dct handle (pffft_hip_dct_new_setup) on the calling thread's device: the table the 1-D routes
// multiply by, built at the first use on a device like theirs (not during a capture: hipErrorStreamCaptureUnsupported).  0, or the
// error with its text set; hipErrorInvalidHandle for anything that is no float dct handle.
int dct_device_table(void* dct_setup, hipStream_t st, const cx<float>** tab);

}  // namespace pf
