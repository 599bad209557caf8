// The four instantiations of k_conv_f32 that sd_yolo_api.hip launches, alone in one translation unit: tests/test_conv_f32_resources.py
// compiles it for gfx950 with -Rpass-analysis=kernel-resource-usage and reads registers, scratch, spills and occupancy from the remarks.
#include <hip/hip_runtime.h>
#include "k_yolo32.h"

template __global__ void k_conv_f32<16, 2, 2, 4>(SdConvArgsF);
template __global__ void k_conv_f32<16, 1, 2, 4>(SdConvArgsF);
template __global__ void k_conv_f32<16, 1, 1, 4>(SdConvArgsF);
template __global__ void k_conv_f32<8, 1, 1, 8>(SdConvArgsF);
