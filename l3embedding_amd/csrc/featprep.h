// featprep.h -- the l3_feat handle of featprep.hip (include/l3hip.h, "Fold preprocessing"): one float32 (n, D) row-major matrix on one
// device.  mlp.hip reads it for the device-to-device hand-off of l3_mlp_set_data_dev / l3_mlp_predict_dev.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "host_common.h"

struct l3_feat {
    int device = 0;
    int64_t n = 0, D = 0;
    float* x = nullptr;
    hipStream_t s = nullptr;
    l3::DeviceBufs bufs;
};
