// clips.hip -- the 1-second frames of whole clips, cut on the GPU.
//
// Replaces (reference call sites, relative to the reference tree):
//   get_l3_frames_uniform's padding + librosa.util.frame   data/usc/features.py:276-300
// The framing rule itself lives in l3embedding_amd/features.py (frame_table); the kernel only follows its table:
// one row of three int64 per frame, (start, lo, hi), and output sample j of the frame is samples[start + j] when
// lo <= start + j < hi, else 0.  Every frame is thereby padded on its own (the front-end's STFT padding never sees a
// neighbouring second of the clip), and offsets are int64 because a long clip passes 2^31 samples.
#include "kernels.h"

namespace l3 {

// One thread per 4 consecutive output samples: a 16-byte store (rows are T floats, T % 4 == 0, the engine's input buffer is
// hipMalloc-aligned) from four dword loads (the source offset start + 4q has no alignment: any hop, any clip offset).  Grid
// (row quads / 256, rows): the row's table entry is wave-uniform (scalar loads).  Rows >= n_real are written as zeros.
__global__ __launch_bounds__(256) void gather_frames_kernel(const float* __restrict__ samples, const int64_t* __restrict__ table,
                                                            float* __restrict__ out, int n_real, int T) {
    const int row = blockIdx.y;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (4 * q >= T) return;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (row < n_real) {
        const int64_t start = table[3 * (int64_t)row], lo = table[3 * (int64_t)row + 1], hi = table[3 * (int64_t)row + 2];
        const int64_t i0 = start + 4 * (int64_t)q;
        if (i0 >= lo && i0 + 4 <= hi) {
            v.x = samples[i0];
            v.y = samples[i0 + 1];
            v.z = samples[i0 + 2];
            v.w = samples[i0 + 3];
        } else {
            if (i0 >= lo && i0 < hi) v.x = samples[i0];
            if (i0 + 1 >= lo && i0 + 1 < hi) v.y = samples[i0 + 1];
            if (i0 + 2 >= lo && i0 + 2 < hi) v.z = samples[i0 + 2];
            if (i0 + 3 >= lo && i0 + 3 < hi) v.w = samples[i0 + 3];
        }
    }
    *reinterpret_cast<float4*>(out + (size_t)row * T + 4 * q) = v;
}

void gather_frames(const float* samples, const int64_t* table, float* out, int rows, int n_real, int T, hipStream_t s) {
    const int quads = T / 4;
    const int bx = (quads + 255) / 256;
    for (int r0 = 0; r0 < rows; r0 += 65535) {          // gridDim.y limit
        const int nr = rows - r0 < 65535 ? rows - r0 : 65535;
        const int real = n_real - r0 < 0 ? 0 : n_real - r0;
        hipLaunchKernelGGL(gather_frames_kernel, dim3(bx, nr), dim3(256), 0, s, samples, table + 3 * (int64_t)r0,
                           out + (size_t)r0 * T, real, T);
    }
}

}  // namespace l3
