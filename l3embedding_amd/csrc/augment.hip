// augment.hip -- training-set augmentation of 02_generate_samples.py --augment, in the pass that scales a stored batch.
//
// Reference semantics restated (paths relative to the reference tree):
//   crop                 data/avc/sample.py:169-193   frame[start_x : start_x + 224, start_y : start_y + 224]
//   flip                 data/avc/sample.py:59-69     frame[:, ::-1]
//   img_as_float         data/avc/sample.py:237       u8 / 255
//   adjust_brightness    data/avc/sample.py:41-56     clip(x + delta, 0, 1)
//   adjust_saturation    data/avc/sample.py:24-38     rgb2hsv, S = clip(S * factor, 0, 1), hsv2rgb
//   order of the two     data/avc/sample.py:252-273
//   img_as_ubyte         data/avc/sample.py:281       clip(rint(x * 255), 0, 255), rint = half to even
//   audio gain           data/avc/sample.py:146-162   gain = 1 + uniform(-0.1, min(0.1, 32768 / peak - 1)), x * gain in float64,
//                                                     astype(int16) = truncation towards zero
//
// Arithmetic.  The frame is processed in float64 along skimage's own sequence of operations (hue, sector, the p / q / t blends of
// hsv2rgb), not in the closed form c = V - (V - c0) * min(factor, V / (V - min)) that follows from hue and value being unchanged.
// The closed form is exact algebra, but with factor 0.5 (and every factor on two-level images) x * 255 lands on k + 1/2 for a large
// share of the values, and which way such a tie falls is decided by the LAST BITS of the float64 original: an fp32 closed form
// disagreed with it on 5 % of the values of a uniform random frame at factor 0.5 (one level each), far outside the 1e-4 the tests
// allow.  Following the original's operations in its own precision, without fused multiply-adds, reproduces its bytes exactly, and
// the kernel stays bound by its 48 MB of HBM traffic per 64 frames, not by the ~150 float64 operations per pixel.
//
// Audio: no deviation either.  The bound 32768 / peak on the gain keeps every product inside int16 except one: a row whose peak is
// +32767 with a draw so close to 1 that the gain rounds to 32768 / 32767 gives 32767 * gain == 32768.0, which numpy's astype(int16)
// wraps to -32768 (double -> int32 -> low 16 bits on the reference's x86 hosts).  The kernel converts the same way, so that it is
// bit-exact on that row too; |x * gain| <= 1.1 * 32768 always fits the int32.
#include "kernels.h"

// every float64 operation below is rounded on its own, as numpy rounds it
#pragma clang fp contract(off)

namespace l3 {

namespace {

constexpr int VID_PX = 4;                                              // pixels per thread: 12 bytes = 3 dwords in, 3 dwords or 3 float4 out
constexpr int VID_GROUPS_ROW = AUG_CROP / VID_PX;                      // 56
constexpr int VID_GROUPS = AUG_CROP * VID_GROUPS_ROW;                  // 12544 per sample
constexpr int VID_BLOCK = 256;
constexpr int VID_BLOCKS_SAMPLE = VID_GROUPS / VID_BLOCK;              // 49: a block never straddles two samples
static_assert(VID_GROUPS % VID_BLOCK == 0, "one parameter record per block");

__device__ __forceinline__ double clip01(double x) { return fmin(fmax(x, 0.0), 1.0); }

// adjust_saturation (sample.py:24-38): skimage's rgb2hsv, S = clip(S * factor, 0, 1), hsv2rgb, operation by operation
__device__ __forceinline__ void saturate_px(double& r, double& g, double& b, double factor) {
    const double v = fmax(r, fmax(g, b)), delta = v - fmin(r, fmin(g, b));
    if (delta == 0.0) return;          // a grey: S = 0 and H = 0, hsv2rgb returns (V, V, V)
    double h = (g - b) / delta;        // the channel that holds the maximum picks the formula; blue wins over green over red
    if (g == v) h = 2.0 + (b - r) / delta;
    if (b == v) h = 4.0 + (r - g) / delta;
    h = h / 6.0;
    if (h < 0.0) h = h + 1.0;          // (h / 6) % 1 of a value in (-1/6, 5/6]
    const double s = clip01((delta / v) * factor);
    const double h6 = h * 6.0, hi = floor(h6), f = h6 - hi;
    const double p = v * (1.0 - s), q = v * (1.0 - f * s), t = v * (1.0 - (1.0 - f) * s);
    switch ((unsigned)hi % 6u) {
        case 0: r = v; g = t; b = p; break;
        case 1: r = q; g = v; b = p; break;
        case 2: r = p; g = v; b = t; break;
        case 3: r = p; g = q; b = v; break;
        case 4: r = t; g = p; b = v; break;
        default: r = v; g = p; b = q; break;
    }
}

// one pixel, img_as_float values in, img_as_ubyte levels out
__device__ __forceinline__ void augment_px(double r, double g, double b, int sat_first, double factor, double delta, uint32_t q[3]) {
    if (sat_first) saturate_px(r, g, b, factor);
    r = clip01(r + delta);
    g = clip01(g + delta);
    b = clip01(b + delta);
    if (!sat_first) saturate_px(r, g, b, factor);
    q[0] = (uint32_t)fmin(fmax(rint(r * 255.0), 0.0), 255.0);
    q[1] = (uint32_t)fmin(fmax(rint(g * 255.0), 0.0), 255.0);
    q[2] = (uint32_t)fmin(fmax(rint(b * 255.0), 0.0), 255.0);
}

struct Dwords3 {
    uint32_t a, b, c;
};

// grid = N * 49 blocks of 256 threads; thread = 4 neighbouring output pixels of one row
__global__ __launch_bounds__(VID_BLOCK) void augment_video_kernel(const uint8_t* __restrict__ in, int64_t in_bytes, int H, int W,
                                                                  const AugmentParams* __restrict__ params,
                                                                  Dwords3* __restrict__ out_u8, float4* __restrict__ out_f32) {
    // byte -> value at both ends, one entry per thread: img_as_float's u8 / 255 and the engine's scaling of a stored byte, the
    // expression of preprocess_video_kernel (train.py:186) -- their float64 divisions once per block, not once per value
    __shared__ double lut_in[256];
    __shared__ float lut_out[256];
    const int t = threadIdx.x;
    lut_in[t] = (double)t / 255.0;
    {
        const float f = (float)((double)t / 255.0);
        lut_out[t] = 2.f * f - 1.f;
    }
    __syncthreads();
    const int n = blockIdx.x / VID_BLOCKS_SAMPLE;
    const AugmentParams p = params[n];
    const int grp = (blockIdx.x - n * VID_BLOCKS_SAMPLE) * VID_BLOCK + t;
    const int row = grp / VID_GROUPS_ROW, g4 = grp - row * VID_GROUPS_ROW;
    // source columns of the group: mirrored, the group at the other end of the row in reverse pixel order
    const int col0 = p.start_y + (p.flip ? AUG_CROP - VID_PX - g4 * VID_PX : g4 * VID_PX);
    const int64_t a = (((int64_t)n * H + (p.start_x + row)) * W + col0) * 3;
    const int64_t a0 = a & ~(int64_t)3;
    const int sh = (int)(a & 3) * 8;
    uint32_t d[4];
#pragma unroll
    for (int i = 0; i < 3; ++i) d[i] = *reinterpret_cast<const uint32_t*>(in + a0 + 4 * i);
    d[3] = 0;
    if (sh != 0) {          // the twelve bytes straddle four dwords; the last of them may be cut short by the end of the buffer
        if (a0 + 16 <= in_bytes) {
            d[3] = *reinterpret_cast<const uint32_t*>(in + a0 + 12);
        } else {
            for (int k = 0; k < 4; ++k)
                if (a0 + 12 + k < in_bytes) d[3] |= (uint32_t)in[a0 + 12 + k] << (8 * k);
        }
    }
    uint32_t w[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] = (uint32_t)((((uint64_t)d[i + 1] << 32) | d[i]) >> sh);
    double x[12];
#pragma unroll
    for (int byte = 0; byte < 12; ++byte) x[byte] = lut_in[(w[byte >> 2] >> ((byte & 3) * 8)) & 0xffu];
    uint32_t ob[3] = {0u, 0u, 0u};
    float of[12];
#pragma unroll
    for (int j = 0; j < VID_PX; ++j) {
        const int mj = VID_PX - 1 - j;
        double c[3];
        uint32_t q[3];
#pragma unroll
        for (int e = 0; e < 3; ++e) c[e] = p.flip ? x[mj * 3 + e] : x[j * 3 + e];
        augment_px(c[0], c[1], c[2], p.sat_first, (double)p.saturation, (double)p.brightness, q);
#pragma unroll
        for (int e = 0; e < 3; ++e) {
            const uint32_t level = q[e];
            const int byte = j * 3 + e;
            ob[byte >> 2] |= level << ((byte & 3) * 8);
            of[byte] = lut_out[level];
        }
    }
    const int64_t o = (int64_t)n * VID_GROUPS + grp;
    if (out_u8 != nullptr) out_u8[o] = Dwords3{ob[0], ob[1], ob[2]};
    if (out_f32 != nullptr) {
#pragma unroll
        for (int i = 0; i < 3; ++i) out_f32[o * 3 + i] = make_float4(of[4 * i], of[4 * i + 1], of[4 * i + 2], of[4 * i + 3]);
    }
}

constexpr int AUD_BLOCK = 512;
constexpr int AUD_SLICES = 4;          // blocks per row: each finds the row's peak (the row comes from L2 after the first) and writes a quarter

__device__ __forceinline__ int abs_pair_max(uint32_t w, int m) {
    const int lo = (int)(int16_t)(w & 0xffffu), hi = (int)w >> 16;
    return max(m, max(abs(lo), abs(hi)));
}

// random.uniform(-0.1, max_gain) = a + (b - a) * u in float64, each operation rounded on its own (no fused multiply-add)
__device__ __forceinline__ double gain_of(int peak, double u) {
    double max_gain = 0.1;
    if (peak > 0) {
        const double m = __dsub_rn(__ddiv_rn(32768.0, (double)peak), 1.0);
        max_gain = m < 0.1 ? m : 0.1;
    }
    return __dadd_rn(1.0, __dadd_rn(-0.1, __dmul_rn(__dadd_rn(max_gain, 0.1), u)));
}

__device__ __forceinline__ int apply_gain(int x, double gain) {
    const double y = __dmul_rn((double)x, gain);
    return (int)(int16_t)(int)y;          // truncation towards zero, then the low 16 bits: astype(int16)
}

// grid = N * AUD_SLICES blocks; vec = 1: T % 8 == 0 and 16-byte aligned bases, the rows go through 16-byte loads and stores
__global__ __launch_bounds__(AUD_BLOCK) void augment_audio_kernel(const int16_t* __restrict__ pcm, int T, const double* __restrict__ u,
                                                                  int16_t* __restrict__ out_i16, float* __restrict__ out_f32,
                                                                  double* __restrict__ gains, int vec) {
    __shared__ int wave_max[AUD_BLOCK / 64];
    const int t = threadIdx.x;
    const int row = blockIdx.x / AUD_SLICES, slice = blockIdx.x - row * AUD_SLICES;
    const int16_t* x = pcm + (int64_t)row * T;
    int m = 0;
    if (vec) {
        const uint4* x8 = reinterpret_cast<const uint4*>(x);
        for (int i = t; i < T / 8; i += AUD_BLOCK) {
            const uint4 v = x8[i];
            m = abs_pair_max(v.x, m);
            m = abs_pair_max(v.y, m);
            m = abs_pair_max(v.z, m);
            m = abs_pair_max(v.w, m);
        }
    } else {
        for (int i = t; i < T; i += AUD_BLOCK) m = max(m, abs((int)x[i]));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
    if ((t & 63) == 0) wave_max[t >> 6] = m;
    __syncthreads();
    int peak = 0;
#pragma unroll
    for (int k = 0; k < AUD_BLOCK / 64; ++k) peak = max(peak, wave_max[k]);
    const double gain = gain_of(peak, u[row]);
    if (slice == 0 && t == 0) gains[row] = gain;
    const int64_t ob = (int64_t)row * T;
    if (vec) {
        const int n8 = T / 8;
        const int i0 = (int)((int64_t)n8 * slice / AUD_SLICES), i1 = (int)((int64_t)n8 * (slice + 1) / AUD_SLICES);
        const uint4* x8 = reinterpret_cast<const uint4*>(x);
        for (int i = i0 + t; i < i1; i += AUD_BLOCK) {
            const uint4 v = x8[i];
            const uint32_t wv[4] = {v.x, v.y, v.z, v.w};
            uint32_t qw[4];
            float f[8];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int lo = apply_gain((int)(int16_t)(wv[k] & 0xffffu), gain), hi = apply_gain((int)wv[k] >> 16, gain);
                qw[k] = ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16);
                f[2 * k] = (float)lo / 32768.f;          // preprocess_audio_kernel's expression (audio.py:28-31)
                f[2 * k + 1] = (float)hi / 32768.f;
            }
            if (out_i16 != nullptr) reinterpret_cast<uint4*>(out_i16 + ob)[i] = make_uint4(qw[0], qw[1], qw[2], qw[3]);
            if (out_f32 != nullptr) {
                float4* o4 = reinterpret_cast<float4*>(out_f32 + ob) + 2 * (int64_t)i;
                o4[0] = make_float4(f[0], f[1], f[2], f[3]);
                o4[1] = make_float4(f[4], f[5], f[6], f[7]);
            }
        }
    } else {
        const int i0 = (int)((int64_t)T * slice / AUD_SLICES), i1 = (int)((int64_t)T * (slice + 1) / AUD_SLICES);
        for (int i = i0 + t; i < i1; i += AUD_BLOCK) {
            const int q = apply_gain((int)x[i], gain);
            if (out_i16 != nullptr) out_i16[ob + i] = (int16_t)q;
            if (out_f32 != nullptr) out_f32[ob + i] = (float)q / 32768.f;
        }
    }
}

inline bool aligned16(const void* p) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

void augment_video(const uint8_t* u8, int N, int H, int W, const AugmentParams* params, uint8_t* out_u8, float* out_f32,
                   hipStream_t s) {
    if (N <= 0) return;
    hipLaunchKernelGGL(augment_video_kernel, dim3(N * VID_BLOCKS_SAMPLE), dim3(VID_BLOCK), 0, s, u8, (int64_t)N * H * W * 3, H, W,
                       params, reinterpret_cast<Dwords3*>(out_u8), reinterpret_cast<float4*>(out_f32));
}

void augment_audio(const int16_t* pcm, int N, int T, const double* u, int16_t* out_i16, float* out_f32, double* gains,
                   hipStream_t s) {
    if (N <= 0 || T <= 0) return;
    const int vec = T % 8 == 0 && aligned16(pcm) && aligned16(out_i16) && aligned16(out_f32);
    hipLaunchKernelGGL(augment_audio_kernel, dim3(N * AUD_SLICES), dim3(AUD_BLOCK), 0, s, pcm, T, u, out_i16, out_f32, gains, vec);
}

}  // namespace l3
