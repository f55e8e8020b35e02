// frames.hip -- 224 x 224 x 3 network inputs from raw uint8 frames of any size, resized and cropped on the GPU.
//
// Replaces (reference call sites, relative to the reference tree):
//   read_video's resize to a shorter side of 256       data/avc/sample.py:286-316 (ffmpeg's scaler there: DESIGN.md section 8n)
//   the 224 x 224 crop                                 data/avc/sample.py:169-193
//   2 * img_as_float(u8) - 1                           l3embedding/train.py:186 (preprocess_video_kernel's expression)
// The rule of where to resize to and where to crop lives in l3embedding_amd/features.py (image_table); the kernel follows its
// table: one row of IMAGE_ROW int64 per output frame, {offset, H, W, Ho, Wo, y0, x0}.  Rows [y0, y0 + 224) x [x0, x0 + 224) of the
// H x W frame at pixels[offset ..) resized to Ho x Wo become one row of the engine's video batch; only that window is computed.
//
// The resize is bilinear with half-pixel centres, the tent widened by the scale when shrinking (PIL's, and
// torch.nn.functional.interpolate(mode='bilinear', antialias=True, align_corners=False)'s definition).  Per axis, r = n_in / n_out
// and s = max(r, 1) in float64; output i has the centre c = r * (i + 0.5), the taps j in [lo, hi) with lo = max(0, (int)(c - s + 0.5))
// and hi = min(n_in, (int)(c + s + 0.5)), raw weights t_j = max(0, 1 - |(j - c + 0.5) / s|) and weights t_j / sum t_j (ascending j).
// The contract is an order of float64 operations (this file is compiled with -ffp-contract=off): horizontal sums first, ascending
// j, multiply then add; then vertical, ascending k; u = clamp(floor(v + 0.5), 0, 255); out = 2.f * (float)((double)u / 255.0) - 1.f.
// tests/image_ref.py restates it in NumPy and the kernel's uint8 and float32 values equal it exactly.
//
// The weights are worked out on the host (image_plan, the same IEEE operations in the same order), once per distinct
// (n_in, n_out, first output) of a call, and uploaded: per axis table IMG words lo, IMG words count, then the float64 weights.
#include <cmath>
#include <cstring>
#include <map>
#include <tuple>

#include "kernels.h"

namespace l3 {

const char* image_table_error(const int64_t* table, int64_t n_frames, int64_t n_bytes, int64_t* bad_row) {
    for (int64_t f = 0; f < n_frames; ++f) {
        const int64_t* t = table + IMAGE_ROW * f;
        const int64_t off = t[0], H = t[1], W = t[2], Ho = t[3], Wo = t[4], y0 = t[5], x0 = t[6];
        *bad_row = f;
        if (H < 1 || H > IMAGE_MAX_SIDE || W < 1 || W > IMAGE_MAX_SIDE) return "H and W must be in [1, 8192]";
        if (Ho < IMG || Ho > IMAGE_MAX_SIDE || Wo < IMG || Wo > IMAGE_MAX_SIDE) return "Ho and Wo must be in [224, 8192]";
        if (y0 < 0 || y0 > Ho - IMG || x0 < 0 || x0 > Wo - IMG) return "the 224 x 224 crop is outside Ho x Wo";
        if (off < 0) return "offset < 0";
        if (n_bytes < 3 * H * W || off > n_bytes - 3 * H * W) return "offset + 3 * H * W > n_bytes";
    }
    return nullptr;
}

// One axis: outputs [first, first + IMG) of n_in -> n_out, appended to `words`.  Weights lie tap-major, w[j * IMG + i], as many
// taps as the widest output has, so that a wavefront's loads of one tap are consecutive.
static void axis_taps(int64_t n_in, int64_t n_out, int64_t first, std::vector<int64_t>* words) {
    const double r = (double)n_in / (double)n_out;
    const double s = r > 1.0 ? r : 1.0;
    int lo[IMG], cnt[IMG];
    int64_t stride = 0;
    for (int i = 0; i < IMG; ++i) {
        const double c = r * ((double)(first + i) + 0.5);
        const int64_t a = (int64_t)(c - s + 0.5), b = (int64_t)(c + s + 0.5);
        lo[i] = (int)(a > 0 ? a : 0);
        cnt[i] = (int)((b < n_in ? b : n_in) - lo[i]);
        if (cnt[i] > stride) stride = cnt[i];
    }
    const size_t base = words->size();
    words->resize(base + 2 * IMG + (size_t)stride * IMG, 0);
    int64_t* w = words->data() + base;
    for (int i = 0; i < IMG; ++i) {
        w[i] = lo[i];
        w[IMG + i] = cnt[i];
        const double c = r * ((double)(first + i) + 0.5);
        double sum = 0.0;
        for (int k = 0; k < cnt[i]; ++k) {
            const double t = 1.0 - std::fabs(((double)(lo[i] + k) - c + 0.5) / s);
            sum += t > 0.0 ? t : 0.0;
        }
        for (int k = 0; k < cnt[i]; ++k) {
            const double t = 1.0 - std::fabs(((double)(lo[i] + k) - c + 0.5) / s);
            const double wk = (t > 0.0 ? t : 0.0) / sum;
            memcpy(&w[2 * IMG + (size_t)k * IMG + i], &wk, 8);
        }
    }
}

void image_plan(const int64_t* table, int64_t n_frames, ImagePlan* plan) {
    plan->frames.assign((size_t)n_frames * IMAGE_DESC, 0);
    plan->taps.clear();
    std::map<std::tuple<int64_t, int64_t, int64_t>, int64_t> seen;          // -> the table's first word
    auto axis = [&](int64_t n_in, int64_t n_out, int64_t first) {
        const auto key = std::make_tuple(n_in, n_out, first);
        auto it = seen.find(key);
        if (it == seen.end()) {
            it = seen.emplace(key, (int64_t)plan->taps.size()).first;
            axis_taps(n_in, n_out, first, &plan->taps);
        }
        return it->second;
    };
    for (int64_t f = 0; f < n_frames; ++f) {
        const int64_t* t = table + IMAGE_ROW * f;
        int64_t* d = plan->frames.data() + IMAGE_DESC * f;
        const auto x = axis(t[2], t[4], t[6]), y = axis(t[1], t[3], t[5]);
        d[0] = t[0], d[1] = t[2], d[2] = x, d[3] = y;
    }
}

// A workgroup takes one frame and a band of IMAGE_BAND output rows; thread x owns output column x, its three channels.  It walks
// the source rows the band reads in ascending order, forms each row's three horizontal sums once and adds them into the
// accumulators of the output rows that source row feeds (their tap ranges move monotonically with the output row, so the rows
// between the first row's lo and the last row's hi are all the band reads): the contract's vertical order, no row held in LDS.
// The band's own tap ranges and weights are uniform over the workgroup.  Pixel loads are single bytes (any offset).
constexpr int IMAGE_BAND = 8;
static_assert(IMG % IMAGE_BAND == 0, "whole bands");

__global__ __launch_bounds__(256) void image_frames_kernel(const uint8_t* __restrict__ pixels, const int64_t* __restrict__ frames,
                                                           const int64_t* __restrict__ taps, uint8_t* __restrict__ out_u8,
                                                           float* __restrict__ out_f32, int n_real) {
    const int f = blockIdx.y, oy0 = blockIdx.x * IMAGE_BAND, x = threadIdx.x;
    if (x >= IMG) return;
    const size_t o0 = (((size_t)f * IMG + oy0) * IMG + x) * 3;
    if (f >= n_real) {
#pragma unroll
        for (int r = 0; r < IMAGE_BAND; ++r)
            for (int ch = 0; ch < 3; ++ch) {
                if (out_u8) out_u8[o0 + (size_t)r * IMG * 3 + ch] = 0;
                if (out_f32) out_f32[o0 + (size_t)r * IMG * 3 + ch] = 0.f;
            }
        return;
    }
    const int64_t* d = frames + (int64_t)IMAGE_DESC * f;
    const int64_t off = d[0], W = d[1];
    const int64_t* xt = taps + d[2];
    const int64_t* yt = taps + d[3];
    const int xlo = (int)xt[x], xcnt = (int)xt[IMG + x];
    const double* wx = reinterpret_cast<const double*>(xt + 2 * IMG) + x;
    const double* wy = reinterpret_cast<const double*>(yt + 2 * IMG) + oy0;
    int ylo[IMAGE_BAND], ycnt[IMAGE_BAND];
#pragma unroll
    for (int r = 0; r < IMAGE_BAND; ++r) {
        ylo[r] = (int)yt[oy0 + r];
        ycnt[r] = (int)yt[IMG + oy0 + r];
    }
    double acc[IMAGE_BAND][3];
#pragma unroll
    for (int r = 0; r < IMAGE_BAND; ++r) acc[r][0] = acc[r][1] = acc[r][2] = 0.0;
    const int y_end = ylo[IMAGE_BAND - 1] + ycnt[IMAGE_BAND - 1];
    for (int y = ylo[0]; y < y_end; ++y) {
        const uint8_t* p = pixels + off + ((int64_t)y * W + xlo) * 3;
        double h0 = 0.0, h1 = 0.0, h2 = 0.0;
        for (int j = 0; j < xcnt; ++j) {
            const double w = wx[(size_t)j * IMG];
            h0 += w * (double)p[3 * j];
            h1 += w * (double)p[3 * j + 1];
            h2 += w * (double)p[3 * j + 2];
        }
#pragma unroll
        for (int r = 0; r < IMAGE_BAND; ++r) {
            const int k = y - ylo[r];
            if (k >= 0 && k < ycnt[r]) {
                const double w = wy[(size_t)k * IMG + r];
                acc[r][0] += w * h0;
                acc[r][1] += w * h1;
                acc[r][2] += w * h2;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < IMAGE_BAND; ++r)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            double u = floor(acc[r][ch] + 0.5);
            u = u < 0.0 ? 0.0 : u > 255.0 ? 255.0 : u;
            const uint8_t b = (uint8_t)u;
            const size_t o = o0 + (size_t)r * IMG * 3 + ch;
            if (out_u8) out_u8[o] = b;
            if (out_f32) {
                const float v = (float)((double)b / 255.0);
                out_f32[o] = 2.f * v - 1.f;
            }
        }
}

void image_frames(const uint8_t* pixels, const int64_t* frames, const int64_t* taps, uint8_t* out_u8, float* out_f32, int rows,
                  int n_real, hipStream_t s) {
    for (int r0 = 0; r0 < rows; r0 += 65535) {          // gridDim.y limit
        const int nr = rows - r0 < 65535 ? rows - r0 : 65535;
        const int real = n_real - r0 < 0 ? 0 : n_real - r0;
        const size_t o = (size_t)r0 * IMG * IMG * 3;
        hipLaunchKernelGGL(image_frames_kernel, dim3(IMG / IMAGE_BAND, nr), dim3(256), 0, s, pixels, frames + (int64_t)IMAGE_DESC * r0,
                           taps, out_u8 ? out_u8 + o : nullptr, out_f32 ? out_f32 + o : nullptr, real);
    }
}

}  // namespace l3
