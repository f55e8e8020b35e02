// vggish.hip -- the reference's VGGish baseline features (data/usc/features.py:166-240 extract_vggish_embedding,
// get_vggish_frames_uniform), inference only, fp32, and the l3_vggish handle of the C ABI.
//
//   audio      load_audio(path, 16000) (features.py:18-28) + the zero pad to 15600 samples (features.py:170-181): the resample launch
//              of resample.hip at sr_new = 16000 writes every clip at its padded place in one zeroed 16 kHz buffer
//   log-mel    vggish/mel_features.py:71-97,114-218 with vggish_input.py:25-29: frames of 400 at hop 160, periodic Hann, 512-point
//              real DFT, magnitude, 257 x 64 mel matrix, log(x + 0.01) -- ONE launch per call over every clip (vggish_logmel_kernel):
//              the windowed DFT as a 400 x 576 matrix on v_mfma_f32_32x32x2_f32, magnitude, mel projection and log in the same
//              workgroup; the spectrum never reaches HBM
//   examples   vggish_input.py:64-75: 96 log-mel rows every int(round(hop * 100)) rows; a host-built table of first rows, followed
//              by the first convolution's loads (no example tensor in HBM)
//   network    vggish/vggish_slim.py:66-99: conv 64, pool, conv 128, pool, conv 256 x2, pool, conv 512 x2, pool (3x3 'SAME', bias,
//              ReLU; 2x2 / 2 max pools), flatten NHWC, fc 4096, 4096, 128 (ReLU each)
//   postproc   vggish/vggish_postprocess.py:51-94: pca (e - means), clip to [-2, 2], (x + 2) * 63.75 truncated
// Launches per batch of examples: 1 first convolution (gather + bias + ReLU + pool fused), 5 convolutions of conv.hip / conv_wino*.hip
// each followed by vggish_bias_relu_kernel (bias + ReLU, + 2x2 max where a pool follows), 3 mlp_dense_fwd, 1 postprocess.
// No float atomics: the same inputs give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/l3hip.h"
#include "conv_path.h"
#include "device_common.h"
#include "kernels.h"
#include "mlp.h"
#include "vggish.h"

namespace l3 {

// ---- log-mel ----------------------------------------------------------------------------------------------------------------------
// One workgroup per 32 frames of one clip.  The 5360 samples the frames span sit in LDS (sample s at s + s / 32: frame starts are 160
// apart, a multiple of the bank count, and the skew spreads the 32 rows of an A operand over the banks).  Wave w owns the 32-bin
// blocks w, w + 4, w + 8 of the spectrum: per block two accumulators (real, imaginary part of the same 32 bins: columns nb * 64 + j
// and nb * 64 + 32 + j of the DFT matrix), K = 400 in steps of 2, summed in eight blocks of 50; their magnitude goes to LDS as the A
// operand of the mel product (K = 288 zero-padded bins), whose two 32 x 32 tiles waves 0 and 1 compute.
constexpr int LM_SEG = (VG_LM_FRAMES - 1) * VG_HOP + VG_WIN;          // 5360
constexpr int LM_SEG_LDS = LM_SEG + LM_SEG / 32 + 1;
constexpr int LM_MAG_LD = VG_BINS_PAD + 1;                            // 289: rows a bank apart
constexpr int LM_KCHUNK = 50;                                         // products per partial sum of the DFT (400 = 8 x 50)
static_assert(VG_WIN % LM_KCHUNK == 0 && LM_KCHUNK % 2 == 0, "whole chunks of MFMA steps");

__device__ __forceinline__ int lm_idx(int s) { return s + (s >> 5); }

__global__ __launch_bounds__(256) void vggish_logmel_kernel(const float* x, const int64_t* blocks, const float* dft,
                                                            const float* mel, float* out) {
    __shared__ float seg[LM_SEG_LDS];
    __shared__ float mag[VG_LM_FRAMES * LM_MAG_LD];
    const int64_t* blk = blocks + 3 * (int64_t)blockIdx.x;
    const int64_t start = blk[0], out_row = blk[2];
    const int nv = (int)blk[1];                                       // frames of this block that exist (1..32)
    const int span = (nv - 1) * VG_HOP + VG_WIN;                      // samples they read: all inside the clip (host-checked)
    for (int s = threadIdx.x; s < LM_SEG; s += 256) seg[lm_idx(s)] = s < span ? x[start + s] : 0.f;
    __syncthreads();
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5, wave = threadIdx.x >> 6;
    for (int nb = wave; nb < VG_BIN_BLOCKS; nb += 4) {
        // blocked summation: the matrix core adds the 400 products of a bin one after the other, and the rounding error of a
        // running sum grows with the square root of its length.  Summed that way the log-mel of a hard-clipped clip was 2.9e-6 from
        // float64 where a float32 FFT is 6.6e-7 away (profiles/r12_vggish.txt); eight sums of 50, added up afterwards, carry
        // sqrt(50) roundings each.
        f32x16 re = {}, im = {};
        const float* d = dft + nb * 64 + r;
        for (int kc = 0; kc < VG_WIN; kc += LM_KCHUNK) {
            f32x16 pr = {}, pi = {};
#pragma unroll 5
            for (int k0 = kc; k0 < kc + LM_KCHUNK; k0 += 2) {
                const int k = k0 + h;
                const float a = seg[lm_idx(r * VG_HOP + k)];
                const float br = d[k * VG_DFT_COLS], bi = d[k * VG_DFT_COLS + 32];
                pr = __builtin_amdgcn_mfma_f32_32x32x2f32(a, br, pr, 0, 0, 0);
                pi = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bi, pi, 0, 0, 0);
            }
            re += pr;
            im += pi;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) mag[mfma_row(i, h) * LM_MAG_LD + nb * 32 + r] = sqrtf(re[i] * re[i] + im[i] * im[i]);
    }
    __syncthreads();
    if (wave >= 2) return;
    f32x16 acc = {};
    const float* m = mel + wave * 32 + r;
#pragma unroll 4
    for (int k0 = 0; k0 < VG_BINS_PAD; k0 += 2) {
        const int k = k0 + h;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(mag[r * LM_MAG_LD + k], m[k * VG_MELS], acc, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int row = mfma_row(i, h);
        if (row < nv) out[(out_row + row) * VG_MELS + wave * 32 + r] = logf(acc[i] + 0.01f);
    }
}

void vggish_logmel(const float* x, const int64_t* blocks, int64_t n_blocks, const float* dft, const float* mel, float* out,
                   hipStream_t s) {
    if (n_blocks > 0) hipLaunchKernelGGL(vggish_logmel_kernel, dim3((unsigned)n_blocks), dim3(256), 0, s, x, blocks, dft, mel, out);
}

// host constants: the windowed DFT [400][576] (block nb: 32 real then 32 imaginary columns of bins nb * 32 ..; bins >= 257 zero) and
// the mel matrix [288][64] (rows >= 257 zero), computed in double and rounded once
void vggish_host_dft(std::vector<float>* dft) {
    dft->assign((size_t)VG_WIN * VG_DFT_COLS, 0.f);
    const double two_pi = 6.283185307179586476925286766559;
    for (int n = 0; n < VG_WIN; ++n) {
        const double win = 0.5 - 0.5 * std::cos(two_pi / VG_WIN * n);            // mel_features.py:67-68
        for (int k = 0; k < VG_BINS; ++k) {
            const double ph = two_pi * (double)((n * k) % VG_NFFT) / VG_NFFT;
            float* row = dft->data() + (size_t)n * VG_DFT_COLS + (k / 32) * 64 + (k % 32);
            row[0] = (float)(win * std::cos(ph));
            row[32] = (float)(-win * std::sin(ph));
        }
    }
}

void vggish_host_mel(std::vector<float>* mel) {
    // spectrogram_to_mel_matrix(64, 257, 16000, 125, 7500), mel_features.py:114-184
    mel->assign((size_t)VG_BINS_PAD * VG_MELS, 0.f);
    auto to_mel = [](double hz) { return 1127.0 * std::log(1.0 + hz / 700.0); };
    const double lo = to_mel(125.0), hi = to_mel(7500.0), step = (hi - lo) / (VG_MELS + 1);
    std::vector<double> edges(VG_MELS + 2);
    for (int i = 0; i < VG_MELS + 2; ++i) edges[i] = i == VG_MELS + 1 ? hi : lo + step * i;      // np.linspace
    for (int k = 1; k < VG_BINS; ++k) {                                                          // DC row stays zero
        const double fm = to_mel(k == VG_BINS - 1 ? 8000.0 : (8000.0 / (VG_BINS - 1)) * k);
        for (int i = 0; i < VG_MELS; ++i) {
            const double up = (fm - edges[i]) / (edges[i + 1] - edges[i]), down = (edges[i + 2] - fm) / (edges[i + 2] - edges[i + 1]);
            (*mel)[(size_t)k * VG_MELS + i] = (float)std::max(0.0, std::min(up, down));
        }
    }
}

// segments {offset, length} of the 16 kHz buffer -> blocks {first sample, frames, first output row}; returns the log-mel rows
int64_t vggish_logmel_blocks(const int64_t* segs, int64_t n_seg, std::vector<int64_t>* blocks, std::vector<int64_t>* seg_row0) {
    int64_t rows = 0;
    blocks->clear();
    if (seg_row0) seg_row0->clear();
    for (int64_t i = 0; i < n_seg; ++i) {
        const int64_t off = segs[2 * i], len = segs[2 * i + 1];
        const int64_t frames = len < VG_WIN ? 0 : 1 + (len - VG_WIN) / VG_HOP;
        if (seg_row0) seg_row0->push_back(rows);
        for (int64_t f = 0; f < frames; f += VG_LM_FRAMES) {
            blocks->push_back(off + f * VG_HOP);
            blocks->push_back(std::min<int64_t>(VG_LM_FRAMES, frames - f));
            blocks->push_back(rows + f);
        }
        rows += frames;
    }
    if (seg_row0) seg_row0->push_back(rows);
    return rows;
}

// ---- first convolution: example gather + 3x3 'SAME' (Cin = 1) + bias + ReLU + 2x2 max ---------------------------------------------
// One workgroup per (example, pooled row): the four log-mel rows it needs (zero outside the example: the padding is per example,
// not per clip) in LDS, lane = output channel (its 9 weights in registers), each thread 8 pooled columns; relu(max + b) ==
// max(relu(. + b)) since both are monotone.
__global__ __launch_bounds__(256) void vggish_conv1_kernel(const float* logmel, const int64_t* ex_rows, const float* w,
                                                           const float* b, float* y) {
    __shared__ float in[4][VG_MELS + 2];
    const int e = blockIdx.x / (VG_ROWS / 2), ph = blockIdx.x - e * (VG_ROWS / 2);
    const float* src = logmel + ex_rows[e] * VG_MELS;
    for (int i = threadIdx.x; i < 4 * (VG_MELS + 2); i += 256) {
        const int rr = i / (VG_MELS + 2), cc = i - rr * (VG_MELS + 2);
        const int row = 2 * ph - 1 + rr, col = cc - 1;
        in[rr][cc] = (row >= 0 && row < VG_ROWS && col >= 0 && col < VG_MELS) ? src[row * VG_MELS + col] : 0.f;
    }
    __syncthreads();
    const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
    float wt[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) wt[t] = w[t * 64 + c];
    const float bias = b[c];
    float* dst = y + ((size_t)blockIdx.x * (VG_MELS / 2)) * 64 + c;
#pragma unroll 2
    for (int j = 0; j < 8; ++j) {
        const int pw = q * 8 + j;
        float best = -INFINITY;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                float acc = 0.f;
#pragma unroll
                for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) acc = fmaf(in[dy + kh][2 * pw + dx + kw], wt[kh * 3 + kw], acc);
                best = fmaxf(best, acc);
            }
        dst[(size_t)pw * 64] = fmaxf(best + bias, 0.f);
    }
}

void vggish_conv1(const float* logmel, const int64_t* ex_rows, const float* w, const float* b, float* y, int n, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(vggish_conv1_kernel, dim3((unsigned)n * (VG_ROWS / 2)), dim3(256), 0, s, logmel, ex_rows, w, b, y);
}

// ---- BatchNorm-free convolution tail: y = relu(x + b), or its 2x2 / stride 2 maximum ----------------------------------------------
// x (n, H, W, C), C % 4 == 0; POOL: H, W even, y (n, H / 2, W / 2, C).  In place is allowed without POOL only.
template <bool POOL>
__global__ __launch_bounds__(256) void vggish_bias_relu_kernel(const float* x, const float* b, float* y, int64_t total4, int H, int W,
                                                               int C) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const int c4 = C >> 2;
    const int c = (int)(i % c4) * 4;
    const f32x4 bias = *reinterpret_cast<const f32x4*>(b + c);
    f32x4 v;
    if (POOL) {
        const int Wo = W >> 1, Ho = H >> 1;
        const int64_t p = i / c4;
        const int xo = (int)(p % Wo);
        const int64_t q = p / Wo;
        const int yo = (int)(q % Ho);
        const int64_t n = q / Ho;
        const float* s = x + (((n * H + 2 * yo) * W + 2 * xo) * (int64_t)C) + c;
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(s), a1 = *reinterpret_cast<const f32x4*>(s + C);
        const f32x4 a2 = *reinterpret_cast<const f32x4*>(s + (int64_t)W * C), a3 = *reinterpret_cast<const f32x4*>(s + (int64_t)W * C + C);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = fmaxf(fmaxf(a0[j], a1[j]), fmaxf(a2[j], a3[j]));
    } else {
        v = *reinterpret_cast<const f32x4*>(x + i * 4);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = fmaxf(v[j] + bias[j], 0.f);
    *reinterpret_cast<f32x4*>(y + i * 4) = v;
}

void vggish_bias_relu(const float* x, const float* b, float* y, int n, int H, int W, int C, int pool, hipStream_t s) {
    const int64_t total4 = (int64_t)n * (pool ? (H / 2) * (W / 2) : H * W) * (C / 4);
    if (total4 <= 0) return;
    const dim3 grid((unsigned)((total4 + 255) / 256));
    if (pool)
        hipLaunchKernelGGL(vggish_bias_relu_kernel<true>, grid, dim3(256), 0, s, x, b, y, total4, H, W, C);
    else
        hipLaunchKernelGGL(vggish_bias_relu_kernel<false>, grid, dim3(256), 0, s, x, b, y, total4, H, W, C);
}

// ---- postprocessor ----------------------------------------------------------------------------------------------------------------
// out[e][j] = clip(sum_k pca[j][k] (emb[e][k] - means[k]), -2, 2), quantised: trunc((. + 2) * 63.75).  pca_t is the matrix
// transposed ([k][j]: coalesced); the sum runs k = 0..127 in order in one thread.
__global__ __launch_bounds__(VG_EMB) void vggish_postprocess_kernel(const float* emb, const float* pca_t, const float* means,
                                                                    float* out, int quantize) {
    __shared__ float d[VG_EMB];
    const int j = threadIdx.x;
    d[j] = emb[(size_t)blockIdx.x * VG_EMB + j] - means[j];
    __syncthreads();
    float acc = 0.f;
#pragma unroll 8
    for (int k = 0; k < VG_EMB; ++k) acc = fmaf(pca_t[k * VG_EMB + j], d[k], acc);
    acc = fminf(fmaxf(acc, -2.f), 2.f);
    if (quantize) acc = truncf((acc + 2.f) * 63.75f);
    out[(size_t)blockIdx.x * VG_EMB + j] = acc;
}

void vggish_postprocess(const float* emb, const float* pca_t, const float* means, float* out, int n, int quantize, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(vggish_postprocess_kernel, dim3((unsigned)n), dim3(VG_EMB), 0, s, emb, pca_t, means, out, quantize);
}

}  // namespace l3

// ---- the handle ---------------------------------------------------------------------------------------------------------------------
using namespace l3;

namespace {
struct VgLayer {
    const char* scope;      // TF variable scope under "vggish/"
    int H, W, Cin, Cout;    // convolutions: input map; dense: H = 0, Cin -> Cout
    int pool;
};
// vggish_slim.py:66-99
const VgLayer VG_LAYERS[9] = {
    {"conv1", 96, 64, 1, 64, 1},           {"conv2", 48, 32, 64, 128, 1},         {"conv3/conv3_1", 24, 16, 128, 256, 0},
    {"conv3/conv3_2", 24, 16, 256, 256, 1}, {"conv4/conv4_1", 12, 8, 256, 512, 0}, {"conv4/conv4_2", 12, 8, 512, 512, 1},
    {"fc1/fc1_1", 0, 0, 12288, 4096, 0},    {"fc1/fc1_2", 0, 0, 4096, 4096, 0},    {"fc2", 0, 0, 4096, 128, 0}};
constexpr int64_t VG_ACT_FLOATS = 48 * 32 * 128;        // largest activation of one example (conv2's output)

int64_t layer_w_numel(const VgLayer& L) { return (int64_t)(L.H ? 9 : 1) * L.Cin * L.Cout; }
}  // namespace

struct l3_vggish {
    int device = 0, batch = 0, conv = L3_VGGISH_CONV_DIRECT;      // the default: see l3_vggish_set_conv in l3hip.h
    hipStream_t s = nullptr;
    float *w[9] = {}, *b[9] = {}, *u[9] = {};
    bool w_set[9] = {}, b_set[9] = {}, u_fresh[9] = {}, pca_set = false;
    float *dft = nullptr, *mel = nullptr, *pca_t = nullptr, *means = nullptr;
    float *act[2] = {}, *part = nullptr;
    int* ctr = nullptr;
    // grow-only buffers of a call, with their capacities in elements
    float *d_16k = nullptr, *d_logmel = nullptr, *d_out = nullptr;
    int64_t *d_lblocks = nullptr, *d_ex = nullptr;
    size_t cap_16k = 0, cap_logmel = 0, cap_out = 0, cap_lblocks = 0, cap_ex = 0;
    ResampleStage resample;
    DeviceBufs bufs;          // owns every pointer above
};

namespace {
ConvGeom layer_geom(const l3_vggish* v, const VgLayer& L, int n) {
    ConvGeom g = conv_geom(n, L.H, L.W, L.Cin, L.Cout, 3, 3, true, v->conv == L3_FP32_CONV_F2X2 ? 1 : 0);
    g.solo = 1;
    return g;
}

// layers 1..5 of n examples: act[0] holds conv1's pooled output; returns the buffer index that holds the flattened pool4
int run_convs(l3_vggish* v, int n) {
    int cur = 0;
    for (int l = 1; l <= 5; ++l) {
        const VgLayer& L = VG_LAYERS[l];
        const ConvGeom g = layer_geom(v, L, n);
        const ConvFwdPath p = conv_resolve_fwd(g, ConvStorage{}, v->conv != L3_VGGISH_CONV_DIRECT);
        ConvBufs b;          // no bias: it goes with the ReLU below.  The transformed filter is kept until the weights change
        b.x = v->act[cur], b.w = v->w[l], b.y = v->act[cur ^ 1], b.wino_u = v->u[l], b.u_ready = v->u_fresh[l];
        conv_run_fwd(p, g, ConvStorage{}, b, v->s);
        if (p.wino_filter) v->u_fresh[l] = true;
        cur ^= 1;
        if (L.pool) {
            vggish_bias_relu(v->act[cur], v->b[l], v->act[cur ^ 1], n, L.H, L.W, L.Cout, 1, v->s);
            cur ^= 1;
        } else {
            vggish_bias_relu(v->act[cur], v->b[l], v->act[cur], n, L.H, L.W, L.Cout, 0, v->s);
        }
    }
    return cur;
}

// the three dense layers; the embedding (n, 128) goes to `emb`
void run_dense(l3_vggish* v, int cur, int n, float* emb) {
    for (int l = 6; l < 9; ++l) {
        const VgLayer& L = VG_LAYERS[l];
        float* y = l == 8 ? emb : v->act[cur ^ 1];
        mlp_dense_fwd(v->act[cur], nullptr, L.Cin, v->w[l], v->b[l], y, n, L.Cin, L.Cout, 1, v->part, v->ctr, v->s);
        cur ^= 1;
    }
}
}  // namespace

extern "C" {

int l3_vggish_create(int device, int batch, l3_vggish** out) {
    if (!out) return fail(L3_EINVAL, "l3_vggish_create: NULL out");
    *out = nullptr;
    if (batch == 0) batch = L3_VGGISH_DEFAULT_BATCH;
    if (batch < 1 || batch > L3_VGGISH_MAX_BATCH)
        return fail(L3_EINVAL, "l3_vggish_create: batch must be in [1, " + std::to_string(L3_VGGISH_MAX_BATCH) + "]");
    if (!device_ok(device)) return fail(L3_EHIP, no_gpu_message("l3_vggish_create", device));
    l3_vggish* v = new l3_vggish();
    v->device = device;
    v->batch = batch;
    DeviceBufs& dev = v->bufs;
    for (int l = 0; l < 9; ++l) {
        const VgLayer& L = VG_LAYERS[l];
        v->w[l] = dev.alloc<float>((size_t)layer_w_numel(L)), v->b[l] = dev.alloc<float>((size_t)L.Cout);
        if (l >= 1 && l <= 5) v->u[l] = dev.alloc<float>((size_t)36 * L.Cin * L.Cout);
    }
    std::vector<float> dft, mel;
    vggish_host_dft(&dft);
    vggish_host_mel(&mel);
    v->dft = dev.alloc<float>(dft.size()), v->mel = dev.alloc<float>(mel.size());
    v->pca_t = dev.alloc<float>(VG_EMB * VG_EMB), v->means = dev.alloc<float>(VG_EMB);
    v->act[0] = dev.alloc<float>((size_t)batch * VG_ACT_FLOATS), v->act[1] = dev.alloc<float>((size_t)batch * VG_ACT_FLOATS);
    v->part = dev.alloc<float>((size_t)MLP_PART_FLOATS), v->ctr = dev.alloc<int>((size_t)MLP_FWD_COUNTERS);
    const bool ok = dev.ok() && hipStreamCreate(&v->s) == hipSuccess &&
                    hipMemset(v->ctr, 0, (size_t)MLP_FWD_COUNTERS * 4) == hipSuccess &&
                    hipMemcpy(v->dft, dft.data(), dft.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
                    hipMemcpy(v->mel, mel.data(), mel.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
        l3_vggish_destroy(v);
        return fail(L3_ENOMEM, "l3_vggish_create: device allocation failed");
    }
    *out = v;
    return L3_OK;
}

void l3_vggish_destroy(l3_vggish* v) {
    if (!v) return;
    (void)hipSetDevice(v->device);
    if (v->s) (void)hipStreamSynchronize(v->s);
    if (v->s) (void)hipStreamDestroy(v->s);
    delete v;
}

int l3_vggish_batch(const l3_vggish* v) { return v ? v->batch : 0; }

int l3_vggish_set_conv(l3_vggish* v, int fp32_conv) {
    if (!v || (fp32_conv != L3_FP32_CONV_F4X4 && fp32_conv != L3_FP32_CONV_F2X2 && fp32_conv != L3_VGGISH_CONV_DIRECT))
        return fail(L3_EINVAL, "l3_vggish_set_conv: fp32_conv must be L3_FP32_CONV_F4X4, L3_FP32_CONV_F2X2 or L3_VGGISH_CONV_DIRECT");
    if (fp32_conv != v->conv)
        for (int l = 0; l < 9; ++l) v->u_fresh[l] = false;          // the two Winograd forms keep different transformed filters
    v->conv = fp32_conv;
    return L3_OK;
}

int l3_vggish_set_weight(l3_vggish* v, const char* name, const float* src, int64_t numel) {
    if (!v || !name || !src) return fail(L3_EINVAL, "l3_vggish_set_weight: NULL argument");
    for (int l = 0; l < 9; ++l) {
        const VgLayer& L = VG_LAYERS[l];
        const std::string base = std::string("vggish/") + L.scope;
        const bool is_w = base + "/weights" == name, is_b = base + "/biases" == name;
        if (!is_w && !is_b) continue;
        const int64_t want = is_w ? layer_w_numel(L) : L.Cout;
        if (numel != want)
            return fail(L3_EINVAL, std::string("l3_vggish_set_weight: ") + name + " has " + std::to_string(want) + " elements, got " +
                                       std::to_string(numel));
        if (hipSetDevice(v->device) != hipSuccess || hipStreamSynchronize(v->s) != hipSuccess ||
            hipMemcpy(is_w ? v->w[l] : v->b[l], src, (size_t)numel * 4, hipMemcpyHostToDevice) != hipSuccess)
            return fail(L3_EHIP, std::string("l3_vggish_set_weight: copy of ") + name + " failed");
        (is_w ? v->w_set : v->b_set)[l] = true;
        if (is_w) v->u_fresh[l] = false;
        return L3_OK;
    }
    return fail(L3_EINVAL, std::string("l3_vggish_set_weight: no VGGish variable named ") + name);
}

int l3_vggish_set_pca(l3_vggish* v, const float* pca_matrix, const float* pca_means) {
    if (!v || !pca_matrix || !pca_means) return fail(L3_EINVAL, "l3_vggish_set_pca: NULL argument");
    std::vector<float> t((size_t)VG_EMB * VG_EMB);
    for (int j = 0; j < VG_EMB; ++j)
        for (int k = 0; k < VG_EMB; ++k) t[(size_t)k * VG_EMB + j] = pca_matrix[(size_t)j * VG_EMB + k];
    if (hipSetDevice(v->device) != hipSuccess || hipStreamSynchronize(v->s) != hipSuccess ||
        hipMemcpy(v->pca_t, t.data(), t.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(v->means, pca_means, VG_EMB * 4, hipMemcpyHostToDevice) != hipSuccess)
        return fail(L3_EHIP, "l3_vggish_set_pca: copy failed");
    v->pca_set = true;
    return L3_OK;
}

int l3_vggish_embed_clips_resampled(l3_vggish* v, const float* native, int64_t n_native, const int64_t* clips, int64_t n_clips,
                                    const double* half_window, int64_t n_window, int num_table, int64_t n_samples,
                                    const int64_t* segments, int64_t n_segments, const int64_t* example_rows, int64_t n_examples,
                                    int postprocess, float* out) {
    const char* me = "l3_vggish_embed_clips_resampled: ";
    if (!v || !native || !clips || !half_window || !segments || !example_rows || !out || n_native < 0 || n_clips < 0 || n_samples < 0 ||
        n_segments < 0 || n_examples < 0)
        return fail(L3_EINVAL, std::string(me) + "NULL pointer or negative count");
    if (postprocess < L3_VGGISH_RAW || postprocess > L3_VGGISH_QUANTIZED) return fail(L3_EINVAL, std::string(me) + "bad postprocess mode");
    for (int l = 0; l < 9; ++l)
        if (!v->w_set[l] || !v->b_set[l])
            return fail(L3_ESTATE, std::string(me) + "vggish/" + VG_LAYERS[l].scope + (v->w_set[l] ? "/biases" : "/weights") + " was never set");
    if (postprocess != L3_VGGISH_RAW && !v->pca_set) return fail(L3_ESTATE, std::string(me) + "the PCA parameters were never set");
    int64_t bad = 0;
    if (const char* why = resample_clips_error(clips, n_clips, n_native, VG_SR, n_window, num_table, n_samples, true, &bad))
        return fail(L3_EINVAL, std::string(me) + (bad >= 0 ? "clip " + std::to_string(bad) + ": " : std::string()) + why);
    for (int64_t i = 0; i < n_segments; ++i) {
        const int64_t off = segments[2 * i], len = segments[2 * i + 1];
        if (off < 0 || len < 0 || off > n_samples || len > n_samples - off)
            return fail(L3_EINVAL, std::string(me) + "segment " + std::to_string(i) + " outside the 16 kHz buffer");
    }
    std::vector<int64_t> blocks, row0;
    const int64_t rows = vggish_logmel_blocks(segments, n_segments, &blocks, &row0);
    for (int64_t e = 0; e < n_examples; ++e) {           // an example's 96 rows lie inside one segment's log-mel
        const int64_t r = example_rows[e];
        bool ok = r >= 0 && r + VG_ROWS <= rows;
        if (ok) {
            const int64_t sgm = std::upper_bound(row0.begin(), row0.end(), r) - row0.begin() - 1;
            ok = r + VG_ROWS <= row0[sgm + 1];
        }
        if (!ok) return fail(L3_EINVAL, std::string(me) + "example " + std::to_string(e) + " does not lie inside one segment's log-mel rows");
    }
    if (n_examples == 0) return L3_OK;
    if (hipSetDevice(v->device) != hipSuccess) return fail(L3_EHIP, std::string(me) + "hipSetDevice failed");

    DeviceBufs& dev = v->bufs;
    dev.grow(&v->d_16k, &v->cap_16k, (size_t)n_samples);
    dev.grow(&v->d_lblocks, &v->cap_lblocks, blocks.size());
    dev.grow(&v->d_logmel, &v->cap_logmel, (size_t)rows * VG_MELS);
    dev.grow(&v->d_ex, &v->cap_ex, (size_t)n_examples);
    dev.grow(&v->d_out, &v->cap_out, (size_t)n_examples * VG_EMB + (size_t)v->batch * VG_EMB);      // + one batch of raw embeddings
    float *d_16k = v->d_16k, *d_logmel = v->d_logmel, *d_out = v->d_out;
    int64_t *d_lblocks = v->d_lblocks, *d_ex = v->d_ex;
    if (!d_16k || !d_lblocks || !d_logmel || !d_ex || !d_out) return fail(L3_ENOMEM, std::string(me) + "device allocation failed");
    std::string why;
    if (const int rc = v->resample.run(native, n_native, clips, n_clips, VG_SR, half_window, n_window, num_table, true, d_16k,
                                       n_samples, v->s, &why))
        return fail(rc, std::string(me) + why);
    if (hipMemcpyAsync(d_lblocks, blocks.data(), blocks.size() * 8, hipMemcpyHostToDevice, v->s) != hipSuccess ||
        hipMemcpyAsync(d_ex, example_rows, (size_t)n_examples * 8, hipMemcpyHostToDevice, v->s) != hipSuccess) {
        (void)stream_wait(v->s);          // `blocks` goes out of scope
        return fail(L3_EHIP, std::string(me) + "upload failed");
    }
    vggish_logmel(d_16k, d_lblocks, (int64_t)blocks.size() / 3, v->dft, v->mel, d_logmel, v->s);
    float* d_emb = d_out + (size_t)n_examples * VG_EMB;
    for (int64_t e0 = 0; e0 < n_examples; e0 += v->batch) {
        const int n = (int)std::min<int64_t>(v->batch, n_examples - e0);
        vggish_conv1(d_logmel, d_ex + e0, v->w[0], v->b[0], v->act[0], n, v->s);
        const int cur = run_convs(v, n);
        float* dst = d_out + (size_t)e0 * VG_EMB;
        run_dense(v, cur, n, postprocess == L3_VGGISH_RAW ? dst : d_emb);
        if (postprocess != L3_VGGISH_RAW)
            vggish_postprocess(d_emb, v->pca_t, v->means, dst, n, postprocess == L3_VGGISH_QUANTIZED ? 1 : 0, v->s);
    }
    if (hipMemcpyAsync(out, d_out, (size_t)n_examples * VG_EMB * 4, hipMemcpyDeviceToHost, v->s) != hipSuccess ||
        stream_wait(v->s) != hipSuccess)
        return fail(L3_EHIP, std::string(me) + "a launch or the read-back failed: " + hipGetErrorString(hipGetLastError()));
    return L3_OK;
}

}  // extern "C"
