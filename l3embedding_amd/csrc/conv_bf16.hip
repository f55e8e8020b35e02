// conv_bf16.hip -- mixed-precision convolution: bf16 operands, fp32 accumulate (v_mfma_f32_32x32x16_bf16).
//
// BASELINE.json configs[4] ("bf16 compute / fp32 accumulate with mixed-precision MFMA"): in bf16
// mode the 3x3 'same' convolutions with Cin and Cout multiples of 64 (the same 14 Conv2D layers
// of l3embedding/audio_model.py:372-445 / vision_model.py:126-205 that the fp32 build runs as
// Winograd, 98.6 % of the flops) round BOTH operands to bfloat16 (round-to-nearest-even,
// v_cvt_pk_bf16_f32) as they leave LDS and multiply-accumulate in fp32.  Activations, weights,
// BatchNorm, the loss and Adam stay fp32 in HBM (master weights), so the rounding is exactly
// "conv(bf16(x), bf16(w)) with fp32 accumulation" -- which is what oracle/l3_oracle.py restates
// for this mode, and bf16 x bf16 products are exact in fp32, so parity is tight.
//
// Kernel = the direct implicit GEMM of conv.hip with both tiles in [row][32 k] form:
//   block 128x128 (Cout >= 128) or 256x64 outputs, 4 waves x 64x64, stage = 32 channels of one tap;
//   A rows = output pixels (NHWC gather), B rows = output channels of the filter given as
//   [flipped tap][Cout][Cin] (conv_flip_weights() for the forward pass; the forward filter itself
//   for the data gradient); HBM -> LDS with buffer_load_dwordx4 ... lds, scalar tap/chunk offsets,
//   padding taps = out-of-range lane offsets; 128-B rows XOR-swizzled by (row >> 1) & 7 so the two
//   ds_read_b128 a lane needs per 16-k step are conflict free; 8 bf16 MFMAs (K = 16) per stage.
#include "kernels.h"
#include "device_common.h"

#include <stdlib.h>

#include <mutex>

namespace l3 {

namespace {


struct BfArgs {
    const float* x;
    const float* wn;
    const float* bias;
    float* y;
    int N, H, W, Cin, Ho, Wo, Cout, KH, KW, padT, padL;
    int M, nkt, mtiles, ntiles;
    float* stat_part;     // STATS: BatchNorm partial sums [m tile][2][Cout] about the pivot bias[c] (bn_fused.hip layout)
    int stat_mode;        // 1: moments of y, 2: moments of relu(y)
};


__device__ __forceinline__ bf16x8 to_bf16x8(f32x4 lo, f32x4 hi) {
    bf16x8 r;
    r[0] = (__bf16)lo.x; r[1] = (__bf16)lo.y; r[2] = (__bf16)lo.z; r[3] = (__bf16)lo.w;
    r[4] = (__bf16)hi.x; r[5] = (__bf16)hi.y; r[6] = (__bf16)hi.z; r[7] = (__bf16)hi.w;
    return r;
}

template <int WAVES_M, int WAVES_N>
__global__ __launch_bounds__(256, 2) void conv_igemm_bf16_kernel(BfArgs a) {
    constexpr int BKT = 32;
    constexpr int BM = WAVES_M * 64, BN = WAVES_N * 64;
    constexpr int A_TILE = BM * BKT, B_TILE = BN * BKT;
    constexpr int A_PW = BM / 32, B_PW = BN / 32;        // 1-KiB pieces (8 rows x 128 B) per wave
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;
    float* Bs = smem + 2 * A_TILE;

    const int t = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
    const int logical = xcd_remap(blockIdx.x, a.mtiles * a.ntiles);
    const int nt = logical % a.ntiles, mt = logical / a.ntiles;
    const int m0 = mt * BM, n0 = nt * BN;
    const int HoWo = a.Ho * a.Wo;
    const int margin = (a.padT * a.W + a.padL) * a.Cin * 4;

    unsigned avoff[A_PW], anot[A_PW], bvoff[B_PW];
#pragma unroll
    for (int i = 0; i < A_PW; ++i) {
        const int r = (wave * A_PW + i) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((r >> 1) & 7);           // logical 16-B chunk stored at this slot
        const int m = m0 + r;
        unsigned mask = 0;
        int off = 0;
        if (m < a.M) {
            const int n = m / HoWo, rem = m - n * HoWo;
            const int ho = rem / a.Wo, wo = rem - ho * a.Wo;
            const int h0 = ho - a.padT, w0 = wo - a.padL;
            off = ((n * a.H + h0) * a.W + w0) * a.Cin * 4 + c * 16 + margin;
            for (int tap = 0; tap < a.KH * a.KW; ++tap) {
                const int dh = tap / a.KW, dw = tap - dh * a.KW;
                if ((unsigned)(h0 + dh) < (unsigned)a.H && (unsigned)(w0 + dw) < (unsigned)a.W) mask |= 1u << tap;
            }
        }
        avoff[i] = (unsigned)off;
        anot[i] = ~mask;
    }
#pragma unroll
    for (int j = 0; j < B_PW; ++j) {
        const int r = (wave * B_PW + j) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((r >> 1) & 7);
        bvoff[j] = n0 + r < a.Cout ? (unsigned)(((n0 + r) * a.Cin + c * 4) * 4) : 0x80000000u;
    }
    const __amdgpu_buffer_rsrc_t xsrd = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((const char*)a.x - margin), 0, (int)((size_t)a.N * a.H * a.W * a.Cin * 4 + margin), 0x00020000);
    const __amdgpu_buffer_rsrc_t wsrd = __builtin_amdgcn_make_buffer_rsrc(
        (void*)a.wn, 0, (int)((size_t)a.KH * a.KW * a.Cin * a.Cout * 4), 0x00020000);

    int ld_tap = 0, ld_c0 = 0, ld_dh = 0, ld_dw = 0;
    const int ntaps = a.KH * a.KW;
    auto issue = [&](int buf) {
        // k order: 32-channel chunk OUTER, filter tap INNER (the taps of a chunk re-hit L1/L2)
        const int asoff = ((ld_dh * a.W + ld_dw) * a.Cin + ld_c0) * 4;
        const int bsoff = ((ntaps - 1 - ld_tap) * a.Cout * a.Cin + ld_c0) * 4;
#pragma unroll
        for (int i = 0; i < A_PW; ++i) {
            const unsigned vo = ((anot[i] >> ld_tap) << 31) | avoff[i];
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                xsrd, (__attribute__((address_space(3))) void*)(As + buf * A_TILE + (wave * A_PW + i) * 256), 16, (int)vo,
                asoff, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < B_PW; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                wsrd, (__attribute__((address_space(3))) void*)(Bs + buf * B_TILE + (wave * B_PW + j) * 256), 16,
                (int)bvoff[j], bsoff, 0, 0);
        ++ld_tap;
        if (++ld_dw == a.KW) {
            ld_dw = 0;
            if (++ld_dh == a.KH) {
                ld_dh = 0;
                ld_tap = 0;
                ld_c0 += BKT;
            }
        }
    };

    const int wm = wave / WAVES_N, wn = wave - wm * WAVES_N;
    const int l31 = lane & 31, hi32 = lane >> 5;
    const int swz = (l31 >> 1) & 7;
    const int a_lane = (wm * 64 + l31) * BKT, b_lane = (wn * 64 + l31) * BKT;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    auto compute = [&](int buf) {
        const float* Ab = As + buf * A_TILE + a_lane;
        const float* Bb = Bs + buf * B_TILE + b_lane;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            // this lane's 8 consecutive k of the 16-k step: logical chunks c, c + 1
            const int c = 4 * s2 + 2 * hi32;
            const int o0 = (c ^ swz) * 4, o1 = ((c + 1) ^ swz) * 4;
            bf16x8 av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
                av[i] = to_bf16x8(*reinterpret_cast<const f32x4*>(Ab + i * 32 * BKT + o0),
                                  *reinterpret_cast<const f32x4*>(Ab + i * 32 * BKT + o1));
#pragma unroll
            for (int j = 0; j < 2; ++j)
                bv[j] = to_bf16x8(*reinterpret_cast<const f32x4*>(Bb + j * 32 * BKT + o0),
                                  *reinterpret_cast<const f32x4*>(Bb + j * 32 * BKT + o1));
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
    };

    issue(0);
    __syncthreads();
    for (int kt = 0; kt < a.nkt; kt += 2) {
        if (kt + 1 < a.nkt) issue(1);
        compute(0);
        __syncthreads();
        if (kt + 1 < a.nkt) {
            if (kt + 2 < a.nkt) issue(0);
            compute(1);
            __syncthreads();
        }
    }

    // epilogue: 64 x 64 wave tile leaves through an LDS transpose as 16-B stores (as conv.hip)
    float* Es = smem + wave * (32 * 64);
    const int n_base = n0 + wn * 64;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int jn = 0; jn < 2; ++jn)
#pragma unroll
            for (int r = 0; r < 16; ++r) Es[((r & 3) + 8 * (r >> 2) + 4 * hi32) * 64 + jn * 32 + l31] = acc[i][jn][r];
        __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0)
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int row = p * 4 + (lane >> 4), c4 = (lane & 15) * 4;
            const int m = m0 + wm * 64 + i * 32 + row, n = n_base + c4;
            f32x4 v = *reinterpret_cast<const f32x4*>(Es + row * 64 + c4);
            if (m < a.M && n < a.Cout) {
                if (a.bias != nullptr) v += *reinterpret_cast<const f32x4*>(a.bias + n);
                *reinterpret_cast<f32x4*>(a.y + (size_t)m * a.Cout + n) = v;
            }
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
    }
}

// Same kernel for operands that are ALREADY bfloat16 in HBM (activations written as bf16 by the
// BatchNorm / pool kernels, filters cast once per step by conv_weights_bf16): rows are 64 channels
// = 128 B, so the LDS image, the swizzle and the staging addresses are byte-for-byte those of the
// fp32-input kernel, but a stage now holds K = 64 (16 MFMAs per barrier), a lane's ds_read_b128 IS
// its 8-element MFMA operand (no conversion), and every load moves half the bytes per k.  Same products
// as the fp32-input kernel (the stored value IS the rounded operand); only the fp32 summation order
// differs (64-channel instead of 32-channel stages).
template <int WAVES_M, int WAVES_N, bool STATS, bool OBF>
__global__ __launch_bounds__(256, 2) void conv_igemm_bf16in_kernel(BfArgs a) {
    constexpr int BKB = 128;                                  // bytes per tile row = 64 bf16
    constexpr int BM = WAVES_M * 64, BN = WAVES_N * 64;
    constexpr int A_TILE = BM * BKB / 4, B_TILE = BN * BKB / 4;   // in floats (LDS is declared as float)
    constexpr int A_PW = BM / 32, B_PW = BN / 32;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;
    float* Bs = smem + 2 * A_TILE;

    const int t = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
    const int logical = xcd_remap(blockIdx.x, a.mtiles * a.ntiles);
    const int nt = logical % a.ntiles, mt = logical / a.ntiles;
    const int m0 = mt * BM, n0 = nt * BN;
    const int HoWo = a.Ho * a.Wo;
    const int margin = (a.padT * a.W + a.padL) * a.Cin * 2;

    unsigned avoff[A_PW], anot[A_PW], bvoff[B_PW];
#pragma unroll
    for (int i = 0; i < A_PW; ++i) {
        const int r = (wave * A_PW + i) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((r >> 1) & 7);
        const int m = m0 + r;
        unsigned mask = 0;
        int off = 0;
        if (m < a.M) {
            const int n = m / HoWo, rem = m - n * HoWo;
            const int ho = rem / a.Wo, wo = rem - ho * a.Wo;
            const int h0 = ho - a.padT, w0 = wo - a.padL;
            off = ((n * a.H + h0) * a.W + w0) * a.Cin * 2 + c * 16 + margin;
            for (int tap = 0; tap < a.KH * a.KW; ++tap) {
                const int dh = tap / a.KW, dw = tap - dh * a.KW;
                if ((unsigned)(h0 + dh) < (unsigned)a.H && (unsigned)(w0 + dw) < (unsigned)a.W) mask |= 1u << tap;
            }
        }
        avoff[i] = (unsigned)off;
        anot[i] = ~mask;
    }
#pragma unroll
    for (int j = 0; j < B_PW; ++j) {
        const int r = (wave * B_PW + j) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((r >> 1) & 7);
        bvoff[j] = n0 + r < a.Cout ? (unsigned)((n0 + r) * a.Cin * 2 + c * 16) : 0x80000000u;
    }
    const __amdgpu_buffer_rsrc_t xsrd = __builtin_amdgcn_make_buffer_rsrc(
        (void*)((const char*)a.x - margin), 0, (int)((size_t)a.N * a.H * a.W * a.Cin * 2 + margin), 0x00020000);
    const __amdgpu_buffer_rsrc_t wsrd = __builtin_amdgcn_make_buffer_rsrc(
        (void*)a.wn, 0, (int)((size_t)a.KH * a.KW * a.Cin * a.Cout * 2), 0x00020000);

    int ld_tap = 0, ld_c0 = 0, ld_dh = 0, ld_dw = 0;
    const int ntaps = a.KH * a.KW;
    auto issue = [&](int buf) {
        const int asoff = ((ld_dh * a.W + ld_dw) * a.Cin + ld_c0) * 2;
        const int bsoff = ((ntaps - 1 - ld_tap) * a.Cout * a.Cin + ld_c0) * 2;
#pragma unroll
        for (int i = 0; i < A_PW; ++i) {
            const unsigned vo = ((anot[i] >> ld_tap) << 31) | avoff[i];
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                xsrd, (__attribute__((address_space(3))) void*)(As + buf * A_TILE + (wave * A_PW + i) * 256), 16, (int)vo,
                asoff, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < B_PW; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(
                wsrd, (__attribute__((address_space(3))) void*)(Bs + buf * B_TILE + (wave * B_PW + j) * 256), 16,
                (int)bvoff[j], bsoff, 0, 0);
        ++ld_tap;
        if (++ld_dw == a.KW) {
            ld_dw = 0;
            if (++ld_dh == a.KH) {
                ld_dh = 0;
                ld_tap = 0;
                ld_c0 += 64;
            }
        }
    };

    const int wm = wave / WAVES_N, wn = wave - wm * WAVES_N;
    const int l31 = lane & 31, hi32 = lane >> 5;
    const int swz = (l31 >> 1) & 7;
    const int a_lane = (wm * 64 + l31) * 32, b_lane = (wn * 64 + l31) * 32;      // 32 floats = 128 B per row

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    auto compute = [&](int buf) {
        const float* Ab = As + buf * A_TILE + a_lane;
        const float* Bb = Bs + buf * B_TILE + b_lane;
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            const int o = ((2 * s4 + hi32) ^ swz) * 4;          // this lane's 8 consecutive k of the 16-k step
            bf16x8 av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) av[i] = *reinterpret_cast<const bf16x8*>(Ab + i * 32 * 32 + o);
#pragma unroll
            for (int j = 0; j < 2; ++j) bv[j] = *reinterpret_cast<const bf16x8*>(Bb + j * 32 * 32 + o);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
    };

    issue(0);
    __syncthreads();
    for (int kt = 0; kt < a.nkt; kt += 2) {
        if (kt + 1 < a.nkt) issue(1);
        compute(0);
        __syncthreads();
        if (kt + 1 < a.nkt) {
            if (kt + 2 < a.nkt) issue(0);
            compute(1);
            __syncthreads();
        }
    }

    float* Es = smem + wave * (32 * 64);
    const int n_base = n0 + wn * 64;
    // STATS: sum / sum of squares of this block's outputs per channel, about the pivot bias[c], for the
    // BatchNorm that follows (its statistics pass then only combines the per-block partials)
    f32x4 st0 = {0.f, 0.f, 0.f, 0.f}, st1 = {0.f, 0.f, 0.f, 0.f};
    const bool srelu = STATS && a.stat_mode == 2;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int jn = 0; jn < 2; ++jn)
#pragma unroll
            for (int r = 0; r < 16; ++r) Es[((r & 3) + 8 * (r >> 2) + 4 * hi32) * 64 + jn * 32 + l31] = acc[i][jn][r];
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int row = p * 4 + (lane >> 4), c4 = (lane & 15) * 4;
            const int m = m0 + wm * 64 + i * 32 + row, n = n_base + c4;
            f32x4 v = *reinterpret_cast<const f32x4*>(Es + row * 64 + c4);
            if (m < a.M && n < a.Cout) {
                f32x4 bz = {0.f, 0.f, 0.f, 0.f};
                if (a.bias != nullptr) bz = *reinterpret_cast<const f32x4*>(a.bias + n);
                if constexpr (OBF) {
                    // the output tensor lives in HBM as bfloat16: round (nearest even) accumulator + bias, and take
                    // the statistics of the ROUNDED values -- the tensor the BatchNorm that follows will read
                    v += bz;
                    bf16x4 h;
#pragma unroll
                    for (int e = 0; e < 4; ++e) h[e] = (__bf16)v[e];
                    if constexpr (STATS) {
                        f32x4 d;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float yr = (float)h[e];
                            d[e] = srelu ? fmaxf(yr, 0.f) - fmaxf(bz[e], 0.f) : yr - bz[e];
                        }
                        st0 += d;
                        st1 += d * d;
                    }
                    *reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(a.y) + (size_t)m * a.Cout + n) = h;
                } else {
                    v += bz;                                           // the statistics are those of the STORED values
                    if constexpr (STATS) {
                        f32x4 d;
#pragma unroll
                        for (int e = 0; e < 4; ++e) d[e] = srelu ? fmaxf(v[e], 0.f) - fmaxf(bz[e], 0.f) : v[e] - bz[e];
                        st0 += d;
                        st1 += d * d;
                    }
                    *reinterpret_cast<f32x4*>(a.y + (size_t)m * a.Cout + n) = v;
                }
            }
        }
        __builtin_amdgcn_s_waitcnt(0xc07f);
        __builtin_amdgcn_wave_barrier();
    }
    if constexpr (STATS) {
        // lanes with equal (lane & 15) hold the same channel quad: combine the four row groups ...
#pragma unroll
        for (int off = 16; off < 64; off <<= 1)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                st0[e] += __shfl_xor(st0[e], off, 64);
                st1[e] += __shfl_xor(st1[e], off, 64);
            }
        // ... and the waves that share this column range, in wave order, through LDS
        __syncthreads();
        float* red = smem;                                         // [which 2][wave 4][64]
        if (lane < 16) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                red[(0 * 4 + wave) * 64 + lane * 4 + e] = st0[e];
                red[(1 * 4 + wave) * 64 + lane * 4 + e] = st1[e];
            }
        }
        __syncthreads();
        if (t < 2 * BN) {
            const int which = t / BN, col = t - which * BN;        // column inside the block tile
            const int cw = col / 64, ch = col - cw * 64;
            float sum = 0.f;
#pragma unroll
            for (int w2 = 0; w2 < WAVES_M; ++w2) sum += red[(which * 4 + w2 * WAVES_N + cw) * 64 + ch];
            if (n0 + col < a.Cout) a.stat_part[((size_t)mt * 2 + which) * a.Cout + n0 + col] = sum;
        }
    }
}

// filter fp32 [tap][ci][co] (keras HWIO) -> bfloat16, as [flipped tap][co][ci] (flip = 1: forward operand) or
// unchanged order (flip = 0: the data gradient's operand is the forward filter read as [flipped tap][n][k]): [tap'][N][K] either
// way.  A SECOND copy follows it when K % 32 == 0, chunk-major: [tap'][K / 32][N][32] -- the 32-channel-chunk forms of the halo
// kernel fetch a filter slice (all N of one tap and chunk) as one contiguous run, eight whole cache lines per 1-KiB LDS-DMA piece
// instead of sixteen half lines.
__global__ __launch_bounds__(256) void weights_bf16_kernel(const float* __restrict__ w, __bf16* __restrict__ out, int taps,
                                                           int Cin, int Cout, int flip) {
    const int total = taps * Cin * Cout;
    const int N = flip ? Cout : Cin, K = flip ? Cin : Cout;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int k = i % K;
        int r = i / K;
        const int n = r % N;
        const int tap = r / N;
        const __bf16 v = flip ? (__bf16)w[((size_t)(taps - 1 - tap) * Cin + k) * Cout + n] : (__bf16)w[i];
        out[i] = v;
        if ((K & 31) == 0) out[(size_t)total + (((size_t)tap * (K >> 5) + (k >> 5)) * N + n) * 32 + (k & 31)] = v;
    }
}

template <int WAVES_M, int WAVES_N>
void launch_bf16(BfArgs a, hipStream_t s) {
    constexpr int BM = WAVES_M * 64, BN = WAVES_N * 64;
    constexpr size_t LDS = 2 * (size_t)(BM + BN) * 32 * sizeof(float);
    static_assert(LDS >= 4 * 32 * 64 * sizeof(float), "stage buffers must hold the epilogue");
    a.mtiles = (a.M + BM - 1) / BM;
    a.ntiles = (a.Cout + BN - 1) / BN;
    // the opt-in for > 64 KiB of dynamic LDS is per device: once per (kernel instantiation, device)
    static std::once_flag once[L3_MAX_DEVICES];
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::call_once(once[dev & (L3_MAX_DEVICES - 1)], [] {
        (void)hipFuncSetAttribute((const void*)conv_igemm_bf16_kernel<WAVES_M, WAVES_N>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS);
    });
    hipLaunchKernelGGL((conv_igemm_bf16_kernel<WAVES_M, WAVES_N>), dim3(a.mtiles * a.ntiles), dim3(256), LDS, s, a);
}

}  // namespace

// The mixed-precision rule (one rule for forward, data gradient and weight gradient, restated in
// oracle/l3_oracle.py:_mp_conv): 3x3 'same' convolutions whose Cin and Cout are multiples of 64.
bool conv_bf16_ok(const ConvGeom& g) {
    return g.KH == 3 && g.KW == 3 && g.padT == 1 && g.padL == 1 && g.Ho == g.H && g.Wo == g.W && g.Cin % 64 == 0 &&
           g.Cout % 64 == 0 &&
           (size_t)g.H * g.W * g.Cin * 4 + (size_t)(g.padT * g.W + g.padL) * g.Cin * 4 < (1ull << 31) &&
           (size_t)g.KH * g.KW * g.Cin * g.Cout * 4 < (1ull << 31);
}

template <int WAVES_M, int WAVES_N, bool STATS, bool OBF>
void launch_bf16in2(const BfArgs& a, hipStream_t s) {
    constexpr int BM = WAVES_M * 64, BN = WAVES_N * 64;
    constexpr size_t LDS = 2 * (size_t)(BM + BN) * 128;
    static_assert(LDS >= 4 * 32 * 64 * sizeof(float), "stage buffers must hold the epilogue");
    // the opt-in for > 64 KiB of dynamic LDS is per device: once per (kernel instantiation, device)
    static std::once_flag once[L3_MAX_DEVICES];
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::call_once(once[dev & (L3_MAX_DEVICES - 1)], [] {
        (void)hipFuncSetAttribute((const void*)conv_igemm_bf16in_kernel<WAVES_M, WAVES_N, STATS, OBF>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS);
    });
    hipLaunchKernelGGL((conv_igemm_bf16in_kernel<WAVES_M, WAVES_N, STATS, OBF>), dim3(a.mtiles * a.ntiles), dim3(256), LDS, s, a);
}

template <int WAVES_M, int WAVES_N>
void launch_bf16in(BfArgs a, hipStream_t s, bool out_bf16) {
    constexpr int BM = WAVES_M * 64, BN = WAVES_N * 64;
    a.mtiles = (a.M + BM - 1) / BM;
    a.ntiles = (a.Cout + BN - 1) / BN;
    if (a.stat_part != nullptr) {
        if (out_bf16) launch_bf16in2<WAVES_M, WAVES_N, true, true>(a, s); else launch_bf16in2<WAVES_M, WAVES_N, true, false>(a, s);
    } else {
        if (out_bf16) launch_bf16in2<WAVES_M, WAVES_N, false, true>(a, s); else launch_bf16in2<WAVES_M, WAVES_N, false, false>(a, s);
    }
}

void conv_weights_bf16(const float* w, void* out, int KH, int KW, int Cin, int Cout, bool flip, hipStream_t s) {
    const int total = KH * KW * Cin * Cout;
    const int blocks = (total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048;
    hipLaunchKernelGGL(weights_bf16_kernel, dim3(blocks), dim3(256), 0, s, w, reinterpret_cast<__bf16*>(out), KH * KW, Cin,
                       Cout, flip ? 1 : 0);
}

static int bf16_chunk_samples(const ConvGeom& g, bool operands_bf16) {
    // sample ranges whose input stays below the 2 GiB the 32-bit buffer offsets reach
    const size_t esz = operands_bf16 ? 2 : 4;
    const size_t per_sample = (size_t)g.H * g.W * g.Cin * esz;
    size_t ncs = ((1ull << 31) - 1 - (size_t)(g.padT * g.W + g.padL) * g.Cin * esz) / per_sample;
    if (ncs > (size_t)g.N) ncs = (size_t)g.N;
    return ncs < 1 ? 1 : (int)ncs;
}

int conv_bf16_stat_blocks(const ConvGeom& g) {
    if (!conv_bf16_ok(g)) return 0;
    const int nc = bf16_chunk_samples(g, true), bm = g.Cout > 64 ? 128 : 256;
    int blocks = 0;
    for (int n0 = 0; n0 < g.N; n0 += nc) {
        const int nn = g.N - n0 < nc ? g.N - n0 : nc;
        blocks += conv_bf16_halo_ok(g) ? conv_bf16_halo_patches(g, nn) : (nn * g.Ho * g.Wo + bm - 1) / bm;
    }
    return blocks;
}

void conv_bf16_fwd(const float* x, const float* wn, const float* bias, float* y, const ConvGeom& g, hipStream_t s,
                   bool operands_bf16, float* stat_part, int stat_mode, bool out_bf16, const BnBwdFuse* bn_bwd) {
    const size_t esz = operands_bf16 ? 2 : 4;
    const size_t per_sample = (size_t)g.H * g.W * g.Cin * esz;
    const int nc = bf16_chunk_samples(g, operands_bf16);
    if (!operands_bf16) {        // only the bf16-operand kernel carries the statistics / bf16-output epilogues
        stat_part = nullptr;
        out_bf16 = false;
    }
    const size_t osz = out_bf16 ? 2 : 4;
    for (int n0 = 0; n0 < g.N; n0 += nc) {
        const int nn = g.N - n0 < nc ? g.N - n0 : nc;
        BfArgs a;
        a.x = reinterpret_cast<const float*>(reinterpret_cast<const char*>(x) + (size_t)n0 * per_sample);
        a.wn = wn; a.bias = bias;
        a.y = reinterpret_cast<float*>(reinterpret_cast<char*>(y) + (size_t)n0 * g.Ho * g.Wo * g.Cout * osz);
        a.N = nn; a.H = g.H; a.W = g.W; a.Cin = g.Cin; a.Ho = g.Ho; a.Wo = g.Wo; a.Cout = g.Cout;
        a.KH = g.KH; a.KW = g.KW; a.padT = g.padT; a.padL = g.padL;
        a.M = nn * g.Ho * g.Wo;
        a.nkt = g.KH * g.KW * (g.Cin / (operands_bf16 ? 64 : 32));
        a.mtiles = a.ntiles = 0;
        a.stat_part = stat_part;
        a.stat_mode = stat_mode;
        if (operands_bf16 && conv_bf16_halo_ok(g)) {
            // LDS-resident halo kernel (conv_bf16_halo.hip): one statistics block per 256-pixel patch
            BnBwdFuse bb;
            if (bn_bwd != nullptr) {         // the BatchNorm input of this sample range (bf16-stored: 2 bytes per element)
                bb = *bn_bwd;
                bb.x = reinterpret_cast<const float*>(reinterpret_cast<const char*>(bn_bwd->x) + (size_t)n0 * g.Ho * g.Wo * g.Cout * 2);
            }
            conv_bf16_halo_launch(a.x, wn, bias, a.y, g, nn, s, stat_part, stat_mode, out_bf16,
                                  bn_bwd != nullptr && stat_part != nullptr && out_bf16 ? &bb : nullptr);
            if (stat_part != nullptr) stat_part += (size_t)conv_bf16_halo_patches(g, nn) * 2 * g.Cout;
            continue;
        }
        if (operands_bf16) {
            if (g.Cout > 64)
                launch_bf16in<2, 2>(a, s, out_bf16);
            else
                launch_bf16in<4, 1>(a, s, out_bf16);
        } else if (g.Cout > 64) {
            launch_bf16<2, 2>(a, s);     // 128 x 128
        } else {
            launch_bf16<4, 1>(a, s);     // 256 x 64
        }
        if (stat_part != nullptr) stat_part += (size_t)((a.M + (g.Cout > 64 ? 128 : 256) - 1) / (g.Cout > 64 ? 128 : 256)) * 2 * g.Cout;
    }
}

}  // namespace l3
