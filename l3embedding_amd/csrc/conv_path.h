// conv_path.h -- the kernel path of ONE 2-D convolution: its geometry, which kernel its forward, weight gradient and data gradient
// take, and the launches of each path.  Host code only.  The engine (plan_tower / tower_forward / tower_backward_block), the
// operator entry points (ops.hip l3_op_conv2d_*, l3_op_vggish_conv) and the VGGish handle all come here, so a path is added or
// retired in conv_path.hip alone and the operators the tests call run the engine's own choice.
#pragma once
#include "kernels.h"

namespace l3 {

// Forward geometry of a stride-1 convolution ('same' as TensorFlow pads it, else 'valid').  f2x2: ConvGeom::f2x2.  solo, dynamic
// and tail_scratch* are per-pass settings: the caller writes them afterwards.
ConvGeom conv_geom(int n, int h, int w, int cin, int cout, int kh, int kw, bool same, int f2x2);
// Its data gradient = the stride-1 convolution of dY with the flipped / transposed filter: pad' = k - 1 - pad, channels swapped;
// f2x2 and solo carried over.
ConvGeom conv_dgrad_geom(const ConvGeom& g);

// What the caller's tensors are.  The resolvers read it and never decide it: an engine fixes its tensors' storage when it
// allocates them, an operator derives it from its `dtype` argument.
struct ConvStorage {
    bool mixed = false;                                               // mixed precision: bf16 operands, fp32 accumulate, where a kernel applies
    bool x_bf16 = false, y_bf16 = false, dy_bf16 = false, dx_bf16 = false;      // that tensor lives in HBM as bfloat16
};

enum ConvFwd { CF_BF16_STORED, CF_BF16_CAST, CF_FIRST, CF_FP32 };      // bf16 MFMA (operands stored bf16 / cast at fetch), FMA first layer, conv_fwd
enum ConvWgrad { WG_BF16_STORED, WG_BF16_CAST, WG_FP32 };
enum ConvDgrad { DG_NONE, DG_SMALL, DG_BF16_STORED, DG_BF16_CAST, DG_WINO, DG_FLIPPED };
// A resolved path with the flops its kernel issues (-1: the algorithmic count).
struct ConvFwdPath {
    ConvFwd path = CF_FP32;
    bool wino_filter = false;    // the filter is transformed into the Winograd domain first and conv_fwd is given it
    double executed = -1.0;
};
struct ConvWgradPath {
    ConvWgrad path = WG_FP32;
    double executed = -1.0;
};
struct ConvDgradPath {
    ConvDgrad path = DG_NONE;
    double executed = -1.0;
};
// The only callers of the kernels' predicates (and, through them, of the per-call debug knobs L3_WINO4, L3_CONV_FIRST,
// L3_BF16_HALO: a path holds for the pass it was resolved for).  have_u: the caller offers a buffer of conv_wino_floats() for the
// Winograd-domain filter; without one an fp32 convolution takes the direct implicit GEMM (VGGish's L3_VGGISH_CONV_DIRECT).
// g is the forward geometry everywhere, dg = conv_dgrad_geom(g).
ConvFwdPath conv_resolve_fwd(const ConvGeom& g, const ConvStorage& st, bool have_u);
ConvWgradPath conv_resolve_wgrad(const ConvGeom& g, const ConvStorage& st);
ConvDgradPath conv_resolve_dgrad(const ConvGeom& g, const ConvGeom& dg, const ConvStorage& st, bool have_u);
// Partial blocks of [2][Cout] the forward epilogue of a resolved path leaves in ConvBufs::stat_part for the BatchNorm behind it
// (0: that path writes no statistics -- the direct implicit GEMM, the cast-at-fetch bf16 kernel).
int conv_fwd_stat_blocks(const ConvFwdPath& p, const ConvGeom& g);
// Partial blocks of [2][dg.Cout] the data gradient's epilogue leaves for the backward reduction of the BatchNorm in front of the
// convolution (ConvBufs::bn_bwd), -1 where it does not fuse: the halo kernel on bf16-stored tensors (dx and the BatchNorm's
// input both bfloat16), the Winograd kernels on fp32 ones (both fp32).
int conv_dgrad_bn_blocks(const ConvDgradPath& p, const ConvGeom& dg, bool dx_bf16, bool bn_x_bf16);

// The device buffers of one launch.  A path reads only those it needs; the rest may be null.
struct ConvBufs {
    const float* x = nullptr;          // input (forward, weight gradient)
    const float* w = nullptr;          // the filter, fp32 HWIO
    const float* bias = nullptr;       // forward only
    float* y = nullptr;                // forward: the output.  Backward: dY
    float* dx = nullptr;
    float* dw = nullptr;
    float* wprep = nullptr;            // KH * KW * Cin * Cout floats: the flipped filter, or both bf16 layouts of conv_weights_bf16
    float* wino_u = nullptr;           // conv_wino_floats() of the launch's geometry
    bool u_ready = false;              // wino_u already holds the transform of w: skip it (a handle whose weights did not change)
    float* wg_part = nullptr;          // conv_wgrad_scratch_floats(g)
    float* stat_part = nullptr;        // forward: BatchNorm statistic partials (stat_mode 1 output, 2 relu(output)); data gradient:
    int stat_mode = 0;                 // ... the backward reduction partials of *bn_bwd
    const BnBwdFuse* bn_bwd = nullptr;
};
void conv_run_fwd(const ConvFwdPath& p, const ConvGeom& g, const ConvStorage& st, const ConvBufs& b, hipStream_t s);
void conv_run_wgrad(const ConvWgradPath& p, const ConvGeom& g, const ConvBufs& b, hipStream_t s);
void conv_run_dgrad(const ConvDgradPath& p, const ConvGeom& g, const ConvGeom& dg, const ConvStorage& st, const ConvBufs& b, hipStream_t s);

}  // namespace l3
