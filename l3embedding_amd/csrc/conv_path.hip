// conv_path.hip -- geometry, path resolution and path execution of one 2-D convolution (conv_path.h); host code only
#include "conv_path.h"

namespace l3 {

ConvGeom conv_geom(int n, int h, int w, int cin, int cout, int kh, int kw, bool same, int f2x2) {
    ConvGeom g{n, h, w, cin, 0, 0, cout, kh, kw, 0, 0};
    if (same) {
        tf_same(h, kh, 1, &g.Ho, &g.padT);
        tf_same(w, kw, 1, &g.Wo, &g.padL);
    } else {
        g.Ho = h - kh + 1;
        g.Wo = w - kw + 1;
    }
    g.f2x2 = f2x2;
    return g;
}

ConvGeom conv_dgrad_geom(const ConvGeom& g) {
    ConvGeom dg{g.N, g.Ho, g.Wo, g.Cout, g.H, g.W, g.Cin, g.KH, g.KW, g.KH - 1 - g.padT, g.KW - 1 - g.padL};
    dg.f2x2 = g.f2x2;
    dg.solo = g.solo;
    return dg;
}

ConvFwdPath conv_resolve_fwd(const ConvGeom& g, const ConvStorage& st, bool have_u) {
    ConvFwdPath p;
    const bool mp = st.mixed && conv_bf16_ok(g);      // mixed precision: bf16 operands, fp32 accumulate (conv_bf16.hip)
    p.path = mp ? (st.x_bf16 ? CF_BF16_STORED : CF_BF16_CAST) : conv_first_ok(g) ? CF_FIRST : CF_FP32;
    p.wino_filter = have_u && !mp && conv_wino_ok(g);
    p.executed = p.wino_filter ? conv_wino_executed_flops(g) : -1.0;
    return p;
}

ConvWgradPath conv_resolve_wgrad(const ConvGeom& g, const ConvStorage& st) {
    ConvWgradPath p;
    const bool wbf = st.mixed && conv_wgrad_bf16_ok(g);
    p.path = !wbf ? WG_FP32 : st.x_bf16 && st.dy_bf16 ? WG_BF16_STORED : WG_BF16_CAST;
    p.executed = conv_wgrad_executed_flops(g, wbf);
    return p;
}

ConvDgradPath conv_resolve_dgrad(const ConvGeom& g, const ConvGeom& dg, const ConvStorage& st, bool have_u) {
    ConvDgradPath p;
    const bool dbf = st.mixed && conv_bf16_ok(dg), wino = have_u && conv_wino_ok(dg);
    p.path = conv_dgrad_small_ok(g) ? DG_SMALL : dbf ? (st.dy_bf16 ? DG_BF16_STORED : DG_BF16_CAST) : wino ? DG_WINO : DG_FLIPPED;
    p.executed = wino && !dbf ? conv_wino_executed_flops(dg) : -1.0;
    return p;
}

int conv_fwd_stat_blocks(const ConvFwdPath& p, const ConvGeom& g) {
    return p.path == CF_BF16_STORED ? conv_bf16_stat_blocks(g)
           : p.path == CF_FIRST     ? conv_first_stat_blocks(g)
           : p.path == CF_FP32 && p.wino_filter ? conv_wino_stat_blocks(g) : 0;
}

int conv_dgrad_bn_blocks(const ConvDgradPath& p, const ConvGeom& dg, bool dx_bf16, bool bn_x_bf16) {
    int blocks = -1;
    if (p.path == DG_BF16_STORED && dx_bf16 && bn_x_bf16 && conv_bf16_halo_ok(dg)) blocks = conv_bf16_stat_blocks(dg);
    if (p.path == DG_WINO && !dx_bf16 && !bn_x_bf16 && conv_wino_ok(dg)) blocks = conv_wino_stat_blocks(dg);
    return blocks;
}

void conv_run_fwd(const ConvFwdPath& p, const ConvGeom& g, const ConvStorage& st, const ConvBufs& b, hipStream_t s) {
    if (p.wino_filter && !b.u_ready) conv_wino_transform_weights(b.w, b.wino_u, g, false, s);
    switch (p.path) {
        case CF_BF16_STORED:
            conv_weights_bf16(b.w, b.wprep, g.KH, g.KW, g.Cin, g.Cout, true, s);
            conv_bf16_fwd(b.x, b.wprep, b.bias, b.y, g, s, true, b.stat_part, b.stat_mode, st.y_bf16);
            break;
        case CF_BF16_CAST:
            conv_flip_weights(b.w, b.wprep, g.KH, g.KW, g.Cin, g.Cout, s);
            conv_bf16_fwd(b.x, b.wprep, b.bias, b.y, g, s);
            break;
        case CF_FIRST:      // FMA kernel with the statistics (and, bf16 storage, the bf16 store) fused
            conv_first_fwd(b.x, b.w, b.bias, b.y, g, s, b.stat_part, b.stat_mode, st.y_bf16);
            break;
        case CF_FP32:
            conv_fwd(b.x, b.w, b.bias, b.y, g, s, p.wino_filter ? b.wino_u : nullptr, b.stat_part, b.stat_mode);
            break;
    }
}

void conv_run_wgrad(const ConvWgradPath& p, const ConvGeom& g, const ConvBufs& b, hipStream_t s) {
    conv_wgrad(b.x, b.y, b.dw, b.wg_part, g, s, p.path != WG_FP32, p.path == WG_BF16_STORED);
}

void conv_run_dgrad(const ConvDgradPath& p, const ConvGeom& g, const ConvGeom& dg, const ConvStorage& st, const ConvBufs& b, hipStream_t s) {
    switch (p.path) {
        case DG_SMALL:
            (void)conv_dgrad_small(b.y, b.w, b.dx, g, s);
            break;
        case DG_BF16_STORED:       // filter cast once into the (now free) forward-operand buffer
            conv_weights_bf16(b.w, b.wprep, g.KH, g.KW, g.Cin, g.Cout, false, s);
            conv_bf16_fwd(b.y, b.wprep, nullptr, b.dx, dg, s, true, b.stat_part, 0, st.dx_bf16, b.bn_bwd);
            break;
        case DG_BF16_CAST:         // the forward filter is the data gradient's [flip][n][k]
            conv_bf16_fwd(b.y, b.w, nullptr, b.dx, dg, s);
            break;
        case DG_WINO:              // flip + transpose are folded into the transform: conv_fwd takes no spatial filter
            conv_wino_transform_weights(b.w, b.wino_u, dg, true, s);
            conv_fwd(b.y, nullptr, nullptr, b.dx, dg, s, b.wino_u, b.stat_part, 0, b.bn_bwd);
            break;
        case DG_FLIPPED:
            conv_flip_weights(b.w, b.wprep, g.KH, g.KW, g.Cin, g.Cout, s);
            conv_fwd(b.y, b.wprep, nullptr, b.dx, dg, s);
            break;
        case DG_NONE: break;
    }
}

}  // namespace l3
