// ops.hip -- stand-alone operator entry points of the C ABI (host buffers in/out).
// They run the kernels the engine uses -- the convolutions through the engine's own path resolution and launches (conv_path.h) --
// and exist for the op-level parity tests in tests/ (each op replaces a TF op instantiated by a Keras/kapre layer,
// SURVEY.md section 2.3).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/l3hip.h"
#include "conv_path.h"
#include "kernels.h"
#include "knobs.h"
#include "mlp.h"
#include "vggish.h"

namespace {
using namespace l3;

struct Scope {
    DeviceBufs bufs;
    hipStream_t s = nullptr;
    bool ok = true;
    explicit Scope(int device) : ok(device_ok(device)) {}
    ~Scope() { (void)hipDeviceSynchronize(); }          // before bufs frees
    template <class T>
    T* alloc(size_t count) {
        T* p = bufs.alloc<T>(count);
        if (!p) ok = false;
        return p;
    }
    template <class T>
    T* put(const T* host, size_t count) {
        T* d = alloc<T>(count);
        if (d && host && hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) ok = false;
        return d;
    }
    template <class T>
    void get(T* host, const T* dev, size_t count) {
        if (!host) return;
        if (hipDeviceSynchronize() != hipSuccess) ok = false;
        if (hipMemcpy(host, dev, count * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) ok = false;
    }
    // `dev` holds count floats, or (bf16) count bfloat16 values: returned widened, every value a bfloat16
    void get_stored(float* host, const float* dev, size_t count, bool bf16) {
        if (!bf16) return get(host, dev, count);
        std::vector<uint16_t> h16(count);
        get(h16.data(), reinterpret_cast<const uint16_t*>(dev), count);
        if (host) widen_bf16(host, h16.data(), count);
    }
    int status() {
        if (hipDeviceSynchronize() != hipSuccess) ok = false;
        if (hipGetLastError() != hipSuccess) ok = false;
        return ok ? L3_OK : L3_EHIP;
    }
};

ConvGeom make_geom(int n, int h, int w, int cin, int cout, int kh, int kw, int same) {
    const char* algo = l3_knob("L3_FP32_CONV");          // the tests run every l3_config.fp32_conv value through the operators
    ConvGeom g = conv_geom(n, h, w, cin, cout, kh, kw, same != 0,
                           algo == nullptr ? 0 : strcmp(algo, "f2x2_bf16x6") == 0 ? 2 : strcmp(algo, "f2x2") == 0 ? 1 : 0);
    g.solo = 1;          // an operator on its own: nothing queued beside it
    return g;
}

PoolGeom make_pool(int n, int h, int w, int c, int ph, int pw, int sh, int sw, int same) {
    PoolGeom g{n, h, w, c, 0, 0, ph, pw, sh, sw, 0, 0, 0};
    if (same) {
        tf_same(h, ph, sh, &g.Ho, &g.padT);
        tf_same(w, pw, sw, &g.Wo, &g.padL);
    } else {
        g.Ho = (h - ph) / sh + 1;
        g.Wo = (w - pw) / sw + 1;
    }
    g.out_batch_stride = (int64_t)g.Ho * g.Wo * c;
    return g;
}
}  // namespace

extern "C" {

// Upload, map `dtype` to the tensors' storage, resolve as the engine does (conv_path.h), run, download.  L3_OP_BF16_STORED(_OUT):
// bfloat16 in HBM as alloc_everything lays a mixed-precision layer out -- x where the bf16 kernel reads it, y (_OUT; returned
// widened) where that kernel or the first-layer kernel writes it.
int l3_op_conv2d_fwd_dt(int device, int dtype, const float* x, const float* w, const float* b, float* y, int n, int h,
                        int wd, int cin, int cout, int kh, int kw, int same) {
    Scope sc(device);
    if (!sc.ok) return L3_EHIP;
    const ConvGeom g = make_geom(n, h, wd, cin, cout, kh, kw, same);
    const size_t nx = (size_t)n * h * wd * cin, nw = (size_t)kh * kw * cin * cout, ny = (size_t)n * g.Ho * g.Wo * cout;
    const bool stored = dtype == L3_OP_BF16_STORED || dtype == L3_OP_BF16_STORED_OUT;
    ConvStorage st;
    st.mixed = dtype != L3_DTYPE_F32;
    st.x_bf16 = stored && conv_bf16_ok(g);
    const ConvFwdPath p = conv_resolve_fwd(g, st, conv_wino_floats(g) != 0);
    st.y_bf16 = dtype == L3_OP_BF16_STORED_OUT && (p.path == CF_BF16_STORED || p.path == CF_FIRST);
    ConvBufs cb;
    float* d_x = sc.put(x, nx);
    cb.x = d_x;
    cb.w = sc.put(w, nw);
    cb.bias = b ? sc.put(b, (size_t)cout) : nullptr;
    cb.y = sc.alloc<float>(ny);
    cb.wprep = sc.alloc<float>(nw);
    cb.wino_u = p.wino_filter ? sc.alloc<float>(conv_wino_floats(g)) : nullptr;
    uint16_t* xb = st.x_bf16 ? sc.alloc<uint16_t>(nx) : nullptr;
    if (!sc.ok) return L3_ENOMEM;
    if (st.x_bf16) {
        cast_bf16(d_x, xb, (int64_t)nx, sc.s);
        cb.x = reinterpret_cast<const float*>(xb);
    }
    conv_run_fwd(p, g, st, cb, sc.s);
    sc.get_stored(y, cb.y, ny, st.y_bf16);
    return sc.status();
}

int l3_op_conv2d_fwd(int device, const float* x, const float* w, const float* b, float* y, int n, int h, int wd,
                     int cin, int cout, int kh, int kw, int same) {
    return l3_op_conv2d_fwd_dt(device, L3_DTYPE_F32, x, w, b, y, n, h, wd, cin, cout, kh, kw, same);
}

// As the forward: bfloat16-stored operands (x, dy; _OUT: dx too, returned widened) where the engine keeps them so, i.e. where
// both gradients of the layer take a bf16 kernel; the bias gradient stays a plain fp32 column sum of the unrounded dy.
int l3_op_conv2d_bwd_dt(int device, int dtype, const float* x, const float* w, const float* dy, float* dx, float* dw,
                        float* db, int n, int h, int wd, int cin, int cout, int kh, int kw, int same) {
    Scope sc(device);
    if (!sc.ok) return L3_EHIP;
    const ConvGeom g = make_geom(n, h, wd, cin, cout, kh, kw, same), dg = conv_dgrad_geom(g);
    const size_t nx = (size_t)n * h * wd * cin, ny = (size_t)n * g.Ho * g.Wo * cout, nw = (size_t)kh * kw * cin * cout;
    const bool stored = (dtype == L3_OP_BF16_STORED || dtype == L3_OP_BF16_STORED_OUT) && conv_wgrad_bf16_ok(g) && conv_bf16_ok(dg);
    ConvStorage st;
    st.mixed = dtype != L3_DTYPE_F32;
    st.x_bf16 = st.dy_bf16 = stored;
    st.dx_bf16 = stored && dtype == L3_OP_BF16_STORED_OUT;
    const ConvWgradPath pw = conv_resolve_wgrad(g, st);
    const ConvDgradPath pd = conv_resolve_dgrad(g, dg, st, conv_wino_floats(dg) != 0);
    ConvBufs cb;
    float* d_x = sc.put(x, nx);
    float* d_dy = sc.put(dy, ny);
    cb.x = d_x;
    cb.y = d_dy;
    cb.w = sc.put(w, nw);
    cb.dx = sc.alloc<float>(nx);
    cb.dw = sc.alloc<float>(nw);
    cb.wprep = sc.alloc<float>(nw);
    cb.wino_u = pd.path == DG_WINO ? sc.alloc<float>(conv_wino_floats(dg)) : nullptr;
    cb.wg_part = sc.alloc<float>(conv_wgrad_scratch_floats(g));
    float* d_db = sc.alloc<float>((size_t)cout);
    float* d_red = sc.alloc<float>(colreduce_scratch_floats((int64_t)n * g.Ho * g.Wo, cout));
    uint16_t* xb = stored ? sc.alloc<uint16_t>(nx) : nullptr;
    uint16_t* gb = stored ? sc.alloc<uint16_t>(ny) : nullptr;
    if (!sc.ok) return L3_ENOMEM;
    if (stored) {
        cast_bf16(d_x, xb, (int64_t)nx, sc.s);
        cast_bf16(d_dy, gb, (int64_t)ny, sc.s);
        cb.x = reinterpret_cast<const float*>(xb);
        cb.y = reinterpret_cast<float*>(gb);
    }
    conv_run_wgrad(pw, g, cb, sc.s);
    colsum(d_dy, d_db, d_red, (int64_t)n * g.Ho * g.Wo, cout, sc.s);
    conv_run_dgrad(pd, g, dg, st, cb, sc.s);
    sc.get_stored(dx, cb.dx, nx, st.dx_bf16);
    sc.get(dw, cb.dw, nw);
    sc.get(db, d_db, (size_t)cout);
    return sc.status();
}

int l3_op_conv2d_bwd(int device, const float* x, const float* w, const float* dy, float* dx, float* dw, float* db,
                     int n, int h, int wd, int cin, int cout, int kh, int kw, int same) {
    return l3_op_conv2d_bwd_dt(device, L3_DTYPE_F32, x, w, dy, dx, dw, db, n, h, wd, cin, cout, kh, kw, same);
}

int l3_op_bn_relu_fwd(int device, const float* x, const float* gamma, const float* beta, float* y, float* mean,
                      float* var, int64_t rows, int c, int relu, int x_bf16) {
    Scope sc(device);
    if (!sc.ok) return L3_EHIP;
    const bool obf = (x_bf16 & 4) != 0;          // y stored as bfloat16 (returned widened): the fast kernels for either input form
    if ((x_bf16 & 5) && !bn_fast_ok(c)) return L3_EINVAL;
    const size_t n = (size_t)rows * c, cp = (size_t)(c + 3) / 4 * 4;
    float* d_x = sc.put(x, n);
    float* d_g = sc.alloc<float>(cp);
    float* d_b = sc.alloc<float>(cp);
    float *d_m = sc.alloc<float>(cp), *d_v = sc.alloc<float>(cp), *d_sc = sc.alloc<float>(cp), *d_sh = sc.alloc<float>(cp);
    float* d_y = sc.alloc<float>(n);
    float* d_red = sc.alloc<float>(colreduce_scratch_floats(rows, c));
    if (!sc.ok) return L3_ENOMEM;
    (void)hipMemcpy(d_g, gamma, c * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(d_b, beta, c * 4, hipMemcpyHostToDevice);
    if (x_bf16 & 1) {  // x as a mixed-precision conv leaves it: bfloat16 in HBM
        uint16_t* xb = sc.alloc<uint16_t>(n);
        if (!sc.ok) return L3_ENOMEM;
        cast_bf16(d_x, xb, (int64_t)n, sc.s);
        bn_stats_fast(reinterpret_cast<const float*>(xb), d_g, d_b, d_m, d_v, d_sc, d_sh, d_red, rows, c, 1e-3f, 0, sc.s, 1);
        bn_apply_fast(reinterpret_cast<const float*>(xb), d_sc, d_sh, d_y, rows, c, relu, sc.s, obf ? 1 : 0, 1);
    } else if (obf) {
        bn_stats_fast(d_x, d_g, d_b, d_m, d_v, d_sc, d_sh, d_red, rows, c, 1e-3f, 0, sc.s, 0);
        bn_apply_fast(d_x, d_sc, d_sh, d_y, rows, c, relu, sc.s, 1, 0);
    } else {
        bn_stats(d_x, d_g, d_b, d_m, d_v, d_sc, d_sh, d_red, rows, c, 1e-3f, sc.s);
        bn_apply(d_x, d_sc, d_sh, d_y, rows, c, relu, sc.s);
    }
    sc.get_stored(y, d_y, n, obf);
    sc.get(mean, d_m, (size_t)c);
    sc.get(var, d_v, (size_t)c);
    return sc.status();
}

int l3_op_bn_relu_bwd(int device, const float* x, const float* y, const float* dy, const float* gamma,
                      const float* beta, const float* mean, const float* var, float* dx, float* dgamma, float* dbeta,
                      int64_t rows, int c, int relu, int x_bf16) {
    Scope sc(device);
    if (!sc.ok) return L3_EHIP;
    const size_t n = (size_t)rows * c, cp = (size_t)(c + 3) / 4 * 4;
    float* d_x = sc.put(x, n);
    float* d_y = sc.put(y, n);
    float* d_dy = sc.put(dy, n);
    float *d_g = sc.alloc<float>(cp), *d_m = sc.alloc<float>(cp), *d_v = sc.alloc<float>(cp);
    float *d_dg = sc.alloc<float>(cp), *d_db = sc.alloc<float>(cp);
    float* d_dx = sc.alloc<float>(n);
    const bool fast = beta != nullptr && bn_fast_ok(c) && rows < (int64_t)1 << 30;
    if (x_bf16 && !fast) return L3_EINVAL;
    const bool obf = (x_bf16 & 4) != 0;          // dx stored as bfloat16 (returned widened)
    size_t red = colreduce_scratch_floats(rows, c);
    if (fast && bn_fast_scratch_floats(c) > red) red = bn_fast_scratch_floats(c);
    float* d_red = sc.alloc<float>(red);
    if (!sc.ok) return L3_ENOMEM;
    (void)hipMemcpy(d_g, gamma, c * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(d_m, mean, c * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(d_v, var, c * 4, hipMemcpyHostToDevice);
    if (fast) {
        // the engine's dispatch for power-of-two channel counts: ReLU mask recomputed from x*scale+shift
        float *d_b = sc.put(beta, (size_t)c), *d_sc = sc.alloc<float>(cp), *d_sh = sc.alloc<float>(cp);
        if (!sc.ok) return L3_ENOMEM;
        bn_scale_shift(d_g, d_b, d_m, d_v, d_sc, d_sh, c, 1e-3f, sc.s);
        const float* xin = d_x;
        const float* dyin = d_dy;
        if (x_bf16 & 1) {
            uint16_t* xb = sc.alloc<uint16_t>(n);
            if (!sc.ok) return L3_ENOMEM;
            cast_bf16(d_x, xb, (int64_t)n, sc.s);
            xin = reinterpret_cast<const float*>(xb);
        }
        if (x_bf16 & 2) {       // dy as the mixed-precision data-gradient kernel leaves it: bfloat16 in HBM
            uint16_t* gb = sc.alloc<uint16_t>(n);
            if (!sc.ok) return L3_ENOMEM;
            cast_bf16(d_dy, gb, (int64_t)n, sc.s);
            dyin = reinterpret_cast<const float*>(gb);
        }
        bn_bwd_fast(xin, d_sc, d_sh, d_m, d_v, d_g, dyin, 0, 1, 1, (int)rows, c, 1, (int)rows, (int64_t)rows * c, d_dx, d_dg,
                    d_db, nullptr, d_red, 1e-3f, relu, 1, sc.s, obf ? 1 : 0, (x_bf16 & 1) ? 1 : 0, (x_bf16 & 2) ? 1 : 0);
    } else {
        bn_bwd(d_x, d_y, d_dy, d_g, d_m, d_v, d_dx, d_dg, d_db, d_red, rows, c, 1e-3f, relu, 1, sc.s);
    }
    sc.get_stored(dx, d_dx, n, obf);
    sc.get(dgamma, d_dg, (size_t)c);
    sc.get(dbeta, d_db, (size_t)c);
    return sc.status();
}

static int pool2_common(int device, const float* x, const float* gamma, const float* beta, const float* dp, float* p,
                        float* mean, float* var, float* dx, float* dgamma, float* dbeta, float* dbias, int n, int h,
                        int wd, int c, int same, int mode, int x_bf16, float* xwin = nullptr) {
    if (!bn_fast_ok(c) || (mode != 1 && mode != 2)) return L3_EINVAL;
    Scope sc(device);
    if (!sc.ok) return L3_EHIP;
    const PoolGeom g = make_pool(n, h, wd, c, 2, 2, 2, 2, same);
    const size_t nx = (size_t)n * h * wd * c, np_ = (size_t)n * g.Ho * g.Wo * c;
    const bool obf = (x_bf16 & 4) != 0;          // p (forward) / dx (backward) stored as bfloat16, returned widened
    float* d_x = sc.put(x, nx);
    float* d_g = sc.put(gamma, (size_t)c);
    float* d_b = sc.put(beta, (size_t)c);
    float *d_m = sc.alloc<float>(c), *d_v = sc.alloc<float>(c), *d_sc = sc.alloc<float>(c), *d_sh = sc.alloc<float>(c);
    float* d_p = sc.alloc<float>(np_);
    float* d_red = sc.alloc<float>(colreduce_scratch_floats((int64_t)n * h * wd, c));
    if (!sc.ok) return L3_ENOMEM;
    if (x_bf16 & 1) {  // x as a mixed-precision conv leaves it: bfloat16 in HBM
        uint16_t* xb = sc.alloc<uint16_t>(nx);
        if (!sc.ok) return L3_ENOMEM;
        cast_bf16(d_x, xb, (int64_t)nx, sc.s);
        d_x = reinterpret_cast<float*>(xb);
    }
    if (mode == 2 || (x_bf16 & 1))      // mode 2 = ReLU -> BN (vision_model.py:138-139): moments of relu(x)
        bn_stats_fast(d_x, d_g, d_b, d_m, d_v, d_sc, d_sh, d_red, (int64_t)n * h * wd, c, 1e-3f, mode == 2 ? 1 : 0, sc.s, x_bf16 & 1);
    else
        bn_stats(d_x, d_g, d_b, d_m, d_v, d_sc, d_sh, d_red, (int64_t)n * h * wd, c, 1e-3f, sc.s);
    float* d_win = xwin ? sc.alloc<float>(np_) : nullptr;      // the window winners, in x's storage type (the training forward)
    if (!sc.ok) return L3_ENOMEM;
    bn_relu_pool2_fwd(d_x, d_sc, d_sh, d_p, n, h, wd, c, g.Ho, g.Wo, g.out_batch_stride, mode, sc.s, obf ? 1 : 0, x_bf16 & 1, d_win);
    sc.get_stored(p, d_p, np_, obf);
    if (xwin) sc.get_stored(xwin, d_win, np_, (x_bf16 & 1) != 0);
    sc.get(mean, d_m, (size_t)c);
    sc.get(var, d_v, (size_t)c);
    if (dp) {
        float* d_dp = sc.put(dp, np_);
        if (x_bf16 & 2) {   // the pooled gradient as the mixed-precision data-gradient kernel leaves it: bfloat16 in HBM
            uint16_t* gb = sc.alloc<uint16_t>(np_);
            if (!sc.ok) return L3_ENOMEM;
            cast_bf16(d_dp, gb, (int64_t)np_, sc.s);
            d_dp = reinterpret_cast<float*>(gb);
        }
        float* d_dx = sc.alloc<float>(nx);
        float *d_dg = sc.alloc<float>(c), *d_db = sc.alloc<float>(c), *d_dbias = sc.alloc<float>(c);
        if (!sc.ok) return L3_ENOMEM;
        bn_bwd_fast(d_x, d_sc, d_sh, d_m, d_v, d_g, d_dp, 1, n, h, wd, c, g.Ho, g.Wo, g.out_batch_stride, d_dx, d_dg,
                    d_db, d_dbias, d_red, 1e-3f, mode, 1, sc.s, obf ? 1 : 0, x_bf16 & 1, (x_bf16 & 2) ? 1 : 0);
        sc.get_stored(dx, d_dx, nx, obf);
        sc.get(dgamma, d_dg, (size_t)c);
        sc.get(dbeta, d_db, (size_t)c);
        sc.get(dbias, d_dbias, (size_t)c);
    }
    return sc.status();
}

int l3_op_bn_relu_pool2_fwd(int device, const float* x, const float* gamma, const float* beta, float* p, float* mean,
                            float* var, int n, int h, int wd, int c, int same, int relu_mode, int x_bf16) {
    return pool2_common(device, x, gamma, beta, nullptr, p, mean, var, nullptr, nullptr, nullptr, nullptr, n, h, wd, c,
                        same, relu_mode, x_bf16);
}

int l3_op_bn_relu_pool2_fwd_xwin(int device, const float* x, const float* gamma, const float* beta, float* p, float* mean,
                                 float* var, float* xwin, int n, int h, int wd, int c, int same, int relu_mode, int x_bf16) {
    if (!xwin) return L3_EINVAL;
    return pool2_common(device, x, gamma, beta, nullptr, p, mean, var, nullptr, nullptr, nullptr, nullptr, n, h, wd, c,
                        same, relu_mode, x_bf16, xwin);
}

int l3_op_bn_relu_pool2_bwd(int device, const float* x, const float* gamma, const float* beta, const float* dp,
                            float* dx, float* dgamma, float* dbeta, float* dbias, int n, int h, int wd, int c, int same,
                            int relu_mode, int x_bf16) {
    return pool2_common(device, x, gamma, beta, dp, nullptr, nullptr, nullptr, dx, dgamma, dbeta, dbias, n, h, wd, c,
                        same, relu_mode, x_bf16);
}

int l3_op_maxpool_fwd(int device, const float* x, float* y, int n, int h, int wd, int c, int ph, int pw, int sh,
                      int sw, int same) {
    Scope sc(device);
    if (!sc.ok) return L3_EHIP;
    const PoolGeom g = make_pool(n, h, wd, c, ph, pw, sh, sw, same);
    float* d_x = sc.put(x, (size_t)n * h * wd * c);
    float* d_y = sc.alloc<float>((size_t)n * g.Ho * g.Wo * c);
    if (!sc.ok) return L3_ENOMEM;
    maxpool_fwd(d_x, d_y, g, sc.s);
    sc.get(y, d_y, (size_t)n * g.Ho * g.Wo * c);
    return sc.status();
}

int l3_op_maxpool_bwd(int device, const float* x, const float* dy, float* dx, int n, int h, int wd, int c, int ph,
                      int pw, int sh, int sw, int same) {
    Scope sc(device);
    if (!sc.ok) return L3_EHIP;
    if (sh < ph || sw < pw) return L3_EINVAL;
    const PoolGeom g = make_pool(n, h, wd, c, ph, pw, sh, sw, same);
    float* d_x = sc.put(x, (size_t)n * h * wd * c);
    float* d_dy = sc.put(dy, (size_t)n * g.Ho * g.Wo * c);
    float* d_dx = sc.alloc<float>((size_t)n * h * wd * c);
    if (!sc.ok) return L3_ENOMEM;
    maxpool_bwd(d_x, d_dy, d_dx, g, sc.s);
    sc.get(dx, d_dx, (size_t)n * h * wd * c);
    return sc.status();
}

// BatchNormalization batch moments from the partial sums a convolution epilogue leaves (`nblk` rows of [sum, sum of squares][c]
// about `pivot`): the engine's stage 2 (bn_fused.hip launch_fast_final, its fp64 pre-reduction above 2048 rows included) on a
// buffer of EXACTLY nblk rows followed by a guard region, which must come back untouched (L3_EINVAL otherwise).
int l3_op_bn_stats_from_partials(int device, const float* part, int nblk, int c, const float* pivot, int64_t rows, float eps,
                                 float* mean, float* var) {
    Scope sc(device);
    if (!sc.ok) return L3_EHIP;
    if (nblk < 1 || c < 4 || c % 4) return L3_EINVAL;
    const size_t n = (size_t)nblk * 2 * c, guard = (size_t)8 * c;
    std::vector<float> host(n + guard);
    memcpy(host.data(), part, n * sizeof(float));
    for (size_t i = 0; i < guard; ++i) host[n + i] = -12345.f;
    float* d_part = sc.put(host.data(), n + guard);
    float* d_pivot = sc.put(pivot, (size_t)c);
    std::vector<float> ones((size_t)c, 1.f), zeros((size_t)c, 0.f);
    float* d_gamma = sc.put(ones.data(), (size_t)c);
    float* d_beta = sc.put(zeros.data(), (size_t)c);
    float* d_mean = sc.alloc<float>((size_t)c);
    float* d_var = sc.alloc<float>((size_t)c);
    float* d_scale = sc.alloc<float>((size_t)c);
    float* d_shift = sc.alloc<float>((size_t)c);
    if (!sc.ok) return L3_ENOMEM;
    bn_stats_from_partials(d_part, nblk, d_pivot, d_gamma, d_beta, d_mean, d_var, d_scale, d_shift, rows, c, eps, 0, sc.s);
    sc.get(mean, d_mean, (size_t)c);
    sc.get(var, d_var, (size_t)c);
    sc.get(host.data() + n, d_part + n, guard);
    for (size_t i = 0; i < guard; ++i)
        if (host[n + i] != -12345.f) return L3_EINVAL;
    return sc.status();
}

}  // extern "C"

// ---- what the convolution epilogues leave for the BatchNorm beside them, on its own ------------------------------------------------
namespace {
// The partial buffer of an epilogue under test: EXACTLY nblk blocks of [2][c], NaN before the launch (a block the kernel does not
// write stays NaN), and a guard of max(nblk, 8) further blocks of a sentinel behind them (a kernel that writes more blocks than
// conv_path.h counts changes it).
struct GuardedPartials {
    static constexpr float SENTINEL = -12345.f;
    size_t n = 0, guard = 0, row = 0;
    float* dev = nullptr;
    std::vector<float> host;
    GuardedPartials(Scope& sc, int nblk, int c) {
        row = (size_t)2 * c;
        n = (size_t)nblk * 2 * c;
        guard = (size_t)(nblk > 8 ? nblk : 8) * 2 * c;
        host.assign(n + guard, SENTINEL);
        uint32_t nan_bits = 0x7fc00000u;
        float nan;
        memcpy(&nan, &nan_bits, sizeof nan);
        for (size_t i = 0; i < n; ++i) host[i] = nan;
        dev = sc.put(host.data(), n + guard);
    }
    // after the launch that fills them (and BEFORE stage 2, which may reduce in place): download, check, hand out
    int fetch(Scope& sc, const char* name, float* part) {
        sc.get(host.data(), dev, n + guard);
        if (!sc.ok) return L3_EHIP;
        if (const int rc = guard_check(name)) return rc;
        for (size_t i = 0; i < n; ++i)
            if (host[i] != host[i]) {
                set_op_error(std::string(name) + ": the epilogue left partial block " + std::to_string(i / row) + " unwritten");
                return L3_EINVAL;
            }
        if (part) memcpy(part, host.data(), n * sizeof(float));
        return L3_OK;
    }
    // after stage 2: the guard once more
    int recheck(Scope& sc, const char* name) {
        sc.get(host.data() + n, dev + n, guard);
        if (!sc.ok) return L3_EHIP;
        return guard_check(name);
    }
    int guard_check(const char* name) {
        for (size_t i = 0; i < guard; ++i)
            if (host[n + i] != SENTINEL) {
                set_op_error(std::string(name) + ": float " + std::to_string(i) + " of the guard behind the partial blocks changed");
                return L3_EINVAL;
            }
        return L3_OK;
    }
};
}  // namespace

extern "C" {

// The forward of l3_op_conv2d_fwd_dt with the BatchNorm statistics of its epilogue: same storage, same resolution, same launch,
// ConvBufs::stat_part / stat_mode set as tower_forward sets them; then the engine's stage 2 with pivot = bias.
int l3_op_conv2d_fwd_stats(int device, int dtype, const float* x, const float* w, const float* b, float* y, float* part, int* nblk,
                           float* mean, float* var, int n, int h, int wd, int cin, int cout, int kh, int kw, int same,
                           int stat_mode) {
    const char* name = "l3_op_conv2d_fwd_stats";
    if (!nblk || (stat_mode != 1 && stat_mode != 2)) {
        set_op_error(std::string(name) + ": NULL nblk or a stat_mode other than 1 (output) and 2 (relu(output))");
        return L3_EINVAL;
    }
    const ConvGeom g = make_geom(n, h, wd, cin, cout, kh, kw, same);
    const size_t nx = (size_t)n * h * wd * cin, nw = (size_t)kh * kw * cin * cout, ny = (size_t)n * g.Ho * g.Wo * cout;
    const bool stored = dtype == L3_OP_BF16_STORED || dtype == L3_OP_BF16_STORED_OUT;
    ConvStorage st;
    st.mixed = dtype != L3_DTYPE_F32;
    st.x_bf16 = stored && conv_bf16_ok(g);
    const ConvFwdPath p = conv_resolve_fwd(g, st, conv_wino_floats(g) != 0);
    st.y_bf16 = dtype == L3_OP_BF16_STORED_OUT && (p.path == CF_BF16_STORED || p.path == CF_FIRST);
    const int blocks = conv_fwd_stat_blocks(p, g);
    if (blocks <= 0) {
        set_op_error(std::string(name) + ": the resolved forward path leaves no statistics");
        return L3_EINVAL;
    }
    *nblk = blocks;
    if (!part) return L3_OK;           // the query form: how many blocks to bring
    if (!x || !w || !b || !y || !mean || !var) {
        set_op_error(std::string(name) + ": NULL pointer (the bias is the pivot of the sums)");
        return L3_EINVAL;
    }
    Scope sc(device);
    if (!sc.ok) return L3_EHIP;
    ConvBufs cb;
    float* d_x = sc.put(x, nx);
    cb.x = d_x;
    cb.w = sc.put(w, nw);
    cb.bias = sc.put(b, (size_t)cout);
    cb.y = sc.alloc<float>(ny);
    cb.wprep = sc.alloc<float>(nw);
    cb.wino_u = p.wino_filter ? sc.alloc<float>(conv_wino_floats(g)) : nullptr;
    uint16_t* xb = st.x_bf16 ? sc.alloc<uint16_t>(nx) : nullptr;
    GuardedPartials gp(sc, blocks, cout);
    std::vector<float> ones((size_t)cout, 1.f), zeros((size_t)cout, 0.f);
    float* d_gamma = sc.put(ones.data(), (size_t)cout);
    float* d_beta = sc.put(zeros.data(), (size_t)cout);
    float *d_mean = sc.alloc<float>((size_t)cout), *d_var = sc.alloc<float>((size_t)cout);
    float *d_scale = sc.alloc<float>((size_t)cout), *d_shift = sc.alloc<float>((size_t)cout);
    if (!sc.ok) return L3_ENOMEM;
    if (st.x_bf16) {
        cast_bf16(d_x, xb, (int64_t)nx, sc.s);
        cb.x = reinterpret_cast<const float*>(xb);
    }
    cb.stat_part = gp.dev, cb.stat_mode = stat_mode;
    conv_run_fwd(p, g, st, cb, sc.s);
    sc.get_stored(y, cb.y, ny, st.y_bf16);
    if (const int rc = gp.fetch(sc, name, part)) return rc;
    bn_stats_from_partials(gp.dev, blocks, cb.bias, d_gamma, d_beta, d_mean, d_var, d_scale, d_shift, (int64_t)n * g.Ho * g.Wo, cout,
                           1e-3f, stat_mode == 2 ? 1 : 0, sc.s);
    sc.get(mean, d_mean, (size_t)cout);
    sc.get(var, d_var, (size_t)cout);
    if (const int rc = gp.recheck(sc, name)) return rc;
    return sc.status();
}

// The data gradient of l3_op_conv2d_bwd_dt with the backward reduction of the BatchNorm(+ReLU) in FRONT of the convolution in its
// epilogue (BnBwdFuse): n, h, wd, cin, cout are the FORWARD convolution's, so dy is (n, Ho, Wo, cout) and dx, bn_x are
// (n, h, wd, cin); gamma, beta, mean, var have cin channels.  L3_DTYPE_F32: the Winograd kernels on fp32 tensors;
// L3_OP_BF16_STORED_OUT: the halo kernel with dy, bn_x and dx bfloat16-stored.  Then bn_bwd_fast's stage 2 alone (dx = NULL).
int l3_op_conv2d_dgrad_bn_bwd(int device, int dtype, const float* dy, const float* w, const float* bn_x, const float* gamma,
                              const float* beta, const float* mean, const float* var, float* dx, float* part, int* nblk,
                              float* dgamma, float* dbeta, int n, int h, int wd, int cin, int cout, int kh, int kw, int same,
                              int relu, int64_t bn_rows) {
    const char* name = "l3_op_conv2d_dgrad_bn_bwd";
    if (!nblk || (dtype != L3_DTYPE_F32 && dtype != L3_OP_BF16_STORED_OUT) || bn_rows < 1 || bn_rows >= (int64_t)1 << 30) {
        set_op_error(std::string(name) + ": NULL nblk, a dtype other than f32 / bf16_stored_out, or bn_rows outside [1, 2^30)");
        return L3_EINVAL;
    }
    const ConvGeom g = make_geom(n, h, wd, cin, cout, kh, kw, same), dg = conv_dgrad_geom(g);
    const size_t nx = (size_t)n * h * wd * cin, ny = (size_t)n * g.Ho * g.Wo * cout, nw = (size_t)kh * kw * cin * cout;
    const bool stored = dtype == L3_OP_BF16_STORED_OUT && conv_bf16_ok(dg);
    ConvStorage st;
    st.mixed = dtype != L3_DTYPE_F32;
    st.dy_bf16 = st.dx_bf16 = stored;
    const ConvDgradPath pd = conv_resolve_dgrad(g, dg, st, conv_wino_floats(dg) != 0);
    const int blocks = bn_fast_ok(cin) ? conv_dgrad_bn_blocks(pd, dg, st.dx_bf16, stored) : -1;
    if (blocks <= 0) {
        set_op_error(std::string(name) + ": the engine would not leave this BatchNorm's reduction to this data gradient");
        return L3_EINVAL;
    }
    *nblk = blocks;
    if (!part) return L3_OK;           // the query form
    if (!dy || !w || !bn_x || !gamma || !beta || !mean || !var || !dx || !dgamma || !dbeta) {
        set_op_error(std::string(name) + ": NULL pointer");
        return L3_EINVAL;
    }
    Scope sc(device);
    if (!sc.ok) return L3_EHIP;
    ConvBufs cb;
    float* d_dy = sc.put(dy, ny);
    float* d_bx = sc.put(bn_x, nx);
    cb.y = d_dy;
    cb.w = sc.put(w, nw);
    cb.dx = sc.alloc<float>(nx);
    cb.wprep = sc.alloc<float>(nw);
    cb.wino_u = pd.path == DG_WINO ? sc.alloc<float>(conv_wino_floats(dg)) : nullptr;
    float *d_g = sc.put(gamma, (size_t)cin), *d_b = sc.put(beta, (size_t)cin), *d_m = sc.put(mean, (size_t)cin), *d_v = sc.put(var, (size_t)cin);
    float *d_sc = sc.alloc<float>((size_t)cin), *d_sh = sc.alloc<float>((size_t)cin);
    float *d_dg = sc.alloc<float>((size_t)cin), *d_db = sc.alloc<float>((size_t)cin);
    float* d_red = sc.alloc<float>(bn_fast_scratch_floats(cin));
    uint16_t* gb = stored ? sc.alloc<uint16_t>(ny) : nullptr;
    uint16_t* xb = stored ? sc.alloc<uint16_t>(nx) : nullptr;
    GuardedPartials gp(sc, blocks, cin);
    if (!sc.ok) return L3_ENOMEM;
    const float* bx = d_bx;
    if (stored) {
        cast_bf16(d_dy, gb, (int64_t)ny, sc.s);
        cast_bf16(d_bx, xb, (int64_t)nx, sc.s);
        cb.y = reinterpret_cast<float*>(gb);
        bx = reinterpret_cast<const float*>(xb);
    }
    bn_scale_shift(d_g, d_b, d_m, d_v, d_sc, d_sh, cin, 1e-3f, sc.s);
    const BnBwdFuse bb{bx, d_sc, d_sh, d_m, d_v, 1e-3f, relu ? 1 : 0};
    cb.bn_bwd = &bb, cb.stat_part = gp.dev;
    conv_run_dgrad(pd, g, dg, st, cb, sc.s);
    sc.get_stored(dx, cb.dx, nx, st.dx_bf16);
    if (const int rc = gp.fetch(sc, name, part)) return rc;
    bn_bwd_fast(bx, d_sc, d_sh, d_m, d_v, d_g, cb.dx, 0, 1, 1, (int)bn_rows, cin, 1, (int)bn_rows, bn_rows * cin, nullptr, d_dg, d_db,
                nullptr, d_red, 1e-3f, relu ? 1 : 0, 1, sc.s, 0, stored ? 1 : 0, stored ? 1 : 0, gp.dev, blocks);
    sc.get(dgamma, d_dg, (size_t)cin);
    sc.get(dbeta, d_db, (size_t)cin);
    if (const int rc = gp.recheck(sc, name)) return rc;
    return sc.status();
}

// The backward of a tower's first block as tower_forward / tower_backward_block run it (engine.hip, OP_BN's bn_xhat_ones and
// OP_CONV's `p.aug != FW_NONE` branch): the same library calls in the same order on ONE reduction scratch -- the coefficients
// conv_first_wgrad reads are bn_bwd_fast_coeffs of it -- and one weight-gradient scratch of exactly
// conv_wgrad_scratch_floats(ageom) floats, NaN before the launch, with a guard behind it.  The convolution's stored output y is an
// input, so the BatchNorm behind it takes its statistics from y itself (bn_stats_fast, the engine's pass where no epilogue left
// partials).  form 0: FW_AUG (bn_bwd_fast writes dY and the bias gradient); 1 / 2: FW_AUG_DEFERRED on fp32 / bfloat16-stored y, dA.
int l3_op_first_block_bwd(int device, int form, int relu, const float* x, const float* gamma_in, const float* beta_in, const float* w,
                          const float* y, const float* gamma2, const float* beta2, const float* dA, float* mean_in, float* var_in,
                          float* xaug, float* mean2, float* var2, float* scale2, float* shift2, float* dgamma2, float* dbeta2,
                          float* coeffs, float* dY, float* gaug, float* dw, float* dbias, float* dgamma_in, float* dbeta_in, int n,
                          int h, int wd, int c, int cout) {
    const char* name = "l3_op_first_block_bwd";
    if (form < 0 || form > 2 || (relu != 0 && relu != 1) || n < 1 || h < 1 || wd < 1 || c < 1 || cout < 1) {
        set_op_error(std::string(name) + ": form outside 0..2, relu outside 0..1 or an empty shape");
        return L3_EINVAL;
    }
    if (!x || !gamma_in || !beta_in || !w || !y || !gamma2 || !beta2 || !dA || !mean_in || !var_in || !xaug || !mean2 || !var2 ||
        !scale2 || !shift2 || !dgamma2 || !dbeta2 || !(form == 0 ? dY : coeffs) || !gaug || !dw || !dbias || !dgamma_in || !dbeta_in) {
        set_op_error(std::string(name) + ": NULL pointer");
        return L3_EINVAL;
    }
    ConvGeom ageom = make_geom(n, h, wd, c, cout, 3, 3, 1);
    ageom.Cin = c + 1;
    if (!conv_first_wgrad_ok(ageom) || !bn_fast_ok(cout)) {
        set_op_error(std::string(name) + ": not a first block (3x3 'same', 1 or 3 channels, 64 filters, L3_FIRST_WGRAD on): the "
                     "generic weight gradient would run");
        return L3_EINVAL;
    }
    const bool defer = form != 0, bf16 = form == 2;
    const int64_t rows = (int64_t)n * h * wd;
    const int ca = c + 1;
    const size_t nx = (size_t)rows * c, nxa = (size_t)rows * ca, ny = (size_t)rows * cout, nw = (size_t)9 * c * cout,
                 ng = (size_t)9 * ca * cout, cp = (size_t)(c + 3) / 4 * 4, co = (size_t)cout;
    const size_t wg = conv_wgrad_scratch_floats(ageom), guard = 4096;
    size_t red = colreduce_scratch_floats(rows, c);
    if (bn_fast_scratch_floats(cout) > red) red = bn_fast_scratch_floats(cout);
    Scope sc(device);
    if (!sc.ok) return L3_EHIP;
    const uint32_t nan_bits = 0x7fc00000u;
    float sentinel = -12345.f;
    uint32_t sentinel_bits;
    memcpy(&sentinel_bits, &sentinel, sizeof sentinel_bits);
    auto fresh = [&](size_t count) {          // an output or scratch buffer: NaN until a kernel writes it
        float* p = sc.alloc<float>(count);
        if (p && hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(p), (int)nan_bits, count) != hipSuccess) sc.ok = false;
        return p;
    };
    float* d_x = sc.put(x, nx);
    float* d_w = sc.put(w, nw);
    float* d_y = sc.put(y, ny);
    float* d_dA = sc.put(dA, ny);
    float *d_gi = sc.alloc<float>(cp), *d_bi = sc.alloc<float>(cp);
    float *d_g2 = sc.put(gamma2, co), *d_b2 = sc.put(beta2, co);
    float *d_mi = fresh(cp), *d_vi = fresh(cp), *d_sci = fresh(cp), *d_shi = fresh(cp);
    float *d_m2 = fresh(co), *d_v2 = fresh(co), *d_sc2 = fresh(co), *d_sh2 = fresh(co), *d_dg2 = fresh(co), *d_db2 = fresh(co);
    float* d_xa = fresh(nxa);
    float* d_dY = defer ? nullptr : fresh(ny);
    float* d_gaug = fresh(ng);
    float *d_dw = fresh(nw), *d_dbias = fresh(co), *d_dgi = fresh(cp), *d_dbi = fresh(cp);
    float* d_red = fresh(red);
    float* d_part = fresh(wg + guard);
    uint16_t* yb = bf16 ? sc.alloc<uint16_t>(ny) : nullptr;
    uint16_t* ab = bf16 ? sc.alloc<uint16_t>(ny) : nullptr;
    if (!sc.ok) return L3_ENOMEM;
    if (hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(d_part + wg), (int)sentinel_bits, guard) != hipSuccess) return L3_EHIP;
    (void)hipMemcpy(d_gi, gamma_in, c * 4, hipMemcpyHostToDevice);
    (void)hipMemcpy(d_bi, beta_in, c * 4, hipMemcpyHostToDevice);
    const float *ys = d_y, *as = d_dA;
    if (bf16) {          // both tensors as the mixed-precision kernels leave them (the engine's defers())
        cast_bf16(d_y, yb, (int64_t)ny, sc.s);
        cast_bf16(d_dA, ab, (int64_t)ny, sc.s);
        ys = reinterpret_cast<const float*>(yb);
        as = reinterpret_cast<const float*>(ab);
    }
    // forward: the input BatchNorm's statistics and [x^, 1] (engine.hip OP_BN, BS_PLAIN); the following BatchNorm's from y
    bn_stats(d_x, d_gi, d_bi, d_mi, d_vi, d_sci, d_shi, d_red, rows, c, 1e-3f, sc.s);
    bn_xhat_ones(d_x, d_mi, d_vi, 1e-3f, d_xa, rows, c, sc.s);
    bn_stats_fast(ys, d_g2, d_b2, d_m2, d_v2, d_sc2, d_sh2, d_red, rows, cout, 1e-3f, 0, sc.s, bf16 ? 1 : 0);
    // backward, in the engine's order: BatchNorm behind the conv (BB_FAST / BB_FAST_DEFERRED), then the conv's FW_AUG(_DEFERRED)
    bn_bwd_fast(ys, d_sc2, d_sh2, d_m2, d_v2, d_g2, as, 0, n, h, wd, cout, h, wd, (int64_t)h * wd * cout, defer ? nullptr : d_dY, d_dg2,
                d_db2, defer ? nullptr : d_dbias, d_red, 1e-3f, relu, 1, sc.s, 0, bf16 ? 1 : 0, bf16 ? 1 : 0);
    const float* cf = bn_bwd_fast_coeffs(d_red, cout);
    if (defer) {
        const FirstWgFuse f{ys, as, d_sc2, d_sh2, cf, cf + cout, cf + 2 * cout, relu, bf16 ? 1 : 0};
        conv_wgrad(d_xa, nullptr, d_gaug, d_part, ageom, sc.s, false, false, &f);
    } else {
        conv_wgrad(d_xa, d_dY, d_gaug, d_part, ageom, sc.s);
    }
    first_conv_grads(d_gaug, d_w, d_gi, d_bi, d_dw, d_dgi, d_dbi, defer ? d_dbias : nullptr, 9, c, cout, sc.s);
    std::vector<float> g(guard);
    sc.get(g.data(), d_part + wg, guard);
    if (!sc.ok) return L3_EHIP;
    for (size_t i = 0; i < guard; ++i)
        if (g[i] != sentinel) {
            set_op_error(std::string(name) + ": float " + std::to_string(i) + " of the guard behind the weight-gradient partials changed");
            return L3_EINVAL;
        }
    sc.get(mean_in, d_mi, (size_t)c);
    sc.get(var_in, d_vi, (size_t)c);
    sc.get(xaug, d_xa, nxa);
    sc.get(mean2, d_m2, co);
    sc.get(var2, d_v2, co);
    sc.get(scale2, d_sc2, co);
    sc.get(shift2, d_sh2, co);
    sc.get(dgamma2, d_dg2, co);
    sc.get(dbeta2, d_db2, co);
    if (defer) sc.get(coeffs, cf, 3 * co);
    else sc.get(dY, d_dY, ny);
    sc.get(gaug, d_gaug, ng);
    sc.get(dw, d_dw, nw);
    sc.get(dbias, d_dbias, co);
    sc.get(dgamma_in, d_dgi, (size_t)c);
    sc.get(dbeta_in, d_dbi, (size_t)c);
    return sc.status();
}

// first_conv_grads (elementwise.hip) alone on a caller's gaug (taps, c + 1, co) and filter w (taps, c, co): dw, dgamma (c),
// dbeta (c) and, unless NULL, dbias (co) -- the ones-channel row of tap taps / 2.
int l3_op_first_conv_grads(int device, const float* gaug, const float* w, const float* gamma, const float* beta, float* dw,
                           float* dgamma, float* dbeta, float* dbias, int taps, int c, int co) {
    if (!gaug || !w || !gamma || !beta || !dw || !dgamma || !dbeta || taps < 1 || c < 1 || co < 1 ||
        (int64_t)taps * (c + 1) * co >= (int64_t)1 << 31) {
        set_op_error("l3_op_first_conv_grads: NULL pointer, an empty shape or more than 2^31 entries");
        return L3_EINVAL;
    }
    Scope sc(device);
    if (!sc.ok) return L3_EHIP;
    const size_t ng = (size_t)taps * (c + 1) * co, nw = (size_t)taps * c * co;
    const uint32_t nan_bits = 0x7fc00000u;
    auto fresh = [&](size_t count) {
        float* p = sc.alloc<float>(count);
        if (p && hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(p), (int)nan_bits, count) != hipSuccess) sc.ok = false;
        return p;
    };
    float *d_g = sc.put(gaug, ng), *d_w = sc.put(w, nw), *d_ga = sc.put(gamma, (size_t)c), *d_be = sc.put(beta, (size_t)c);
    float *d_dw = fresh(nw), *d_dg = fresh((size_t)c), *d_db = fresh((size_t)c), *d_dbias = dbias ? fresh((size_t)co) : nullptr;
    if (!sc.ok) return L3_ENOMEM;
    first_conv_grads(d_g, d_w, d_ga, d_be, d_dw, d_dg, d_db, d_dbias, taps, c, co, sc.s);
    sc.get(dw, d_dw, nw);
    sc.get(dgamma, d_dg, (size_t)c);
    sc.get(dbeta, d_db, (size_t)c);
    if (dbias) sc.get(dbias, d_dbias, (size_t)co);
    return sc.status();
}

int l3_op_preprocess(int device, const uint8_t* video_u8, int64_t nv, float* video, const int16_t* audio_i16,
                     int64_t na, float* audio) {
    Scope sc(device);
    if (!sc.ok) return L3_EHIP;
    if (video_u8 && nv > 0) {
        uint8_t* d_in = sc.put(video_u8, (size_t)nv);
        float* d_out = sc.alloc<float>((size_t)nv);
        if (!sc.ok) return L3_ENOMEM;
        preprocess_video(d_in, d_out, nv, sc.s);
        sc.get(video, d_out, (size_t)nv);
    }
    if (audio_i16 && na > 0) {
        int16_t* d_in = sc.put(audio_i16, (size_t)na);
        float* d_out = sc.alloc<float>((size_t)na);
        if (!sc.ok) return L3_ENOMEM;
        preprocess_audio(d_in, d_out, na, sc.s);
        sc.get(audio, d_out, (size_t)na);
    }
    return sc.status();
}

static_assert(sizeof(l3_augment_params) == sizeof(AugmentParams) && sizeof(AugmentParams) == 24, "one record layout on both sides");

int l3_op_augment_video(int device, const uint8_t* u8, int n, int h, int w, const l3_augment_params* params, uint8_t* out_u8,
                        float* out_f32) {
    if (!u8 || !params || (!out_u8 && !out_f32) || n <= 0 || h < AUG_CROP || w < AUG_CROP) {
        set_op_error("l3_op_augment_video: NULL pointer, n <= 0 or a frame smaller than 224 x 224");
        return L3_EINVAL;
    }
    for (int i = 0; i < n; ++i)
        if (params[i].start_x < 0 || params[i].start_x > h - AUG_CROP || params[i].start_y < 0 || params[i].start_y > w - AUG_CROP) {
            set_op_error("l3_op_augment_video: record " + std::to_string(i) + ": crop start (" + std::to_string(params[i].start_x) +
                         ", " + std::to_string(params[i].start_y) + ") outside a " + std::to_string(h) + " x " + std::to_string(w) +
                         " frame");
            return L3_EINVAL;
        }
    Scope sc(device);
    if (!sc.ok) return L3_EHIP;
    const size_t n_out = (size_t)n * AUG_CROP * AUG_CROP * 3;
    uint8_t* d_in = sc.put(u8, (size_t)n * h * w * 3);
    AugmentParams* d_par = sc.put(reinterpret_cast<const AugmentParams*>(params), (size_t)n);
    uint8_t* d_u8 = out_u8 ? sc.alloc<uint8_t>(n_out) : nullptr;
    float* d_f32 = out_f32 ? sc.alloc<float>(n_out) : nullptr;
    if (!sc.ok) return L3_ENOMEM;
    augment_video(d_in, n, h, w, d_par, d_u8, d_f32, sc.s);
    if (out_u8) sc.get(out_u8, d_u8, n_out);
    if (out_f32) sc.get(out_f32, d_f32, n_out);
    return sc.status();
}

int l3_op_augment_audio(int device, const int16_t* i16, int n, int t, const double* u, int16_t* out_i16, float* out_f32,
                        double* gains) {
    if (!i16 || !u || !gains || (!out_i16 && !out_f32) || n <= 0 || t <= 0) {
        set_op_error("l3_op_augment_audio: NULL pointer or an empty batch");
        return L3_EINVAL;
    }
    Scope sc(device);
    if (!sc.ok) return L3_EHIP;
    const size_t cnt = (size_t)n * t;
    int16_t* d_in = sc.put(i16, cnt);
    double* d_u = sc.put(u, (size_t)n);
    double* d_g = sc.alloc<double>((size_t)n);
    int16_t* d_i16 = out_i16 ? sc.alloc<int16_t>(cnt) : nullptr;
    float* d_f32 = out_f32 ? sc.alloc<float>(cnt) : nullptr;
    if (!sc.ok) return L3_ENOMEM;
    augment_audio(d_in, n, t, d_u, d_i16, d_f32, d_g, sc.s);
    if (out_i16) sc.get(out_i16, d_i16, cnt);
    if (out_f32) sc.get(out_f32, d_f32, cnt);
    sc.get(gains, d_g, (size_t)n);
    return sc.status();
}

int l3_op_gather_frames(int device, const float* samples, int64_t n_samples, const int64_t* table, int64_t n_frames,
                        float* frames) {
    if (!samples || !table || !frames || n_samples < 0 || n_frames < 0) {
        set_op_error("l3_op_gather_frames: NULL pointer or negative count");
        return L3_EINVAL;
    }
    int64_t bad = 0;
    if (const char* why = frame_table_error(table, n_frames, n_samples, &bad)) {
        set_op_error(std::string("l3_op_gather_frames: frame ") + std::to_string(bad) + ": " + why);
        return L3_EINVAL;
    }
    Scope sc(device);
    if (!sc.ok) {
        set_op_error(no_gpu_message("l3_op_gather_frames", device));
        return L3_EHIP;
    }
    constexpr int T = 48000;
    const float* d_s = sc.put(samples, (size_t)n_samples);
    const int64_t* d_t = sc.put(table, (size_t)n_frames * 3);
    float* d_f = sc.alloc<float>((size_t)n_frames * T);
    if (!sc.ok) return L3_ENOMEM;
    for (int64_t r0 = 0; r0 < n_frames; r0 += 65535) {
        const int rows = (int)(n_frames - r0 < 65535 ? n_frames - r0 : 65535);
        gather_frames(d_s, d_t + 3 * r0, d_f + (size_t)r0 * T, rows, rows, T, sc.s);
    }
    sc.get(frames, d_f, (size_t)n_frames * T);
    return sc.status();
}

int l3_op_image_frames(int device, const uint8_t* pixels, int64_t n_bytes, const int64_t* table, int64_t n_frames, uint8_t* out_u8,
                       float* out_f32) {
    if (!pixels || !table || n_bytes < 0 || n_frames < 0) {
        set_op_error("l3_op_image_frames: NULL pointer or negative count");
        return L3_EINVAL;
    }
    int64_t bad = 0;
    if (const char* why = image_table_error(table, n_frames, n_bytes, &bad)) {
        set_op_error(std::string("l3_op_image_frames: frame ") + std::to_string(bad) + ": " + why);
        return L3_EINVAL;
    }
    if (n_frames == 0) return L3_OK;
    Scope sc(device);
    if (!sc.ok) {
        set_op_error(no_gpu_message("l3_op_image_frames", device));
        return L3_EHIP;
    }
    ImagePlan plan;
    image_plan(table, n_frames, &plan);
    const size_t n_out = (size_t)n_frames * IMG * IMG * 3;
    const uint8_t* d_p = sc.put(pixels, (size_t)n_bytes);
    const int64_t* d_d = sc.put(plan.frames.data(), plan.frames.size());
    const int64_t* d_t = sc.put(plan.taps.data(), plan.taps.size());
    uint8_t* d_u8 = out_u8 ? sc.alloc<uint8_t>(n_out) : nullptr;
    float* d_f32 = out_f32 ? sc.alloc<float>(n_out) : nullptr;
    if (!sc.ok) return L3_ENOMEM;
    for (int64_t r0 = 0; r0 < n_frames; r0 += 65535) {
        const int rows = (int)(n_frames - r0 < 65535 ? n_frames - r0 : 65535);
        const size_t o = (size_t)r0 * IMG * IMG * 3;
        image_frames(d_p, d_d + IMAGE_DESC * r0, d_t, d_u8 ? d_u8 + o : nullptr, d_f32 ? d_f32 + o : nullptr, rows, rows, sc.s);
    }
    if (out_u8) sc.get(out_u8, d_u8, n_out);
    if (out_f32) sc.get(out_f32, d_f32, n_out);
    return sc.status();
}

int l3_op_sample_batch(l3_clipbank* bank, const l3_sample* records, int n, int augment, uint8_t* out_u8, int16_t* out_i16,
                       double* gains) {
    if (!bank || !records || !out_u8 || !out_i16 || n < 1 || (augment && !gains)) {
        set_op_error("l3_op_sample_batch: NULL pointer, n < 1 or an augmented batch without a place for its gains");
        return L3_EINVAL;
    }
    SampledHost h;
    std::string why;
    if (int rc = sampled_plan(bank, records, n, augment != 0, &h, &why)) {
        set_op_error("l3_op_sample_batch: " + why);
        return rc;
    }
    const int device = clipbank_device(bank);
    Scope sc(device);
    if (!sc.ok) {
        set_op_error(no_gpu_message("l3_op_sample_batch", device));
        return L3_EHIP;
    }
    const size_t n_out = (size_t)n * IMG * IMG * 3, n_aud = (size_t)n * SAMPLE_T;
    const int64_t* d_d = sc.put(h.plan.frames.data(), h.plan.frames.size());
    const int64_t* d_t = sc.put(h.plan.taps.data(), h.plan.taps.size());
    const int64_t* d_s = sc.put(h.seconds.data(), h.seconds.size());
    uint8_t* d_u8 = sc.alloc<uint8_t>(n_out);
    int16_t* d_i16 = sc.alloc<int16_t>(n_aud);
    if (!sc.ok) return L3_ENOMEM;
    image_frames(h.pixels, d_d, d_t, d_u8, nullptr, n, n, sc.s);
    audio_seconds(h.audio, d_s, d_i16, n, SAMPLE_T, sc.s);
    if (augment) {          // as BatchFeed::convert augments the rows of a sampled batch, in the stored dtypes
        const AugmentParams* d_par = sc.put(h.params.data(), (size_t)n);
        const double* d_u = sc.put(h.u.data(), (size_t)n);
        uint8_t* d_u8a = sc.alloc<uint8_t>(n_out);
        int16_t* d_i16a = sc.alloc<int16_t>(n_aud);
        double* d_g = sc.alloc<double>((size_t)n);
        if (!sc.ok) return L3_ENOMEM;
        augment_video(d_u8, n, AUG_CROP, AUG_CROP, d_par, d_u8a, nullptr, sc.s);
        augment_audio(d_i16, n, SAMPLE_T, d_u, d_i16a, nullptr, d_g, sc.s);
        d_u8 = d_u8a, d_i16 = d_i16a;
        sc.get(gains, d_g, (size_t)n);
    }
    sc.get(out_u8, d_u8, n_out);
    sc.get(out_i16, d_i16, n_aud);
    return sc.status();
}

static int op_resample(const char* name, int device, const float* x, int64_t n_in, const int64_t* clips, int64_t n_clips,
                       int64_t sr_new, const double* half_window, int64_t n_window, int num_table, int64_t n_samples, bool copy_equal,
                       float* y) {
    if (!x || !clips || !half_window || !y || n_in < 0 || n_clips < 0 || n_samples < 0) {
        set_op_error(std::string(name) + ": NULL pointer or negative count");
        return L3_EINVAL;
    }
    int64_t bad = 0;
    if (const char* why = resample_clips_error(clips, n_clips, n_in, sr_new, n_window, num_table, n_samples, copy_equal, &bad)) {
        set_op_error(std::string(name) + ": " + (bad >= 0 ? "clip " + std::to_string(bad) + ": " : std::string()) + why);
        return L3_EINVAL;
    }
    Scope sc(device);
    if (!sc.ok) {
        set_op_error(no_gpu_message(name, device));
        return L3_EHIP;
    }
    float* d_y = sc.alloc<float>((size_t)n_samples);
    if (!sc.ok) return L3_ENOMEM;
    ResampleStage stage;          // lives for the call: sc.get below waits for the device before it goes
    std::string why;
    if (const int rc = stage.run(x, n_in, clips, n_clips, sr_new, half_window, n_window, num_table, copy_equal, d_y, n_samples, sc.s, &why)) {
        set_op_error(std::string(name) + ": " + why);
        return rc;
    }
    sc.get(y, d_y, (size_t)n_samples);
    return sc.status();
}

int l3_op_resample(int device, const float* x, int64_t n_in, int64_t sr_orig, int64_t sr_new, const double* half_window,
                   int64_t n_window, int num_table, int64_t t0, int64_t n_out, float* y) {
    const int64_t row[RESAMPLE_ROW] = {0, n_in, sr_orig, t0, n_out, 0};
    return op_resample("l3_op_resample", device, x, n_in, row, 1, sr_new, half_window, n_window, num_table, n_out, false, y);
}

int l3_op_resample_clips(int device, const float* x, int64_t n_in, const int64_t* clips, int64_t n_clips, int64_t sr_new,
                         const double* half_window, int64_t n_window, int num_table, int64_t n_samples, int copy_equal, float* y) {
    return op_resample("l3_op_resample_clips", device, x, n_in, clips, n_clips, sr_new, half_window, n_window, num_table, n_samples,
                       copy_equal != 0, y);
}

int l3_op_frontend(int device, int model_type, const float* audio, int n, int db_max_scope, float* out) {
    // runs the engine's own front-end path on a throw-away engine of batch n
    l3_config cfg{};
    cfg.struct_size = (int32_t)sizeof(l3_config);
    cfg.model_type = model_type;
    cfg.batch = n;
    cfg.device = device;
    cfg.db_max_scope = db_max_scope;
    cfg.bn_zero_debias = 1;
    l3_engine* e = nullptr;
    int rc = l3_create(&cfg, 1, &e);
    if (rc) return rc;
    rc = l3_upload_batch(e, nullptr, audio, nullptr);
    if (!rc) rc = l3_step_forward(e, 0);
    int64_t numel = 0;
    if (!rc) rc = l3_activation_numel(e, "audio_model/frontend", &numel);
    if (!rc) rc = l3_get_activation(e, "audio_model/frontend", out, numel);
    l3_destroy(e);
    return rc;
}

int l3_op_frontend_form(int device, int model_type, int frontend, const float* audio, int n, float* out) {
    // l3_op_frontend with the form: a throw-away engine of batch n, per-sample maximum
    l3_config cfg{};
    cfg.struct_size = (int32_t)sizeof(l3_config);
    cfg.model_type = model_type;
    cfg.batch = n;
    cfg.device = device;
    cfg.bn_zero_debias = 1;
    cfg.frontend = frontend;
    l3_engine* e = nullptr;
    int rc = l3_create(&cfg, 1, &e);
    if (rc) return rc;
    rc = l3_upload_batch(e, nullptr, audio, nullptr);
    if (!rc) rc = l3_step_forward(e, 0);
    int64_t numel = 0;
    if (!rc) rc = l3_activation_numel(e, "audio_model/frontend", &numel);
    if (!rc) rc = l3_get_activation(e, "audio_model/frontend", out, numel);
    l3_destroy(e);
    return rc;
}

}  // extern "C"

// ---- the audio front-end's kernels one by one (frontend.hip; tests/frontend_ref.py) -------------------------------------------------
// Every output buffer is NaN before the launch and has a guard of a sentinel behind it that must come back untouched.
namespace {
constexpr size_t FE_GUARD = 4096;
constexpr float FE_SENTINEL = -12345.f;

struct FeOut {
    float* d = nullptr;
    size_t n = 0;
    const char* what = "";
};

// the kernels' outputs of one front-end operator
struct FeBufs {
    Scope& sc;
    std::vector<FeOut> outs;
    explicit FeBufs(Scope& s) : sc(s) {}
    // `count` floats, NaN (or the `count` floats at init: an in-place operand), and the guard
    float* fresh(size_t count, const char* what, const float* init = nullptr) {
        const uint32_t nan_bits = 0x7fc00000u;
        uint32_t sentinel_bits;
        memcpy(&sentinel_bits, &FE_SENTINEL, sizeof sentinel_bits);
        float* p = sc.alloc<float>(count + FE_GUARD);
        if (!p) return nullptr;
        if (init) {
            if (count && hipMemcpy(p, init, count * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) sc.ok = false;
        } else if (count && hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(p), (int)nan_bits, count) != hipSuccess) {
            sc.ok = false;
        }
        if (hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(p + count), (int)sentinel_bits, FE_GUARD) != hipSuccess) sc.ok = false;
        outs.push_back({p, count, what});
        return p;
    }
    // after the launches: waits, then every guard
    int check(const char* name) {
        std::vector<float> g(FE_GUARD);
        for (const FeOut& o : outs) {
            sc.get(g.data(), o.d + o.n, FE_GUARD);
            if (!sc.ok) return L3_EHIP;
            for (size_t i = 0; i < FE_GUARD; ++i)
                if (g[i] != FE_SENTINEL)
                    return fail(L3_EINVAL, std::string(name) + ": float " + std::to_string(i) + " of the guard behind " + o.what + " changed");
        }
        return L3_OK;
    }
};

// the geometry of an operator's call: the frames must stay inside int sample indices and the outputs inside 2^31 floats
bool fe_geometry_ok(int B, int T, int n_dft, int n_hop, int pad_left, int n_frames) {
    if (B < 1 || T < 1 || n_dft < 32 || n_dft % 32 != 0 || n_dft > 8192 || n_hop < 1 || pad_left < 0 || n_frames < 1) return false;
    if ((int64_t)(n_frames - 1) * n_hop + n_dft + pad_left >= (int64_t)1 << 31) return false;
    if ((int64_t)B * T >= (int64_t)1 << 31) return false;
    return (int64_t)B * n_frames * (2 * n_dft) < (int64_t)1 << 31;
}

FrontendCfg fe_cfg(int T, int n_dft, int n_hop, int pad_left, int n_frames, int n_mels, int flags) {
    FrontendCfg c = frontend_cfg(T, n_dft, n_hop, false, n_mels, flags & 1, (flags >> 1) & 1, (flags >> 2) & 1);
    c.pad_left = pad_left;
    c.n_frames = n_frames;
    return c;
}

// the filterbank an operator runs with, as the engine would pack it: the caller's (nb, n_mels), or the stock one
void fe_bands(const float* freq2mel, int n_dft, int n_mels, MelBands& m) {
    std::vector<float> stock;
    if (!freq2mel) {
        host_mel_basis(48000, n_dft, n_mels, stock);
        freq2mel = stock.data();
    }
    mel_pack_bands(freq2mel, n_dft / 2 + 1, n_mels, m);
}

struct FeDevBands {
    float* w = nullptr;
    int *start = nullptr, *len = nullptr, *off = nullptr;
    void put(Scope& sc, const MelBands& m) {
        w = sc.put(m.w.data(), m.w.size());
        start = sc.put(m.start.data(), m.start.size());
        len = sc.put(m.len.data(), m.len.size());
        off = sc.put(m.off.data(), m.off.size());
    }
};
}  // namespace

extern "C" {

int l3_frontend_cfg(int t, int n_dft, int n_hop, int same, int n_mels, int32_t* cfg) {
    if (!cfg || t < 1 || n_dft < 2 || n_hop < 1 || n_mels < 0 || (!same && t < n_dft))
        return fail(L3_EINVAL, "l3_frontend_cfg: NULL pointer, an empty shape or 'valid' framing of fewer samples than one frame");
    const FrontendCfg f = frontend_cfg(t, n_dft, n_hop, same != 0, n_mels, 0, 0, 0);
    const int32_t v[L3_FRONTEND_CFG_FIELDS] = {f.n_frames, f.pad_left, f.n_freq, f.ncols_pad, f.ke, f.ko, f.nc, f.N1, f.N2};
    memcpy(cfg, v, sizeof v);
    return L3_OK;
}

int l3_frontend_tables(const float* freq2mel, int n_mels, float* win, float* b1, float* b2, float* tw, int32_t* mel_start,
                       int32_t* mel_len, int32_t* mel_off, float* melw, int64_t melw_cap, int64_t* n_melw) {
    const int N = 2048, N1 = 32, N2 = 64;
    if (!win || !b1 || !b2 || !tw || n_mels < 0 || (n_mels > 0 && (!mel_start || !mel_len || !mel_off || !melw || !n_melw || melw_cap < 0)))
        return fail(L3_EINVAL, "l3_frontend_tables: NULL pointer or a negative count");
    DftTables t;
    dft_factor_tables(N, N1, N2, t);
    memcpy(win, t.win.data(), t.win.size() * 4);
    memcpy(b1, t.b1.data(), t.b1.size() * 4);
    memcpy(b2, t.b2.data(), t.b2.size() * 4);
    memcpy(tw, t.tw.data(), t.tw.size() * 4);
    if (n_mels == 0) return L3_OK;
    MelBands m;
    fe_bands(freq2mel, N, n_mels, m);
    *n_melw = (int64_t)m.w.size();
    if ((int64_t)m.w.size() > melw_cap) return fail(L3_EINVAL, "l3_frontend_tables: the packed bands hold more weights than melw_cap");
    memcpy(mel_start, m.start.data(), (size_t)n_mels * 4);
    memcpy(mel_len, m.len.data(), (size_t)n_mels * 4);
    memcpy(mel_off, m.off.data(), (size_t)n_mels * 4);
    if (!m.w.empty()) memcpy(melw, m.w.data(), m.w.size() * 4);
    return L3_OK;
}

int l3_op_frontend_frames(int device, const float* audio, int b, int t, int n_dft, int n_hop, int pad_left, int n_frames,
                          float* frames, float* fe, float* fo, float* a1) {
    const char* name = "l3_op_frontend_frames";
    if (!audio || !frames || !fe || !fo || !fe_geometry_ok(b, t, n_dft, n_hop, pad_left, n_frames) || (a1 && n_dft != 2048))
        return fail(L3_EINVAL, std::string(name) + ": NULL pointer, a shape outside the kernels' index range, or a1 asked for n_dft != 2048");
    const FrontendCfg c = fe_cfg(t, n_dft, n_hop, pad_left, n_frames, 0, 0);
    const size_t rows = (size_t)b * n_frames;
    Scope sc(device);
    if (!sc.ok) return fail(L3_EHIP, no_gpu_message(name, device));
    FeBufs out(sc);
    float* d_audio = sc.put(audio, (size_t)b * t);
    float* d_frames = out.fresh(rows * n_dft, "frames");
    float* d_fe = out.fresh(rows * c.ke, "fe");
    float* d_fo = out.fresh(rows * c.ko, "fo");
    float *d_a1 = nullptr, *d_win = nullptr;
    if (a1) {
        DftTables tb;
        dft_factor_tables(n_dft, c.N1, c.N2, tb);
        d_win = sc.put(tb.win.data(), tb.win.size());
        d_a1 = out.fresh(rows * n_dft, "a1");
    }
    if (!sc.ok) return L3_ENOMEM;
    frame_audio(d_audio, d_frames, b, t, c, sc.s);
    frame_audio_folded(d_audio, d_fe, d_fo, b, t, c, sc.s);
    if (a1) dft_pack_frames(d_audio, d_win, d_a1, b, t, c, sc.s);
    if (const int rc = out.check(name)) return rc;
    sc.get(frames, d_frames, rows * n_dft);
    sc.get(fe, d_fe, rows * c.ke);
    sc.get(fo, d_fo, rows * c.ko);
    if (a1) sc.get(a1, d_a1, rows * n_dft);
    return sc.status();
}

int l3_op_dft_twiddle(int device, const float* y, int frames, float* a2, float* nyq) {
    const char* name = "l3_op_dft_twiddle";
    if (!y || !a2 || !nyq || frames < 1 || (int64_t)frames * 4096 >= (int64_t)1 << 31)
        return fail(L3_EINVAL, std::string(name) + ": NULL pointer or a frame count outside 1 .. 2^19 - 1");
    const FrontendCfg c = fe_cfg(2048, 2048, 1, 0, 1, 0, 0);
    const size_t n = (size_t)frames * 2 * c.n_dft;
    Scope sc(device);
    if (!sc.ok) return fail(L3_EHIP, no_gpu_message(name, device));
    FeBufs out(sc);
    DftTables tb;
    dft_factor_tables(c.n_dft, c.N1, c.N2, tb);
    float* d_y = sc.put(y, n);
    float* d_tw = sc.put(tb.tw.data(), tb.tw.size());
    float* d_a2 = out.fresh(n, "a2");
    float* d_nyq = out.fresh((size_t)frames, "nyq");
    if (!sc.ok) return L3_ENOMEM;
    dft_twiddle(d_y, d_tw, d_a2, d_nyq, frames, c, sc.s);
    if (const int rc = out.check(name)) return rc;
    sc.get(a2, d_a2, n);
    sc.get(nyq, d_nyq, (size_t)frames);
    return sc.status();
}

int l3_op_spec_to_features(int device, int layout, const float* spec, const float* nyq, int b, int n_frames, int n_dft, int n_mels,
                           const float* freq2mel, int flags, float* out_feat) {
    const char* name = "l3_op_spec_to_features";
    if (!spec || !out_feat || layout < L3_SPEC_UNFOLDED || layout > L3_SPEC_FACTORED || b < 1 || n_frames < 1 || n_mels < 0 ||
        n_mels > 65536 || flags < 0 || flags > 7 || !fe_geometry_ok(b, n_dft, n_dft, 1, 0, n_frames) ||
        (layout == L3_SPEC_FACTORED && (n_dft != 2048 || !nyq)))
        return fail(L3_EINVAL, std::string(name) + ": NULL pointer, an unknown layout or flag, an empty shape, or the factored layout without "
                                                   "n_dft = 2048 and the Nyquist bins");
    FrontendCfg c = fe_cfg(n_dft, n_dft, 1, 0, n_frames, n_mels, flags);
    c.folded = layout == L3_SPEC_FOLDED;
    c.factored = layout == L3_SPEC_FACTORED;
    const size_t rows = (size_t)b * n_frames, F = n_mels ? (size_t)n_mels : (size_t)c.n_freq;
    const size_t n_spec = layout == L3_SPEC_UNFOLDED ? rows * c.ncols_pad : layout == L3_SPEC_FOLDED ? 2 * rows * c.nc : rows * n_dft;
    if ((int64_t)rows * (int64_t)F >= (int64_t)1 << 31) return fail(L3_EINVAL, std::string(name) + ": more than 2^31 outputs");
    MelBands m;
    if (n_mels) fe_bands(freq2mel, n_dft, n_mels, m);
    Scope sc(device);
    if (!sc.ok) return fail(L3_EHIP, no_gpu_message(name, device));
    FeBufs out(sc);
    float* d_spec = sc.put(spec, n_spec);
    float* d_nyq = layout == L3_SPEC_FACTORED ? sc.put(nyq, rows) : nullptr;
    FeDevBands db;
    if (n_mels) db.put(sc, m);
    float* d_out = out.fresh(rows * F, "the features");
    if (!sc.ok) return L3_ENOMEM;
    spec_to_features(d_spec, db.w, db.start, db.len, db.off, d_out, b, c, sc.s, d_nyq);
    if (const int rc = out.check(name)) return rc;
    sc.get(out_feat, d_out, rows * F);
    return sc.status();
}

int l3_op_dft_fused(int device, const float* audio, int b, int t, int n_hop, int pad_left, int n_frames, int n_mels,
                    const float* freq2mel, int flags, float* out_feat) {
    const char* name = "l3_op_dft_fused";
    if (!audio || !out_feat || n_mels < 1 || n_mels > 65536 || flags < 0 || flags > 7 ||
        !fe_geometry_ok(b, t, 2048, n_hop, pad_left, n_frames) || (int64_t)b * n_frames * n_mels >= (int64_t)1 << 31)
        return fail(L3_EINVAL, std::string(name) + ": NULL pointer, no filter, an unknown flag or a shape outside the kernel's index range");
    FrontendCfg c = fe_cfg(t, 2048, n_hop, pad_left, n_frames, n_mels, flags);
    c.factored = 1;
    const size_t rows = (size_t)b * n_frames;
    MelBands m;
    fe_bands(freq2mel, c.n_dft, n_mels, m);
    DftTables tb;
    dft_factor_tables(c.n_dft, c.N1, c.N2, tb);
    Scope sc(device);
    if (!sc.ok) return fail(L3_EHIP, no_gpu_message(name, device));
    FeBufs out(sc);
    float* d_audio = sc.put(audio, (size_t)b * t);
    float *d_win = sc.put(tb.win.data(), tb.win.size()), *d_b1 = sc.put(tb.b1.data(), tb.b1.size());
    float *d_b2 = sc.put(tb.b2.data(), tb.b2.size()), *d_tw = sc.put(tb.tw.data(), tb.tw.size());
    FeDevBands db;
    db.put(sc, m);
    float* d_out = out.fresh(rows * n_mels, "the features");
    if (!sc.ok) return L3_ENOMEM;
    dft_fused(d_audio, d_win, d_b1, d_b2, d_tw, db.w, db.start, db.len, db.off, d_out, b, t, c, sc.s);
    if (const int rc = out.check(name)) return rc;
    sc.get(out_feat, d_out, rows * n_mels);
    return sc.status();
}

int l3_op_db_normalize(int device, float* x, int b, int64_t per_sample, int batch_scope) {
    const char* name = "l3_op_db_normalize";
    if (!x || b < 1 || per_sample < 1 || (batch_scope != 0 && batch_scope != 1) || (int64_t)b * per_sample >= (int64_t)1 << 31)
        return fail(L3_EINVAL, std::string(name) + ": NULL pointer, an empty shape, a scope outside 0..1 or more than 2^31 values");
    const size_t n = (size_t)b * per_sample;
    Scope sc(device);
    if (!sc.ok) return fail(L3_EHIP, no_gpu_message(name, device));
    FeBufs out(sc);
    float* d_x = out.fresh(n, "x", x);
    float* d_max = out.fresh((size_t)b, "the maxima");
    if (!sc.ok) return L3_ENOMEM;
    db_normalize(d_x, d_max, b, per_sample, batch_scope, sc.s);
    if (const int rc = out.check(name)) return rc;
    sc.get(x, d_x, n);
    return sc.status();
}

}  // extern "C"

// ---- MLP classifier operators (mlp.hip; classifier/train.py:230-257) ---------------------------------------------------------
namespace {
int mlp_op_check(const char* name, int device, bool ptrs_ok, int rows, int K, int N, const int32_t* idx, int64_t n_x) {
    if (!ptrs_ok || rows <= 0 || K <= 0 || N <= 0 || n_x < 0) {
        set_op_error(std::string(name) + ": NULL pointer or non-positive size");
        return L3_EINVAL;
    }
    if (!idx && n_x < rows) {
        set_op_error(std::string(name) + ": fewer rows in x than `rows`");
        return L3_EINVAL;
    }
    for (int i = 0; idx && i < rows; ++i)
        if (idx[i] < 0 || idx[i] >= n_x) {
            set_op_error(std::string(name) + ": idx[" + std::to_string(i) + "] outside [0, n_x)");
            return L3_EINVAL;
        }
    if (!device_ok(device)) {
        set_op_error(no_gpu_message(name, device));
        return L3_EHIP;
    }
    return L3_OK;
}
}  // namespace

extern "C" int l3_op_mlp_dense_fwd(int device, const float* x, int64_t n_x, const int32_t* idx, int rows, int K, int N, const float* w,
                                   const float* b, int relu, float* y) {
    const int rc = mlp_op_check("l3_op_mlp_dense_fwd", device, x && w && b && y, rows, K, N, idx, n_x);
    if (rc != L3_OK) return rc;
    Scope sc(device);
    const float* dx = sc.put(x, (size_t)n_x * K);
    const int* di = idx ? sc.put(idx, rows) : nullptr;
    const float* dw = sc.put(w, (size_t)K * N);
    const float* db = sc.put(b, N);
    float* dy = sc.alloc<float>((size_t)rows * N);
    float* part = sc.alloc<float>(MLP_PART_FLOATS);
    int* ctr = sc.alloc<int>(MLP_FWD_COUNTERS);
    if (!sc.ok || hipMemset(ctr, 0, MLP_FWD_COUNTERS * sizeof(int)) != hipSuccess) return L3_ENOMEM;
    mlp_dense_fwd(dx, di, K, dw, db, dy, rows, K, N, relu, part, ctr, sc.s);
    sc.get(y, dy, (size_t)rows * N);
    return sc.status();
}

extern "C" int l3_op_mlp_dense_bwd_x(int device, const float* dy, const float* w, const float* h, int rows, int K, int N, float* dx) {
    const int rc = mlp_op_check("l3_op_mlp_dense_bwd_x", device, dy && w && dx, rows, K, N, nullptr, rows);
    if (rc != L3_OK) return rc;
    Scope sc(device);
    const float* ddy = sc.put(dy, (size_t)rows * N);
    const float* dw = sc.put(w, (size_t)K * N);
    const float* dh = h ? sc.put(h, (size_t)rows * K) : nullptr;
    float* ddx = sc.alloc<float>((size_t)rows * K);
    if (!sc.ok) return L3_ENOMEM;
    mlp_dense_bwd_x(ddy, dw, dh, ddx, rows, K, N, sc.s);
    sc.get(dx, ddx, (size_t)rows * K);
    return sc.status();
}

namespace {
int mlp_wgrad_op(int device, const float* x, int64_t n_x, const int32_t* idx, int rows, int K, int N, const float* dy, float* dw,
                 float* db, float* w, float* b, float* mw, float* vw, float* mb, float* vb, float wd, float lr_t, float* w2_out) {
    const bool adam = w != nullptr;
    const char* name = adam ? "l3_op_mlp_wgrad_adam" : "l3_op_mlp_wgrad";
    const bool ptrs = x && dy && (adam ? (b && mw && vw && mb && vb) : (dw && db));
    const int rc = mlp_op_check(name, device, ptrs, rows, K, N, idx, n_x);
    if (rc != L3_OK) return rc;
    Scope sc(device);
    MlpWgrad a{};
    a.nl = 1, a.rows = rows, a.adam = adam ? 1 : 0;
    a.l2x2 = 2.f * wd, a.lr_t = lr_t, a.b1 = 0.9f, a.b2 = 0.999f, a.eps = 1e-8f, a.wd = wd;
    MlpWgLayer& L = a.L[0];
    L.x = sc.put(x, (size_t)n_x * K), L.idx = idx ? sc.put(idx, rows) : nullptr, L.ldx = K;
    L.dy = sc.put(dy, (size_t)rows * N), L.K = K, L.N = N;
    const size_t nw = (size_t)K * N;
    if (adam) {
        L.w = sc.put(w, nw), L.mw = sc.put(mw, nw), L.vw = sc.put(vw, nw);
        L.b = sc.put(b, N), L.mb = sc.put(mb, N), L.vb = sc.put(vb, N);
    } else {
        L.dw = sc.alloc<float>(nw), L.db = sc.alloc<float>(N);
    }
    float* w2part = sc.alloc<float>(mlp_wgrad_tiles(a));
    int* ctr = sc.alloc<int>(1);
    a.w2out = sc.alloc<float>(1);
    if (!sc.ok || hipMemset(ctr, 0, sizeof(int)) != hipSuccess) return L3_ENOMEM;
    mlp_wgrad(a, w2part, ctr, sc.s);
    if (adam) {
        sc.get(w, L.w, nw), sc.get(mw, L.mw, nw), sc.get(vw, L.vw, nw);
        sc.get(b, L.b, N), sc.get(mb, L.mb, N), sc.get(vb, L.vb, N);
        if (w2_out) sc.get(w2_out, a.w2out, 1);
    } else {
        sc.get(dw, L.dw, nw), sc.get(db, L.db, N);
    }
    return sc.status();
}
}  // namespace

extern "C" int l3_op_mlp_wgrad(int device, const float* x, int64_t n_x, const int32_t* idx, int rows, int K, int N, const float* dy,
                               float* dw, float* db) {
    if (!dw || !db) {
        set_op_error("l3_op_mlp_wgrad: NULL output");
        return L3_EINVAL;
    }
    return mlp_wgrad_op(device, x, n_x, idx, rows, K, N, dy, dw, db, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0.f,
                        nullptr);
}

extern "C" int l3_op_mlp_wgrad_adam(int device, const float* x, int64_t n_x, const int32_t* idx, int rows, int K, int N,
                                    const float* dy, float* w, float* b, float* mw, float* vw, float* mb, float* vb,
                                    float weight_decay, float lr_t, float* w2_out) {
    if (!w) {
        set_op_error("l3_op_mlp_wgrad_adam: NULL w");
        return L3_EINVAL;
    }
    return mlp_wgrad_op(device, x, n_x, idx, rows, K, N, dy, nullptr, nullptr, w, b, mw, vw, mb, vb, weight_decay, lr_t, w2_out);
}

extern "C" int l3_op_mlp_softmax_ce(int device, const float* z, const int32_t* labels, int rows, int C, float gscale, float* probs,
                                    float* dz, float* ce, float* correct) {
    int rc = mlp_op_check("l3_op_mlp_softmax_ce", device, z && labels, rows, 1, C, nullptr, rows);
    if (rc == L3_OK && (C < 2 || C > MLP_MAX_CLASSES)) {
        set_op_error("l3_op_mlp_softmax_ce: class count must be in [2, 64]");
        rc = L3_EINVAL;
    }
    for (int i = 0; rc == L3_OK && i < rows; ++i)
        if (labels[i] < 0 || labels[i] >= C) {
            set_op_error("l3_op_mlp_softmax_ce: labels[" + std::to_string(i) + "] outside [0, C)");
            rc = L3_EINVAL;
        }
    if (rc != L3_OK) return rc;
    Scope sc(device);
    const size_t n = (size_t)rows * C;
    const float* dzin = sc.put(z, n);
    const int* dl = sc.put(labels, rows);
    float* dp = probs ? sc.alloc<float>(n) : nullptr;
    float* ddz = dz ? sc.alloc<float>(n) : nullptr;
    float* dce = ce ? sc.alloc<float>(rows) : nullptr;
    float* dco = correct ? sc.alloc<float>(rows) : nullptr;
    if (!sc.ok) return L3_ENOMEM;
    mlp_softmax_ce(dzin, dl, nullptr, rows, C, gscale, dp, ddz, dce, dco, sc.s);
    if (probs) sc.get(probs, dp, n);
    if (dz) sc.get(dz, ddz, n);
    if (ce) sc.get(ce, dce, rows);
    if (correct) sc.get(correct, dco, rows);
    return sc.status();
}

extern "C" int l3_op_file_mean(int device, const float* probs, int64_t n, int C, const int64_t* file_idxs, int64_t n_files,
                               float* file_mean, int32_t* file_pred) {
    if (!probs || !file_idxs || n < 1 || C < 1 || C > MLP_MAX_CLASSES) {
        set_op_error("l3_op_file_mean: NULL pointer, n < 1 or a class count outside [1, 64]");
        return L3_EINVAL;
    }
    const std::string bad = mlp_file_ranges_error(file_idxs, n_files, n);
    if (!bad.empty()) {
        set_op_error("l3_op_file_mean: " + bad);
        return L3_EINVAL;
    }
    if (!device_ok(device)) {
        set_op_error(no_gpu_message("l3_op_file_mean", device));
        return L3_EHIP;
    }
    Scope sc(device);
    const float* dp = sc.put(probs, (size_t)(n * C));
    const int64_t* df = sc.put(file_idxs, (size_t)(2 * n_files));
    float* dm = sc.alloc<float>((size_t)(n_files * C));
    int* dq = sc.alloc<int>((size_t)n_files);
    if (!sc.ok) return L3_ENOMEM;
    mlp_file_mean(dp, C, df, n_files, dm, dq, sc.s);
    if (file_mean) sc.get(file_mean, dm, (size_t)(n_files * C));
    if (file_pred) sc.get(file_pred, dq, (size_t)n_files);
    return sc.status();
}

extern "C" int l3_op_adam(int device, float* p, const float* g, float* m, float* v, int64_t n, int64_t n_l2, float l2x2, float lr_t) {
    const int rc = mlp_op_check("l3_op_adam", device, p && g && m && v && n_l2 >= 0 && n_l2 <= n, 1, 1, 1, nullptr, n > 0 ? 1 : 0);
    if (rc != L3_OK || n <= 0) {
        if (rc == L3_OK) set_op_error("l3_op_adam: n <= 0");
        return rc != L3_OK ? rc : L3_EINVAL;
    }
    Scope sc(device);
    float* dp = sc.put(p, n);
    const float* dg = sc.put(g, n);
    float* dm = sc.put(m, n);
    float* dv = sc.put(v, n);
    if (!sc.ok) return L3_ENOMEM;
    adam_step(dp, dg, dm, dv, n, n_l2, l2x2, lr_t, 0.9f, 0.999f, 1e-8f, 1.f, sc.s);
    sc.get(p, dp, n), sc.get(m, dm, n), sc.get(v, dv, n);
    return sc.status();
}

extern "C" int l3_op_adam_scaled(int device, float* p, const float* g, float* m, float* v, int64_t n, int64_t n_l2, float l2x2,
                                 float lr_t, float b1, float b2, float eps, float gscale) {
    const int rc = mlp_op_check("l3_op_adam_scaled", device, p && g && m && v && n_l2 >= 0 && n_l2 <= n, 1, 1, 1, nullptr, n > 0 ? 1 : 0);
    if (rc != L3_OK || n <= 0) {
        if (rc == L3_OK) set_op_error("l3_op_adam_scaled: n <= 0");
        return rc != L3_OK ? rc : L3_EINVAL;
    }
    Scope sc(device);
    float* dp = sc.put(p, n);
    const float* dg = sc.put(g, n);
    float* dm = sc.put(m, n);
    float* dv = sc.put(v, n);
    if (!sc.ok) return L3_ENOMEM;
    adam_step(dp, dg, dm, dv, n, n_l2, l2x2, lr_t, b1, b2, eps, gscale, sc.s);
    sc.get(p, dp, n), sc.get(m, dm, n), sc.get(v, dv, n);
    return sc.status();
}

extern "C" int l3_op_arena_fold(int device, float* acc, float* g, int64_t total, int64_t off, int64_t n, int mode) {
    if (!acc || !g || total <= 0 || off < 0 || n < 0 || off > total || n > total - off || mode < ARENA_FOLD_SET || mode > ARENA_FOLD_OUT) {
        set_op_error("l3_op_arena_fold: NULL arena, a range [" + std::to_string(off) + ", " + std::to_string(off) + " + " +
                     std::to_string(n) + ") outside the " + std::to_string(total) + " floats, or mode " + std::to_string(mode) +
                     " (0 set, 1 add, 2 out)");
        return L3_EINVAL;
    }
    Scope sc(device);
    float* da = sc.put(acc, (size_t)total);
    float* dg = sc.put(g, (size_t)total);
    if (!sc.ok) return L3_ENOMEM;
    arena_fold(da + off, dg + off, n, mode, sc.s);
    sc.get(acc, da, (size_t)total), sc.get(g, dg, (size_t)total);
    return sc.status();
}

// ---- head, loss, L2 sums and BatchNorm moving averages on their own (elementwise.hip; model.py:25-31, train.py:270-284) ----------
namespace {
constexpr size_t HEAD_MAX_DYN_LDS = 64 * 1024;      // dynamic LDS of a launch that sets no function attribute
int head_op_check(const char* name, int device, bool ptrs_ok, int B, int K, int N, size_t lds_bytes) {
    if (ptrs_ok && B > 0 && K > 0 && N > 0 && lds_bytes > HEAD_MAX_DYN_LDS) {
        set_op_error(std::string(name) + ": K / N need " + std::to_string(lds_bytes) + " bytes of dynamic LDS, above the 65536 of a plain launch");
        return L3_EINVAL;
    }
    return mlp_op_check(name, device, ptrs_ok, B, K, N, nullptr, B);
}
}  // namespace

extern "C" int l3_op_head_dense_fwd(int device, const float* x, const float* w, const float* b, float* y, int B, int K, int N,
                                    int relu) {
    const int rc = head_op_check("l3_op_head_dense_fwd", device, x && w && b && y, B, K, N, ((size_t)K + 8 * (size_t)N) * 4);
    if (rc != L3_OK) return rc;
    Scope sc(device);
    const float* dx = sc.put(x, (size_t)B * K);
    const float* dw = sc.put(w, (size_t)K * N);
    const float* db = sc.put(b, (size_t)N);
    float* dy = sc.alloc<float>((size_t)B * N);
    if (!sc.ok) return L3_ENOMEM;
    dense_fwd(dx, dw, db, dy, B, K, N, relu ? 1 : 0, sc.s);
    sc.get(y, dy, (size_t)B * N);
    return sc.status();
}

extern "C" int l3_op_head_dense_bwd(int device, const float* x, const float* w, const float* dy, float* dw, float* db, float* dx,
                                    int B, int K, int N) {
    const int rc = head_op_check("l3_op_head_dense_bwd", device, x && w && dy && dw && db && dx, B, K, N, (size_t)N * 4);
    if (rc != L3_OK) return rc;
    Scope sc(device);
    const float* d_x = sc.put(x, (size_t)B * K);
    const float* d_w = sc.put(w, (size_t)K * N);
    const float* d_dy = sc.put(dy, (size_t)B * N);
    float* d_dw = sc.alloc<float>((size_t)K * N);
    float* d_db = sc.alloc<float>((size_t)N);
    float* d_dx = sc.alloc<float>((size_t)B * K);
    if (!sc.ok) return L3_ENOMEM;
    dense_bwd_w(d_x, d_dy, d_dw, d_db, B, K, N, sc.s);
    dense_bwd_x(d_dy, d_w, d_dx, B, K, N, sc.s);
    sc.get(dw, d_dw, (size_t)K * N);
    sc.get(db, d_db, (size_t)N);
    sc.get(dx, d_dx, (size_t)B * K);
    return sc.status();
}

extern "C" int l3_op_softmax_ce2(int device, const float* logits, const float* labels, int B, float gscale, float* probs,
                                 float* dlogits, float* stats) {
    const int rc = mlp_op_check("l3_op_softmax_ce2", device, logits && labels && probs && dlogits && stats, B, 1, 2, nullptr, B);
    if (rc != L3_OK) return rc;
    Scope sc(device);
    const float* d_z = sc.put(logits, (size_t)B * 2);
    const float* d_t = sc.put(labels, (size_t)B * 2);
    float* d_p = sc.alloc<float>((size_t)B * 2);
    float* d_g = sc.alloc<float>((size_t)B * 2);
    float* d_s = sc.alloc<float>(2);
    if (!sc.ok) return L3_ENOMEM;
    softmax_ce(d_z, d_t, d_p, d_g, d_s, B, gscale, sc.s);
    sc.get(probs, d_p, (size_t)B * 2);
    sc.get(dlogits, d_g, (size_t)B * 2);
    sc.get(stats, d_s, 2);
    return sc.status();
}

extern "C" int l3_op_sumsq(int device, const float* base, int64_t n_base, const int64_t* off, const int64_t* n, int count,
                           int multi, float* out) {
    if (!base || !off || !n || !out || n_base <= 0 || count <= 0 || (multi && count > SUMSQ_MAX_SEGS)) {
        set_op_error("l3_op_sumsq: NULL pointer, empty base, or a range count outside [1, " +
                     std::string(multi ? std::to_string(SUMSQ_MAX_SEGS) : "inf") + "]");
        return L3_EINVAL;
    }
    for (int i = 0; i < count; ++i)
        if (off[i] < 0 || n[i] < 0 || off[i] > n_base || n[i] > n_base - off[i]) {
            set_op_error("l3_op_sumsq: range " + std::to_string(i) + " outside base");
            return L3_EINVAL;
        }
    const int rc = mlp_op_check("l3_op_sumsq", device, true, 1, 1, 1, nullptr, 1);
    if (rc != L3_OK) return rc;
    Scope sc(device);
    const float* d_b = sc.put(base, (size_t)n_base);
    float* d_o = sc.alloc<float>((size_t)count);
    float* d_s = sc.alloc<float>(multi ? (size_t)SUMSQ_MAX_SEGS * SUMSQ_BLOCKS : sumsq_scratch_floats(n_base));
    if (!sc.ok) return L3_ENOMEM;
    if (multi) {
        SumsqSegs segs{};
        for (int i = 0; i < count; ++i) {
            segs.off[i] = off[i];
            segs.n[i] = n[i];
        }
        segs.count = count;
        sumsq_multi(d_b, segs, d_o, d_s, sc.s);
    } else {
        for (int i = 0; i < count; ++i) sumsq(d_b + off[i], n[i], d_o + i, d_s, sc.s);
    }
    sc.get(out, d_o, (size_t)count);
    return sc.status();
}

extern "C" int l3_op_bn_moving_update(int device, int entries, const int32_t* c, const int64_t* slot_off, int64_t n_slots,
                                      float* moving, float* biased, const float* batch, const float* gathered, int64_t n_gathered,
                                      int replicas, int64_t stride, float momentum, int zero_debias, int64_t step, float* packed,
                                      int64_t n_packed) {
    const char* name = "l3_op_bn_moving_update";
    if (!c || !slot_off || !moving || !biased || !batch || !packed || entries <= 0 || entries > 65535 || n_slots <= 0 || step < 1) {
        set_op_error(std::string(name) + ": NULL pointer, entry count outside [1, 65535] or step < 1");
        return L3_EINVAL;
    }
    int64_t total = 0;
    int max_c = 0;
    for (int i = 0; i < entries; ++i) {
        const int64_t end = i + 1 < entries ? slot_off[i + 1] : n_slots;
        if (c[i] <= 0 || slot_off[i] < 0 || slot_off[i] > end || c[i] > end - slot_off[i] || end > n_slots) {
            set_op_error(std::string(name) + ": entry " + std::to_string(i) + " does not fit its slot");
            return L3_EINVAL;
        }
        total += c[i];
        max_c = c[i] > max_c ? c[i] : max_c;
    }
    if (total > n_packed || total > INT32_MAX) {
        set_op_error(std::string(name) + ": packed holds fewer floats than the channel counts add up to");
        return L3_EINVAL;
    }
    if (gathered && (replicas < 1 || stride < total || n_gathered < (int64_t)(replicas - 1) * stride + total)) {
        set_op_error(std::string(name) + ": gathered needs replicas >= 1, stride >= the packed size and (replicas - 1) * stride + "
                     "the packed size floats");
        return L3_EINVAL;
    }
    const int rc = mlp_op_check(name, device, true, 1, 1, 1, nullptr, 1);
    if (rc != L3_OK) return rc;
    Scope sc(device);
    float* d_m = sc.put(moving, (size_t)n_slots);
    float* d_b = sc.put(biased, (size_t)n_slots);
    const float* d_v = sc.put(batch, (size_t)n_slots);
    const float* d_g = gathered ? sc.put(gathered, (size_t)n_gathered) : nullptr;
    float* d_p = sc.put(packed, (size_t)n_packed);
    std::vector<BnMovingEntry> tab;
    int off = 0;
    for (int i = 0; i < entries; ++i) {
        tab.push_back(BnMovingEntry{d_m + slot_off[i], d_b + slot_off[i], d_v + slot_off[i], c[i], off});
        off += c[i];
    }
    const BnMovingEntry* d_t = sc.put(tab.data(), tab.size());
    if (!sc.ok) return L3_ENOMEM;
    bn_moving_pack(d_t, entries, max_c, d_p, sc.s);
    bn_moving_update_all(d_t, entries, max_c, momentum, zero_debias ? 1 : 0, step, sc.s, d_g, replicas, stride);
    sc.get(moving, d_m, (size_t)n_slots);
    sc.get(biased, d_b, (size_t)n_slots);
    sc.get(packed, d_p, (size_t)n_packed);
    return sc.status();
}

// ---- VGGish operators (vggish.hip; data/usc/features.py:166-240) -------------------------------------------------------------
namespace {
int vggish_op_device(const char* name, Scope& sc, int device) {
    if (sc.ok) return L3_OK;
    set_op_error(no_gpu_message(name, device));
    return L3_EHIP;
}
}  // namespace

extern "C" int l3_op_vggish_logmel(int device, const float* x, int64_t n, const int64_t* segments, int64_t n_segments, float* out) {
    if (!x || !segments || !out || n < 0 || n_segments < 0) {
        set_op_error("l3_op_vggish_logmel: NULL pointer or negative count");
        return L3_EINVAL;
    }
    for (int64_t i = 0; i < n_segments; ++i) {
        const int64_t off = segments[2 * i], len = segments[2 * i + 1];
        if (off < 0 || len < 0 || off > n || len > n - off) {
            set_op_error("l3_op_vggish_logmel: segment " + std::to_string(i) + " outside x");
            return L3_EINVAL;
        }
    }
    std::vector<int64_t> blocks;
    const int64_t rows = vggish_logmel_blocks(segments, n_segments, &blocks, nullptr);
    if (rows == 0) return L3_OK;
    Scope sc(device);
    if (int rc = vggish_op_device("l3_op_vggish_logmel", sc, device)) return rc;
    std::vector<float> dft, mel;
    vggish_host_dft(&dft);
    vggish_host_mel(&mel);
    const float* d_x = sc.put(x, (size_t)n);
    const int64_t* d_b = sc.put(blocks.data(), blocks.size());
    const float* d_dft = sc.put(dft.data(), dft.size());
    const float* d_mel = sc.put(mel.data(), mel.size());
    float* d_o = sc.alloc<float>((size_t)rows * VG_MELS);
    if (!sc.ok) return L3_ENOMEM;
    vggish_logmel(d_x, d_b, (int64_t)blocks.size() / 3, d_dft, d_mel, d_o, sc.s);
    sc.get(out, d_o, (size_t)rows * VG_MELS);
    return sc.status();
}

extern "C" int l3_op_vggish_conv1(int device, const float* logmel, int64_t n_rows, const int64_t* example_rows, int64_t n_examples,
                                  const float* w, const float* b, float* y) {
    if (!logmel || !example_rows || !w || !b || !y || n_rows < 0 || n_examples < 0 || n_examples > (1 << 20)) {
        set_op_error("l3_op_vggish_conv1: NULL pointer or bad count");
        return L3_EINVAL;
    }
    for (int64_t e = 0; e < n_examples; ++e)
        if (example_rows[e] < 0 || example_rows[e] + VG_ROWS > n_rows) {
            set_op_error("l3_op_vggish_conv1: example " + std::to_string(e) + " outside the log-mel rows");
            return L3_EINVAL;
        }
    if (n_examples == 0) return L3_OK;
    Scope sc(device);
    if (int rc = vggish_op_device("l3_op_vggish_conv1", sc, device)) return rc;
    const float* d_l = sc.put(logmel, (size_t)n_rows * VG_MELS);
    const int64_t* d_e = sc.put(example_rows, (size_t)n_examples);
    const float* d_w = sc.put(w, 9 * 64);
    const float* d_b = sc.put(b, 64);
    const size_t ny = (size_t)n_examples * (VG_ROWS / 2) * (VG_MELS / 2) * 64;
    float* d_y = sc.alloc<float>(ny);
    if (!sc.ok) return L3_ENOMEM;
    vggish_conv1(d_l, d_e, d_w, d_b, d_y, (int)n_examples, sc.s);
    sc.get(y, d_y, ny);
    return sc.status();
}

extern "C" int l3_op_vggish_bias_relu(int device, const float* x, const float* b, float* y, int n, int h, int wd, int c, int pool) {
    if (!x || !b || !y || n <= 0 || h <= 0 || wd <= 0 || c <= 0 || c % 4 != 0 || (pool && (h % 2 != 0 || wd % 2 != 0))) {
        set_op_error("l3_op_vggish_bias_relu: NULL pointer, c not a multiple of 4, or an odd map under the pool");
        return L3_EINVAL;
    }
    Scope sc(device);
    if (int rc = vggish_op_device("l3_op_vggish_bias_relu", sc, device)) return rc;
    const size_t nx = (size_t)n * h * wd * c, ny = pool ? nx / 4 : nx;
    const float* d_x = sc.put(x, nx);
    const float* d_b = sc.put(b, (size_t)c);
    float* d_y = sc.alloc<float>(ny);
    if (!sc.ok) return L3_ENOMEM;
    vggish_bias_relu(d_x, d_b, d_y, n, h, wd, c, pool ? 1 : 0, sc.s);
    sc.get(y, d_y, ny);
    return sc.status();
}

extern "C" int l3_op_vggish_postprocess(int device, const float* emb, int64_t n, const float* pca_matrix, const float* pca_means,
                                        int quantize, float* out) {
    if (!emb || !pca_matrix || !pca_means || !out || n <= 0 || n > (1 << 24)) {
        set_op_error("l3_op_vggish_postprocess: NULL pointer or bad count");
        return L3_EINVAL;
    }
    Scope sc(device);
    if (int rc = vggish_op_device("l3_op_vggish_postprocess", sc, device)) return rc;
    std::vector<float> t((size_t)VG_EMB * VG_EMB);
    for (int j = 0; j < VG_EMB; ++j)
        for (int k = 0; k < VG_EMB; ++k) t[(size_t)k * VG_EMB + j] = pca_matrix[(size_t)j * VG_EMB + k];
    const float* d_e = sc.put(emb, (size_t)n * VG_EMB);
    const float* d_p = sc.put(t.data(), t.size());
    const float* d_m = sc.put(pca_means, (size_t)VG_EMB);
    float* d_o = sc.alloc<float>((size_t)n * VG_EMB);
    if (!sc.ok) return L3_ENOMEM;
    vggish_postprocess(d_e, d_p, d_m, d_o, (int)n, quantize ? 1 : 0, sc.s);
    sc.get(out, d_o, (size_t)n * VG_EMB);
    return sc.status();
}

// one of the five wide convolutions as the handle runs it: conv_fwd without bias under `fp32_conv` (a Winograd form where
// conv_wino_ok, else the implicit GEMM), then the bias + ReLU (+ pool) tail
extern "C" int l3_op_vggish_conv(int device, int fp32_conv, const float* x, const float* w, const float* b, float* y, int n, int h,
                                 int wd, int cin, int cout, int pool) {
    if (!x || !w || !b || !y || n <= 0 || h <= 0 || wd <= 0 || cin <= 0 || cout <= 0 || cout % 4 != 0 ||
        (pool && (h % 2 != 0 || wd % 2 != 0)) ||
        (fp32_conv != L3_FP32_CONV_F4X4 && fp32_conv != L3_FP32_CONV_F2X2 && fp32_conv != L3_VGGISH_CONV_DIRECT)) {
        set_op_error("l3_op_vggish_conv: NULL pointer, bad size, cout not a multiple of 4, an odd map under the pool, or a bad fp32_conv");
        return L3_EINVAL;
    }
    Scope sc(device);
    if (int rc = vggish_op_device("l3_op_vggish_conv", sc, device)) return rc;
    ConvGeom g = conv_geom(n, h, wd, cin, cout, 3, 3, true, fp32_conv == L3_FP32_CONV_F2X2 ? 1 : 0);
    g.solo = 1;
    const ConvFwdPath p = conv_resolve_fwd(g, ConvStorage{}, fp32_conv != L3_VGGISH_CONV_DIRECT);
    const size_t nx = (size_t)n * h * wd * cin, nc = (size_t)n * h * wd * cout, ny = pool ? nc / 4 : nc;
    ConvBufs cb;
    cb.x = sc.put(x, nx);
    cb.w = sc.put(w, (size_t)9 * cin * cout);
    const float* d_b = sc.put(b, (size_t)cout);
    cb.wino_u = p.wino_filter ? sc.alloc<float>(conv_wino_floats(g)) : nullptr;
    float* d_c = cb.y = sc.alloc<float>(nc);
    float* d_y = sc.alloc<float>(ny);
    if (!sc.ok) return L3_ENOMEM;
    conv_run_fwd(p, g, ConvStorage{}, cb, sc.s);
    vggish_bias_relu(d_c, d_b, d_y, n, h, wd, cout, pool ? 1 : 0, sc.s);
    sc.get(y, d_y, ny);
    return sc.status();
}
