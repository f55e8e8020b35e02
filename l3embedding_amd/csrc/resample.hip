// resample.hip -- band-limited resampling of whole clips on the GPU (resampy 0.2.x resample + resample_f, filter='kaiser_best').
//
// Replaces (reference call sites, relative to the reference tree):
//   resampy.resample(data, sr_orig, sr)   data/usc/features.py:25-26 (load_audio)
// One lane per output sample.  Output t of a clip of L native samples at sr_o, resampled to sr_n, sits at the exact rational time
// t * sr_o / sr_n: n = (t * sr_o) // sr_n and time - n = ((t * sr_o) % sr_n) / sr_n in f64 (resampy accumulates 1 / ratio in an
// f64 register instead; DESIGN.md section 8 states the deviation).  The taps are resampy's: a left wing on x[n - i] and a right
// wing on x[n + k + 1], weights interpolated from the half window and its differences, accumulated left wing first, each wing in
// tap order, as y = f32(f64(y) + w * f64(x)) -- the float32 output array of resampy's numba loop.  No fp contraction anywhere in
// this file: the weights and the sums must round as NumPy's float64 arithmetic rounds them (tests/resample_ref.py).
#include <cstring>

#include "../../include/l3hip.h"
#include "kernels.h"
#include "knobs.h"

#pragma clang fp contract(off)

namespace l3 {

// Block b resamples outputs [blocks[2b + 1], + 256) of clip blocks[2b] (clipped to the clip's range).  The filter table of a clip
// is tabs + d.table: nwin (win, delta) pairs, one 16-byte load per tap; d.table < 0 copies x[t] instead (a clip already at the
// target rate, which load_audio never resamples).
__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ x, const ResampleClip* __restrict__ clips,
                                                       const int64_t* __restrict__ blocks, const double2* __restrict__ tabs,
                                                       int nwin, int num_table, float* __restrict__ y) {
    const ResampleClip d = clips[blocks[2 * (int64_t)blockIdx.x]];
    const int64_t t = blocks[2 * (int64_t)blockIdx.x + 1] + threadIdx.x;
    if (t >= d.t0 + d.n_out) return;
    float* dst = y + d.y_off + (t - d.t0);
    const float* xc = x + d.x_off;
    if (d.table < 0) {
        *dst = xc[t];
        return;
    }
    const int64_t num = t * d.sr_o;
    const int64_t n = num / d.sr_n;
    if (n >= d.L) {             // never for t < int(L * ratio) (the host checks the range); kept so no read leaves the clip
        *dst = 0.f;
        return;
    }
    const double ratio = (double)d.sr_n / (double)d.sr_o;
    const double scale = ratio < 1.0 ? ratio : 1.0;
    const int64_t step = (int64_t)(scale * num_table);
    const double2* tab = tabs + d.table;

    double frac = scale * ((double)(num - n * d.sr_n) / (double)d.sr_n);
    double index_frac = frac * num_table;
    int64_t offset = (int64_t)index_frac;
    double eta = index_frac - (double)offset;
    int64_t imax = (nwin - offset) / step;
    if (imax > n + 1) imax = n + 1;
    float acc = 0.f;
    for (int64_t i = 0; i < imax; ++i) {
        const double2 we = tab[offset + i * step];
        const double w = we.x + eta * we.y;
        acc = (float)((double)acc + w * (double)xc[n - i]);
    }
    frac = scale - frac;
    index_frac = frac * num_table;
    offset = (int64_t)index_frac;
    eta = index_frac - (double)offset;
    int64_t kmax = (nwin - offset) / step;
    if (kmax > d.L - n - 1) kmax = d.L - n - 1;
    for (int64_t k = 0; k < kmax; ++k) {
        const double2 we = tab[offset + k * step];
        const double w = we.x + eta * we.y;
        acc = (float)((double)acc + w * (double)xc[n + k + 1]);
    }
    *dst = acc;
}

int64_t resample_out_len(int64_t L, int64_t sr_o, int64_t sr_n) {
    const double ratio = (double)sr_n / (double)sr_o;        // resampy: float(sr_new) / sr_orig, then int(L * ratio)
    return (int64_t)((double)L * ratio);
}

const char* resample_clips_error(const int64_t* clips, int64_t n_clips, int64_t n_native, int64_t sr_new, int64_t n_window,
                                 int num_table, int64_t n_samples, bool copy_equal, int64_t* bad) {
    *bad = -1;
    if (sr_new <= 0) return "sr_new <= 0";
    if (n_window < 1 || n_window > ((int64_t)1 << 30)) return "n_window out of range [1, 2^30]";
    if (num_table < 1) return "num_table < 1";
    const int64_t lim = (int64_t)1 << 40;
    for (int64_t c = 0; c < n_clips; ++c) {
        const int64_t* r = clips + RESAMPLE_ROW * c;
        const int64_t x_off = r[0], L = r[1], sr_o = r[2], t0 = r[3], n_out = r[4], y_off = r[5];
        *bad = c;
        if (sr_o <= 0) return "sr_orig <= 0";
        if (sr_o > ((int64_t)1 << 24) || sr_new > ((int64_t)1 << 24)) return "sample rate above 2^24 Hz";
        if (L < 0 || L > lim) return "native length out of range";
        // the kernel forms t * sr_orig < (L + 1) * max(sr_orig, sr_new) in int64
        if (!(copy_equal && sr_o == sr_new) && L + 1 > ((int64_t)1 << 62) / (sr_o > sr_new ? sr_o : sr_new))
            return "native length times sample rate reaches 2^62";
        if (x_off < 0 || x_off > n_native - L) return "native samples outside the upload";
        const bool copy = copy_equal && sr_o == sr_new;
        const int64_t len = copy ? L : resample_out_len(L, sr_o, sr_new);
        if (!copy && len < 1) return "input too short to resample (output length < 1)";
        if (!copy && (int64_t)(((double)sr_new / (double)sr_o < 1.0 ? (double)sr_new / (double)sr_o : 1.0) * num_table) < 1)
            return "filter step int(scale * num_table) < 1";
        if (t0 < 0 || n_out < 0 || t0 > len - n_out) return "output range past the output length";
        if (y_off < 0 || y_off > n_samples - n_out) return "destination outside the output buffer";
    }
    *bad = -1;
    return nullptr;
}

namespace {
void resample_plan(const int64_t* clips, int64_t n_clips, int64_t sr_new, const double* half_window, int64_t n_window,
                   bool copy_equal, ResampleTables* tabs, ResamplePlan* p) {
    p->clips.clear();
    p->blocks.clear();
    if (tabs->window.size() != (size_t)n_window ||
        std::memcmp(tabs->window.data(), half_window, (size_t)n_window * sizeof(double)) != 0) {
        tabs->window.assign(half_window, half_window + n_window);         // another window: every table is rebuilt
        tabs->keys.clear();
        tabs->tables.clear();
        ++tabs->generation;
    }
    for (int64_t c = 0; c < n_clips; ++c) {
        const int64_t* r = clips + RESAMPLE_ROW * c;
        ResampleClip d{};
        d.x_off = r[0]; d.L = r[1]; d.sr_o = r[2]; d.sr_n = sr_new; d.t0 = r[3]; d.n_out = r[4]; d.y_off = r[5]; d.table = -1;
        if (!(copy_equal && d.sr_o == sr_new)) {
            const double ratio = (double)sr_new / (double)d.sr_o;
            const double key = ratio < 1.0 ? ratio : 1.0;
            size_t k = 0;
            while (k < tabs->keys.size() && tabs->keys[k] != key) ++k;
            if (k == tabs->keys.size()) {
                tabs->keys.push_back(key);
                ++tabs->generation;
                // resampy: interp_win *= sample_ratio when sample_ratio < 1; interp_delta[:-1] = diff(interp_win), last 0
                const size_t base = tabs->tables.size();
                tabs->tables.resize(base + 2 * (size_t)n_window);
                double* tb = tabs->tables.data() + base;
                for (int64_t i = 0; i < n_window; ++i) tb[2 * i] = ratio < 1.0 ? half_window[i] * ratio : half_window[i];
                for (int64_t i = 0; i + 1 < n_window; ++i) tb[2 * i + 1] = tb[2 * (i + 1)] - tb[2 * i];
                tb[2 * (n_window - 1) + 1] = 0.0;
            }
            d.table = (int64_t)k * n_window;
        }
        for (int64_t t = d.t0; t < d.t0 + d.n_out; t += 256) {
            p->blocks.push_back((int64_t)p->clips.size());
            p->blocks.push_back(t);
        }
        p->clips.push_back(d);
    }
}

void resample_launch(const float* x, const ResampleClip* clips, const int64_t* blocks, int64_t n_blocks, const double* tabs,
                     int nwin, int num_table, float* y, hipStream_t s) {
    for (int64_t b0 = 0; b0 < n_blocks; b0 += (int64_t)1 << 30) {        // gridDim.x limit
        const int64_t nb = n_blocks - b0 < ((int64_t)1 << 30) ? n_blocks - b0 : ((int64_t)1 << 30);
        hipLaunchKernelGGL(resample_kernel, dim3((unsigned)nb), dim3(256), 0, s, x, clips, blocks + 2 * b0,
                           reinterpret_cast<const double2*>(tabs), nwin, num_table, y);
    }
}

}  // namespace

int ResampleStage::run(const float* native, int64_t n_native, const int64_t* clips, int64_t n_clips, int64_t sr_new,
                       const double* half_window, int64_t n_window, int num_table, bool copy_equal, float* d_out, int64_t n_samples,
                       hipStream_t s, std::string* err) {
    ResamplePlan plan;
    resample_plan(clips, n_clips, sr_new, half_window, n_window, copy_equal, &tabs, &plan);
    bufs.grow(&d_native, &cap_native, (size_t)n_native);
    bufs.grow(&d_clips, &cap_clips, plan.clips.size());
    bufs.grow(&d_blocks, &cap_blocks, plan.blocks.size());
    if (bufs.grow(&d_tabs, &cap_tabs, tabs.tables.size())) tabs_on_device = ~(uint64_t)0;      // a new buffer holds nothing yet
    if (!d_native || !d_clips || !d_blocks || !d_tabs) {
        *err = "hipMalloc of the resampling buffers failed";
        return L3_ENOMEM;
    }
    auto up = [s](void* dst, const void* src, size_t bytes) {
        return bytes == 0 ? hipSuccess : hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s);
    };
    const bool new_tabs = tabs_on_device != tabs.generation;          // only a new window scale or another window uploads
    tabs_on_device = ~(uint64_t)0;
    hipError_t st = up(d_native, native, (size_t)n_native * sizeof(float));
    if (st == hipSuccess) st = up(d_clips, plan.clips.data(), plan.clips.size() * sizeof(ResampleClip));
    if (st == hipSuccess) st = up(d_blocks, plan.blocks.data(), plan.blocks.size() * sizeof(int64_t));
    if (st == hipSuccess && new_tabs) st = up(d_tabs, tabs.tables.data(), tabs.tables.size() * sizeof(double));
    // the copies read `plan`, which ends with this call, and `tabs`, which the next call may rebuild: none is left in flight
    const hipError_t waited = stream_wait(s);
    if (st != hipSuccess || waited != hipSuccess) {
        *err = std::string("resampling upload: ") + hipGetErrorString(st != hipSuccess ? st : waited);
        return L3_EHIP;
    }
    tabs_on_device = tabs.generation;
    // samples no clip row writes read as zeros
    if (n_samples > 0 && (st = hipMemsetAsync(d_out, 0, (size_t)n_samples * sizeof(float), s)) != hipSuccess) {
        *err = std::string("resampling zero-fill: ") + hipGetErrorString(st);
        return L3_EHIP;
    }
    resample_launch(d_native, d_clips, d_blocks, (int64_t)plan.blocks.size() / 2, d_tabs, (int)n_window, num_table, d_out, s);
    return L3_OK;
}

}  // namespace l3
