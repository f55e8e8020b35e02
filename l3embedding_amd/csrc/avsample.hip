// avsample.hip -- AVC training samples cut on the GPU from decoded clips that live there.
//
// Replaces (reference call sites, relative to the reference tree), once the clips are decoded and the draws are made:
//   the mono mix                 data/avc/sample.py:445-448   audio.mean(axis=-1).astype('int16')
//   the second and its padding   data/avc/sample.py:136-144   audio[start : start + 48000], zeros past the clip's end
//   the frame and its crop       data/avc/sample.py:234,181-191  video[frame][start_x : start_x + 224, start_y : start_y + 224]
//   read_video's resize          data/avc/sample.py:303-310   (csrc/frames.hip's resize instead of ffmpeg's scaler: DESIGN.md 8n, 8o)
// The rule of WHICH second, frame and crop lives in l3embedding_amd/avsample.py (draw_samples, the reference's order of random
// calls); this file holds the bank (l3_clipbank: two arenas filled by bump allocation, nothing ever moves), the two kernels and
// the host-side check that turns a batch of l3_sample records into the tables the kernels and image_frames follow.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>

#include "../../include/l3hip.h"
#include "kernels.h"
#include "knobs.h"

struct l3_clipbank {
    struct Clip {
        int64_t pix_off, aud_off, samples;
        int frames, H, W, Ho, Wo;
    };
    int device = 0, resize = 0;
    int64_t pixel_cap = 0, audio_cap = 0, pixel_used = 0, audio_used = 0;
    uint8_t* pixels = nullptr;
    int16_t* audio = nullptr;          // holds audio_cap rounded up to 8 samples: audio_seconds reads whole 16-byte vectors
    int16_t* staging = nullptr;        // an upload's interleaved channels, grown on demand
    size_t staging_cap = 0;
    hipStream_t stream = nullptr;
    std::vector<Clip> clips;
    l3::DeviceBufs bufs;
};

static_assert(sizeof(l3_sample) == 56 && offsetof(l3_sample, u_gain) == 24 && offsetof(l3_sample, aug) == 32,
              "the record layout l3embedding_amd/avsample.py SAMPLE packs");

namespace l3 {

namespace {

constexpr int VEC = 8;          // int16 per 16-byte vector

// numpy's mean over the channels of one sample, then astype('int16'): the sum of up to 8 int16 is exact in float64 whatever the
// order, one IEEE division, truncation toward zero (|mean| <= 32768 and -32768 itself is an int16)
__host__ __device__ inline int16_t downmix_one(const int16_t* x, int C) {
    double sum = 0.0;
    for (int c = 0; c < C; ++c) sum += (double)x[c];
    return (int16_t)(int)(sum / (double)C);
}

// One thread per 8 consecutive outputs: C 16-byte loads (its 8 C interleaved inputs start at a multiple of 16 bytes), one 16-byte
// store.  The ragged tail (n % 8 outputs) is one thread's, element by element.
template <int C>
__global__ __launch_bounds__(256) void downmix_kernel(const int16_t* __restrict__ in, int16_t* __restrict__ out, int64_t n) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i0 = g * VEC;
    if (i0 >= n) return;
    if (i0 + VEC <= n) {
        int16_t x[VEC * C], y[VEC];
        const uint4* p = reinterpret_cast<const uint4*>(in + i0 * C);
#pragma unroll
        for (int k = 0; k < C; ++k) {
            const uint4 v = p[k];
            __builtin_memcpy(x + VEC * k, &v, sizeof(v));
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) y[j] = downmix_one(x + j * C, C);
        uint4 o;
        __builtin_memcpy(&o, y, sizeof(o));
        *reinterpret_cast<uint4*>(out + i0) = o;
    } else {
        for (int64_t i = i0; i < n; ++i) out[i] = downmix_one(in + i * C, C);
    }
}

// elements [a, a + 8) of the 16 int16 in (lo, hi), a in [1, 7]: what an unaligned 16-byte load at lo + a would return
__device__ __forceinline__ uint4 funnel(const uint4 lo, const uint4 hi, int a) {
    const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
    uint32_t o[4];
    const int wo = a >> 1;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t x0 = 0, x1 = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {          // (a is uniform over the workgroup: a select chain, no indexed registers)
            x0 = wo == q ? w[k + q] : x0;
            x1 = wo == q ? w[k + q + 1] : x1;
        }
        o[k] = (a & 1) ? (x0 >> 16) | (x1 << 16) : x0;
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}

// Grid (T / 8 / 256, rows): one thread per 16-byte vector of an output row, whose table entry is uniform over the workgroup.
// Vectors that lie wholly inside the clip come from 16-byte loads -- one when the row's source offset is a multiple of 8 samples,
// else the two aligned vectors around it, shifted together -- the vector that straddles the clip's end element by element, the
// rest of the row is zeros.  The second aligned load may reach past the clip's last sample by up to 7 samples, never past the
// arena (rounded up to whole vectors by its owner); none of those samples reaches the output.
__global__ __launch_bounds__(256) void seconds_kernel(const int16_t* __restrict__ samples, const int64_t* __restrict__ table,
                                                      int16_t* __restrict__ out, int T) {
    const int row = blockIdx.y;
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k * VEC >= T) return;
    const int64_t src = table[2 * (int64_t)row], valid = table[2 * (int64_t)row + 1];
    const int64_t j0 = (int64_t)k * VEC;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (j0 + VEC <= valid) {
        const int a = (int)(src & (VEC - 1));
        const uint4* p = reinterpret_cast<const uint4*>(samples + (src - a)) + k;
        v = p[0];
        if (a != 0) v = funnel(v, p[1], a);
    } else if (j0 < valid) {
        int16_t x[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) x[e] = j0 + e < valid ? samples[src + j0 + e] : (int16_t)0;
        __builtin_memcpy(&v, x, sizeof(v));
    }
    reinterpret_cast<uint4*>(out + (int64_t)row * T)[k] = v;
}

}  // namespace

void audio_downmix(const int16_t* in, int16_t* out, int64_t n, int C, hipStream_t s) {
    if (n <= 0) return;
    const int64_t threads = (n + VEC - 1) / VEC;
    const dim3 grid((unsigned)((threads + 255) / 256)), block(256);
    switch (C) {
        case 1: hipLaunchKernelGGL(downmix_kernel<1>, grid, block, 0, s, in, out, n); break;
        case 2: hipLaunchKernelGGL(downmix_kernel<2>, grid, block, 0, s, in, out, n); break;
        case 3: hipLaunchKernelGGL(downmix_kernel<3>, grid, block, 0, s, in, out, n); break;
        case 4: hipLaunchKernelGGL(downmix_kernel<4>, grid, block, 0, s, in, out, n); break;
        case 5: hipLaunchKernelGGL(downmix_kernel<5>, grid, block, 0, s, in, out, n); break;
        case 6: hipLaunchKernelGGL(downmix_kernel<6>, grid, block, 0, s, in, out, n); break;
        case 7: hipLaunchKernelGGL(downmix_kernel<7>, grid, block, 0, s, in, out, n); break;
        case 8: hipLaunchKernelGGL(downmix_kernel<8>, grid, block, 0, s, in, out, n); break;
        default: break;          // (the callers have checked 1 <= C <= 8)
    }
}

void audio_seconds(const int16_t* samples, const int64_t* table, int16_t* out, int rows, int T, hipStream_t s) {
    if (rows <= 0 || T <= 0) return;
    const int vecs = T / VEC;          // T % 8 == 0: the callers' rows are SAMPLE_T long
    for (int r0 = 0; r0 < rows; r0 += 65535) {          // gridDim.y limit
        const int nr = rows - r0 < 65535 ? rows - r0 : 65535;
        hipLaunchKernelGGL(seconds_kernel, dim3((vecs + 255) / 256, nr), dim3(256), 0, s, samples, table + 2 * (int64_t)r0,
                           out + (int64_t)r0 * T, T);
    }
}

int clipbank_device(const ::l3_clipbank* bank) { return bank->device; }

int sampled_plan(const ::l3_clipbank* bank, const ::l3_sample* rec, int n, bool aug, SampledHost* out, std::string* err) {
    const int64_t n_clips = (int64_t)bank->clips.size();
    auto bad = [&](int i, const std::string& what) {
        *err = "sample " + std::to_string(i) + ": " + what;
        return L3_EINVAL;
    };
    out->n = n, out->aug = aug;
    out->pixels = bank->pixels, out->audio = bank->audio;
    out->table.resize((size_t)n * IMAGE_ROW);
    out->seconds.resize((size_t)n * 2);
    out->labels.resize((size_t)n * 2);
    out->params.resize(aug ? (size_t)n : 0);
    out->u.resize(aug ? (size_t)n : 0);
    for (int i = 0; i < n; ++i) {
        const l3_sample& r = rec[i];
        if (r.video_clip < 0 || r.video_clip >= n_clips)
            return bad(i, "video_clip " + std::to_string(r.video_clip) + " is not one of the bank's " + std::to_string(n_clips) + " clips");
        if (r.audio_clip < 0 || r.audio_clip >= n_clips)
            return bad(i, "audio_clip " + std::to_string(r.audio_clip) + " is not one of the bank's " + std::to_string(n_clips) + " clips");
        const l3_clipbank::Clip &vc = bank->clips[r.video_clip], &ac = bank->clips[r.audio_clip];
        if (r.frame < 0 || r.frame >= vc.frames)
            return bad(i, "frame " + std::to_string(r.frame) + " outside the clip's " + std::to_string(vc.frames) + " frames");
        const int64_t last = ac.samples > SAMPLE_T ? ac.samples - SAMPLE_T : 0;
        if (r.audio_start < 0 || r.audio_start > last)
            return bad(i, "audio_start " + std::to_string(r.audio_start) + " outside [0, " + std::to_string(last) + "]");
        if (r.aug.start_x < 0 || r.aug.start_x > vc.Ho - IMG || r.aug.start_y < 0 || r.aug.start_y > vc.Wo - IMG)
            return bad(i, "the crop at (" + std::to_string(r.aug.start_x) + ", " + std::to_string(r.aug.start_y) + ") is outside the " +
                              std::to_string(vc.Ho) + " x " + std::to_string(vc.Wo) + " frame");
        if (r.label != 0 && r.label != 1) return bad(i, "label " + std::to_string(r.label) + " is neither 0 nor 1");
        int64_t* t = out->table.data() + (size_t)i * IMAGE_ROW;
        t[0] = vc.pix_off + (int64_t)r.frame * 3 * vc.H * vc.W;
        t[1] = vc.H, t[2] = vc.W, t[3] = vc.Ho, t[4] = vc.Wo;
        t[5] = r.aug.start_x, t[6] = r.aug.start_y;
        const int64_t rest = ac.samples - r.audio_start;
        out->seconds[2 * (size_t)i] = ac.aud_off + r.audio_start;
        out->seconds[2 * (size_t)i + 1] = rest < SAMPLE_T ? rest : SAMPLE_T;
        out->labels[2 * (size_t)i] = r.label;
        out->labels[2 * (size_t)i + 1] = 1 - r.label;
        if (aug) {
            AugmentParams& p = out->params[i];
            p.start_x = p.start_y = 0;          // the crop is done by the time these records are read
            p.flip = r.aug.flip, p.sat_first = r.aug.sat_first;
            p.saturation = r.aug.saturation, p.brightness = r.aug.brightness;
            out->u[i] = r.u_gain;
        }
    }
    int64_t row = 0;
    if (const char* why = image_table_error(out->table.data(), n, bank->pixel_used, &row)) return bad((int)row, why);
    image_plan(out->table.data(), n, &out->plan);
    return L3_OK;
}

}  // namespace l3

using namespace l3;

extern "C" {

int l3_clipbank_create(int device, int64_t pixel_bytes, int64_t audio_samples, int resize, l3_clipbank** bank) {
    if (!bank) return fail(L3_EINVAL, "l3_clipbank_create: NULL bank");
    *bank = nullptr;
    if (pixel_bytes < 1 || audio_samples < 1 || (resize != 0 && (resize <= IMG || resize > IMAGE_MAX_SIDE)))
        return fail(L3_EINVAL, "l3_clipbank_create: pixel_bytes and audio_samples must be >= 1, resize 0 or in [225, 8192]");
    if (!device_ok(device)) return fail(L3_EHIP, no_gpu_message("l3_clipbank_create", device));
    l3_clipbank* b = new l3_clipbank();
    b->device = device, b->resize = resize;
    b->pixel_cap = pixel_bytes, b->audio_cap = audio_samples;
    const size_t audio_alloc = ((size_t)audio_samples + VEC - 1) / VEC * VEC;
    b->pixels = b->bufs.alloc<uint8_t>((size_t)pixel_bytes);
    b->audio = b->bufs.alloc<int16_t>(audio_alloc);
    if (!b->pixels || !b->audio || hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMemsetAsync(b->audio, 0, audio_alloc * sizeof(int16_t), b->stream) != hipSuccess || stream_wait(b->stream) != hipSuccess) {
        (void)hipGetLastError();
        if (b->stream) (void)hipStreamDestroy(b->stream);
        delete b;
        return fail(L3_ENOMEM, "l3_clipbank_create: could not allocate " + std::to_string(pixel_bytes) + " bytes of pixels and " +
                                   std::to_string(audio_samples) + " samples of audio");
    }
    *bank = b;
    return L3_OK;
}

int l3_clipbank_add(l3_clipbank* b, const uint8_t* frames, int n_frames, int h, int w, const int16_t* audio, int64_t n, int channels,
                    int* clip_id) {
    if (!b || !frames || !audio || !clip_id) return fail(L3_EINVAL, "l3_clipbank_add: NULL pointer");
    if (n_frames < 1 || n < 1) return fail(L3_EINVAL, "l3_clipbank_add: a clip needs at least one frame and one sample");
    if (h < 1 || h > IMAGE_MAX_SIDE || w < 1 || w > IMAGE_MAX_SIDE)
        return fail(L3_EINVAL, "l3_clipbank_add: frame sides must be in [1, 8192]");
    if (b->resize == 0 && (h <= IMG || w <= IMG))
        return fail(L3_EINVAL, "l3_clipbank_add: frames of " + std::to_string(h) + " x " + std::to_string(w) +
                                   " in a bank without a resize: both sides must be >= 225");
    if (channels < 1 || channels > DOWNMIX_MAX_CHANNELS) return fail(L3_EINVAL, "l3_clipbank_add: channels must be in [1, 8]");
    if (n > (int64_t)INT32_MAX) return fail(L3_EINVAL, "l3_clipbank_add: a clip holds at most 2^31 - 1 samples");
    l3_clipbank::Clip c{};
    c.frames = n_frames, c.H = h, c.W = w, c.samples = n;
    if (b->resize == 0) {
        c.Ho = h, c.Wo = w;
    } else {          // read_video's rule (sample.py:303-305), features.image_table's operations
        const double scaling = (double)b->resize / (double)(w < h ? w : h);
        c.Ho = (int)std::ceil(scaling * (double)h);
        c.Wo = (int)std::ceil(scaling * (double)w);
        if (c.Ho > IMAGE_MAX_SIDE || c.Wo > IMAGE_MAX_SIDE)
            return fail(L3_EINVAL, "l3_clipbank_add: the resized frame would be " + std::to_string(c.Ho) + " x " + std::to_string(c.Wo));
    }
    const int64_t bytes = (int64_t)n_frames * 3 * h * w;
    c.pix_off = b->pixel_used;
    c.aud_off = (b->audio_used + VEC - 1) / VEC * VEC;          // clips start on a 16-byte boundary: the downmix stores vectors
    if (bytes > b->pixel_cap - c.pix_off || n > b->audio_cap - c.aud_off)
        return fail(L3_ENOMEM, "l3_clipbank_add: the bank is full: the clip needs " + std::to_string(bytes) + " bytes of pixels and " +
                                   std::to_string(n) + " samples, " + std::to_string(b->pixel_cap - c.pix_off) + " of " +
                                   std::to_string(b->pixel_cap) + " bytes and " +
                                   std::to_string(b->audio_cap > c.aud_off ? b->audio_cap - c.aud_off : 0) + " of " +
                                   std::to_string(b->audio_cap) + " samples are free");
    if (hipSetDevice(b->device) != hipSuccess) return fail(L3_EHIP, "l3_clipbank_add: hipSetDevice failed");
    hipError_t st = hipMemcpyAsync(b->pixels + c.pix_off, frames, (size_t)bytes, hipMemcpyHostToDevice, b->stream);
    if (st == hipSuccess && channels == 1) {
        st = hipMemcpyAsync(b->audio + c.aud_off, audio, (size_t)n * sizeof(int16_t), hipMemcpyHostToDevice, b->stream);
    } else if (st == hipSuccess) {
        const size_t count = (size_t)n * channels;
        if (count > b->staging_cap) {
            if (stream_wait(b->stream) != hipSuccess) return fail(L3_EHIP, "l3_clipbank_add: the bank's stream failed");
            if (!b->bufs.grow(&b->staging, &b->staging_cap, count))
                return fail(L3_ENOMEM, "l3_clipbank_add: hipMalloc(" + std::to_string(count * sizeof(int16_t)) + ") for the channels failed");
        }
        st = hipMemcpyAsync(b->staging, audio, count * sizeof(int16_t), hipMemcpyHostToDevice, b->stream);
        if (st == hipSuccess) {
            audio_downmix(b->staging, b->audio + c.aud_off, n, channels, b->stream);
            st = hipGetLastError();
        }
    }
    if (st == hipSuccess) st = stream_wait(b->stream);
    if (st != hipSuccess) return fail(L3_EHIP, std::string("l3_clipbank_add: ") + hipGetErrorString(st));
    b->pixel_used = c.pix_off + bytes;
    b->audio_used = c.aud_off + n;
    *clip_id = (int)b->clips.size();
    b->clips.push_back(c);
    return L3_OK;
}

int l3_clipbank_info(const l3_clipbank* b, int clip, int64_t* info) {
    if (!b || !info) return fail(L3_EINVAL, "l3_clipbank_info: NULL pointer");
    if (clip == -1) {
        info[0] = (int64_t)b->clips.size(), info[1] = b->pixel_used, info[2] = b->pixel_cap;
        info[3] = b->audio_used, info[4] = b->audio_cap, info[5] = b->resize;
        return L3_OK;
    }
    if (clip < 0 || clip >= (int)b->clips.size())
        return fail(L3_EINVAL, "l3_clipbank_info: clip " + std::to_string(clip) + " of " + std::to_string(b->clips.size()));
    const l3_clipbank::Clip& c = b->clips[clip];
    info[0] = c.frames, info[1] = c.H, info[2] = c.W, info[3] = c.Ho, info[4] = c.Wo, info[5] = c.samples;
    return L3_OK;
}

int l3_clipbank_audio(l3_clipbank* b, int clip, int16_t* out) {
    if (!b || !out) return fail(L3_EINVAL, "l3_clipbank_audio: NULL pointer");
    if (clip < 0 || clip >= (int)b->clips.size())
        return fail(L3_EINVAL, "l3_clipbank_audio: clip " + std::to_string(clip) + " of " + std::to_string(b->clips.size()));
    const l3_clipbank::Clip& c = b->clips[clip];
    if (hipSetDevice(b->device) != hipSuccess ||
        hipMemcpy(out, b->audio + c.aud_off, (size_t)c.samples * sizeof(int16_t), hipMemcpyDeviceToHost) != hipSuccess)
        return fail(L3_EHIP, "l3_clipbank_audio: the download failed");
    return L3_OK;
}

void l3_clipbank_destroy(l3_clipbank* b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    (void)hipDeviceSynchronize();          // a batch staged from the arenas may still be reading them
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
}

}  // extern "C"
