// batch_feed.hip -- BatchFeed (kernels.h): the one way a training batch in the stored dtypes reaches an engine's float inputs.
#include <hip/hip_runtime.h>

#include <utility>

#include "../../include/l3hip.h"
#include "kernels.h"
#include "knobs.h"

namespace l3 {

namespace {

constexpr size_t FRAME = 224 * 224 * 3;

#define FEEDCHK(call)                                                  \
    do {                                                               \
        hipError_t _st = (call);                                       \
        if (_st != hipSuccess) {                                       \
            *err = std::string(#call) + ": " + hipGetErrorString(_st); \
            return L3_EHIP;                                            \
        }                                                              \
    } while (0)

template <class T>
int grow(DeviceBufs& bufs, T** p, size_t* cap, size_t count, std::string* err) {
    if (count <= *cap) return L3_OK;
    if (bufs.grow(p, cap, count)) return L3_OK;        // (hipFree of the old buffer waits for the device: no reader is left)
    *err = "hipMalloc(" + std::to_string(DeviceBufs::bytes_of<T>(count)) + "): " + hipGetErrorString(hipGetLastError());
    return L3_ENOMEM;
}

bool is_global(BatchForm f) { return f == BATCH_GLOBAL || f == BATCH_GLOBAL_FLOAT; }

}  // namespace

void BatchFeed::bind(int rows, int samples, float* video, float* audio, float* labels) {
    B = rows, T = samples;
    out_video = video, out_audio = audio, out_labels = labels;
}

void BatchFeed::inputs_replaced(BatchForm form) {
    if (nxt.form != BATCH_NONE && is_global(nxt.form) == is_global(form)) nxt.form = BATCH_NONE;
    if (!is_global(form)) gains_valid = false;
}

// The one send: `slices` x B rows into `dst` on s, buffers grown on demand; a null input is left as it was, the records go only
// with an augmented batch.
int BatchFeed::send(RawBatch& dst, BatchForm form, int slices, const uint8_t* video_u8, const int16_t* audio_i16,
                    const int32_t* labels_i32, const AugmentParams* params, const double* u, hipStream_t s, std::string* err) {
    const size_t rows = (size_t)slices * B;
    int rc;
    if ((rc = grow(bufs, &dst.video, &dst.cap_video, rows * FRAME, err))) return rc;
    if ((rc = grow(bufs, &dst.audio, &dst.cap_audio, rows * T, err))) return rc;
    if ((rc = grow(bufs, &dst.labels, &dst.cap_labels, rows * 2, err))) return rc;
    if (params) {
        if ((rc = grow(bufs, &dst.params, &dst.cap_params, rows, err))) return rc;
        if ((rc = grow(bufs, &dst.u, &dst.cap_u, rows, err))) return rc;
        if (!gains && !(gains = bufs.alloc<double>((size_t)B))) {
            *err = "hipMalloc of the batch gains failed";
            return L3_ENOMEM;
        }
    }
    dst.form = BATCH_NONE;      // until every copy is enqueued
    // host memory is the caller's (pageable) array: these calls return once it has been read, while the device side of a staged
    // copy overlaps whatever the engine's streams are running
    if (params) {
        FEEDCHK(hipMemcpyAsync(dst.params, params, rows * sizeof(AugmentParams), hipMemcpyHostToDevice, s));
        FEEDCHK(hipMemcpyAsync(dst.u, u, rows * sizeof(double), hipMemcpyHostToDevice, s));
    }
    if (video_u8) FEEDCHK(hipMemcpyAsync(dst.video, video_u8, rows * FRAME, hipMemcpyHostToDevice, s));
    if (audio_i16) FEEDCHK(hipMemcpyAsync(dst.audio, audio_i16, rows * T * sizeof(int16_t), hipMemcpyHostToDevice, s));
    if (labels_i32) FEEDCHK(hipMemcpyAsync(dst.labels, labels_i32, rows * 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    dst.form = form, dst.slices = slices, dst.aug = params != nullptr;
    return L3_OK;
}

int BatchFeed::upload(BatchForm form, int slices, const uint8_t* video_u8, const int16_t* audio_i16, const int32_t* labels_i32,
                      const AugmentParams* params, const double* u, hipStream_t s, std::string* err) {
    inputs_replaced(form);      // an explicit upload supersedes a staged batch of its kind
    int rc = send(cur, form, slices, video_u8, audio_i16, labels_i32, params, u, s, err);
    if (rc) return rc;
    if (form == BATCH_SINGLE && (rc = convert(0, s, err, video_u8 != nullptr, audio_i16 != nullptr, labels_i32 != nullptr))) return rc;
    FEEDCHK(stream_wait(s));
    return L3_OK;
}

int BatchFeed::upload_float(int slices, const float* video, const float* audio, const float* labels, hipStream_t s, std::string* err) {
    const size_t rows = (size_t)slices * B;
    int rc;
    if ((rc = grow(bufs, &f_video, &cap_f_video, rows * FRAME, err))) return rc;
    if ((rc = grow(bufs, &f_audio, &cap_f_audio, rows * T, err))) return rc;
    if ((rc = grow(bufs, &f_labels, &cap_f_labels, rows * 2, err))) return rc;
    inputs_replaced(BATCH_GLOBAL_FLOAT);
    cur.form = BATCH_NONE;
    FEEDCHK(hipMemcpyAsync(f_video, video, rows * FRAME * sizeof(float), hipMemcpyHostToDevice, s));
    FEEDCHK(hipMemcpyAsync(f_audio, audio, rows * T * sizeof(float), hipMemcpyHostToDevice, s));
    FEEDCHK(hipMemcpyAsync(f_labels, labels, rows * 2 * sizeof(float), hipMemcpyHostToDevice, s));
    FEEDCHK(stream_wait(s));
    cur.form = BATCH_GLOBAL_FLOAT, cur.slices = slices, cur.aug = false;
    return L3_OK;
}

// The staging protocol, for single and global batches alike.  There are two sets: `cur` holds the resident batch and is written
// on the engine's stream only (upload), `nxt` is written on the copy stream only (stage); adopt() makes them change places in the
// engine's stream order.  The one rule: a set the copy stream fills must have no reader still queued.  The readers of a set are
// the conversions enqueued while it was `cur` -- for a single batch the one conversion at its adoption, for a resident global
// batch those of every step until it is replaced -- and all of them are in front of the swap that made it `nxt`.  So adopt()
// records ev_adopted on the engine's stream at the swap and every later stage() makes the copy stream wait for it; in the other
// direction adopt() makes the engine's stream wait for ev_staged, recorded behind the copies.  A second stage() before an
// adoption overwrites the first, whatever their forms: the later stage wins.
int BatchFeed::stage_begin(std::string* err) {
    if (!copy_stream) {
        FEEDCHK(hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking));
        FEEDCHK(hipEventCreateWithFlags(&ev_staged, hipEventDisableTiming));
        FEEDCHK(hipEventCreateWithFlags(&ev_adopted, hipEventDisableTiming));
    }
    if (adopted_once) FEEDCHK(hipStreamWaitEvent(copy_stream, ev_adopted, 0));
    return L3_OK;
}

int BatchFeed::stage(BatchForm form, int slices, const uint8_t* video_u8, const int16_t* audio_i16, const int32_t* labels_i32,
                     const AugmentParams* params, const double* u, std::string* err) {
    int rc = stage_begin(err);
    if (rc) return rc;
    if ((rc = send(nxt, form, slices, video_u8, audio_i16, labels_i32, params, u, copy_stream, err))) return rc;
    FEEDCHK(hipEventRecord(ev_staged, copy_stream));
    return L3_OK;
}

// A batch built on the device from sample records.  The set's raw buffers are written by two kernels instead of two copies, on the
// same stream the copies of send() would take, so the staging rule above covers them as it stands: the copy stream has waited for
// ev_adopted before either kernel writes into `nxt`.  What is new is host memory that asynchronous copies read: the tables live in
// the set (RawBatch::host), and a set's tables are rewritten only after the event behind its last fill's copies has passed.
int BatchFeed::plan_sampled(RawBatch& dst, const ::l3_clipbank* bank, const ::l3_sample* records, int n, bool aug, std::string* err) {
    if (n != B) {
        *err = std::to_string(n) + " sample records for a batch of " + std::to_string(B);
        return L3_EINVAL;
    }
    if (T != SAMPLE_T) {
        *err = "sampled batches are rows of " + std::to_string(SAMPLE_T) + " samples, the engine's are " + std::to_string(T);
        return L3_EINVAL;
    }
    int rc = sampled_plan(bank, records, n, aug, &planned, err);
    if (rc) return rc;
    if (dst.tables_pending) {
        FEEDCHK(event_wait(dst.tables_read));
        dst.tables_pending = false;
    }
    std::swap(dst.host, planned);
    return L3_OK;
}

int BatchFeed::fill_sampled(RawBatch& dst, hipStream_t s, std::string* err) {
    const SampledHost& h = dst.host;
    const size_t rows = (size_t)B, n_desc = h.plan.frames.size(), n_sec = h.seconds.size(), n_taps = h.plan.taps.size();
    int rc;
    if ((rc = grow(bufs, &dst.video, &dst.cap_video, rows * FRAME, err))) return rc;
    if ((rc = grow(bufs, &dst.audio, &dst.cap_audio, rows * T, err))) return rc;
    if ((rc = grow(bufs, &dst.labels, &dst.cap_labels, rows * 2, err))) return rc;
    if ((rc = grow(bufs, &dst.tables, &dst.cap_tables, n_desc + n_sec + n_taps, err))) return rc;
    if (h.aug) {
        if ((rc = grow(bufs, &dst.params, &dst.cap_params, rows, err))) return rc;
        if ((rc = grow(bufs, &dst.u, &dst.cap_u, rows, err))) return rc;
        if (!gains && !(gains = bufs.alloc<double>((size_t)B))) {
            *err = "hipMalloc of the batch gains failed";
            return L3_ENOMEM;
        }
    }
    if (!dst.tables_read) FEEDCHK(hipEventCreateWithFlags(&dst.tables_read, hipEventDisableTiming));
    dst.form = BATCH_NONE;      // until everything is enqueued
    int64_t *d_desc = dst.tables, *d_sec = dst.tables + n_desc, *d_taps = d_sec + n_sec;
    dst.tables_pending = true;          // from the first copy on, whatever happens to the later ones
    FEEDCHK(hipMemcpyAsync(d_desc, h.plan.frames.data(), n_desc * sizeof(int64_t), hipMemcpyHostToDevice, s));
    FEEDCHK(hipMemcpyAsync(d_sec, h.seconds.data(), n_sec * sizeof(int64_t), hipMemcpyHostToDevice, s));
    FEEDCHK(hipMemcpyAsync(d_taps, h.plan.taps.data(), n_taps * sizeof(int64_t), hipMemcpyHostToDevice, s));
    if (mark) mark(mark_ctx, "sampled: image_frames", s, 1);
    image_frames(h.pixels, d_desc, d_taps, dst.video, nullptr, B, B, s);
    if (mark) mark(mark_ctx, "sampled: image_frames", s, 0);
    if (mark) mark(mark_ctx, "sampled: audio_seconds", s, 1);
    audio_seconds(h.audio, d_sec, dst.audio, B, T, s);
    if (mark) mark(mark_ctx, "sampled: audio_seconds", s, 0);
    FEEDCHK(hipMemcpyAsync(dst.labels, h.labels.data(), rows * 2 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (h.aug) {
        FEEDCHK(hipMemcpyAsync(dst.params, h.params.data(), rows * sizeof(AugmentParams), hipMemcpyHostToDevice, s));
        FEEDCHK(hipMemcpyAsync(dst.u, h.u.data(), rows * sizeof(double), hipMemcpyHostToDevice, s));
    }
    FEEDCHK(hipEventRecord(dst.tables_read, s));
    FEEDCHK(hipGetLastError());
    dst.form = BATCH_SINGLE, dst.slices = 1, dst.aug = h.aug;
    return L3_OK;
}

int BatchFeed::upload_sampled(const ::l3_clipbank* bank, const ::l3_sample* records, int n, bool aug, hipStream_t s, std::string* err) {
    int rc = plan_sampled(cur, bank, records, n, aug, err);          // a refusal leaves both sets as they were
    if (rc) return rc;
    inputs_replaced(BATCH_SINGLE);
    if ((rc = fill_sampled(cur, s, err))) return rc;
    if ((rc = convert(0, s, err))) return rc;
    FEEDCHK(stream_wait(s));
    return L3_OK;
}

int BatchFeed::stage_sampled(const ::l3_clipbank* bank, const ::l3_sample* records, int n, bool aug, std::string* err) {
    int rc = plan_sampled(nxt, bank, records, n, aug, err);
    if (rc) return rc;
    if ((rc = stage_begin(err))) return rc;
    if ((rc = fill_sampled(nxt, copy_stream, err))) return rc;
    FEEDCHK(hipEventRecord(ev_staged, copy_stream));
    return L3_OK;
}

int BatchFeed::adopt(BatchForm form, hipStream_t s, std::string* err) {
    if (nxt.form != form) return L3_OK;
    FEEDCHK(hipStreamWaitEvent(s, ev_staged, 0));
    std::swap(cur, nxt);
    nxt.form = BATCH_NONE;
    FEEDCHK(hipEventRecord(ev_adopted, s));
    adopted_once = true;
    return form == BATCH_SINGLE ? convert(0, s, err) : L3_OK;
}

// slice r of the resident batch into the float inputs
int BatchFeed::convert(int r, hipStream_t s, std::string* err, bool video, bool audio, bool labels) {
    const size_t pv = (size_t)B * FRAME, pa = (size_t)B * T, pl = (size_t)B * 2;
    if (cur.form == BATCH_GLOBAL_FLOAT) {
        FEEDCHK(hipMemcpyAsync(out_video, f_video + r * pv, pv * sizeof(float), hipMemcpyDeviceToDevice, s));
        FEEDCHK(hipMemcpyAsync(out_audio, f_audio + r * pa, pa * sizeof(float), hipMemcpyDeviceToDevice, s));
        FEEDCHK(hipMemcpyAsync(out_labels, f_labels + r * pl, pl * sizeof(float), hipMemcpyDeviceToDevice, s));
        gains_valid = false;
        return L3_OK;
    }
    if (cur.aug) {      // data/avc/sample.py:146-162,241-281 in the pass that otherwise spends train.py:186,189 on the batch
        augment_video(cur.video + r * pv, B, 224, 224, cur.params + (size_t)r * B, nullptr, out_video, s);
        augment_audio(cur.audio + r * pa, B, T, cur.u + (size_t)r * B, nullptr, out_audio, gains, s);
    } else {
        if (video) preprocess_video(cur.video + r * pv, out_video, (int64_t)pv, s);
        if (audio) preprocess_audio(cur.audio + r * pa, out_audio, (int64_t)pa, s);
    }
    if (labels) labels_onehot(cur.labels + r * pl, out_labels, (int64_t)pl, s);
    gains_valid = cur.aug;
    return L3_OK;
}

void BatchFeed::destroy() {
    if (copy_stream) {
        (void)stream_wait(copy_stream);
        (void)hipStreamDestroy(copy_stream);
        (void)hipEventDestroy(ev_staged);
        (void)hipEventDestroy(ev_adopted);
        copy_stream = nullptr;
    }
    for (RawBatch* b : {&cur, &nxt})
        if (b->tables_read) {
            (void)hipEventDestroy(b->tables_read);
            b->tables_read = nullptr;
        }
    bufs.clear();
}

}  // namespace l3
