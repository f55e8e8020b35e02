/* l3hip.h -- C ABI of libl3hip.so: the MI355X-native L3-Net AVC training path.
 *
 * The reference (marl/l3embedding) has no FFI seam; its boundary is the Python
 * object protocol between l3embedding/train.py + model.py and Keras (SURVEY.md
 * section 8b).  Each entry point below names the reference call it stands in for
 * (paths relative to the reference tree).  The Python mirror of the reference's
 * interface (l3embedding_amd/model.py, train.py) binds these with ctypes; the
 * stub a reference maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions: plain C, host pointers unless the name ends in _dev, float32 data,
 * NHWC activations, HWIO conv kernels, (in,out) dense kernels.  Every function
 * returns 0 on success and a negative L3_E* code on failure; l3_last_error() gives
 * the message.  One engine per process/GPU; calls on one engine are not
 * re-entrant.  Inputs/outputs stay caller-owned; weights are copied in/out.
 */
#ifndef L3HIP_H
#define L3HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define L3_OK 0
#define L3_EINVAL (-1)   /* bad argument (mirrors ValueError: model.py:113-114,175-176) */
#define L3_EHIP (-2)     /* HIP runtime error */
#define L3_ENOMEM (-3)
#define L3_ESTATE (-4)   /* call out of order */
#define L3_ECOMM (-5)    /* RCCL error (or librccl could not be loaded) */

/* MODELS registry keys, model.py:307-313 */
#define L3_MODEL_CNN_L3_ORIG 0
#define L3_MODEL_TINY_L3 1
#define L3_MODEL_CNN_L3_KAPREDBINPUTBN 2
#define L3_MODEL_CNN_L3_MELSPEC1 3
#define L3_MODEL_CNN_L3_MELSPEC2 4

typedef struct l3_engine l3_engine;

#define L3_DTYPE_F32 0
#define L3_DTYPE_BF16 1

/* fp32 convolution algorithm of the 14 3x3 'same' layers (forward and data gradient).  Both are plain fp32 arithmetic on
 * the fp32 matrix cores; they differ in rounding error and speed:
 *   L3_FP32_CONV_F4X4 (default)  Winograd F(4x4,3x3): layer outputs within ~8e-6 of the output range of a direct fp32
 *                                convolution (float64 oracle; tests/test_layer_parity_gpu.py bound 3e-5); fastest
 *   L3_FP32_CONV_F2X2            Winograd F(2x2,3x3): within ~1e-6 (bound 3e-6), the step ~17 % slower -- for a caller
 *                                that wants the tightest parity with the reference's direct convolution */
#define L3_FP32_CONV_F4X4 0
#define L3_FP32_CONV_F2X2 1
/* Value 2 (L3_FP32_CONV_F2X2_BF16X6: F(2x2,3x3) on exact bfloat16 triples, bf16 matrix cores) is a measured experiment that is
 * slower than the default at the accuracy class of L3_FP32_CONV_F2X2 (profiles/r05_bx6_ablations.txt).  It is not part of the
 * product library: l3_create accepts it only from a library built with L3_BUILD_EXPERIMENTS=1 (l3_build_experiments() == 1). */
#define L3_FP32_CONV_F2X2_BF16X6 2

/* BatchNormalization moving statistics of a data-parallel step (l3_step_dp, world > 1).  The reference's multi_gpu_model CALLS
 * the one template model once per replica (training_utils.py:155 `outputs = model(inputs)`), so every BatchNormalization
 * (vision_model.py:124-187, audio_model.py:370-433) adds one moving-average update PER REPLICA to ONE shared variable.
 *   L3_DP_MOVING_REPLICAS (default)  every rank gathers all ranks' batch means / variances (one small all-gather per step on
 *                                    the communicator stream) and applies the `world` updates in replica order 0..world-1 to
 *                                    its moving variables: identical on every rank, momentum 0.99^world per step, every
 *                                    shard's statistics in the checkpoint whichever rank writes it
 *   L3_DP_MOVING_RANK_LOCAL          one update per step from the rank's own shard (rounds 1-5); ranks then validate with
 *                                    different statistics */
#define L3_DP_MOVING_REPLICAS 0
#define L3_DP_MOVING_RANK_LOCAL 1

/* The form of the audio front-end, fixed at l3_create.
 *   L3_FRONTEND_KAPRE (default)  the kapre layer the models were trained with (audio_model.py:39-43,149-151,257-260,367-369)
 *   L3_FRONTEND_MINISPEC         the spectrogram of the deployed pipeline, notebooks/pimodel.ipynb cell 12: every frame centred
 *                                (n_dft / 2 zeros on both sides, 199 frames for all three models), the mel filterbank applied to
 *                                the MAGNITUDE, dB = 10 log10(max(v^2, 1e-10)) with v = mel(|X|) or |X|, minus the sample's
 *                                maximum, clipped at -80.  Only for cnn_L3_kapredbinputbn, cnn_L3_melspec1 and cnn_L3_melspec2,
 *                                the models notebooks/extract_*_models_from_avc_models.ipynb convert; refused with
 *                                db_max_scope = 1.  Such an engine is for inference: every call that computes gradients or
 *                                updates weights returns L3_EINVAL. */
#define L3_FRONTEND_KAPRE 0
#define L3_FRONTEND_MINISPEC 1

typedef struct l3_config {
    int32_t struct_size;     /* sizeof(l3_config) */
    int32_t model_type;      /* L3_MODEL_* */
    int32_t batch;           /* per-device batch (fixed for the engine's life) */
    int32_t global_batch;    /* batch over all ranks (0 => batch); loss gradient is
                                scaled 1/global_batch so a SUM all-reduce gives the
                                gradient of the mean loss over the concatenated batch
                                (training_utils.py:165-170 + keras mean loss) */
    int32_t device;          /* HIP device ordinal */
    int32_t db_max_scope;    /* 0: per-sample max (kapre 0.1.4), 1: batch max (0.1.3.1) */
    int32_t bn_zero_debias;  /* 1: keras-2.0.9/TF-1.4 assign_moving_average(zero_debias=True) */
    int32_t dtype;           /* L3_DTYPE_F32 (0): fp32 everywhere (reference: Input(dtype='float32'),
                                audio_model.py:363, vision_model.py:123).  L3_DTYPE_BF16 (1): mixed precision
                                of BASELINE configs[4] -- the 14 3x3 'same' convolutions with Cin, Cout % 64 == 0
                                round both operands to bfloat16 and accumulate in fp32 (forward, data gradient,
                                weight gradient); every tower convolution that feeds a BatchNormalization STORES
                                its output as bfloat16 (and the data gradient it hands to the preceding BatchNorm);
                                the BatchNorm arithmetic on those tensors, weights, BN parameters and statistics,
                                the two embedding-layer outputs, the head, the loss and Adam stay fp32
                                (oracle.mixed_precision('bf16') restates the three rules) */
    void *stream;            /* hipStream_t to launch on, NULL => engine-owned stream */
    int32_t fp32_conv;       /* L3_FP32_CONV_*: see above (ignored by the bf16 engine's 14 layers) */
    int32_t dp_moving;       /* L3_DP_MOVING_*: see above (was reserved0; 0 keeps the struct compatible) */
    int32_t frontend;        /* L3_FRONTEND_*: see above.  A caller whose struct_size ends before this field gets
                                L3_FRONTEND_KAPRE */
} l3_config;

/* MODELS[model_type](num_gpus=...) -- model.py:184-195,307-313; train.py:267.
 * Weights are initialised like the reference (he_normal kernels, zero biases, BN
 * gamma=1 beta=0 mean=0 var=1; kapre DFT / mel constants) from `seed`.
 * (Host waits of the library -- l3_sync, the result readers -- sleep between hipStreamQuery calls instead of spinning in
 * hipStreamSynchronize: one host core per rank less; L3_HOST_WAIT=spin restores the spin.) */
int l3_create(const l3_config *cfg, uint64_t seed, l3_engine **out);
void l3_destroy(l3_engine *e);
const char *l3_last_error(const l3_engine *e);   /* e may be NULL (create errors) */
int l3_model_type_from_name(const char *name);   /* <0 if not in MODELS (model.py:113-114) */
int l3_build_experiments(void);                  /* 1: built with L3_BUILD_EXPERIMENTS=1 (measured-and-rejected kernel variants compiled in) */
/* AMD GPUs visible to this process (0 without one) -- _get_available_devices(), training_utils.py:12-18,
 * behind multi_gpu_model's "we expect the following devices to be available" check (:107-119). */
int l3_device_count(void);

/* model.get_weights()/set_weights()/load_weights() -- model.py:77,119.
 * Parameters are enumerated in keras get_weights() order (layer by layer; kapre
 * tensors first in the audio tower); names look like
 * "vision_model/conv2d_1/kernel", "audio_model/batch_normalization_10/moving_mean". */
int l3_param_count(const l3_engine *e);
int l3_param_info(const l3_engine *e, int index, char *name, int name_cap,
                  int32_t *ndim, int64_t shape[4], int32_t *trainable, int64_t *numel);
int l3_set_param(l3_engine *e, const char *name, const float *src, int64_t numel);
int l3_get_param(l3_engine *e, const char *name, float *dst, int64_t numel);
int l3_get_grad(l3_engine *e, const char *name, float *dst, int64_t numel);
/* Adam moments + iteration counter reset (keras save_weights does not store the
 * optimizer: a resumed run restarts them -- train.py:263-265,316-355). */
int l3_reset_optimizer(l3_engine *e);
/* A Keras model keeps ONE set of variables whatever batch size is fed (fit_generator alternates
 * train_batch_size / validation_batch_size steps on the same model, train.py:408-414).  An engine's
 * activation buffers are sized for one batch, so the host keeps one engine per fed batch size and moves
 * the model state between them, device to device: every parameter (trainable and not), the Adam
 * moments and step count, and the BatchNorm zero-debias accumulators + update count. */
int l3_copy_state(l3_engine *dst, l3_engine *src);
int l3_optimizer_steps(const l3_engine *e, int64_t *adam_t, int64_t *bn_steps);

/* model.predict / test-mode forward (BN moving statistics) or training-mode
 * forward (batch statistics).  video (B,224,224,3) in [-1,1], audio (B,1,48000);
 * probs/logits (B,2), either may be NULL.  train.py:382-384 feed order. */
int l3_forward(l3_engine *e, const float *video, const float *audio, int training,
               float *probs, float *logits);

/* One fit_generator step -- train.py:282-284,408-414: forward(training) ->
 * categorical_crossentropy + L2 -> backward -> Adam(lr) -> BN moving update.
 * labels (B,2) one-hot.  loss includes the L2 penalty like keras' logged loss. */
int l3_train_step(l3_engine *e, const float *video, const float *audio,
                  const float *labels, float lr, float *loss, float *acc);
/* test_on_batch (validation, train.py:408-414 validation_data): inference-mode BN. */
int l3_eval_step(l3_engine *e, const float *video, const float *audio,
                 const float *labels, float *loss, float *acc);

/* Device-resident input path (the measured one: inputs already in HBM).
 * l3_upload_batch copies caller host buffers into the engine's input tensors;
 * l3_upload_batch_raw takes the HDF5 blob dtypes (uint8 frames, int16 PCM, int
 * labels; data/avc/sample.py:371-377) and applies train.py:186,189 on the GPU; a NULL input stays as it was.
 *
 * Every batch in the stored dtypes goes through ONE feed, which keeps two sets of device buffers: the resident batch and the
 * staged one.  A batch is either single (B rows: l3_upload_batch_raw*, l3_stage_batch_raw*; converted into the float inputs once,
 * by the upload or by the step that adopts it) or the global batch of serial replicas (R * B rows: l3_replicas_*; it stays
 * resident and slice r is converted when its turn comes in every l3_step_replicas / l3_eval_replicas).  The engine holds one
 * resident batch: a single raw batch, uploaded or adopted, replaces a resident raw global batch (l3_upload_batch and the float
 * entry points leave it alone).  An explicit upload supersedes a staged batch of its kind (single / global), a resident global
 * batch supersedes a staged single batch when a replicas step begins, and of two batches staged without an adoption in between,
 * single or global, the later one wins. */
int l3_upload_batch(l3_engine *e, const float *video, const float *audio, const float *labels);
int l3_upload_batch_raw(l3_engine *e, const uint8_t *video_u8, const int16_t *audio_i16,
                        const int32_t *labels_i32);
/* Pipelined variant for a training loop: copies the NEXT batch (stored dtypes) into the feed's staged set over the
 * engine's own copy stream and returns; the copy overlaps the step that is still running, and the
 * following l3_step_forward() / l3_tower_step() adopts the staged batch (the sets change places and the scaling
 * kernels run in stream order) before it starts.  Keras' fit_generator keeps batches queued ahead of the device the
 * same way (train.py:408-414, max_queue_size=10). */
int l3_stage_batch_raw(l3_engine *e, const uint8_t *video_u8, const int16_t *audio_i16, const int32_t *labels_i32);
/* Training-set augmentation (02_generate_samples.py --augment; data/avc/sample.py:24-69,117-166,169-283), one record per sample.
 * The draws are the caller's (l3embedding_amd/augment.py draw_params keeps the reference's order of random calls); the library
 * applies them.  start_x is the crop's first ROW and start_y its first COLUMN, the reference's names (sample.py:181-191). */
typedef struct l3_augment_params {
    int32_t start_x, start_y;   /* sample_cropped_frame, sample.py:182: 0 <= start_x <= H - 224, 0 <= start_y <= W - 224 */
    int32_t flip;               /* horiz_flip, sample.py:59-69,244-247 */
    int32_t sat_first;          /* 1: saturation then brightness (sample.py:253-262); 0: brightness first (sample.py:264-273) */
    float saturation;           /* adjust_saturation's factor, sample.py:24-38 */
    float brightness;           /* adjust_brightness's delta on the [0, 1] image, sample.py:41-56 */
} l3_augment_params;
/* l3_upload_batch_raw / l3_stage_batch_raw with the batch augmented in the pass that scales it: the kernels of
 * l3_op_augment_video / l3_op_augment_audio run in place of the plain scaling ones, on the engine's 224 x 224 frames (so
 * start_x = start_y = 0) and 48000-sample rows.  params: B records; u: B draws of random() in [0, 1), the audio gain's
 * (sample.py:156).  Labels are unchanged.  The staged variant sends the records over the copy stream with the batch; staged
 * plain and augmented batches may follow each other in any order.  L3_EINVAL for a NULL pointer or a non-zero crop start. */
int l3_upload_batch_raw_aug(l3_engine *e, const uint8_t *video_u8, const int16_t *audio_i16, const int32_t *labels_i32,
                            const l3_augment_params *params, const double *u);
int l3_stage_batch_raw_aug(l3_engine *e, const uint8_t *video_u8, const int16_t *audio_i16, const int32_t *labels_i32,
                           const l3_augment_params *params, const double *u);
/* The audio gains (sample.py:156,162 'gain') of the batch the engine holds -- the last one uploaded, or staged and adopted by a
 * step -- B doubles.  Waits for the device: for tests and metadata.  L3_ESTATE if that batch was not augmented. */
int l3_batch_gains(l3_engine *e, double *gains);
/* ---- AVC training samples cut on the GPU from decoded clips held there (csrc/avsample.hip) --------------------------------------
 * 02_generate_samples.py's sampler after decoding (data/avc/sample.py:117-166 sample_one_second, :169-193 sample_cropped_frame,
 * :196-283 sample_one_frame, :319-387 generate_sample, :445-448 the mono mix).  The draws are the caller's
 * (l3embedding_amd/avsample.py draw_samples keeps the reference's order of random calls); the library follows the records.
 *
 * A bank is two arenas allocated once by l3_clipbank_create -- pixel_bytes of uint8 frames, audio_samples of int16 mono samples --
 * and filled by bump allocation: nothing ever moves or is freed before l3_clipbank_destroy, so a batch staged from the bank can
 * never read a freed buffer.  Pixels are kept as uploaded (original size); only a sample's 224 x 224 window is ever resized.  What
 * that costs: a 10 s clip of 360 x 640 at 30 fps is 300 * 360 * 640 * 3 = 207 MB of pixels and 0.96 MB of audio.
 * resize: the shorter side frames are resized to before the crop, read_video's rule (sample.py:303-305: scaling = resize /
 * min(W, H), Wo = ceil(scaling * W), Ho = ceil(scaling * H); >= 225), or 0 for frames the caller's decoder has already resized
 * (Ho = H, Wo = W, both >= 225: sample.py:182's randrange(n - 224) raises at 224).  Errors: l3_last_error(NULL). */
typedef struct l3_clipbank l3_clipbank;
int l3_clipbank_create(int device, int64_t pixel_bytes, int64_t audio_samples, int resize, l3_clipbank **bank);
/* One decoded clip: frames (n_frames, h, w, 3) uint8 and audio (n, channels) int16 PCM at 48 kHz, interleaved, 1 <= channels <= 8,
 * n >= 1.  The audio is stored as sample.py:445-448 leaves it, audio.mean(axis=-1).astype('int16'): the channels summed in float64
 * (exact), one IEEE division by `channels`, truncation toward zero; a mono clip is copied as it is.  Waits for the uploads.
 * *clip_id: the clip's number, counted from 0.  L3_ENOMEM, with the sizes in the message, when an arena is full; L3_EINVAL for a
 * NULL pointer, an empty clip, sides outside [1, 8192] or (resize 0) below 225, or a channel count outside [1, 8]. */
int l3_clipbank_add(l3_clipbank *bank, const uint8_t *frames, int n_frames, int h, int w, const int16_t *audio, int64_t n,
                    int channels, int *clip_id);
/* info[0..5] = {n_frames, H, W, Ho, Wo, samples} of a clip; clip == -1: {clips, pixel bytes used, pixel_bytes, samples used,
 * audio_samples, resize} of the bank. */
int l3_clipbank_info(const l3_clipbank *bank, int clip, int64_t *info);
/* A clip's mono samples back on the host (for tests and metadata): `samples` int16. */
int l3_clipbank_audio(l3_clipbank *bank, int clip, int16_t *out);
void l3_clipbank_destroy(l3_clipbank *bank);
/* One sample of generate_sample (sample.py:319-387) after its draws. */
typedef struct l3_sample {
    int32_t video_clip, frame;      /* sample_one_frame's frame of that clip (sample.py:212-234) */
    int32_t audio_clip, audio_start; /* sample_one_second's start, in samples (sample.py:130-136): 0 <= start <= max(len - 48000, 0);
                                     * the row is zero past the clip's end (sample.py:138-144) */
    int32_t label;                  /* int(video_choice != audio_choice), sample.py:363; the labels row is {label, 1 - label} (:376) */
    int32_t reserved;
    double u_gain;                  /* the gain's draw of random() (sample.py:156); read only when augmenting */
    l3_augment_params aug;          /* start_x / start_y: the crop in the Ho x Wo frame (sample.py:181-191), always applied; the
                                     * rest only when augmenting */
} l3_sample;
/* l3_upload_batch_raw[_aug] / l3_stage_batch_raw[_aug] of a batch that the engine builds itself from n = batch records: the
 * records' tables go up on the stream, csrc/frames.hip's resize writes each record's window -- rows [start_x, start_x + 224) x
 * columns [start_y, start_y + 224) of the frame resized to Ho x Wo -- into the feed's uint8 video rows, the seconds kernel writes
 * the int16 audio rows, then the labels follow; with augment != 0 also the l3_augment_params rows, crop offsets zeroed because the
 * crop is done, and the gain draws.  From there on the batch is a raw batch: the same scaling or augmenting conversion, the same
 * staging protocol, l3_batch_gains.  augment is per batch.  Every record is checked before anything is launched: L3_EINVAL, with
 * the sample's number in l3_last_error(e), for a clip id out of range, a frame outside the clip, an audio_start outside
 * [0, max(len - 48000, 0)], a crop outside Ho x Wo or a label other than 0 / 1; also for n != batch or a bank on another device. */
int l3_upload_batch_sampled(l3_engine *e, l3_clipbank *bank, const l3_sample *records, int n, int augment);
int l3_stage_batch_sampled(l3_engine *e, l3_clipbank *bank, const l3_sample *records, int n, int augment);
/* The same kernels alone, in the stored dtypes, for any n >= 1: out_u8 (n, 224, 224, 3), out_i16 (n, 48000) -- what
 * generate_sample leaves as 'video' and 'audio' -- and, when augmenting, gains (n doubles; else it may be NULL).  Augmented rows
 * are l3_op_augment_video / l3_op_augment_audio of the un-augmented ones.  Errors as above, in l3_last_error(NULL). */
int l3_op_sample_batch(l3_clipbank *bank, const l3_sample *records, int n, int augment, uint8_t *out_u8, int16_t *out_i16,
                       double *gains);
/* Staged step on the resident batch, so the host can overlap the gradient
 * all-reduce with backward (buckets complete head -> block4 -> ... -> block1):
 *   l3_step_forward          forward + loss + head backward          (bucket 0 ready)
 *   l3_step_backward_bucket  backward of tower block k = 1..n-1      (bucket k ready)
 *   l3_step_update           Adam on (all-reduced) grads * grad_scale + BN moving update */
int l3_step_forward(l3_engine *e, int training);
/* One sub-network alone on the resident batch (SURVEY 8(d) config "audio tower only"): forward in
 * training mode (batch-norm batch statistics; tower 1 includes the kapre front-end of
 * audio_model.py:367-369), and with backward != 0 the backward pass from the stand-in loss
 * mean(tower output).  tower: 0 = vision_model, 1 = audio_model.  No optimizer step.  Asynchronous:
 * l3_sync() to wait. */
int l3_tower_step(l3_engine *e, int tower, int backward);
int l3_step_bucket_count(const l3_engine *e);
int l3_step_backward_bucket(l3_engine *e, int bucket);
int l3_step_update(l3_engine *e, float lr, float grad_scale);
int l3_step_resident(l3_engine *e, float lr);   /* all of the above, world size 1 */
int l3_step_results(l3_engine *e, float *loss, float *acc, float *probs, float *logits); /* syncs */
/* The same loss / accuracy without stalling the pipeline: _enqueue copies the sums of the step just enqueued to pinned slot 0 or 1
 * behind it (call it right after l3_step_resident), _wait waits for that copy only -- the caller may enqueue the next step in
 * between, which is how fit_generator (train.py:408-414) reads every step's loss while the GPU never waits for the host. */
int l3_step_results_enqueue(l3_engine *e, int slot, int reduce);   /* reduce = 1 (after l3_comm_init): the sums are added up over the
                                                                       ranks first -- loss / acc of the concatenated batch,
                                                                       training_utils.py:165-170; every rank must call it */
int l3_step_results_wait(l3_engine *e, int slot, float *loss, float *acc);

/* Serial replicas -- multi_gpu_model on ONE GPU, training_utils.py:121-170.  The reference cuts the fed batch into `gpus` slices
 * (:121-133), calls the one template model on each (:141-157: each replica normalises with its own batch statistics and adds its
 * own moving-average update to the shared BatchNormalization variables) and adds the replicas' gradients (:165-170).  Nothing makes
 * the replicas run at the same time: an engine created like a data-parallel rank's -- batch = B, the slice; global_batch = R * B --
 * works through the R slices of a resident global batch one after another, so the activations are those of one slice and a step
 * of R * B pairs fits where a step of B pairs fits.  The result is l3_step_dp's over R ranks, bit for bit: the gradient arena holds
 * ((g0 + g1) + g2) + ... in replica order (fp32 addition does not associate: the order is part of the contract), the moving
 * statistics receive the R updates in replica order, Adam runs once.
 *   l3_replicas_upload          float global batch: video (R*B,224,224,3), audio (R*B,1,48000), labels (R*B,2); kept on the device
 *   l3_replicas_upload_raw      the stored dtypes (uint8 frames, int16 PCM, int32 labels); slice r is scaled by the kernels of
 *                               l3_upload_batch_raw from rows [rB, (r+1)B) of the resident raw batch when its turn comes
 *   l3_replicas_upload_raw_aug  ... augmented by the kernels of l3_upload_batch_raw_aug: R*B records and R*B gain draws
 *   l3_replicas_stage_raw(_aug) the NEXT global batch into the same staged set, over the same copy stream, as l3_stage_batch_raw;
 *                               the next l3_step_replicas / l3_eval_replicas adopts it; an explicit l3_replicas_upload* supersedes it
 *   l3_step_replicas            for r = 0 .. R-1: slice r -> training forward, loss, every backward bucket (the towers overlap as in
 *                               l3_step_resident) -> the slice's BatchNorm batch statistics into slot r of the replica buffer, its
 *                               loss / accuracy sums and its gradient arena folded into accumulators; then ONE l3_step_update:
 *                               one Adam step, R moving-average updates (l3_optimizer_steps moves by (1, R)).  One global step
 *                               counts once against the two-steps-in-flight bound of l3_step_forward.
 *   l3_eval_replicas            test_on_batch of the resident global batch (inference-mode BatchNorm), slice by slice
 * After either, l3_step_results / l3_step_results_enqueue(slot, 0) + _wait give the loss (L2 term included) and accuracy of the
 * concatenated batch -- the sums over the slices divided by global_batch; probs / logits are refused (L3_ESTATE: the engine holds
 * one slice's).  Refused, with the numbers in l3_last_error: replicas < 1 (L3_EINVAL); global_batch != replicas * batch
 * (L3_EINVAL); no resident global batch (L3_ESTATE); l3_config.dp_moving == L3_DP_MOVING_RANK_LOCAL (L3_ESTATE: one update per
 * step is not what R replicas apply); an engine that holds a communicator (L3_ESTATE: l3_step_dp is its step).  The feed's
 * buffers are allocated by the first batch that needs them, grow on demand and are freed with the engine. */
int l3_replicas_upload(l3_engine *e, const float *video, const float *audio, const float *labels, int replicas);
int l3_replicas_upload_raw(l3_engine *e, const uint8_t *video_u8, const int16_t *audio_i16, const int32_t *labels_i32, int replicas);
int l3_replicas_upload_raw_aug(l3_engine *e, const uint8_t *video_u8, const int16_t *audio_i16, const int32_t *labels_i32,
                               const l3_augment_params *params, const double *u, int replicas);
int l3_replicas_stage_raw(l3_engine *e, const uint8_t *video_u8, const int16_t *audio_i16, const int32_t *labels_i32, int replicas);
int l3_replicas_stage_raw_aug(l3_engine *e, const uint8_t *video_u8, const int16_t *audio_i16, const int32_t *labels_i32,
                              const l3_augment_params *params, const double *u, int replicas);
int l3_step_replicas(l3_engine *e, float lr);
int l3_eval_replicas(l3_engine *e, float *loss, float *acc);

/* Data parallelism -- multi_gpu_model, training_utils.py:21-170, reached through gpu_wrapper
 * (model.py:184-195).  One process per GPU; every rank owns an engine created with batch = its shard
 * (training_utils.py:121-133) and global_batch = the batch over all ranks.  The reference's implicit
 * gradient AddN over replicas (training_utils.py:141-170) becomes an RCCL SUM all-reduce of the flat
 * gradient arena, issued by the library itself:
 *   l3_comm_unique_id   rank 0 obtains the 128-byte ncclUniqueId and ships it to the other ranks by any
 *                       means the host has (file, TCP store, MPI); no engine needed
 *   l3_comm_init        ncclCommInitRank for this engine's GPU (collective over all ranks); on any failure
 *                       (L3_ECOMM / L3_EHIP / L3_ENOMEM) no communicator is left: it may be called again
 *   l3_step_dp          one training step on the resident batch: as each gradient bucket completes
 *                       (head, vision block 4..1, audio block 4..1) its ncclAllReduce is enqueued on the
 *                       communicator's own HIP stream behind an event, while backward continues on the
 *                       engine's streams; Adam waits for the last bucket.  No host code in the overlap path.
 *   l3_comm_allreduce_host  sum (op 0) / max (op 1) of up to 64 host doubles over the ranks (logged
 *                       loss/accuracy over the concatenated batch, timing, and -- it synchronises -- a barrier)
 * librccl is bound at the first call (dlopen), see csrc/comm.hip. */
#define L3_COMM_ID_BYTES 128
int l3_comm_unique_id(void *id128);
int l3_comm_init(l3_engine *e, const void *id128, int world, int rank);
int l3_comm_destroy(l3_engine *e);
int l3_comm_info(const l3_engine *e, int *world, int *rank, char *library_path, int path_cap);
int l3_comm_version(void);   /* ncclGetVersion() code of the bound librccl (0 before the first l3_comm_* call) */
int l3_comm_allreduce_host(l3_engine *e, double *vals, int n, int op);
int l3_step_dp(l3_engine *e, float lr);
/* Measurement mode of l3_step_dp (never on in a timed region: every step is waited for): hipEvents around each bucket's
 * ncclAllReduce on the communicator's stream, at "backward done" on the engine's stream and behind the last collective.
 * _read returns per-step averages since the last l3_comm_timing(e, 1):
 *   exposed_ms  how long the optimizer step had to wait for the wire after backward was done (0 when the collectives
 *               are hidden behind backward -- what the overlap of training_utils.py:141-170's gradient sum is for)
 *   span_ms     first collective started -> last collective done
 *   bucket_ms   duration of each bucket's all-reduce (l3_step_bucket_count() entries: head, vision 4..1, audio 4..1) */
int l3_comm_timing(l3_engine *e, int on);
int l3_comm_timing_read(l3_engine *e, double *exposed_ms, double *span_ms, double *bucket_ms, int cap, int *steps);

/* Flat fp32 gradient arena (device) and its buckets, for RCCL all-reduce
 * (replaces the implicit gradient AddN of training_utils.py:141-170). */
int l3_grad_arena_dev(l3_engine *e, void **dev_ptr, int64_t *numel);
int l3_bucket_range(const l3_engine *e, int bucket, int64_t *offset, int64_t *numel);
/* BatchNormalization moving statistics under data parallelism for a caller that runs its own collectives (l3_step_dp does this
 * itself; l3_config.dp_moving, training_utils.py:141-157): after l3_step_forward(e, 1), l3_bn_stats_pack_dev packs this rank's
 * batch means / variances (`numel` floats, engine stream) -> the caller all-gathers them into the buffer
 * l3_bn_stats_replicas_dev returns (world x numel floats, rank-major) -> the next l3_step_update applies the `world` replica
 * updates in rank order instead of the rank's own single one.  l3_bn_stats_replicas_dev refuses (L3_ESTATE, nothing armed) unless a
 * training forward is current and l3_bn_stats_pack_dev ran behind it. */
int l3_bn_stats_pack_dev(l3_engine *e, void **send_dev, int64_t *numel);
int l3_bn_stats_replicas_dev(l3_engine *e, int world, void **gathered_dev);

/* load_embedding(...).predict -- model.py:131-181; audio_model.py:445-487;
 * vision_model.py:198-218: MaxPooling2D(pool, padding='same') on the conv output
 * of '<audio|vision>_embedding_layer' (before its BN/ReLU), inference-mode BN,
 * Flatten.  n may exceed the engine batch (processed in chunks).  out (n, D). */
int l3_embed_audio(l3_engine *e, const float *audio, int64_t n, int pool_h, int pool_w, float *out);
int l3_embed_vision(l3_engine *e, const float *video, int64_t n, int pool_h, int pool_w, float *out);
int64_t l3_embed_dim(const l3_engine *e, int vision, int pool_h, int pool_w);
/* get_l3_frames_uniform -- data/usc/features.py:256-306: one audio embedding per 1-second frame of whole clips.
 * samples: n_samples floats, one or more clips back to back.  table: n_frames rows of {start, lo, hi} (int64):
 * frames[f] = samples[start_f .. start_f + 48000), zero outside [lo_f, hi_f) -- every frame padded on its own, as the
 * front-end pads it in training.  The framing rule (reference padding and librosa.util.frame) is the caller's:
 * l3embedding_amd/features.py frame_table.  The samples and the table go to the device once; per engine batch the frames are
 * gathered there (clips.hip) and run through the path of l3_embed_audio; one device-to-host copy of out (n_frames, D) and
 * one host wait per call (up to 256 MiB of output).  L3_EINVAL (message in l3_last_error) for a NULL pointer, a row with
 * lo < 0, lo > hi or hi > n_samples, a bad pooling size, or a model without an audio embedding layer (tiny_L3). */
int l3_embed_audio_frames(l3_engine *e, const float *samples, int64_t n_samples, const int64_t *table,
                          int64_t n_frames, int pool_h, int pool_w, float *out);
/* load_audio's resampling + get_l3_frames_uniform -- data/usc/features.py:18-28 (resampy.resample(data, sr_orig, sr), filter
 * 'kaiser_best') and :256-306: l3_embed_audio_frames on samples the device produces from native-rate clips.
 * native: n_native floats, the clips at their own rates back to back, uploaded once.  clips: n_clips rows of 6 int64
 * {x_off, L, sr_orig, t0, n_out, y_off}: outputs [t0, t0 + n_out) of the 48 kHz version of the L samples at native[x_off ..)
 * go to samples[y_off ..) of a device buffer of n_samples floats, which `table` (n_frames x {start, lo, hi}, as above) frames.
 * One launch of the resample kernel (csrc/resample.hip) covers every row, mixed rates included; a row with sr_orig == 48000
 * is copied, not filtered (the reference skips resampy then).  The engine keeps the filter tables between calls and uploads
 * them again only for a new window scale or another half_window.  Output t of a clip sits at the exact time t * sr_orig / 48000
 * (resampy accumulates the time in an f64 register: DESIGN.md section 8).  half_window: the filter's n_window-entry half window
 * (resampy's interp_win, e.g. l3embedding_amd/resample.py kaiser_best), num_table entries per zero crossing; the library scales
 * it by the ratio when downsampling and takes its differences, as resampy does.  Samples no row writes are zero.
 * L3_EINVAL (message in l3_last_error) for a NULL pointer, a rate <= 0 or above 2^24, (L + 1) * max(rate) >= 2^62, a
 * native range outside the upload, an output range past int(L * 48000 / sr_orig) (or an output length < 1, resampy's
 * ValueError), a destination outside the buffer, a bad frame table, a bad pooling size, or a model without an audio
 * embedding layer. */
int l3_embed_audio_clips_resampled(l3_engine *e, const float *native, int64_t n_native, const int64_t *clips,
                                   int64_t n_clips, const double *half_window, int64_t n_window, int num_table,
                                   int64_t n_samples, const int64_t *table, int64_t n_frames, int pool_h, int pool_w,
                                   float *out);
/* Vision embeddings from raw frames of any size -- read_video's resize (data/avc/sample.py:286-316), the 224 x 224 crop
 * (:169-193) and 2 * img_as_float(u8) - 1 (train.py:186) on the device, then the path of l3_embed_vision.
 * pixels: n_bytes of uint8, frames of H x W x 3 (HWC) back to back at any byte offsets.  table: n_frames rows of 7 int64
 * {offset, H, W, Ho, Wo, y0, x0}: rows [y0, y0 + 224) x [x0, x0 + 224) of the frame at pixels[offset ..) resized from H x W to
 * Ho x Wo become one input row; only that window is computed.  The sizes and the crop are the caller's rule:
 * l3embedding_amd/features.py image_table.  The resize is bilinear with half-pixel centres, the tent widened by the scale when
 * shrinking (PIL's and torch's antialiased bilinear), defined as an order of float64 operations (csrc/frames.hip, DESIGN.md
 * section 8n; tests/image_ref.py is its NumPy form), rounded half up to uint8 and scaled as preprocess_video scales: with
 * H == Ho and W == Wo the window is the source bytes.  The pixels and the table's device form (a descriptor per frame, one tap
 * table per distinct axis) go to the device once, in buffers the engine keeps and grows; per engine batch the frame kernel fills
 * the real rows of the video batch and zeroes the rest.  out (n_frames, D); n_frames == 0 is L3_OK.
 * L3_EINVAL (message in l3_last_error, naming the frame) for a NULL pointer, H or W outside [1, 8192], Ho or Wo outside
 * [224, 8192], a crop outside Ho x Wo, offset < 0 or offset + 3 * H * W > n_bytes, a bad pooling size, or a model without a
 * vision embedding layer; nothing is uploaded then. */
int l3_embed_vision_frames(l3_engine *e, const uint8_t *pixels, int64_t n_bytes, const int64_t *table, int64_t n_frames,
                           int pool_h, int pool_w, float *out);

/* Diagnostics / parity taps. */
int l3_get_activation(l3_engine *e, const char *name, float *dst, int64_t numel); /* e.g. "audio_model/frontend", "vision_model/conv2d_1" */
int l3_activation_numel(l3_engine *e, const char *name, int64_t *numel);
int l3_sync(l3_engine *e);
/* Per-kernel-family device time (ms) accumulated with hipEvents on the engine's
 * stream while profiling is enabled; families: 0 conv_fwd, 1 conv_dgrad, 2 conv_wgrad,
 * 3 elementwise/bn/pool, 4 frontend, 5 head+loss, 6 adam. */
int l3_profile_enable(l3_engine *e, int on);
/* The engine runs the audio tower (front-end included) on an internal second stream beside
 * the vision tower, forked from and joined back into the engine's stream by events, so one
 * tower's HBM-bound BatchNorm/pool kernels overlap the other's MFMA-bound convolutions
 * (the two sub-networks are independent until model.py:218's concatenate).  on=0 serialises
 * both towers on the engine's stream -- per-kernel durations are only meaningful that way.
 * Results are identical either way.  Default on (environment L3_TWO_STREAMS=0 disables). */
int l3_set_tower_overlap(l3_engine *e, int on);
int l3_profile_read(l3_engine *e, int family, double *ms, int64_t *launches, double *flops);
/* `flops` above are ALGORITHMIC (direct convolution, 2*M*K*N).  This returns the flops the
 * family's kernels actually issued: the 3x3 forward / data-gradient launches run Winograd
 * F(4x4,3x3) (36 multiplies per 4x4 output tile and channel pair instead of 144: 9/36 of direct, plus tile
 * padding; F(2x2,3x3) with L3_FP32_CONV_F2X2: 16/36), the weight gradient F(3x3,2x2) (16/36). */
int l3_profile_read_executed(l3_engine *e, int family, double *flops);
/* ... and its ALGORITHMIC HBM bytes: the sum, over the family's launches, of every tensor a launch must read once and write
 * once (convolutions: input + output + filter; BatchNorm / pool kernels: the tensors of each pass) -- what the launch durations
 * and the rocprofv3 FETCH_SIZE / WRITE_SIZE counters are compared with (bench.py hbm_tbs, traffic_over_algorithmic). */
int l3_profile_read_bytes(l3_engine *e, int family, double *bytes);

/* Stand-alone operator entry points (host buffers) used by the op-level parity
 * tests; each replaces the TF op a Keras/kapre layer instantiates. */
/* dtype variants of the two conv operators: same arguments plus L3_DTYPE_*; BF16 falls back to the
 * fp32 kernels for geometries the mixed-precision kernels do not take (first layers).
 * L3_OP_BF16_STORED (these two entry points only): the operands are first written to HBM as bfloat16
 * and the stored-operand kernels run -- the path an L3_DTYPE_BF16 engine takes for its mixed-precision
 * layers (same products as L3_DTYPE_BF16, different fp32 summation order). */
#define L3_OP_BF16_STORED 2
/* L3_OP_BF16_STORED_OUT: as above, and the output tensor is stored as bfloat16 too -- y of l3_op_conv2d_fwd_dt (what
 * the engine does for a tower conv that feeds a BatchNormalization) and dx of l3_op_conv2d_bwd_dt (the data gradient
 * a mixed-precision conv hands to the preceding BatchNorm's backward); the stored values are returned widened. */
#define L3_OP_BF16_STORED_OUT 3
int l3_op_conv2d_fwd_dt(int device, int dtype, const float *x, const float *w, const float *b, float *y,
                        int n, int h, int wd, int cin, int cout, int kh, int kw, int same);
int l3_op_conv2d_bwd_dt(int device, int dtype, const float *x, const float *w, const float *dy, float *dx,
                        float *dw, float *db, int n, int h, int wd, int cin, int cout, int kh, int kw, int same);
int l3_op_conv2d_fwd(int device, const float *x, const float *w, const float *b, float *y,
                     int n, int h, int wd, int cin, int cout, int kh, int kw, int same);
int l3_op_conv2d_bwd(int device, const float *x, const float *w, const float *dy,
                     float *dx, float *dw, float *db,
                     int n, int h, int wd, int cin, int cout, int kh, int kw, int same);
/* x_bf16 (these four BatchNorm operators; c a power of two >= 4), a bit mask: bit 0 -- x is first written to HBM as
 * bfloat16 and the kernels that widen it on load run (how an L3_DTYPE_BF16 engine reads the output of a
 * mixed-precision conv); bit 1 (the two backward operators) -- the incoming gradient dy / dp likewise (how it
 * reads the data gradient a mixed-precision conv stored); bit 2 -- the tensor output (y; the pooled p; dx of the two backward
 * operators) is stored in HBM as bfloat16, rounded to nearest even, as such an engine keeps the operands of its mixed-precision
 * convs, and comes back widened; l3_op_bn_relu_fwd then runs the fast kernels for either form of x.  The per-channel outputs
 * (mean, var, dgamma, dbeta, and dbias, the column sum of the UNROUNDED dx) do not depend on bit 2. */
int l3_op_bn_relu_fwd(int device, const float *x, const float *gamma, const float *beta,
                      float *y, float *mean, float *var, int64_t rows, int c, int relu, int x_bf16);
/* beta non-NULL and c a power of two >= 4: the engine's fast kernels (ReLU mask recomputed from
 * x*scale+shift, y unused); beta NULL: the generic kernels (mask from y). */
int l3_op_bn_relu_bwd(int device, const float *x, const float *y, const float *dy,
                      const float *gamma, const float *beta, const float *mean, const float *var,
                      float *dx, float *dgamma, float *dbeta, int64_t rows, int c, int relu, int x_bf16);
/* Conv-BN-ReLU-MaxPool2D((2,2), strides=2) tail as the engine fuses it (c must be a power of
 * two >= 4), batch statistics; backward from the pooled gradient.  relu_mode 1: p = pool(relu(bn(x)))
 * (vision_model.py:130-134 and every other block); relu_mode 2: p = pool(bn(relu(x))), the
 * Activation-before-BatchNormalization order of vision_model.py:137-139. */
int l3_op_bn_relu_pool2_fwd(int device, const float *x, const float *gamma, const float *beta, float *p,
                            float *mean, float *var, int n, int h, int wd, int c, int same, int relu_mode, int x_bf16);
int l3_op_bn_relu_pool2_bwd(int device, const float *x, const float *gamma, const float *beta, const float *dp,
                            float *dx, float *dgamma, float *dbeta, float *dbias, int n, int h, int wd, int c,
                            int same, int relu_mode, int x_bf16);
int l3_op_maxpool_fwd(int device, const float *x, float *y, int n, int h, int wd, int c,
                      int ph, int pw, int sh, int sw, int same);
int l3_op_maxpool_bwd(int device, const float *x, const float *dy, float *dx, int n, int h,
                      int wd, int c, int ph, int pw, int sh, int sw, int same);
int l3_op_frontend(int device, int model_type, const float *audio, int n, int db_max_scope, float *out);
/* l3_op_frontend with the front-end form (L3_FRONTEND_*; per-sample maximum): L3_FRONTEND_MINISPEC is the spectrogram of
 * notebooks/pimodel.ipynb cell 12, out (n, F, 199). */
int l3_op_frontend_form(int device, int model_type, int frontend, const float *audio, int n, float *out);
/* The front-end's kernels one by one (csrc/frontend.hip; tests/frontend_ref.py).  Every output buffer is NaN before the launch and
 * has a guard behind it that must come back untouched (L3_EINVAL otherwise); shapes the kernels cannot index are L3_EINVAL.
 *
 * l3_frontend_cfg (host only): the geometry the engine derives for t samples, 'same' (TensorFlow) or 'valid' framing:
 * cfg[L3_FRONTEND_CFG_FIELDS] = n_frames, pad_left, n_freq, ncols_pad, ke, ko, nc, N1, N2.
 * l3_frontend_tables (host only), n_dft = 2048 = 32 x 64: the periodic Hann window win (2048), the factored DFT's b1 (32, 64),
 * b2 (128, 64) and twiddles tw (64, 32, 2), and -- n_mels > 0 -- the filterbank freq2mel (1025, n_mels; NULL: the stock HTK bank at
 * 48 kHz) packed as bands: filter q = melw[mel_off[q] .. + mel_len[q]) on the bins from mel_start[q], first to last nonzero weight.
 * *n_melw = the number of packed weights; more than melw_cap is L3_EINVAL.  All exactly as an engine uploads them. */
#define L3_FRONTEND_CFG_FIELDS 9
int l3_frontend_cfg(int t, int n_dft, int n_hop, int same, int n_mels, int32_t *cfg);
int l3_frontend_tables(const float *freq2mel, int n_mels, float *win, float *b1, float *b2, float *tw, int32_t *mel_start,
                       int32_t *mel_len, int32_t *mel_off, float *melw, int64_t melw_cap, int64_t *n_melw);
/* frame_audio, frame_audio_folded and (a1 != NULL, n_dft = 2048) dft_pack_frames on audio (b, t), frame f of a sample = its samples
 * f n_hop - pad_left ..., zeros outside: frames (b n_frames, n_dft), fe (b n_frames, ke), fo (b n_frames, ko), a1 (b n_frames, 64, 32). */
int l3_op_frontend_frames(int device, const float *audio, int b, int t, int n_dft, int n_hop, int pad_left, int n_frames,
                          float *frames, float *fe, float *fo, float *a1);
/* dft_twiddle on y (frames, 64, [re k1 (32) | im k1 (32)]): a2 (frames, 32, [re n2 (64) | im n2 (64)]) and nyq (frames). */
int l3_op_dft_twiddle(int device, const float *y, int frames, float *a2, float *nyq);
/* spec_to_features on a caller's transform of b n_frames rows.  L3_SPEC_UNFOLDED: spec (rows, ncols_pad) = [re | im | pad];
 * L3_SPEC_FOLDED: (2 rows, nc), the re rows then the im rows; L3_SPEC_FACTORED (n_dft = 2048): (rows, 32, [re k2 (32) | im k2 (32)]),
 * bin k1 + 32 k2, and nyq (rows).  n_mels = 0: no mel projection.  flags: bit 0 sqrt_out, bit 1 db, bit 2 loglambda.
 * out (b, n_mels or n_freq, n_frames), before db_normalize. */
#define L3_SPEC_UNFOLDED 0
#define L3_SPEC_FOLDED 1
#define L3_SPEC_FACTORED 2
int l3_op_spec_to_features(int device, int layout, const float *spec, const float *nyq, int b, int n_frames, int n_dft, int n_mels,
                           const float *freq2mel, int flags, float *out);
/* dft_fused (n_dft = 2048) on audio (b, t) with the library's own tables: out (b, n_mels, n_frames), before db_normalize. */
int l3_op_dft_fused(int device, const float *audio, int b, int t, int n_hop, int pad_left, int n_frames, int n_mels,
                    const float *freq2mel, int flags, float *out);
/* db_normalize in place on x (b, per_sample): x - max (of the sample, or batch_scope = 1 of the batch), clamped at -80. */
int l3_op_db_normalize(int device, float *x, int b, int64_t per_sample, int batch_scope);
/* The frame gather of l3_embed_audio_frames on its own: frames (n_frames, 48000) from samples + table as above (parity tests). */
int l3_op_gather_frames(int device, const float *samples, int64_t n_samples, const int64_t *table,
                        int64_t n_frames, float *frames);
/* The frame kernel of l3_embed_vision_frames on its own: from pixels + table as there, out_u8 (n_frames, 224, 224, 3) the resized
 * and cropped uint8 frames and out_f32 the same scaled to [-1, 1], the network's input rows.  Either output may be NULL. */
int l3_op_image_frames(int device, const uint8_t *pixels, int64_t n_bytes, const int64_t *table, int64_t n_frames,
                       uint8_t *out_u8, float *out_f32);
/* resampy.resample(x, sr_orig, sr_new, filter=...)[t0 : t0 + n_out] -- data/usc/features.py:25-26 -- for one clip of n_in
 * samples, on the device (csrc/resample.hip, exact output times as above).  Always filters, equal rates included, as resampy
 * does.  L3_EINVAL for rates <= 0, int(n_in * sr_new / sr_orig) < 1, or a range past that length. */
int l3_op_resample(int device, const float *x, int64_t n_in, int64_t sr_orig, int64_t sr_new, const double *half_window,
                   int64_t n_window, int num_table, int64_t t0, int64_t n_out, float *y);
/* The resample launch of l3_embed_audio_clips_resampled on its own: clip rows as there, any sr_new, into y (n_samples floats,
 * zero where no row writes); copy_equal != 0 copies rows with sr_orig == sr_new. */
int l3_op_resample_clips(int device, const float *x, int64_t n_in, const int64_t *clips, int64_t n_clips, int64_t sr_new,
                         const double *half_window, int64_t n_window, int num_table, int64_t n_samples, int copy_equal,
                         float *y);
/* keras BatchNormalization batch moments (vision_model.py:124-187, audio_model.py:370-433) from the partial sums the
 * convolution epilogues leave: nblk rows of [sum, sum of squares][c] about pivot[c] over `rows` elements per channel.
 * Runs the engine's second reduction stage on a buffer of exactly nblk rows; L3_EINVAL if it wrote past them. */
int l3_op_bn_stats_from_partials(int device, const float *part, int nblk, int c, const float *pivot, int64_t rows,
                                 float eps, float *mean, float *var);
/* What a convolution's epilogue leaves for the BatchNormalization behind it (vision_model.py:124-187, audio_model.py:370-433), on
 * its own: the convolution of l3_op_conv2d_fwd_dt (same dtype values, same kernel choice) with the statistics on.  stat_mode 1:
 * moments of y, 2: of relu(y) (the Activation-before-BatchNormalization order).  part (nblk, 2, cout): per-block [sum, sum of
 * squares] about the pivot b[c] (relu(b[c]) in mode 2), bf16-stored output: of the ROUNDED values; mean, var: the engine's second
 * stage over them.  y comes back widened when stored as bfloat16.  *nblk is the engine's block count for the layer; with part
 * NULL the call only reports it (no device work).  The kernel writes into a buffer of exactly *nblk blocks preset to NaN with a
 * guard behind it: L3_EINVAL (message in l3_last_error(NULL)) if a block stayed unwritten or the guard changed, and for a layer
 * whose kernel leaves no statistics (direct implicit GEMM, bf16 operands cast at fetch). */
int l3_op_conv2d_fwd_stats(int device, int dtype, const float *x, const float *w, const float *b, float *y, float *part, int *nblk,
                           float *mean, float *var, int n, int h, int wd, int cin, int cout, int kh, int kw, int same,
                           int stat_mode);
/* The data gradient of a convolution with the backward reduction of the BatchNormalization(+ReLU) in FRONT of it in the epilogue:
 * n, h, wd, cin, cout describe the forward convolution; dy (n, ho, wo, cout); bn_x (n, h, wd, cin) is that BatchNorm's input (or,
 * for a pooled BatchNorm, the window winners of l3_op_bn_relu_pool2_fwd_xwin) with parameters and batch moments of cin channels
 * over bn_rows rows.  part (nblk, 2, cin): per-block [sum of m dx, sum of m dx x_hat], m the ReLU mask bn_x * scale + shift > 0
 * (relu != 0) or 1; dgamma, dbeta: the second stage over them.  dtype L3_DTYPE_F32 (Winograd kernels) or L3_OP_BF16_STORED_OUT
 * (dy, bn_x, dx bfloat16 in HBM; dx returned widened).  nblk, part NULL, the guarded buffer and L3_EINVAL as above; L3_EINVAL
 * also wherever an engine would not fuse the two. */
int l3_op_conv2d_dgrad_bn_bwd(int device, int dtype, const float *dy, const float *w, const float *bn_x, const float *gamma,
                              const float *beta, const float *mean, const float *var, float *dx, float *part, int *nblk,
                              float *dgamma, float *dbeta, int n, int h, int wd, int cin, int cout, int kh, int kw, int same,
                              int relu, int64_t bn_rows);
/* The backward of a tower's first block -- input BatchNorm (c = 1 or 3 channels) -> 3x3 'same' convolution to 64 filters ->
 * BatchNorm(+ReLU) -- as an engine runs it: bn_stats and bn_xhat_ones (engine.hip:1363, :1371, tower_forward, OP_BN: `p.bwd ==
 * BB_BY_FIRST_CONV`), bn_bwd_fast of the BatchNorm behind the convolution (engine.hip:1447-1453, tower_backward_block, OP_BN), then
 * conv_wgrad over [x^, 1] and first_conv_grads (engine.hip:1459-1480, OP_CONV: `p.aug != FW_NONE`).  form 0: FW_AUG -- bn_bwd_fast writes dY
 * (n, h, wd, 64) and dbias; form 1 / 2: FW_AUG_DEFERRED on fp32 / bfloat16-stored y and dA -- bn_bwd_fast(dx = NULL) leaves
 * coeffs (3, 64) = cA, cB, cC (bn_bwd_fast_coeffs of the one scratch), the weight-gradient kernel forms dY = cA mask(dA) + cB y + cC
 * itself (FirstWgFuse) and first_conv_grads writes dbias.  y (n, h, wd, 64), the convolution's stored output, is an input: the
 * second BatchNorm's statistics are bn_stats_fast's over it.  Every stage's result comes back: mean_in, var_in (c); xaug
 * (n, h, wd, c + 1); mean2 .. dbeta2 (64); coeffs or dY (the other may be NULL); gaug (9, c + 1, 64); dw (3, 3, c, 64); dbias (64);
 * dgamma_in, dbeta_in (c).  Every output and scratch buffer is NaN before the launches; the weight-gradient partials have exactly
 * conv_wgrad_scratch_floats floats and a guard behind them.  L3_EINVAL where conv_first_wgrad would not run (another shape,
 * L3_FIRST_WGRAD=0) or the guard changed. */
int l3_op_first_block_bwd(int device, int form, int relu, const float *x, const float *gamma_in, const float *beta_in, const float *w,
                          const float *y, const float *gamma2, const float *beta2, const float *dA, float *mean_in, float *var_in,
                          float *xaug, float *mean2, float *var2, float *scale2, float *shift2, float *dgamma2, float *dbeta2,
                          float *coeffs, float *dY, float *gaug, float *dw, float *dbias, float *dgamma_in, float *dbeta_in, int n,
                          int h, int wd, int c, int cout);
/* first_conv_grads (engine.hip:1476-1479, the call behind conv_wgrad in tower_backward_block) alone: gaug (taps, c + 1, co), channel c
 * the ones channel, and the filter w (taps, c, co) to dw = gamma G + beta S (taps, c, co), dgamma = sum W G, dbeta = sum W S (c)
 * and, unless NULL, dbias (co) = the ones-channel row of tap taps / 2.  Any taps, c, co. */
int l3_op_first_conv_grads(int device, const float *gaug, const float *w, const float *gamma, const float *beta, float *dw,
                           float *dgamma, float *dbeta, float *dbias, int taps, int c, int co);
/* l3_op_bn_relu_pool2_fwd as a TRAINING forward runs it: also xwin (n, ho, wo, c), the input element (relu_mode 2: the rectified
 * one) that won each window -- what the backward reduction above reads for a pooled BatchNorm.  Widened when x_bf16. */
int l3_op_bn_relu_pool2_fwd_xwin(int device, const float *x, const float *gamma, const float *beta, float *p, float *mean,
                                 float *var, float *xwin, int n, int h, int wd, int c, int same, int relu_mode, int x_bf16);
int l3_op_preprocess(int device, const uint8_t *video_u8, int64_t nv, float *video,
                     const int16_t *audio_i16, int64_t na, float *audio);
/* sample_one_frame(augment=True) after the frame has been chosen (data/avc/sample.py:235-281): crop to 224 x 224 at
 * (start_x, start_y), flip, img_as_float, saturation and brightness in the record's order, img_as_ubyte.  u8: n frames
 * (h, w, 3) with h, w >= 224.  out_u8 (n, 224, 224, 3) is the stored byte; out_f32 is l3_op_preprocess of it, bit for bit;
 * either may be NULL.  float64 arithmetic along skimage's own sequence of operations: the bytes are the original's.
 * L3_EINVAL (message in l3_last_error(NULL)) for a crop outside the frame. */
int l3_op_augment_video(int device, const uint8_t *u8, int n, int h, int w, const l3_augment_params *params,
                        uint8_t *out_u8, float *out_f32);
/* sample_one_second(augment=True) after the second has been cut (data/avc/sample.py:146-162): per row of t samples,
 * gain = 1 + (-0.1 + (min(0.1, 32768 / peak - 1) + 0.1) * u[row]) in float64 (random.uniform's own arithmetic; 0.1 for a silent
 * row), out = (int16) trunc(x * gain) as numpy's astype(int16) converts it -- bit-exact with the original.
 * out_i16 (n, t); out_f32 is l3_op_preprocess of it; either may be NULL.  gains: n doubles, always written. */
int l3_op_augment_audio(int device, const int16_t *i16, int n, int t, const double *u, int16_t *out_i16, float *out_f32,
                        double *gains);

/* ---- Downstream MLP classifier (classifier/train.py:230-391) ------------------------------------------------------------------
 * construct_mlp_model (train.py:230-257): Dense(512, relu) -> Dense(128, relu) -> Dense(C, softmax), kernel_regularizer
 * l2(weight_decay) on each kernel (biases not regularised), compiled with keras-2.0.9 Adam(lr) and categorical_crossentropy; fit as
 * train_mlp does (train.py:260-391).  fp32 throughout on the fp32 matrix cores; deterministic (no float atomics).  A handle owns its
 * device buffers and one stream; calls on one handle are not re-entrant.  Errors: l3_last_error(NULL) gives the message. */
typedef struct l3_mlp l3_mlp;
/* construct_mlp_model(input_shape=(D,), weight_decay, num_classes=C) + Adam state for batches of up to `batch` rows (1..4096),
 * 2 <= C <= 64.  Kernels: keras glorot_uniform (U(-l, l), l = sqrt(6 / (fan_in + fan_out))) from a host generator seeded with
 * `seed`; biases zero; Adam moments zero. */
int l3_mlp_create(int device, int D, int C, int batch, float weight_decay, uint64_t seed, l3_mlp **m);
void l3_mlp_destroy(l3_mlp *m);
/* D*512 + 512 + 512*128 + 128 + 128*C + C */
int64_t l3_mlp_param_count(const l3_mlp *m);
/* m.fit's x / y and validation_data (train.py:357-359): float32 (n, D) row-major features and int32 class indices, copied to the
 * device once (replacing any earlier set).  n_valid may be 0 (no validation: val_* are NaN).  L3_EINVAL: a label outside [0, C),
 * n_train <= 0, more than 2^31 - 1 rows; L3_ENOMEM: more than 64 GiB of features (the documented cap) or a failed allocation. */
int l3_mlp_set_data(l3_mlp *m, const float *X_train, const int32_t *y_train, int64_t n_train,
                    const float *X_valid, const int32_t *y_valid, int64_t n_valid);
/* One epoch of keras fit (shuffle=True): the ceil(n_train / batch) Adam steps over the rows in `perm` order (a permutation of
 * [0, n_train) drawn by the caller; the last batch is partial), Adam steps t0 + 1, t0 + 2, ... (t0 = steps taken before), then
 * the validation rows.  stats_out[4] = loss, acc, val_loss, val_acc as keras logs them: a batch's loss is its mean cross-entropy +
 * weight_decay * sum of the squared kernels before its update, loss / acc are batch-size-weighted means over the epoch, val_loss
 * holds the L2 term of the end-of-epoch weights.  No host synchronisation between the steps. */
int l3_mlp_epoch(l3_mlp *m, const int32_t *perm, float lr, int64_t t0, double *stats_out);
/* m.predict(X) (train.py:372-384): softmax probabilities (n, C) of host rows X (n, D), staged in large row blocks. */
int l3_mlp_predict(l3_mlp *m, const float *X, int64_t n, float *probs_out);
/* get_weights / set_weights in keras order: dense_1 kernel (D,512), bias (512), dense_2 kernel (512,128), bias (128), dense_3
 * kernel (128,C), bias (C), concatenated; n must be l3_mlp_param_count.  set_weights leaves the Adam moments as they are. */
int l3_mlp_get_weights(l3_mlp *m, float *dst, int64_t n);
int l3_mlp_set_weights(l3_mlp *m, const float *src, int64_t n);

/* Operators of the MLP step on their own (host buffers; parity tests).  x has n_x rows of K floats; idx (int32, may be NULL =
 * identity) picks the `rows` rows the product uses, in order -- the gathered rows of the epoch's shuffle.
 * y (rows, N) = act(x[idx] . w + b), w (K, N); relu 0/1.  The first layer's split-K path included. */
int l3_op_mlp_dense_fwd(int device, const float *x, int64_t n_x, const int32_t *idx, int rows, int K, int N, const float *w,
                        const float *b, int relu, float *y);
/* dx (rows, K) = (dy (rows, N) . w^T) * [h > 0]; h (rows, K) NULL: no ReLU mask */
int l3_op_mlp_dense_bwd_x(int device, const float *dy, const float *w, const float *h, int rows, int K, int N, float *dx);
/* dw (K, N) = x[idx]^T . dy, db (N) = column sums of dy: the kernel of l3_op_mlp_wgrad_adam with Adam switched off */
int l3_op_mlp_wgrad(int device, const float *x, int64_t n_x, const int32_t *idx, int rows, int K, int N, const float *dy, float *dw,
                    float *db);
/* The fused step: the same gradient, + 2 * weight_decay * w (kernel only), keras Adam at lr_t (beta 0.9 / 0.999, eps 1e-8) on
 * w, b and their moments (all in/out); w2_out (may be NULL) = sum of the PRE-update w^2.  Bit for bit l3_op_mlp_wgrad followed
 * by l3_op_adam. */
int l3_op_mlp_wgrad_adam(int device, const float *x, int64_t n_x, const int32_t *idx, int rows, int K, int N, const float *dy,
                         float *w, float *b, float *mw, float *vw, float *mb, float *vb, float weight_decay, float lr_t,
                         float *w2_out);
/* softmax + keras categorical_crossentropy of logits z (rows, C <= 64) against class indices; gscale scales the gradient dz (keras
 * mean: 1 / rows).  probs / dz / ce (per-row loss) / correct (per-row 0/1) may each be NULL. */
int l3_op_mlp_softmax_ce(int device, const float *z, const int32_t *labels, int rows, int C, float gscale, float *probs, float *dz,
                         float *ce, float *correct);
/* The engine's Adam kernel (keras 2.0.9 + L2 gradient 2 * l2 * p on the first n_l2 elements) on its own: p, m, v in/out. */
int l3_op_adam(int device, float *p, const float *g, float *m, float *v, int64_t n, int64_t n_l2, float l2x2, float lr_t);
/* The same kernel with every scalar the engine passes: beta_1, beta_2, epsilon and the gradient scale (g * gscale before the L2
 * term; l3_step_update's grad_scale). */
int l3_op_adam_scaled(int device, float *p, const float *g, float *m, float *v, int64_t n, int64_t n_l2, float l2x2, float lr_t,
                      float b1, float b2, float eps, float gscale);
/* The arena fold of l3_step_replicas (the replicas' gradient sum, training_utils.py:165-170) on its own: acc and g are two host
 * arenas of `total` floats (in/out); the fold runs on the elements [off, off + n) of both and leaves every other element as it
 * was.  mode 0: acc = g; 1: acc = acc + g; 2: g = acc + g.  Each sum is one IEEE fp32 addition (NumPy float32 a + b, subnormals
 * kept).  L3_EINVAL for a NULL pointer, a range outside the arenas or another mode. */
int l3_op_arena_fold(int device, float *acc, float *g, int64_t total, int64_t off, int64_t n, int mode);

/* Operators of the engine's head, loss and update on their own (host buffers; parity tests).  Each runs the launcher the engine
 * calls.  y (B, N) = x (B, K) . w (K, N) + b, ReLU when relu != 0.  L3_EINVAL when the launch's dynamic LDS, (K + 8 N) * 4 bytes,
 * is above the 64 KiB a launch may ask for without a function attribute. */
int l3_op_head_dense_fwd(int device, const float *x, const float *w, const float *b, float *y, int B, int K, int N, int relu);
/* dw (K, N) = x^T . dy, db (N) = column sums of dy, dx (B, K) = dy . w^T (no ReLU mask); same limit on N * 4 bytes. */
int l3_op_head_dense_bwd(int device, const float *x, const float *w, const float *dy, float *dw, float *db, float *dx, int B,
                         int K, int N);
/* The engine's two-class softmax + keras categorical_crossentropy: logits (B, 2), labels (B, 2) float32 (one-hot or soft) ->
 * probs (B, 2), dlogits (B, 2) = gscale * d(sum of the losses) / dlogits, stats[0] = sum of the losses, stats[1] = correct rows. */
int l3_op_softmax_ce2(int device, const float *logits, const float *labels, int B, float gscale, float *probs, float *dlogits,
                      float *stats);
/* out[i] = sum of the squares of base[off[i] .. off[i] + n[i]) (base holds n_base floats).  multi 1: the one-call form for up to
 * 24 ranges; multi 0: one single-range call per range, the engine's fallback above 24 regularised tensors. */
int l3_op_sumsq(int device, const float *base, int64_t n_base, const int64_t *off, const int64_t *n, int count, int multi,
                float *out);
/* One launch of the moving-average update of every BatchNormalization statistic over a table of `entries` vectors of c[i]
 * channels.  moving, biased (in/out) and batch hold entry i at slot_off[i] (slot_off[i + 1] - slot_off[i] >= c[i]; n_slots floats in
 * all); the table's packed offsets are the running sum of c, as the engine builds them.  gathered NULL: one update from batch.
 * Else `replicas` updates in order, replica r's statistic i at gathered[r * stride + packed offset of i] (n_gathered floats).
 * `step` = updates applied once the call is done.  packed (in/out, n_packed floats >= sum of c) receives bn_moving_pack's output
 * of the same table. */
int l3_op_bn_moving_update(int device, int entries, const int32_t *c, const int64_t *slot_off, int64_t n_slots, float *moving,
                           float *biased, const float *batch, const float *gathered, int64_t n_gathered, int replicas,
                           int64_t stride, float momentum, int zero_debias, int64_t step, float *packed, int64_t n_packed);

/* ---- Downstream SVM classifier (classifier/train.py:79-166) ------------------------------------------------------------------
 * train_svm's sklearn.svm.SVC (libsvm's C-SVC) on the GPU: the binary problems of one-vs-one and of probability estimates solved
 * together by decomposition (working sets of q variables, libsvm's WSS3 inside each), kernel values in fp32 on the fp32 matrix
 * cores, alpha and the gradient in float64.  Deterministic (no float atomics).  The multiclass shell (pairs, probability
 * estimates, votes) is Python (classifier.py).  Errors: l3_last_error(NULL) gives the message. */
#define L3_SVM_LINEAR 0     /* u.v                                  (libsvm kernel_type order) */
#define L3_SVM_POLY 1       /* (gamma u.v + coef0)^degree */
#define L3_SVM_RBF 2        /* exp(-gamma |u - v|^2), |u|^2 + |v|^2 - 2 u.v clamped at 0 */
#define L3_SVM_SIGMOID 3    /* tanh(gamma u.v + coef0) */
#define L3_SVM_DEFAULT_WS 64          /* working-set size q when l3_svm_fit is given 0 */
#define L3_SVM_LOCAL_REL 0.1          /* a local solve stops at max(tol, 0.1 x its first gap) */
typedef struct l3_svm_kernel {
    int32_t kind, degree;
    double gamma, coef0;
} l3_svm_kernel;
typedef struct l3_svm l3_svm;
int l3_svm_create(int device, l3_svm **m);
void l3_svm_destroy(l3_svm *m);
/* The training matrix X (n, D) float32, copied to the device once and kept for every later fit (the grid search over C of
 * train_param_search refits on the same rows).  The labels travel with the problems, as signs. */
int l3_svm_set_data(l3_svm *m, const float *X, int64_t n, int D);
/* SVC.fit's libsvm svm_train_one, for n_prob binary problems at once (svm.cpp Solver::Solve with WSS3, shrinking off).  Problem p
 * holds entries [prob_off[p], prob_off[p + 1]) of rows (indices into the set_data matrix) and signs (+1 / -1); alpha_out (one per
 * entry), rho_out (libsvm's rho: decision = sum y alpha K - rho), updates_out (local SMO updates), outer_out (outer iterations)
 * and gap_out (the last m(alpha) - M(alpha) seen; < tol when converged) per problem; the last three may be NULL.  max_iter caps
 * the updates per problem (-1: libsvm's max(10^7, 100 l)); q is the working-set size (0: L3_SVM_DEFAULT_WS; even, <= 128).
 * Every launch covers all problems still active; the host waits once per outer iteration. */
int l3_svm_fit(l3_svm *m, const l3_svm_kernel *k, double C, double tol, int64_t max_iter, int n_prob, const int64_t *prob_off,
               const int32_t *rows, const int8_t *signs, int q, double *alpha_out, double *rho_out, int64_t *updates_out,
               int32_t *outer_out, double *gap_out);
/* l3_svm_fit with one box bound per problem, C[p] for problem p (each finite and > 0, else L3_EINVAL): the grid of a parameter
 * search over C goes through one call, every cost's pair problems and cross-validation sub-problems side by side.  A problem's
 * result does not depend on what else is in the batch, with one exception that l3_svm_fit shares: the update cap of max_iter = -1
 * is max(10^7, 100 x the largest problem of the batch).  l3_svm_fit is this call with its scalar broadcast. */
int l3_svm_fit_costs(l3_svm *m, const l3_svm_kernel *k, const double *C, double tol, int64_t max_iter, int n_prob,
                     const int64_t *prob_off, const int32_t *rows, const int8_t *signs, int q, double *alpha_out, double *rho_out,
                     int64_t *updates_out, int32_t *outer_out, double *gap_out);
/* svm_binary_svc_probability's held-out decision values (svm.cpp) for n_jobs binary models in one launch and one host wait.  Job j
 * scores the resident rows held_rows[held_off[j] .. held_off[j + 1]) against the support vectors sv_rows[sv_off[j] .. sv_off[j + 1])
 * (resident rows too): the positives first, the negatives from sv_off[j] + sv_neg[j]; coef holds one coefficient per support vector
 * (y alpha), rho one value per job.  dec_out holds one value per held-out row, in the order of held_rows, bit-equal to
 * l3_svm_decision(x_idx = the job's held-out rows, sv_idx = its support vectors, n_class = 2).  A job may have no support vectors on
 * either side (none at all: dec = -rho) and no held-out rows (it is skipped).  L3_EINVAL for a row outside [0, n), a decreasing
 * offset or an sv_neg outside its job. */
int l3_svm_cv_decision(l3_svm *m, const l3_svm_kernel *k, int n_jobs, const int64_t *held_off, const int32_t *held_rows,
                       const int64_t *sv_off, const int64_t *sv_neg, const int32_t *sv_rows, const double *coef, const double *rho,
                       double *dec_out);
/* svm_predict_values (svm.cpp) of n rows, one fused launch per block of rows: dec_out (n, n_class (n_class - 1) / 2) in libsvm's
 * pair order (0,1), (0,2), ..., positive for the first class of the pair.  Rows come as a host matrix X (n, D) or as x_idx into the
 * set_data matrix; support vectors likewise as SV (n_sv, D) or sv_idx.  Support vectors are grouped by class: class c owns
 * [sv_start[c], sv_start[c + 1]); coef is libsvm's sv_coef (n_class - 1, n_sv), rho one per pair.  2 <= n_class <= 64. */
int l3_svm_decision(l3_svm *m, const l3_svm_kernel *k, const float *X, const int32_t *x_idx, int64_t n, int D, const float *SV,
                    const int32_t *sv_idx, int64_t n_sv, int n_class, const int64_t *sv_start, const double *coef,
                    const double *rho, double *dec_out);
/* Operators on their own (host buffers; parity tests).  kernel rows: out (na, nb) = k(x[a_idx[w]], x[b_idx[t]]), fp32. */
int l3_op_svm_kernel_rows(int device, const l3_svm_kernel *k, const float *x, int64_t n_x, int D, const int32_t *a_idx, int na,
                          const int32_t *b_idx, int nb, float *out);
/* one local SMO solve of the q-variable problem (q <= 128): block K (q, q), signs y, alpha in/out, gradient grad at alpha; stops
 * at a gap below max(eps, local_rel x the first gap), when no pair can move, or after max_updates (<= 0: no cap) updates. */
int l3_op_svm_smo(int device, const float *K, const int8_t *y, int q, double C, double eps, double local_rel, int64_t max_updates,
                  double *alpha, const double *grad, int64_t *updates_out);
/* Scoring a fitted model on the device (csrc/svm_eval.hip): what train_svm reports after the fit (classifier/train.py:134-166:
 * clf.predict, clf.decision_function -> hinge_loss, clf.predict_proba -> the per-file argmax of the mean) without the pair decisions
 * leaving the device.  All of it float64, rounded operation by operation, deterministic.  struct l3_feat: the device matrix of
 * "Fold preprocessing" below. */
/* l3_svm_set_data from rows [lo, hi) of a device matrix (preprocess_split_data's output, features.py:52-150): one copy on the SVM's
 * stream, then the norms; the l3_feat may be destroyed afterwards.  L3_EINVAL for a handle on another device or a bad or empty range. */
int l3_svm_set_data_dev(l3_svm *m, const struct l3_feat *f, int64_t lo, int64_t hi);
/* out (n, D) = rows idx of the resident matrix: SVC.support_vectors_ (sklearn svm/base.py: the rows libsvm copies out of a fit)
 * when the fit came from the device */
int l3_svm_get_rows(l3_svm *m, const int32_t *idx, int64_t n, float *out);
/* The model svm_predict_values / svm_predict_probability read (svm.cpp svm_model), resident until the next set_model: the kernel, the
 * support vectors as a host matrix SV (n_sv, D) or as sv_idx into the resident matrix (their rows are copied, so the model
 * outlives the matrix), sv_start / coef / rho as in l3_svm_decision, and Platt's probA / probB per pair (both or neither; NULL: a
 * model without probability estimates).  Everything is copied once, with the norms.  Argument checks as l3_svm_decision. */
int l3_svm_set_model(l3_svm *m, const l3_svm_kernel *k, const float *SV, const int32_t *sv_idx, int64_t n_sv, int D, int n_class,
                     const int64_t *sv_start, const double *coef, const double *rho, const double *probA, const double *probB);
/* One scoring pass over n rows with the resident model (train.py:134-166).  Rows: exactly one of a host matrix X (n, D), x_idx (n)
 * into the resident matrix, or rows [lo, hi) of a device matrix (n = hi - lo), else L3_EINVAL; a host matrix is staged in
 * l3_svm_decision's row blocks.  labels (n) host class indices in [0, n_class) or NULL; files (n_files, 2) int64 row ranges, each
 * non-empty and inside [0, n), or NULL.  Every output may be NULL (not wanted): pred (n) the one-vs-one vote, ties to the lower class
 * (svm.cpp svm_predict_values); ovr (n, n_class) sklearn 0.19's _ovr_decision_function(dec < 0, -dec), or (n) = -dec for two
 * classes; hinge_sum the sum of sklearn's hinge_loss terms (needs labels; the caller divides by n; chunks of 256 rows added in row
 * order, then the chunk sums in chunk order); proba (n, n_class) svm_predict_probability; file_proba (n_files, n_class) the mean of a
 * file's rows in row order and file_pred its argmax, ties to the lower class (train.py:158-163).  Per row block: decision values,
 * pairs, tail, coupling; the file means after the last block; proba stays on the device unless asked for.  One host wait per call.
 * L3_ESTATE without a model, or when a probability output is asked of a model set without probA / probB. */
int l3_svm_score(l3_svm *m, const float *X, const int32_t *x_idx, const struct l3_feat *feat, int64_t lo, int64_t hi, int64_t n,
                 int D, const int32_t *labels, const int64_t *files, int64_t n_files, int32_t *pred_out, double *ovr_out,
                 double *hinge_sum_out, double *proba_out, double *file_proba_out, int32_t *file_pred_out);
/* The kernels behind l3_svm_score on a host block of pair decisions dec (n, P), no kernel evaluation in front (parity tests).
 * The outputs of l3_svm_score, plus pair_proba (n, P): sigmoid_predict (svm.cpp) of each decision clipped to [1e-7, 1 - 1e-7], and
 * iters (n): the sweeps multiclass_probability (svm.cpp) made for the row, max(100, n_class) at its cap. */
int l3_op_svm_tail(int device, const double *dec, int64_t n, int n_class, const double *probA, const double *probB,
                   const int32_t *labels, const int64_t *files, int64_t n_files, int32_t *pred_out, double *ovr_out,
                   double *hinge_sum_out, double *pair_proba_out, double *proba_out, double *file_proba_out, int32_t *file_pred_out,
                   int32_t *iters_out);
/* svm.cpp sigmoid_train (Platt's A, B by Newton's method with backtracking; Lin, Lin and Weng) for n_jobs pairs in one launch, one
 * workgroup per job: job j fits dec[off[j] .. off[j + 1]) (at least one row, finite) against signs (+1 / -1) there.  Float64
 * throughout; every sum over a job's rows is reduced in a fixed order (strided partials per thread, then a tree), so a job's
 * result does not depend on the batch it is in.  iters_out (may be NULL): the Newton iterations made, i.e. sigmoid_train's `iter`
 * when it stopped (100 at the cap). */
int l3_op_svm_sigmoid_train(int device, int n_jobs, const int64_t *off, const double *dec, const int8_t *signs, double *A_out,
                            double *B_out, int32_t *iters_out);

/* ---- VGGish baseline features (data/usc/features.py:166-240) --------------------------------------------------------------------
 * extract_vggish_embedding / get_vggish_frames_uniform on the GPU, inference only, fp32: load_audio's resampling to 16 kHz and the
 * zero pad to 15600 samples (features.py:170-181), the log-mel front-end (vggish/mel_features.py:71-97,114-218 with the
 * parameters of vggish/vggish_input.py:25-29), the examples (vggish_input.py:64-75), the network (vggish/vggish_slim.py:66-99)
 * and the postprocessor (vggish/vggish_postprocess.py:51-94).  A handle separate from l3_engine: it owns its weights, its
 * activation buffers for `batch` examples and one stream; calls on one handle are not re-entrant.  Deterministic (no float
 * atomics).  Errors: l3_last_error(NULL) gives the message. */
#define L3_VGGISH_DEFAULT_BATCH 128   /* examples per pass when l3_vggish_create is given 0: fc1 reads its 201 MB of weights once
                                         per pass whatever the batch, so a larger pass spreads that read over more examples (where
                                         the read stops bounding fc1 is not measured) */
#define L3_VGGISH_MAX_BATCH 1024
#define L3_VGGISH_CONV_DIRECT 3       /* l3_vggish_set_conv: the implicit-GEMM convolution instead of a Winograd form */
#define L3_VGGISH_RAW 0               /* the embedding after fc2's ReLU (vggish_slim.py:96-99) */
#define L3_VGGISH_PCA 1               /* Postprocessor.postprocess(quantize=False): pca (e - means) clipped to [-2, 2] */
#define L3_VGGISH_QUANTIZED 2         /* quantize=True: (x + 2) * (255 / 4) truncated to an integer in [0, 255], as float32 */
typedef struct l3_vggish l3_vggish;
int l3_vggish_create(int device, int batch, l3_vggish **out);
void l3_vggish_destroy(l3_vggish *v);
int l3_vggish_batch(const l3_vggish *v);
/* fp32 algorithm of the five 3x3 convolutions behind the first: L3_VGGISH_CONV_DIRECT (the default), L3_FP32_CONV_F4X4 or
 * L3_FP32_CONV_F2X2.  The default is the implicit GEMM because it sums the 9 Cin products of an output directly, the arithmetic the
 * parity bounds of this path are stated in; the two Winograd forms issue 4x / 2.25x fewer multiplies at the rounding error the
 * l3_config.fp32_conv comment above gives for them.  Their speed and error on these maps are not measured yet. */
int l3_vggish_set_conv(l3_vggish *v, int fp32_conv);
/* One tensor by its TF variable name (vggish_slim.py:66-99 scopes): vggish/conv1/weights (3,3,1,64) HWIO, vggish/conv1/biases,
 * vggish/conv2/..., vggish/conv3/conv3_1/..., vggish/conv3/conv3_2/..., vggish/conv4/conv4_1/..., vggish/conv4/conv4_2/...,
 * vggish/fc1/fc1_1/weights (12288, 4096) (in, out), vggish/fc1/fc1_2/..., vggish/fc2/weights (4096, 128), vggish/fc2/biases.
 * L3_EINVAL for another name or element count. */
int l3_vggish_set_weight(l3_vggish *v, const char *name, const float *src, int64_t numel);
/* vggish_pca_params.npz: pca_eigen_vectors (128, 128) row major and pca_means (128) */
int l3_vggish_set_pca(l3_vggish *v, const float *pca_matrix, const float *pca_means);
/* extract_vggish_embedding for many files at once.  native / clips / half_window / n_window / num_table / n_samples as in
 * l3_embed_audio_clips_resampled, at 16 kHz: row {x_off, L, sr_orig, t0, n_out, y_off} writes outputs [t0, t0 + n_out) of the 16 kHz
 * version of a clip to a zeroed device buffer of n_samples floats (a row at 16 kHz is copied); y_off carries the left pad of a
 * short clip.  segments: n_segments rows {offset, length} of that buffer, one per (padded) clip; each gets 1 + (length - 400) / 160
 * log-mel rows, computed once, laid back to back in segment order.  example_rows: the first log-mel row of each example (96 rows
 * inside one segment).  The examples run through the network in passes of the handle's batch; out (n_examples, 128) float32 in
 * the form `postprocess` names.  One device-to-host copy and one host wait per call.  L3_ESTATE if a weight (or, for a
 * postprocessed form, the PCA parameters) was never set; L3_EINVAL for a bad row, segment or example. */
int l3_vggish_embed_clips_resampled(l3_vggish *v, const float *native, int64_t n_native, const int64_t *clips, int64_t n_clips,
                                    const double *half_window, int64_t n_window, int num_table, int64_t n_samples,
                                    const int64_t *segments, int64_t n_segments, const int64_t *example_rows, int64_t n_examples,
                                    int postprocess, float *out);
/* Operators of that path on their own (host buffers; parity tests).  Log-mel of segments {offset, length} of x (n floats):
 * out (rows, 64), rows = sum of 1 + (length - 400) / 160 (a segment shorter than 400 gives none). */
int l3_op_vggish_logmel(int device, const float *x, int64_t n, const int64_t *segments, int64_t n_segments, float *out);
/* the first convolution with the example gather, bias, ReLU and 2x2 max pool fused: y (n_examples, 48, 32, 64) */
int l3_op_vggish_conv1(int device, const float *logmel, int64_t n_rows, const int64_t *example_rows, int64_t n_examples,
                       const float *w, const float *b, float *y);
/* the BatchNorm-free convolution tail: y = relu(x + b) (pool 0) or its 2x2 / stride-2 maximum (pool 1: h, wd even); c % 4 == 0 */
int l3_op_vggish_bias_relu(int device, const float *x, const float *b, float *y, int n, int h, int wd, int c, int pool);
/* one of the five wide convolutions as the handle runs it under `fp32_conv` (l3_vggish_set_conv), with that tail: x (n, h, wd, cin),
 * w (3, 3, cin, cout) HWIO, y (n, h, wd, cout) or pooled */
int l3_op_vggish_conv(int device, int fp32_conv, const float *x, const float *w, const float *b, float *y, int n, int h, int wd,
                      int cin, int cout, int pool);
/* the postprocessor: emb (n, 128) -> out (n, 128), quantize 0 / 1 */
int l3_op_vggish_postprocess(int device, const float *emb, int64_t n, const float *pca_matrix, const float *pca_means,
                             int quantize, float *out);

/* ---- Fold preprocessing of the downstream classifier (data/usc/features.py:52-150,243-253) -------------------------------------
 * preprocess_split_data's passes over the (n, D) feature matrix on the GPU: the row selection of remove_data_overlap (:60-73) and of
 * the final shuffle (:143-148), MinMaxScaler's fit and transform (:107-113), compute_stats_features per file (:76-85,243-253) and
 * StandardScaler's fit and transform (:131-141).  A handle separate from l3_engine, l3_mlp and l3_svm: it owns ONE float32 row-major
 * matrix on one device and one stream; every operation replaces that matrix (l3_feat_assemble and l3_feat_split only read their
 * sources and make new handles) and has finished when the call returns; calls on one handle are not re-entrant.  Every D-sized piece of scaler arithmetic (ranges, scales, square roots, the zero rule of sklearn's
 * _handle_zeros) stays with the caller.  Deterministic: no float atomics, and the sums over rows run over fixed chunks of
 * L3_FEAT_CHUNK_ROWS rows whose partial results are added in chunk order, whatever the launch geometry.  NaN inputs are out of
 * contract (the extrema and the median order values as finite floats; -0.0 sorts below +0.0).  Errors: l3_last_error(NULL). */
#define L3_FEAT_CHUNK_ROWS 256        /* rows per partial sum of l3_feat_minmax / l3_feat_moments */
#define L3_FEAT_STATS_LDS_ROWS 64     /* l3_feat_file_stats keeps a file of up to this many rows in LDS; longer files are re-read
                                         from global memory by the same kernel */
typedef struct l3_feat l3_feat;
/* X (n, D) float32 row major, copied to the device once.  1 <= n <= 2^31 - 1, 1 <= D <= 2^21 (any D, not only multiples of 4). */
int l3_feat_create(int device, const float *X, int64_t n, int64_t D, l3_feat **f);
/* A zero-filled (n, D) matrix for rows the device produces (l3_embed_audio_frames_dev); limits and errors as l3_feat_create */
int l3_feat_alloc(int device, int64_t n, int64_t D, l3_feat **f);
void l3_feat_destroy(l3_feat *f);
int l3_feat_shape(const l3_feat *f, int64_t *n, int64_t *D);
/* rows [lo, hi) -> dst ((hi - lo), D) */
int l3_feat_download(l3_feat *f, int64_t lo, int64_t hi, float *dst);
/* A new handle on `device` whose matrix is the rows [lo, hi) of each segment's source, in segment order, copied device to device by
 * ONE kernel launch (the np.vstack of get_fold and get_train_folds, data/usc/folds.py:24-112, for folds that already are on the
 * device).  The sources are only read and stay as they are; a source may occur in any number of segments; a segment with lo == hi
 * contributes nothing.  L3_EINVAL, with a message that names the segment, *out untouched and nothing allocated on the device: a NULL
 * source, a source on another device, a source of another width D than segment 0's, lo / hi outside the source, n_segs < 1, a total
 * of 0 rows or of more than 2^31 - 1.  Rows move as 16-byte accesses wherever a segment's first source and output addresses are both
 * 16-byte aligned (always when D % 4 == 0) and as 4-byte accesses otherwise; the result is the same bits either way.
 * Ordering: the copy runs on the new handle's stream and has finished when the call returns.  It relies on every l3_feat call having
 * finished on its handle's stream when it returns, so the sources hold their final values at entry; each source's stream is
 * synchronised before the launch all the same.  As for every l3_feat call, no other call may run on a source meanwhile. */
typedef struct { const l3_feat *src; int64_t lo, hi; } l3_feat_segment;   /* rows [lo, hi) of src */
int l3_feat_assemble(int device, const l3_feat_segment *segs, int64_t n_segs, l3_feat **out);
/* X <- X[rows]: n_out >= 1 host indices, each in [0, n) (else L3_EINVAL, and the matrix stays as it was).  The caller builds the
 * table -- every chunk_size-th row of each file, or the shuffle's permutation -- and the device moves the rows. */
int l3_feat_gather(l3_feat *f, const int64_t *rows, int64_t n_out);
/* src[rows_a] and src[rows_b] as NumPy's integer indexing gives them, as two NEW handles on src's device, written by ONE kernel launch
 * (train_param_search's cut of the training rows into a search part and a validation part, classifier/train.py:416-423).  src is
 * only read: it keeps its matrix and stays usable.  n_a >= 1; n_b == 0 with rows_b and out_b both NULL is a plain out-of-place take.
 * Host int64 indices in any order, repeats allowed; each output has at most 2^31 - 1 rows.  L3_EINVAL, with *out_a and *out_b
 * untouched and nothing allocated on the device: an index outside [0, n) (the message names the table and the position, as in
 * "rows_b[3] = 9 outside [0, 9)"), n_a < 1, a missing src / rows_a / out_a, or n_b that does not match rows_b and out_b (both NULL
 * for 0, both given otherwise).  The two tables go to the device once, in one buffer; output rows are cut into spans of about 4096
 * floats, one wave per span; a row moves as 16-byte accesses when D % 4 == 0 and as 4-byte accesses otherwise, the same bits
 * either way; no atomics, deterministic.
 * Ordering as l3_feat_assemble's: src's stream is synchronised first, each new handle gets a stream of its own, and both outputs
 * have finished when the call returns. */
int l3_feat_split(const l3_feat *src, const int64_t *rows_a, int64_t n_a, const int64_t *rows_b, int64_t n_b, l3_feat **out_a,
                  l3_feat **out_b);
/* np.min / np.max(X, axis=0), D floats each, exact */
int l3_feat_minmax(l3_feat *f, float *min_out, float *max_out);
/* MinMaxScaler.transform's `X *= scale_; X += min_` on a float32 matrix: x <- fl32(fl32(x * scale[j]) + shift[j]), two float32
 * roundings, never a fused multiply-add */
int l3_feat_affine32(l3_feat *f, const float *scale, const float *shift);
/* X.mean(axis=0, dtype=float64) and X.var(axis=0, dtype=float64) (population variance), D doubles each: two passes, the second over
 * fl64(x) - mean.  NumPy adds the rows one after the other; here each chunk of L3_FEAT_CHUNK_ROWS rows is added in row order and
 * the chunks' sums in chunk order, so the results agree to the rounding error of two float64 sums of n terms, and
 * two calls give the same bits. */
int l3_feat_moments(l3_feat *f, double *mean_out, double *var_out);
/* StandardScaler.transform's in-place `X -= mean_; X /= scale_` on a float32 matrix with float64 operands:
 * x <- fl32(fl64(fl32(fl64(x) - mean[j])) / scale[j]), each step computed in float64 and rounded to float32 */
int l3_feat_standardize(l3_feat *f, const double *mean, const double *scale);
/* framewise_to_stats: X <- (n_files, 7 D), row i = compute_stats_features(X[s_i:e_i]) for file_idxs[i] = {s_i, e_i} (int64 pairs,
 * 0 <= s_i < e_i <= n; 7 D <= 2^21).  Per column, in blocks of D: min, max (exact); median (the middle element, or fl32(fl32(a + b) / 2) of the
 * two middle ones; a bitwise radix select, linear in the file's rows); mean (float32 sum in row order / fl32(F)); var (float32 sum
 * in row order of fl32(x - mean)^2, / fl32(F)); skew and excess kurtosis with scipy's bias=True defaults: float64 mean in row order,
 * d = fl64(x) - mean, m2 m3 m4 the row-order float64 means of d^2 d^3 d^4, skew 0 and kurtosis -3 where
 * m2 <= (1e-15 * mean)^2, else m3 / m2^1.5 and m4 / m2^2 - 3, cast to float32.  The first five blocks are NumPy's bits;
 * the last two differ from NumPy by the roundings of d * d * d against pow(d, 3). */
int l3_feat_file_stats(l3_feat *f, const int64_t *file_idxs, int64_t n_files);

/* l3_mlp_set_data from device matrices: rows [lo, hi) of `train` and rows [vlo, vhi) of `valid` (NULL or vlo == vhi: none; it may be
 * the same handle as `train`) are copied device to device, on the MLP's stream, into the MLP's own resident matrices; the l3_feat
 * handles may be destroyed afterwards.  y / yv: host class indices, one per copied row.  Checks and error codes as l3_mlp_set_data;
 * also L3_EINVAL for a handle on another device or of another width than the MLP's D. */
int l3_mlp_set_data_dev(l3_mlp *m, const l3_feat *train, int64_t lo, int64_t hi, const int32_t *y, const l3_feat *valid, int64_t vlo,
                        int64_t vhi, const int32_t *yv);
/* l3_mlp_predict of rows [lo, hi) of a device matrix, in l3_mlp_predict's row blocks without its staging copy: the same bits */
int l3_mlp_predict_dev(l3_mlp *m, const l3_feat *x, int64_t lo, int64_t hi, float *probs_out);
/* The per-file step of the classifiers' test metrics and of notebooks/pimodel.ipynb on l3_mlp_predict_dev's probabilities, which
 * stay on the device: file_mean (n_files, C) float32 and file_pred (n_files) int32 (either may be NULL) of the rows [s_i, e_i) of x
 * that file_idxs[i] = {s_i, e_i} names (host int64 pairs, 0 <= s_i < e_i <= n, in any order, overlaps allowed).  The arithmetic is
 * NumPy's probs[s:e].mean(axis=0).argmax() on float32 rows: a float32 sum in row order, one float32 division by fl32(e - s), the
 * first maximum.  One wave per file, a lane per class (C <= 64), no atomics: deterministic.  L3_EINVAL for a NULL pointer, a matrix
 * on another device or of another width, C > 64, n_files < 1 or a bad range (the message names the file). */
int l3_mlp_predict_files_dev(l3_mlp *m, const l3_feat *x, const int64_t *file_idxs, int64_t n_files, float *file_mean,
                             int32_t *file_pred);
/* That reduction on its own, on host probabilities probs (n, C) float32 (kernel tests) */
int l3_op_file_mean(int device, const float *probs, int64_t n, int C, const int64_t *file_idxs, int64_t n_files, float *file_mean,
                    int32_t *file_pred);

/* l3_embed_audio_frames and l3_embed_audio_clips_resampled with the pooled rows kept on the device: the same validation, gather or
 * resampling, front-end, tower and pooling, whose kernel writes rows [row0, row0 + n_frames) of dst directly (of the last, partial
 * engine batch only its real rows) -- the same bits as `out` receives, and no other row of dst is touched.  The work runs on the
 * engine's stream and has finished when the call returns, as every call on an l3_feat has; no other call may run on dst meanwhile.
 * L3_EINVAL (message in l3_last_error(e)) with nothing written also for a NULL dst, a dst on another device than the engine, of
 * another width than l3_embed_dim, row0 < 0 or row0 + n_frames > n. */
int l3_embed_audio_frames_dev(l3_engine *e, const float *samples, int64_t n_samples, const int64_t *table, int64_t n_frames,
                              int pool_h, int pool_w, l3_feat *dst, int64_t row0);
int l3_embed_audio_clips_resampled_dev(l3_engine *e, const float *native, int64_t n_native, const int64_t *clips, int64_t n_clips,
                                       const double *half_window, int64_t n_window, int num_table, int64_t n_samples,
                                       const int64_t *table, int64_t n_frames, int pool_h, int pool_w, l3_feat *dst, int64_t row0);
/* l3_embed_vision_frames likewise: rows [row0, row0 + n_frames) of dst, the bits `out` receives; dst is checked before the table */
int l3_embed_vision_frames_dev(l3_engine *e, const uint8_t *pixels, int64_t n_bytes, const int64_t *table, int64_t n_frames,
                               int pool_h, int pool_w, l3_feat *dst, int64_t row0);

/* ---- Spectrograms out, spectrograms in --------------------------------------------------------------------------------
 * The "spec model" of notebooks/extract_spectrogram_models_from_avc_models.ipynb is the audio tower without its front-end layer: it
 * takes a spectrogram (F, frames, 1).  notebooks/pimodel.ipynb cell 12 computes that spectrogram per second and calls the spec
 * model's predict.  Here the front-end's output tensor is the interface: the engine exports it and accepts it.
 * l3_spectrogram_shape: rows = F (n_mels, or n_dft / 2 + 1 for the linear model) and frames = the frame count of the engine's
 * front-end output -- the spec model's input_shape[1:3] (extract_spectrogram_models cell that builds the Input layer). */
int l3_spectrogram_shape(const l3_engine *e, int64_t *rows, int64_t *frames);
/* The spectrogram pimodel.ipynb cell 12 computes for every second (an L3_FRONTEND_MINISPEC engine), or the one the model saw in
 * training (an L3_FRONTEND_KAPRE engine): samples, table and their validation as l3_embed_audio_frames; every engine batch is
 * gathered on the device and run through the front-end, and the front-end tensor of its real rows goes to
 * out (n_frames, F, frames) float32.  n_frames == 0 is L3_OK. */
int l3_audio_spectrograms(l3_engine *e, const float *samples, int64_t n_samples, const int64_t *table, int64_t n_frames, float *out);
/* The spec model's predict (pimodel.ipynb cell 12, `model.predict(spectrogram)`): spec (n, F, frames) float32 host rows go straight
 * into the front-end's output tensor (the rows behind a partial last batch zeroed), the front-end does not run, and the tower and
 * the pooling run as in l3_embed_audio: out (n, D).  Fed with what l3_audio_spectrograms of the same engine returned, the result
 * equals l3_embed_audio_frames bit for bit.  Both dtypes: the front-end's output is float32 in the bf16 engine too.
 * _dev: rows [row0, row0 + n) of dst, with the conventions and checks of l3_embed_audio_frames_dev.  Argument errors are reported
 * before anything is uploaded. */
int l3_embed_audio_spec(l3_engine *e, const float *spec, int64_t n, int pool_h, int pool_w, float *out);
int l3_embed_audio_spec_dev(l3_engine *e, const float *spec, int64_t n, int pool_h, int pool_w, l3_feat *dst, int64_t row0);

/* ---- Cross-modal retrieval: every (frame, second) pair through the AVC head (csrc/pairs.hip) ---------------------------
 * A tower's flattened output -- its half of the concatenate input (model.py:25), nv or na wide: l3_tower_dim -- from ONE tower run in
 * inference mode, as l3_embed_* run it; the other tower does not run.  tower: 0 = vision_model, rows (n, 224, 224, 3); 1 =
 * audio_model, rows (n, 1, 48000).  n may exceed the engine batch.
 *   l3_tower_features              host rows -> out (n, width) on the host
 *   l3_tower_features_dev          ... -> rows [row0, row0 + n) of dst (width columns, on the engine's device); only the real rows of
 *                                  the last engine batch are written
 *   l3_tower_features_sampled_dev  n >= 1 l3_sample records of a bank, not augmented: each engine batch is built by the feed of
 *                                  l3_upload_batch_sampled (window resize, seconds kernel, conversion to float; the last batch is filled
 *                                  up with copies of its last record) and REPLACES the engine's resident batch; then both towers run
 *                                  solo.  vis / aud: the destinations of the frames' and the seconds' rows; either may be NULL (that
 *                                  tower does not run), not both.  Every record is checked as l3_upload_batch_sampled checks it,
 *                                  before anything is launched.
 * L3_EINVAL (message in l3_last_error(e)): a NULL pointer, n < 0 (sampled: n < 1), a tower other than 0 / 1, a destination on another
 * device, of another width, or too short. */
int l3_tower_dim(const l3_engine *e, int tower);
int l3_tower_features(l3_engine *e, int tower, const float *rows, int64_t n, float *out);
int l3_tower_features_dev(l3_engine *e, int tower, const float *rows, int64_t n, l3_feat *dst, int64_t row0);
int l3_tower_features_sampled_dev(l3_engine *e, l3_clipbank *bank, const l3_sample *records, int64_t n, l3_feat *vis, l3_feat *aud,
                                  int64_t row0);
/* The head over pairs.  dense_1 splits over the concatenation, W1 = [W1v; W1a] (vision rows first), and only the difference of the two
 * logits matters:
 *     u_i = v_i W1v   (Nv, head)        t_j = a_j W1a + b1   (Na, head)        wd = fl32(W2[:, 1] - W2[:, 0]),  bd = fl32(b2[1] - b2[0])
 *     margin_ij = sum_k relu(u_ik + t_jk) wd_k + bd = logit(corresponding) - logit(not);   P(corresponding)_ij = 1 / (1 + exp(-margin_ij))
 * (index 1 is `corresponding`: the labels row is {label, 1 - label}, sample.py:363,376).  A handle of its own: one device, one stream,
 * the head and the two projected sets resident; every call has finished when it returns; calls on one handle are not re-entrant.
 * Arithmetic, which is the contract (tests/pairs_ref.py derives the bounds from it):
 *   projection   every element is one float32 fma chain over k = 0 .. K-1 in that order, started at 0; t adds b1 last (one rounding).
 *                A row's bits depend on the row and the weights only: not on the rows projected with it, nor on its position.
 *   pair         acc = 0; for k = 0 .. head-1: acc = fma(max(fl32(u_k + t_k), 0), wd_k, acc); margin = fl32(acc + bd).  The same bits
 *                for the same pair in l3_pairs_matrix, any block of it, l3_pairs_list and l3_pairs_ranks.
 *   probability  fl32(1 / fl32(1 + expf(-margin))).
 * head: a multiple of 32 in [32, 4096]; a set holds at most 65535 * L3_PAIRS_TILE items.
 *   l3_pairs_set_head        w1 (nv + na, head), b1 (head), w2 (head, 2), b2 (2), row major; voids the projected sets
 *   l3_pairs_set_vision/_audio[_dev]   n host rows (n, nv | na), or rows [lo, hi) of an l3_feat on the handle's device -> U / T
 *   l3_pairs_matrix          the block [v0, v1) x [a0, a1) to the host, row major: margins, or probabilities when prob != 0
 *   l3_pairs_list            margin_out[q] = margin of the pair (iv[q], ia[q]), n >= 1
 *   l3_pairs_ranks           rank_v2a[i] = #{j : margin_ij > margin_{i, truth_a[i]} and group_a[j] != group_v[i]}   (Nv int32)
 *                            rank_a2v[j] = #{i : margin_ij > margin_{truth_v[j], j} and group_a[j] != group_v[i]}   (Na int32)
 *                            The comparison is strict: a tie with the truth does not count, and the truth pair never counts against
 *                            itself.  group_v / group_a: int32 clip ids, both NULL to exclude nothing.  A direction whose truth and
 *                            rank vectors are both NULL is not computed.  The matrix is never stored: a tile's comparisons are counted
 *                            in registers, summed over lanes, and added with one integer atomic per (row, tile); exact, and the same
 *                            from run to run.
 *   l3_pairs_topk            for every frame the k best-scoring seconds (idx_v2a, margin_v2a: (Nv, k) int32 / float32, row major), for
 *                            every second the k best-scoring frames (idx_a2v, margin_a2v: (Na, k)), by the order below.  A direction
 *                            is asked for by giving both of its outputs; one at least is needed, and the truth of a direction that is
 *                            not asked for is not read.  The matrix is never stored; the segment count is the library's choice.
 *   l3_pairs_time            device time in ms per launch over `reps` launches (hipEvents, one untimed launch first): what 0 the
 *                            whole matrix of margins, 1 the rank mode with the diagonal as truth (Nv == Na), 2 / 3 the vision / audio
 *                            projection of n_rows zero rows, 4 the top-k lists of both directions (all four launches) with the
 *                            diagonal as truth and no groups (Nv == Na) at k = 10, or at k = n_rows when n_rows != 0, 5 the merge
 *                            kernel of the frames' lists alone at that k.  For the records under profiles/.
 * The order of a list.  For a query frame i the candidates are the seconds j with group_a[j] != group_v[i] -- every j when no groups
 * are given -- and, when truth_a is given, j = truth_a[i] as well, whatever its group.  They stand in a strict total order:
 *   1. the larger margin first, by float comparison (+0 and -0 are equal);
 *   2. among equal margins the smaller index first;
 *   3. a candidate whose margin is NaN is never listed.
 * The list of i is the first k candidates of that order, in that order; a list with fewer than k candidates is filled up with index -1
 * and margin -inf.  The other direction is the same with frames and seconds exchanged (truth_v, lists of shape (Na, k)).  Every listed
 * margin has the bits l3_pairs_matrix and l3_pairs_list give for that pair: the same chain; fl32(u + t) is commutative, so the second
 * direction is the same kernel with U and T exchanged.  The order is strict, so the result is a function of the inputs alone: not of
 * the segment count, not of the order in which candidates meet inside a workgroup, not of the run.  No float atomics.
 * k in [1, L3_PAIRS_TOPK_MAX].  A truth without groups is refused (nothing is excluded, so there is nothing to keep); group_v and
 * group_a come together or not at all.  Truth values are checked before anything is launched.
 * L3_EINVAL (message in l3_last_error(NULL)): a NULL pointer, widths that do not match, an empty set or block, a block, a pair or a
 * truth index out of range, an l3_feat on another device.  L3_ESTATE: a call before the head or the sets it needs. */
#define L3_PAIRS_TILE 64        /* frames and seconds of one workgroup's tile of pairs */
#define L3_PAIRS_TOPK_MAX 64    /* entries of a top-k list: one per lane of a wave */
typedef struct l3_pairs l3_pairs;
int l3_pairs_create(int device, int nv, int na, int head, l3_pairs **p);
void l3_pairs_destroy(l3_pairs *p);
int l3_pairs_set_head(l3_pairs *p, const float *w1, const float *b1, const float *w2, const float *b2);
int l3_pairs_set_vision(l3_pairs *p, const float *rows, int64_t n);
int l3_pairs_set_audio(l3_pairs *p, const float *rows, int64_t n);
int l3_pairs_set_vision_dev(l3_pairs *p, const l3_feat *f, int64_t lo, int64_t hi);
int l3_pairs_set_audio_dev(l3_pairs *p, const l3_feat *f, int64_t lo, int64_t hi);
int l3_pairs_matrix(l3_pairs *p, int64_t v0, int64_t v1, int64_t a0, int64_t a1, int prob, float *out);
int l3_pairs_list(l3_pairs *p, const int32_t *iv, const int32_t *ia, int64_t n, float *margin_out);
int l3_pairs_ranks(l3_pairs *p, const int32_t *truth_a, const int32_t *truth_v, const int32_t *group_v, const int32_t *group_a,
                   int32_t *rank_v2a, int32_t *rank_a2v);
int l3_pairs_topk(l3_pairs *p, int k, const int32_t *truth_a, const int32_t *truth_v, const int32_t *group_v, const int32_t *group_a,
                  int32_t *idx_v2a, float *margin_v2a, int32_t *idx_a2v, float *margin_a2v);
int l3_pairs_time(l3_pairs *p, int what, int64_t n_rows, int reps, double *ms);
/* The two kernels alone on host buffers: out (n, H) = x (n, K) w (K, H) [+ b when b != NULL]; out (Nv, Na) = the margins of u (Nv, H)
 * and t (Na, H). */
int l3_op_project(int device, const float *x, const float *w, const float *b, int64_t n, int K, int H, float *out);
int l3_op_pair_margins(int device, const float *u, const float *t, const float *wd, float bd, int64_t Nv, int64_t Na, int H,
                       float *out);
/* One direction of l3_pairs_topk on projected rows from the host: the Nv rows of u are the queries, the Na rows of t the candidates
 * (exchange them for the other direction); truth (Nv) or NULL, group_q (Nv) and group_c (Na) or both NULL; idx, margin (Nv, k).
 * segments: into how many runs of tiles the candidates are cut, each with its own partial lists that a second kernel merges; 0 lets
 * the library choose, as l3_pairs_topk does; a count above the number of tiles is clamped to it.  In [0, 256]. */
int l3_op_pair_topk(int device, const float *u, const float *t, const float *wd, float bd, int64_t Nv, int64_t Na, int H, int k,
                    const int32_t *truth, const int32_t *group_q, const int32_t *group_c, int segments, int32_t *idx, float *margin);

/* ---- Sound localisation maps: the AVC head at every location of a tower's last feature map (csrc/locmap.hip) ---------
 * Both towers end in a global max pool -- the last MaxPooling2D of vision_model / audio_model reduces the feature map to 1 x 1, and
 * model.py:25-31 concatenates the two pooled rows into dense_1 -- so a pooled feature is the maximum of a per-location activation, and
 * the head has a value at every location: that location's C channels in place of the pooled row.  cnn_L3_melspec2: 28 x 28 image
 * locations, 32 x 24 time-frequency locations, C = 512.  The network was trained on the pooled rows only: a map is a read-out.
 *   l3_tower_locations_shape        H, W, C of the input of the tower's last pool (each may be NULL).  L3_EINVAL with a message when that
 *                                   pool does not reduce to 1 x 1 or C != l3_tower_dim(e, tower): such a model (tiny_L3's vision tower)
 *                                   has no per-location form of its head input.
 *   l3_tower_locations_dev          the tower run as l3_tower_features_dev runs it; the H W C values of each of the n items go to rows
 *                                   [(row0 + s) L, (row0 + s + 1) L) of dst, L = H W, a matrix with D == C: location-major (y, then x),
 *                                   as stored.  The values are the stored ones (a bfloat16-stored map is widened, which is exact):
 *                                   their maximum over the L rows of an item is that item's row of l3_tower_features, bit for bit.
 *                                   Only the real items of the last engine batch are written.
 *   l3_tower_locations_sampled_dev  the same from n >= 1 records of a bank, with the feed of l3_tower_features_sampled_dev; pooled
 *                                   (n rows from row0; may be NULL) receives the pooled rows of the same run.
 * Arguments and destinations are checked before anything is uploaded, with the conventions of l3_tower_features_dev.
 *
 * The map side of a pair handle.  One side's locations are projected like items -- vision: W1v, no bias; audio: W1a, + b1 -- into a
 * resident matrix M (n_items L, head); the queries are the opposite projected set (side 0: l3_pairs_set_audio*, side 1:
 * l3_pairs_set_vision*).  A (location, query) margin is the pair chain above, so it has the bits l3_pairs_list gives when that
 * location row is set as an item.
 *   l3_pairs_map_reserve   side 0: vision locations queried by seconds; 1: audio locations queried by frames.  n_items items of H x W
 *                          locations, n_items H W <= 2^31 - 65.  Drops an earlier map.
 *   l3_pairs_map_put       projects n_items L rows of loc (D == the tower's C, on the handle's device) from row lo_row into the items
 *                          [item0, item0 + n_items) of M.  Callers put chunks: the raw locations of 64 frames are 103 MB, M is 0.4 MB a
 *                          frame.  l3_pairs_set_head voids what was put (not the reservation); every item must be put again.
 *   l3_pairs_map_list      listed (item, query) pairs in CSR form by item: the queries of item i are query_idx[item_ptr[i] ..
 *                          item_ptr[i + 1]), item_ptr[0] == 0, n = item_ptr[n_items] >= 1.  For the q-th listed pair: maps (n, L) its
 *                          map, peak[q] = max_l and arg[q] the location attaining it.  Any of the three may be NULL, not all.
 *   l3_pairs_map_peaks     the block [i0, i1) x [j0, j1) of S_ij = max_l margin_ijl (row major, items x queries) and, when arg != NULL,
 *                          the locations attaining it.  No map is stored.
 *   l3_pairs_map_ranks     l3_pairs_ranks (its arguments and conventions; frames x seconds whichever side the map is) taken over S:
 *                          the truth pairs' S by the list mode, then one counting pass with integer adds.  S is never stored; strict,
 *                          exact and the same from run to run.
 *   l3_pairs_map_time      device ms per launch: what 0 the list mode over the diagonal (maps and peaks stored), 1 the peaks mode over
 *                          every (item, query), 2 the rank mode's counting pass with the diagonal as truth.  For the records.
 * The order of a peak.  The locations l = 0 .. L-1 of a (item, query) pair stand in a strict total order:
 *   1. the larger margin first, by float comparison (+0 and -0 are equal);
 *   2. among equal margins the smaller location index first;
 *   3. a location whose margin is NaN is never the peak.
 * peak and arg are the first location's margin and index; a pair whose margins are all NaN gives peak -inf and arg -1.  The order is
 * strict, so the result is a function of the inputs alone: not of the tiling, not of the order in which lanes meet.  No float atomics.
 * Checked before any launch: L >= 1, indices and blocks in range, loc on the handle's device and C wide; L3_ESTATE before the head, the
 * whole map or the query set is present.
 * l3_op_map_list / l3_op_map_peaks: the kernel alone on host buffers, m (n_items L, H) projected locations, t (n_q, H) queries. */
int l3_tower_locations_shape(const l3_engine *e, int tower, int *H, int *W, int *C);
int l3_tower_locations_dev(l3_engine *e, int tower, const float *rows, int64_t n, l3_feat *dst, int64_t row0);
int l3_tower_locations_sampled_dev(l3_engine *e, l3_clipbank *bank, const l3_sample *records, int64_t n, int tower, l3_feat *pooled,
                                   l3_feat *loc, int64_t row0);
int l3_pairs_map_reserve(l3_pairs *p, int side, int64_t n_items, int H, int W);
int l3_pairs_map_put(l3_pairs *p, const l3_feat *loc, int64_t lo_row, int64_t item0, int64_t n_items);
int l3_pairs_map_list(l3_pairs *p, const int64_t *item_ptr, const int32_t *query_idx, float *maps, float *peak, int32_t *arg);
int l3_pairs_map_peaks(l3_pairs *p, int64_t i0, int64_t i1, int64_t j0, int64_t j1, float *S, int32_t *arg);
int l3_pairs_map_ranks(l3_pairs *p, const int32_t *truth_a, const int32_t *truth_v, const int32_t *group_v, const int32_t *group_a,
                       int32_t *rank_v2a, int32_t *rank_a2v);
int l3_pairs_map_time(l3_pairs *p, int what, int reps, double *ms);
int l3_op_map_list(int device, const float *m, const float *t, const float *wd, float bd, int64_t n_items, int64_t L, int64_t n_q, int H,
                   const int64_t *item_ptr, const int32_t *query_idx, float *maps, float *peak, int32_t *arg);
int l3_op_map_peaks(int device, const float *m, const float *t, const float *wd, float bd, int64_t n_items, int64_t L, int64_t n_q, int H,
                    int64_t i0, int64_t i1, int64_t j0, int64_t j1, float *S, int32_t *arg);

/* ---- A group of MLP classifiers (the learning_rate x weight_decay search of classifier/train.py:638-651) ---------------------------
 * n_members models of one shape (D, C, batch) trained on ONE resident data set in the same launches: an epoch's step is seven
 * launches whatever the number of members, and the validation pass and prediction run every member per launch too.
 * Per member: weights, Adam moments, activations, split-K partials and counters, learning rate, weight decay.  Shared: the features,
 * labels and permutation.  Member i computes, bit for bit, what an l3_mlp created with (weight_decay[i], seed[i]) computes from the
 * same calls: l3_mlp is a group of one, on the same kernels, and no member's arithmetic depends on the others.  One stream per
 * handle; calls on one handle are not re-entrant.  Errors as l3_mlp: l3_last_error(NULL) gives the message. */
typedef struct l3_mlp_group l3_mlp_group;
/* l3_mlp_create for 1 <= n_members <= 16 models: member i gets weight_decay[i] and the Glorot draw l3_mlp_create makes from seed[i].
 * L3_EINVAL: D, C or batch outside l3_mlp_create's ranges, n_members outside [1, 16], a NULL array, a negative weight decay;
 * L3_ENOMEM: a failed allocation (a member needs what an l3_mlp needs but the staging block of predict, which is shared). */
int l3_mlp_group_create(int device, int D, int C, int batch, int n_members, const float *weight_decay, const uint64_t *seed,
                        l3_mlp_group **g);
void l3_mlp_group_destroy(l3_mlp_group *g);
/* a member's element count: l3_mlp_param_count */
int64_t l3_mlp_group_param_count(const l3_mlp_group *g);
/* l3_mlp_set_data / l3_mlp_set_data_dev: the same contract, checks and error codes; one resident copy serves all members. */
int l3_mlp_group_set_data(l3_mlp_group *g, const float *X_train, const int32_t *y_train, int64_t n_train, const float *X_valid,
                          const int32_t *y_valid, int64_t n_valid);
int l3_mlp_group_set_data_dev(l3_mlp_group *g, const l3_feat *train, int64_t lo, int64_t hi, const int32_t *y, const l3_feat *valid,
                              int64_t vlo, int64_t vhi, const int32_t *yv);
/* l3_mlp_epoch of every live member (live[i] != 0) at its own rate lr[i]: the steps over `perm` (Adam steps t0 + 1, ... for all of
 * them), then the validation rows.  lr, live: n_members entries.  stats_out (n_members x 4): loss, acc, val_loss, val_acc per member
 * as l3_mlp_epoch gives them.  A member that is not live is left as it is (weights, moments) and its four statistics are NaN; with
 * no live member nothing is launched.  L3_EINVAL: a NULL argument, t0 < 0, a perm entry outside [0, n_train); L3_ESTATE: no data. */
int l3_mlp_group_epoch(l3_mlp_group *g, const int32_t *perm, const float *lr, const int32_t *live, int64_t t0, double *stats_out);
/* keep_best: member i's weights (bit i of mask) are copied, device to device, into the member's own slot, replacing what it held;
 * restore_best copies them back.  The search's stand-in for ModelCheckpoint(save_best_only, save_weights_only) and the load_weights
 * that follows the fit: float32 copies, so the bits are those of the trip through model.h5.  The Adam moments are not part of it.
 * L3_EINVAL: a mask bit at or past n_members; L3_ESTATE: restore_best of a member that never was kept; L3_ENOMEM: the slots (one
 * more copy of the weights, allocated by the first keep_best) could not be allocated. */
int l3_mlp_group_keep_best(l3_mlp_group *g, uint32_t mask);
int l3_mlp_group_restore_best(l3_mlp_group *g, uint32_t mask);
/* l3_mlp_predict / l3_mlp_predict_dev through every member in one pass: probs_out (n_members, n, C), member i's rows as l3_mlp_predict
 * gives them (the same row blocks).  predict_resident: of the rows l3_mlp_group_set_data left on the device, the training rows
 * (valid 0) or the validation rows (valid 1), without another upload; L3_ESTATE when there are none. */
int l3_mlp_group_predict(l3_mlp_group *g, const float *X, int64_t n, float *probs_out);
int l3_mlp_group_predict_dev(l3_mlp_group *g, const l3_feat *x, int64_t lo, int64_t hi, float *probs_out);
int l3_mlp_group_predict_resident(l3_mlp_group *g, int valid, float *probs_out);
/* l3_mlp_get_weights / l3_mlp_set_weights of one member (keras order; n must be l3_mlp_group_param_count).  L3_EINVAL: no such
 * member, NULL, wrong n. */
int l3_mlp_group_get_weights(l3_mlp_group *g, int member, float *dst, int64_t n);
int l3_mlp_group_set_weights(l3_mlp_group *g, int member, const float *src, int64_t n);

/* ---- Downstream random forest (classifier/train.py:169-227) ----------------------------------------------------------------------
 * train_rf's sklearn.ensemble.RandomForestClassifier(n_estimators, random_state) with sklearn 0.19's defaults (Gini, bootstrap,
 * max_features sqrt(D), trees grown out), as a level-wise histogram forest on the GPU (csrc/forest.hip): per feature at
 * most 255 float32 cuts from a row sample, uint8 bin codes stored feature-major, every tree grown one level per launch group with
 * integer class counts and one float64 formula for a split's worth, so the trees do not depend on the order of any sum and equal a
 * NumPy restatement of the algorithm exactly (tests/forest_ref.py).  The caller draws the bootstrap multiplicities and the tree
 * seeds (NumPy's RandomState); a node's features are drawn on the device by a counter-based mixer of (tree seed, node, draw).
 * One handle owns one resident float32 matrix, one stream and at most one fitted or uploaded forest; calls on one handle are not
 * re-entrant and have finished when they return.  NaN inputs are out of contract.  Errors: l3_last_error(NULL). */
#define L3_FOREST_MAX_CLASSES 60       /* the (bin x class) histogram of a node and feature, 256 (C + 1) words, stays within 64 KiB of LDS */
#define L3_FOREST_MAX_CUTS 255         /* cuts per feature: a bin code is a uint8 */
#define L3_FOREST_MAX_DRAWS 256        /* max_features: the features drawn per node */
#define L3_FOREST_MAX_BIN_SAMPLE 8192  /* rows of the cut sample: one column of it is sorted in LDS */
#define L3_FOREST_NARROW_ROWS 64       /* a node of at most this many distinct rows can be searched by one wave, a lane per row */
typedef struct l3_forest_config {
    int32_t n_classes;          /* 1 .. L3_FOREST_MAX_CLASSES; labels are indices below it */
    int32_t max_features;       /* K distinct features per node, 1 .. min(D, L3_FOREST_MAX_DRAWS) */
    int32_t max_depth;          /* <= 0: unbounded (the level loop is bounded by n) */
    int32_t min_samples_split;  /* >= 2, counted in distinct rows as sklearn counts them under bootstrap weights */
    int32_t min_samples_leaf;   /* >= 1, distinct rows on each side of a split */
    int32_t wide_min_rows;      /* a node of at least this many distinct rows, or of more than L3_FOREST_NARROW_ROWS, is searched by a
                                   workgroup per (node, drawn feature) with the histogram in LDS; smaller ones by a wave per node.
                                   0: L3_FOREST_NARROW_ROWS + 1.  Both searches give the same trees. */
    int64_t n_bin_rows;         /* rows of the cut sample (<= L3_FOREST_MAX_BIN_SAMPLE); 0: every row (then n <= the same bound) */
    const int32_t *bin_rows;    /* the sample's rows, ascending and distinct; NULL with n_bin_rows 0 */
} l3_forest_config;
typedef struct l3_forest l3_forest;
int l3_forest_create(int device, l3_forest **m);
void l3_forest_destroy(l3_forest *m);
/* classifier/train.py:169-227 (clf.fit's X): X (n, D) float32 row major, copied once.  1 <= n < 2^31, 1 <= D <= 2^21 */
int l3_forest_set_data(l3_forest *m, const float *X, int64_t n, int D);
/* classifier/train.py:169-227 (clf.fit's X when preprocess_split_data left it on the device): l3_forest_set_data from rows [lo, hi)
 * of a device matrix, copied device to device; the l3_feat may be destroyed afterwards */
int l3_forest_set_data_dev(l3_forest *m, const struct l3_feat *f, int64_t lo, int64_t hi);
/* classifier/train.py:169-227 (clf.fit): n_trees trees on the resident matrix.  labels (n) class indices; boot (n_trees, n) the
 * bootstrap multiplicities of each tree's rows (a tree needs one non-zero row at least); seeds (n_trees) in [0, 2^31).  Every label,
 * sample row and config field is checked here, on the host, before anything is launched: L3_EINVAL names the first one out of
 * range.  The fitted forest replaces the handle's forest and is resident for l3_forest_predict_proba. */
int l3_forest_fit(l3_forest *m, const l3_forest_config *cfg, const int32_t *labels, int n_trees, const uint16_t *boot,
                  const int64_t *seeds);
/* the handle's forest: trees, nodes over all trees, classes, features (L3_ESTATE without one) */
int l3_forest_sizes(const l3_forest *m, int *n_trees, int64_t *n_nodes, int *n_classes, int *D);
/* classifier/train.py:169-227 (what joblib.dump keeps of clf.estimators_): the trees as flat arrays.  Tree t owns the nodes
 * [tree_off[t], tree_off[t + 1]) (tree_off has n_trees + 1 entries), numbered level by level in parent order, left before right,
 * the root first; left / right are node numbers inside the tree (-1 at a leaf); feature and bin are -1 and threshold 0 at a leaf;
 * a row goes left iff x[feature] <= threshold (threshold = the feature's cut number bin); counts (n_nodes, n_classes) are the
 * bootstrap-weighted class counts of the node's rows and n_distinct the number of distinct rows. */
int l3_forest_get_trees(l3_forest *m, int64_t *tree_off, int32_t *left, int32_t *right, int32_t *feature, float *threshold,
                        int32_t *bin, int32_t *counts, int32_t *n_distinct);
/* classifier/train.py:169-227 (joblib.load's side): a forest in l3_forest_get_trees' arrays becomes the handle's forest.  Checked on
 * the host: each child number lies above its parent's and inside the tree, both children or neither, features in [0, D), counts
 * non-negative with a positive sum at every leaf; L3_EINVAL otherwise. */
int l3_forest_set_trees(l3_forest *m, int n_trees, int n_classes, int D, const int64_t *tree_off, const int32_t *left,
                        const int32_t *right, const int32_t *feature, const float *threshold, const int32_t *counts);
/* classifier/train.py:169-227 (clf.predict_proba): out (n, n_classes) float64.  One thread per row walks the trees in order on the
 * raw features, adds each leaf's counts / their sum in float64 and divides by n_trees at the end: deterministic. */
int l3_forest_predict_proba(l3_forest *m, const float *X, int64_t n, int D, double *out);
/* classifier/train.py:169-227 (clf.predict_proba of a split on the device): l3_forest_predict_proba of rows [lo, hi) of a device
 * matrix: the same bits */
int l3_forest_predict_proba_dev(l3_forest *m, const struct l3_feat *f, int64_t lo, int64_t hi, double *out);
/* classifier/train.py:193-227, 623-630 (clf.predict / predict_proba of every forest of the n_estimators grid, and the per-file means
 * of :211-222; the entries around it cite classifier/train.py:169-227 for the forest as a whole): the rows scored by the first
 * prefix[g] trees of the resident forest for every g at once, each tree walked once per row.  Rows: exactly one of
 * host rows X (hi of them, lo 0, D features), rows [lo, hi) of the device matrix f, and rows [lo, hi) of the handle's resident matrix
 * (resident != 0).  prefix: n_prefix forest sizes, strictly increasing, in [1, n_trees].  labels: int32 class indices of the rows,
 * or NULL.  files: n_files pairs [start, end) over the rows, or NULL.  Outputs, each NULL when not wanted (a NULL proba is never
 * allocated or copied): pred (n_prefix, n) int32, the first of the largest probabilities; correct (n_prefix) int64, the rows whose
 * pred is their label (needs labels); file_mean (n_prefix, n_files, n_classes) float64 and file_pred (n_prefix, n_files) int32, a
 * file's rows added in row order, / their number, and the first of the largest (files and a file output come together); proba
 * (n_prefix, n, n_classes) float64.  For every row and class count / total of the leaf is added in float64 strictly in tree order
 * and divided by prefix[g] after tree prefix[g] - 1: the bits of l3_forest_predict_proba on the forest of the first prefix[g]
 * trees.  chunk_rows: the rows per launch, which bounds every scratch buffer (0: 2^28 bytes of float32 rows); stage_bytes: the LDS
 * budget of a workgroup's 4 rows, above which the walk reads them from global memory (0: 96 KiB, so D <= 6144); neither changes a
 * bit of the result.  Everything is checked on the host before anything is launched: L3_ESTATE without a forest or without the
 * resident matrix asked for, L3_EINVAL otherwise. */
int l3_forest_score(l3_forest *m, const float *X, const struct l3_feat *f, int64_t lo, int64_t hi, int D, int resident,
                    const int32_t *prefix, int n_prefix, const int32_t *labels, const int64_t *files, int64_t n_files,
                    int64_t chunk_rows, int64_t stage_bytes, int32_t *pred, int64_t *correct, double *file_mean, int32_t *file_pred,
                    double *proba);
/* classifier/train.py:169-227 (what oob_score=True adds to clf.fit, sklearn's _set_oob_score, at every forest size of the
 * n_estimators grid of :623-630): all rows of the handle's resident matrix -- the one the fit left there, or one set again with
 * l3_forest_set_data[_dev] after l3_forest_set_trees -- scored by the trees whose bootstrap missed them, for the first prefix[g]
 * trees of the resident forest for every g at once.  boot (n_trees, n): the bootstrap multiplicities the trees were
 * fitted with; n_trees must be the forest's tree count.  It is uploaded in slabs of 64 trees and kept as one 64-bit word per (row,
 * pass of 64 trees): bit j is set iff tree 64 pass + j has multiplicity 0 at the row.  prefix, labels, chunk_rows and stage_bytes
 * are l3_forest_score's.  Outputs, each NULL when not wanted (a NULL sums is never allocated or copied): pred (n_prefix, n) int32,
 * the first of the largest sums, 0 for a row that no tree of the prefix left out; correct (n_prefix) int64, the rows whose pred is
 * their label (needs labels); n_oob (n_prefix, n) int32, the trees of the prefix that left the row out; sums (n_prefix, n,
 * n_classes) float64, count / total of the leaf added in float64 strictly in tree order over those trees alone.  Nothing is divided
 * by a tree count here: sklearn's normalisation is the caller's.  Everything is checked on the host before anything is launched:
 * L3_ESTATE without a forest or without a resident matrix; L3_EINVAL for another tree count than the forest's, a matrix of another
 * width than the forest's, prefixes that are not strictly increasing or lie outside [1, n_trees], labels outside the classes, correct
 * without labels, or no output. */
int l3_forest_oob(l3_forest *m, const uint16_t *boot, int n_trees, const int32_t *prefix, int n_prefix, const int32_t *labels,
                  int64_t chunk_rows, int64_t stage_bytes, int32_t *pred, int64_t *correct, int32_t *n_oob, double *sums);
/* classifier/train.py:169-227 (the fit's binning, for tests): cuts (D, L3_FOREST_MAX_CUTS) and ncuts (D) of the last fit */
int l3_forest_get_cuts(l3_forest *m, float *cuts, int32_t *ncuts);
/* classifier/train.py:169-227 (the fit's course, for profiles): the last fit's levels -> their number; up to max_levels entries each of
 * the nodes searched at the level over all trees, those of them searched by the wide kernel, and the level's wall time in ms */
int l3_forest_level_stats(const l3_forest *m, int max_levels, int64_t *nodes, int64_t *wide, double *ms);

/* ---- Nearest neighbours among embedding rows: distance blocks, top-k lists, votes (csrc/knn.hip) ----------------------
 * A handle holds a database of n rows of D float32 (its own copy, with int32 labels or without) and a query set: rows of its own, or
 * the database itself (l3_knn_query_self: no second copy).  The N x N matrix is never stored: l3_knn_topk keeps only the lists.
 * Arithmetic, which is the contract (tests/knn_ref.py derives the bounds from it), the same in every call:
 *   dot(q, c) = fmaf(q[D-1], c[D-1], ... fmaf(q[0], c[0], 0)), one float32 chain in ascending feature order (what one accumulator of
 *               the fp32 matrix-core instruction gives); nn(x) = dot(x, x), once per row when the rows are set.
 *   L3_KNN_SQEUCLIDEAN  d = max(0, fl(fl(nn(q) + nn(c)) - 2 dot(q, c)))          (a NaN stays a NaN)
 *   L3_KNN_COSINE       d = fl(1 - fl(fl(dot(q, c) r(q)) r(c))), r(x) = fl(1 / fl(sqrt(nn(x)))), correctly rounded, and 0 for a row of
 *                       zero norm, whose distance to every row is therefore 1 (sklearn's convention).
 * The same pair has the same bits in l3_knn_matrix, any block of it, l3_knn_list and the lists, at every segment count.
 * The order of a neighbour list.  For a query i the candidates are the database rows j with group_c[j] != group_q[i] -- every j when
 * no groups are given.  Entry (d, j) is ahead of (d', j') iff d < d', or d == d' and j < j' (float comparison: +0 == -0); a candidate
 * whose distance is NaN is never listed.  The list of i is the first k candidates of that order, in that order; a list with fewer than
 * k candidates is filled up with index -1 and distance +inf.  The order is strict, so the lists are a function of the inputs alone.
 *   l3_knn_set_database[_dev]  n host rows (n, D), or rows [lo, hi) of an l3_feat on the handle's device (copied device to device);
 *                              labels (n, each >= 0) or NULL.  At most 2^31 - 1 rows.  Voids a self query's set until it returns.
 *   l3_knn_set_queries[_dev]   the same for the query side; l3_knn_query_self makes the database the query set.
 *   l3_knn_matrix              the block [q0, q1) x [c0, c1) of distances to the host, row major (tests and small jobs)
 *   l3_knn_list                out[p] = the distance of (query iq[p], database row ic[p]), n >= 1
 *   l3_knn_topk                idx_out, dist_out (nQ, k) int32 / float32, row major; group_q (nQ) and group_c (n) together or both NULL
 *   l3_knn_vote                l3_knn_topk at k, then, without downloading the lists, the votes of the neighbours' labels at the S <=
 *                              L3_KNN_MAX_SIZES list sizes ks (strictly ascending, in [1, k]: the first ks[s] entries of a sorted k-list
 *                              are the ks[s]-list).  Outputs, each NULL when not wanted: counts (nQ, S, n_classes) int32; pred (nQ, S)
 *                              int32, the class of the most votes, the lowest class among equals, -1 for a query without neighbours
 *                              (empty slots do not vote); with file_idxs (n_files int64 pairs [s, e) over the queries, 0 <= s < e <=
 *                              nQ) file_counts (n_files, S, n_classes) int32, the sum of the rows' votes, and file_pred (n_files, S),
 *                              chosen from them in the same way.  n_classes <= L3_KNN_MAX_CLASSES.  Integer arithmetic only.
 *   l3_knn_time                device time in ms per launch over `reps` launches (hipEvents, one untimed launch first): what 0 the
 *                              top-k pass at k (every segment's lists and their merge), 1 the matrix kernel over the block [0, min(nQ,
 *                              8192)) x [0, min(n, 8192)).  For the records under profiles/.
 *   l3_op_knn_topk             l3_knn_topk on host rows Q (nq, D) and C (nc, D) by the kernels alone.  segments: into how many runs of
 *                              tiles the candidates are cut, each with partial lists of its own that a second kernel merges; 0 lets the
 *                              library choose, as l3_knn_topk does; a count above the number of tiles is clamped to it.  In [0, 256].
 * L3_EINVAL (message in l3_last_error(NULL), naming the call): a NULL pointer, D <= 0, an unknown metric, k outside [1,
 * L3_KNN_TOPK_MAX], ks not ascending or above k, groups on one side only, a negative label, a label outside [0, n_classes), l3_knn_vote
 * on a database without labels, a query before both sides are set, a block, a pair or a file out of range, an l3_feat of another
 * width or on another device. */
#define L3_KNN_SQEUCLIDEAN 0
#define L3_KNN_COSINE 1
#define L3_KNN_TOPK_MAX 64        /* entries of a neighbour list: one per lane of a wave (the value of L3_PAIRS_TOPK_MAX) */
#define L3_KNN_MAX_SEGMENTS 256
#define L3_KNN_MAX_SIZES 8        /* list sizes of one l3_knn_vote */
#define L3_KNN_MAX_CLASSES 256
typedef struct l3_knn l3_knn;
int l3_knn_create(int device, int D, int metric, l3_knn **h);
void l3_knn_destroy(l3_knn *h);
int l3_knn_set_database(l3_knn *h, const float *rows, int64_t n, const int32_t *labels);
int l3_knn_set_database_dev(l3_knn *h, const l3_feat *f, int64_t lo, int64_t hi, const int32_t *labels);
int l3_knn_set_queries(l3_knn *h, const float *rows, int64_t n);
int l3_knn_set_queries_dev(l3_knn *h, const l3_feat *f, int64_t lo, int64_t hi);
int l3_knn_query_self(l3_knn *h);
int l3_knn_matrix(l3_knn *h, int64_t q0, int64_t q1, int64_t c0, int64_t c1, float *out);
int l3_knn_list(l3_knn *h, const int32_t *iq, const int32_t *ic, int64_t n, float *out);
int l3_knn_topk(l3_knn *h, int k, const int32_t *group_q, const int32_t *group_c, int32_t *idx_out, float *dist_out);
int l3_knn_vote(l3_knn *h, int k, const int32_t *ks, int S, int n_classes, const int32_t *group_q, const int32_t *group_c,
                const int64_t *file_idxs, int64_t n_files, int32_t *counts, int32_t *pred, int32_t *file_counts, int32_t *file_pred);
int l3_op_knn_topk(int device, const float *Q, const float *C, int64_t nq, int64_t nc, int D, int metric, int k, int segments,
                   const int32_t *group_q, const int32_t *group_c, int32_t *idx, float *dist);
int l3_knn_time(l3_knn *h, int what, int k, int reps, double *ms);

/* ---- K-means over embedding rows: Lloyd iterations, k-means++ seeding, label statistics (csrc/kmeans.hip) -------------
 * A handle holds n rows of D float32 (its own copy) and K centroids on one device.  Arithmetic, which is the contract (tests/
 * cluster_ref.py is its NumPy oracle), the same in every call:
 * Distances.  Squared Euclidean only (L3_KNN_COSINE is refused: a mean does not minimise it).  d(i, c) has exactly the bits that
 *   l3_knn_matrix gives for row i against centroid c under L3_KNN_SQEUCLIDEAN: dot is the ascending fmaf chain, nn(x) = dot(x, x) is
 *   computed once per row when the rows are set and once per centroid after every update, d = max(0, fl(fl(nn(q) + nn(c)) - 2 dot)),
 *   and a NaN stays a NaN.
 * Assignment.  label(i) is the centroid of the smallest distance, the smaller index among equal distances (the strict order of a
 *   neighbour list; +0 == -0); a NaN distance never wins.  A row whose distances are all NaN has label -1 and distance NaN and is
 *   left out of every count, sum and inertia.  The order is strict, so tiling and lane order do not enter.
 * The order of a float64 sum.  The members of a set, in ascending row index, are cut into consecutive runs of L3_KMEANS_RUN members;
 *   each run is summed sequentially from 0.0 in float64; the run sums are then added sequentially in ascending order.  There are no
 *   float atomics.  The order holds for the centroid sums S_c (members: the rows of cluster c), the inertia (members: the rows with
 *   label >= 0; terms: their float32 distances widened) and the seeding's cumulative potential (below).
 * Update.  n_c members: C[c][f] = (float)(S_c[f] / (double)n_c) where n_c > 0; an empty cluster keeps its centroid bit for bit and
 *   is counted (`empty`).  Empty clusters are not relocated.
 * l3_kmeans_fit runs the iterations it = 0 .. max_iter - 1: assign with the current centroids; record history[3 it ..] = inertia,
 *   changed (rows whose label differs from the iteration before; at it = 0 every row), empty (clusters without members); stop when
 *   changed == 0 (labels and centroids agree), else update.  When max_iter is used up one more assignment runs, so the labels, the
 *   distances and the inertia always belong to the centroids the handle holds.  *n_iter = the iterations run = history's rows.  The
 *   iteration's only read-back is those scalars.
 * Seeding.  l3_kmeans_seed_rows: centroid c = row rows[c].  l3_kmeans_seed_pp: plain k-means++, one candidate per step, from K draws
 *   u in [0, 1) made by the caller.  Centre 0 is row floor(u[0] n); mind[i] = d(i, centre 0); for t = 1 .. K - 1: cum[i] = the
 *   running total of mind in the order above (rows in runs of L3_KMEANS_RUN: within a run the sequential prefix from 0.0, a run's
 *   offset the sequential sum of the earlier runs' totals, cum[i] = fl(offset + prefix)); the pick is the first i with cum[i] >
 *   fl(u[t] cum[n - 1]); then mind[i] = d < mind[i] ? d : mind[i] with d = d(i, new centre).  Edge rules: a NaN mind counts as 0 in
 *   cum (such a row is never picked by the search) and stays NaN; when the total is 0 the pick is floor(u[t] n); when no i qualifies
 *   the pick is the last row with mind > 0.  A centre is a data row, so d(i, centre) has the bits l3_knn_list gives for that pair.
 *   chosen_out (K int64, or NULL): the centres' rows.
 *   l3_kmeans_set_rows[_dev]   n >= K host rows (n, D), or rows [lo, hi) of an l3_feat on the handle's device; voids the labels
 *   l3_kmeans_set_centroids    K host centroids (K, D)
 *   l3_kmeans_assign           one assignment of the rows: labels (n) int32, dist (n) float32, *inertia, *changed (against the
 *                              assignment before; every row after l3_kmeans_set_rows or a seeding).  Every output may be NULL:
 *                              nothing but the scalars is downloaded.  Also sorts the rows by label for l3_kmeans_update.
 *   l3_kmeans_update           the centroids of the last assignment's labels; counts_out (K int64, or NULL) = n_c
 *   l3_kmeans_get_labels       the last assignment's labels, distances and inertia (each may be NULL)
 *   l3_kmeans_get_centroids    (K, D) float32
 *   l3_kmeans_predict[_dev]    other rows against the current centroids: labels and dist (each may be NULL); they stay on the device
 *   l3_kmeans_contingency      table (K, n_classes) int64, row major: table[label][class] counts the rows of `which` (0: the fitted
 *                              rows' last assignment, 1: the last l3_kmeans_predict); classes: one int32 in [0, n_classes) per row;
 *                              n_classes <= L3_KMEANS_MAX_CLASSES.  Rows of label -1 are not counted.  Integer adds only.
 *   l3_kmeans_file_hist        hist (n_files, K) int32: the labels of the rows [s, e) of each file counted per cluster (file_idxs:
 *                              n_files int64 pairs, 0 <= s < e <= the rows of `which`).  Integer adds only.
 *   l3_kmeans_time             device time in ms per round over `reps` rounds (hipEvents, one untimed round first): what 0 the
 *                              assignment kernel, 1 the update, 2 a whole iteration (the centroids move on), 3 a k-means++ seeding of
 *                              all K centres (every draw 0.5; replaces the centroids), 4 the sort by label, 5 the inertia.  Voids
 *                              the labels.  For the records under profiles/.
 *   l3_op_kmeans_step          host rows (n, D) and centroids (K, D) in; labels, dist, *inertia, counts (K int64) and the updated
 *                              centroids out (each may be NULL), by the kernels alone.
 * L3_EINVAL (message in l3_last_error(NULL), naming the call, before the device is touched): a NULL pointer, D <= 0, K outside [1,
 * L3_KMEANS_MAX_CLUSTERS], K > n, L3_KNN_COSINE, max_iter < 1, a draw outside [0, 1), a seed row, class or file out of range,
 * n_classes outside [1, L3_KMEANS_MAX_CLASSES], a call before what it needs, an l3_feat of another width or on another device. */
#define L3_KMEANS_RUN 256               /* members of a run of a float64 sum */
#define L3_KMEANS_MAX_CLUSTERS 65536
#define L3_KMEANS_MAX_CLASSES 256
typedef struct l3_kmeans l3_kmeans;
int l3_kmeans_create(int device, int D, int K, int metric, l3_kmeans **h);
void l3_kmeans_destroy(l3_kmeans *h);
int l3_kmeans_set_rows(l3_kmeans *h, const float *rows, int64_t n);
int l3_kmeans_set_rows_dev(l3_kmeans *h, const l3_feat *f, int64_t lo, int64_t hi);
int l3_kmeans_set_centroids(l3_kmeans *h, const float *centroids);
int l3_kmeans_seed_rows(l3_kmeans *h, const int64_t *rows);
int l3_kmeans_seed_pp(l3_kmeans *h, const double *u, int64_t *chosen_out);
int l3_kmeans_assign(l3_kmeans *h, int32_t *labels, float *dist, double *inertia, int64_t *changed);
int l3_kmeans_update(l3_kmeans *h, int64_t *counts_out);
int l3_kmeans_fit(l3_kmeans *h, int max_iter, double *history_out, int *n_iter_out);
int l3_kmeans_get_labels(l3_kmeans *h, int32_t *labels, float *dist, double *inertia);
int l3_kmeans_get_centroids(l3_kmeans *h, float *out);
int l3_kmeans_predict(l3_kmeans *h, const float *rows, int64_t n, int32_t *labels, float *dist);
int l3_kmeans_predict_dev(l3_kmeans *h, const l3_feat *f, int64_t lo, int64_t hi, int32_t *labels, float *dist);
int l3_kmeans_contingency(l3_kmeans *h, int which, const int32_t *classes, int n_classes, int64_t *table);
int l3_kmeans_file_hist(l3_kmeans *h, int which, const int64_t *file_idxs, int64_t n_files, int32_t *hist);
int l3_kmeans_time(l3_kmeans *h, int what, int reps, double *ms);
int l3_op_kmeans_step(int device, const float *rows, const float *centroids, int64_t n, int K, int D, int32_t *labels, float *dist,
                      double *inertia, int64_t *counts, float *new_centroids);

/* ---- t-SNE: a map of n points in the plane from neighbour lists (csrc/tsne.hip) ---------------------------------------
 * Exact t-SNE (no tree, no grid, no approximation parameter) over a sparse symmetric P.  The map is 2-D only.  Arithmetic, which is
 * the contract (tests/tsne_ref.py is its float64 oracle and derives the bounds), the same in every call; a fit is a function of its
 * inputs alone, there are no float atomics, two runs give the same bits:
 * Calibration.  l3_op_tsne_conditional: per row of k sorted-or-not distances d_j, p_j = exp(-beta (d_j - min_j d_j)) / sum_p with
 *   H(beta) = log(perplexity), H the Shannon entropy in nats.  Everything is float64; every sum runs over j ascending from 0.0:
 *   sum_p += p_j, sum_dp += fl(d_j p_j); H = log(sum_p) + fl(fl(beta sum_dp) / sum_p).  The search is the bracket rule: beta = 1, lo =
 *   -inf, hi = +inf; H > log(perplexity): lo = beta, beta = hi == +inf ? 2 beta : (beta + hi) / 2; else hi = beta, beta = lo == -inf ?
 *   beta / 2 : (beta + lo) / 2.  Exactly L3_TSNE_SEARCH_STEPS moves run, with no early exit; p_out and beta_out are those of the beta
 *   the last move left (one more evaluation).  A row of equal distances gives the uniform row.  A row with a NaN or an infinite
 *   distance gives a NaN row and beta, and *bad_rows (may be NULL) counts such rows.
 * Repulsive pass.  R_i = sum_{j != i} q_ij^2 (y_i - y_j), z_i = sum_{j != i} q_ij, q_ij = 1 / (1 + |y_i - y_j|^2); the term j = i is
 *   left out (not subtracted); a coincident other point counts 1 in z_i and 0 in R_i.  Per pair, float32: dx = y_i.x - y_j.x (dy
 *   likewise), d2 = fmaf(dx, dx, fl(dy dy)), q = rcp(fl(1 + d2)) with the hardware's approximate reciprocal (1 ulp), R.x =
 *   fmaf(fl(q q), dx, R.x), z = fl(z + q).  Order: j ascending in runs of L3_TSNE_RUN; a run is a float32 chain from 0; the run sums
 *   are added into float64 in ascending order, per segment of consecutive runs, from 0.0; the segments' float64 partials are added in
 *   ascending order from 0.0.  l3_tsne_geometry gives what the bits depend on, a function of n alone: row_block = 256 for n <= 8192,
 *   else 1024 (rows of a workgroup; a lane owns row_block / 256 rows); with runs = ceil(n / 256) and row_blocks = ceil(n / row_block):
 *   runs_per_segment = max(1, ceil(runs row_blocks / 1024)), segments = ceil(runs / runs_per_segment).
 * Sums over rows.  Z = sum_i z_i and the KL part sum_i kl_i: rows ascending in runs of L3_TSNE_RUN, a run summed sequentially from 0.0
 *   in float64, the run sums added sequentially in ascending order.
 * Attractive pass.  A_i = sum_{j in row i} P_ij q_ij (y_i - y_j), kl_i = sum_j P_ij log1p(d2_ij), in float64 from the float32
 *   coordinates: d2 = fma(dx, dx, fl(dy dy)), pq = fl(P fl(1 / fl(1 + d2))), A.x = fma(pq, dx, A.x), kl = fma(P, log1p(d2), kl).  Lane l
 *   of 64 takes the row's entries l, l + 64, ... in order from 0.0; the lanes are folded by the xor butterfly 32, 16, ..., 1 (v = v +
 *   v[lane ^ m]).  KL = sum P log P + sum_i kl_i + log Z, with P log P summed on the host over the entries in order (0 log 0 = 0).
 * Update.  Per coordinate: g = (float)(4.0 * (exaggeration * A - R / Z)) in float64; inc = fl(u g) < 0.0f (a zero product is not an
 *   increase); gain = inc ? fl(gain + 0.2f) : fl(gain 0.8f), then 0.01f where gain < 0.01f; u = fl(fl(momentum u) - fl(fl(lr gain)
 *   g)) with momentum and lr narrowed to float32; y = fl(y + u).  There is no recentring.
 *   l3_tsne_create             a handle for maps of n points on one device
 *   l3_tsne_set_affinities     P as CSR: indptr (n + 1) int64, cols int32, vals float32.  Any symmetric P whose entries sum to 1 (the
 *                              caller's to ensure); a row may be empty.  Refused: unsorted (not strictly ascending) or out-of-range
 *                              columns, a diagonal entry, a negative or non-finite value.  Computes sum P log P once.
 *   l3_tsne_set_embedding      y (n, 2) float32; the last update becomes 0, the gains 1, the iteration count 0
 *   l3_tsne_get_embedding      y (n, 2) float32
 *   l3_tsne_run                n_iter iterations (repulsive, attractive, update) with no read-back except the records: at every
 *                              kl_every-th iteration of the call and at its last, one record of 3 float64 into history_out (may be
 *                              NULL): the iteration's index since l3_tsne_set_embedding, KL (of the map before that iteration's
 *                              update, with the P that was set: exaggeration does not enter), Z.  history_out holds n_iter / kl_every
 *                              + 1 records; *n_records the number written.  Z stays on the device for the update.  A Z that is zero
 *                              or not finite at a record stops the run with L3_EINVAL.
 *   l3_tsne_time               device time in ms per round over `reps` rounds (hipEvents, one untimed round first): what 0 the
 *                              repulsive pass with its finish and Z, 1 the attractive pass, 2 the update, 3 a whole iteration, 4 the
 *                              pair kernel alone.  The map moves on under 2 and 3.  For the records under profiles/.
 *   l3_op_tsne_repulsive       y (n, 2) in; R (n, 2), z (n) float64 and *Z out (each may be NULL), by the kernels alone
 *   l3_op_tsne_attractive      y and a CSR P in; A (n, 2) float64, *kl_rows = sum_i kl_i and *plogp = sum P log P out
 *   l3_op_tsne_update          y, update, gains (n, 2) float32 in and out; A, R (n, 2) float64 and Z in
 * L3_EINVAL (message in l3_last_error(NULL), naming the call): a NULL pointer, n outside [1, 2^24], k outside [2, L3_KNN_TOPK_MAX],
 * perplexity outside (1, k), a CSR as above, n_iter or kl_every < 1, exaggeration or learning rate <= 0, momentum outside [0, 1).
 * L3_ESTATE: l3_tsne_run or l3_tsne_get_embedding before what it needs. */
#define L3_TSNE_RUN 256                 /* pairs of a float32 chain; rows of a run of a float64 sum */
#define L3_TSNE_SEARCH_STEPS 100        /* moves of the calibration's bracket, always all of them */
typedef struct l3_tsne l3_tsne;
int l3_op_tsne_conditional(int device, const float *dist, int64_t n, int k, double perplexity, double *p_out, double *beta_out,
                           int64_t *bad_rows);
int l3_tsne_geometry(int64_t n, int *row_block, int *segments);
int l3_tsne_create(int device, int64_t n, l3_tsne **h);
void l3_tsne_destroy(l3_tsne *h);
int l3_tsne_set_affinities(l3_tsne *h, const int64_t *indptr, const int32_t *cols, const float *vals);
int l3_tsne_set_embedding(l3_tsne *h, const float *y);
int l3_tsne_get_embedding(l3_tsne *h, float *y);
int l3_tsne_run(l3_tsne *h, int n_iter, double exaggeration, double momentum, double learning_rate, int kl_every, double *history_out,
                int *n_records);
int l3_tsne_time(l3_tsne *h, int what, int reps, double *ms);
int l3_op_tsne_repulsive(int device, const float *y, int64_t n, double *R_out, double *z_out, double *Z_out);
int l3_op_tsne_attractive(int device, const float *y, int64_t n, const int64_t *indptr, const int32_t *cols, const float *vals,
                          double *A_out, double *kl_rows_out, double *plogp_out);
int l3_op_tsne_update(int device, int64_t n, float *y, float *update, float *gains, const double *A, const double *R, double Z,
                      double exaggeration, double momentum, double learning_rate);

/* ---- Principal components of embedding rows: mean, scatter matrix, projection (csrc/pca.hip) -------------------------
 * A handle holds n >= 2 rows of D float32 (its own copy) on one device and, apart from them, a model of k <= D components.  The
 * eigendecomposition between the two is the caller's (l3embedding_amd/pca.py: numpy.linalg.eigh of S / (n - 1) in float64).
 * Arithmetic, which is the contract (tests/pca_ref.py derives the bounds from it), the same in every call and on every device; there
 * are no float atomics, and two calls give the same bits:
 * Mean.  The rows are cut into segments of L3_PCA_MEAN_SEG consecutive rows.  A column's sum over a segment is sequential in float64,
 *   in ascending row order from 0.0; the segment sums are added sequentially in ascending order from 0.0; m64 = sum / (double)n and m32
 *   = (float)m64.  The handle keeps both.  l3_pca_set_mean instead gives the handle an m32 of the caller's (m64 is its widening).
 * Scatter.  S = sum over the rows of xc xc^T with xc = fl32(x - m32): one float32 subtraction as a row is staged.  The rows are cut into
 *   chains of L3_PCA_CHAIN consecutive rows: chain c is the rows [L3_PCA_CHAIN c, min(n, L3_PCA_CHAIN (c + 1))), C = ceil(n /
 *   L3_PCA_CHAIN) of them.  Within a chain an entry (i, j) is one float32 accumulator of v_mfma_f32_32x32x2_f32 taking the rows in
 *   ascending order from 0: fmaf(xc[r][i], xc[r][j], acc).  The chains are dealt to `splits` row ranges: split s is the chains [floor(s
 *   C / splits), floor((s + 1) C / splits)).  A split's partial is the float64 sum of its chains' results, widened, in ascending chain
 *   order from 0.0; S is the float64 sum of the splits' partials in ascending split order, starting from the first.  Only the entries
 *   i <= j are computed; each is written to (i, j) and (j, i), so S equals its transpose bit for bit.  The error of an entry against
 *   the exact sum of the float32 xc is at most gamma_R sum_rows |xc_i xc_j|, gamma_R = R u / (1 - R u) with R = L3_PCA_CHAIN and u =
 *   2^-24, plus the float64 sums' term.  L3_PCA_CHAIN is 256: the bound grows with it, and the float64 fold at a chain's end (64
 *   conversions and additions a lane against the chain's 512 matrix instructions a wave) is already about one percent of the time.
 *   splits: in [0, L3_PCA_MAX_SPLITS]; a count above C is clamped to C; 0 means the count l3_pca_splits names, a function of n and D
 *   alone and never of the device: max(1, min(C, L3_PCA_MAX_SPLITS, floor(L3_PCA_FILL / U))) with T = ceil(D / 128) and U = T (T + 1) / 2, the
 *   128 x 128 tiles on or above the diagonal (D = 512: U = 10, 51 splits at n >= 12 801; D = 6144: U = 1176, 1 split).
 *   Workspace rule: beside the rows the handle holds splits x D x D float64 of partials and D x D float64 of S, grown on demand and
 *   kept (D = 512 at 51 splits: 107 MB + 2 MB; D = 6144 at 1 split: 302 MB + 302 MB).
 * Projection.  l3_pca_transform: y[i][c] = the ascending fmaf chain over d from 0 of fl32(x[i][d] - mean[d]) w[c][d] (the dot product
 *   of the nearest-neighbour tile: D is never split over waves or accumulators), then, with a scale, fl32(y scale[c]) once.
 *   l3_pca_inverse: x[i][d] = fl32(chain + mean[d]), chain over c from 0 of fl32(y[i][c] / scale[c]) w[c][d], the same kernel on the transposed
 *   components, which l3_pca_set_model makes once; without a scale there is no division.
 *   l3_pca_set_rows[_dev]      n >= 2 host rows (n, D), or rows [lo, hi) of an l3_feat on the handle's device (copied device to device);
 *                              voids the mean.  A NaN or an infinity in the rows is refused with the lowest such row named.
 *   l3_pca_mean                computes m64 and m32 of the rows; mean_out (D float64) and mean32_out (D float32) may each be NULL
 *   l3_pca_set_mean            m32 = mean32 (D finite float32): a scatter about a mean of the caller's
 *   l3_pca_scatter             S_out (D, D) float64, row major, about the handle's m32; S_out may be NULL, and S then only stays on the
 *                              device (l3_eig_set_matrix_pca)
 *   l3_pca_splits              the count that splits = 0 stands for at (n, D)
 *   l3_pca_set_model           k components (k, D) row major, the model's mean32 (D) and scale (k, each finite and > 0) or NULL;
 *                              independent of the rows and of the mean the scatter uses
 *   l3_pca_transform[_dev]     n >= 1 host rows (n, D) -> out (n, k); the _dev form takes rows [lo, hi) of an l3_feat and writes to out
 *                              (host, may be NULL) and / or to a new l3_feat of (hi - lo, k) on the same device (*out_feat, when
 *                              out_feat is not NULL), which the caller destroys
 *   l3_pca_inverse[_dev]       the same from (n, k) to (n, D)
 *   l3_pca_time                device time in ms per round over `reps` rounds (hipEvents, one untimed round first): what 0 the mean, 1
 *                              the scatter (both kernels, splits = 0), 2 the projection of the fitted rows, 3 the scatter's tile
 *                              kernel alone.  For the records under profiles/.
 * L3_EINVAL (message in l3_last_error(NULL), naming the call): a NULL pointer, D outside [1, L3_PCA_MAX_D], n outside [2, 2^31 - 1]
 * (projections: [1, 2^31 - 1]), a row that is not finite, splits outside [0, L3_PCA_MAX_SPLITS], k outside [1, D], a scale that is not
 * positive and finite, a projection with no output, an l3_feat of another width or on another device.  L3_ESTATE: a call before the
 * rows, the mean or the model it needs. */
#define L3_PCA_CHAIN 256                /* rows of a float32 chain of the scatter: R of the error bound */
#define L3_PCA_MEAN_SEG 256             /* rows of a segment of the mean's float64 sums */
#define L3_PCA_FILL 512                 /* workgroups that splits = 0 aims at: two on each of 256 compute units */
#define L3_PCA_MAX_SPLITS 256
#define L3_PCA_MAX_D 16384
typedef struct l3_pca l3_pca;
int l3_pca_create(int device, int D, l3_pca **h);
void l3_pca_destroy(l3_pca *h);
int l3_pca_splits(int64_t n, int D, int *splits);
int l3_pca_set_rows(l3_pca *h, const float *rows, int64_t n);
int l3_pca_set_rows_dev(l3_pca *h, const l3_feat *f, int64_t lo, int64_t hi);
int l3_pca_mean(l3_pca *h, double *mean_out, float *mean32_out);
int l3_pca_set_mean(l3_pca *h, const float *mean32);
int l3_pca_scatter(l3_pca *h, int splits, double *S_out);
int l3_pca_set_model(l3_pca *h, int k, const float *mean32, const float *components, const float *scale);
int l3_pca_transform(l3_pca *h, const float *rows, int64_t n, float *out);
int l3_pca_transform_dev(l3_pca *h, const l3_feat *f, int64_t lo, int64_t hi, float *out, l3_feat **out_feat);
int l3_pca_inverse(l3_pca *h, const float *Y, int64_t n, float *out);
int l3_pca_inverse_dev(l3_pca *h, const l3_feat *f, int64_t lo, int64_t hi, float *out, l3_feat **out_feat);
int l3_pca_time(l3_pca *h, int what, int reps, double *ms);

/* ---- Symmetric top-k problems: the device side of block subspace iteration ("The subspace solver"; csrc/eig.hip) --------
 * A handle holds a symmetric float64 matrix S (D, D) on one device and two blocks of m vectors, V and W: the rows of (m, D) row-major
 * float64 matrices.  The iteration is the caller's (l3embedding_amd/eigen.py): its m x m problems go to LAPACK on the host, whatever
 * is D long stays on the device.
 * Arithmetic, which is the contract (tests/eig_ref.py derives the bounds from it).  Every entry of the result of apply, gram and mix is
 *   ONE float64 accumulator of v_mfma_f64_16x16x4_f64 that takes its reduction index in ascending steps of 4 from 0, padded with zeros
 *   past the end.  No reduction is split, so the order is a function of (D, m) alone, there are no float atomics, and two calls give
 *   the same bits.  The order of the four products inside one instruction is the hardware's, so the claim is a bound and not equality
 *   with an ascending chain: |c - exact| <= gamma_(K + 1) sum |a b|, gamma_n = n u / (1 - n u), u = 2^-53, K the reduction length (D
 *   for apply and gram, m for mix).  Products and sums of small integers are exact.
 *   l3_eig_create            1 <= D <= L3_PCA_MAX_D, 1 <= m <= min(D, L3_EIG_MAX_M).  The handle allocates S, three blocks (the third is
 *                            what a mix writes) and two m x m matrices: 8 (D^2 + 3 m D + 2 m^2) bytes.  The blocks start as zeros.
 *   l3_eig_set_matrix        S from the host (D, D).  Refused unless every entry is finite and S equals its transpose bit for bit; the
 *                            message names the lowest offending (i, j) in row-major order.
 *   l3_eig_set_matrix_pca    S = the scatter matrix that the last l3_pca_scatter of `pca` left on the same device (a copy on the
 *                            device); L3_ESTATE if there is none, L3_EINVAL for another device or another D.
 *   l3_eig_trace             the diagonal of S summed in ascending order in float64 on the host
 *   l3_eig_set_block / l3_eig_get_block   block `which` (L3_EIG_V or L3_EIG_W) from / to the host (m, D)
 *   l3_eig_apply             W_j = S V_j for every j: W[j][d] = sum over e of V[j][e] S[d][e]
 *   l3_eig_gram              G[i][j] = <a_i, b_j> to the host (m, m), a and b each L3_EIG_V or L3_EIG_W.  With a == b only i <= j is
 *                            computed and written to (i, j) and (j, i): G equals its transpose bit for bit.
 *   l3_eig_mix               dst_j = sum over i of M[j][i] src_i, M (m, m) row major from the host.  The result is written to the third
 *                            block, which then changes places with dst: dst may be src, with the same bits as into the other block.
 *   l3_eig_residual          res[j] = ||W_j - theta_j V_j||_2 to the host (m): fl(w - fl(theta v)) squared, 256 interleaved sequential
 *                            sums a row folded by a fixed tree, one square root
 *   l3_eig_time              device time in ms per round over `reps` rounds (hipEvents, one untimed round first): what 0 apply, 1
 *                            gram(V, W), 2 the product of a mix of V by the resident m x m matrix, 3 residual.  For profiles/.
 * L3_EINVAL: a NULL pointer, D or m out of range, a block index that is neither L3_EIG_V nor L3_EIG_W, a matrix that is not finite or
 * not symmetric.  L3_ESTATE: apply or trace before the matrix. */
#define L3_EIG_MAX_M 1024
#define L3_EIG_V 0
#define L3_EIG_W 1
typedef struct l3_eig l3_eig;
int l3_eig_create(int device, int D, int m, l3_eig **h);
void l3_eig_destroy(l3_eig *h);
int l3_eig_set_matrix(l3_eig *h, const double *S);
int l3_eig_set_matrix_pca(l3_eig *h, const l3_pca *pca);
int l3_eig_trace(l3_eig *h, double *trace);
int l3_eig_set_block(l3_eig *h, int which, const double *B);
int l3_eig_get_block(l3_eig *h, int which, double *B);
int l3_eig_apply(l3_eig *h);
int l3_eig_gram(l3_eig *h, int a, int b, double *G);
int l3_eig_mix(l3_eig *h, int src, const double *M, int dst);
int l3_eig_residual(l3_eig *h, const double *theta, double *res);
int l3_eig_time(l3_eig *h, int what, int reps, double *ms);

#ifdef __cplusplus
}
#endif
#endif /* L3HIP_H */
