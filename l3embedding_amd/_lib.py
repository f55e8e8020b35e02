"""ctypes binding of libl3hip.so (the C ABI declared in include/l3hip.h).

There is deliberately no CPU fallback: if the HIP library is missing or no AMD GPU is
visible the product path raises.
"""
import ctypes as C
import os

import numpy as np

from . import _build

MODEL_IDS = {
    'cnn_L3_orig': 0,
    'tiny_L3': 1,
    'cnn_L3_kapredbinputbn': 2,
    'cnn_L3_melspec1': 3,
    'cnn_L3_melspec2': 4,
}

FAMILIES = ('conv_fwd', 'conv_dgrad', 'conv_wgrad', 'elementwise', 'frontend', 'head', 'adam')


DTYPES = {'f32': 0, 'fp32': 0, 'float32': 0, 'bf16': 1}
FP32_CONV = {'f4x4': 0, 'f2x2': 1, 'f2x2_bf16x6': 2}        # L3_FP32_CONV_*: Winograd F(4x4,3x3) (default, fastest) / F(2x2,3x3) (tightest parity)
DP_MOVING = {'replicas': 0, 'rank_local': 1}       # l3_config.dp_moving (include/l3hip.h L3_DP_MOVING_*)
FRONTENDS = {'kapre': 0, 'minispec': 1}            # l3_config.frontend (include/l3hip.h L3_FRONTEND_*)
OP_DTYPES = dict(DTYPES, bf16_stored=2, bf16_stored_out=3)     # L3_OP_BF16_STORED: conv operator entry points only


class L3Config(C.Structure):
    _fields_ = [
        ('struct_size', C.c_int32),
        ('model_type', C.c_int32),
        ('batch', C.c_int32),
        ('global_batch', C.c_int32),
        ('device', C.c_int32),
        ('db_max_scope', C.c_int32),
        ('bn_zero_debias', C.c_int32),
        ('dtype', C.c_int32),
        ('stream', C.c_void_p),
        ('fp32_conv', C.c_int32),
        ('dp_moving', C.c_int32),
    ]


class L3Config2(L3Config):
    """`struct l3_config` of include/l3hip.h as it is now: L3Config, the struct as it was before the front-end form (a
    struct_size the library still accepts, and gives the kapre form), and the field added at its end."""
    _fields_ = [('frontend', C.c_int32)]


class L3Error(RuntimeError):
    pass


_f32p = C.POINTER(C.c_float)
_lib = None
TORCH_LOADED_FIRST = None     # set by load()

# name -> (restype, argtypes); every symbol include/l3hip.h declares
SIGNATURES = {
    'l3_create': (C.c_int, [C.POINTER(L3Config), C.c_uint64, C.POINTER(C.c_void_p)]),
    'l3_destroy': (None, [C.c_void_p]),
    'l3_last_error': (C.c_char_p, [C.c_void_p]),
    'l3_build_experiments': (C.c_int, []),
    'l3_comm_version': (C.c_int, []),
    'l3_bn_stats_pack_dev': (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    'l3_bn_stats_replicas_dev': (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    'l3_model_type_from_name': (C.c_int, [C.c_char_p]),
    'l3_device_count': (C.c_int, []),
    'l3_param_count': (C.c_int, [C.c_void_p]),
    'l3_param_info': (C.c_int, [C.c_void_p, C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int32),
                                C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
    'l3_set_param': (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64]),
    'l3_get_param': (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64]),
    'l3_get_grad': (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64]),
    'l3_reset_optimizer': (C.c_int, [C.c_void_p]),
    'l3_copy_state': (C.c_int, [C.c_void_p, C.c_void_p]),
    'l3_optimizer_steps': (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'l3_forward': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    'l3_train_step': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float,
                                C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    'l3_eval_step': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    'l3_upload_batch': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'l3_upload_batch_raw': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'l3_tower_step': (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    'l3_stage_batch_raw': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'l3_upload_batch_raw_aug': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'l3_stage_batch_raw_aug': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'l3_batch_gains': (C.c_int, [C.c_void_p, C.c_void_p]),
    # AVC samples cut on the device from decoded clips held there (csrc/avsample.hip)
    'l3_clipbank_create': (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]),
    'l3_clipbank_add': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int,
                                  C.POINTER(C.c_int)]),
    'l3_clipbank_info': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    'l3_clipbank_audio': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    'l3_clipbank_destroy': (None, [C.c_void_p]),
    'l3_upload_batch_sampled': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    'l3_stage_batch_sampled': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    'l3_op_sample_batch': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'l3_step_forward': (C.c_int, [C.c_void_p, C.c_int]),
    'l3_step_bucket_count': (C.c_int, [C.c_void_p]),
    'l3_step_backward_bucket': (C.c_int, [C.c_void_p, C.c_int]),
    'l3_step_update': (C.c_int, [C.c_void_p, C.c_float, C.c_float]),
    'l3_step_resident': (C.c_int, [C.c_void_p, C.c_float]),
    # serial replicas: multi_gpu_model's replicas one after another on one engine (csrc/engine.hip)
    'l3_replicas_upload': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    'l3_replicas_upload_raw': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    'l3_replicas_stage_raw': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    'l3_replicas_upload_raw_aug': (C.c_int, [C.c_void_p] * 6 + [C.c_int]),
    'l3_replicas_stage_raw_aug': (C.c_int, [C.c_void_p] * 6 + [C.c_int]),
    'l3_step_replicas': (C.c_int, [C.c_void_p, C.c_float]),
    'l3_eval_replicas': (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    'l3_step_results': (C.c_int, [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p, C.c_void_p]),
    'l3_step_results_enqueue': (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    'l3_step_results_wait': (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    'l3_comm_unique_id': (C.c_int, [C.c_void_p]),
    'l3_comm_init': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    'l3_comm_destroy': (C.c_int, [C.c_void_p]),
    'l3_comm_info': (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_int]),
    'l3_comm_allreduce_host': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int, C.c_int]),
    'l3_step_dp': (C.c_int, [C.c_void_p, C.c_float]),
    'l3_comm_timing': (C.c_int, [C.c_void_p, C.c_int]),
    'l3_comm_timing_read': (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int)]),
    'l3_grad_arena_dev': (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    'l3_bucket_range': (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'l3_embed_audio': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    'l3_embed_vision': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    'l3_embed_dim': (C.c_int64, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    'l3_embed_audio_frames': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                                        C.c_void_p]),
    'l3_embed_audio_clips_resampled': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                                 C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                                                 C.c_void_p]),
    # ... with the pooled rows kept on the device, in rows [row0, row0 + n_frames) of an l3_feat
    'l3_embed_audio_frames_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                                            C.c_void_p, C.c_int64]),
    'l3_embed_audio_clips_resampled_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                                     C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                                                     C.c_void_p, C.c_int64]),
    # vision embeddings from raw uint8 frames of any size, resized and cropped on the device (csrc/frames.hip)
    'l3_embed_vision_frames': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                                         C.c_void_p]),
    'l3_embed_vision_frames_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                                             C.c_void_p, C.c_int64]),
    'l3_get_activation': (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64]),
    'l3_activation_numel': (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64)]),
    'l3_sync': (C.c_int, [C.c_void_p]),
    'l3_profile_enable': (C.c_int, [C.c_void_p, C.c_int]),
    'l3_set_tower_overlap': (C.c_int, [C.c_void_p, C.c_int]),
    'l3_profile_read_executed': (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double)]),
    'l3_profile_read_bytes': (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double)]),
    'l3_profile_read': (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                  C.POINTER(C.c_double)]),
    'l3_op_conv2d_fwd': (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 8),
    'l3_op_conv2d_fwd_dt': (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 8),
    'l3_op_conv2d_bwd_dt': (C.c_int, [C.c_int, C.c_int] + [C.c_void_p] * 6 + [C.c_int] * 8),
    'l3_op_conv2d_bwd': (C.c_int, [C.c_int] + [C.c_void_p] * 6 + [C.c_int] * 8),
    'l3_op_bn_relu_fwd': (C.c_int, [C.c_int] + [C.c_void_p] * 6 + [C.c_int64, C.c_int, C.c_int, C.c_int]),
    'l3_op_bn_relu_bwd': (C.c_int, [C.c_int] + [C.c_void_p] * 10 + [C.c_int64, C.c_int, C.c_int, C.c_int]),
    'l3_op_bn_relu_pool2_fwd': (C.c_int, [C.c_int] + [C.c_void_p] * 6 + [C.c_int] * 7),
    'l3_op_bn_relu_pool2_bwd': (C.c_int, [C.c_int] + [C.c_void_p] * 8 + [C.c_int] * 7),
    'l3_op_maxpool_fwd': (C.c_int, [C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 9),
    'l3_op_maxpool_bwd': (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 9),
    'l3_op_frontend': (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    'l3_op_frontend_form': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    'l3_spectrogram_shape': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'l3_audio_spectrograms': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    'l3_embed_audio_spec': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    'l3_embed_audio_spec_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int64]),
    'l3_tower_dim': (C.c_int, [C.c_void_p, C.c_int]),
    'l3_tower_features': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    'l3_tower_features_dev': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]),
    'l3_tower_features_sampled_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]),
    'l3_tower_locations_shape': (C.c_int, [C.c_void_p, C.c_int] + [C.POINTER(C.c_int)] * 3),
    'l3_tower_locations_dev': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]),
    'l3_tower_locations_sampled_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int64]),
    'l3_pairs_map_reserve': (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.c_int]),
    'l3_pairs_map_put': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64]),
    'l3_pairs_map_list': (C.c_int, [C.c_void_p] * 6),
    'l3_pairs_map_peaks': (C.c_int, [C.c_void_p] + [C.c_int64] * 4 + [C.c_void_p, C.c_void_p]),
    'l3_pairs_map_ranks': (C.c_int, [C.c_void_p] * 7),
    'l3_pairs_map_time': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    'l3_op_map_list': (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int64, C.c_int64, C.c_int64, C.c_int] + [C.c_void_p] * 5),
    'l3_op_map_peaks': (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int64, C.c_int64, C.c_int64, C.c_int] + [C.c_int64] * 4 +
                        [C.c_void_p, C.c_void_p]),
    'l3_pairs_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    'l3_pairs_destroy': (None, [C.c_void_p]),
    'l3_pairs_set_head': (C.c_int, [C.c_void_p] * 5),
    'l3_pairs_set_vision': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    'l3_pairs_set_audio': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    'l3_pairs_set_vision_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]),
    'l3_pairs_set_audio_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]),
    'l3_pairs_matrix': (C.c_int, [C.c_void_p] + [C.c_int64] * 4 + [C.c_int, C.c_void_p]),
    'l3_pairs_list': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'l3_pairs_ranks': (C.c_int, [C.c_void_p] * 7),
    'l3_pairs_topk': (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 8),
    'l3_pairs_time': (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int, C.POINTER(C.c_double)]),
    'l3_op_project': (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p]),
    'l3_op_pair_margins': (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int64, C.c_int64, C.c_int, C.c_void_p]),
    'l3_op_pair_topk': (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_int64, C.c_int64, C.c_int, C.c_int] +
                        [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_void_p]),
    # nearest neighbours among embedding rows (csrc/knn.hip)
    'l3_knn_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    'l3_knn_destroy': (None, [C.c_void_p]),
    'l3_knn_set_database': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'l3_knn_set_database_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    'l3_knn_set_queries': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    'l3_knn_set_queries_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]),
    'l3_knn_query_self': (C.c_int, [C.c_void_p]),
    'l3_knn_matrix': (C.c_int, [C.c_void_p] + [C.c_int64] * 4 + [C.c_void_p]),
    'l3_knn_list': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'l3_knn_topk': (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 4),
    'l3_knn_vote': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64] +
                    [C.c_void_p] * 4),
    'l3_op_knn_topk': (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64] + [C.c_int] * 4 + [C.c_void_p] * 4),
    'l3_knn_time': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    # k-means over embedding rows (csrc/kmeans.hip)
    'l3_kmeans_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    'l3_kmeans_destroy': (None, [C.c_void_p]),
    'l3_kmeans_set_rows': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    'l3_kmeans_set_rows_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]),
    'l3_kmeans_set_centroids': (C.c_int, [C.c_void_p, C.c_void_p]),
    'l3_kmeans_seed_rows': (C.c_int, [C.c_void_p, C.c_void_p]),
    'l3_kmeans_seed_pp': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'l3_kmeans_assign': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    'l3_kmeans_update': (C.c_int, [C.c_void_p, C.c_void_p]),
    'l3_kmeans_fit': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_int)]),
    'l3_kmeans_get_labels': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    'l3_kmeans_get_centroids': (C.c_int, [C.c_void_p, C.c_void_p]),
    'l3_kmeans_predict': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    'l3_kmeans_predict_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]),
    'l3_kmeans_contingency': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    'l3_kmeans_file_hist': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    'l3_kmeans_time': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    # t-SNE maps (csrc/tsne.hip)
    'l3_op_tsne_conditional': (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    'l3_tsne_geometry': (C.c_int, [C.c_int64, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'l3_tsne_create': (C.c_int, [C.c_int, C.c_int64, C.POINTER(C.c_void_p)]),
    'l3_tsne_destroy': (None, [C.c_void_p]),
    'l3_tsne_set_affinities': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    'l3_tsne_set_embedding': (C.c_int, [C.c_void_p, C.c_void_p]),
    'l3_tsne_get_embedding': (C.c_int, [C.c_void_p, C.c_void_p]),
    'l3_tsne_run': (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int, C.c_void_p, C.POINTER(C.c_int)]),
    'l3_tsne_time': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    'l3_op_tsne_repulsive': (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    'l3_op_tsne_attractive': (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double),
                                        C.POINTER(C.c_double)]),
    'l3_op_tsne_update': (C.c_int, [C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_double] * 4),
    # principal components of embedding rows (csrc/pca.hip)
    'l3_pca_create': (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    'l3_pca_destroy': (None, [C.c_void_p]),
    'l3_pca_splits': (C.c_int, [C.c_int64, C.c_int, C.POINTER(C.c_int)]),
    'l3_pca_set_rows': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    'l3_pca_set_rows_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]),
    'l3_pca_mean': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'l3_pca_set_mean': (C.c_int, [C.c_void_p, C.c_void_p]),
    'l3_pca_scatter': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    'l3_pca_set_model': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'l3_pca_transform': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'l3_pca_transform_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.POINTER(C.c_void_p)]),
    'l3_pca_inverse': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'l3_pca_inverse_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.POINTER(C.c_void_p)]),
    'l3_pca_time': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    # symmetric top-k problems: the device side of block subspace iteration (csrc/eig.hip)
    'l3_eig_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    'l3_eig_destroy': (None, [C.c_void_p]),
    'l3_eig_set_matrix': (C.c_int, [C.c_void_p, C.c_void_p]),
    'l3_eig_set_matrix_pca': (C.c_int, [C.c_void_p, C.c_void_p]),
    'l3_eig_trace': (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    'l3_eig_set_block': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    'l3_eig_get_block': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    'l3_eig_apply': (C.c_int, [C.c_void_p]),
    'l3_eig_gram': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    'l3_eig_mix': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    'l3_eig_residual': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'l3_eig_time': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double)]),
    'l3_op_kmeans_step': (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_double),
                                    C.c_void_p, C.c_void_p]),
    'l3_frontend_cfg': (C.c_int, [C.c_int] * 5 + [C.c_void_p]),
    'l3_frontend_tables': (C.c_int, [C.c_void_p, C.c_int] + [C.c_void_p] * 8 + [C.c_int64, C.POINTER(C.c_int64)]),
    'l3_op_frontend_frames': (C.c_int, [C.c_int, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p] * 4),
    'l3_op_dft_twiddle': (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    'l3_op_spec_to_features': (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p, C.c_int, C.c_void_p]),
    'l3_op_dft_fused': (C.c_int, [C.c_int, C.c_void_p] + [C.c_int] * 6 + [C.c_void_p, C.c_int, C.c_void_p]),
    'l3_op_db_normalize': (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int64, C.c_int]),
    'l3_op_gather_frames': (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    'l3_op_image_frames': (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    'l3_op_resample': (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int,
                                 C.c_int64, C.c_int64, C.c_void_p]),
    'l3_op_resample_clips': (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64,
                                       C.c_int, C.c_int64, C.c_int, C.c_void_p]),
    'l3_op_bn_stats_from_partials': (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_float,
                                               C.c_void_p, C.c_void_p]),
    'l3_op_conv2d_fwd_stats': (C.c_int, [C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.POINTER(C.c_int), C.c_void_p, C.c_void_p] +
                               [C.c_int] * 9),
    'l3_op_conv2d_dgrad_bn_bwd': (C.c_int, [C.c_int, C.c_int] + [C.c_void_p] * 9 + [C.POINTER(C.c_int), C.c_void_p, C.c_void_p] +
                                  [C.c_int] * 9 + [C.c_int64]),
    'l3_op_first_block_bwd': (C.c_int, [C.c_int] * 3 + [C.c_void_p] * 24 + [C.c_int] * 5),
    'l3_op_first_conv_grads': (C.c_int, [C.c_int] + [C.c_void_p] * 8 + [C.c_int] * 3),
    'l3_op_bn_relu_pool2_fwd_xwin': (C.c_int, [C.c_int] + [C.c_void_p] * 7 + [C.c_int] * 7),
    'l3_op_preprocess': (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'l3_op_augment_video': (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    'l3_op_augment_audio': (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # downstream MLP classifier (csrc/mlp.hip)
    'l3_mlp_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_uint64, C.POINTER(C.c_void_p)]),
    'l3_mlp_destroy': (None, [C.c_void_p]),
    'l3_mlp_param_count': (C.c_int64, [C.c_void_p]),
    'l3_mlp_set_data': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]),
    'l3_mlp_epoch': (C.c_int, [C.c_void_p, C.c_void_p, C.c_float, C.c_int64, C.POINTER(C.c_double)]),
    'l3_mlp_predict': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'l3_mlp_get_weights': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    'l3_mlp_set_weights': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    'l3_op_mlp_dense_fwd': (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                      C.c_void_p, C.c_int, C.c_void_p]),
    'l3_op_mlp_dense_bwd_x': (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    'l3_op_mlp_wgrad': (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    'l3_op_mlp_wgrad_adam': (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
                             + [C.c_void_p] * 6 + [C.c_float, C.c_float, C.c_void_p]),
    'l3_op_mlp_softmax_ce': (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float] + [C.c_void_p] * 4),
    'l3_op_adam': (C.c_int, [C.c_int] + [C.c_void_p] * 4 + [C.c_int64, C.c_int64, C.c_float, C.c_float]),
    'l3_op_adam_scaled': (C.c_int, [C.c_int] + [C.c_void_p] * 4 + [C.c_int64, C.c_int64] + [C.c_float] * 6),
    'l3_op_arena_fold': (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int]),
    # head / loss / L2 sums / BatchNorm moving averages on their own (csrc/elementwise.hip)
    'l3_op_head_dense_fwd': (C.c_int, [C.c_int] + [C.c_void_p] * 4 + [C.c_int] * 4),
    'l3_op_head_dense_bwd': (C.c_int, [C.c_int] + [C.c_void_p] * 6 + [C.c_int] * 3),
    'l3_op_softmax_ce2': (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_float] + [C.c_void_p] * 3),
    'l3_op_sumsq': (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    'l3_op_bn_moving_update': (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 4
                               + [C.c_int64, C.c_int, C.c_int64, C.c_float, C.c_int, C.c_int64, C.c_void_p, C.c_int64]),
    # downstream SVM classifier (csrc/svm.hip)
    'l3_svm_create': (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    'l3_svm_destroy': (None, [C.c_void_p]),
    'l3_svm_set_data': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int]),
    'l3_svm_fit': (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int64, C.c_int] + [C.c_void_p] * 3
                   + [C.c_int] + [C.c_void_p] * 5),
    'l3_svm_fit_costs': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int64, C.c_int] + [C.c_void_p] * 3
                         + [C.c_int] + [C.c_void_p] * 5),
    'l3_svm_cv_decision': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 8),
    'l3_op_svm_sigmoid_train': (C.c_int, [C.c_int, C.c_int] + [C.c_void_p] * 6),
    'l3_svm_decision': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,
                                  C.c_int64, C.c_int] + [C.c_void_p] * 4),
    'l3_op_svm_kernel_rows': (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                        C.c_int, C.c_void_p]),
    'l3_op_svm_smo': (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_double, C.c_int64,
                                C.c_void_p, C.c_void_p, C.c_void_p]),
    # ... its scoring (csrc/svm_eval.hip)
    'l3_svm_set_data_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]),
    'l3_svm_get_rows': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'l3_svm_set_model': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int] + [C.c_void_p] * 5),
    'l3_svm_score': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_void_p,
                               C.c_void_p, C.c_int64] + [C.c_void_p] * 6),
    'l3_op_svm_tail': (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
                       + [C.c_void_p] * 8),
    # VGGish baseline features (csrc/vggish.hip)
    'l3_vggish_create': (C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    'l3_vggish_destroy': (None, [C.c_void_p]),
    'l3_vggish_batch': (C.c_int, [C.c_void_p]),
    'l3_vggish_set_conv': (C.c_int, [C.c_void_p, C.c_int]),
    'l3_vggish_set_weight': (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64]),
    'l3_vggish_set_pca': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'l3_vggish_embed_clips_resampled': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                                  C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int,
                                                  C.c_void_p]),
    'l3_op_vggish_logmel': (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    'l3_op_vggish_conv1': (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    'l3_op_vggish_bias_relu': (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 5),
    'l3_op_vggish_postprocess': (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    'l3_op_vggish_conv': (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p] + [C.c_int] * 6),
    # fold preprocessing of the classifier (csrc/featprep.hip) and its hand-off to the MLP (csrc/mlp.hip)
    'l3_feat_create': (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_void_p)]),
    'l3_feat_alloc': (C.c_int, [C.c_int, C.c_int64, C.c_int64, C.POINTER(C.c_void_p)]),
    'l3_feat_destroy': (None, [C.c_void_p]),
    'l3_feat_shape': (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    'l3_feat_download': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    'l3_feat_assemble': (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]),
    'l3_feat_gather': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    'l3_feat_split': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    'l3_feat_minmax': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'l3_feat_affine32': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'l3_feat_moments': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'l3_feat_standardize': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'l3_feat_file_stats': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    'l3_mlp_set_data_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                      C.c_void_p]),
    'l3_mlp_predict_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    'l3_mlp_predict_files_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    'l3_op_file_mean': (C.c_int, [C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    # a group of MLPs trained in the same launches (csrc/mlp.hip)
    'l3_mlp_group_create': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    'l3_mlp_group_destroy': (None, [C.c_void_p]),
    'l3_mlp_group_param_count': (C.c_int64, [C.c_void_p]),
    'l3_mlp_group_set_data': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64]),
    'l3_mlp_group_set_data_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                                            C.c_int64, C.c_void_p]),
    'l3_mlp_group_epoch': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'l3_mlp_group_keep_best': (C.c_int, [C.c_void_p, C.c_uint32]),
    'l3_mlp_group_restore_best': (C.c_int, [C.c_void_p, C.c_uint32]),
    'l3_mlp_group_predict': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    'l3_mlp_group_predict_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    'l3_mlp_group_predict_resident': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    'l3_mlp_group_get_weights': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]),
    'l3_mlp_group_set_weights': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]),
    # downstream random forest (csrc/forest.hip): classifier/train.py:169-227
    'l3_forest_create': (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    'l3_forest_destroy': (None, [C.c_void_p]),
    'l3_forest_set_data': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int]),
    'l3_forest_set_data_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]),
    'l3_forest_fit': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    'l3_forest_sizes': (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'l3_forest_get_trees': (C.c_int, [C.c_void_p] * 9),
    'l3_forest_set_trees': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6),
    'l3_forest_predict_proba': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]),
    'l3_forest_predict_proba_dev': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    'l3_forest_score': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                  C.c_void_p, C.c_int64, C.c_int64, C.c_int64] + [C.c_void_p] * 5),
    'l3_forest_oob': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64] + [C.c_void_p] * 4),
    'l3_forest_get_cuts': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    'l3_forest_level_stats': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
}


def lib_path():
    # developer A/B of two builds on one box (scripts/ab_step.sh); like every other switch only behind L3_DEBUG_KNOBS=1
    if os.environ.get('L3_DEBUG_KNOBS') == '1' and os.environ.get('L3_LIB_PATH'):
        return os.path.abspath(os.environ['L3_LIB_PATH'])
    return _build.LIBPATH


def load():
    """dlopen libl3hip.so and bind every declared symbol.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise L3Error('libl3hip.so not built (%s); run `python -c "import __graft_entry__ as g; g.build()"`. '
                      'There is no CPU fallback.' % path)
    global TORCH_LOADED_FIRST
    import sys
    # PyTorch-ROCm bundles its own libamdhip64 / librccl under the system SONAMEs.  Imported BEFORE this
    # library, its copies satisfy libl3hip's dependencies and the process has one HIP runtime (needed to
    # share streams / device pointers with torch or with the RCCL torch loaded); imported AFTER, the
    # process ends up with two runtimes that cannot see each other's memory.
    TORCH_LOADED_FIRST = 'torch' in sys.modules
    # An engine uses up to four HIP streams (two towers, input staging, RCCL); with HIP's default of 4 hardware queues
    # per process they start sharing queues with each other (and with torch's), and one stream's event waits become
    # false dependencies of another (csrc/comm.hip).  Read by the HIP runtime when it initialises, so it only takes
    # effect if no HIP call was made yet in this process; launchers should export it themselves.
    os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)      # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def experiments_built():
    """True if libl3hip.so carries the measured-and-rejected kernel variants (_build.py L3_BUILD_EXPERIMENTS=1)."""
    return bool(load().l3_build_experiments())


def comm_unique_id():
    """Rank 0: the 128-byte ncclUniqueId to hand to every rank's Engine.comm_init()."""
    buf = C.create_string_buffer(128)
    check(load().l3_comm_unique_id(buf))
    return buf.raw


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def require_single_hip_runtime(what):
    """Raises if torch is about to be (or was) imported after libl3hip in this process."""
    import sys
    if _lib is not None and not TORCH_LOADED_FIRST and 'torch' in sys.modules:
        raise L3Error('%s needs torch and libl3hip to share one HIP runtime: `import torch` before the first engine / '
                      'l3embedding_amd._lib.load() in this process' % what)
    if _lib is not None and not TORCH_LOADED_FIRST and 'torch' not in sys.modules:
        raise L3Error('%s would import torch after libl3hip was loaded (two HIP runtimes in one process): '
                      '`import torch` first' % what)


def check(rc, handle=None):
    if rc != 0:
        msg = load().l3_last_error(handle)
        raise L3Error('libl3hip error %d: %s' % (rc, msg.decode() if msg else '?'))


class Engine(object):
    """Thin RAII wrapper over an l3_engine handle."""

    def __init__(self, model_type, batch, device=0, global_batch=0, db_max_scope='sample',
                 bn_zero_debias=True, seed=20180123, stream=None, dtype='f32', fp32_conv='f4x4', dp_moving='replicas',
                 frontend='kapre'):
        if model_type not in MODEL_IDS:
            raise ValueError('Invalid model type: "{}"'.format(model_type))
        self.lib = load()
        self.model_type = model_type
        self.batch = int(batch)
        self.device = int(device)
        cfg = L3Config2()
        cfg.struct_size = C.sizeof(L3Config2)
        cfg.model_type = MODEL_IDS[model_type]
        cfg.batch = int(batch)
        cfg.global_batch = int(global_batch)
        cfg.device = int(device)
        cfg.db_max_scope = 0 if db_max_scope == 'sample' else 1
        cfg.bn_zero_debias = 1 if bn_zero_debias else 0
        cfg.stream = stream
        if dtype not in DTYPES:
            raise ValueError('dtype must be one of %s' % sorted(DTYPES))
        cfg.dtype = DTYPES[dtype]
        self.dtype = dtype
        if fp32_conv not in FP32_CONV:
            raise ValueError('fp32_conv must be one of %s' % sorted(FP32_CONV))
        cfg.fp32_conv = FP32_CONV[fp32_conv]
        self.fp32_conv = fp32_conv
        if dp_moving not in DP_MOVING:
            raise ValueError('dp_moving must be one of %s' % sorted(DP_MOVING))
        cfg.dp_moving = DP_MOVING[dp_moving]
        self.dp_moving = dp_moving
        if frontend not in FRONTENDS:
            raise ValueError('frontend must be one of %s' % sorted(FRONTENDS))
        cfg.frontend = FRONTENDS[frontend]
        self.frontend = frontend
        h = C.c_void_p()
        rc = self.lib.l3_create(C.byref(cfg), int(seed), C.byref(h))
        check(rc, None)
        self.h = h
        self._params = None

    def close(self):
        if getattr(self, 'h', None):
            self.lib.l3_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- parameters ---------------------------------------------------------------------
    def param_table(self):
        if self._params is None:
            out = []
            n = self.lib.l3_param_count(self.h)
            buf = C.create_string_buffer(256)
            for i in range(n):
                nd, tr, ne = C.c_int32(), C.c_int32(), C.c_int64()
                shp = (C.c_int64 * 4)()
                check(self.lib.l3_param_info(self.h, i, buf, 256, C.byref(nd), shp, C.byref(tr), C.byref(ne)), self.h)
                out.append((buf.value.decode(), tuple(int(shp[k]) for k in range(nd.value)), bool(tr.value)))
            self._params = out
        return self._params

    def set_param(self, name, value):
        v = _f32(value)
        check(self.lib.l3_set_param(self.h, name.encode(), _ptr(v), v.size), self.h)

    def get_param(self, name, shape):
        out = np.empty(shape, dtype=np.float32)
        check(self.lib.l3_get_param(self.h, name.encode(), _ptr(out), out.size), self.h)
        return out

    def get_grad(self, name, shape):
        out = np.empty(shape, dtype=np.float32)
        check(self.lib.l3_get_grad(self.h, name.encode(), _ptr(out), out.size), self.h)
        return out

    def set_params(self, P):
        for name, shape, _ in self.param_table():
            if name in P:
                self.set_param(name, np.asarray(P[name]).reshape(shape))

    def get_params(self):
        from collections import OrderedDict
        return OrderedDict((n, self.get_param(n, s)) for n, s, _ in self.param_table())

    def get_grads(self):
        from collections import OrderedDict
        return OrderedDict((n, self.get_grad(n, s)) for n, s, t in self.param_table() if t)

    def reset_optimizer(self):
        check(self.lib.l3_reset_optimizer(self.h), self.h)

    def copy_state_from(self, other):
        """Parameters, Adam moments / step and BatchNorm debias accumulators of `other`, device to device."""
        check(self.lib.l3_copy_state(self.h, other.h), self.h)

    def optimizer_steps(self):
        """(Adam iterations, BatchNorm moving-average updates) applied so far."""
        t, b = C.c_int64(), C.c_int64()
        check(self.lib.l3_optimizer_steps(self.h, C.byref(t), C.byref(b)), self.h)
        return t.value, b.value

    # -- steps --------------------------------------------------------------------------
    def forward(self, video, audio, training=False):
        v, a = _f32(video), _f32(audio)
        assert v.shape[0] == self.batch and a.shape[0] == self.batch
        probs = np.empty((self.batch, 2), np.float32)
        logits = np.empty((self.batch, 2), np.float32)
        check(self.lib.l3_forward(self.h, _ptr(v), _ptr(a), int(training), _ptr(probs), _ptr(logits)), self.h)
        return probs, logits

    def train_step(self, video, audio, labels, lr):
        v, a, l = _f32(video), _f32(audio), _f32(labels)
        loss, acc = C.c_float(), C.c_float()
        check(self.lib.l3_train_step(self.h, _ptr(v), _ptr(a), _ptr(l), lr, C.byref(loss), C.byref(acc)), self.h)
        return loss.value, acc.value

    def eval_step(self, video, audio, labels):
        v, a, l = _f32(video), _f32(audio), _f32(labels)
        loss, acc = C.c_float(), C.c_float()
        check(self.lib.l3_eval_step(self.h, _ptr(v), _ptr(a), _ptr(l), C.byref(loss), C.byref(acc)), self.h)
        return loss.value, acc.value

    def upload_batch(self, video=None, audio=None, labels=None):
        v, a, l = _f32(video), _f32(audio), _f32(labels)
        check(self.lib.l3_upload_batch(self.h, _ptr(v), _ptr(a), _ptr(l)), self.h)

    def _aug_args(self, params, u, replicas=None):
        p, g = augment_records(params), np.ascontiguousarray(u, dtype=np.float64)
        if replicas is not None:
            self._replica_rows(replicas, p, g)
        elif len(p) != self.batch or len(g) != self.batch:
            raise ValueError('%d augmentation records and %d gain draws for a batch of %d' % (len(p), len(g), self.batch))
        return p, g

    def _send_raw(self, fn, video_u8, audio_i16, labels_i32, records=None, replicas=None):
        """One batch in the stored dtypes to the entry point `fn`: the arrays cast (None: that input stays as it was), their rows
        checked against `replicas` slices, the (params, u) records packed."""
        args = [None if x is None else np.ascontiguousarray(x, dtype=t)
                for x, t in ((video_u8, np.uint8), (audio_i16, np.int16), (labels_i32, np.int32))]
        if replicas is not None:
            self._replica_rows(replicas, *args)
        if records is not None:
            args += self._aug_args(records[0], records[1], replicas)
        tail = [] if replicas is None else [int(replicas)]
        check(fn(self.h, *([_ptr(x) for x in args] + tail)), self.h)

    def upload_batch_raw(self, video_u8=None, audio_i16=None, labels_i32=None):
        self._send_raw(self.lib.l3_upload_batch_raw, video_u8, audio_i16, labels_i32)

    def stage_batch_raw(self, video_u8, audio_i16, labels_i32):
        """Next batch to the device while the current step runs; adopted by the next step_forward()."""
        self._send_raw(self.lib.l3_stage_batch_raw, video_u8, audio_i16, labels_i32)

    def upload_batch_raw_aug(self, video_u8, audio_i16, labels_i32, params, u):
        """upload_batch_raw with the batch augmented on the way (data/avc/sample.py:146-162,241-281)."""
        self._send_raw(self.lib.l3_upload_batch_raw_aug, video_u8, audio_i16, labels_i32, (params, u))

    def stage_batch_raw_aug(self, video_u8, audio_i16, labels_i32, params, u):
        """stage_batch_raw with the records; the adopting step augments the batch in place of scaling it."""
        self._send_raw(self.lib.l3_stage_batch_raw_aug, video_u8, audio_i16, labels_i32, (params, u))

    def batch_gains(self):
        """Audio gains of the augmented batch the engine holds (waits for the device)."""
        out = np.empty(self.batch, np.float64)
        check(self.lib.l3_batch_gains(self.h, _ptr(out)), self.h)
        return out

    def upload_batch_sampled(self, bank, records, augment=False):
        """upload_batch_raw[_aug] of a batch the engine cuts itself from a ClipBank's clips by `records` (SAMPLE_RECORD rows)."""
        r = sample_records(records)
        check(self.lib.l3_upload_batch_sampled(self.h, bank.h, _ptr(r), len(r), int(bool(augment))), self.h)

    def stage_batch_sampled(self, bank, records, augment=False):
        """stage_batch_raw[_aug] of such a batch: the tables go up and the kernels run on the copy stream, behind the running step."""
        r = sample_records(records)
        check(self.lib.l3_stage_batch_sampled(self.h, bank.h, _ptr(r), len(r), int(bool(augment))), self.h)

    def tower_step(self, tower, backward=True):
        """One tower alone ('vision' | 'audio') on the resident batch: training-mode forward (+ backward
        from mean(output))."""
        check(self.lib.l3_tower_step(self.h, {'vision': 0, 'audio': 1}[tower], int(backward)), self.h)

    def step_forward(self, training=True):
        check(self.lib.l3_step_forward(self.h, int(training)), self.h)

    def bucket_count(self):
        return self.lib.l3_step_bucket_count(self.h)

    def step_backward_bucket(self, b):
        check(self.lib.l3_step_backward_bucket(self.h, b), self.h)

    def step_update(self, lr, grad_scale=1.0):
        check(self.lib.l3_step_update(self.h, lr, grad_scale), self.h)

    def step_resident(self, lr):
        check(self.lib.l3_step_resident(self.h, lr), self.h)

    # -- serial replicas: multi_gpu_model's replicas one after another on this engine (batch = the slice, global_batch = R * batch) --
    def _replica_rows(self, replicas, *arrays):
        rows = int(replicas) * self.batch
        for a in arrays:
            if len(a) != rows:
                raise ValueError('%d rows for %d replicas of batch %d (%d rows)' % (len(a), replicas, self.batch, rows))

    def replicas_upload(self, video, audio, labels, replicas):
        """Float global batch of replicas * batch rows, kept on the device for step_replicas / eval_replicas."""
        v, a, l = _f32(video), _f32(audio), _f32(labels)
        self._replica_rows(replicas, v, a, l)
        check(self.lib.l3_replicas_upload(self.h, _ptr(v), _ptr(a), _ptr(l), int(replicas)), self.h)

    def replicas_upload_raw(self, video_u8, audio_i16, labels_i32, replicas):
        """The stored dtypes of a global batch; each slice is scaled by upload_batch_raw's kernels when its turn comes."""
        self._send_raw(self.lib.l3_replicas_upload_raw, video_u8, audio_i16, labels_i32, replicas=replicas)

    def replicas_stage_raw(self, video_u8, audio_i16, labels_i32, replicas):
        """Next global batch to the device while the current step runs; adopted by the next step_replicas / eval_replicas."""
        self._send_raw(self.lib.l3_replicas_stage_raw, video_u8, audio_i16, labels_i32, replicas=replicas)

    def replicas_upload_raw_aug(self, video_u8, audio_i16, labels_i32, params, u, replicas):
        self._send_raw(self.lib.l3_replicas_upload_raw_aug, video_u8, audio_i16, labels_i32, (params, u), replicas)

    def replicas_stage_raw_aug(self, video_u8, audio_i16, labels_i32, params, u, replicas):
        self._send_raw(self.lib.l3_replicas_stage_raw_aug, video_u8, audio_i16, labels_i32, (params, u), replicas)

    def step_replicas(self, lr):
        """One training step of the resident global batch, slice by slice: the replicas' gradients added in replica order, one
        moving-average update per replica, one Adam step.  step_results() / results_enqueue() then give the global batch's."""
        check(self.lib.l3_step_replicas(self.h, lr), self.h)

    def eval_replicas(self):
        """test_on_batch (inference-mode BatchNorm) of the resident global batch: (loss, acc)."""
        loss, acc = C.c_float(), C.c_float()
        check(self.lib.l3_eval_replicas(self.h, C.byref(loss), C.byref(acc)), self.h)
        return loss.value, acc.value

    def step_results(self, want_probs=False):
        loss, acc = C.c_float(), C.c_float()
        probs = np.empty((self.batch, 2), np.float32) if want_probs else None
        logits = np.empty((self.batch, 2), np.float32) if want_probs else None
        check(self.lib.l3_step_results(self.h, C.byref(loss), C.byref(acc), _ptr(probs), _ptr(logits)), self.h)
        if want_probs:
            return loss.value, acc.value, probs, logits
        return loss.value, acc.value

    def results_enqueue(self, slot, reduce=False):
        """Copies the loss / accuracy sums of the step just enqueued to pinned slot 0 / 1 behind it (no wait).  reduce: summed
        over the ranks of the engine's communicator first (every rank calls it)."""
        check(self.lib.l3_step_results_enqueue(self.h, int(slot), 1 if reduce else 0), self.h)

    def results_wait(self, slot):
        """(loss, acc) of the step whose results went to `slot`; waits for that copy only."""
        loss, acc = C.c_float(), C.c_float()
        check(self.lib.l3_step_results_wait(self.h, int(slot), C.byref(loss), C.byref(acc)), self.h)
        return loss.value, acc.value

    # -- data parallelism through the library's own RCCL communicator -----------------------------------------
    def comm_init(self, unique_id, world, rank):
        """ncclCommInitRank for this engine's GPU; `unique_id` = the 128 bytes rank 0 got from comm_unique_id()."""
        buf = C.create_string_buffer(bytes(unique_id), 128)
        check(self.lib.l3_comm_init(self.h, buf, int(world), int(rank)), self.h)

    def comm_destroy(self):
        check(self.lib.l3_comm_destroy(self.h), self.h)

    def comm_info(self):
        w, r = C.c_int(), C.c_int()
        path = C.create_string_buffer(512)
        check(self.lib.l3_comm_info(self.h, C.byref(w), C.byref(r), path, 512), self.h)
        return dict(world=w.value, rank=r.value, library=path.value.decode())

    def comm_allreduce(self, values, op='sum'):
        """Sum / max of a few host doubles over the ranks (synchronises: also a barrier)."""
        vals = (C.c_double * len(values))(*[float(v) for v in values])
        check(self.lib.l3_comm_allreduce_host(self.h, vals, len(values), {'sum': 0, 'max': 1}[op]), self.h)
        return list(vals)

    def comm_timing(self, on=True):
        """Measurement mode of step_dp (hipEvents around every bucket's all-reduce; every step is waited for)."""
        check(self.lib.l3_comm_timing(self.h, 1 if on else 0), self.h)

    def comm_timing_read(self):
        nb = self.bucket_count()
        ex, sp, st = C.c_double(), C.c_double(), C.c_int()
        bm = (C.c_double * nb)()
        check(self.lib.l3_comm_timing_read(self.h, C.byref(ex), C.byref(sp), bm, nb, C.byref(st)), self.h)
        return {'exposed_ms': ex.value, 'span_ms': sp.value, 'bucket_ms': [bm[i] for i in range(nb)], 'steps': st.value}

    def step_dp(self, lr):
        """One data-parallel training step on the resident batch (bucketed RCCL all-reduce inside the library)."""
        check(self.lib.l3_step_dp(self.h, lr), self.h)

    def grad_arena(self):
        p, n = C.c_void_p(), C.c_int64()
        check(self.lib.l3_grad_arena_dev(self.h, C.byref(p), C.byref(n)), self.h)
        return p.value, n.value

    def bn_stats_pack(self):
        """(device pointer, numel) of this rank's packed BatchNorm batch means / variances (after a training forward)."""
        p, n = C.c_void_p(), C.c_int64()
        check(self.lib.l3_bn_stats_pack_dev(self.h, C.byref(p), C.byref(n)), self.h)
        return p.value, n.value

    def bn_stats_replicas(self, world):
        """Device pointer of the (world, numel) buffer the gathered statistics go to; arms the next step_update."""
        p = C.c_void_p()
        check(self.lib.l3_bn_stats_replicas_dev(self.h, int(world), C.byref(p)), self.h)
        return p.value

    def bucket_range(self, b):
        o, n = C.c_int64(), C.c_int64()
        check(self.lib.l3_bucket_range(self.h, b, C.byref(o), C.byref(n)), self.h)
        return o.value, n.value

    # -- embeddings / taps -----------------------------------------------------------------
    def embed_audio(self, audio, pool):
        a = _f32(audio)
        d = self.lib.l3_embed_dim(self.h, 0, pool[0], pool[1])
        out = np.empty((a.shape[0], d), np.float32)
        check(self.lib.l3_embed_audio(self.h, _ptr(a), a.shape[0], pool[0], pool[1], _ptr(out)), self.h)
        return out

    def embed_audio_frames(self, samples, table, pool, out=None, dst=None, row0=0):
        """l3_embed_audio_frames: samples (n,) float32 (clips back to back), table (n_frames, 3) int64 {start, lo, hi}
        (features.frame_table) -> (n_frames, D) embeddings, written into `out` when given (C-contiguous float32).
        dst: a Features on the engine's device; the rows then stay there, in rows [row0, row0 + n_frames) of dst
        (l3_embed_audio_frames_dev), and dst is returned."""
        s = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
        t = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, 3)
        if dst is not None:
            if out is not None:
                raise ValueError('give out or dst, not both')
            if s.size == 0:
                s = np.zeros(1, np.float32)[:0]
            check(self.lib.l3_embed_audio_frames_dev(self.h, _ptr(s), s.size, _ptr(t), t.shape[0], pool[0], pool[1], dst.h,
                                                     int(row0)), self.h)
            return dst
        d = self.lib.l3_embed_dim(self.h, 0, pool[0], pool[1])
        if out is None:
            out = np.empty((t.shape[0], max(d, 0)), np.float32)
        elif out.dtype != np.float32 or not out.flags['C_CONTIGUOUS'] or out.shape != (t.shape[0], d):
            raise ValueError('out must be a C-contiguous float32 array of shape %s' % ((t.shape[0], d),))
        if s.size == 0:
            s = np.zeros(1, np.float32)[:0]
        check(self.lib.l3_embed_audio_frames(self.h, _ptr(s), s.size, _ptr(t), t.shape[0], pool[0], pool[1], _ptr(out)),
              self.h)
        return out

    def spectrogram_shape(self):
        """l3_spectrogram_shape: (F, frames) of the front-end's output, the spec model's input."""
        r, f = C.c_int64(), C.c_int64()
        check(self.lib.l3_spectrogram_shape(self.h, C.byref(r), C.byref(f)), self.h)
        return r.value, f.value

    def audio_spectrograms(self, samples, table):
        """l3_audio_spectrograms: samples and table as embed_audio_frames' -> (n_frames, F, frames) float32, the front-end's
        output of every frame (of the engine's form: 'minispec' the deployed pipeline's, 'kapre' the training-time one)."""
        s = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
        t = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, 3)
        if s.size == 0:
            s = np.zeros(1, np.float32)[:0]
        out = np.empty((t.shape[0],) + self.spectrogram_shape(), np.float32)
        check(self.lib.l3_audio_spectrograms(self.h, _ptr(s), s.size, _ptr(t), t.shape[0], _ptr(out)), self.h)
        return out

    def embed_audio_spec(self, spec, pool, out=None, dst=None, row0=0):
        """l3_embed_audio_spec: spec (n, F, frames) float32, the front-end's output -> (n, D) embeddings; the front-end does
        not run.  out, dst, row0: as embed_audio_frames' (l3_embed_audio_spec_dev)."""
        x = np.ascontiguousarray(spec, dtype=np.float32)
        shape = self.spectrogram_shape()
        if x.ndim == 4 and x.shape[3] == 1:
            x = x.reshape(x.shape[:3])
        if x.ndim != 3 or x.shape[1:] != shape:
            raise ValueError('spec must have shape (n, %d, %d) or (n, %d, %d, 1), not %s' % (shape + shape + (x.shape,)))
        n = x.shape[0]
        if dst is not None:
            if out is not None:
                raise ValueError('give out or dst, not both')
            check(self.lib.l3_embed_audio_spec_dev(self.h, _ptr(x), n, pool[0], pool[1], dst.h, int(row0)), self.h)
            return dst
        d = self.lib.l3_embed_dim(self.h, 0, pool[0], pool[1])
        if out is None:
            out = np.empty((n, max(d, 0)), np.float32)
        elif out.dtype != np.float32 or not out.flags['C_CONTIGUOUS'] or out.shape != (n, d):
            raise ValueError('out must be a C-contiguous float32 array of shape %s' % ((n, d),))
        check(self.lib.l3_embed_audio_spec(self.h, _ptr(x), n, pool[0], pool[1], _ptr(out)), self.h)
        return out

    def embed_audio_clips_resampled(self, native, clips, half_window, num_table, n_samples, table, pool, out=None, dst=None,
                                    row0=0):
        """l3_embed_audio_clips_resampled: native (n,) float32 (clips at their own rates back to back), clips (n_clips, 6) int64
        {x_off, L, sr_orig, t0, n_out, y_off}, half_window (n_window,) float64 with num_table entries per zero crossing,
        n_samples the 48 kHz buffer the rows fill, table (n_frames, 3) int64 {start, lo, hi} over it -> (n_frames, D)
        embeddings, written into `out` when given (C-contiguous float32).  dst, row0: as embed_audio_frames'
        (l3_embed_audio_clips_resampled_dev)."""
        x = np.ascontiguousarray(native, dtype=np.float32).reshape(-1)
        c = np.ascontiguousarray(clips, dtype=np.int64).reshape(-1, 6)
        w = np.ascontiguousarray(half_window, dtype=np.float64).reshape(-1)
        t = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, 3)
        if dst is not None:
            if out is not None:
                raise ValueError('give out or dst, not both')
            if x.size == 0:
                x = np.zeros(1, np.float32)[:0]
            check(self.lib.l3_embed_audio_clips_resampled_dev(self.h, _ptr(x), x.size, _ptr(c), c.shape[0], _ptr(w), w.size,
                                                              int(num_table), int(n_samples), _ptr(t), t.shape[0], pool[0],
                                                              pool[1], dst.h, int(row0)), self.h)
            return dst
        d = self.lib.l3_embed_dim(self.h, 0, pool[0], pool[1])
        if out is None:
            out = np.empty((t.shape[0], max(d, 0)), np.float32)
        elif out.dtype != np.float32 or not out.flags['C_CONTIGUOUS'] or out.shape != (t.shape[0], d):
            raise ValueError('out must be a C-contiguous float32 array of shape %s' % ((t.shape[0], d),))
        if x.size == 0:
            x = np.zeros(1, np.float32)[:0]
        check(self.lib.l3_embed_audio_clips_resampled(self.h, _ptr(x), x.size, _ptr(c), c.shape[0], _ptr(w), w.size,
                                                      int(num_table), int(n_samples), _ptr(t), t.shape[0], pool[0], pool[1],
                                                      _ptr(out)), self.h)
        return out

    def embed_vision(self, video, pool=(7, 7)):
        v = _f32(video)
        d = self.lib.l3_embed_dim(self.h, 1, pool[0], pool[1])
        out = np.empty((v.shape[0], d), np.float32)
        check(self.lib.l3_embed_vision(self.h, _ptr(v), v.shape[0], pool[0], pool[1], _ptr(out)), self.h)
        return out

    def embed_vision_frames(self, pixels, table, pool=(7, 7), out=None, dst=None, row0=0):
        """l3_embed_vision_frames: pixels (n_bytes,) uint8 (HWC frames back to back), table (n_frames, 7) int64
        {offset, H, W, Ho, Wo, y0, x0} (features.image_table) -> (n_frames, D) embeddings, written into `out` when given
        (C-contiguous float32).  dst, row0: as embed_audio_frames' (l3_embed_vision_frames_dev)."""
        p = np.ascontiguousarray(pixels, dtype=np.uint8).reshape(-1)
        t = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, 7)
        if p.size == 0:
            p = np.zeros(1, np.uint8)[:0]
        if dst is not None:
            if out is not None:
                raise ValueError('give out or dst, not both')
            check(self.lib.l3_embed_vision_frames_dev(self.h, _ptr(p), p.size, _ptr(t), t.shape[0], pool[0], pool[1], dst.h,
                                                      int(row0)), self.h)
            return dst
        d = self.lib.l3_embed_dim(self.h, 1, pool[0], pool[1])
        if out is None:
            out = np.empty((t.shape[0], max(d, 0)), np.float32)
        elif out.dtype != np.float32 or not out.flags['C_CONTIGUOUS'] or out.shape != (t.shape[0], d):
            raise ValueError('out must be a C-contiguous float32 array of shape %s' % ((t.shape[0], d),))
        check(self.lib.l3_embed_vision_frames(self.h, _ptr(p), p.size, _ptr(t), t.shape[0], pool[0], pool[1], _ptr(out)),
              self.h)
        return out

    def tower_dim(self, tower):
        """l3_tower_dim: the width of a tower's flattened output (0 = vision_model, 1 = audio_model)."""
        d = self.lib.l3_tower_dim(self.h, int(tower))
        if d < 0:
            raise ValueError('tower must be 0 (vision_model) or 1 (audio_model), not %r' % (tower,))
        return d

    def tower_features(self, tower, rows, out=None, dst=None, row0=0):
        """l3_tower_features: (n, 224, 224, 3) frames (tower 0) or (n, 1, 48000) waveforms (tower 1) -> the tower's flattened output
        (n, width) from that tower alone, inference-mode BatchNorm.  out, dst, row0: as embed_audio_frames'
        (l3_tower_features_dev)."""
        x = _f32(rows)
        n = x.shape[0]
        per = 224 * 224 * 3 if tower == 0 else 48000
        if x.size != n * per:
            raise ValueError('tower %d takes rows of %d values, not an array of shape %s' % (tower, per, x.shape))
        if dst is not None:
            if out is not None:
                raise ValueError('give out or dst, not both')
            check(self.lib.l3_tower_features_dev(self.h, int(tower), _ptr(x), n, dst.h, int(row0)), self.h)
            return dst
        d = self.tower_dim(tower)
        if out is None:
            out = np.empty((n, d), np.float32)
        elif out.dtype != np.float32 or not out.flags['C_CONTIGUOUS'] or out.shape != (n, d):
            raise ValueError('out must be a C-contiguous float32 array of shape %s' % ((n, d),))
        check(self.lib.l3_tower_features(self.h, int(tower), _ptr(x), n, _ptr(out)), self.h)
        return out

    def tower_features_sampled(self, bank, records, vis=None, aud=None, row0=0):
        """l3_tower_features_sampled_dev: both towers' outputs of the (frame, second) of every record (SAMPLE_RECORD rows, not
        augmented) of a ClipBank, into rows [row0, row0 + n) of the Features vis and aud (either may be None).  Replaces the
        engine's resident batch."""
        r = sample_records(records)
        if vis is None and aud is None:
            raise ValueError('give vis, aud or both')
        check(self.lib.l3_tower_features_sampled_dev(self.h, bank.h, _ptr(r), len(r), None if vis is None else vis.h,
                                                     None if aud is None else aud.h, int(row0)), self.h)

    def tower_locations_shape(self, tower):
        """l3_tower_locations_shape: (H, W, C) of the input of the tower's last pool -- the locations of its last feature map.
        ValueError for a tower whose last pool does not reduce to 1 x 1 (tiny_L3's vision tower)."""
        if tower not in (0, 1):
            raise ValueError('tower must be 0 (vision_model) or 1 (audio_model), not %r' % (tower,))
        h, w, c = C.c_int(), C.c_int(), C.c_int()
        try:
            check(self.lib.l3_tower_locations_shape(self.h, int(tower), C.byref(h), C.byref(w), C.byref(c)), self.h)
        except L3Error as err:
            raise ValueError(str(err))
        return h.value, w.value, c.value

    def tower_locations(self, tower, rows, dst=None, row0=0):
        """l3_tower_locations_dev: (n, 224, 224, 3) frames (tower 0) or (n, 1, 48000) waveforms (tower 1) -> the tower's last feature
        map before its global max pool, one row of C channels per location: rows [(row0 + i) L, (row0 + i + 1) L) of the Features
        dst (C columns) are item i's L = H W locations, y first.  dst None: a new Features of n L rows.  Returns dst."""
        H, W, Cc = self.tower_locations_shape(tower)
        x = _f32(rows)
        n = x.shape[0]
        per = 224 * 224 * 3 if tower == 0 else 48000
        if x.size != n * per:
            raise ValueError('tower %d takes rows of %d values, not an array of shape %s' % (tower, per, x.shape))
        if dst is None:
            if row0:
                raise ValueError('row0 goes with dst')
            dst = Features.alloc(max(n, 1) * H * W, Cc, device=self.device)
        check(self.lib.l3_tower_locations_dev(self.h, int(tower), _ptr(x), n, dst.h, int(row0)), self.h)
        return dst

    def tower_locations_sampled(self, bank, records, tower, loc, pooled=None, row0=0):
        """l3_tower_locations_sampled_dev: tower_locations of the frame (tower 0) or second (tower 1) of every record of a ClipBank
        into the Features loc from item row0; pooled (or None) receives the tower's pooled rows of the same run from row row0.
        Replaces the engine's resident batch."""
        if tower not in (0, 1):
            raise ValueError('tower must be 0 (vision_model) or 1 (audio_model), not %r' % (tower,))
        if loc is None:
            raise ValueError('loc must not be None')
        r = sample_records(records)
        check(self.lib.l3_tower_locations_sampled_dev(self.h, bank.h, _ptr(r), len(r), int(tower), None if pooled is None else pooled.h,
                                                      loc.h, int(row0)), self.h)
        return loc

    def activation(self, name):
        n = C.c_int64()
        check(self.lib.l3_activation_numel(self.h, name.encode(), C.byref(n)), self.h)
        out = np.empty((n.value,), np.float32)
        check(self.lib.l3_get_activation(self.h, name.encode(), _ptr(out), n.value), self.h)
        return out

    def sync(self):
        check(self.lib.l3_sync(self.h), self.h)

    def set_tower_overlap(self, on=True):
        """Audio tower on the internal side stream beside the vision tower (default) or serialised."""
        check(self.lib.l3_set_tower_overlap(self.h, int(on)), self.h)

    def profile_enable(self, on=True):
        check(self.lib.l3_profile_enable(self.h, int(on)), self.h)

    def profile_read(self):
        out = {}
        for i, fam in enumerate(FAMILIES):
            ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
            check(self.lib.l3_profile_read(self.h, i, C.byref(ms), C.byref(n), C.byref(fl)), self.h)
            ex = C.c_double()
            check(self.lib.l3_profile_read_executed(self.h, i, C.byref(ex)), self.h)
            by = C.c_double()
            check(self.lib.l3_profile_read_bytes(self.h, i, C.byref(by)), self.h)
            out[fam] = dict(ms=ms.value, launches=n.value, flops=fl.value, executed_flops=ex.value, alg_bytes=by.value)
        return out


# -- stand-alone operators (op-level parity tests) ------------------------------------------
def op_conv2d_fwd(x, w, b, same, device=0, dtype='f32'):
    lib = load()
    x, w = _f32(x), _f32(w)
    b = _f32(b)
    n, h, wd, cin = x.shape
    kh, kw, _, cout = w.shape
    ho, wo = (h, wd) if same else (h - kh + 1, wd - kw + 1)
    y = np.empty((n, ho, wo, cout), np.float32)
    if OP_DTYPES[dtype]:
        check(lib.l3_op_conv2d_fwd_dt(device, OP_DTYPES[dtype], _ptr(x), _ptr(w), _ptr(b), _ptr(y), n, h, wd, cin, cout,
                                      kh, kw, int(same)))
    else:
        check(lib.l3_op_conv2d_fwd(device, _ptr(x), _ptr(w), _ptr(b), _ptr(y), n, h, wd, cin, cout, kh, kw, int(same)))
    return y


def op_conv2d_bwd(x, w, dy, same, device=0, dtype='f32'):
    lib = load()
    x, w, dy = _f32(x), _f32(w), _f32(dy)
    n, h, wd, cin = x.shape
    kh, kw, _, cout = w.shape
    dx, dw, db = np.empty_like(x), np.empty_like(w), np.empty((cout,), np.float32)
    if OP_DTYPES[dtype]:
        check(lib.l3_op_conv2d_bwd_dt(device, OP_DTYPES[dtype], _ptr(x), _ptr(w), _ptr(dy), _ptr(dx), _ptr(dw), _ptr(db),
                                      n, h, wd, cin, cout, kh, kw, int(same)))
    else:
        check(lib.l3_op_conv2d_bwd(device, _ptr(x), _ptr(w), _ptr(dy), _ptr(dx), _ptr(dw), _ptr(db),
                                   n, h, wd, cin, cout, kh, kw, int(same)))
    return dx, dw, db


def op_conv2d_fwd_stats(x, w, b, same, stat_mode, dtype='f32', device=0):
    """The convolution of op_conv2d_fwd with its epilogue's BatchNorm statistics: y, partials (nblk, 2, Cout) about the pivot b
    (relu(b) when stat_mode == 2: moments of relu(y)), and the batch mean / biased variance the engine's second stage makes of them."""
    lib = load()
    x, w, b = _f32(x), _f32(w), _f32(b)
    n, h, wd, cin = x.shape
    kh, kw, _, cout = w.shape
    ho, wo = (h, wd) if same else (h - kh + 1, wd - kw + 1)
    dims = (n, h, wd, cin, cout, kh, kw, int(same), int(stat_mode))
    nblk = C.c_int(0)
    check(lib.l3_op_conv2d_fwd_stats(device, OP_DTYPES[dtype], None, None, None, None, None, C.byref(nblk), None, None, *dims))
    y = np.empty((n, ho, wo, cout), np.float32)
    part = np.empty((nblk.value, 2, cout), np.float32)
    mean, var = np.empty(cout, np.float32), np.empty(cout, np.float32)
    check(lib.l3_op_conv2d_fwd_stats(device, OP_DTYPES[dtype], _ptr(x), _ptr(w), _ptr(b), _ptr(y), _ptr(part), C.byref(nblk),
                                     _ptr(mean), _ptr(var), *dims))
    assert nblk.value == part.shape[0]
    return y, part, mean, var


def op_conv2d_stat_blocks(shape, cout, dtype='f32', same=True, kh=3, kw=3):
    """The library's own count of statistics blocks (patches, flat tiles or tile blocks) of the forward launch op_conv2d_fwd makes for
    an x of `shape` (N, H, W, Cin): the query form of op_conv2d_fwd_stats alone -- nothing is uploaded or launched."""
    lib = load()
    n, h, wd, cin = shape
    nblk = C.c_int(0)
    check(lib.l3_op_conv2d_fwd_stats(0, OP_DTYPES[dtype], None, None, None, None, None, C.byref(nblk), None, None,
                                     n, h, wd, cin, cout, kh, kw, int(same), 1))
    return nblk.value


def op_conv2d_dgrad_bn_bwd(dy, w, same, bn_x, gamma, beta, mean, var, relu, bn_rows=None, dtype='f32', device=0):
    """The data gradient of the convolution with filter w (KH, KW, Cin, Cout) from dy (N, Ho, Wo, Cout), with the backward reduction
    of the BatchNorm(+ReLU) in front of the convolution -- input bn_x (N, H, W, Cin), moments over bn_rows rows (default: bn_x's) --
    in its epilogue: dx, partials (nblk, 2, Cin) of [mask * dx, mask * dx * x_hat], dgamma, dbeta."""
    lib = load()
    dy, w, bn_x = _f32(dy), _f32(w), _f32(bn_x)
    n, h, wd, cin = bn_x.shape
    kh, kw, wci, cout = w.shape
    ho, wo = (h, wd) if same else (h - kh + 1, wd - kw + 1)
    assert wci == cin and dy.shape == (n, ho, wo, cout)
    rows = int(bn_rows) if bn_rows is not None else n * h * wd
    dims = (n, h, wd, cin, cout, kh, kw, int(same), int(relu), rows)
    nblk = C.c_int(0)
    check(lib.l3_op_conv2d_dgrad_bn_bwd(device, OP_DTYPES[dtype], *([None] * 9), C.byref(nblk), None, None, *dims))
    dx = np.empty_like(bn_x)
    part = np.empty((nblk.value, 2, cin), np.float32)
    dg, db = np.empty(cin, np.float32), np.empty(cin, np.float32)
    vecs = [_f32(v) for v in (gamma, beta, mean, var)]
    assert all(v.shape == (cin,) for v in vecs)
    check(lib.l3_op_conv2d_dgrad_bn_bwd(device, OP_DTYPES[dtype], _ptr(dy), _ptr(w), _ptr(bn_x), *[_ptr(v) for v in vecs], _ptr(dx),
                                        _ptr(part), C.byref(nblk), _ptr(dg), _ptr(db), *dims))
    return dx, part, dg, db


FIRST_BLOCK_FORMS = dict(explicit=0, deferred=1, deferred_bf16=2)


def op_first_block_bwd(x, gamma_in, beta_in, w, y, gamma2, beta2, dA, relu, form, device=0):
    """The backward of a tower's first block as the engine runs it (include/l3hip.h l3_op_first_block_bwd), every stage's result in
    a dict: mean_in, var_in, xaug, mean2, var2, scale2, shift2, dgamma2, dbeta2, cA / cB / cC (deferred forms) or dY ('explicit'),
    gaug, dw, dbias, dgamma_in, dbeta_in.  form 'deferred_bf16': y and dA are stored as bfloat16 on the device."""
    lib = load()
    x, w, y, dA = _f32(x), _f32(w), _f32(y), _f32(dA)
    n, h, wd, c = x.shape
    co = w.shape[3]
    assert w.shape == (3, 3, c, co) and y.shape == (n, h, wd, co) and dA.shape == y.shape
    vin = [_f32(v) for v in (gamma_in, beta_in)]
    v2 = [_f32(v) for v in (gamma2, beta2)]
    assert all(v.shape == (c,) for v in vin) and all(v.shape == (co,) for v in v2)
    f32 = np.float32
    out = dict(mean_in=np.empty(c, f32), var_in=np.empty(c, f32), xaug=np.empty((n, h, wd, c + 1), f32))
    for k in ('mean2', 'var2', 'scale2', 'shift2', 'dgamma2', 'dbeta2'):
        out[k] = np.empty(co, f32)
    coeffs = np.empty((3, co), f32) if form != 'explicit' else None
    dY = np.empty_like(y) if form == 'explicit' else None
    out.update(gaug=np.empty((9, c + 1, co), f32), dw=np.empty((3, 3, c, co), f32), dbias=np.empty(co, f32),
               dgamma_in=np.empty(c, f32), dbeta_in=np.empty(c, f32))
    names = ('mean_in', 'var_in', 'xaug', 'mean2', 'var2', 'scale2', 'shift2', 'dgamma2', 'dbeta2')
    tail = ('gaug', 'dw', 'dbias', 'dgamma_in', 'dbeta_in')
    check(lib.l3_op_first_block_bwd(device, FIRST_BLOCK_FORMS[form], int(relu), _ptr(x), _ptr(vin[0]), _ptr(vin[1]), _ptr(w), _ptr(y),
                                    _ptr(v2[0]), _ptr(v2[1]), _ptr(dA), *([_ptr(out[k]) for k in names] + [_ptr(coeffs), _ptr(dY)] +
                                                                          [_ptr(out[k]) for k in tail] + [n, h, wd, c, co])))
    if dY is not None:
        out['dY'] = dY
    else:
        out['cA'], out['cB'], out['cC'] = coeffs
    return out


def op_first_conv_grads(gaug, w, gamma, beta, want_dbias=True, device=0):
    """first_conv_grads alone: gaug (taps, C + 1, Co), w (taps, C, Co), gamma, beta (C) -> dw, dgamma, dbeta, dbias (None unless
    want_dbias)."""
    lib = load()
    gaug, w, gamma, beta = _f32(gaug), _f32(w), _f32(gamma), _f32(beta)
    taps, c, co = w.shape
    assert gaug.shape == (taps, c + 1, co) and gamma.shape == (c,) and beta.shape == (c,)
    dw = np.empty_like(w)
    dg, db = np.empty(c, np.float32), np.empty(c, np.float32)
    dbias = np.empty(co, np.float32) if want_dbias else None
    check(lib.l3_op_first_conv_grads(device, _ptr(gaug), _ptr(w), _ptr(gamma), _ptr(beta), _ptr(dw), _ptr(dg), _ptr(db), _ptr(dbias),
                                     taps, c, co))
    return dw, dg, db, dbias


def op_bn_relu_fwd(x, gamma, beta, relu, device=0, x_bf16=False, out_bf16=False):
    """out_bf16 (the BatchNorm operators): the tensor output -- y, the pooled p, dx -- is stored as bfloat16 on the device (bit 2 of
    the x_bf16 flag word) and returned widened."""
    lib = load()
    x = _f32(x)
    c = x.shape[-1]
    rows = x.size // c
    y = np.empty_like(x)
    mean, var = np.empty((c,), np.float32), np.empty((c,), np.float32)
    check(lib.l3_op_bn_relu_fwd(device, _ptr(x), _ptr(_f32(gamma)), _ptr(_f32(beta)), _ptr(y), _ptr(mean),
                                _ptr(var), rows, c, int(relu), int(x_bf16) | (4 if out_bf16 else 0)))
    return y, mean, var


def op_bn_relu_bwd(x, y, dy, gamma, mean, var, relu, device=0, beta=None, x_bf16=False, out_bf16=False):
    lib = load()
    x, y, dy = _f32(x), _f32(y), _f32(dy)
    c = x.shape[-1]
    rows = x.size // c
    dx = np.empty_like(x)
    dg, db = np.empty((c,), np.float32), np.empty((c,), np.float32)
    check(lib.l3_op_bn_relu_bwd(device, _ptr(x), _ptr(y), _ptr(dy), _ptr(_f32(gamma)), _ptr(_f32(beta)), _ptr(_f32(mean)),
                                _ptr(_f32(var)), _ptr(dx), _ptr(dg), _ptr(db), rows, c, int(relu), int(x_bf16) | (4 if out_bf16 else 0)))
    return dx, dg, db


def op_bn_relu_pool2_fwd(x, gamma, beta, same, device=0, relu_mode=1, x_bf16=False, want_xwin=False, out_bf16=False):
    """want_xwin: as a training forward runs it -- also returns the window winners (p's shape; widened when x_bf16)."""
    lib = load()
    flags = int(x_bf16) | (4 if out_bf16 else 0)
    x = _f32(x)
    n, h, wd, c = x.shape
    p = np.empty((n, _pool_out(h, 2, 2, same), _pool_out(wd, 2, 2, same), c), np.float32)
    mean, var = np.empty((c,), np.float32), np.empty((c,), np.float32)
    if want_xwin:
        xwin = np.empty_like(p)
        check(lib.l3_op_bn_relu_pool2_fwd_xwin(device, _ptr(x), _ptr(_f32(gamma)), _ptr(_f32(beta)), _ptr(p), _ptr(mean), _ptr(var),
                                               _ptr(xwin), n, h, wd, c, int(same), int(relu_mode), flags))
        return p, mean, var, xwin
    check(lib.l3_op_bn_relu_pool2_fwd(device, _ptr(x), _ptr(_f32(gamma)), _ptr(_f32(beta)), _ptr(p), _ptr(mean),
                                      _ptr(var), n, h, wd, c, int(same), int(relu_mode), flags))
    return p, mean, var


def op_bn_relu_pool2_bwd(x, gamma, beta, dp, same, device=0, relu_mode=1, x_bf16=False, out_bf16=False):
    lib = load()
    x, dp = _f32(x), _f32(dp)
    n, h, wd, c = x.shape
    dx = np.empty_like(x)
    dg, db, dbias = (np.empty((c,), np.float32) for _ in range(3))
    check(lib.l3_op_bn_relu_pool2_bwd(device, _ptr(x), _ptr(_f32(gamma)), _ptr(_f32(beta)), _ptr(dp), _ptr(dx),
                                      _ptr(dg), _ptr(db), _ptr(dbias), n, h, wd, c, int(same), int(relu_mode), int(x_bf16) | (4 if out_bf16 else 0)))
    return dx, dg, db, dbias


def _pool_out(h, p, s, same):
    return -(-h // s) if same else (h - p) // s + 1


def op_maxpool_fwd(x, ph, pw, sh, sw, same, device=0):
    lib = load()
    x = _f32(x)
    n, h, wd, c = x.shape
    y = np.empty((n, _pool_out(h, ph, sh, same), _pool_out(wd, pw, sw, same), c), np.float32)
    check(lib.l3_op_maxpool_fwd(device, _ptr(x), _ptr(y), n, h, wd, c, ph, pw, sh, sw, int(same)))
    return y


def op_maxpool_bwd(x, dy, ph, pw, sh, sw, same, device=0):
    lib = load()
    x, dy = _f32(x), _f32(dy)
    n, h, wd, c = x.shape
    dx = np.empty_like(x)
    check(lib.l3_op_maxpool_bwd(device, _ptr(x), _ptr(dy), _ptr(dx), n, h, wd, c, ph, pw, sh, sw, int(same)))
    return dx


def op_bn_stats_from_partials(part, pivot, rows, eps=1e-3, device=0):
    """part: (nblk, 2, C) partial [sum, sum of squares] about pivot (C,) -> batch mean, biased variance (C,)."""
    lib = load()
    part, pivot = _f32(part), _f32(pivot)
    nblk, two, c = part.shape
    assert two == 2 and pivot.shape == (c,)
    mean, var = np.empty(c, np.float32), np.empty(c, np.float32)
    check(lib.l3_op_bn_stats_from_partials(device, _ptr(part), nblk, c, _ptr(pivot), int(rows), float(eps), _ptr(mean), _ptr(var)))
    return mean, var


def op_frontend(model_type, audio, db_max_scope='sample', device=0):
    lib = load()
    a = _f32(audio)
    n = a.shape[0]
    probe = {'cnn_L3_orig': (257, 197), 'tiny_L3': (257, 198), 'cnn_L3_kapredbinputbn': (257, 197),
             'cnn_L3_melspec1': (128, 199), 'cnn_L3_melspec2': (256, 199)}[model_type]
    out = np.empty((n, probe[0], probe[1], 1), np.float32)
    check(lib.l3_op_frontend(device, MODEL_IDS[model_type], _ptr(a), n, 0 if db_max_scope == 'sample' else 1, _ptr(out)))
    return out


def op_frontend_form(model_type, audio, frontend='minispec', device=0):
    """l3_op_frontend_form: the front-end of the given form on audio (n, 48000) -> (n, F, frames, 1), per-sample maximum."""
    lib = load()
    a = _f32(audio)
    n = a.shape[0]
    f, frames = {'cnn_L3_orig': (257, 197), 'tiny_L3': (257, 198), 'cnn_L3_kapredbinputbn': (257, 197),
                 'cnn_L3_melspec1': (128, 199), 'cnn_L3_melspec2': (256, 199)}[model_type]
    if frontend == 'minispec':
        frames = 199
    out = np.empty((n, f, frames, 1), np.float32)
    check(lib.l3_op_frontend_form(device, MODEL_IDS[model_type], FRONTENDS[frontend], _ptr(a), n, _ptr(out)))
    return out


FRONTEND_CFG_FIELDS = ('n_frames', 'pad_left', 'n_freq', 'ncols_pad', 'ke', 'ko', 'nc', 'N1', 'N2')
SPEC_LAYOUTS = dict(unfolded=0, folded=1, factored=2)


def frontend_cfg(t, n_dft, n_hop, same, n_mels=0):
    """The front-end geometry the engine derives for t samples (include/l3hip.h l3_frontend_cfg; host only): a dict of
    FRONTEND_CFG_FIELDS."""
    v = np.zeros(len(FRONTEND_CFG_FIELDS), np.int32)
    check(load().l3_frontend_cfg(int(t), int(n_dft), int(n_hop), int(bool(same)), int(n_mels), _ptr(v)))
    return dict(zip(FRONTEND_CFG_FIELDS, (int(x) for x in v)))


def frontend_tables(n_mels=0, freq2mel=None):
    """The tables of the 2048-point front-end as an engine uploads them (l3_frontend_tables; host only): dict of win (2048),
    b1 (32, 64), b2 (128, 64), tw (64, 32, 2) and, n_mels > 0, mel_start / mel_len / mel_off (n_mels) and melw, the packed bands of
    freq2mel (1025, n_mels), None = the stock bank."""
    f32 = np.float32
    out = dict(win=np.empty(2048, f32), b1=np.empty((32, 64), f32), b2=np.empty((128, 64), f32), tw=np.empty((64, 32, 2), f32))
    fb = _f32(freq2mel)
    assert fb is None or fb.shape == (1025, n_mels)
    st, ln, of = (np.zeros(n_mels, np.int32) for _ in range(3))
    cap = 1025 * max(n_mels, 1)
    melw = np.empty(cap, f32)
    n = C.c_int64(0)
    check(load().l3_frontend_tables(_ptr(fb), int(n_mels), _ptr(out['win']), _ptr(out['b1']), _ptr(out['b2']), _ptr(out['tw']), _ptr(st),
                                    _ptr(ln), _ptr(of), _ptr(melw), cap, C.byref(n)))
    if n_mels:
        out.update(mel_start=st, mel_len=ln, mel_off=of, melw=melw[:n.value].copy())
    return out


def op_frontend_frames(audio, n_dft, n_hop, pad_left, n_frames, device=0):
    """frame_audio, frame_audio_folded and (n_dft = 2048) dft_pack_frames on audio (B, T): frames (B, n_frames, n_dft), fe
    (B, n_frames, ke), fo (B, n_frames, ko), a1 (B, n_frames, 64, 32) or None."""
    a = _f32(audio)
    b, t = a.shape
    cfg = frontend_cfg(max(t, n_dft), n_dft, n_hop, False)
    f32 = np.float32
    frames, fe, fo = (np.empty((b, n_frames, w), f32) for w in (n_dft, cfg['ke'], cfg['ko']))
    a1 = np.empty((b, n_frames, 64, 32), f32) if n_dft == 2048 else None
    check(load().l3_op_frontend_frames(device, _ptr(a), b, t, int(n_dft), int(n_hop), int(pad_left), int(n_frames), _ptr(frames), _ptr(fe),
                                       _ptr(fo), _ptr(a1)))
    return frames, fe, fo, a1


def op_dft_twiddle(y, device=0):
    """dft_twiddle on y (frames, 64, 64) = [re k1 | im k1] per n2: a2 (frames, 32, 128) = [re n2 | im n2] per k1, nyq (frames)."""
    y = _f32(y)
    frames = y.shape[0]
    assert y.shape == (frames, 64, 64)
    a2, nyq = np.empty((frames, 32, 128), np.float32), np.empty(frames, np.float32)
    check(load().l3_op_dft_twiddle(device, _ptr(y), frames, _ptr(a2), _ptr(nyq)))
    return a2, nyq


def _frontend_flags(sqrt_out, db, loglambda):
    return int(bool(sqrt_out)) | int(bool(db)) << 1 | int(bool(loglambda)) << 2


def op_spec_to_features(layout, spec, b, n_frames, n_dft, n_mels=0, freq2mel=None, nyq=None, sqrt_out=False, db=False, loglambda=False,
                        device=0):
    """spec_to_features on a caller's transform in layout 'unfolded' (rows, ncols_pad), 'folded' (2 rows, nc) or 'factored'
    (rows, 32, 64) with nyq (rows); rows = b n_frames: (b, n_mels or n_freq, n_frames)."""
    spec, nyq, fb = _f32(spec), _f32(nyq), _f32(freq2mel)
    rows, nb = b * n_frames, n_dft // 2 + 1
    cfg = frontend_cfg(n_dft, n_dft, 1, False)
    want = {'unfolded': rows * cfg['ncols_pad'], 'folded': 2 * rows * cfg['nc'], 'factored': rows * n_dft}[layout]
    assert spec.size == want and (nyq is None or nyq.size == rows) and (fb is None or fb.shape == (nb, n_mels))
    out = np.empty((b, n_mels or nb, n_frames), np.float32)
    check(load().l3_op_spec_to_features(device, SPEC_LAYOUTS[layout], _ptr(spec), _ptr(nyq), b, n_frames, n_dft, n_mels, _ptr(fb),
                                        _frontend_flags(sqrt_out, db, loglambda), _ptr(out)))
    return out


def op_dft_fused(audio, n_hop, pad_left, n_frames, n_mels, freq2mel=None, sqrt_out=False, db=False, loglambda=False, device=0):
    """dft_fused on audio (B, T): (B, n_mels, n_frames), before db_normalize.  freq2mel (1025, n_mels), None = the stock bank."""
    a, fb = _f32(audio), _f32(freq2mel)
    b, t = a.shape
    assert fb is None or fb.shape == (1025, n_mels)
    out = np.empty((b, n_mels, n_frames), np.float32)
    check(load().l3_op_dft_fused(device, _ptr(a), b, t, int(n_hop), int(pad_left), int(n_frames), int(n_mels), _ptr(fb),
                                 _frontend_flags(sqrt_out, db, loglambda), _ptr(out)))
    return out


def op_db_normalize(x, scope='sample', device=0):
    """db_normalize on a copy of x (B, per_sample): x - max (per sample, or scope 'batch' of everything), clamped at -80."""
    x = np.array(x, dtype=np.float32, order='C')
    b, per = x.shape
    check(load().l3_op_db_normalize(device, _ptr(x), b, per, 0 if scope == 'sample' else 1))
    return x


def op_gather_frames(samples, table, device=0):
    """l3_op_gather_frames: the (n_frames, 48000) frames l3_embed_audio_frames feeds the front-end."""
    lib = load()
    s = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
    t = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, 3)
    if s.size == 0:
        s = np.zeros(1, np.float32)[:0]
    out = np.empty((t.shape[0], 48000), np.float32)
    check(lib.l3_op_gather_frames(device, _ptr(s), s.size, _ptr(t), t.shape[0], _ptr(out)))
    return out


def op_image_frames(pixels, table, device=0, want_u8=True, want_f32=True):
    """l3_op_image_frames: (u8, f32), each (n_frames, 224, 224, 3) -- the resized and cropped uint8 frames and the input rows
    l3_embed_vision_frames feeds the vision tower (None for an output not asked for)."""
    lib = load()
    p = np.ascontiguousarray(pixels, dtype=np.uint8).reshape(-1)
    t = np.ascontiguousarray(table, dtype=np.int64).reshape(-1, 7)
    if p.size == 0:
        p = np.zeros(1, np.uint8)[:0]
    u8 = np.empty((t.shape[0], 224, 224, 3), np.uint8) if want_u8 else None
    f32 = np.empty((t.shape[0], 224, 224, 3), np.float32) if want_f32 else None
    check(lib.l3_op_image_frames(device, _ptr(p), p.size, _ptr(t), t.shape[0], _ptr(u8), _ptr(f32)))
    return u8, f32


def op_resample(x, sr_orig, sr_new, half_window, num_table, t0=0, n_out=None, device=0):
    """l3_op_resample: outputs [t0, t0 + n_out) of resampy.resample(x, sr_orig, sr_new) with the given half window (float32);
    n_out defaults to the rest of the output."""
    lib = load()
    a = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    w = np.ascontiguousarray(half_window, dtype=np.float64).reshape(-1)
    if n_out is None:
        n_out = max(0, int(a.size * (float(sr_new) / sr_orig)) - int(t0)) if sr_orig > 0 else 0
    out = np.empty(max(int(n_out), 0), np.float32)
    check(lib.l3_op_resample(device, _ptr(a), a.size, int(sr_orig), int(sr_new), _ptr(w), w.size, int(num_table), int(t0),
                             int(n_out), _ptr(out)))
    return out


def op_resample_clips(x, clips, sr_new, half_window, num_table, n_samples, copy_equal=False, device=0):
    """l3_op_resample_clips: one launch over clip rows (n_clips, 6) int64 {x_off, L, sr_orig, t0, n_out, y_off} of x into a
    buffer of n_samples float32 (zero where no row writes)."""
    lib = load()
    a = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    c = np.ascontiguousarray(clips, dtype=np.int64).reshape(-1, 6)
    w = np.ascontiguousarray(half_window, dtype=np.float64).reshape(-1)
    out = np.empty(int(n_samples), np.float32)
    check(lib.l3_op_resample_clips(device, _ptr(a), a.size, _ptr(c), c.shape[0], int(sr_new), _ptr(w), w.size, int(num_table),
                                   int(n_samples), 1 if copy_equal else 0, _ptr(out)))
    return out


def op_preprocess(video_u8=None, audio_i16=None, device=0):
    lib = load()
    v = None if video_u8 is None else np.ascontiguousarray(video_u8, dtype=np.uint8)
    a = None if audio_i16 is None else np.ascontiguousarray(audio_i16, dtype=np.int16)
    vo = None if v is None else np.empty(v.shape, np.float32)
    ao = None if a is None else np.empty(a.shape, np.float32)
    check(lib.l3_op_preprocess(device, _ptr(v), 0 if v is None else v.size, _ptr(vo),
                               _ptr(a), 0 if a is None else a.size, _ptr(ao)))
    return vo, ao


# l3_augment_params of include/l3hip.h
AUGMENT_RECORD = np.dtype([('start_x', np.int32), ('start_y', np.int32), ('flip', np.int32), ('sat_first', np.int32),
                           ('saturation', np.float32), ('brightness', np.float32)])


def augment_records(params):
    """The fields of l3_augment_params out of any structured array that has them, packed as the library reads them."""
    params = np.asarray(params)
    rec = np.empty(params.shape, AUGMENT_RECORD)
    for name in AUGMENT_RECORD.names:
        rec[name] = params[name]
    return rec


def op_augment_video(video_u8, params, out='u8', device=0):
    """(N, H, W, 3) uint8 frames -> (N, 224, 224, 3) augmented: out = 'u8' the stored byte, 'f32' the engine's float, 'both'."""
    lib = load()
    v = np.ascontiguousarray(video_u8, dtype=np.uint8)
    if v.ndim != 4 or v.shape[3] != 3:
        raise ValueError('frames must be (N, H, W, 3), got %r' % (v.shape,))
    p = augment_records(params)
    if p.shape != (v.shape[0],):
        raise ValueError('%d frames but %r augmentation records' % (v.shape[0], p.shape))
    n, h, w = v.shape[:3]
    o8 = np.empty((n, 224, 224, 3), np.uint8) if out in ('u8', 'both') else None
    of = np.empty((n, 224, 224, 3), np.float32) if out in ('f32', 'both') else None
    if o8 is None and of is None:
        raise ValueError("out must be 'u8', 'f32' or 'both'")
    check(lib.l3_op_augment_video(device, _ptr(v), n, h, w, _ptr(p), _ptr(o8), _ptr(of)))
    return (o8, of) if out == 'both' else (o8 if of is None else of)


def op_augment_audio(audio_i16, u, out='i16', device=0):
    """(N, T) int16 rows and the draws u (N,) -> (augmented rows, gains): out = 'i16', 'f32' or 'both'."""
    lib = load()
    a = np.ascontiguousarray(audio_i16, dtype=np.int16)
    g = np.ascontiguousarray(u, dtype=np.float64)
    if a.ndim != 2 or g.shape != (a.shape[0],):
        raise ValueError('rows must be (N, T) with one draw each, got %r and %r' % (a.shape, g.shape))
    oi = np.empty(a.shape, np.int16) if out in ('i16', 'both') else None
    of = np.empty(a.shape, np.float32) if out in ('f32', 'both') else None
    if oi is None and of is None:
        raise ValueError("out must be 'i16', 'f32' or 'both'")
    gains = np.empty(a.shape[0], np.float64)
    check(lib.l3_op_augment_audio(device, _ptr(a), a.shape[0], a.shape[1], _ptr(g), _ptr(oi), _ptr(of), _ptr(gains)))
    return ((oi, of) if out == 'both' else (oi if of is None else of)), gains


# l3_sample of include/l3hip.h: one sample of generate_sample (data/avc/sample.py:319-387) after its draws
SAMPLE_RECORD = np.dtype({'names': ['video_clip', 'frame', 'audio_clip', 'audio_start', 'label', 'u_gain', 'start_x', 'start_y',
                                    'flip', 'sat_first', 'saturation', 'brightness'],
                          'formats': [np.int32] * 5 + [np.float64] + [np.int32] * 4 + [np.float32] * 2,
                          'offsets': [0, 4, 8, 12, 16, 24, 32, 36, 40, 44, 48, 52], 'itemsize': 56})


def sample_records(records):
    """Any structured array with the fields of l3_sample, packed as the library reads them."""
    records = np.asarray(records)
    if records.dtype == SAMPLE_RECORD and records.flags['C_CONTIGUOUS']:
        return records
    rec = np.zeros(records.shape, SAMPLE_RECORD)
    for name in SAMPLE_RECORD.names:
        rec[name] = records[name]
    return rec


class ClipBank(object):
    """Thin RAII wrapper over an l3_clipbank handle: decoded clips resident on the device (csrc/avsample.hip)."""

    def __init__(self, device, pixel_bytes, audio_samples, resize):
        self.lib = load()
        h = C.c_void_p()
        check(self.lib.l3_clipbank_create(int(device), int(pixel_bytes), int(audio_samples), int(resize or 0), C.byref(h)))
        self.h = h
        self.device = int(device)

    def close(self):
        if getattr(self, 'h', None):
            self.lib.l3_clipbank_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add(self, frames_u8, audio_i16):
        """(T, H, W, 3) uint8 and (n, C) int16 -> the clip's id."""
        f, a = np.ascontiguousarray(frames_u8, dtype=np.uint8), np.ascontiguousarray(audio_i16, dtype=np.int16)
        if f.ndim != 4 or f.shape[3] != 3 or a.ndim != 2:
            raise ValueError('a clip is (T, H, W, 3) frames and (n, C) samples, got %r and %r' % (f.shape, a.shape))
        cid = C.c_int()
        check(self.lib.l3_clipbank_add(self.h, _ptr(f), f.shape[0], f.shape[1], f.shape[2], _ptr(a), a.shape[0], a.shape[1],
                                       C.byref(cid)))
        return cid.value

    def info(self, clip=-1):
        """{n_frames, H, W, Ho, Wo, samples} of a clip; clip = -1: {clips, pixel bytes used, capacity, samples used, capacity,
        resize} of the bank."""
        out = np.zeros(6, np.int64)
        check(self.lib.l3_clipbank_info(self.h, int(clip), _ptr(out)))
        return tuple(int(x) for x in out)

    def audio(self, clip):
        out = np.empty(self.info(clip)[5], np.int16)
        check(self.lib.l3_clipbank_audio(self.h, int(clip), _ptr(out)))
        return out


def op_sample_batch(bank, records, augment=False):
    """l3_op_sample_batch: (video (n, 224, 224, 3) uint8, audio (n, 48000) int16, gains (n,) float64 or None)."""
    r = sample_records(records)
    n = len(r)
    v, a = np.empty((n, 224, 224, 3), np.uint8), np.empty((n, 48000), np.int16)
    g = np.empty(n, np.float64) if augment else None
    check(load().l3_op_sample_batch(bank.h, _ptr(r), n, int(bool(augment)), _ptr(v), _ptr(a), _ptr(g)))
    return v, a, g


# ---- cross-modal retrieval: the AVC head over every (frame, second) pair (csrc/pairs.hip) ---------------------------
PAIRS_TILE = 64                    # L3_PAIRS_TILE
PAIRS_MAX_ITEMS = 65535 * PAIRS_TILE
PAIRS_TOPK_MAX = 64                # L3_PAIRS_TOPK_MAX
PAIRS_TOPK_MAX_SEGMENTS = 256


def _head_width_ok(h):
    return 32 <= h <= 4096 and h % 32 == 0


def _index32(a, name, n, bound, what):
    """`a` as n int32 indices in [0, bound); ValueError otherwise"""
    if a is None:
        raise ValueError('%s must not be None' % name)
    a = np.asarray(a)
    if a.ndim != 1 or len(a) != n or a.dtype.kind not in 'iu':
        raise ValueError('%s must be %d integers, one per %s' % (name, n, what))
    if n and (a.min() < 0 or a.max() >= bound):
        bad = int(np.flatnonzero((a < 0) | (a >= bound))[0])
        raise ValueError('%s[%d] = %d outside [0, %d)' % (name, bad, int(a[bad]), bound))
    return np.ascontiguousarray(a, dtype=np.int32)


MAP_MAX_ROWS = 2 ** 31 - 1 - PAIRS_TILE          # location rows of a map; values of one call's output


def csr_check(item_ptr, query_idx, n_items, n_queries):
    """(item_ptr as int64, query_idx as int32) of listed (item, query) pairs in CSR form by item; ValueError unless item_ptr holds
    n_items + 1 offsets from 0, not decreasing, ending at len(query_idx) >= 1, and every query is in [0, n_queries)"""
    if item_ptr is None or query_idx is None:
        raise ValueError('item_ptr and query_idx must not be None')
    ptr, q = np.asarray(item_ptr), np.asarray(query_idx)
    if ptr.ndim != 1 or len(ptr) != n_items + 1 or ptr.dtype.kind not in 'iu':
        raise ValueError('item_ptr must be %d integers: one offset per item and the end' % (n_items + 1))
    if ptr[0] != 0 or np.any(np.diff(ptr.astype(np.int64)) < 0):
        raise ValueError('item_ptr must start at 0 and not decrease')
    if q.ndim != 1 or len(q) < 1 or len(q) != ptr[-1]:
        raise ValueError('query_idx must be item_ptr[-1] = %d >= 1 indices, not %s' % (int(ptr[-1]), q.shape))
    return np.ascontiguousarray(ptr, dtype=np.int64), _index32(q, 'query_idx', len(q), n_queries, 'listed pair')


def csr_by_item(items, n_items):
    """Listed pairs with the item of each, in any order, repeated or absent items allowed -> (item_ptr (n_items + 1) int64, order):
    order is the stable permutation that sorts the pairs by item, so pair order[r] stands at place r of the CSR list and a result
    in CSR order goes back to the caller's with out[order] = result."""
    items = _index32(items, 'items', len(items) if items is not None and np.ndim(items) == 1 else -1, n_items, 'listed pair')
    order = np.argsort(items, kind='stable')
    ptr = np.zeros(n_items + 1, np.int64)
    np.cumsum(np.bincount(items, minlength=n_items), out=ptr[1:])
    return ptr, order


class Pairs(object):
    """RAII wrapper over an l3_pairs handle: the head and the two projected sets resident on one device.  Every argument is checked
    here first (ValueError) and the handle is created by the first call that needs the device."""

    def __init__(self, nv, na, head, device=0):
        nv, na, head = int(nv), int(na), int(head)
        if nv < 1 or na < 1 or not _head_width_ok(head):
            raise ValueError('tower widths must be >= 1 and the head width a multiple of 32 in [32, 4096]; got %d, %d, %d' % (nv, na, head))
        self.nv, self.na, self.head, self.device = nv, na, head, int(device)
        self.lib = None
        self.h = None
        self.head_set = False
        self.n_vision = self.n_audio = 0

    def _handle(self):
        if self.h is None:
            self.lib = load()
            h = C.c_void_p()
            check(self.lib.l3_pairs_create(self.device, self.nv, self.na, self.head, C.byref(h)))
            self.h = h
        return self.h

    def close(self):
        if getattr(self, 'h', None):
            self.lib.l3_pairs_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_head(self, w1, b1, w2, b2):
        """dense_1 kernel (nv + na, head) and bias (head), dense_2 kernel (head, 2) and bias (2).  Voids the projected sets."""
        shapes = ((self.nv + self.na, self.head), (self.head,), (self.head, 2), (2,))
        arrs = []
        for name, a, shape in zip(('w1', 'b1', 'w2', 'b2'), (w1, b1, w2, b2), shapes):
            if a is None:
                raise ValueError('%s must not be None' % name)
            a = _f32(a)
            if a.shape != shape:
                raise ValueError('%s must have shape %s, not %s' % (name, shape, a.shape))
            arrs.append(a)
        h = self._handle()
        self.head_set = False
        self.n_vision = self.n_audio = 0
        self.map_done = set()
        check(self.lib.l3_pairs_set_head(h, *[_ptr(a) for a in arrs]))
        self.head_set = True

    def _set(self, vision, rows, lo, hi):
        side, width = ('vision', self.nv) if vision else ('audio', self.na)
        if rows is None:
            raise ValueError('the %s rows must not be None' % side)
        if not self.head_set:
            raise ValueError('set_head comes before set_%s' % side)
        if isinstance(rows, Features):
            if not rows.h:
                raise ValueError('the %s features are closed' % side)
            if rows.device != self.device:
                raise ValueError('the %s features are on device %d, the scorer on device %d' % (side, rows.device, self.device))
            n, d = rows.shape
            hi = n if hi is None else int(hi)
            lo = int(lo)
            if d != width:
                raise ValueError('the %s features have %d columns, the tower\'s output %d' % (side, d, width))
            if lo < 0 or hi > n or lo >= hi:
                raise ValueError('rows [%d, %d) are empty or outside the %d rows of the %s features' % (lo, hi, n, side))
            count = hi - lo
        else:
            x = _f32(rows)
            if x.ndim != 2 or x.shape[1] != width:
                raise ValueError('the %s rows must have shape (n, %d), not %s' % (side, width, x.shape))
            count = x.shape[0]
            if count < 1:
                raise ValueError('the %s set is empty' % side)
        if count > PAIRS_MAX_ITEMS:
            raise ValueError('a set holds at most %d items, not %d' % (PAIRS_MAX_ITEMS, count))
        h = self._handle()
        if vision:
            self.n_vision = 0
        else:
            self.n_audio = 0
        if isinstance(rows, Features):
            fn = self.lib.l3_pairs_set_vision_dev if vision else self.lib.l3_pairs_set_audio_dev
            check(fn(h, rows.h, lo, hi))
        else:
            fn = self.lib.l3_pairs_set_vision if vision else self.lib.l3_pairs_set_audio
            check(fn(h, _ptr(x), count))
        if vision:
            self.n_vision = count
        else:
            self.n_audio = count

    def set_vision(self, rows, lo=0, hi=None):
        """(Nv, nv) host rows, or rows [lo, hi) of a Features on this device -> U = V W1v, resident"""
        self._set(True, rows, lo, hi)

    def set_audio(self, rows, lo=0, hi=None):
        """(Na, na) host rows, or rows [lo, hi) of a Features on this device -> T = A W1a + b1, resident"""
        self._set(False, rows, lo, hi)

    def _need_sets(self):
        if not self.head_set or self.n_vision < 1 or self.n_audio < 1:
            raise ValueError('set_head, set_vision and set_audio come first')

    def matrix(self, v0=0, v1=None, a0=0, a1=None, prob=False):
        """the block [v0, v1) x [a0, a1) of margins (logit(corresponding) - logit(not)), or of P(corresponding) with prob"""
        self._need_sets()
        v1 = self.n_vision if v1 is None else int(v1)
        a1 = self.n_audio if a1 is None else int(a1)
        v0, a0 = int(v0), int(a0)
        if v0 < 0 or v1 > self.n_vision or v0 >= v1 or a0 < 0 or a1 > self.n_audio or a0 >= a1:
            raise ValueError('the block [%d, %d) x [%d, %d) is empty or outside the %d x %d pairs' % (v0, v1, a0, a1, self.n_vision,
                                                                                                      self.n_audio))
        out = np.empty((v1 - v0, a1 - a0), np.float32)
        h = self._handle()
        check(self.lib.l3_pairs_matrix(h, v0, v1, a0, a1, int(bool(prob)), _ptr(out)))
        return out

    def list(self, iv, ia):
        """margins of the pairs (iv[q], ia[q])"""
        self._need_sets()
        n = len(iv) if iv is not None and np.ndim(iv) == 1 else -1
        if n < 1:
            raise ValueError('iv and ia must be two equally long, non-empty 1-d index arrays')
        iv = _index32(iv, 'iv', n, self.n_vision, 'pair')
        ia = _index32(ia, 'ia', n, self.n_audio, 'pair')
        out = np.empty(n, np.float32)
        h = self._handle()
        check(self.lib.l3_pairs_list(h, _ptr(iv), _ptr(ia), n, _ptr(out)))
        return out

    def ranks(self, truth_a=None, truth_v=None, group_v=None, group_a=None):
        """(rank_v2a, rank_a2v): for every frame i the seconds j that score strictly above its true second truth_a[i] with
        group_a[j] != group_v[i], and for every second the frames likewise (truth_v).  A direction whose truth is None is not
        computed and comes back as None; the groups are given together or not at all."""
        self._need_sets()
        if truth_a is None and truth_v is None:
            raise ValueError('truth_a, truth_v or both are needed')
        if (group_v is None) != (group_a is None):
            raise ValueError('group_v and group_a are given together or both left None')
        ta = None if truth_a is None else _index32(truth_a, 'truth_a', self.n_vision, self.n_audio, 'frame')
        tv = None if truth_v is None else _index32(truth_v, 'truth_v', self.n_audio, self.n_vision, 'second')
        gv = ga = None
        if group_v is not None:
            gv = _index32(group_v, 'group_v', self.n_vision, 2 ** 31, 'frame')
            ga = _index32(group_a, 'group_a', self.n_audio, 2 ** 31, 'second')
        rv = None if ta is None else np.empty(self.n_vision, np.int32)
        ra = None if tv is None else np.empty(self.n_audio, np.int32)
        h = self._handle()
        check(self.lib.l3_pairs_ranks(h, _ptr(ta), _ptr(tv), _ptr(gv), _ptr(ga), _ptr(rv), _ptr(ra)))
        return rv, ra

    def topk(self, k, truth_a=None, truth_v=None, groups_v=None, groups_a=None, directions=('v2a', 'a2v')):
        """((idx_v2a, margin_v2a), (idx_a2v, margin_a2v)): for every frame its k best-scoring seconds among those of other groups
        (all seconds without groups) plus, with truth_a, its own second truth_a[i]; for every second the frames likewise (truth_v).
        (n, k) int32 indices and float32 margins, the larger margin first and the smaller index first among equal margins; a list
        with fewer candidates ends in index -1 and margin -inf.  directions: 'v2a', 'a2v' or both; a direction that is not asked
        for comes back as None, and its truth is checked but not used."""
        self._need_sets()
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= PAIRS_TOPK_MAX:
            raise ValueError('k must be an integer in [1, %d], not %r' % (PAIRS_TOPK_MAX, k))
        if isinstance(directions, str):
            directions = (directions,)
        directions = tuple(directions)
        if not directions or any(d not in ('v2a', 'a2v') for d in directions):
            raise ValueError("directions must be 'v2a', 'a2v' or both, not %r" % (directions,))
        if (groups_v is None) != (groups_a is None):
            raise ValueError('groups_v and groups_a are given together or both left None')
        if groups_v is None and (truth_a is not None or truth_v is not None):
            raise ValueError('a truth without groups keeps nothing: nothing is excluded')
        ta = None if truth_a is None else _index32(truth_a, 'truth_a', self.n_vision, self.n_audio, 'frame')
        tv = None if truth_v is None else _index32(truth_v, 'truth_v', self.n_audio, self.n_vision, 'second')
        gv = ga = None
        if groups_v is not None:
            gv = _index32(groups_v, 'groups_v', self.n_vision, 2 ** 31, 'frame')
            ga = _index32(groups_a, 'groups_a', self.n_audio, 2 ** 31, 'second')
        k = int(k)
        iv = mv = ia = ma = None
        if 'v2a' in directions:
            iv, mv = np.empty((self.n_vision, k), np.int32), np.empty((self.n_vision, k), np.float32)
        if 'a2v' in directions:
            ia, ma = np.empty((self.n_audio, k), np.int32), np.empty((self.n_audio, k), np.float32)
        h = self._handle()
        check(self.lib.l3_pairs_topk(h, k, _ptr(ta), _ptr(tv), _ptr(gv), _ptr(ga), _ptr(iv), _ptr(mv), _ptr(ia), _ptr(ma)))
        return (None if iv is None else (iv, mv)), (None if ia is None else (ia, ma))

    # ---- the location map of one side (csrc/locmap.hip) ----
    map_side = -1
    map_items = map_done = 0
    map_hw = (0, 0)

    def map_reserve(self, side, n_items, H, W):
        """l3_pairs_map_reserve: a map of n_items items of H x W locations; side 0: vision locations queried by the audio set, 1:
        audio locations queried by the vision set"""
        if side not in (0, 1):
            raise ValueError('side must be 0 (vision locations) or 1 (audio locations), not %r' % (side,))
        n_items, H, W = int(n_items), int(H), int(W)
        if n_items < 1 or H < 1 or W < 1 or n_items * H * W > MAP_MAX_ROWS:
            raise ValueError('need n_items >= 1 and H, W >= 1 with n_items H W <= %d; got %d items of %d x %d' % (MAP_MAX_ROWS, n_items, H, W))
        h = self._handle()
        self.map_side = -1
        check(self.lib.l3_pairs_map_reserve(h, int(side), n_items, H, W))
        self.map_side, self.map_items, self.map_hw, self.map_done = int(side), n_items, (H, W), set()

    def map_put(self, loc, lo_row, item0, n_items):
        """l3_pairs_map_put: the n_items H W rows of the Features loc from row lo_row -> the items [item0, item0 + n_items) of the map"""
        if self.map_side < 0:
            raise ValueError('map_reserve comes before map_put')
        if not self.head_set:
            raise ValueError('set_head comes before map_put')
        if not isinstance(loc, Features) or not loc.h:
            raise ValueError('the location rows must be an open Features')
        if loc.device != self.device:
            raise ValueError('the location rows are on device %d, the scorer on device %d' % (loc.device, self.device))
        width = self.nv if self.map_side == 0 else self.na
        n, d = loc.shape
        lo_row, item0, n_items = int(lo_row), int(item0), int(n_items)
        L = self.map_hw[0] * self.map_hw[1]
        if d != width:
            raise ValueError('the location rows have %d columns, the tower\'s last feature map %d channels' % (d, width))
        if n_items < 1 or item0 < 0 or item0 + n_items > self.map_items:
            raise ValueError('items [%d, %d) are empty or outside the %d items of the map' % (item0, item0 + n_items, self.map_items))
        if lo_row < 0 or lo_row + n_items * L > n:
            raise ValueError('rows [%d, %d) outside the %d rows of the location matrix' % (lo_row, lo_row + n_items * L, n))
        check(self.lib.l3_pairs_map_put(self._handle(), loc.h, lo_row, item0, n_items))
        self.map_done.update(range(item0, item0 + n_items))

    @property
    def map_queries(self):
        """the number of queries of the map: the size of the opposite set"""
        return self.n_audio if self.map_side == 0 else self.n_vision

    def _need_map(self):
        if not self.head_set or self.map_side < 0 or len(self.map_done) != self.map_items or self.map_queries < 1:
            raise ValueError('set_head, map_reserve, map_put of every item and the query set (set_%s) come first' %
                             ('audio' if self.map_side == 0 else 'vision'))

    def map_list(self, item_ptr, query_idx, maps=True, peaks=True):
        """l3_pairs_map_list: the listed (item, query) pairs in CSR form by item (item_ptr: map_items + 1 offsets into query_idx) ->
        (maps (n, L) or None, peak (n,) or None, arg (n,) or None) in the order of query_idx"""
        self._need_map()
        if not maps and not peaks:
            raise ValueError('maps, peaks or both')
        ptr, q = csr_check(item_ptr, query_idx, self.map_items, self.map_queries)
        n, L = len(q), self.map_hw[0] * self.map_hw[1]
        if maps and n * L > MAP_MAX_ROWS:
            raise ValueError('%d maps of %d locations are more than %d values: list fewer pairs a call' % (n, L, MAP_MAX_ROWS))
        m = np.empty((n, L), np.float32) if maps else None
        pk = np.empty(n, np.float32) if peaks else None
        ar = np.empty(n, np.int32) if peaks else None
        check(self.lib.l3_pairs_map_list(self._handle(), _ptr(ptr), _ptr(q), _ptr(m), _ptr(pk), _ptr(ar)))
        return m, pk, ar

    def map_peaks(self, i0=0, i1=None, j0=0, j1=None):
        """l3_pairs_map_peaks: (S, arg) of the block [i0, i1) x [j0, j1) of items x queries: S_ij = max over item i's locations of
        the margin with query j, arg the location attaining it (-1: every margin NaN)"""
        self._need_map()
        i1 = self.map_items if i1 is None else int(i1)
        j1 = self.map_queries if j1 is None else int(j1)
        i0, j0 = int(i0), int(j0)
        if i0 < 0 or i1 > self.map_items or i0 >= i1 or j0 < 0 or j1 > self.map_queries or j0 >= j1 or (i1 - i0) * (j1 - j0) > MAP_MAX_ROWS:
            raise ValueError('the block [%d, %d) x [%d, %d) is empty, too large or outside the %d items x %d queries' %
                             (i0, i1, j0, j1, self.map_items, self.map_queries))
        S, arg = np.empty((i1 - i0, j1 - j0), np.float32), np.empty((i1 - i0, j1 - j0), np.int32)
        check(self.lib.l3_pairs_map_peaks(self._handle(), i0, i1, j0, j1, _ptr(S), _ptr(arg)))
        return S, arg

    def map_ranks(self, truth_a=None, truth_v=None, group_v=None, group_a=None):
        """l3_pairs_map_ranks: Pairs.ranks over S, the best-location score of every (frame, second) pair; frames x seconds whichever
        side the map is: the map's items stand for their side's set"""
        self._need_map()
        nv, na = (self.map_items, self.n_audio) if self.map_side == 0 else (self.n_vision, self.map_items)
        if truth_a is None and truth_v is None:
            raise ValueError('truth_a, truth_v or both are needed')
        if (group_v is None) != (group_a is None):
            raise ValueError('group_v and group_a are given together or both left None')
        ta = None if truth_a is None else _index32(truth_a, 'truth_a', nv, na, 'frame')
        tv = None if truth_v is None else _index32(truth_v, 'truth_v', na, nv, 'second')
        gv = ga = None
        if group_v is not None:
            gv = _index32(group_v, 'group_v', nv, 2 ** 31, 'frame')
            ga = _index32(group_a, 'group_a', na, 2 ** 31, 'second')
        rv = None if ta is None else np.empty(nv, np.int32)
        ra = None if tv is None else np.empty(na, np.int32)
        check(self.lib.l3_pairs_map_ranks(self._handle(), _ptr(ta), _ptr(tv), _ptr(gv), _ptr(ga), _ptr(rv), _ptr(ra)))
        return rv, ra

    def map_time(self, what, reps=10):
        """l3_pairs_map_time: device ms per launch of 'list' (the diagonal, maps stored), 'peaks' (every pair) or 'ranks' (the
        counting pass, the diagonal as truth)"""
        kinds = ('list', 'peaks', 'ranks')
        if what not in kinds:
            raise ValueError('what must be one of %s' % (kinds,))
        self._need_map()
        ms = C.c_double()
        check(self.lib.l3_pairs_map_time(self._handle(), kinds.index(what), int(reps), C.byref(ms)))
        return ms.value

    def time(self, what, n_rows=0, reps=10):
        """l3_pairs_time: device ms per launch of 'matrix', 'ranks', 'project_vision' or 'project_audio' (n_rows rows), of 'topk'
        (both directions, all four launches) or 'topk_merge' (the frames' merge kernel alone) at k = n_rows, 10 when that is 0"""
        kinds = ('matrix', 'ranks', 'project_vision', 'project_audio', 'topk', 'topk_merge')
        if what not in kinds:
            raise ValueError('what must be one of %s' % (kinds,))
        ms = C.c_double()
        h = self._handle()
        check(self.lib.l3_pairs_time(h, kinds.index(what), int(n_rows), int(reps), C.byref(ms)))
        return ms.value


def op_project(x, w, b=None, device=0):
    """l3_op_project: x (n, K) w (K, H) [+ b] by the projection kernel of csrc/pairs.hip"""
    x, w, b = _f32(x), _f32(w), _f32(b)
    if x.ndim != 2 or w.ndim != 2 or x.shape[1] != w.shape[0] or x.shape[0] < 1 or not _head_width_ok(w.shape[1]) or \
            (b is not None and b.shape != (w.shape[1],)):
        raise ValueError('need x (n >= 1, K), w (K, H) with H a multiple of 32 in [32, 4096] and b (H,) or None')
    out = np.empty((x.shape[0], w.shape[1]), np.float32)
    check(load().l3_op_project(int(device), _ptr(x), _ptr(w), _ptr(b), x.shape[0], x.shape[1], w.shape[1], _ptr(out)))
    return out


def op_pair_margins(u, t, wd, bd, device=0):
    """l3_op_pair_margins: margins (Nv, Na) of u (Nv, H) and t (Na, H) by the pair kernel alone"""
    u, t, wd = _f32(u), _f32(t), _f32(wd)
    if u.ndim != 2 or t.ndim != 2 or u.shape[0] < 1 or t.shape[0] < 1 or u.shape[1] != t.shape[1] or wd.shape != (u.shape[1],) or \
            not _head_width_ok(u.shape[1]):
        raise ValueError('need u (Nv >= 1, H), t (Na >= 1, H) and wd (H,) with H a multiple of 32 in [32, 4096]')
    out = np.empty((u.shape[0], t.shape[0]), np.float32)
    check(load().l3_op_pair_margins(int(device), _ptr(u), _ptr(t), _ptr(wd), float(np.float32(bd)), u.shape[0], t.shape[0], u.shape[1],
                                    _ptr(out)))
    return out


def _op_map_args(m, t, wd, L):
    m, t, wd = _f32(m), _f32(t), _f32(wd)
    L = int(L)
    if m.ndim != 2 or t.ndim != 2 or L < 1 or m.shape[0] < 1 or m.shape[0] % L or t.shape[0] < 1 or m.shape[1] != t.shape[1] or \
            wd.shape != (m.shape[1],) or not _head_width_ok(m.shape[1]) or m.shape[0] > MAP_MAX_ROWS:
        raise ValueError('need m (n_items L, H), t (n_q >= 1, H) and wd (H,) with L >= 1 and H a multiple of 32 in [32, 4096]')
    return m, t, wd, L, m.shape[0] // L


def op_map_list(m, t, wd, bd, L, item_ptr, query_idx, maps=True, peaks=True, device=0):
    """l3_op_map_list: (maps (n, L) | None, peak | None, arg | None) of the listed (item, query) pairs (CSR by item) of projected
    location rows m (n_items L, H) and query rows t (n_q, H), by the map kernel alone"""
    m, t, wd, L, n_items = _op_map_args(m, t, wd, L)
    if not maps and not peaks:
        raise ValueError('maps, peaks or both')
    ptr, q = csr_check(item_ptr, query_idx, n_items, t.shape[0])
    n = len(q)
    if maps and n * L > MAP_MAX_ROWS:
        raise ValueError('%d maps of %d locations are more than %d values' % (n, L, MAP_MAX_ROWS))
    mp = np.empty((n, L), np.float32) if maps else None
    pk = np.empty(n, np.float32) if peaks else None
    ar = np.empty(n, np.int32) if peaks else None
    check(load().l3_op_map_list(int(device), _ptr(m), _ptr(t), _ptr(wd), float(np.float32(bd)), n_items, L, t.shape[0], m.shape[1],
                                _ptr(ptr), _ptr(q), _ptr(mp), _ptr(pk), _ptr(ar)))
    return mp, pk, ar


def op_map_peaks(m, t, wd, bd, L, i0=0, i1=None, j0=0, j1=None, device=0):
    """l3_op_map_peaks: (S, arg) of the block [i0, i1) x [j0, j1) of items x queries, by the map kernel alone"""
    m, t, wd, L, n_items = _op_map_args(m, t, wd, L)
    i1 = n_items if i1 is None else int(i1)
    j1 = t.shape[0] if j1 is None else int(j1)
    i0, j0 = int(i0), int(j0)
    if i0 < 0 or i1 > n_items or i0 >= i1 or j0 < 0 or j1 > t.shape[0] or j0 >= j1 or (i1 - i0) * (j1 - j0) > MAP_MAX_ROWS:
        raise ValueError('the block [%d, %d) x [%d, %d) is empty, too large or outside the %d items x %d queries' %
                         (i0, i1, j0, j1, n_items, t.shape[0]))
    S, arg = np.empty((i1 - i0, j1 - j0), np.float32), np.empty((i1 - i0, j1 - j0), np.int32)
    check(load().l3_op_map_peaks(int(device), _ptr(m), _ptr(t), _ptr(wd), float(np.float32(bd)), n_items, L, t.shape[0], m.shape[1],
                                 i0, i1, j0, j1, _ptr(S), _ptr(arg)))
    return S, arg


def op_pair_topk(u, t, wd, bd, k, truth=None, group_q=None, group_c=None, segments=0, device=0):
    """l3_op_pair_topk: (idx, margin), both (Nq, k): for every row of u (Nq, H) its k best-scoring rows of t (Nc, H) by the order of
    Pairs.topk, by the top-k kernels alone.  segments: runs of candidate tiles with partial lists of their own, 0: the library's
    choice."""
    u, t, wd = _f32(u), _f32(t), _f32(wd)
    if u.ndim != 2 or t.ndim != 2 or u.shape[0] < 1 or t.shape[0] < 1 or u.shape[1] != t.shape[1] or wd.shape != (u.shape[1],) or \
            not _head_width_ok(u.shape[1]):
        raise ValueError('need u (Nq >= 1, H), t (Nc >= 1, H) and wd (H,) with H a multiple of 32 in [32, 4096]')
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= PAIRS_TOPK_MAX:
        raise ValueError('k must be an integer in [1, %d], not %r' % (PAIRS_TOPK_MAX, k))
    if not 0 <= int(segments) <= PAIRS_TOPK_MAX_SEGMENTS:
        raise ValueError('segments must be in [0, %d]' % PAIRS_TOPK_MAX_SEGMENTS)
    if (group_q is None) != (group_c is None):
        raise ValueError('group_q and group_c are given together or both left None')
    if truth is not None and group_q is None:
        raise ValueError('a truth without groups keeps nothing: nothing is excluded')
    nq, nc = u.shape[0], t.shape[0]
    tr = None if truth is None else _index32(truth, 'truth', nq, nc, 'query')
    gq = gc = None
    if group_q is not None:
        gq, gc = _index32(group_q, 'group_q', nq, 2 ** 31, 'query'), _index32(group_c, 'group_c', nc, 2 ** 31, 'candidate')
    idx, margin = np.empty((nq, int(k)), np.int32), np.empty((nq, int(k)), np.float32)
    check(load().l3_op_pair_topk(int(device), _ptr(u), _ptr(t), _ptr(wd), float(np.float32(bd)), nq, nc, u.shape[1], int(k), _ptr(tr),
                                 _ptr(gq), _ptr(gc), int(segments), _ptr(idx), _ptr(margin)))
    return idx, margin


# ---- nearest neighbours among embedding rows (csrc/knn.hip) -----------------------------------------------------------
KNN_METRICS = {'sqeuclidean': 0, 'cosine': 1}          # L3_KNN_SQEUCLIDEAN, L3_KNN_COSINE
KNN_TOPK_MAX = 64                  # L3_KNN_TOPK_MAX
KNN_MAX_SEGMENTS = 256             # L3_KNN_MAX_SEGMENTS
KNN_MAX_SIZES = 8                  # L3_KNN_MAX_SIZES
KNN_MAX_CLASSES = 256              # L3_KNN_MAX_CLASSES
KNN_MAX_ROWS = 2 ** 31 - 1


def knn_check_k(k):
    """k as an int in [1, KNN_TOPK_MAX]; ValueError otherwise"""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= KNN_TOPK_MAX:
        raise ValueError('n_neighbors must be an integer in [1, %d], not %r' % (KNN_TOPK_MAX, k))
    return int(k)


def knn_check_sizes(ks, k):
    """the list sizes of one vote as int32: 1 .. KNN_MAX_SIZES of them, strictly ascending, in [1, k]; ValueError otherwise"""
    sizes = list(ks) if ks is not None and np.ndim(ks) == 1 else []
    if not 1 <= len(sizes) <= KNN_MAX_SIZES or any(isinstance(s, bool) or not isinstance(s, (int, np.integer)) for s in sizes):
        raise ValueError('ks must hold 1 to %d integers, not %r' % (KNN_MAX_SIZES, ks))
    if sizes[0] < 1 or sizes[-1] > k or any(b <= a for a, b in zip(sizes, sizes[1:])):
        raise ValueError('ks must ascend strictly within [1, n_neighbors = %d], not %r' % (k, ks))
    return np.asarray(sizes, np.int32)


def _group32(a, name, n, what):
    if a is None:
        raise ValueError('%s must not be None' % name)
    a = np.asarray(a)
    if a.ndim != 1 or len(a) != n or a.dtype.kind not in 'iu':
        raise ValueError('%s must be %d integers, one per %s' % (name, n, what))
    if n and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
        raise ValueError('%s must fit 32-bit integers' % name)
    return np.ascontiguousarray(a, dtype=np.int32)


def _knn_groups(group_q, group_c, nq, nc):
    if (group_q is None) != (group_c is None):
        raise ValueError('the groups of the queries and of the fitted rows are given together or both left None')
    if group_q is None:
        return None, None
    return _group32(group_q, 'groups_q', nq, 'query'), _group32(group_c, 'groups_fit', nc, 'fitted row')


def _knn_rows(rows, D, side):
    """(Features or float32 array, count) of one side's rows; ValueError unless they are (n >= 1, D)"""
    if rows is None:
        raise ValueError('the %s rows must not be None' % side)
    if isinstance(rows, Features):
        if not rows.h:
            raise ValueError('the %s features are closed' % side)
        n, d = rows.shape
        x = rows
    else:
        x = np.asarray(rows)
        if x.dtype != np.float32:
            raise ValueError('the %s rows must be float32, not %s (there is no silent conversion)' % (side, x.dtype))
        x = np.ascontiguousarray(x)
        if x.ndim != 2:
            raise ValueError('the %s rows must have shape (n, %d), not %s' % (side, D, x.shape))
        n, d = x.shape
    if d != D:
        raise ValueError('the %s rows have %d columns, the handle\'s %d' % (side, d, D))
    if not 1 <= n <= KNN_MAX_ROWS:
        raise ValueError('the %s set must hold 1 to 2^31 - 1 rows, not %d' % (side, n))
    return x, n


class KNN(object):
    """RAII wrapper over an l3_knn handle: a database of float32 rows (with labels or without) and a query set resident on one
    device.  Every argument is checked here first (ValueError) and the handle is created by the first call that needs the device."""

    def __init__(self, D, metric='sqeuclidean', device=0):
        if isinstance(D, bool) or not isinstance(D, (int, np.integer)) or not 1 <= D <= 2 ** 20:
            raise ValueError('D must be an integer in [1, 2^20], not %r' % (D,))
        if metric not in KNN_METRICS:
            raise ValueError('metric must be one of %s, not %r' % (sorted(KNN_METRICS), metric))
        self.D, self.metric, self.device = int(D), metric, int(device)
        self.lib = None
        self.h = None
        self.n_database = self.n_queries = 0
        self.has_labels = False
        self.label_max = -1
        self.self_query = False

    def _handle(self):
        if self.h is None:
            self.lib = load()
            h = C.c_void_p()
            check(self.lib.l3_knn_create(self.device, self.D, KNN_METRICS[self.metric], C.byref(h)))
            self.h = h
        return self.h

    def close(self):
        if getattr(self, 'h', None):
            self.lib.l3_knn_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check_device(self, x, side):
        if isinstance(x, Features) and x.device != self.device:
            raise ValueError('the %s features are on device %d, the handle on device %d' % (side, x.device, self.device))

    def set_database(self, rows, labels=None):
        """(n, D) host rows or a Features on this device -> the handle's own copy; labels: n integers >= 0, or None"""
        x, n = _knn_rows(rows, self.D, 'database')
        self._check_device(x, 'database')
        lab = None
        if labels is not None:
            lab = _index32(np.asarray(labels).reshape(-1), 'labels', n, 2 ** 31, 'database row')
        h = self._handle()
        self.n_database = 0
        if self.self_query:
            self.n_queries = 0
        if isinstance(x, Features):
            check(self.lib.l3_knn_set_database_dev(h, x.h, 0, n, _ptr(lab)))
        else:
            check(self.lib.l3_knn_set_database(h, _ptr(x), n, _ptr(lab)))
        self.n_database = n
        self.has_labels = lab is not None
        self.label_max = int(lab.max()) if lab is not None else -1
        if self.self_query:
            self.n_queries = n

    def set_queries(self, rows):
        """(n, D) host rows or a Features on this device -> the handle's own copy"""
        x, n = _knn_rows(rows, self.D, 'query')
        self._check_device(x, 'query')
        h = self._handle()
        self.n_queries, self.self_query = 0, False
        if isinstance(x, Features):
            check(self.lib.l3_knn_set_queries_dev(h, x.h, 0, n))
        else:
            check(self.lib.l3_knn_set_queries(h, _ptr(x), n))
        self.n_queries = n

    def query_self(self):
        """the database is the query set (no second copy)"""
        if self.n_database < 1:
            raise ValueError('set_database comes first')
        check(self.lib.l3_knn_query_self(self._handle()))
        self.self_query, self.n_queries = True, self.n_database

    def _need_sets(self):
        if self.n_database < 1 or self.n_queries < 1:
            raise ValueError('set_database and set_queries (or query_self) come first')

    def matrix(self, q0=0, q1=None, c0=0, c1=None):
        """the block [q0, q1) x [c0, c1) of distances"""
        self._need_sets()
        q1 = self.n_queries if q1 is None else int(q1)
        c1 = self.n_database if c1 is None else int(c1)
        q0, c0 = int(q0), int(c0)
        if q0 < 0 or q1 > self.n_queries or q0 >= q1 or c0 < 0 or c1 > self.n_database or c0 >= c1:
            raise ValueError('the block [%d, %d) x [%d, %d) is empty or outside the %d x %d pairs' % (q0, q1, c0, c1, self.n_queries,
                                                                                                      self.n_database))
        out = np.empty((q1 - q0, c1 - c0), np.float32)
        check(self.lib.l3_knn_matrix(self._handle(), q0, q1, c0, c1, _ptr(out)))
        return out

    def list(self, iq, ic):
        """distances of the pairs (query iq[p], database row ic[p])"""
        self._need_sets()
        n = len(iq) if iq is not None and np.ndim(iq) == 1 else -1
        if n < 1:
            raise ValueError('iq and ic must be two equally long, non-empty 1-d index arrays')
        iq = _index32(iq, 'iq', n, self.n_queries, 'pair')
        ic = _index32(ic, 'ic', n, self.n_database, 'pair')
        out = np.empty(n, np.float32)
        check(self.lib.l3_knn_list(self._handle(), _ptr(iq), _ptr(ic), n, _ptr(out)))
        return out

    def topk(self, k, group_q=None, group_c=None):
        """(idx, dist), both (n_queries, k): every query's k nearest database rows among those of other groups (all rows without
        groups), the smaller distance first and the smaller index first among equal distances; a list with fewer candidates ends
        in index -1 and distance +inf"""
        self._need_sets()
        k = knn_check_k(k)
        gq, gc = _knn_groups(group_q, group_c, self.n_queries, self.n_database)
        idx, dist = np.empty((self.n_queries, k), np.int32), np.empty((self.n_queries, k), np.float32)
        check(self.lib.l3_knn_topk(self._handle(), k, _ptr(gq), _ptr(gc), _ptr(idx), _ptr(dist)))
        return idx, dist

    def vote(self, k, ks, n_classes, group_q=None, group_c=None, file_idxs=None, outputs=('pred',)):
        """l3_knn_vote -> dict of what `outputs` names: 'counts' (n, S, C) and 'pred' (n, S) int32, and with file_idxs 'file_counts'
        (F, S, C) and 'file_pred' (F, S); the lists stay on the device"""
        self._need_sets()
        k = knn_check_k(k)
        sizes = knn_check_sizes(ks, k)
        outputs = tuple(outputs)
        unknown = set(outputs) - {'counts', 'pred', 'file_counts', 'file_pred'}
        if unknown or not outputs:
            raise ValueError("outputs must name some of 'counts', 'pred', 'file_counts', 'file_pred', not %r" % (outputs,))
        if isinstance(n_classes, bool) or not isinstance(n_classes, (int, np.integer)) or not 1 <= n_classes <= KNN_MAX_CLASSES:
            raise ValueError('n_classes must be an integer in [1, %d], not %r' % (KNN_MAX_CLASSES, n_classes))
        if not self.has_labels:
            raise ValueError('the database was set without labels')
        if self.label_max >= n_classes:
            raise ValueError('the database holds the label %d, outside [0, %d)' % (self.label_max, n_classes))
        gq, gc = _knn_groups(group_q, group_c, self.n_queries, self.n_database)
        files, F = None, 0
        if 'file_counts' in outputs or 'file_pred' in outputs:
            if file_idxs is None:
                raise ValueError("'file_counts' and 'file_pred' need file_idxs")
            files = np.ascontiguousarray(np.asarray(file_idxs, np.int64).reshape(-1, 2))
            F = len(files)
            if F < 1 or np.any(files[:, 0] < 0) or np.any(files[:, 0] >= files[:, 1]) or np.any(files[:, 1] > self.n_queries):
                raise ValueError('file_idxs must hold row ranges [s, e) with 0 <= s < e <= %d' % self.n_queries)
        n, S, nc = self.n_queries, len(sizes), int(n_classes)
        got = {}
        if 'counts' in outputs:
            got['counts'] = np.empty((n, S, nc), np.int32)
        if 'pred' in outputs:
            got['pred'] = np.empty((n, S), np.int32)
        if 'file_counts' in outputs:
            got['file_counts'] = np.empty((F, S, nc), np.int32)
        if 'file_pred' in outputs:
            got['file_pred'] = np.empty((F, S), np.int32)
        check(self.lib.l3_knn_vote(self._handle(), k, _ptr(sizes), S, nc, _ptr(gq), _ptr(gc), _ptr(files), F, _ptr(got.get('counts')),
                                   _ptr(got.get('pred')), _ptr(got.get('file_counts')), _ptr(got.get('file_pred'))))
        return got

    def time(self, what, k=5, reps=3):
        """l3_knn_time: device ms per launch of 'topk' (lists and merge at k) or 'matrix' (a block of at most 8192 x 8192)"""
        kinds = ('topk', 'matrix')
        if what not in kinds:
            raise ValueError('what must be one of %s' % (kinds,))
        self._need_sets()
        ms = C.c_double()
        check(self.lib.l3_knn_time(self._handle(), kinds.index(what), knn_check_k(k), int(reps), C.byref(ms)))
        return ms.value


def op_knn_topk(Q, X, k, metric='sqeuclidean', segments=0, group_q=None, group_c=None, device=0):
    """l3_op_knn_topk: (idx, dist), both (nq, k): for every row of Q (nq, D) its k nearest rows of X (nc, D) by the order of KNN.topk,
    by the kernels alone.  segments: runs of candidate tiles with partial lists of their own, 0: the library's choice."""
    if metric not in KNN_METRICS:
        raise ValueError('metric must be one of %s, not %r' % (sorted(KNN_METRICS), metric))
    Q, X = _f32(Q), _f32(X)
    if Q.ndim != 2 or X.ndim != 2 or Q.shape[0] < 1 or X.shape[0] < 1 or Q.shape[1] != X.shape[1] or Q.shape[1] < 1:
        raise ValueError('need Q (nq >= 1, D) and X (nc >= 1, D) with D >= 1')
    k = knn_check_k(k)
    if not 0 <= int(segments) <= KNN_MAX_SEGMENTS:
        raise ValueError('segments must be in [0, %d]' % KNN_MAX_SEGMENTS)
    nq, nc = Q.shape[0], X.shape[0]
    gq, gc = _knn_groups(group_q, group_c, nq, nc)
    idx, dist = np.empty((nq, k), np.int32), np.empty((nq, k), np.float32)
    check(load().l3_op_knn_topk(int(device), _ptr(Q), _ptr(X), nq, nc, Q.shape[1], KNN_METRICS[metric], k, int(segments), _ptr(gq), _ptr(gc),
                                _ptr(idx), _ptr(dist)))
    return idx, dist


# ---- k-means over embedding rows (csrc/kmeans.hip) --------------------------------------------------------------------
KMEANS_RUN = 256                   # L3_KMEANS_RUN
KMEANS_MAX_CLUSTERS = 65536        # L3_KMEANS_MAX_CLUSTERS
KMEANS_MAX_CLASSES = 256           # L3_KMEANS_MAX_CLASSES
KMEANS_TIMED = ('assign', 'update', 'iteration', 'seed', 'sort', 'inertia')


def kmeans_check_k(K, n=None):
    """K as an int in [1, min(n, KMEANS_MAX_CLUSTERS)]; ValueError otherwise"""
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or not 1 <= K <= KMEANS_MAX_CLUSTERS:
        raise ValueError('n_clusters must be an integer in [1, %d], not %r' % (KMEANS_MAX_CLUSTERS, K))
    if n is not None and K > n:
        raise ValueError('%d clusters need at least as many rows, not %d' % (K, n))
    return int(K)


def kmeans_check_metric(metric):
    if metric == 'cosine':
        raise ValueError("k-means is defined for the squared Euclidean distance only: a cluster's mean minimises it and not the cosine "
                         "distance (normalise the rows and use 'sqeuclidean')")
    if metric != 'sqeuclidean':
        raise ValueError("metric must be 'sqeuclidean', not %r" % (metric,))
    return metric


def _file_ranges(file_idxs, n):
    files = np.ascontiguousarray(np.asarray(file_idxs, np.int64).reshape(-1, 2))
    if len(files) < 1 or np.any(files[:, 0] < 0) or np.any(files[:, 0] >= files[:, 1]) or np.any(files[:, 1] > n):
        raise ValueError('file_idxs must hold row ranges [s, e) with 0 <= s < e <= %d' % n)
    return files


class KMeans(object):
    """RAII wrapper over an l3_kmeans handle: float32 rows and K centroids resident on one device.  Every argument is checked here
    first (ValueError) and the handle is created by the first call that needs the device."""

    def __init__(self, D, K, metric='sqeuclidean', device=0):
        if isinstance(D, bool) or not isinstance(D, (int, np.integer)) or not 1 <= D <= 2 ** 20:
            raise ValueError('D must be an integer in [1, 2^20], not %r' % (D,))
        self.D, self.K, self.metric, self.device = int(D), kmeans_check_k(K), kmeans_check_metric(metric), int(device)
        self.lib = None
        self.h = None
        self.n = self.n_predicted = 0
        self.has_centroids = self.assigned = False

    def _handle(self):
        if self.h is None:
            self.lib = load()
            h = C.c_void_p()
            check(self.lib.l3_kmeans_create(self.device, self.D, self.K, KNN_METRICS[self.metric], C.byref(h)))
            self.h = h
        return self.h

    def close(self):
        if getattr(self, 'h', None):
            self.lib.l3_kmeans_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _rows(self, rows, side):
        x, n = _knn_rows(rows, self.D, side)
        if isinstance(x, Features) and x.device != self.device:
            raise ValueError('the %s features are on device %d, the handle on device %d' % (side, x.device, self.device))
        return x, n

    def set_rows(self, rows):
        """(n >= K, D) host rows or a Features on this device -> the handle's own copy; voids the labels"""
        x, n = self._rows(rows, 'fitted')
        kmeans_check_k(self.K, n)
        h = self._handle()
        self.n, self.assigned = 0, False
        if isinstance(x, Features):
            check(self.lib.l3_kmeans_set_rows_dev(h, x.h, 0, n))
        else:
            check(self.lib.l3_kmeans_set_rows(h, _ptr(x), n))
        self.n = n

    def _need_rows(self):
        if self.n < 1:
            raise ValueError('set_rows comes first')

    def _need_centroids(self):
        if not self.has_centroids:
            raise ValueError('the centroids come first: set_centroids, seed_rows or seed_pp')

    def set_centroids(self, centroids):
        c = np.asarray(centroids)
        if c.dtype != np.float32 or c.shape != (self.K, self.D):
            raise ValueError('the centroids must be float32 of shape (%d, %d), not %s %s' % (self.K, self.D, c.dtype, c.shape))
        c = np.ascontiguousarray(c)
        h = self._handle()
        self.has_centroids = self.assigned = False
        check(self.lib.l3_kmeans_set_centroids(h, _ptr(c)))
        self.has_centroids = True

    def seed_rows(self, rows):
        """the centroids become the fitted rows `rows` (K indices)"""
        self._need_rows()
        idx = np.asarray(rows)
        if idx.ndim != 1 or len(idx) != self.K or idx.dtype.kind not in 'iu' or idx.min() < 0 or idx.max() >= self.n:
            raise ValueError('rows must be %d indices in [0, %d)' % (self.K, self.n))
        idx = np.ascontiguousarray(idx, np.int64)
        self.has_centroids = self.assigned = False
        check(self.lib.l3_kmeans_seed_rows(self._handle(), _ptr(idx)))
        self.has_centroids = True

    def seed_pp(self, u):
        """k-means++ from the K draws u in [0, 1) -> the K chosen rows (int64)"""
        self._need_rows()
        u = np.asarray(u)
        if u.dtype != np.float64 or u.shape != (self.K,) or not np.all((u >= 0.0) & (u < 1.0)):
            raise ValueError('u must be %d float64 draws in [0, 1)' % self.K)
        u = np.ascontiguousarray(u)
        chosen = np.empty(self.K, np.int64)
        self.has_centroids = self.assigned = False
        check(self.lib.l3_kmeans_seed_pp(self._handle(), _ptr(u), _ptr(chosen)))
        self.has_centroids = True
        return chosen

    def assign(self, outputs=('labels', 'dist')):
        """one assignment -> dict with 'inertia', 'changed' and what `outputs` names of 'labels' (n int32) and 'dist' (n float32)"""
        self._need_rows()
        self._need_centroids()
        got = {}
        if 'labels' in outputs:
            got['labels'] = np.empty(self.n, np.int32)
        if 'dist' in outputs:
            got['dist'] = np.empty(self.n, np.float32)
        inertia, changed = C.c_double(), C.c_int64()
        check(self.lib.l3_kmeans_assign(self._handle(), _ptr(got.get('labels')), _ptr(got.get('dist')), C.byref(inertia), C.byref(changed)))
        self.assigned = True
        got['inertia'], got['changed'] = inertia.value, changed.value
        return got

    def update(self):
        """the centroids of the last assignment's labels -> the K member counts (int64)"""
        if not self.assigned:
            raise ValueError('assign comes first')
        counts = np.empty(self.K, np.int64)
        check(self.lib.l3_kmeans_update(self._handle(), _ptr(counts)))
        return counts

    def fit(self, max_iter):
        """l3_kmeans_fit -> history (n_iter, 3) float64: inertia, changed, empty of every iteration"""
        self._need_rows()
        self._need_centroids()
        if isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or not 1 <= max_iter < 2 ** 31:
            raise ValueError('max_iter must be an integer >= 1, not %r' % (max_iter,))
        history = np.zeros((int(max_iter), 3), np.float64)
        n_iter = C.c_int()
        check(self.lib.l3_kmeans_fit(self._handle(), int(max_iter), _ptr(history), C.byref(n_iter)))
        self.assigned = True
        return history[:n_iter.value].copy()

    def labels(self, outputs=('labels', 'dist')):
        """the last assignment's 'labels', 'dist' (as `outputs` names them) and 'inertia'"""
        if not self.assigned:
            raise ValueError('assign or fit comes first')
        got = {}
        if 'labels' in outputs:
            got['labels'] = np.empty(self.n, np.int32)
        if 'dist' in outputs:
            got['dist'] = np.empty(self.n, np.float32)
        inertia = C.c_double()
        check(self.lib.l3_kmeans_get_labels(self._handle(), _ptr(got.get('labels')), _ptr(got.get('dist')), C.byref(inertia)))
        got['inertia'] = inertia.value
        return got

    def centroids(self):
        self._need_centroids()
        out = np.empty((self.K, self.D), np.float32)
        check(self.lib.l3_kmeans_get_centroids(self._handle(), _ptr(out)))
        return out

    def predict(self, rows, outputs=('labels', 'dist')):
        """other rows against the current centroids -> dict of 'labels' and 'dist' as `outputs` names them"""
        self._need_centroids()
        x, n = self._rows(rows, 'other')
        got = {}
        if 'labels' in outputs:
            got['labels'] = np.empty(n, np.int32)
        if 'dist' in outputs:
            got['dist'] = np.empty(n, np.float32)
        self.n_predicted = 0
        if isinstance(x, Features):
            check(self.lib.l3_kmeans_predict_dev(self._handle(), x.h, 0, n, _ptr(got.get('labels')), _ptr(got.get('dist'))))
        else:
            check(self.lib.l3_kmeans_predict(self._handle(), _ptr(x), n, _ptr(got.get('labels')), _ptr(got.get('dist'))))
        self.n_predicted = n
        return got

    def _which(self, predicted):
        if predicted and self.n_predicted < 1:
            raise ValueError('predict comes first')
        if not predicted and not self.assigned:
            raise ValueError('assign or fit comes first')
        return (1, self.n_predicted) if predicted else (0, self.n)

    def contingency(self, classes, n_classes, predicted=False):
        """(K, n_classes) int64: the rows of every (label, class) pair; of the fitted rows, or of the last predict's"""
        which, n = self._which(predicted)
        if isinstance(n_classes, bool) or not isinstance(n_classes, (int, np.integer)) or not 1 <= n_classes <= KMEANS_MAX_CLASSES:
            raise ValueError('n_classes must be an integer in [1, %d], not %r' % (KMEANS_MAX_CLASSES, n_classes))
        cls = _index32(np.asarray(classes).reshape(-1), 'classes', n, int(n_classes), 'row')
        table = np.empty((self.K, int(n_classes)), np.int64)
        check(self.lib.l3_kmeans_contingency(self._handle(), which, _ptr(cls), int(n_classes), _ptr(table)))
        return table

    def file_hist(self, file_idxs, predicted=False):
        """(F, K) int32: the labels of each file's rows [s, e) counted per cluster"""
        which, n = self._which(predicted)
        files = _file_ranges(file_idxs, n)
        hist = np.empty((len(files), self.K), np.int32)
        check(self.lib.l3_kmeans_file_hist(self._handle(), which, _ptr(files), len(files), _ptr(hist)))
        return hist

    def time(self, what, reps=3):
        """l3_kmeans_time: device ms per round of one of KMEANS_TIMED; voids the labels"""
        if what not in KMEANS_TIMED:
            raise ValueError('what must be one of %s' % (KMEANS_TIMED,))
        self._need_rows()
        if what != 'seed':
            self._need_centroids()
        ms = C.c_double()
        self.assigned = False
        check(self.lib.l3_kmeans_time(self._handle(), KMEANS_TIMED.index(what), int(reps), C.byref(ms)))
        if what == 'seed':
            self.has_centroids = True
        return ms.value


def op_kmeans_step(X, centroids, device=0):
    """l3_op_kmeans_step: one assignment of the rows X (n, D) to the centroids (K, D) and the update that follows, by the kernels
    alone -> dict of labels (n) int32, dist (n) float32, inertia, counts (K) int64 and the new centroids (K, D)"""
    X, cen = np.asarray(X), np.asarray(centroids)
    if X.dtype != np.float32 or cen.dtype != np.float32:
        raise ValueError('the rows and the centroids must be float32 (there is no silent conversion)')
    if X.ndim != 2 or cen.ndim != 2 or X.shape[1] != cen.shape[1] or X.shape[1] < 1:
        raise ValueError('need X (n, D) and centroids (K, D) with D >= 1')
    n, D = X.shape
    K = kmeans_check_k(cen.shape[0], n)
    X, cen = np.ascontiguousarray(X), np.ascontiguousarray(cen)
    got = dict(labels=np.empty(n, np.int32), dist=np.empty(n, np.float32), counts=np.empty(K, np.int64), centroids=np.empty((K, D), np.float32))
    inertia = C.c_double()
    check(load().l3_op_kmeans_step(int(device), _ptr(X), _ptr(cen), n, K, D, _ptr(got['labels']), _ptr(got['dist']), C.byref(inertia),
                                   _ptr(got['counts']), _ptr(got['centroids'])))
    got['inertia'] = inertia.value
    return got


# ---- t-SNE maps of embedding rows (csrc/tsne.hip) ----------------------------------------------------------------------
TSNE_RUN = 256                     # L3_TSNE_RUN
TSNE_SEARCH_STEPS = 100            # L3_TSNE_SEARCH_STEPS
TSNE_MAX_POINTS = 2 ** 24
TSNE_TIMED = ('repulsive', 'attractive', 'update', 'iteration', 'pairs')


def tsne_check_n(n):
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= n <= TSNE_MAX_POINTS:
        raise ValueError('a map holds 1 to 2^24 points, not %r' % (n,))
    return int(n)


def tsne_check_perplexity(perplexity, k):
    """(perplexity as float, k as int) with 2 <= k <= KNN_TOPK_MAX and 1 < perplexity < k; ValueError otherwise"""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 2 <= k <= KNN_TOPK_MAX:
        raise ValueError('a neighbour list must hold 2 to %d entries, not %r' % (KNN_TOPK_MAX, k))
    if isinstance(perplexity, bool) or not isinstance(perplexity, (int, float, np.integer, np.floating)) or not 1.0 < perplexity < k:
        raise ValueError('perplexity must be a number with 1 < perplexity < k = %d, not %r' % (k, perplexity))
    return float(perplexity), int(k)


def tsne_check_csr(n, indptr, cols, vals):
    """a CSR matrix over n points as (int64 indptr, int32 cols, float32 vals): strictly ascending columns inside [0, n) in every row,
    no diagonal entry, values finite and >= 0; ValueError otherwise"""
    indptr, cols, vals = np.asarray(indptr), np.asarray(cols), np.asarray(vals)
    if indptr.ndim != 1 or len(indptr) != n + 1 or indptr.dtype.kind not in 'iu' or indptr[0] != 0 or np.any(np.diff(indptr) < 0):
        raise ValueError('indptr must be %d ascending integers that start at 0' % (n + 1))
    nnz = int(indptr[-1])
    if cols.ndim != 1 or len(cols) != nnz or cols.dtype.kind not in 'iu':
        raise ValueError('cols must be %d integers, one per entry' % nnz)
    if vals.dtype != np.float32 or vals.shape != (nnz,):
        raise ValueError('vals must be %d float32 values, one per entry, not %s %s' % (nnz, vals.dtype, vals.shape))
    indptr, cols = np.ascontiguousarray(indptr, np.int64), cols.astype(np.int64)
    row = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    if nnz and (cols.min() < 0 or cols.max() >= n):
        raise ValueError('a column lies outside the %d points' % n)
    if np.any(cols == row):
        raise ValueError('the affinities hold a diagonal entry (row %d)' % int(row[cols == row][0]))
    same_row = row[1:] == row[:-1]
    if np.any(same_row & (cols[1:] <= cols[:-1])):
        raise ValueError("the columns of row %d are unsorted: every row's columns ascend strictly" % int(row[1:][same_row & (cols[1:] <= cols[:-1])][0]))
    if not np.all(np.isfinite(vals)) or np.any(vals < 0):
        raise ValueError('the affinities must be finite and >= 0')
    return indptr, np.ascontiguousarray(cols, np.int32), np.ascontiguousarray(vals)


def _tsne_map(y, n, name='y'):
    y = np.asarray(y)
    if y.dtype != np.float32 or y.shape != (n, 2):
        raise ValueError('%s must be float32 of shape (%d, 2), not %s %s (the map is 2-D only)' % (name, n, y.dtype, y.shape))
    return np.ascontiguousarray(y)


def _tsne_schedule(exaggeration, momentum, learning_rate):
    ex, mom, lr = float(exaggeration), float(momentum), float(learning_rate)
    if not (np.isfinite(ex) and ex > 0 and 0 <= mom < 1 and np.isfinite(lr) and lr > 0):
        raise ValueError('need exaggeration > 0, 0 <= momentum < 1 and learning_rate > 0, not %r, %r, %r' % (exaggeration, momentum, learning_rate))
    return ex, mom, lr


def tsne_geometry(n):
    """l3_tsne_geometry -> (row_block, segments) of the repulsive pass at n points: what its bits depend on besides the points"""
    rb, seg = C.c_int(), C.c_int()
    check(load().l3_tsne_geometry(tsne_check_n(n), C.byref(rb), C.byref(seg)))
    return rb.value, seg.value


def op_tsne_conditional(dist, perplexity, device=0):
    """l3_op_tsne_conditional: (p (n, k) float64, beta (n) float64, bad_rows) of the neighbour distances dist (n, k) float32"""
    dist = np.asarray(dist)
    if dist.dtype != np.float32 or dist.ndim != 2 or dist.shape[0] < 1:
        raise ValueError('dist must be float32 of shape (n >= 1, k), not %s %s' % (dist.dtype, dist.shape))
    n = tsne_check_n(dist.shape[0])
    perplexity, k = tsne_check_perplexity(perplexity, dist.shape[1])
    dist = np.ascontiguousarray(dist)
    p, beta, bad = np.empty((n, k), np.float64), np.empty(n, np.float64), C.c_int64()
    check(load().l3_op_tsne_conditional(int(device), _ptr(dist), n, k, perplexity, _ptr(p), _ptr(beta), C.byref(bad)))
    return p, beta, bad.value


class TSNE(object):
    """RAII wrapper over an l3_tsne handle: a map of n points, its update and gains, and a CSR P resident on one device.  Every
    argument is checked here first (ValueError) and the handle is created by the first call that needs the device."""

    def __init__(self, n, device=0):
        self.n, self.device = tsne_check_n(n), int(device)
        self.lib = None
        self.h = None
        self.has_affinities = self.has_embedding = False

    def _handle(self):
        if self.h is None:
            self.lib = load()
            h = C.c_void_p()
            check(self.lib.l3_tsne_create(self.device, self.n, C.byref(h)))
            self.h = h
        return self.h

    def close(self):
        if getattr(self, 'h', None):
            self.lib.l3_tsne_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_affinities(self, indptr, cols, vals):
        indptr, cols, vals = tsne_check_csr(self.n, indptr, cols, vals)
        h = self._handle()
        self.has_affinities = False
        check(self.lib.l3_tsne_set_affinities(h, _ptr(indptr), _ptr(cols), _ptr(vals)))
        self.has_affinities = True

    def set_embedding(self, y):
        """y (n, 2) float32; the update becomes 0 and the gains 1"""
        y = _tsne_map(y, self.n)
        h = self._handle()
        self.has_embedding = False
        check(self.lib.l3_tsne_set_embedding(h, _ptr(y)))
        self.has_embedding = True

    def embedding(self):
        if not self.has_embedding:
            raise ValueError('set_embedding comes first')
        y = np.empty((self.n, 2), np.float32)
        check(self.lib.l3_tsne_get_embedding(self._handle(), _ptr(y)))
        return y

    def run(self, n_iter, exaggeration, momentum, learning_rate, kl_every=50):
        """l3_tsne_run -> records (m, 3) float64: iteration, KL, Z"""
        if not (self.has_affinities and self.has_embedding):
            raise ValueError('set_affinities and set_embedding come first')
        for name, value in (('n_iter', n_iter), ('kl_every', kl_every)):
            if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 1 <= value < 2 ** 31:
                raise ValueError('%s must be an integer >= 1, not %r' % (name, value))
        ex, mom, lr = _tsne_schedule(exaggeration, momentum, learning_rate)
        history = np.zeros((int(n_iter) // int(kl_every) + 1, 3), np.float64)
        m = C.c_int()
        try:
            check(self.lib.l3_tsne_run(self._handle(), int(n_iter), ex, mom, lr, int(kl_every), _ptr(history), C.byref(m)))
        finally:
            self.records = history[:m.value].copy()
        return self.records

    def time(self, what, reps=3):
        """l3_tsne_time: device ms per round of one of TSNE_TIMED; 'update' and 'iteration' move the map"""
        if what not in TSNE_TIMED:
            raise ValueError('what must be one of %s' % (TSNE_TIMED,))
        if not self.has_embedding or (what not in ('repulsive', 'pairs') and not self.has_affinities):
            raise ValueError('set_embedding (and set_affinities) come first')
        ms = C.c_double()
        check(self.lib.l3_tsne_time(self._handle(), TSNE_TIMED.index(what), int(reps), C.byref(ms)))
        return ms.value


def op_tsne_repulsive(y, device=0):
    """l3_op_tsne_repulsive: dict of R (n, 2), z (n) float64 and Z of the map y (n, 2) float32, by the kernels alone"""
    y = np.asarray(y)
    n = tsne_check_n(y.shape[0] if y.ndim == 2 else 0)
    y = _tsne_map(y, n)
    R, z, Z = np.empty((n, 2), np.float64), np.empty(n, np.float64), C.c_double()
    check(load().l3_op_tsne_repulsive(int(device), _ptr(y), n, _ptr(R), _ptr(z), C.byref(Z)))
    return dict(R=R, z=z, Z=Z.value)


def op_tsne_attractive(y, indptr, cols, vals, device=0):
    """l3_op_tsne_attractive: dict of A (n, 2) float64, kl_rows = sum P log1p(d^2) and plogp = sum P log P"""
    y = np.asarray(y)
    n = tsne_check_n(y.shape[0] if y.ndim == 2 else 0)
    y = _tsne_map(y, n)
    indptr, cols, vals = tsne_check_csr(n, indptr, cols, vals)
    A, kl, plogp = np.empty((n, 2), np.float64), C.c_double(), C.c_double()
    check(load().l3_op_tsne_attractive(int(device), _ptr(y), n, _ptr(indptr), _ptr(cols), _ptr(vals), _ptr(A), C.byref(kl), C.byref(plogp)))
    return dict(A=A, kl_rows=kl.value, plogp=plogp.value)


def op_tsne_update(y, update, gains, A, R, Z, exaggeration, momentum, learning_rate, device=0):
    """l3_op_tsne_update -> the new (y, update, gains), float32 (n, 2); the inputs are left as they are"""
    y = np.asarray(y)
    n = tsne_check_n(y.shape[0] if y.ndim == 2 else 0)
    y, u, g = _tsne_map(y, n).copy(), _tsne_map(update, n, 'update').copy(), _tsne_map(gains, n, 'gains').copy()
    A, R = np.asarray(A), np.asarray(R)
    if A.dtype != np.float64 or R.dtype != np.float64 or A.shape != (n, 2) or R.shape != (n, 2):
        raise ValueError('A and R must be float64 of shape (%d, 2)' % n)
    A, R = np.ascontiguousarray(A), np.ascontiguousarray(R)
    ex, mom, lr = _tsne_schedule(exaggeration, momentum, learning_rate)
    check(load().l3_op_tsne_update(int(device), n, _ptr(y), _ptr(u), _ptr(g), _ptr(A), _ptr(R), float(Z), ex, mom, lr))
    return y, u, g


# ---- principal components of embedding rows (csrc/pca.hip) --------------------------------------------------------------
PCA_CHAIN = 256                    # L3_PCA_CHAIN
PCA_MEAN_SEG = 256                 # L3_PCA_MEAN_SEG
PCA_FILL = 512                     # L3_PCA_FILL
PCA_MAX_SPLITS = 256               # L3_PCA_MAX_SPLITS
PCA_MAX_D = 16384                  # L3_PCA_MAX_D
PCA_TIMED = ('mean', 'scatter', 'transform', 'scatter_tiles')


def pca_check_d(D):
    if isinstance(D, bool) or not isinstance(D, (int, np.integer)) or not 1 <= D <= PCA_MAX_D:
        raise ValueError('D must be an integer in [1, %d], not %r' % (PCA_MAX_D, D))
    return int(D)


def pca_splits(n, D):
    """l3_pca_splits: the split count that splits=0 stands for at n rows of D features (a function of the two alone; no device)"""
    D = pca_check_d(D)
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 2 <= n <= KNN_MAX_ROWS:
        raise ValueError('n must be an integer in [2, 2^31 - 1], not %r' % (n,))
    out = C.c_int()
    check(load().l3_pca_splits(int(n), D, C.byref(out)))
    return out.value


class PCA(object):
    """RAII wrapper over an l3_pca handle: float32 rows resident on one device, their mean and scatter matrix, and a model of k
    components to project onto.  Every argument is checked here first (ValueError) and the handle is created by the first call that
    needs the device."""

    def __init__(self, D, device=0):
        self.D, self.device = pca_check_d(D), int(device)
        self.lib = None
        self.h = None
        self.n = self.k = 0
        self.has_mean = False

    def _handle(self):
        if self.h is None:
            self.lib = load()
            h = C.c_void_p()
            check(self.lib.l3_pca_create(self.device, self.D, C.byref(h)))
            self.h = h
        return self.h

    def close(self):
        if getattr(self, 'h', None):
            self.lib.l3_pca_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _rows(self, rows, width, side):
        x, n = _knn_rows(rows, width, side)
        if isinstance(x, Features) and x.device != self.device:
            raise ValueError('the %s features are on device %d, the handle on device %d' % (side, x.device, self.device))
        return x, n

    def set_rows(self, rows, lo=0, hi=None):
        """(n >= 2, D) host rows, or the rows [lo, hi) of a Features on this device -> the handle's own copy; voids the mean.  A
        row that is not finite is refused by the library (L3Error naming the row)."""
        x, n = self._rows(rows, self.D, 'fitted')
        hi = n if hi is None else int(hi)
        lo = int(lo)
        if not 0 <= lo < hi <= n:
            raise ValueError('rows [%d, %d) are empty or outside the %d rows' % (lo, hi, n))
        if hi - lo < 2:
            raise ValueError('principal components need at least 2 rows, not %d' % (hi - lo))
        h = self._handle()
        self.n, self.has_mean = 0, False
        if isinstance(x, Features):
            check(self.lib.l3_pca_set_rows_dev(h, x.h, lo, hi))
        else:
            check(self.lib.l3_pca_set_rows(h, _ptr(x[lo:hi]), hi - lo))
        self.n = hi - lo

    def _need_rows(self):
        if self.n < 2:
            raise ValueError('set_rows comes first')

    def mean(self):
        """l3_pca_mean -> (m64 (D) float64, m32 (D) float32), which the handle keeps"""
        self._need_rows()
        m64, m32 = np.empty(self.D, np.float64), np.empty(self.D, np.float32)
        self.has_mean = False
        check(self.lib.l3_pca_mean(self._handle(), _ptr(m64), _ptr(m32)))
        self.has_mean = True
        return m64, m32

    def set_mean(self, mean32):
        """the handle's m32 becomes `mean32` (D finite float32): a scatter about a mean of the caller's"""
        m = np.asarray(mean32)
        if m.dtype != np.float32 or m.shape != (self.D,) or not np.all(np.isfinite(m)):
            raise ValueError('the mean must be %d finite float32, not %s %s' % (self.D, m.dtype, m.shape))
        m = np.ascontiguousarray(m)
        self.has_mean = False
        check(self.lib.l3_pca_set_mean(self._handle(), _ptr(m)))
        self.has_mean = True

    def scatter(self, splits=0, download=True):
        """l3_pca_scatter -> S (D, D) float64, the sum over the rows of xc xc^T with xc = float32(x - m32); splits 0: pca_splits.
        download=False leaves S on the device (for Eig.set_matrix_pca) and returns None."""
        self._need_rows()
        if not self.has_mean:
            raise ValueError('the mean comes first: mean or set_mean')
        if isinstance(splits, bool) or not isinstance(splits, (int, np.integer)) or not 0 <= splits <= PCA_MAX_SPLITS:
            raise ValueError('splits must be an integer in [0, %d], not %r' % (PCA_MAX_SPLITS, splits))
        S = np.empty((self.D, self.D), np.float64) if download else None
        check(self.lib.l3_pca_scatter(self._handle(), int(splits), _ptr(S)))
        return S

    def set_model(self, mean32, components, scale=None):
        """the model to project onto: mean (D), components (k <= D, D) and scale (k, > 0) or None, all float32"""
        m, w = np.asarray(mean32), np.asarray(components)
        if m.dtype != np.float32 or m.shape != (self.D,):
            raise ValueError('the mean must be float32 of shape (%d,), not %s %s' % (self.D, m.dtype, m.shape))
        if w.dtype != np.float32 or w.ndim != 2 or w.shape[1] != self.D or not 1 <= w.shape[0] <= self.D:
            raise ValueError('the components must be float32 of shape (1 <= k <= %d, %d), not %s %s' % (self.D, self.D, w.dtype, w.shape))
        sc = None
        if scale is not None:
            sc = np.asarray(scale)
            if sc.dtype != np.float32 or sc.shape != (w.shape[0],) or not np.all(np.isfinite(sc) & (sc > 0)):
                raise ValueError('the scale must be %d positive finite float32' % w.shape[0])
            sc = np.ascontiguousarray(sc)
        m, w = np.ascontiguousarray(m), np.ascontiguousarray(w)
        h = self._handle()
        self.k = 0
        check(self.lib.l3_pca_set_model(h, w.shape[0], _ptr(m), _ptr(w), _ptr(sc)))
        self.k = w.shape[0]

    def _project(self, rows, lo, hi, to_device, forward):
        if self.k < 1:
            raise ValueError('set_model comes first')
        win, wout = (self.D, self.k) if forward else (self.k, self.D)
        x, n = self._rows(rows, win, 'projected')
        hi = n if hi is None else int(hi)
        lo = int(lo)
        if not 0 <= lo < hi <= n:
            raise ValueError('rows [%d, %d) are empty or outside the %d rows' % (lo, hi, n))
        host, dev = ((self.lib.l3_pca_transform, self.lib.l3_pca_transform_dev) if forward else
                     (self.lib.l3_pca_inverse, self.lib.l3_pca_inverse_dev))
        if not isinstance(x, Features):
            if to_device:
                raise ValueError('a result on the device needs rows on the device (a Features)')
            out = np.empty((hi - lo, wout), np.float32)
            check(host(self._handle(), _ptr(x[lo:hi]), hi - lo, _ptr(out)))
            return out
        if not to_device:
            out = np.empty((hi - lo, wout), np.float32)
            check(dev(self._handle(), x.h, lo, hi, _ptr(out), None))
            return out
        f = Features.__new__(Features)
        f.lib, f.h, f.device = self.lib, C.c_void_p(), self.device
        check(dev(self._handle(), x.h, lo, hi, None, C.byref(f.h)))
        return f

    def transform(self, rows, lo=0, hi=None, to_device=False):
        """the rows [lo, hi) of host rows or a Features (n, D) projected onto the model -> (hi - lo, k) float32, or with to_device
        (Features input only) a new Features on this device"""
        return self._project(rows, lo, hi, to_device, True)

    def inverse(self, Y, lo=0, hi=None, to_device=False):
        """the rows of the input space that the rows [lo, hi) of Y (n, k) stand for -> (hi - lo, D)"""
        return self._project(Y, lo, hi, to_device, False)

    def time(self, what, reps=3):
        """l3_pca_time: device ms per round of one of PCA_TIMED"""
        if what not in PCA_TIMED:
            raise ValueError('what must be one of %s' % (PCA_TIMED,))
        self._need_rows()
        if what == 'transform' and self.k < 1:
            raise ValueError('set_model comes first')
        if what not in ('mean', 'transform') and not self.has_mean:
            raise ValueError('the mean comes first: mean or set_mean')
        ms = C.c_double()
        check(self.lib.l3_pca_time(self._handle(), PCA_TIMED.index(what), int(reps), C.byref(ms)))
        if what == 'mean':
            self.has_mean = True
        return ms.value


# ---- symmetric top-k problems (csrc/eig.hip; DESIGN.md 8v, the subspace solver) ---------------------------------------------------------
EIG_MAX_M = 1024                   # L3_EIG_MAX_M
EIG_BLOCKS = {'V': 0, 'W': 1}      # L3_EIG_V, L3_EIG_W
EIG_TIMED = ('apply', 'gram', 'mix', 'residual')


def _eig_which(which):
    if which not in EIG_BLOCKS:
        raise ValueError("a block is 'V' or 'W', not %r" % (which,))
    return EIG_BLOCKS[which]


class Eig(object):
    """RAII wrapper over an l3_eig handle: a symmetric float64 matrix S (D, D) on one device and two blocks 'V' and 'W' of m vectors,
    the rows of (m, D) float64 matrices.  It is the `ops` of eigen.top_eigh.  Every argument is checked here first (ValueError) and
    the handle is created by the first call that needs the device."""

    def __init__(self, D, m, device=0):
        self.D = pca_check_d(D)
        if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 1 <= m <= min(self.D, EIG_MAX_M):
            raise ValueError('m must be an integer in [1, min(D, %d) = %d], not %r' % (EIG_MAX_M, min(self.D, EIG_MAX_M), m))
        self.m, self.device = int(m), int(device)
        self.lib = None
        self.h = None
        self.has_matrix = False

    def _handle(self):
        if self.h is None:
            self.lib = load()
            h = C.c_void_p()
            check(self.lib.l3_eig_create(self.device, self.D, self.m, C.byref(h)))
            self.h = h
        return self.h

    def close(self):
        if getattr(self, 'h', None):
            self.lib.l3_eig_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _square(self, M, what):
        M = np.asarray(M)
        if M.dtype != np.float64 or M.shape != (self.m, self.m):
            raise ValueError('%s must be float64 of shape (%d, %d), not %s %s' % (what, self.m, self.m, M.dtype, M.shape))
        return np.ascontiguousarray(M)

    def set_matrix(self, S):
        """S (D, D) float64 from the host; the library refuses one that is not finite or not equal to its transpose bit for bit"""
        S = np.asarray(S)
        if S.dtype != np.float64 or S.shape != (self.D, self.D):
            raise ValueError('the matrix must be float64 of shape (%d, %d), not %s %s' % (self.D, self.D, S.dtype, S.shape))
        S = np.ascontiguousarray(S)
        h = self._handle()
        self.has_matrix = False
        check(self.lib.l3_eig_set_matrix(h, _ptr(S)))
        self.has_matrix = True

    def set_matrix_pca(self, pca):
        """S = the scatter matrix that the last scatter() of the _lib.PCA `pca` left on this device: no trip through the host"""
        if not isinstance(pca, PCA):
            raise ValueError('a _lib.PCA is needed, not %r' % type(pca).__name__)
        if pca.D != self.D or pca.device != self.device:
            raise ValueError('the PCA handle has D = %d on device %d, this one D = %d on device %d' % (pca.D, pca.device, self.D, self.device))
        if not pca.h:
            raise ValueError('the PCA handle holds no scatter matrix: scatter comes first')
        h = self._handle()
        self.has_matrix = False
        check(self.lib.l3_eig_set_matrix_pca(h, pca.h))
        self.has_matrix = True

    def _need_matrix(self):
        if not self.has_matrix:
            raise ValueError('the matrix comes first: set_matrix or set_matrix_pca')

    def trace(self):
        self._need_matrix()
        t = C.c_double()
        check(self.lib.l3_eig_trace(self._handle(), C.byref(t)))
        return t.value

    def set_block(self, which, B):
        w = _eig_which(which)
        B = np.asarray(B)
        if B.dtype != np.float64 or B.shape != (self.m, self.D):
            raise ValueError('a block is float64 of shape (%d, %d), not %s %s' % (self.m, self.D, B.dtype, B.shape))
        B = np.ascontiguousarray(B)
        check(self.lib.l3_eig_set_block(self._handle(), w, _ptr(B)))

    def get_block(self, which):
        w = _eig_which(which)
        B = np.empty((self.m, self.D), np.float64)
        check(self.lib.l3_eig_get_block(self._handle(), w, _ptr(B)))
        return B

    def apply(self):
        """W_j = S V_j for every j"""
        self._need_matrix()
        check(self.lib.l3_eig_apply(self._handle()))

    def gram(self, a, b):
        """G (m, m): G[i][j] = <a_i, b_j>"""
        ia, ib = _eig_which(a), _eig_which(b)
        G = np.empty((self.m, self.m), np.float64)
        check(self.lib.l3_eig_gram(self._handle(), ia, ib, _ptr(G)))
        return G

    def mix(self, src, M, dst):
        """dst_j = sum_i M[j][i] src_i; dst may be src"""
        isrc, idst = _eig_which(src), _eig_which(dst)
        M = self._square(M, 'M')
        check(self.lib.l3_eig_mix(self._handle(), isrc, _ptr(M), idst))

    def residual(self, theta):
        """res (m): ||W_j - theta_j V_j||_2"""
        th = np.asarray(theta)
        if th.dtype != np.float64 or th.shape != (self.m,):
            raise ValueError('theta must be %d float64, not %s %s' % (self.m, th.dtype, th.shape))
        th = np.ascontiguousarray(th)
        res = np.empty(self.m, np.float64)
        check(self.lib.l3_eig_residual(self._handle(), _ptr(th), _ptr(res)))
        return res

    def time(self, what, reps=3):
        """l3_eig_time: device ms per round of one of EIG_TIMED"""
        if what not in EIG_TIMED:
            raise ValueError('what must be one of %s' % (EIG_TIMED,))
        if what == 'apply':
            self._need_matrix()
        ms = C.c_double()
        check(self.lib.l3_eig_time(self._handle(), EIG_TIMED.index(what), int(reps), C.byref(ms)))
        return ms.value


# ---- downstream MLP classifier (classifier/train.py:230-391; csrc/mlp.hip) ---------------------------------------------------------
MLP_HIDDEN = (512, 128)
MLP_MAX_CLASSES = 64
MLP_MAX_BATCH = 4096


def mlp_shapes(D, num_classes):
    """keras get_weights() order of construct_mlp_model: kernel (in, out), bias per Dense layer."""
    return [(D, 512), (512,), (512, 128), (128,), (128, num_classes), (num_classes,)]


def _i32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32)


class MLP(object):
    """RAII wrapper over an l3_mlp handle: construct_mlp_model + Adam state on one device."""

    def __init__(self, D, num_classes, batch, weight_decay=1e-5, seed=0, device=0):
        self.lib = load()
        self.D, self.C, self.batch, self.weight_decay = int(D), int(num_classes), int(batch), float(weight_decay)
        h = C.c_void_p()
        check(self.lib.l3_mlp_create(int(device), self.D, self.C, self.batch, self.weight_decay, int(seed) & (2 ** 64 - 1),
                                     C.byref(h)), None)
        self.h = h
        self.n_train = self.n_valid = 0

    def close(self):
        if getattr(self, 'h', None):
            self.lib.l3_mlp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def param_count(self):
        return int(self.lib.l3_mlp_param_count(self.h))

    def get_weights(self):
        flat = np.empty(self.param_count(), np.float32)
        check(self.lib.l3_mlp_get_weights(self.h, _ptr(flat), flat.size))
        out, o = [], 0
        for shp in mlp_shapes(self.D, self.C):
            n = int(np.prod(shp))
            out.append(flat[o:o + n].reshape(shp).copy())
            o += n
        return out

    def set_weights(self, weights):
        shapes = mlp_shapes(self.D, self.C)
        if len(weights) != len(shapes):
            raise ValueError('expected %d arrays, got %d' % (len(shapes), len(weights)))
        for w, shp in zip(weights, shapes):
            if tuple(np.shape(w)) != shp:
                raise ValueError('weight shape %s, expected %s' % (np.shape(w), shp))
        flat = np.concatenate([np.asarray(w, np.float32).ravel() for w in weights])
        check(self.lib.l3_mlp_set_weights(self.h, _ptr(flat), flat.size))

    def set_data(self, X_train, y_train, X_valid=None, y_valid=None):
        xt, yt = _f32(X_train), _i32(y_train)
        xv = _f32(X_valid) if X_valid is not None else None
        yv = _i32(y_valid) if y_valid is not None else None
        nv = 0 if xv is None else xv.shape[0]
        check(self.lib.l3_mlp_set_data(self.h, _ptr(xt), _ptr(yt), xt.shape[0], _ptr(xv), _ptr(yv), nv))
        self.n_train, self.n_valid = xt.shape[0], nv

    def epoch(self, perm, lr, t0):
        """-> dict(loss, acc, val_loss, val_acc) of one epoch over the rows in `perm` order, Adam steps t0 + 1, ..."""
        p = _i32(perm)
        if p.shape != (self.n_train,):
            raise ValueError('perm must have n_train = %d entries' % self.n_train)
        st = (C.c_double * 4)()
        check(self.lib.l3_mlp_epoch(self.h, _ptr(p), float(lr), int(t0), st))
        return dict(loss=st[0], acc=st[1], val_loss=st[2], val_acc=st[3])

    def predict(self, X):
        x = _f32(X)
        out = np.empty((x.shape[0], self.C), np.float32)
        if x.shape[0]:
            check(self.lib.l3_mlp_predict(self.h, _ptr(x), x.shape[0], _ptr(out)))
        return out

    def set_data_dev(self, train, lo, hi, y_train, valid=None, vlo=0, vhi=0, y_valid=None):
        """set_data from rows [lo, hi) of the Features `train` and rows [vlo, vhi) of `valid` (may be `train` itself), copied
        device to device; the Features may be closed afterwards"""
        yt = _i32(y_train)
        yv = _i32(y_valid) if valid is not None and vhi > vlo else None
        if yt.shape != (hi - lo,) or (yv is not None and yv.shape != (vhi - vlo,)):
            raise ValueError('one label per copied row is needed')
        check(self.lib.l3_mlp_set_data_dev(self.h, train.h, int(lo), int(hi), _ptr(yt), None if yv is None else valid.h,
                                           int(vlo), int(vhi), _ptr(yv)))
        self.n_train, self.n_valid = int(hi - lo), 0 if yv is None else int(vhi - vlo)

    def predict_dev(self, feat, lo=0, hi=None):
        """predict of rows [lo, hi) of the Features `feat`, without a trip through the host"""
        hi = feat.shape[0] if hi is None else hi
        out = np.empty((max(0, hi - lo), self.C), np.float32)
        if hi > lo:
            check(self.lib.l3_mlp_predict_dev(self.h, feat.h, int(lo), int(hi), _ptr(out)))
        return out

    def predict_files_dev(self, feat, files):
        """-> (file_mean (F, C) float32, file_pred (F,) int32): predict_dev's probabilities of the Features `feat`, kept on the
        device, reduced there over the rows [s, e) of each files entry (l3_mlp_predict_files_dev)"""
        f = _i64(files)
        if f.ndim != 2 or f.shape[1] != 2:
            raise ValueError('files must be (n_files, 2) row ranges')
        mean, pred = np.empty((f.shape[0], self.C), np.float32), np.empty(f.shape[0], np.int32)
        check(self.lib.l3_mlp_predict_files_dev(self.h, feat.h, _ptr(f), f.shape[0], _ptr(mean), _ptr(pred)))
        return mean, pred


MLP_MAX_MEMBERS = 16


class MLPGroup(object):
    """RAII wrapper over an l3_mlp_group handle: len(weight_decays) models of one shape trained on one resident data set in the
    same launches; member i equals MLP(D, num_classes, batch, weight_decays[i], seeds[i]) bit for bit."""

    def __init__(self, D, num_classes, batch, weight_decays, seeds, device=0):
        self.lib = load()
        self.D, self.C, self.batch = int(D), int(num_classes), int(batch)
        self.weight_decays = [float(w) for w in weight_decays]
        self.n_members = len(self.weight_decays)
        if len(seeds) != self.n_members:
            raise ValueError('one seed per member is needed')
        wd = np.asarray(self.weight_decays, np.float32)
        sd = np.asarray([int(s) & (2 ** 64 - 1) for s in seeds], np.uint64)
        h = C.c_void_p()
        check(self.lib.l3_mlp_group_create(int(device), self.D, self.C, self.batch, self.n_members, _ptr(wd), _ptr(sd), C.byref(h)),
              None)
        self.h = h
        self.n_train = self.n_valid = 0

    def close(self):
        if getattr(self, 'h', None):
            self.lib.l3_mlp_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def param_count(self):
        return int(self.lib.l3_mlp_group_param_count(self.h))

    def get_weights(self, member):
        flat = np.empty(self.param_count(), np.float32)
        check(self.lib.l3_mlp_group_get_weights(self.h, int(member), _ptr(flat), flat.size))
        out, o = [], 0
        for shp in mlp_shapes(self.D, self.C):
            n = int(np.prod(shp))
            out.append(flat[o:o + n].reshape(shp).copy())
            o += n
        return out

    def set_weights(self, member, weights):
        shapes = mlp_shapes(self.D, self.C)
        if [tuple(np.shape(w)) for w in weights] != shapes:
            raise ValueError('weight shapes %s, expected %s' % ([np.shape(w) for w in weights], shapes))
        flat = np.concatenate([np.asarray(w, np.float32).ravel() for w in weights])
        check(self.lib.l3_mlp_group_set_weights(self.h, int(member), _ptr(flat), flat.size))

    def set_data(self, X_train, y_train, X_valid=None, y_valid=None):
        xt, yt = _f32(X_train), _i32(y_train)
        xv = _f32(X_valid) if X_valid is not None else None
        yv = _i32(y_valid) if y_valid is not None else None
        nv = 0 if xv is None else xv.shape[0]
        check(self.lib.l3_mlp_group_set_data(self.h, _ptr(xt), _ptr(yt), xt.shape[0], _ptr(xv), _ptr(yv), nv))
        self.n_train, self.n_valid = xt.shape[0], nv

    def set_data_dev(self, train, lo, hi, y_train, valid=None, vlo=0, vhi=0, y_valid=None):
        """MLP.set_data_dev for the group: one resident copy serves every member"""
        yt = _i32(y_train)
        yv = _i32(y_valid) if valid is not None and vhi > vlo else None
        if yt.shape != (hi - lo,) or (yv is not None and yv.shape != (vhi - vlo,)):
            raise ValueError('one label per copied row is needed')
        check(self.lib.l3_mlp_group_set_data_dev(self.h, train.h, int(lo), int(hi), _ptr(yt), None if yv is None else valid.h,
                                                 int(vlo), int(vhi), _ptr(yv)))
        self.n_train, self.n_valid = int(hi - lo), 0 if yv is None else int(vhi - vlo)

    def epoch(self, perm, lrs, t0, live=None):
        """One epoch of the live members (live: one flag per member; None: all) -> one dict(loss, acc, val_loss, val_acc) per
        member, as MLP.epoch gives it; every value of a member that is not live is NaN."""
        p = _i32(perm)
        if p.shape != (self.n_train,):
            raise ValueError('perm must have n_train = %d entries' % self.n_train)
        lr = np.ascontiguousarray(lrs, dtype=np.float32)
        lv = np.ones(self.n_members, np.int32) if live is None else np.ascontiguousarray(np.asarray(live, bool), dtype=np.int32)
        if lr.shape != (self.n_members,) or lv.shape != (self.n_members,):
            raise ValueError('one learning rate and one live flag per member are needed')
        st = np.empty((self.n_members, 4), np.float64)
        check(self.lib.l3_mlp_group_epoch(self.h, _ptr(p), _ptr(lr), _ptr(lv), int(t0), _ptr(st)))
        return [dict(loss=float(s[0]), acc=float(s[1]), val_loss=float(s[2]), val_acc=float(s[3])) for s in st]

    @staticmethod
    def _mask(members):
        mask = 0
        for i in members:
            if not 0 <= int(i) < 32:
                raise ValueError('no member %r' % (i,))
            mask |= 1 << int(i)
        return mask

    def keep_best(self, members):
        """snapshot the weights of `members` (indices) on the device, each into its own slot"""
        check(self.lib.l3_mlp_group_keep_best(self.h, self._mask(members)))

    def restore_best(self, members):
        """the weights of `members` back from their slots"""
        check(self.lib.l3_mlp_group_restore_best(self.h, self._mask(members)))

    def predict(self, X):
        """-> (n_members, n, C): MLP.predict of every member in one pass"""
        x = _f32(X)
        out = np.empty((self.n_members, x.shape[0], self.C), np.float32)
        if x.shape[0]:
            check(self.lib.l3_mlp_group_predict(self.h, _ptr(x), x.shape[0], _ptr(out)))
        return out

    def predict_dev(self, feat, lo=0, hi=None):
        """-> (n_members, hi - lo, C): MLP.predict_dev of every member in one pass"""
        hi = feat.shape[0] if hi is None else hi
        out = np.empty((self.n_members, max(0, hi - lo), self.C), np.float32)
        if hi > lo:
            check(self.lib.l3_mlp_group_predict_dev(self.h, feat.h, int(lo), int(hi), _ptr(out)))
        return out

    def predict_resident(self, valid=False):
        """-> (n_members, n, C) of the rows set_data left on the device: the training rows, or with `valid` the validation rows"""
        out = np.empty((self.n_members, self.n_valid if valid else self.n_train, self.C), np.float32)
        check(self.lib.l3_mlp_group_predict_resident(self.h, int(bool(valid)), _ptr(out)))
        return out


# ---- fold preprocessing of the classifier (data/usc/features.py:52-150,243-253; csrc/featprep.hip) ---------------------------------
FEAT_CHUNK_ROWS = 256          # L3_FEAT_CHUNK_ROWS
FEAT_STATS_LDS_ROWS = 64       # L3_FEAT_STATS_LDS_ROWS


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class Features(object):
    """RAII wrapper over an l3_feat handle: one float32 (n, D) matrix on one device, replaced by each operation."""

    def __init__(self, X, device=0):
        self.lib = load()
        X = np.asarray(X)
        if X.dtype != np.float32 or X.ndim != 2:
            raise ValueError('a 2-d float32 matrix is needed, not %s of %d dimensions' % (X.dtype, X.ndim))
        x = np.ascontiguousarray(X)
        h = C.c_void_p()
        check(self.lib.l3_feat_create(int(device), _ptr(x), x.shape[0], x.shape[1], C.byref(h)), None)
        self.h = h
        self.device = int(device)

    @classmethod
    def alloc(cls, n, D, device=0):
        """A zero-filled (n, D) Features for rows the device writes (Engine.embed_audio_frames(dst=...)): l3_feat_alloc"""
        self = cls.__new__(cls)
        self.lib = load()
        h = C.c_void_p()
        check(self.lib.l3_feat_alloc(int(device), int(n), int(D), C.byref(h)), None)
        self.h = h
        self.device = int(device)
        return self

    SEGMENT = np.dtype([('src', np.uintp), ('lo', np.int64), ('hi', np.int64)])          # l3_feat_segment

    @classmethod
    def assemble(cls, segments, device=0):
        """A new Features whose rows are the rows [lo, hi) of each (Features, lo, hi) of `segments`, in order, copied on the device
        by one kernel (l3_feat_assemble).  The sources stay as they are."""
        segments = list(segments)
        table = np.zeros(len(segments), cls.SEGMENT)
        for i, (src, lo, hi) in enumerate(segments):
            if not isinstance(src, cls) or not src.h:
                raise ValueError('segment %d: the source must be an open Features' % i)
            table[i] = (src.h.value, int(lo), int(hi))
        self = cls.__new__(cls)
        self.lib = load()
        h = C.c_void_p()
        check(self.lib.l3_feat_assemble(int(device), _ptr(table), len(segments), C.byref(h)), None)
        self.h = h
        self.device = int(device)
        return self

    def close(self):
        if getattr(self, 'h', None):
            self.lib.l3_feat_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def shape(self):
        n, d = C.c_int64(), C.c_int64()
        check(self.lib.l3_feat_shape(self.h, C.byref(n), C.byref(d)))
        return (n.value, d.value)

    def download(self, lo=0, hi=None):
        n, d = self.shape
        hi = n if hi is None else hi
        out = np.empty((max(0, hi - lo), d), np.float32)
        check(self.lib.l3_feat_download(self.h, int(lo), int(hi), _ptr(out)))
        return out

    def gather(self, rows):
        r = _i64(rows)
        check(self.lib.l3_feat_gather(self.h, _ptr(r), r.size))

    def split(self, rows_a, rows_b=None):
        """X[rows_a] and X[rows_b] as two new Features on this device, written by one kernel (l3_feat_split); this matrix stays as
        it is.  rows_b None (or empty): a plain out-of-place take -> (Features, None)."""
        a = _i64(rows_a).reshape(-1)
        b = None if rows_b is None else _i64(rows_b).reshape(-1)
        if b is not None and b.size == 0:
            b = None
        out = []
        for _ in range(1 if b is None else 2):
            part = type(self).__new__(type(self))
            part.lib, part.h, part.device = self.lib, C.c_void_p(), self.device
            out.append(part)
        check(self.lib.l3_feat_split(self.h, _ptr(a), a.size, _ptr(b), 0 if b is None else b.size, C.byref(out[0].h),
                                     C.byref(out[1].h) if b is not None else None))
        return out[0], (out[1] if b is not None else None)

    def minmax(self):
        d = self.shape[1]
        lo, hi = np.empty(d, np.float32), np.empty(d, np.float32)
        check(self.lib.l3_feat_minmax(self.h, _ptr(lo), _ptr(hi)))
        return lo, hi

    def affine32(self, scale, shift):
        a, b = _f32(scale), _f32(shift)
        if a.shape != (self.shape[1],) or b.shape != a.shape:
            raise ValueError('scale and shift need one entry per column')
        check(self.lib.l3_feat_affine32(self.h, _ptr(a), _ptr(b)))

    def moments(self):
        d = self.shape[1]
        mean, var = np.empty(d, np.float64), np.empty(d, np.float64)
        check(self.lib.l3_feat_moments(self.h, _ptr(mean), _ptr(var)))
        return mean, var

    def standardize(self, mean, scale):
        a, b = _f64(mean), _f64(scale)
        if a.shape != (self.shape[1],) or b.shape != a.shape:
            raise ValueError('mean and scale need one entry per column')
        check(self.lib.l3_feat_standardize(self.h, _ptr(a), _ptr(b)))

    def file_stats(self, file_idxs):
        f = _i64(file_idxs)
        if f.ndim != 2 or f.shape[1] != 2:
            raise ValueError('file_idxs must be (n_files, 2) row ranges')
        check(self.lib.l3_feat_file_stats(self.h, _ptr(f), f.shape[0]))


def op_file_mean(probs, files, device=0):
    """l3_op_file_mean: probs (n, C) float32, files (F, 2) row ranges -> (file_mean (F, C) float32, file_pred (F,) int32)"""
    p = _f32(probs)
    f = _i64(files).reshape(-1, 2)
    mean, pred = np.empty((f.shape[0], p.shape[1]), np.float32), np.empty(f.shape[0], np.int32)
    check(load().l3_op_file_mean(int(device), _ptr(p), p.shape[0], p.shape[1], _ptr(f), f.shape[0], _ptr(mean), _ptr(pred)))
    return mean, pred


def op_mlp_dense_fwd(x, w, b, idx=None, relu=True, device=0):
    x, w, b = _f32(x), _f32(w), _f32(b)
    idx = _i32(idx)
    rows = x.shape[0] if idx is None else idx.shape[0]
    K, N = w.shape
    y = np.empty((rows, N), np.float32)
    check(load().l3_op_mlp_dense_fwd(device, _ptr(x), x.shape[0], _ptr(idx), rows, K, N, _ptr(w), _ptr(b), int(bool(relu)),
                                     _ptr(y)))
    return y


def op_mlp_dense_bwd_x(dy, w, h=None, device=0):
    dy, w, h = _f32(dy), _f32(w), _f32(h)
    K, N = w.shape
    dx = np.empty((dy.shape[0], K), np.float32)
    check(load().l3_op_mlp_dense_bwd_x(device, _ptr(dy), _ptr(w), _ptr(h), dy.shape[0], K, N, _ptr(dx)))
    return dx


def op_mlp_wgrad(x, dy, idx=None, device=0):
    x, dy, idx = _f32(x), _f32(dy), _i32(idx)
    rows, N = dy.shape
    K = x.shape[1]
    dw, db = np.empty((K, N), np.float32), np.empty(N, np.float32)
    check(load().l3_op_mlp_wgrad(device, _ptr(x), x.shape[0], _ptr(idx), rows, K, N, _ptr(dy), _ptr(dw), _ptr(db)))
    return dw, db


def op_mlp_wgrad_adam(x, dy, w, b, mw, vw, mb, vb, weight_decay, lr_t, idx=None, device=0):
    """-> (w, b, mw, vw, mb, vb) after one fused step, sum of the pre-update w^2"""
    x, dy, idx = _f32(x), _f32(dy), _i32(idx)
    st = [np.array(a, np.float32, copy=True, order='C') for a in (w, b, mw, vw, mb, vb)]
    rows, N = dy.shape
    K = x.shape[1]
    w2 = np.zeros(1, np.float32)
    check(load().l3_op_mlp_wgrad_adam(device, _ptr(x), x.shape[0], _ptr(idx), rows, K, N, _ptr(dy), *[_ptr(a) for a in st],
                                      float(weight_decay), float(lr_t), _ptr(w2)))
    return tuple(st), float(w2[0])


def op_mlp_softmax_ce(z, labels, gscale=None, device=0):
    """-> probs, dz, per-row ce, per-row correct (0/1); gscale defaults to keras' mean, 1 / rows"""
    z, labels = _f32(z), _i32(labels)
    rows, Cn = z.shape
    probs, dz = np.empty_like(z), np.empty_like(z)
    ce, cor = np.empty(rows, np.float32), np.empty(rows, np.float32)
    g = 1.0 / rows if gscale is None else gscale
    check(load().l3_op_mlp_softmax_ce(device, _ptr(z), _ptr(labels), rows, Cn, float(g), _ptr(probs), _ptr(dz), _ptr(ce),
                                      _ptr(cor)))
    return probs, dz, ce, cor


def op_adam(p, g, m, v, n_l2, l2x2, lr_t, device=0):
    """The engine's Adam kernel on flat arrays -> (p, m, v)"""
    p, m, v = [np.array(a, np.float32, copy=True).ravel() for a in (p, m, v)]
    g = _f32(g).ravel()
    check(load().l3_op_adam(device, _ptr(p), _ptr(g), _ptr(m), _ptr(v), p.size, int(n_l2), float(l2x2), float(lr_t)))
    return p, m, v


def op_arena_fold(acc, g, off, n, mode, device=0):
    """The gradient fold of step_replicas on elements [off, off + n) of two arenas: mode 'set' acc = g, 'add' acc += g, 'out'
    g = acc + g.  Returns the two arenas as the device left them."""
    a, b = _f32(acc).copy(), _f32(g).copy()
    assert a.shape == b.shape and a.ndim == 1
    check(load().l3_op_arena_fold(device, _ptr(a), _ptr(b), a.size, int(off), int(n), {'set': 0, 'add': 1, 'out': 2}[mode]))
    return a, b


def op_adam_scaled(p, g, m, v, n_l2, l2x2, lr_t, b1=0.9, b2=0.999, eps=1e-8, gscale=1.0, device=0):
    """The engine's Adam kernel with every scalar of its launch (g * gscale before the L2 term) -> (p, m, v)"""
    p, m, v = [np.array(a, np.float32, copy=True).ravel() for a in (p, m, v)]
    g = _f32(g).ravel()
    check(load().l3_op_adam_scaled(device, _ptr(p), _ptr(g), _ptr(m), _ptr(v), p.size, int(n_l2), float(l2x2), float(lr_t),
                                   float(b1), float(b2), float(eps), float(gscale)))
    return p, m, v


# ---- the engine's head, loss, L2 sums and BatchNorm moving averages on their own (csrc/elementwise.hip) ---------------------------
def op_head_dense_fwd(x, w, b, relu, device=0):
    """y (B, N) = x (B, K) . w (K, N) + b, ReLU when `relu`: the engine's dense_fwd launch"""
    x, w, b = _f32(x), _f32(w), _f32(b)
    (B, K), N = x.shape, w.shape[1]
    assert w.shape == (K, N) and b.shape == (N,)
    y = np.empty((B, N), np.float32)
    check(load().l3_op_head_dense_fwd(device, _ptr(x), _ptr(w), _ptr(b), _ptr(y), B, K, N, int(bool(relu))))
    return y


def op_head_dense_bwd(x, w, dy, device=0):
    """-> dw (K, N), db (N), dx (B, K): the engine's dense_bwd_w and dense_bwd_x launches"""
    x, w, dy = _f32(x), _f32(w), _f32(dy)
    (B, K), N = x.shape, w.shape[1]
    assert w.shape == (K, N) and dy.shape == (B, N)
    dw, db, dx = np.empty((K, N), np.float32), np.empty(N, np.float32), np.empty((B, K), np.float32)
    check(load().l3_op_head_dense_bwd(device, _ptr(x), _ptr(w), _ptr(dy), _ptr(dw), _ptr(db), _ptr(dx), B, K, N))
    return dw, db, dx


def op_softmax_ce2(logits, labels, gscale, device=0):
    """The engine's two-class loss: logits, float labels (B, 2) -> probs, dlogits, sum of the losses, correct rows"""
    z, t = _f32(logits), _f32(labels)
    assert z.ndim == 2 and z.shape[1] == 2 and t.shape == z.shape
    probs, dz, stats = np.empty_like(z), np.empty_like(z), np.empty(2, np.float32)
    check(load().l3_op_softmax_ce2(device, _ptr(z), _ptr(t), z.shape[0], float(gscale), _ptr(probs), _ptr(dz), _ptr(stats)))
    return probs, dz, stats[0], stats[1]


def op_sumsq(base, off, n, multi, device=0):
    """Sums of squares of the ranges [off[i], off[i] + n[i]) of `base`: one sumsq_multi call (multi) or one sumsq call each"""
    base, off, n = _f32(base).ravel(), _i64(off).ravel(), _i64(n).ravel()
    assert off.size == n.size
    out = np.empty(off.size, np.float32)
    check(load().l3_op_sumsq(device, _ptr(base), base.size, _ptr(off), _ptr(n), off.size, int(bool(multi)), _ptr(out)))
    return out


def op_bn_moving_update(c, slot_off, moving, biased, batch, momentum, zero_debias, step, gathered=None, replicas=1, stride=0,
                        packed=None, device=0):
    """One bn_moving_update_all launch over a table of len(c) statistics (entry i: c[i] channels at slot_off[i] of moving /
    biased / batch), and bn_moving_pack of the same table into `packed` -> (moving, biased, packed), copies."""
    c, slot_off = _i32(c).ravel(), _i64(slot_off).ravel()
    moving, biased = [np.array(a, np.float32, copy=True).ravel() for a in (moving, biased)]
    batch = _f32(batch).ravel()
    assert c.size == slot_off.size and moving.size == biased.size == batch.size
    packed = np.zeros(int(c.sum()), np.float32) if packed is None else np.array(packed, np.float32, copy=True).ravel()
    g = None if gathered is None else _f32(gathered).ravel()
    check(load().l3_op_bn_moving_update(device, c.size, _ptr(c), _ptr(slot_off), moving.size, _ptr(moving), _ptr(biased),
                                        _ptr(batch), _ptr(g), 0 if g is None else g.size, int(replicas), int(stride),
                                        float(momentum), int(bool(zero_debias)), int(step), _ptr(packed), packed.size))
    return moving, biased, packed


# ---- downstream SVM classifier (classifier/train.py:79-166; csrc/svm.hip) ---------------------------------------------------------
SVM_KERNELS = {'linear': 0, 'poly': 1, 'rbf': 2, 'sigmoid': 3}     # L3_SVM_* (libsvm's kernel_type order)
SVM_MAX_CLASSES = 64
SVM_MAX_WS = 128


class SvmKernel(C.Structure):
    _fields_ = [('kind', C.c_int32), ('degree', C.c_int32), ('gamma', C.c_double), ('coef0', C.c_double)]


def svm_kernel(kernel, gamma=0.0, coef0=0.0, degree=3):
    if kernel not in SVM_KERNELS:
        raise ValueError('kernel must be one of %s, not %r' % (sorted(SVM_KERNELS), kernel))
    return SvmKernel(SVM_KERNELS[kernel], int(degree), float(gamma), float(coef0))


def _svm_score_io(n, ncls, labels, files, outputs, extra):
    """labels and file ranges as the C ABI takes them, the output arrays `outputs` names and the pointer list of l3_svm_score
    (`extra` = ('pair_proba', 'iters'): of l3_op_svm_tail), NULL where an output is not wanted"""
    lab = None if labels is None else _i32(labels).reshape(-1)
    if lab is not None and lab.size != n:
        raise ValueError('one label per row is needed')
    fl = None if files is None else _i64(files).reshape(-1, 2)
    nf = 0 if fl is None else fl.shape[0]
    P = ncls * (ncls - 1) // 2
    shapes = {'pred': ((n,), np.int32), 'ovr': ((n,) if ncls == 2 else (n, ncls), np.float64), 'hinge_sum': ((1,), np.float64),
              'pair_proba': ((n, P), np.float64), 'proba': ((n, ncls), np.float64), 'file_proba': ((nf, ncls), np.float64),
              'file_pred': ((nf,), np.int32), 'iters': ((n,), np.int32)}
    order = [k for k in ('pred', 'ovr', 'hinge_sum', 'pair_proba', 'proba', 'file_proba', 'file_pred', 'iters')
             if k in extra or k not in ('pair_proba', 'iters')]
    unknown = set(outputs) - set(order)
    if unknown:
        raise ValueError('unknown outputs %s' % sorted(unknown))
    out = {k: np.empty(*shapes[k]) for k in outputs}
    return lab, fl, out, [_ptr(out.get(k)) for k in order]


def _svm_score_result(out):
    if 'hinge_sum' in out:
        out['hinge_sum'] = float(out['hinge_sum'][0])
    return out


class SVM(object):
    """RAII wrapper over an l3_svm handle: the resident training matrix and the batched binary solver on one device."""

    def __init__(self, device=0):
        self.lib = load()
        h = C.c_void_p()
        check(self.lib.l3_svm_create(int(device), C.byref(h)), None)
        self.h = h
        self.n = self.D = 0

    def close(self):
        if getattr(self, 'h', None):
            self.lib.l3_svm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_data(self, X):
        x = _f32(X)
        check(self.lib.l3_svm_set_data(self.h, _ptr(x), x.shape[0], x.shape[1]))
        self.n, self.D = x.shape

    def fit(self, kernel, problems, cost=1.0, tol=1e-3, max_iter=-1, q=0):
        """problems: list of (rows, signs) over the set_data rows; cost: the box bound C, one for all or one per problem.
        -> (alphas (list of float64 arrays), rho (P,), updates (P,), outer iterations (P,), last gaps (P,))"""
        rows = [np.ascontiguousarray(r, np.int32) for r, _ in problems]
        off = np.zeros(len(rows) + 1, np.int64)
        off[1:] = np.cumsum([r.size for r in rows])
        r_all = np.concatenate(rows) if rows else np.zeros(0, np.int32)
        s_all = np.concatenate([np.asarray(s, np.int8) for _, s in problems]) if rows else np.zeros(0, np.int8)
        P = len(rows)
        alpha, rho = np.empty(int(off[-1]), np.float64), np.empty(P, np.float64)
        upd, outer, gap = np.empty(P, np.int64), np.empty(P, np.int32), np.empty(P, np.float64)
        tail = (float(tol), int(max_iter), P, _ptr(off), _ptr(r_all), _ptr(s_all), int(q), _ptr(alpha), _ptr(rho), _ptr(upd),
                _ptr(outer), _ptr(gap))
        if np.ndim(cost) == 0:
            check(self.lib.l3_svm_fit(self.h, C.byref(kernel), float(cost), *tail))
        else:
            costs = _f64(cost).reshape(-1)
            if costs.size != P:
                raise ValueError('cost must be a scalar or hold one value per problem (%d), not %d' % (P, costs.size))
            check(self.lib.l3_svm_fit_costs(self.h, C.byref(kernel), _ptr(costs), *tail))
        return [alpha[off[p]:off[p + 1]] for p in range(P)], rho, upd, outer, gap

    def cv_decision(self, kernel, jobs):
        """the held-out decision values of binary models, all in one launch (l3_svm_cv_decision).  jobs: a list of
        (held, sv, n_pos, coef, rho): resident rows to score, resident rows of the support vectors (the n_pos positives first),
        one coefficient per support vector, the model's rho.  -> a list of float64 arrays, one value per held-out row"""
        J = len(jobs)
        if J == 0:
            return []
        held = [_i32(j[0]).reshape(-1) for j in jobs]
        sv = [_i32(j[1]).reshape(-1) for j in jobs]
        coef = [_f64(j[3]).reshape(-1) for j in jobs]
        if any(c.size != v.size for c, v in zip(coef, sv)):
            raise ValueError('one coefficient per support vector is needed')
        hoff, soff = np.zeros(J + 1, np.int64), np.zeros(J + 1, np.int64)
        hoff[1:] = np.cumsum([a.size for a in held])
        soff[1:] = np.cumsum([a.size for a in sv])
        neg = _i64([int(j[2]) for j in jobs])
        rho = _f64([float(j[4]) for j in jobs])
        # a buffer of at least one element, so that no pointer is NULL when every job is empty on that side
        cat = lambda parts, dt: np.concatenate(parts + [np.zeros(1, dt)])
        out = np.empty(int(hoff[-1]) + 1, np.float64)
        check(self.lib.l3_svm_cv_decision(self.h, C.byref(kernel), J, _ptr(hoff), _ptr(cat(held, np.int32)), _ptr(soff), _ptr(neg),
                                          _ptr(cat(sv, np.int32)), _ptr(cat(coef, np.float64)), _ptr(rho), _ptr(out)))
        return [out[hoff[j]:hoff[j + 1]] for j in range(J)]

    def decision(self, kernel, sv_start, coef, rho, X=None, x_idx=None, SV=None, sv_idx=None):
        """libsvm's pairwise decision values (n, n_class (n_class - 1) / 2) of host rows X or resident rows x_idx, against
        support vectors SV (host) or sv_idx (resident), grouped by class as sv_start says."""
        cs = np.ascontiguousarray(sv_start, np.int64)
        ncls = cs.size - 1
        cf = np.ascontiguousarray(coef, np.float64).reshape(ncls - 1, -1)
        rh = np.ascontiguousarray(rho, np.float64).reshape(-1)
        x, xi = _f32(X), _i32(x_idx)
        sv, si = _f32(SV), _i32(sv_idx)
        n = x.shape[0] if x is not None else xi.size
        D = x.shape[1] if x is not None else (sv.shape[1] if sv is not None else self.D)
        if sv is not None and sv.size == 0:
            sv = np.zeros((1, D), np.float32)
        if si is not None and si.size == 0:
            si = np.zeros(1, np.int32)
        out = np.empty((n, ncls * (ncls - 1) // 2), np.float64)
        if n == 0:
            return out
        check(self.lib.l3_svm_decision(self.h, C.byref(kernel), _ptr(x), _ptr(xi), n, int(D), _ptr(sv), _ptr(si), int(cs[-1]), ncls,
                                       _ptr(cs), _ptr(cf), _ptr(rh), _ptr(out)))
        return out

    def set_data_dev(self, feat, lo=0, hi=None):
        """set_data from rows [lo, hi) of the Features `feat`, copied device to device; it may be closed afterwards"""
        n, d = feat.shape
        hi = n if hi is None else hi
        check(self.lib.l3_svm_set_data_dev(self.h, feat.h, int(lo), int(hi)))
        self.n, self.D = int(hi - lo), int(d)

    def get_rows(self, idx):
        """rows idx of the resident matrix -> (len(idx), D) float32"""
        i = _i32(idx).reshape(-1)
        out = np.empty((i.size, self.D), np.float32)
        if i.size:
            check(self.lib.l3_svm_get_rows(self.h, _ptr(i), i.size, _ptr(out)))
        return out

    def set_model(self, kernel, sv_start, coef, rho, SV=None, sv_idx=None, probA=None, probB=None):
        """the resident model of score(): arguments as decision(), and Platt's (A, B) per pair or neither"""
        cs = np.ascontiguousarray(sv_start, np.int64)
        ncls = cs.size - 1
        cf = np.ascontiguousarray(coef, np.float64).reshape(ncls - 1, -1)
        rh = np.ascontiguousarray(rho, np.float64).reshape(-1)
        if rh.size != ncls * (ncls - 1) // 2 or cf.shape[1] != cs[-1]:
            raise ValueError('coef must be (n_class - 1, n_sv) and rho one per pair')
        sv, si = _f32(SV), _i32(sv_idx)
        D = sv.shape[1] if sv is not None else self.D
        if sv is not None and sv.size == 0:
            sv = np.zeros((1, D), np.float32)
        if si is not None and si.size == 0:
            si = np.zeros(1, np.int32)
        pa = None if probA is None else _f64(probA).reshape(-1)
        pb = None if probB is None else _f64(probB).reshape(-1)
        if (pa is None) != (pb is None) or (pa is not None and (pa.size != rh.size or pb.size != rh.size)):
            raise ValueError('probA and probB come together, one entry per pair')
        check(self.lib.l3_svm_set_model(self.h, C.byref(kernel), _ptr(sv), _ptr(si), int(cs[-1]), int(D), ncls, _ptr(cs), _ptr(cf),
                                        _ptr(rh), _ptr(pa), _ptr(pb)))
        self.model_classes, self.model_D = ncls, int(D)

    def score(self, X=None, x_idx=None, feat=None, lo=0, hi=None, labels=None, files=None,
              outputs=('pred', 'ovr', 'hinge_sum', 'proba', 'file_proba', 'file_pred')):
        """one scoring pass with the resident model over host rows X, resident rows x_idx or rows [lo, hi) of the Features `feat`
        -> dict of the named outputs (l3_svm_score)"""
        if (X is not None) + (x_idx is not None) + (feat is not None) != 1:
            raise ValueError('give rows as exactly one of X, x_idx or feat')
        if not getattr(self, 'model_classes', 0):
            raise L3Error('l3_svm_score: no model (set_model)')
        ncls = self.model_classes
        x, xi = _f32(X), _i32(x_idx)
        if feat is not None:
            hi = feat.shape[0] if hi is None else hi
            n, D = int(hi - lo), self.model_D
        else:
            n = x.shape[0] if x is not None else xi.size
            D = x.shape[1] if x is not None else self.D
            lo = hi = 0
        lab, fl, out, ptrs = _svm_score_io(n, ncls, labels, files, outputs, ())
        check(self.lib.l3_svm_score(self.h, _ptr(x), _ptr(xi), None if feat is None else feat.h, int(lo), int(hi), n, int(D), _ptr(lab),
                                    _ptr(fl), 0 if fl is None else fl.shape[0], *ptrs))
        return _svm_score_result(out)


def op_svm_kernel_rows(x, a_idx, b_idx, kernel='rbf', gamma=0.0, coef0=0.0, degree=3, device=0):
    """(len(a_idx), len(b_idx)) float32: k(x[a], x[b]) through the solver's kernel-row launch"""
    x, a, b = _f32(x), _i32(a_idx), _i32(b_idx)
    out = np.empty((a.size, b.size), np.float32)
    kp = svm_kernel(kernel, gamma, coef0, degree)
    check(load().l3_op_svm_kernel_rows(device, C.byref(kp), _ptr(x), x.shape[0], x.shape[1], _ptr(a), a.size, _ptr(b), b.size,
                                       _ptr(out)))
    return out


def op_svm_smo(K, y, alpha, grad, cost=1.0, eps=1e-3, local_rel=0.0, max_updates=-1, device=0):
    """one local SMO solve on the GPU (box [0, cost]) -> (alpha, updates)"""
    K = _f32(K)
    y = np.ascontiguousarray(y, np.int8)
    a = np.array(alpha, np.float64, copy=True)
    g = np.ascontiguousarray(grad, np.float64)
    u = np.zeros(1, np.int64)
    check(load().l3_op_svm_smo(device, _ptr(K), _ptr(y), y.size, float(cost), float(eps), float(local_rel), int(max_updates), _ptr(a),
                               _ptr(g), _ptr(u)))
    return a, int(u[0])


def svm_sigmoid_train(device, decs, signs):
    """svm.cpp sigmoid_train for every (decision values, +1 / -1 labels) pair of the two lists in one launch
    (l3_op_svm_sigmoid_train) -> (A, B, iters), one entry per pair"""
    decs = [_f64(d).reshape(-1) for d in decs]
    signs = [np.ascontiguousarray(v, np.int8).reshape(-1) for v in signs]
    J = len(decs)
    if len(signs) != J or any(d.size != v.size for d, v in zip(decs, signs)):
        raise ValueError('one label per decision value is needed')
    A, B, it = np.empty(J), np.empty(J), np.empty(J, np.int32)
    if J == 0:
        return A, B, it
    off = np.zeros(J + 1, np.int64)
    off[1:] = np.cumsum([d.size for d in decs])
    check(load().l3_op_svm_sigmoid_train(int(device), J, _ptr(off), _ptr(np.concatenate(decs)), _ptr(np.concatenate(signs)),
                                         _ptr(A), _ptr(B), _ptr(it)))
    return A, B, it


def op_svm_tail(dec, n_classes, probA=None, probB=None, labels=None, files=None,
                outputs=('pred', 'ovr', 'hinge_sum', 'pair_proba', 'proba', 'file_proba', 'file_pred', 'iters'), device=0):
    """the scoring kernels (csrc/svm_eval.hip) on a host block of pair decisions (n, P) -> dict of the named outputs"""
    ncls = int(n_classes)
    P = ncls * (ncls - 1) // 2
    dec = _f64(dec).reshape(-1, P)
    n = dec.shape[0]
    pa = None if probA is None else _f64(probA).reshape(-1)
    pb = None if probB is None else _f64(probB).reshape(-1)
    if (pa is not None and pa.size != P) or (pb is not None and pb.size != P):
        raise ValueError('probA and probB hold one entry per pair')
    lab, fl, out, ptrs = _svm_score_io(n, ncls, labels, files, outputs, ('pair_proba', 'iters'))
    check(load().l3_op_svm_tail(int(device), _ptr(dec), n, ncls, _ptr(pa), _ptr(pb), _ptr(lab), _ptr(fl),
                                0 if fl is None else fl.shape[0], *ptrs))
    return _svm_score_result(out)


# ---- VGGish baseline features (csrc/vggish.hip; data/usc/features.py:166-240) -----------------------------------------------------
VGGISH_CONV = {'f4x4': 0, 'f2x2': 1, 'direct': 3}
VGGISH_POSTPROCESS = {'raw': 0, 'pca': 1, 'quantized': 2}


def _i64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int64)


class VGGish(object):
    """RAII wrapper over an l3_vggish handle: the network's weights and the activation buffers of one example batch."""

    def __init__(self, batch=0, device=0):
        self.lib = load()
        h = C.c_void_p()
        check(self.lib.l3_vggish_create(int(device), int(batch), C.byref(h)), None)
        self.h = h
        self.batch = int(self.lib.l3_vggish_batch(h))

    def close(self):
        if getattr(self, 'h', None):
            self.lib.l3_vggish_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_conv(self, algo):
        check(self.lib.l3_vggish_set_conv(self.h, VGGISH_CONV[algo]))

    def set_weight(self, name, value):
        a = _f32(value)
        check(self.lib.l3_vggish_set_weight(self.h, name.encode(), _ptr(a), a.size))

    def set_pca(self, pca_matrix, pca_means):
        m, mu = _f32(pca_matrix), _f32(np.asarray(pca_means).reshape(-1))
        if m.shape != (128, 128) or mu.shape != (128,):
            raise ValueError('PCA parameters must be (128, 128) and (128,), got %s and %s' % (m.shape, mu.shape))
        check(self.lib.l3_vggish_set_pca(self.h, _ptr(m), _ptr(mu)))

    def embed_clips_resampled(self, native, clips, half_window, num_table, n_samples, segments, example_rows, postprocess='quantized'):
        """native: the clips at their own rates back to back; clips (n, 6) int64 rows {x_off, L, sr_orig, t0, n_out, y_off} into a
        16 kHz buffer of n_samples; segments (n, 2) int64 {offset, length} of that buffer; example_rows: first log-mel row of each
        example -> (n_examples, 128) float32"""
        x, c, w = _f32(native).reshape(-1), _i64(clips).reshape(-1, 6), np.ascontiguousarray(half_window, np.float64).reshape(-1)
        sg, ex = _i64(segments).reshape(-1, 2), _i64(example_rows).reshape(-1)
        out = np.empty((ex.size, 128), np.float32)
        check(self.lib.l3_vggish_embed_clips_resampled(self.h, _ptr(x), x.size, _ptr(c), c.shape[0], _ptr(w), w.size, int(num_table),
                                                       int(n_samples), _ptr(sg), sg.shape[0], _ptr(ex), ex.size,
                                                       VGGISH_POSTPROCESS[postprocess], _ptr(out)))
        return out


def vggish_logmel_rows(lengths):
    """log-mel rows of segments of these lengths: 1 + (n - 400) // 160, none below 400 samples"""
    n = np.asarray(lengths, np.int64)
    return np.where(n < 400, 0, 1 + (np.maximum(n, 400) - 400) // 160)


def op_vggish_logmel(x, segments=None, device=0):
    """(rows, 64) float32 log-mel of x, or of its segments {offset, length} back to back"""
    x = _f32(x).reshape(-1)
    sg = _i64([[0, x.size]] if segments is None else segments).reshape(-1, 2)
    out = np.empty((int(vggish_logmel_rows(sg[:, 1]).sum()), 64), np.float32)
    check(load().l3_op_vggish_logmel(device, _ptr(x), x.size, _ptr(sg), sg.shape[0], _ptr(out)))
    return out


def op_vggish_conv1(logmel, example_rows, w, b, device=0):
    lm, ex, w, b = _f32(logmel), _i64(example_rows).reshape(-1), _f32(w), _f32(b)
    assert lm.ndim == 2 and lm.shape[1] == 64 and w.size == 9 * 64 and b.size == 64
    y = np.empty((ex.size, 48, 32, 64), np.float32)
    check(load().l3_op_vggish_conv1(device, _ptr(lm), lm.shape[0], _ptr(ex), ex.size, _ptr(w), _ptr(b), _ptr(y)))
    return y


def op_vggish_bias_relu(x, b, pool, device=0):
    x, b = _f32(x), _f32(b)
    n, h, w, c = x.shape
    y = np.empty((n, h // 2, w // 2, c) if pool else x.shape, np.float32)
    check(load().l3_op_vggish_bias_relu(device, _ptr(x), _ptr(b), _ptr(y), n, h, w, c, 1 if pool else 0))
    return y


def op_vggish_conv(x, w, b, pool, algo, device=0):
    """one wide VGGish convolution as the handle runs it under `algo` ('f4x4', 'f2x2', 'direct') + bias, ReLU (+ 2x2 pool)"""
    x, w, b = _f32(x), _f32(w), _f32(b)
    n, h, wd, cin = x.shape
    cout = w.shape[3]
    y = np.empty((n, h // 2, wd // 2, cout) if pool else (n, h, wd, cout), np.float32)
    check(load().l3_op_vggish_conv(device, VGGISH_CONV[algo], _ptr(x), _ptr(w), _ptr(b), _ptr(y), n, h, wd, cin, cout,
                                   1 if pool else 0))
    return y


def op_vggish_postprocess(emb, pca_matrix, pca_means, quantize=True, device=0):
    e, m, mu = _f32(emb), _f32(pca_matrix), _f32(np.asarray(pca_means).reshape(-1))
    assert e.ndim == 2 and e.shape[1] == 128 and m.shape == (128, 128) and mu.shape == (128,)
    out = np.empty_like(e)
    check(load().l3_op_vggish_postprocess(device, _ptr(e), e.shape[0], _ptr(m), _ptr(mu), 1 if quantize else 0, _ptr(out)))
    return out


# ---- downstream random forest (csrc/forest.hip) ------------------------------------------------------------------------------------
FOREST_MAX_CLASSES = 60          # L3_FOREST_MAX_CLASSES
FOREST_MAX_CUTS = 255            # L3_FOREST_MAX_CUTS
FOREST_MAX_DRAWS = 256           # L3_FOREST_MAX_DRAWS
FOREST_MAX_BIN_SAMPLE = 8192     # L3_FOREST_MAX_BIN_SAMPLE
FOREST_NARROW_ROWS = 64          # L3_FOREST_NARROW_ROWS
FOREST_SCORE_OUTPUTS = ('pred', 'correct', 'file_mean', 'file_pred', 'proba')          # l3_forest_score's, in its order
FOREST_OOB_OUTPUTS = ('pred', 'correct', 'n_oob', 'sums')          # l3_forest_oob's, in its order
FOREST_TREE_ARRAYS = ('tree_off', 'left', 'right', 'feature', 'threshold', 'bin', 'counts', 'n_distinct')


class ForestConfig(C.Structure):
    """struct l3_forest_config (include/l3hip.h)"""
    _fields_ = [('n_classes', C.c_int32), ('max_features', C.c_int32), ('max_depth', C.c_int32), ('min_samples_split', C.c_int32),
                ('min_samples_leaf', C.c_int32), ('wide_min_rows', C.c_int32), ('n_bin_rows', C.c_int64), ('bin_rows', C.c_void_p)]


class Forest(object):
    """RAII wrapper over an l3_forest handle: the resident training matrix, the level-wise fit and the resident forest of
    classifier/train.py:169-227's random forest on one device."""

    def __init__(self, device=0):
        self.lib = load()
        h = C.c_void_p()
        check(self.lib.l3_forest_create(int(device), C.byref(h)), None)
        self.h = h
        self.n = self.D = 0

    def close(self):
        if getattr(self, 'h', None):
            self.lib.l3_forest_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_data(self, X):
        x = _f32(X)
        check(self.lib.l3_forest_set_data(self.h, _ptr(x), x.shape[0], x.shape[1]))
        self.n, self.D = x.shape

    def set_data_dev(self, feat, lo=0, hi=None):
        """set_data from rows [lo, hi) of the Features `feat`, copied device to device; it may be closed afterwards"""
        n, d = feat.shape
        hi = n if hi is None else hi
        check(self.lib.l3_forest_set_data_dev(self.h, feat.h, int(lo), int(hi)))
        self.n, self.D = int(hi - lo), int(d)

    def fit(self, labels, boot, seeds, n_classes, max_features, max_depth=0, min_samples_split=2, min_samples_leaf=1,
            bin_rows=None, wide_min_rows=0):
        """labels (n) class indices; boot (n_trees, n) bootstrap multiplicities (uint16); seeds (n_trees); bin_rows: the ascending
        rows of the cut sample, None for all rows.  The forest stays resident; trees() downloads it."""
        y = _i32(labels).reshape(-1)
        b = np.ascontiguousarray(boot, np.uint16)
        sd = _i64(seeds).reshape(-1)
        if y.size != self.n or b.ndim != 2 or b.shape[1] != self.n or b.shape[0] != sd.size:
            raise ValueError('labels (n), boot (n_trees, n) and seeds (n_trees) must match the resident matrix of %d rows' % self.n)
        rows = None if bin_rows is None else _i32(bin_rows).reshape(-1)
        cfg = ForestConfig(int(n_classes), int(max_features), int(max_depth or 0), int(min_samples_split), int(min_samples_leaf),
                           int(wide_min_rows), 0 if rows is None else rows.size, None if rows is None else rows.ctypes.data)
        check(self.lib.l3_forest_fit(self.h, C.byref(cfg), _ptr(y), sd.size, _ptr(b), _ptr(sd)))

    def sizes(self):
        """-> (n_trees, n_nodes, n_classes, D) of the resident forest"""
        t, nn, c, d = C.c_int(), C.c_int64(), C.c_int(), C.c_int()
        check(self.lib.l3_forest_sizes(self.h, C.byref(t), C.byref(nn), C.byref(c), C.byref(d)))
        return t.value, nn.value, c.value, d.value

    def trees(self):
        """the resident forest as l3_forest_get_trees' flat arrays -> dict of FOREST_TREE_ARRAYS"""
        t, nn, c, _ = self.sizes()
        out = dict(tree_off=np.empty(t + 1, np.int64), left=np.empty(nn, np.int32), right=np.empty(nn, np.int32),
                   feature=np.empty(nn, np.int32), threshold=np.empty(nn, np.float32), bin=np.empty(nn, np.int32),
                   counts=np.empty((nn, c), np.int32), n_distinct=np.empty(nn, np.int32))
        check(self.lib.l3_forest_get_trees(self.h, *(_ptr(out[k]) for k in FOREST_TREE_ARRAYS)))
        return out

    def set_trees(self, trees, D):
        """a forest in trees()' arrays becomes the resident one"""
        off = _i64(trees['tree_off']).reshape(-1)
        counts = np.ascontiguousarray(trees['counts'], np.int32)
        nn = counts.shape[0]
        arrays = [_i32(trees[k]).reshape(-1) for k in ('left', 'right', 'feature')] + [_f32(trees['threshold']).reshape(-1)]
        if counts.ndim != 2 or off.size < 2 or off[-1] != nn or any(a.size != nn for a in arrays):
            raise ValueError('the tree arrays do not hold one entry per node')
        check(self.lib.l3_forest_set_trees(self.h, off.size - 1, counts.shape[1], int(D), _ptr(off), *(_ptr(a) for a in arrays),
                                           _ptr(counts)))

    def predict_proba(self, X):
        x = _f32(X)
        out = np.empty((x.shape[0], self.sizes()[2]), np.float64)
        check(self.lib.l3_forest_predict_proba(self.h, _ptr(x), x.shape[0], x.shape[1], _ptr(out)))
        return out

    def predict_proba_dev(self, feat, lo=0, hi=None):
        n, _ = feat.shape
        hi = n if hi is None else hi
        out = np.empty((max(int(hi - lo), 0), self.sizes()[2]), np.float64)
        check(self.lib.l3_forest_predict_proba_dev(self.h, feat.h, int(lo), int(hi), _ptr(out)))
        return out

    def score(self, X=None, feat=None, lo=0, hi=None, resident=False, prefixes=None, labels=None, files=None, outputs=('pred',),
              chunk_rows=0, stage_bytes=0):
        """l3_forest_score: the rows of exactly one of X (NumPy rows), rows [lo, hi) of the Features `feat` and rows [lo, hi) of the
        resident matrix, scored by the first prefixes[g] trees for every g in one pass (None: the whole forest) -> dict of the
        FOREST_SCORE_OUTPUTS that `outputs` names, each with the leading axis G.  labels: class indices; files: (F, 2) [start, end).
        chunk_rows, stage_bytes: the rows per launch and the LDS budget of the staged rows (0: the library's), for tests."""
        unknown = set(outputs) - set(FOREST_SCORE_OUTPUTS)
        if unknown:
            raise ValueError('unknown outputs %s; choose from %s' % (sorted(unknown), list(FOREST_SCORE_OUTPUTS)))
        T, _, nc, D = self.sizes()
        x = None
        if X is not None:
            x = _f32(X)
            lo, hi, D = 0, x.shape[0], x.shape[1] if x.ndim == 2 else -1
        elif hi is None:
            hi = feat.shape[0] if feat is not None else self.n
        n = max(int(hi) - int(lo), 0)
        p = _i32([T] if prefixes is None else prefixes).reshape(-1)
        y = None if labels is None else _i32(labels).reshape(-1)
        if y is not None and y.size != n:
            raise ValueError('one label per row')
        fl = None if files is None else _i64(files).reshape(-1, 2)
        F = 0 if fl is None else fl.shape[0]
        shapes = dict(pred=((p.size, n), np.int32), correct=((p.size,), np.int64), file_mean=((p.size, F, nc), np.float64),
                      file_pred=((p.size, F), np.int32), proba=((p.size, n, nc), np.float64))
        out = {k: np.empty(*shapes[k]) for k in FOREST_SCORE_OUTPUTS if k in outputs}
        check(self.lib.l3_forest_score(self.h, _ptr(x), None if feat is None else feat.h, int(lo), int(hi), int(D), 1 if resident else 0,
                                       _ptr(p), p.size, _ptr(y), _ptr(fl), F, int(chunk_rows), int(stage_bytes),
                                       *(_ptr(out.get(k)) for k in FOREST_SCORE_OUTPUTS)))
        return out

    def oob(self, boot, prefixes=None, labels=None, outputs=('correct',), chunk_rows=0, stage_bytes=0):
        """l3_forest_oob: every row of the resident matrix scored by the trees whose bootstrap missed it (boot (n_trees, n): the
        multiplicities the resident forest was fitted with), among the first prefixes[g] trees for every g in one pass (None: the
        whole forest) -> dict of the FOREST_OOB_OUTPUTS that `outputs` names, each with the leading axis G.  labels: class indices.
        chunk_rows, stage_bytes: score()'s."""
        unknown = set(outputs) - set(FOREST_OOB_OUTPUTS)
        if unknown:
            raise ValueError('unknown outputs %s; choose from %s' % (sorted(unknown), list(FOREST_OOB_OUTPUTS)))
        T, _, nc, _ = self.sizes()
        b = np.ascontiguousarray(boot, np.uint16)
        if b.ndim != 2 or (self.n and b.shape[1] != self.n):          # without a matrix the library refuses (L3_ESTATE)
            raise ValueError('boot must be (n_trees, n) for the resident matrix of %d rows' % self.n)
        n = self.n
        p = _i32([T] if prefixes is None else prefixes).reshape(-1)
        y = None if labels is None else _i32(labels).reshape(-1)
        if y is not None and y.size != n:
            raise ValueError('one label per row')
        shapes = dict(pred=((p.size, n), np.int32), correct=((p.size,), np.int64), n_oob=((p.size, n), np.int32),
                      sums=((p.size, n, nc), np.float64))
        out = {k: np.empty(*shapes[k]) for k in FOREST_OOB_OUTPUTS if k in outputs}
        check(self.lib.l3_forest_oob(self.h, _ptr(b), b.shape[0], _ptr(p), p.size, _ptr(y), int(chunk_rows), int(stage_bytes),
                                     *(_ptr(out.get(k)) for k in FOREST_OOB_OUTPUTS)))
        return out

    def cuts(self):
        """the last fit's (cuts (D, 255) float32, ncuts (D))"""
        cuts, ncuts = np.empty((self.D, FOREST_MAX_CUTS), np.float32), np.empty(self.D, np.int32)
        check(self.lib.l3_forest_get_cuts(self.h, _ptr(cuts), _ptr(ncuts)))
        return cuts, ncuts

    def level_stats(self):
        """the last fit's levels -> (nodes searched, of them by the wide kernel, wall ms), one entry per level"""
        L = self.lib.l3_forest_level_stats(self.h, 0, None, None, None)
        nodes, wide, ms = np.empty(L, np.int64), np.empty(L, np.int64), np.empty(L, np.float64)
        self.lib.l3_forest_level_stats(self.h, L, _ptr(nodes), _ptr(wide), _ptr(ms))
        return nodes, wide, ms
