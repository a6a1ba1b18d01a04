"""ctypes binding of libvallex.so (the C ABI in include/vallex.h).

There is deliberately no fallback: if the HIP library is missing or fails to load, importing
the symbols raises, and every product entry point that needs the GPU fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libvallex.so")

VX_PREC_F32, VX_PREC_BF16, VX_PREC_FP8_NAR = 0, 1, 2
BMAX = 64  # slots per engine (csrc/batch_kernels.hpp)
VX_FLAG_TRACE_LOGITS, VX_FLAG_NO_GRAPH, VX_FLAG_SIMPLE_ROWS, VX_FLAG_POST_NORM, VX_FLAG_PRENET, VX_FLAG_VALLF = 1, 2, 4, 8, 16, 32
VX_FLAG_KV_FP8 = 64
VX_FLAG_VALLF_ROWS = 128  # VALL-F: batched prefill / admission / NAR over concatenated rows (Engine(batched_rows=True))
VX_FLAG_LOGPROBS = 256  # generation records the log-probability of every emitted token (Engine(logprobs=True))
KV_CACHES = ("bf16", "fp8")  # storage of the batched decode's slot caches (VX_FLAG_KV_FP8)
VX_ADMIT_BATCHED, VX_ADMIT_PER_SLOT = 0, 1
VX_CODEC_LSTM_GRAPH, VX_CODEC_ENCODER = 1, 2
BE_QKV, BE_RELU, BE_PARTIAL, BE_LOGITS, BE_LOGITS_MAP, BE_BIAS = range(6)  # bgemm_kernel epilogues (csrc/batch_kernels.hpp)
STOP_REASONS = {0: "none", 1: "eos_argmax", 2: "eos_sample", 3: "length", 4: "max_new"}


class VxConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "struct_size", "d_model", "nhead", "num_layers", "nar_d_model", "nar_nhead", "nar_num_layers",
        "num_quantizers", "prefix_mode", "prepend_bos", "precision", "max_text", "max_audio", "device", "flags", "max_batch")]


class VxDecodeParams(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("top_k", C.c_int32), ("temperature", C.c_float), ("max_new_tokens", C.c_int32),
        ("exp_noise", C.c_void_p), ("noise_rows", C.c_int64), ("seed", C.c_uint64),
        ("forced", C.c_void_p), ("n_forced", C.c_int32), ("top_p", C.c_float),
    ]


class VxCodecConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("hidden", C.c_int32), ("filters", C.c_int32), ("ratios", C.c_int32 * 4)] + \
               [(n, C.c_int32) for n in ("kernel", "last_kernel", "res_kernel", "n_codebooks", "codebook_size", "codebook_dim",
                                         "lstm_layers", "max_frames", "max_batch", "device", "flags")]


class VxFbankConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "sample_rate", "n_fft", "hop", "n_mels")] + \
               [(n, C.c_float) for n in ("fmin", "fmax", "clip")] + [("max_batch", C.c_int32)]


class VxVocoderConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "sample_rate", "n_fft", "hop", "n_mels")] + \
               [(n, C.c_float) for n in ("fmin", "fmax", "env_floor")] + [("max_batch", C.c_int32), ("max_total_frames", C.c_int32)]


class VxGanConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("n_mels", C.c_int32), ("n_stages", C.c_int32), ("rates", C.c_int32 * 8),
                ("kernels", C.c_int32 * 8), ("initial_channels", C.c_int32), ("n_resblocks", C.c_int32),
                ("resblock_kernels", C.c_int32 * 4), ("n_dilations", C.c_int32), ("dilations", (C.c_int32 * 4) * 4),
                ("activation", C.c_int32), ("alpha_logscale", C.c_int32), ("lrelu_slope", C.c_float), ("max_batch", C.c_int32),
                ("max_total_frames", C.c_int32)]


VX_GAN_LRELU, VX_GAN_SNAKE, VX_GAN_SNAKEBETA = 0, 1, 2


class VxSpkConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "attention", "hidden", "layers", "heads", "ffn", "n_conv")] + \
               [(n, C.c_int32 * 8) for n in ("conv_dim", "conv_kernel", "conv_stride")] + \
               [(n, C.c_int32) for n in ("conv_bias", "pos_kernel", "pos_groups", "num_buckets", "n_tdnn")] + \
               [(n, C.c_int32 * 8) for n in ("tdnn_dim", "tdnn_kernel", "tdnn_dilation")] + \
               [(n, C.c_int32) for n in ("xvector", "use_weighted_layer_sum", "feat_extract_norm", "do_stable_layer_norm", "add_adapter",
                                         "activation")] + \
               [("layer_norm_eps", C.c_float), ("max_batch", C.c_int32), ("max_samples", C.c_int32), ("flags", C.c_int32)]


VX_SPK_WAVLM, VX_SPK_PLAIN = 0, 1
VX_SPK_KEEP_TAPS = 1   # vx_spk_config.flags
VX_SPK_NORMALIZE = 1   # vx_spk_embed flags


class VxAsrConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "hidden", "layers", "heads", "ffn", "n_conv")] + \
               [(n, C.c_int32 * 8) for n in ("conv_dim", "conv_kernel", "conv_stride")] + \
               [(n, C.c_int32) for n in ("conv_bias", "pos_kernel", "pos_groups", "vocab", "blank", "feat_extract_norm",
                                         "do_stable_layer_norm", "feat_proj_layer_norm", "add_adapter", "conv_pos_batch_norm",
                                         "activation")] + \
               [("layer_norm_eps", C.c_float), ("max_batch", C.c_int32), ("max_samples", C.c_int32), ("flags", C.c_int32)]


VX_ASR_KEEP_TAPS = 1   # vx_asr_config.flags
VX_ASR_ENC_BF16 = 2    # vx_asr_config.flags: the bf16 encoder mode
VX_ASR_NORMALIZE = 1   # vx_asr_recognize flags


class VxWspConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "n_mels", "d_model", "enc_layers", "enc_heads", "enc_ffn", "dec_layers", "dec_heads",
                                         "dec_ffn", "max_source_positions", "max_target_positions", "vocab", "activation", "tie_proj",
                                         "eos_token_id", "max_batch", "flags")]


VX_WSP_KEEP_TAPS = 1   # vx_wsp_config.flags
VX_WSP_ENC_BF16 = 2    # vx_wsp_config.flags: the bf16 encoder mode
ENC_PRECISIONS = ("fp32", "bf16")  # `precision=` of SpeechRecognizer and WhisperRecognizer
EBF_EPI_BF16, EBF_EPI_GELU_BF16, EBF_EPI_RESID_F32 = 0, 1, 2  # vx_op_enc16_gemm's epilogues


class VxDtwConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "dim", "n_ceps", "max_frames", "max_batch")]


class VxPitchConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("sample_rate", C.c_int32), ("fmin_hz", C.c_float), ("fmax_hz", C.c_float),
                ("threshold", C.c_float), ("max_frames", C.c_int32), ("max_batch", C.c_int32)]


PITCH_NSUMS = 11  # doubles per pair of vx_pitch_compare (csrc/pitch_kernels.hpp)


class VxStftConfig(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("sample_rate", C.c_int32), ("n_res", C.c_int32), ("n_fft", C.c_int32 * 4),
                ("hop", C.c_int32 * 4), ("win", C.c_int32 * 4), ("eps", C.c_float), ("max_samples", C.c_int32), ("max_batch", C.c_int32)]


STFT_NSUMS = 4  # doubles per (pair, resolution) of vx_stft_compare (include/vallex.h lists them)


class VxMelConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "d_model", "nhead", "num_layers", "norm_first", "add_prenet", "scaling_xformers",
                                         "precision", "max_text", "max_frames", "device", "flags")]


VX_MEL_NO_GRAPH = 1
MEL_STOP_REASONS = {0: "none", 1: "logit", 2: "length", 3: "max_frames"}
NUM_MEL_BINS = 100


class VxError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"vallex error {code}: {msg}")
        self.code = code


_lib: Optional[C.CDLL] = None

_SIGS = {
    "vx_last_error": (C.c_char_p, []),
    "vx_create": (C.c_int, [C.POINTER(VxConfig), C.POINTER(C.c_void_p)]),
    "vx_destroy": (None, [C.c_void_p]),
    "vx_set_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int32]),
    "vx_set_sine_table": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int64]),
    "vx_finalize_weights": (C.c_int, [C.c_void_p]),
    "vx_ar_prefill": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "vx_ar_decode": (C.c_int, [C.c_void_p, C.POINTER(VxDecodeParams), C.c_void_p]),
    "vx_ar_result": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "vx_ar_logprobs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "vx_batch_logprobs": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "vx_nar_logprobs": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]),
    "vx_nar": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "vx_nar_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                            C.c_void_p, C.c_int32, C.c_void_p]),
    "vx_nar_continual": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "vx_batch_prefill": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "vx_batch_prefill_all": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_void_p),
                                       C.POINTER(C.c_int32), C.c_void_p]),
    "vx_batch_decode": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(VxDecodeParams), C.c_void_p]),
    "vx_batch_result": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "vx_batch_open": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vx_batch_admit": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_void_p), C.POINTER(C.c_int32),
                                 C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(VxDecodeParams), C.c_int32, C.c_void_p]),
    "vx_batch_run": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p]),
    "vx_nar_batch": (C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 7 + [C.c_void_p]),
    "vx_nar_batch_ex": (C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 8 + [C.c_void_p]),
    "vx_score": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32]
                 + [C.c_void_p] * 4 + [C.c_void_p]),
    "vx_score_batch": (C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 11 + [C.c_void_p]),
    "vx_align": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
                 + [C.c_void_p] * 6 + [C.c_void_p]),
    "vx_align_batch": (C.c_int, [C.c_void_p, C.c_int32] + [C.c_void_p] * 12 + [C.c_void_p]),
    "vx_get_timings": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int32]),
    "vx_read_buffer": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_int64]),
    "vx_buffer_bytes": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64)]),
    "vx_op_layernorm": (C.c_int, [C.c_int32] + [C.c_void_p] * 6 + [C.c_int32, C.c_int32, C.c_void_p]),
    "vx_op_gemv": (C.c_int, [C.c_int32] + [C.c_void_p] * 4 + [C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "vx_op_gemm": (C.c_int, [C.c_int32, C.c_int32] + [C.c_void_p] * 4 + [C.c_int32] * 4 + [C.c_void_p]),
    "vx_op_gemm_rows": (C.c_int, [C.c_int32] + [C.c_void_p] * 4 + [C.c_int32] * 4 + [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "vx_op_gemm_partial": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 4 + [C.c_void_p]),
    "vx_op_ln_fold": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64] + [C.c_void_p] * 7 + [C.c_int32, C.c_int32,
                      C.c_void_p]),
    "vx_op_rows_plan": (C.c_int, [C.c_int32] * 3 + [C.POINTER(C.c_int32)]),
    "vx_op_gemm_mx": (C.c_int, [C.c_void_p] * 5 + [C.c_int32] * 5 + [C.c_void_p] * 3),
    "vx_op_layernorm_mx": (C.c_int, [C.c_void_p] * 7 + [C.c_int32, C.c_int32, C.c_void_p]),
    "vx_op_attention": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p]),
    "vx_op_attention_segs": (C.c_int, [C.c_void_p, C.c_void_p] + [C.c_int32] * 4 + [C.POINTER(C.c_int32)] * 3 + [C.c_void_p]),
    "vx_op_cross_attention_segs": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_int64), C.c_int64, C.c_int64,
                                             C.POINTER(C.c_int32), C.c_void_p] + [C.c_int32] * 3 + [C.POINTER(C.c_int32)] * 2 + [C.c_void_p]),
    "vx_op_attn_slots": (C.c_int, [C.c_int32] + [C.c_void_p] * 3 + [C.c_int64, C.c_int64] + [C.c_int32] * 3
                         + [C.POINTER(C.c_int32)] * 2 + [C.c_void_p, C.c_void_p]),
    "vx_op_attn_mem_slots": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64] + [C.c_int32] * 3
                             + [C.POINTER(C.c_int32)] * 2 + [C.c_void_p, C.c_void_p]),
    "vx_op_bgemm": (C.c_int, [C.c_int32, C.c_int32] + [C.c_void_p] * 3 + [C.c_int32] * 4 + [C.POINTER(C.c_int32)] * 3
                    + [C.c_void_p] * 3 + [C.c_int64, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 3 + [C.c_int32, C.c_void_p,
                    C.c_int32, C.POINTER(C.c_int32), C.c_void_p]),
    "vx_op_ln_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 4 + [C.c_int32, C.c_int32, C.POINTER(C.c_int32),
                       C.c_void_p]),
    "vx_op_nll_rows": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 4 + [C.c_void_p]),
    "vx_op_attn_text_rows": (C.c_int, [C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64] + [C.c_int32] * 8
                             + [C.c_void_p] * 4 + [C.c_int32, C.c_void_p]),
    "vx_op_mono_path": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vx_op_attn_text_segs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_int64), C.c_int32] + [C.c_void_p] * 3
                             + [C.c_int64, C.c_int64, C.c_int32, C.c_void_p]),
    "vx_op_mono_path_segs": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p]),
    "vx_op_sample": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p]),
    "vx_op_sample_topp": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_void_p, C.POINTER(C.c_int32),
                                    C.c_void_p]),
    "vx_op_sample_logprob": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_void_p, C.POINTER(C.c_int32),
                                       C.POINTER(C.c_float), C.c_void_p]),
    "vx_op_convert_bf16": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    # EnCodec decoder and encoder (codec.py)
    "vx_codec_create": (C.c_int, [C.POINTER(VxCodecConfig), C.POINTER(C.c_void_p)]),
    "vx_codec_destroy": (None, [C.c_void_p]),
    "vx_codec_set_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int32]),
    "vx_codec_finalize": (C.c_int, [C.c_void_p]),
    "vx_codec_decode": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int32,
                                  C.POINTER(C.c_void_p), C.c_void_p]),
    "vx_codec_encode": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int32,
                                  C.POINTER(C.c_void_p), C.c_void_p]),
    "vx_codec_last_embeddings": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "vx_op_codec_conv_strided": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 6 + [C.POINTER(C.c_int32), C.c_void_p]),
    "vx_op_codec_rvq_encode": (C.c_int, [C.c_void_p] * 3 + [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "vx_op_codec_conv": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 5 + [C.POINTER(C.c_int32), C.c_int32, C.c_void_p]),
    "vx_op_codec_convtr": (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 5 + [C.POINTER(C.c_int32), C.c_int32, C.c_void_p]),
    "vx_op_codec_lstm": (C.c_int, [C.c_void_p] + [C.POINTER(C.c_void_p)] * 4 + [C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                   C.POINTER(C.c_int32), C.c_void_p]),
    # sample-rate conversion and mix-down (codec.Resampler)
    "vx_resampler_create": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]),
    "vx_resampler_destroy": (None, [C.c_void_p]),
    "vx_resample_length": (C.c_int64, [C.c_int32, C.c_int32, C.c_int64]),
    "vx_resample": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                              C.POINTER(C.c_void_p), C.c_void_p]),
    # log-mel filterbank (fbank.BigVGANFbank)
    "vx_fbank_create": (C.c_int, [C.POINTER(VxFbankConfig), C.POINTER(C.c_void_p)]),
    "vx_fbank_destroy": (None, [C.c_void_p]),
    "vx_fbank_set_mel_basis": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vx_fbank_get_mel_basis": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vx_fbank_frames": (C.c_int64, [C.c_int64]),
    "vx_fbank_extract": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_void_p),
                                   C.c_void_p]),
    # dynamic time warping (dtw.DTW)
    "vx_dtw_create": (C.c_int, [C.POINTER(VxDtwConfig), C.POINTER(C.c_void_p)]),
    "vx_dtw_destroy": (None, [C.c_void_p]),
    "vx_dtw_compare": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_void_p),
                                 C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p]),
    "vx_op_dtw_cost": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "vx_op_dtw_path": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # pitch tracking and F0 figures (pitch.PitchTracker)
    "vx_pitch_create": (C.c_int, [C.POINTER(VxPitchConfig), C.POINTER(C.c_void_p)]),
    "vx_pitch_destroy": (None, [C.c_void_p]),
    "vx_pitch_lag_range": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "vx_pitch_track": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32)] + [C.POINTER(C.c_void_p)] * 4
                       + [C.c_void_p]),
    "vx_pitch_compare": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_void_p),
                                   C.POINTER(C.c_int32), C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]),
    "vx_op_pitch_diff": (C.c_int, [C.c_float, C.c_float, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    # multi-resolution STFT distance (stft.MultiResolutionSTFT)
    "vx_stft_create": (C.c_int, [C.POINTER(VxStftConfig), C.POINTER(C.c_void_p)]),
    "vx_stft_destroy": (None, [C.c_void_p]),
    "vx_stft_frames": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "vx_stft_compare": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_void_p),
                                  C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]),
    "vx_stft_magnitude": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_void_p),
                                    C.c_void_p]),
    # mel-spectrogram Transformer (meltf.Transformer)
    "vx_mel_create": (C.c_int, [C.POINTER(VxMelConfig), C.POINTER(C.c_void_p)]),
    "vx_mel_destroy": (None, [C.c_void_p]),
    "vx_mel_set_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int32]),
    "vx_mel_set_sine_table": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]),
    "vx_mel_finalize": (C.c_int, [C.c_void_p]),
    "vx_mel_encode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "vx_mel_decode": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "vx_mel_decode_forced": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "vx_mel_result": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_void_p,
                                C.POINTER(C.c_int32)]),
    "vx_mel_teacher_forced": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vx_mel_get_timings": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int32]),
    "vx_mel_read": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.c_int64]),
    "vx_op_mel_open": (C.c_int, [C.c_int32] + [C.c_void_p] * 13 + [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                 C.POINTER(C.c_int32), C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_uint32), C.c_void_p]),
    # Griffin-Lim vocoder (vocoder.GriffinLim)
    "vx_vocoder_create": (C.c_int, [C.POINTER(VxVocoderConfig), C.POINTER(C.c_void_p)]),
    "vx_vocoder_destroy": (None, [C.c_void_p]),
    "vx_vocoder_set_mel_basis": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vx_vocoder_set_inverse": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vx_vocoder_get_inverse": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vx_vocoder_samples": (C.c_int64, [C.c_int64]),
    "vx_vocoder_synthesize": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_void_p),
                                        C.c_int32, C.c_float, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p]),
    "vx_vocoder_synthesize_warm": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32),
                                             C.POINTER(C.c_void_p), C.c_int32, C.c_float, C.POINTER(C.c_void_p),
                                             C.POINTER(C.c_void_p), C.c_void_p]),
    # HiFi-GAN / BigVGAN generator (ganvoc.GanVocoder)
    "vx_gan_create": (C.c_int, [C.POINTER(VxGanConfig), C.POINTER(C.c_void_p)]),
    "vx_gan_destroy": (None, [C.c_void_p]),
    "vx_gan_set_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int32]),
    "vx_gan_set_filter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "vx_gan_get_filter": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vx_gan_finalize": (C.c_int, [C.c_void_p]),
    "vx_gan_samples": (C.c_int64, [C.c_void_p, C.c_int64]),
    "vx_gan_synthesize": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_void_p),
                                    C.c_void_p]),
    # speaker encoder (spk.SpeakerEncoder)
    "vx_spk_create": (C.c_int, [C.POINTER(VxSpkConfig), C.POINTER(C.c_void_p)]),
    "vx_spk_destroy": (None, [C.c_void_p]),
    "vx_spk_set_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int32]),
    "vx_spk_set_buckets": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "vx_spk_finalize": (C.c_int, [C.c_void_p]),
    "vx_spk_frames": (C.c_int64, [C.c_void_p, C.c_int64]),
    "vx_spk_min_samples": (C.c_int64, [C.c_void_p]),
    "vx_spk_embed": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.c_void_p,
                               C.c_void_p]),
    "vx_spk_similarity": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vx_spk_read": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32, C.c_void_p, C.c_int64]),
    "vx_spk_get_timings": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int32]),
    # CTC recogniser, greedy decode and edit distance (asr.SpeechRecognizer)
    "vx_asr_create": (C.c_int, [C.POINTER(VxAsrConfig), C.POINTER(C.c_void_p)]),
    "vx_asr_destroy": (None, [C.c_void_p]),
    "vx_asr_set_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int32]),
    "vx_asr_finalize": (C.c_int, [C.c_void_p]),
    "vx_asr_frames": (C.c_int64, [C.c_void_p, C.c_int64]),
    "vx_asr_min_samples": (C.c_int64, [C.c_void_p]),
    "vx_asr_recognize": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int32, C.c_void_p, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vx_asr_read": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32, C.c_void_p, C.c_int64]),
    "vx_asr_get_timings": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int32]),
    "vx_ctc_greedy": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "vx_edit_distance": (C.c_int, [C.c_int32, C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]),
    # CTC forced alignment and text likelihood (asr.ctc_forced_align, SpeechRecognizer.align)
    "vx_falign": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
                  + [C.c_void_p] * 8),
    "vx_falign_asr": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)] + [C.c_void_p] * 8),
    # Whisper recogniser (whisper.WhisperRecognizer)
    "vx_wsp_create": (C.c_int, [C.POINTER(VxWspConfig), C.POINTER(C.c_void_p)]),
    "vx_wsp_destroy": (None, [C.c_void_p]),
    "vx_wsp_set_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int32]),
    "vx_wsp_set_suppress": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32), C.c_int32]),
    "vx_wsp_finalize": (C.c_int, [C.c_void_p]),
    "vx_wsp_recognize": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                   C.POINTER(C.c_int32), C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "vx_wsp_read": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32, C.c_void_p, C.c_int64]),
    "vx_wsp_get_timings": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.c_int32]),
    # the token loop's kernels on caller data (whisper.op_wsp_*)
    "vx_op_wsp_gemm": (C.c_int, [C.c_void_p] * 5 + [C.c_int32] * 4 + [C.c_void_p]),
    "vx_op_wsp_decode_attn": (C.c_int, [C.c_void_p] * 6 + [C.c_int32] * 5 + [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p]),
    "vx_op_wsp_head": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 11
                       + [C.c_int32] * 3 + [C.c_void_p]),
    "vx_op_wsp_embed": (C.c_int, [C.c_void_p] * 5 + [C.c_int32] * 4 + [C.c_void_p]),
    # the bf16 encoder mode's kernels on caller data (whisper.op_enc16_*)
    "vx_op_enc16_gemm": (C.c_int, [C.c_int32] + [C.c_void_p] * 5 + [C.c_int64, C.c_int32, C.c_int32, C.c_void_p]),
    "vx_op_enc16_add_ln": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 4 + [C.c_int64, C.c_int32, C.c_float, C.c_void_p]),
    "vx_op_enc16_attn": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.c_void_p]),
}

# measurement probes (csrc/probes.h): exported by the probe builds only (`csrc/build.py --probes|--stamps`), never by libvallex.so
_PROBE_SIGS = {
    "vx_debug_launch_floor": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double)]),
    "vx_debug_stage_chain": (C.c_int, [C.c_int32] * 5 + [C.POINTER(C.c_double)]),
    "vx_debug_l2_fill": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.POINTER(C.c_double)]),
    "vx_debug_read_stamps": (C.c_int, [C.POINTER(C.c_uint64), C.c_int32]),
    "vx_debug_kstamps": (C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_int32)]),
}


def declared_symbols():
    return sorted(_SIGS)


def load_library(path: str = LIB_PATH) -> C.CDLL:
    """Loads libvallex.so and attaches the prototypes.  Raises if the library is absent: build it
    with ``python vall-e_amd/csrc/build.py`` (or ``__graft_entry__.build()``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path} not built — run `python vall-e_amd/csrc/build.py`; there is no CPU fallback")
    lib = C.CDLL(path)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in _PROBE_SIGS.items():  # present in the probe builds only
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    _lib = lib
    return lib


def load_probe_library(stamps: bool = False) -> C.CDLL:
    """Measurement scripts (tests/probes) only: makes the probe build the process's library.  Must be called before anything
    else loads libvallex.so."""
    assert _lib is None, "a library is already loaded in this process"
    return load_library(os.path.join(_HERE, "csrc", "libvallex_stamps.so" if stamps else "libvallex_probes.so"))


def _check(code: int):
    if code != 0:
        raise VxError(code, load_library().vx_last_error().decode())


def _ptr(t) -> Optional[int]:
    if t is None:
        return None
    if isinstance(t, torch.Tensor):
        assert t.is_contiguous()
        return t.data_ptr()
    if isinstance(t, np.ndarray):
        assert t.flags["C_CONTIGUOUS"]
        return t.ctypes.data
    raise TypeError(type(t))


def current_stream_ptr(device) -> Optional[int]:
    s = torch.cuda.current_stream(device).cuda_stream
    return s or None


class Engine:
    """One model replica on one GPU (see include/vallex.h for the contract of each call)."""

    def __init__(self, cfg, precision: str = "bf16", max_text: int = 256, max_audio: int = 2048, device: int = 0,
                 trace_logits: bool = False, no_graph: bool = False, simple_rows: bool = False, max_batch: int = 0,
                 kv_cache: str = "bf16", batched_rows: bool = False, logprobs: bool = False):
        if kv_cache not in KV_CACHES:
            raise ValueError(f"kv_cache must be one of {KV_CACHES}, got {kv_cache!r}")
        if batched_rows and not getattr(cfg, "is_vallf", False):
            raise ValueError("batched_rows=True is the VALL-F option (VX_FLAG_VALLF_ROWS): a VALL-E engine batches its row passes as it is")
        self.lib = load_library()
        self.cfg = cfg
        self.device = int(device)
        self.precision = precision
        c = VxConfig()
        c.struct_size = C.sizeof(VxConfig)
        c.d_model, c.nhead, c.num_layers = cfg.decoder_dim, cfg.nhead, cfg.num_decoder_layers
        c.nar_d_model, c.nar_nhead, c.nar_num_layers = cfg.nar_dim, cfg.nar_nhead, cfg.nar_layers
        c.num_quantizers, c.prefix_mode, c.prepend_bos = cfg.num_quantizers, cfg.prefix_mode, int(cfg.prepend_bos)
        c.precision = {"fp32": VX_PREC_F32, "f32": VX_PREC_F32, "bf16": VX_PREC_BF16, "fp8nar": VX_PREC_FP8_NAR}[precision]
        c.max_text, c.max_audio, c.device = max_text, max_audio, self.device
        c.flags = (VX_FLAG_TRACE_LOGITS if trace_logits else 0) | (VX_FLAG_NO_GRAPH if no_graph else 0) | \
                  (VX_FLAG_SIMPLE_ROWS if simple_rows else 0) | (0 if getattr(cfg, "norm_first", True) else VX_FLAG_POST_NORM) | \
                  (VX_FLAG_PRENET if getattr(cfg, "add_prenet", False) else 0) | \
                  (VX_FLAG_VALLF if getattr(cfg, "is_vallf", False) else 0) | \
                  (VX_FLAG_KV_FP8 if kv_cache == "fp8" else 0) | (VX_FLAG_VALLF_ROWS if batched_rows else 0) | \
                  (VX_FLAG_LOGPROBS if logprobs else 0)
        c.max_batch = int(max_batch)
        self.max_text, self.max_audio, self.trace_logits, self.max_batch = max_text, max_audio, trace_logits, int(max_batch)
        self.kv_cache = kv_cache
        # VALL-F only: the engine also keeps a packed text-memory buffer for the batched NAR pass (2 nar_layers nar_dim bf16 per text
        # row, grown with the other row buffers) and accepts batch_prefill_all / batch_admit(batched=True) / nar_batch
        self.batched_rows = bool(batched_rows)
        # every decode and NAR call also records the log-probability of what it emitted (ar_logprobs / batch_logprobs / nar_logprobs)
        self.logprobs = bool(logprobs)
        self.mfma_rows = c.precision != VX_PREC_F32 and not simple_rows
        h = C.c_void_p()
        _check(self.lib.vx_create(C.byref(c), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.vx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- weights -----------------------------------------------------------------------------
    def load_state_dict(self, sd, sine_tables: bool = True):
        from .weights import expected_keys, sine_table

        keys = expected_keys(self.cfg)
        for k, shape in keys.items():
            if k.endswith("num_batches_tracked"):  # BatchNorm's step counter: not read by the forward pass
                continue
            t = sd[k].detach().to(torch.float32).contiguous()
            assert tuple(t.shape) == tuple(shape), (k, tuple(t.shape), shape)
            shp = (C.c_int64 * t.dim())(*t.shape)
            _check(self.lib.vx_set_weight(self.h, k.encode(), _ptr(t), shp, t.dim()))
        if sine_tables:
            rows = max(4000, self.max_text + self.max_audio)
            pe = sine_table(rows, self.cfg.decoder_dim)
            _check(self.lib.vx_set_sine_table(self.h, 0, _ptr(pe), rows, self.cfg.decoder_dim))
            if self.cfg.num_quantizers > 1:
                pe = sine_table(rows, self.cfg.nar_dim)
                _check(self.lib.vx_set_sine_table(self.h, 1, _ptr(pe), rows, self.cfg.nar_dim))
        _check(self.lib.vx_finalize_weights(self.h))

    # -- hot path ----------------------------------------------------------------------------
    def ar_prefill(self, text: torch.Tensor, prompt_cb0: torch.Tensor, stream=None):
        text = text.to(torch.int64).contiguous()
        prompt_cb0 = prompt_cb0.to(torch.int64).contiguous()
        self._keep = (text, prompt_cb0)
        _check(self.lib.vx_ar_prefill(self.h, _ptr(text), text.numel(), _ptr(prompt_cb0), prompt_cb0.numel(), stream))

    def ar_decode(self, top_k: int = -100, temperature: float = 1.0, exp_noise: Optional[torch.Tensor] = None,
                  seed: int = 0, max_new_tokens: int = -1, forced: Optional[torch.Tensor] = None, stream=None, top_p: float = 1.0):
        p = VxDecodeParams()
        p.struct_size = C.sizeof(VxDecodeParams)
        p.top_k, p.temperature, p.max_new_tokens, p.seed = int(top_k), float(temperature), int(max_new_tokens), int(seed)
        p.top_p = _struct_top_p(top_p)
        keep = []
        if exp_noise is not None:
            exp_noise = exp_noise.to(torch.float32).contiguous()
            assert exp_noise.dim() == 2 and exp_noise.shape[1] == 1025
            p.exp_noise, p.noise_rows = _ptr(exp_noise), exp_noise.shape[0]
            keep.append(exp_noise)
        if forced is not None:
            forced = forced.to(torch.int64).contiguous()
            p.forced, p.n_forced = (_ptr(forced) if forced.numel() else _ptr(torch.zeros(1, dtype=torch.int64))), forced.numel()
            keep.append(forced)
        _check(self.lib.vx_ar_decode(self.h, C.byref(p), stream))

    def ar_result(self):
        n, reason, npass = C.c_int32(), C.c_int32(), C.c_int32()
        _check(self.lib.vx_ar_result(self.h, None, 0, C.byref(n), C.byref(reason), C.byref(npass)))
        toks = torch.empty(n.value, dtype=torch.int64)
        _check(self.lib.vx_ar_result(self.h, _ptr(toks), n.value, C.byref(n), C.byref(reason), C.byref(npass)))
        return toks, reason.value, npass.value

    def _logprobs(self, fn, *lead):
        n = C.c_int32()
        _check(fn(self.h, *lead, None, 0, C.byref(n)))
        out = torch.empty(n.value, dtype=torch.float32)
        _check(fn(self.h, *lead, _ptr(out), n.value, C.byref(n)))
        return out

    def ar_logprobs(self) -> torch.Tensor:
        """(n_pass,) fp32 on the host: the log-probability of every pass of the last ``ar_decode`` (vx_ar_logprobs); needs
        ``logprobs=True``."""
        return self._logprobs(self.lib.vx_ar_logprobs)

    def batch_logprobs(self, slot: int) -> torch.Tensor:
        """``ar_logprobs`` of a slot (vx_batch_logprobs).  In a session: before the ``batch_result`` that vacates the slot."""
        return self._logprobs(self.lib.vx_batch_logprobs, int(slot))

    def nar_logprobs(self, utt: int, T: int) -> torch.Tensor:
        """(Q-1, T) fp32 on the host: per stage and generated frame the log-probability of the code the stage picked, for
        utterance ``utt`` of the last NAR call (vx_nar_logprobs)."""
        out = torch.empty((max(self.cfg.num_quantizers - 1, 0), int(T)), dtype=torch.float32)
        _check(self.lib.vx_nar_logprobs(self.h, int(utt), _ptr(out), out.numel()))
        return out

    @staticmethod
    def op_sample_logprob(logits, top_k, temperature, top_p, exp_noise):
        return op_sample_logprob(logits, top_k, temperature, top_p, exp_noise)

    def nar(self, text_nar: torch.Tensor, prompts: torch.Tensor, ar_tokens: torch.Tensor, out_device=None, stream=None,
            continual: bool = False, forced_codes: Optional[torch.Tensor] = None, stage_logits: bool = False):
        """prompts: (P, Q); returns codes (T, Q) int64 on ``out_device`` (default: prompts' device).  ``continual``:
        the NAR body of VALLE.continual (vx_nar_continual).  Parity-test options (vx_nar_ex): ``forced_codes`` (T, Q) feeds
        every stage the given codes of the earlier stages; ``stage_logits=True`` also returns the (Q-1, T, 1024) logits."""
        text_nar = text_nar.to(torch.int64).contiguous()
        prompts = prompts.to(torch.int64).contiguous()
        ar_tokens = ar_tokens.to(torch.int64).contiguous()
        T, Q = ar_tokens.numel(), self.cfg.num_quantizers
        out = torch.empty((T, Q), dtype=torch.int64, device=out_device if out_device is not None else prompts.device)
        if forced_codes is None and not stage_logits:
            fn = self.lib.vx_nar_continual if continual else self.lib.vx_nar
            _check(fn(self.h, _ptr(text_nar), text_nar.numel(), _ptr(prompts), prompts.shape[0], _ptr(ar_tokens), T, _ptr(out), stream))
            return out
        fc = None if forced_codes is None else forced_codes.to(torch.int64).contiguous()
        assert fc is None or tuple(fc.shape) == (T, Q)
        lg = torch.empty((max(Q - 1, 0), T, 1024), dtype=torch.float32) if stage_logits else None
        _check(self.lib.vx_nar_ex(self.h, _ptr(text_nar), text_nar.numel(), _ptr(prompts), prompts.shape[0], _ptr(ar_tokens), T,
                                  _ptr(out), _ptr(fc), _ptr(lg), int(continual), stream))
        return (out, lg) if stage_logits else out

    # -- batched decode (BASELINE configs[2]) -------------------------------------------------------
    def batch_prefill(self, slot: int, text: torch.Tensor, prompt_cb0: torch.Tensor, stream=None):
        text = text.to(torch.int64).contiguous()
        prompt_cb0 = prompt_cb0.to(torch.int64).contiguous()
        _check(self.lib.vx_batch_prefill(self.h, slot, _ptr(text), text.numel(), _ptr(prompt_cb0), prompt_cb0.numel(), stream))

    def batch_prefill_all(self, texts, prompts_cb0, stream=None):
        """Slots 0..n-1 prefilled in one pass over the concatenated rows (bf16 engines)."""
        n = len(texts)
        texts = [t.to(torch.int64).contiguous() for t in texts]
        proms = [p.to(torch.int64).contiguous() for p in prompts_cb0]
        tp = (C.c_void_p * n)(*[_ptr(t) for t in texts])
        pp = (C.c_void_p * n)(*[_ptr(p) for p in proms])
        S = (C.c_int32 * n)(*[t.numel() for t in texts])
        P = (C.c_int32 * n)(*[p.numel() for p in proms])
        _check(self.lib.vx_batch_prefill_all(self.h, n, tp, S, pp, P, stream))

    @staticmethod
    def _decode_params(n, top_k, temperature, seeds, exp_noise, forced, max_new_tokens, top_p=1.0):
        """(VxDecodeParams array, per-entry list of the device tensors its pointers refer to).  ``top_k`` / ``top_p``: one
        value for every entry, or a sequence of n (the slots of one batch may mix filters)."""
        arr = (VxDecodeParams * n)()
        keep = [[] for _ in range(n)]
        tks = list(top_k) if isinstance(top_k, (list, tuple)) else [top_k] * n
        tps = list(top_p) if isinstance(top_p, (list, tuple)) else [top_p] * n
        assert len(tks) == n and len(tps) == n
        for b in range(n):
            p = arr[b]
            p.struct_size = C.sizeof(VxDecodeParams)
            p.top_k, p.temperature, p.max_new_tokens = int(tks[b]), float(temperature), int(max_new_tokens)
            p.top_p = _struct_top_p(tps[b])
            p.seed = int(seeds[b]) if seeds is not None else b + 1
            if exp_noise is not None and exp_noise[b] is not None:
                t = exp_noise[b].to(torch.float32).contiguous()
                assert t.is_cuda and t.shape[1] == 1025
                p.exp_noise, p.noise_rows = _ptr(t), t.shape[0]
                keep[b].append(t)
            if forced is not None and forced[b] is not None:
                t = forced[b].to(torch.int64).contiguous()
                assert t.is_cuda
                p.forced, p.n_forced = _ptr(t), t.numel()
                keep[b].append(t)
        return arr, keep

    def batch_decode(self, n_slots: int, top_k=-100, temperature=1.0, seeds=None, exp_noise=None, forced=None,
                     max_new_tokens=-1, stream=None, top_p=1.0):
        """exp_noise / forced: optional per-slot lists of DEVICE tensors (kept alive here for the call).  top_k / top_p: one value
        or one per slot."""
        arr, keep = self._decode_params(n_slots, top_k, temperature, seeds, exp_noise, forced, max_new_tokens, top_p)
        _check(self.lib.vx_batch_decode(self.h, n_slots, arr, stream))

    # -- continuous batching (vx_batch_open / _admit / _run) ------------------------------------------
    def batch_open(self, stream=None):
        """Starts a session: every slot vacant."""
        _check(self.lib.vx_batch_open(self.h, stream))
        self._slot_keep = {}

    def batch_admit(self, slots, texts, prompts_cb0, top_k=-100, temperature=1.0, seeds=None, exp_noise=None, forced=None,
                    max_new_tokens=-1, batched=True, stream=None, top_p=1.0):
        """Prefills ``texts[z]`` / ``prompts_cb0[z]`` into vacant slot ``slots[z]`` and arms it (seeds / exp_noise / forced per
        utterance, as for ``batch_decode``).  ``batched``: one pass over the concatenated rows; False: the per-slot prefill.  The
        device tensors a slot's parameters point to are kept until that slot's result is read."""
        n = len(slots)
        texts = [t.to(torch.int64).contiguous() for t in texts]
        proms = [p.to(torch.int64).contiguous() for p in prompts_cb0]
        arr, keep = self._decode_params(n, top_k, temperature, seeds, exp_noise, forced, max_new_tokens, top_p)
        sl = (C.c_int32 * n)(*[int(s) for s in slots])
        tp = (C.c_void_p * n)(*[_ptr(t) for t in texts])
        pp = (C.c_void_p * n)(*[_ptr(p) for p in proms])
        S = (C.c_int32 * n)(*[t.numel() for t in texts])
        P = (C.c_int32 * n)(*[p.numel() for p in proms])
        _check(self.lib.vx_batch_admit(self.h, n, sl, tp, S, pp, P, arr, VX_ADMIT_BATCHED if batched else VX_ADMIT_PER_SLOT, stream))
        for s, k in zip(slots, keep):
            self._slot_keep[int(s)] = k

    def batch_run(self, min_stopped: int = 1, poll_steps: int = 0, stream=None):
        """Decodes until at least ``min_stopped`` live slots have stopped (or none is live); returns the list of stopped slots."""
        out = (C.c_int32 * max(self.max_batch, 1))()
        n = C.c_int32()
        code = self.lib.vx_batch_run(self.h, int(min_stopped), int(poll_steps), out, C.byref(n), stream)
        self._last_stopped = [out[i] for i in range(n.value)]
        _check(code)
        return list(self._last_stopped)

    def batch_result(self, slot: int):
        n, reason = C.c_int32(), C.c_int32()
        _check(self.lib.vx_batch_result(self.h, slot, None, 0, C.byref(n), C.byref(reason)))
        toks = torch.empty(n.value, dtype=torch.int64)
        _check(self.lib.vx_batch_result(self.h, slot, _ptr(toks), n.value, C.byref(n), C.byref(reason)))
        getattr(self, "_slot_keep", {}).pop(int(slot), None)  # continuous batching: the slot's device tensors may go now
        return toks, reason.value

    def nar_batch(self, texts, prompts, tokens, out_device=None, stream=None, forced_codes=None):
        """lists of per-utterance tensors (as for ``nar``) -> list of (T_i, Q) int64 code tensors.  ``forced_codes``: optional
        list of (T_i, Q) tensors, per-stage teacher forcing as in ``nar`` (vx_nar_batch_ex)."""
        n, Q = len(texts), self.cfg.num_quantizers
        texts = [t.to(torch.int64).contiguous() for t in texts]
        prompts = [p.to(torch.int64).contiguous() for p in prompts]
        tokens = [t.to(torch.int64).contiguous() for t in tokens]
        outs = [torch.empty((t.numel(), Q), dtype=torch.int64, device=out_device if out_device is not None else p.device)
                for t, p in zip(tokens, prompts)]
        ptrs = lambda ts: (C.c_void_p * n)(*[_ptr(t) for t in ts])
        ints = lambda vs: (C.c_int32 * n)(*vs)
        fc = None
        if forced_codes is not None:
            forced_codes = [f.to(torch.int64).contiguous() for f in forced_codes]
            fc = ptrs(forced_codes)
        _check(self.lib.vx_nar_batch_ex(self.h, n, ptrs(texts), ints([t.numel() for t in texts]), ptrs(prompts),
                                        ints([p.shape[0] for p in prompts]), ptrs(tokens), ints([t.numel() for t in tokens]),
                                        ptrs(outs), fc, stream))
        return outs

    # -- scoring (vx_score / vx_score_batch) ----------------------------------------------------------
    def score(self, text: torch.Tensor, text_nar: torch.Tensor, codes: torch.Tensor, prompt_frames: int, ar: bool = True,
              nar: bool = True, stream=None):
        """Teacher-forced score of ``codes`` (A, Q) with the first ``prompt_frames`` frames as the prompt (vx_score).  Returns
        device tensors (ar_nll (T+1,) fp32, ar_rank (T+1,) int32, nar_nll (Q-1, T) fp32, nar_rank (Q-1, T) int32); a part that
        is switched off (or the NAR part of a Q = 1 model) is None."""
        text = text.to(torch.int64).contiguous()
        text_nar = text_nar.to(torch.int64).contiguous()
        codes = codes.to(torch.int64).contiguous()
        A, Q = codes.shape
        assert Q == self.cfg.num_quantizers, (Q, self.cfg.num_quantizers)
        P, T = int(prompt_frames), A - int(prompt_frames)
        dev = torch.device("cuda", self.device)
        nar = nar and Q > 1
        an = torch.empty(max(T + 1, 0), dtype=torch.float32, device=dev) if ar else None
        ak = torch.empty(max(T + 1, 0), dtype=torch.int32, device=dev) if ar else None
        nn_ = torch.empty((Q - 1, max(T, 0)), dtype=torch.float32, device=dev) if nar else None
        nk = torch.empty((Q - 1, max(T, 0)), dtype=torch.int32, device=dev) if nar else None
        _check(self.lib.vx_score(self.h, _ptr(text), text.numel(), _ptr(text_nar), text_nar.numel(), _ptr(codes), A, P,
                                 _ptr(an), _ptr(ak), _ptr(nn_), _ptr(nk), stream))
        return an, ak, nn_, nk

    def score_batch(self, texts, texts_nar, codes, prompt_frames, ar: bool = True, nar: bool = True, stream=None):
        """``score`` of n utterances in one pass over the concatenated rows (vx_score_batch): lists of per-utterance tensors and
        prompt lengths -> list of per-utterance (ar_nll, ar_rank, nar_nll, nar_rank) device tensors."""
        n, Q = len(texts), self.cfg.num_quantizers
        texts = [t.to(torch.int64).contiguous() for t in texts]
        texts_nar = [t.to(torch.int64).contiguous() for t in texts_nar]
        codes = [c.to(torch.int64).contiguous() for c in codes]
        P = [int(p) for p in prompt_frames]
        A = [c.shape[0] for c in codes]
        dev = torch.device("cuda", self.device)
        nar = nar and Q > 1
        mk = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        an = [mk(max(a - p + 1, 0), torch.float32) for a, p in zip(A, P)] if ar else None
        ak = [mk(max(a - p + 1, 0), torch.int32) for a, p in zip(A, P)] if ar else None
        nn_ = [mk((Q - 1, max(a - p, 0)), torch.float32) for a, p in zip(A, P)] if nar else None
        nk = [mk((Q - 1, max(a - p, 0)), torch.int32) for a, p in zip(A, P)] if nar else None
        ptrs = lambda ts: None if ts is None else (C.c_void_p * n)(*[_ptr(t) for t in ts])
        ints = lambda vs: (C.c_int32 * n)(*vs)
        _check(self.lib.vx_score_batch(self.h, n, ptrs(texts), ints([t.numel() for t in texts]), ptrs(texts_nar),
                                       ints([t.numel() for t in texts_nar]), ptrs(codes), ints(A), ints(P), ptrs(an), ptrs(ak),
                                       ptrs(nn_), ptrs(nk), stream))
        none = [None] * n
        return list(zip(an or none, ak or none, nn_ or none, nk or none))

    # -- alignment (vx_align) --------------------------------------------------------------------------
    def align(self, text: torch.Tensor, codes: torch.Tensor, prompt_frames: int, c0: int = 0, c1: Optional[int] = None,
              head_w: Optional[torch.Tensor] = None, path: bool = True, per_head: bool = False, stream=None):
        """The attention the AR decoder pays to text tokens [c0, c1) while it predicts frames prompt_frames .. A-1 of ``codes``
        (A, Q), teacher-forced (vx_align).  ``head_w``: (L, H) weights used as given (None: uniform).  Returns device tensors
        (attn (T, c1-c0) fp32, mass (T,) fp32, path (T,) int32 or None, path_score (1,) float64 or None, per_head (L, H, T, c1-c0)
        fp32 or None)."""
        text = text.to(torch.int64).contiguous()
        codes = codes.to(torch.int64).contiguous()
        A, Q = codes.shape
        assert Q == self.cfg.num_quantizers, (Q, self.cfg.num_quantizers)
        S, P = text.numel(), int(prompt_frames)
        c0, c1 = int(c0), S if c1 is None else int(c1)
        T, Sw = max(A - P, 0), max(c1 - c0, 0)
        L, H = self.cfg.num_decoder_layers, self.cfg.nhead
        hw = None
        if head_w is not None:
            hw = torch.as_tensor(head_w).detach().to("cpu", torch.float32).contiguous()
            assert tuple(hw.shape) == (L, H), (tuple(hw.shape), (L, H))
        dev = torch.device("cuda", self.device)
        attn = torch.empty((T, Sw), dtype=torch.float32, device=dev)
        mass = torch.empty(T, dtype=torch.float32, device=dev)
        pth = torch.empty(T, dtype=torch.int32, device=dev) if path else None
        psc = torch.empty(1, dtype=torch.float64, device=dev) if path else None
        ph = torch.empty((L, H, T, Sw), dtype=torch.float32, device=dev) if per_head else None
        _check(self.lib.vx_align(self.h, _ptr(text), S, _ptr(codes), A, P, c0, c1, _ptr(hw), _ptr(attn), _ptr(mass), _ptr(pth),
                                 _ptr(psc), _ptr(ph), stream))
        return attn, mass, pth, psc, ph

    def align_batch(self, texts, codes, prompt_frames, c0=None, head_w: Optional[torch.Tensor] = None, path: bool = True, stream=None):
        """``align`` of n utterances in one pass over the concatenated rows (vx_align_batch): lists of per-utterance tensors,
        prompt lengths and window starts (``c0``, default 0; the windows end at the end of each text); ``head_w`` is shared.
        Returns a list of per-utterance (attn, mass, path or None, path_score or None) device tensors.  VxError code 5 on an engine
        vx_align_batch does not serve."""
        n, Q = len(texts), self.cfg.num_quantizers
        texts = [t.to(torch.int64).contiguous() for t in texts]
        codes = [c.to(torch.int64).contiguous() for c in codes]
        assert all(c.dim() == 2 and c.shape[1] == Q for c in codes), (Q, [tuple(c.shape) for c in codes])
        P = [int(p) for p in prompt_frames]
        A = [c.shape[0] for c in codes]
        S = [t.numel() for t in texts]
        c0 = [0] * n if c0 is None else [int(v) for v in c0]
        L, H = self.cfg.num_decoder_layers, self.cfg.nhead
        hw = None
        if head_w is not None:
            hw = torch.as_tensor(head_w).detach().to("cpu", torch.float32).contiguous()
            assert tuple(hw.shape) == (L, H), (tuple(hw.shape), (L, H))
        dev = torch.device("cuda", self.device)
        T = [max(a - p, 0) for a, p in zip(A, P)]
        Sw = [max(s - c, 0) for s, c in zip(S, c0)]
        attn = [torch.empty((t, w), dtype=torch.float32, device=dev) for t, w in zip(T, Sw)]
        mass = [torch.empty(t, dtype=torch.float32, device=dev) for t in T]
        pth = [torch.empty(t, dtype=torch.int32, device=dev) for t in T] if path else None
        psc = [torch.empty(1, dtype=torch.float64, device=dev) for _ in T] if path else None
        ptrs = lambda ts: None if ts is None else (C.c_void_p * n)(*[_ptr(t) for t in ts])
        ints = lambda vs: (C.c_int32 * n)(*vs)
        _check(self.lib.vx_align_batch(self.h, n, ptrs(texts), ints(S), ptrs(codes), ints(A), ints(P), ints(c0), ints(S), _ptr(hw),
                                       ptrs(attn), ptrs(mass), ptrs(pth), ptrs(psc), stream))
        none = [None] * n
        return list(zip(attn, mass, pth or none, psc or none))

    def align_ms(self) -> float:
        """Device ms of the last ``align`` / ``align_batch``."""
        buf = (C.c_double * 13)()
        _check(self.lib.vx_get_timings(self.h, buf, 13))
        return buf[12]

    def score_timings(self):
        """Device ms of the AR and the NAR part of the last ``score`` / ``score_batch``."""
        buf = (C.c_double * 12)()
        _check(self.lib.vx_get_timings(self.h, buf, 12))
        return dict(score_ar_ms=buf[10], score_nar_ms=buf[11])

    def timings(self):
        buf = (C.c_double * 10)()
        _check(self.lib.vx_get_timings(self.h, buf, 10))
        return dict(prefill_ms=buf[0], decode_ms=buf[1], nar_ms=buf[2], n_pass=int(buf[3]), launches=int(buf[4]),
                    batch_decode_ms=buf[5], batch_launches=int(buf[6]), nar_gemm_ms=buf[7], nar_gemm_flops=buf[8],
                    step_kernels=int(buf[9]))

    def read(self, name: str, shape, dtype=torch.float32, offset_bytes: int = 0) -> torch.Tensor:
        out = torch.empty(shape, dtype=dtype)
        _check(self.lib.vx_read_buffer(self.h, name.encode(), _ptr(out), offset_bytes, out.numel() * out.element_size()))
        return out

    def read_ar_kv(self) -> torch.Tensor:
        """The batch-1 KV cache as (L, 2, H, max_text + max_audio, head_dim): K and V of every layer, fp32 on fp32 engines,
        else bfloat16 (the values the decode attention reads)."""
        return _kv_tap(self.read, "ar_kv", self.cfg.num_decoder_layers, self.cfg.nhead, self.cfg.decoder_dim,
                       self.max_text + self.max_audio, self.precision)

    def read_ar_mem(self) -> torch.Tensor:
        """VALL-F engines: the text memory of the batch-1 cross-attention as (L, 2, H, max_text, head_dim), K and V of every
        layer in the cache's element type.  Rows at and past the last prefilled text's length hold whatever an earlier, longer
        text left there."""
        return _kv_tap(self.read, "ar_mem", self.cfg.num_decoder_layers, self.cfg.nhead, self.cfg.decoder_dim, self.max_text,
                       self.precision)


def _kv_tap(read, name: str, L: int, H: int, d: int, rows: int, precision: str) -> torch.Tensor:
    """A K / V tap ("ar_kv", "ar_mem") through ``read(name, shape, dtype)`` as (L, 2, H, rows, head_dim) in the cache's element
    type: fp32 on fp32 engines, else bfloat16."""
    dtype = torch.float32 if precision in ("fp32", "f32") else torch.bfloat16
    return read(name, (L, 2, H, rows, d // H), dtype)


# ---- kernel-level ops (parity tests call the HIP kernels through the same C ABI) -------------------
def _struct_top_p(top_p) -> float:
    """vx_decode_params.top_p of a Python top_p: 1.0 (the reference's default, no nucleus filter) -> 0, the struct's "off",
    so that calls without the keyword pass exactly the bytes they passed before the field existed.  Other values go through
    unchanged (the engine refuses NaN and negative values, treats >= 1 as off)."""
    top_p = float(top_p)
    return 0.0 if top_p == 1.0 else top_p


def _prec(t_or_name) -> int:
    if isinstance(t_or_name, str):
        return VX_PREC_BF16 if t_or_name == "bf16" else VX_PREC_F32
    return VX_PREC_BF16 if t_or_name.dtype == torch.bfloat16 else VX_PREC_F32


def op_layernorm(x, gamma, beta, ada_w=None, ada_b=None, out_dtype=torch.float32):
    lib = load_library()
    rows, d = x.shape
    out = torch.empty((rows, d), dtype=out_dtype, device=x.device)
    _check(lib.vx_op_layernorm(_prec(out), _ptr(x), _ptr(gamma), _ptr(beta), _ptr(ada_w), _ptr(ada_b), _ptr(out), rows, d,
                               current_stream_ptr(x.device)))
    return out


def op_gemv(W, bias, x, relu=False):
    lib = load_library()
    N, K = W.shape
    y = torch.empty(N, dtype=torch.float32, device=x.device)
    _check(lib.vx_op_gemv(_prec(W), _ptr(W), _ptr(bias), _ptr(x), _ptr(y), N, K, int(relu), current_stream_ptr(x.device)))
    return y


def op_gemm(A, W, bias=None, relu=False, mfma=False, out=None):
    """out: a caller's contiguous fp32 (M, N) buffer (a view into a guarded block, say) in place of a fresh one."""
    lib = load_library()
    M, K = A.shape
    N = W.shape[0]
    Cm = torch.empty((M, N), dtype=torch.float32, device=A.device) if out is None else out
    assert Cm.shape == (M, N) and Cm.dtype == torch.float32
    _check(lib.vx_op_gemm(_prec(A), int(mfma), _ptr(A), _ptr(W), _ptr(bias), _ptr(Cm), M, N, K, int(relu),
                          current_stream_ptr(A.device)))
    return Cm


def op_gemm_rows(A, W, bias, relu=False, resid=None, vt_cols=0):
    """The engine's row-path GEMM forms (vx_op_gemm_rows) on bf16 A (M, K), W (N, K): resid=None -> (C bf16 (M, N), V^T copy of
    the last vt_cols columns (vt_cols, ld) or None); resid = fp32 (M, N) -> updated in place (resid += A.W^T + bias), returned."""
    lib = load_library()
    M, K = A.shape
    N = W.shape[0]
    if resid is not None:
        _check(lib.vx_op_gemm_rows(1, _ptr(A), _ptr(W), _ptr(bias), _ptr(resid), M, N, K, 0, None, 0, 0, current_stream_ptr(A.device)))
        return resid
    Cm = torch.empty((M, N), dtype=torch.bfloat16, device=A.device)
    ld = (M + 255) // 256 * 256
    vt = torch.zeros((vt_cols, ld), dtype=torch.bfloat16, device=A.device) if vt_cols else None
    _check(lib.vx_op_gemm_rows(0, _ptr(A), _ptr(W), _ptr(bias), _ptr(Cm), M, N, K, int(relu), _ptr(vt), N - vt_cols, ld,
                               current_stream_ptr(A.device)))
    return Cm, vt


def op_gemm_partial(A, W, slabs, splits, M=None):
    """The row path's split-K launch (vx_op_gemm_partial) on bf16 A (>= M, K), W (N, K): slab z of the fp32 buffer `slabs` (its
    first splits * M * N elements, as (splits, M, N)) = A[:M, z K / splits : (z + 1) K / splits] @ W[:, same].T"""
    lib = load_library()
    M = A.shape[0] if M is None else M
    K, N = A.shape[1], W.shape[0]
    assert slabs.dtype == torch.float32 and slabs.numel() >= splits * M * N and A.shape[0] >= M and W.shape[1] == K
    _check(lib.vx_op_gemm_partial(_ptr(A), _ptr(W), _ptr(slabs), M, N, K, splits, current_stream_ptr(A.device)))
    return slabs


def op_ln_fold(x, rows, d, out=None, gamma=None, beta=None, ada_w=None, ada_b=None, part=None, nsplit=0, part_stride=0, pbias=None,
               xout=None, out_dtype=torch.bfloat16):
    """layernorm_rows_kernel with its optional arguments (vx_op_ln_fold) on the first `rows` rows of fp32 x (>= rows, d), in place:
    part / nsplit / part_stride / pbias: the split-K fold; out (fp32 or bf16): the normalised rows (None: fold only, on the
    kernel instance of out_dtype); xout: where the fp32 normalised rows also go (may be x itself)."""
    lib = load_library()
    prec = _prec(out) if out is not None else (VX_PREC_BF16 if out_dtype == torch.bfloat16 else VX_PREC_F32)
    _check(lib.vx_op_ln_fold(prec, _ptr(x), _ptr(part), nsplit, part_stride, _ptr(pbias), _ptr(gamma), _ptr(beta), _ptr(ada_w),
                             _ptr(ada_b), _ptr(out), _ptr(xout), rows, d, current_stream_ptr(x.device)))


def op_rows_plan(M, d, num_cu=0):
    """(splitk, sp_d, sp_ff) of the row stack over M rows of width d (vx_op_rows_plan); num_cu = 0: the current device's count"""
    out = (C.c_int32 * 3)()
    _check(load_library().vx_op_rows_plan(M, d, num_cu, out))
    return tuple(out)


def op_gemm_mx(A, W, bias=None, relu=False, out_mx=False, return_quant=False):
    """MXFP8 GEMM (vx_op_gemm_mx): fp32 A (M, K), W (N, K) on the GPU.  out_mx=False -> C (M, N) fp32; True -> (e4m3 bytes (M, N),
    E8M0 scales (N/32, ld)) of ReLU(C + bias).  return_quant adds the engine's quantisation of A: (bytes (M, K), scales (K/32, ld))."""
    lib = load_library()
    M, K = A.shape
    N = W.shape[0]
    ld = (M + 255) // 256 * 256
    dev = A.device
    if out_mx:
        c = torch.empty((M, N), dtype=torch.uint8, device=dev)
        sc = torch.empty((N // 32, ld), dtype=torch.uint8, device=dev)
    else:
        c, sc = torch.empty((M, N), dtype=torch.float32, device=dev), None
    qa = torch.empty((M, K), dtype=torch.uint8, device=dev) if return_quant else None
    sa = torch.empty((K // 32, ld), dtype=torch.uint8, device=dev) if return_quant else None
    _check(lib.vx_op_gemm_mx(_ptr(A), _ptr(W), _ptr(bias), _ptr(c), _ptr(sc), M, N, K, int(relu), 2 if out_mx else 0, _ptr(qa), _ptr(sa),
                             current_stream_ptr(dev)))
    res = (c, sc) if out_mx else c
    return (res, qa, sa) if return_quant else res


def op_layernorm_mx(x, gamma, beta, ada_w=None, ada_b=None):
    lib = load_library()
    rows, d = x.shape
    ld = (rows + 255) // 256 * 256
    q = torch.empty((rows, d), dtype=torch.uint8, device=x.device)
    sc = torch.empty((d // 32, ld), dtype=torch.uint8, device=x.device)
    _check(lib.vx_op_layernorm_mx(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(ada_w), _ptr(ada_b), _ptr(q), _ptr(sc), rows, d,
                                  current_stream_ptr(x.device)))
    return q, sc


def op_attention(qkv, nhead, text_len=-1, mfma=False):
    lib = load_library()
    rows, d3 = qkv.shape
    d = d3 // 3
    out = torch.empty((rows, d), dtype=qkv.dtype, device=qkv.device)
    _check(lib.vx_op_attention(_prec(qkv), int(mfma), _ptr(qkv), _ptr(out), rows, nhead, d // nhead, text_len,
                               current_stream_ptr(qkv.device)))
    return out


def _i32(vals):
    return None if vals is None else (C.c_int32 * len(vals))(*[int(v) for v in vals])


def op_attention_segs(qkv, nhead, starts, lens, texts=None, out=None):
    """Segmented flash attention (vx_op_attention_segs) over bf16 qkv (rows, 3 d): segment z = rows [starts[z], starts[z] + lens[z]),
    prefix mask texts[z] (None: no mask).  `out` (rows, d) bf16 may be supplied: rows outside the segments are left as they are."""
    lib = load_library()
    assert qkv.dtype == torch.bfloat16
    rows, d3 = qkv.shape
    d = d3 // 3
    if out is None:
        out = torch.zeros((rows, d), dtype=qkv.dtype, device=qkv.device)
    assert out.dtype == torch.bfloat16 and out.shape == (rows, d)
    _check(lib.vx_op_attention_segs(_ptr(qkv), _ptr(out), rows, nhead, d // nhead, len(starts), _i32(starts), _i32(lens), _i32(texts),
                                    current_stream_ptr(qkv.device)))
    return out


def op_cross_attention_segs(q, mem, mem_off, head_stride, v_offset, klens, nhead, starts, lens, out=None):
    """Segmented cross-attention (vx_op_cross_attention_segs): q (rows, ldq) bf16, head h at columns [64 h, 64 h + 64); segment z = rows
    [starts[z], starts[z] + lens[z]) attends to the klens[z] keys of its own memory: element (h, j, c) of K at mem.flatten()[mem_off[z]
    + h head_stride + 64 j + c], V at + v_offset.  `out` (rows, 64 nhead) bf16 may be supplied: rows outside the segments are left as
    they are."""
    lib = load_library()
    assert q.dtype == torch.bfloat16 and q.dim() == 2 and q.is_contiguous() and mem.dtype == torch.bfloat16 and mem.is_contiguous()
    rows, ldq = q.shape
    if out is None:
        out = torch.zeros((rows, 64 * nhead), dtype=torch.bfloat16, device=q.device)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and out.shape == (rows, 64 * nhead)
    n = len(starts)
    assert len(lens) == n and len(klens) == n and len(mem_off) == n
    need = max(int(o) + (nhead - 1) * int(head_stride) + int(v_offset) + int(k) * 64 for o, k in zip(mem_off, klens))
    assert need <= mem.numel(), "a segment's memory lies outside `mem`"
    off = (C.c_int64 * n)(*[int(v) for v in mem_off])
    _check(lib.vx_op_cross_attention_segs(_ptr(q), ldq, _ptr(mem), off, int(head_stride), int(v_offset), _i32(klens), _ptr(out), rows,
                                          nhead, n, _i32(starts), _i32(lens), current_stream_ptr(q.device)))
    return out


def op_attn_slots(q, kv, kv_scale, ctx, done, ctx_max, out=None, slot_stride=None, v_offset=None):
    """The batched decode attention (vx_op_attn_slots) of B = len(ctx) slots: q (B, d) fp32; kv bf16 (bf16 caches) or uint8 e4m3
    codes with kv_scale uint8 scale bytes (fp8 caches).  kv may be a strided view (B, 2, H, ctx_max, 64) - one layer of a larger
    cache - whose data pointer is the layer base; slot_stride / v_offset (elements) default to its strides of dims 0 and 1, and
    kv_scale's data pointer is the matching scale base.  done (None: all live): slots whose `out` rows are left as they are."""
    lib = load_library()
    B, d = q.shape
    assert q.dtype == torch.float32 and q.is_contiguous() and len(ctx) == B and (done is None or len(done) == B)
    fp8 = kv.dtype == torch.uint8
    assert fp8 == (kv_scale is not None)
    slot_stride = kv.stride(0) if slot_stride is None else slot_stride
    v_offset = kv.stride(1) if v_offset is None else v_offset
    if out is None:
        out = torch.zeros((B, d), dtype=torch.bfloat16, device=q.device)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and out.shape == (B, d)
    _check(lib.vx_op_attn_slots(int(fp8), _ptr(q), kv.data_ptr(), None if kv_scale is None else kv_scale.data_ptr(), slot_stride,
                                v_offset, ctx_max, B, d // 64, _i32(ctx), _i32(done), _ptr(out), current_stream_ptr(q.device)))
    return out


def op_attn_mem_slots(q, mem, lens, done, out=None):
    """The VALL-F slot step's cross-attention (vx_op_attn_mem_slots) of B = len(lens) slots: q (B, d) fp32; mem bf16 (B, 2, H, max_text,
    64) - or a strided view of one layer of the engine's slot memory - slot b attends to its first lens[b] rows.  done (None: all
    live): slots whose `out` rows are left as they are."""
    lib = load_library()
    B, d = q.shape
    assert q.dtype == torch.float32 and q.is_contiguous() and len(lens) == B and (done is None or len(done) == B)
    assert mem.dtype == torch.bfloat16 and mem.dim() == 5 and mem.shape[0] == B and mem.shape[4] == 64
    if out is None:
        out = torch.zeros((B, d), dtype=torch.bfloat16, device=q.device)
    assert out.dtype == torch.bfloat16 and out.is_contiguous() and out.shape == (B, d)
    _check(lib.vx_op_attn_mem_slots(_ptr(q), mem.data_ptr(), mem.stride(0), mem.stride(1), mem.shape[3], B, d // 64, _i32(lens),
                                    _i32(done), _ptr(out), current_stream_ptr(q.device)))
    return out


def op_bgemm(epi, A, W, bias, B, kgroups=1, done=None, row=None, pass_=None, q=None, kv=None, kv_scale=None, d=0, ctx_max=0,
             f=None, part=None, logits=None, trace=None, slot_map=None):
    """One launch of the batched step's GEMM (vx_op_bgemm) in epilogue `epi` (BE_*) on A bf16 (32 or 64, K), W bf16 (N, K) and the
    caller's output buffers, which are written in place: q fp32, kv a strided (slots, 2, H, ctx_max, 64) view of a bf16 cache or of
    uint8 e4m3 codes (kv_scale: the matching scale bytes), f bf16 (>= B, N), part fp32 (kgroups, 64, N), logits fp32 (rows, stride),
    trace fp32 (slots, trace_rows, N).  done / row / pass_ / slot_map: host sequences (None: zeros)."""
    lib = load_library()
    assert A.dtype == W.dtype == torch.bfloat16 and A.is_contiguous() and W.is_contiguous()
    N, K = W.shape
    kv8 = kv is not None and kv.dtype == torch.uint8
    assert kv8 == (kv_scale is not None)
    ls = 0 if logits is None else logits.stride(0)
    tr = 0 if trace is None else trace.shape[1]
    _check(lib.vx_op_bgemm(epi, int(kv8), _ptr(A), _ptr(W), _ptr(bias), N, K, B, kgroups, _i32(done), _i32(row), _i32(pass_), _ptr(q),
                           None if kv is None else kv.data_ptr(), None if kv_scale is None else kv_scale.data_ptr(),
                           0 if kv is None else kv.stride(0), 0 if kv is None else kv.stride(1), d, ctx_max, _ptr(f), _ptr(part),
                           None if logits is None else logits.data_ptr(), ls, _ptr(trace), tr, _i32(slot_map), current_stream_ptr(A.device)))


def op_ln_batch(x, gamma, beta, h, B, part=None, pbias=None, kgroups=0, slot_map=None):
    """The batched step's LayerNorm (vx_op_ln_batch) in place: x fp32 (64, d) (written back when kgroups > 0), part fp32
    (kgroups, 64, d), h bf16 (>= B, d); slot_map (host sequence, kgroups 0): batched prefill's mapped form."""
    lib = load_library()
    d = x.shape[1]
    assert x.dtype == torch.float32 and h.dtype == torch.bfloat16
    _check(lib.vx_op_ln_batch(_ptr(x), _ptr(part), kgroups, _ptr(pbias), _ptr(gamma), _ptr(beta), _ptr(h), B, d, _i32(slot_map),
                              current_stream_ptr(x.device)))


def op_nll_rows(logits, targets, V=None):
    """nll_rows_kernel on device logits (rows, ld) fp32 (a row's first V columns; default all) and int64 targets (rows,):
    (nll fp32, rank int32, argmax int32), each (rows,)."""
    lib = load_library()
    rows, ld = logits.shape
    V = ld if V is None else int(V)
    assert logits.dtype == torch.float32 and logits.is_contiguous() and targets.dtype == torch.int64
    nll = torch.empty(rows, dtype=torch.float32, device=logits.device)
    rank = torch.empty(rows, dtype=torch.int32, device=logits.device)
    am = torch.empty(rows, dtype=torch.int32, device=logits.device)
    _check(lib.vx_op_nll_rows(_ptr(logits), rows, V, ld, _ptr(targets.contiguous()), _ptr(nll), _ptr(rank), _ptr(am),
                              current_stream_ptr(logits.device)))
    return nll, rank, am


ALIGN_TILE_ROWS = 32  # query rows of one workgroup of attn_text_rows_kernel (csrc/align.hpp)


def op_attn_text_rows(q, k, nhead, hd, text_len, causal, c0, c1, head_w, attn, mass=None, per_head=None, first=True, row0=0,
                      ldk=None, k_head_stride=None):
    """attn_text_rows_kernel on device buffers (vx_op_attn_text_rows): q (rows, ldq), head h at columns [h hd, (h + 1) hd); k any
    contiguous tensor, key j of head h at k.flatten()[j ldk + h k_head_stride:][:hd] (default: rows of q's width, heads side by
    side).  ``attn`` (rows, c1-c0) fp32 and ``mass`` (rows,) are updated in place (``first``: stored); ``per_head`` (nhead, rows,
    c1-c0) is filled.  The operands' extents are checked here: the kernel trusts them."""
    lib = load_library()
    assert q.dim() == 2 and q.is_contiguous() and k.is_contiguous() and q.dtype == k.dtype
    rows, ldq = q.shape
    ldk = k.shape[-1] if ldk is None else int(ldk)
    khs = hd if k_head_stride is None else int(k_head_stride)
    nkeys = text_len + row0 + rows if causal else text_len
    assert nhead * hd <= ldq and (nkeys - 1) * ldk + (nhead - 1) * khs + hd <= k.numel(), "q / k smaller than the launch reads"
    Sw = c1 - c0
    assert head_w.dtype == torch.float32 and head_w.numel() == nhead and head_w.is_cuda
    assert attn.dtype == torch.float32 and attn.is_contiguous() and tuple(attn.shape) == (rows, Sw)
    assert mass is None or (mass.dtype == torch.float32 and mass.numel() == rows)
    assert per_head is None or (per_head.dtype == torch.float32 and per_head.is_contiguous() and tuple(per_head.shape) == (nhead, rows, Sw))
    _check(lib.vx_op_attn_text_rows(_prec(q), _ptr(q), ldq, _ptr(k), ldk, khs, rows, int(row0), nhead, hd, text_len, int(bool(causal)),
                                    c0, c1, _ptr(head_w), _ptr(attn), _ptr(mass), _ptr(per_head), int(bool(first)),
                                    current_stream_ptr(q.device)))
    return attn


def op_mono_path(attn):
    """mono_path_kernel on a device map (T, Sw) fp32 (vx_op_mono_path): (path (T,) int32, score (1,) float64), on the device."""
    lib = load_library()
    assert attn.dtype == torch.float32 and attn.dim() == 2 and attn.is_contiguous() and attn.is_cuda
    T, Sw = attn.shape
    path = torch.empty(T, dtype=torch.int32, device=attn.device)
    score = torch.empty(1, dtype=torch.float64, device=attn.device)
    _check(lib.vx_op_mono_path(_ptr(attn), T, Sw, _ptr(path), _ptr(score), current_stream_ptr(attn.device)))
    return path, score


def op_attn_text_segs(qkv, nhead, segs, head_w, attn, mass=None, first=True):
    """attn_text_seg_kernel + the head pass on device buffers (vx_op_attn_text_segs): qkv (M, 3 d) bf16 packed rows, d = 64 nhead;
    ``segs``: one (start, text_len, qfirst, rows, row0, c0, c1, cell_off, row_off) per segment (AlignSeg, csrc/align.hpp); ``attn``
    (cells,) and ``mass`` (rows_total,) fp32, flat, are updated in place (``first``: stored).  The operands' extents are checked here:
    the kernel trusts them."""
    lib = load_library()
    d = 64 * nhead
    assert qkv.dtype == torch.bfloat16 and qkv.dim() == 2 and qkv.is_contiguous() and qkv.is_cuda and qkv.shape[1] == 3 * d
    assert head_w.dtype == torch.float32 and head_w.numel() == nhead and head_w.is_cuda
    assert attn.dtype == torch.float32 and attn.dim() == 1 and attn.is_contiguous() and attn.is_cuda
    assert mass is None or (mass.dtype == torch.float32 and mass.dim() == 1 and mass.is_contiguous() and mass.is_cuda)
    segs = [tuple(int(v) for v in g) for g in segs]
    for start, text_len, qfirst, rows, row0, c0, c1, cell_off, row_off in segs:
        assert start % 64 == 0 and start + qfirst + rows <= qkv.shape[0] and start + text_len + row0 + rows <= qkv.shape[0], "rows outside qkv"
        assert 0 <= cell_off and cell_off + rows * (c1 - c0) <= attn.numel() and 0 <= row_off
        assert mass is None or row_off + rows <= mass.numel()
    rows_total = mass.numel() if mass is not None else max(g[8] + g[3] for g in segs)
    flat = [v for g in segs for v in g]
    k = qkv.view(-1)[d:]
    _check(lib.vx_op_attn_text_segs(_ptr(qkv), _ptr(k), 3 * d, len(segs), (C.c_int64 * len(flat))(*flat), nhead, _ptr(head_w), _ptr(attn),
                                    _ptr(mass), attn.numel(), rows_total, int(bool(first)), current_stream_ptr(qkv.device)))
    return attn


def op_mono_path_segs(attn, maps):
    """mono_path_seg_kernel on a flat device buffer of maps (vx_op_mono_path_segs): ``maps`` = one (T, Sw, cell_off) per map ->
    (paths, a list of (T,) int32 views; scores (n,) float64), on the device."""
    lib = load_library()
    assert attn.dtype == torch.float32 and attn.dim() == 1 and attn.is_contiguous() and attn.is_cuda
    flat, row_off = [], 0
    for T, Sw, cell_off in maps:
        assert 0 <= cell_off and cell_off + T * Sw <= attn.numel()
        flat += [int(T), int(Sw), int(cell_off), row_off]
        row_off += int(T)
    path = torch.empty(row_off, dtype=torch.int32, device=attn.device)
    score = torch.empty(len(maps), dtype=torch.float64, device=attn.device)
    _check(lib.vx_op_mono_path_segs(_ptr(attn), len(maps), (C.c_int64 * len(flat))(*flat), _ptr(path), _ptr(score),
                                    current_stream_ptr(attn.device)))
    return list(torch.split(path, [int(m[0]) for m in maps])), score


def op_dtw_cost(a, b, n_ceps):
    """The cepstra and cost kernels of vx_dtw_compare on one pair (vx_op_dtw_cost): a (Ta, D), b (Tb, D) float32 on the device ->
    the (Ta, Tb) float32 cost matrix, of the rows' first ``n_ceps`` cepstra or, with ``n_ceps`` = 0, of the rows as given."""
    lib = load_library()
    for t in (a, b):
        assert t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous() and t.is_cuda and t.shape[1] == a.shape[1]
    cost = torch.empty((a.shape[0], b.shape[0]), dtype=torch.float32, device=a.device)
    _check(lib.vx_op_dtw_cost(a.shape[1], int(n_ceps), _ptr(a), a.shape[0], _ptr(b), b.shape[0], _ptr(cost),
                              current_stream_ptr(a.device)))
    return cost


def op_dtw_path(cost, mats, want_path=True):
    """dtw_warp_kernel on a flat device buffer of cost matrices (vx_op_dtw_path): ``mats`` = one (Ta, Tb, cell_off) per matrix ->
    (totals (n,) float64, lengths (n,) int32, paths: a list of (length, 2) int32 tensors, or None), on the device."""
    lib = load_library()
    assert cost.dtype == torch.float32 and cost.dim() == 1 and cost.is_contiguous() and cost.is_cuda
    flat, path_off = [], 0
    for Ta, Tb, cell_off in mats:
        assert 0 <= cell_off and cell_off + Ta * Tb <= cost.numel()
        flat += [int(Ta), int(Tb), int(cell_off), path_off]
        path_off += int(Ta) + int(Tb) - 1
    path = torch.empty((path_off, 2), dtype=torch.int32, device=cost.device) if want_path else None
    total = torch.empty(len(mats), dtype=torch.float64, device=cost.device)
    length = torch.empty(len(mats), dtype=torch.int32, device=cost.device)
    _check(lib.vx_op_dtw_path(_ptr(cost), len(mats), (C.c_int64 * len(flat))(*flat), _ptr(total), _ptr(length), _ptr(path),
                              current_stream_ptr(cost.device)))
    if not want_path:
        return total, length, None
    lens = length.tolist()
    parts = torch.split(path, [int(m[0]) + int(m[1]) - 1 for m in mats])
    return total, length, [p[:n] for p, n in zip(parts, lens)]


def op_pitch_diff(wav, fmin, fmax, tau_max):
    """d' of pitch_track_kernel for one utterance (vx_op_pitch_diff): wav (L,) float32 on the device -> (frames, tau_max + 1)
    float32, ``tau_max`` = ceil(24000 / fmin)."""
    lib = load_library()
    assert wav.dtype == torch.float32 and wav.dim() == 1 and wav.is_contiguous() and wav.is_cuda
    out = torch.empty((int(lib.vx_fbank_frames(wav.numel())), int(tau_max) + 1), dtype=torch.float32, device=wav.device)
    if out.numel():  # an utterance without frames has no storage to point at, and nothing to write
        _check(lib.vx_op_pitch_diff(float(fmin), float(fmax), _ptr(wav), wav.numel(), _ptr(out), current_stream_ptr(wav.device)))
    return out


def op_sample(logits, top_k, temperature, exp_noise):
    lib = load_library()
    out = (C.c_int32 * 2)()
    _check(lib.vx_op_sample(_ptr(logits), logits.numel(), int(top_k), float(temperature), _ptr(exp_noise), out,
                            current_stream_ptr(logits.device)))
    return out[0], out[1]


def op_sample_topp(logits, top_k, temperature, top_p, exp_noise):
    """vx_op_sample_topp: (sampled, argmax) of one logits row under temperature, top-k and the nucleus filter."""
    lib = load_library()
    out = (C.c_int32 * 2)()
    _check(lib.vx_op_sample_topp(_ptr(logits), logits.numel(), int(top_k), float(temperature), _struct_top_p(top_p),
                                 _ptr(exp_noise), out, current_stream_ptr(logits.device)))
    return out[0], out[1]


def op_sample_logprob(logits, top_k, temperature, top_p, exp_noise):
    """vx_op_sample_logprob: (sampled, argmax, lp) - ``op_sample_topp`` on the sampler instantiation that also records the
    log-probability of the sampled token on the raw row."""
    lib = load_library()
    out = (C.c_int32 * 2)()
    lp = C.c_float()
    _check(lib.vx_op_sample_logprob(_ptr(logits), logits.numel(), int(top_k), float(temperature), _struct_top_p(top_p),
                                    _ptr(exp_noise), out, C.byref(lp), current_stream_ptr(logits.device)))
    return out[0], out[1], lp.value


def launch_floor(n_kernels=62, grid=256, block=256, iters=200):  # the three probes below need load_probe_library()
    lib = load_library()
    out = (C.c_double * 2)()
    _check(lib.vx_debug_launch_floor(n_kernels, grid, block, iters, out))
    return dict(graph_us_per_kernel=out[0], eager_us_per_kernel=out[1])


def stage_chain(nwg=256, stages=60, rows=12, mode=2, iters=20):
    lib = load_library()
    out = (C.c_double * 4)()
    _check(lib.vx_debug_stage_chain(nwg, stages, rows, mode, iters, out))
    return dict(us_per_launch=out[0], us_per_stage=out[1], max_err=out[2], spin_timeout=int(out[3]))


def l2_fill(grid=256, threads=256, unroll=8, region_bytes=2 << 20, iters=200):
    lib = load_library()
    out = (C.c_double * 3)()
    _check(lib.vx_debug_l2_fill(grid, threads, unroll, region_bytes, iters, out))
    return dict(gbs=out[0], bytes_per_clk_per_cu=out[1], ghz=out[2])


class MelEngine:
    """One mel-spectrogram Transformer replica on one GPU (the vx_mel_* entries of include/vallex.h)."""

    def __init__(self, cfg, precision: str = "bf16", max_text: int = 256, max_frames: int = 2560, device: int = 0,
                 no_graph: bool = False, scaling_xformers: bool = False):
        self.lib = load_library()
        self.cfg, self.device, self.precision = cfg, int(device), precision
        self.max_text, self.max_frames = int(max_text), int(max_frames)
        c = VxMelConfig()
        c.struct_size = C.sizeof(VxMelConfig)
        c.d_model, c.nhead, c.num_layers = cfg.d_model, cfg.nhead, cfg.num_layers
        c.norm_first, c.add_prenet, c.scaling_xformers = int(cfg.norm_first), int(cfg.add_prenet), int(scaling_xformers)
        c.precision = {"fp32": VX_PREC_F32, "f32": VX_PREC_F32, "bf16": VX_PREC_BF16}[precision]
        c.max_text, c.max_frames, c.device = self.max_text, self.max_frames, self.device
        c.flags = VX_MEL_NO_GRAPH if no_graph else 0
        h = C.c_void_p()
        _check(self.lib.vx_mel_create(C.byref(c), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.vx_mel_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_state_dict(self, sd, sine_table_: bool = True):
        from .weights import mel_expected_keys, sine_table

        for k, shape in mel_expected_keys(self.cfg).items():
            if k.endswith("num_batches_tracked"):  # BatchNorm's step counter: not read by the forward pass
                continue
            t = sd[k].detach().to(torch.float32).contiguous()
            assert tuple(t.shape) == tuple(shape), (k, tuple(t.shape), shape)
            shp = (C.c_int64 * t.dim())(*t.shape)
            _check(self.lib.vx_mel_set_weight(self.h, k.encode(), _ptr(t), shp, t.dim()))
        if sine_table_:
            rows = max(4000, self.max_text + self.max_frames + 2)
            pe = sine_table(rows, self.cfg.d_model)
            _check(self.lib.vx_mel_set_sine_table(self.h, _ptr(pe), rows, self.cfg.d_model))
        _check(self.lib.vx_mel_finalize(self.h))

    def encode(self, text: torch.Tensor, stream=None):
        text = text.to(torch.int64).contiguous()
        _check(self.lib.vx_mel_encode(self.h, _ptr(text), text.numel(), stream))

    def decode(self, max_frames: int = -1, stream=None):
        _check(self.lib.vx_mel_decode(self.h, int(max_frames), stream))

    def decode_forced(self, frames: torch.Tensor, stream=None):
        frames = frames.to(torch.float32).contiguous()
        assert frames.dim() == 2 and frames.shape[1] == NUM_MEL_BINS, tuple(frames.shape)
        _check(self.lib.vx_mel_decode_forced(self.h, _ptr(frames), frames.shape[0], stream))

    def result(self, out: Optional[torch.Tensor] = None, out_device="cpu"):
        """(frames (T, 100) fp32, stop reason name, stop logits (n_pass,) fp32 on the host).  ``out``: a caller buffer (rows, 100)
        whose first T rows are written; the returned frames are a view of it."""
        n, reason, n_pass = C.c_int32(), C.c_int32(), C.c_int32()
        _check(self.lib.vx_mel_result(self.h, None, 0, C.byref(n), C.byref(reason), None, C.byref(n_pass)))
        if out is None:
            out = torch.empty(n.value, NUM_MEL_BINS, dtype=torch.float32, device=out_device)
        assert out.dtype == torch.float32 and out.is_contiguous() and out.shape[1] == NUM_MEL_BINS
        stops = torch.empty(n_pass.value, dtype=torch.float32)
        _check(self.lib.vx_mel_result(self.h, _ptr(out) if out.shape[0] else None, out.shape[0], C.byref(n), C.byref(reason),
                                      _ptr(stops) if n_pass.value else None, C.byref(n_pass)))
        return out[: n.value], MEL_STOP_REASONS[reason.value], stops

    def teacher_forced(self, text: torch.Tensor, frames: torch.Tensor, out_device="cpu", stream=None):
        text = text.to(torch.int64).contiguous()
        frames = frames.to(torch.float32).contiguous()
        T = frames.shape[0]
        predict = torch.empty(T, NUM_MEL_BINS, dtype=torch.float32, device=out_device)
        stops = torch.empty(T, dtype=torch.float32, device=out_device)
        _check(self.lib.vx_mel_teacher_forced(self.h, _ptr(text), text.numel(), _ptr(frames), T, _ptr(predict), _ptr(stops), stream))
        return predict, stops

    def timings(self):
        buf = (C.c_double * 4)()
        _check(self.lib.vx_mel_get_timings(self.h, buf, 4))
        return {"decode_ms": buf[0], "step_launches": buf[1], "kernels_per_step": buf[2], "encode_ms": buf[3]}

    def read(self, name: str, shape, dtype=torch.float32, offset_bytes: int = 0) -> torch.Tensor:
        out = torch.empty(shape, dtype=dtype)
        _check(self.lib.vx_mel_read(self.h, name.encode(), _ptr(out), offset_bytes, out.numel() * out.element_size()))
        return out

    def read_kv(self) -> torch.Tensor:
        """The decoder's self-attention cache as (L, 2, H, max_text + max_frames + 2, head_dim), as Engine.read_ar_kv."""
        return _kv_tap(self.read, "ar_kv", self.cfg.num_layers, self.cfg.nhead, self.cfg.d_model,
                       self.max_text + self.max_frames + 2, self.precision)

    def read_mem(self) -> torch.Tensor:
        """Every decoder layer's cross K / V of the last encode as (L, 2, H, max_text, head_dim), as Engine.read_ar_mem."""
        return _kv_tap(self.read, "ar_mem", self.cfg.num_layers, self.cfg.nhead, self.cfg.d_model, self.max_text, self.precision)


MEL_STATE = ("row", "pass", "n_gen", "S", "done", "stop_reason")


def op_mel_open(xh, gamma, beta, Wh, bh, W0, b0, alpha, pe, x, frames, stops, state, W1=None, b1=None, W2=None, b2=None,
                max_frames=0, n_forced=0, forced=None, launches=1):
    """``launches`` launches of the mel decode step's opening kernel (vx_op_mel_open) on caller device buffers; x (d), frames
    (rows, 100) and stops are written in place.  state: dict of MEL_STATE (stop_reason optional).  Returns (state after, the
    arrival counter after the last launch)."""
    lib = load_library()
    st = (C.c_int32 * 6)(*[int(state.get(k, 0)) for k in MEL_STATE])
    arrive = C.c_uint32(0xFFFFFFFF)
    _check(lib.vx_op_mel_open(xh.numel(), _ptr(xh), _ptr(gamma), _ptr(beta), _ptr(Wh), _ptr(bh), _ptr(W1), _ptr(b1), _ptr(W2), _ptr(b2),
                              _ptr(W0), _ptr(b0), _ptr(alpha), _ptr(pe), pe.shape[0], _ptr(x), _ptr(frames), frames.shape[0], _ptr(stops),
                              stops.numel(), st, int(max_frames), int(n_forced), _ptr(forced), int(launches), C.byref(arrive),
                              current_stream_ptr(xh.device)))
    return dict(zip(MEL_STATE, st)), arrive.value
