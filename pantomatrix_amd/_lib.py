"""ctypes binding of libemage_hip.so (include/emage_hip.h).  There is NO fallback: if the library is
missing or a symbol is absent, importing the ops fails loudly."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libemage_hip.so")
TOOLS_LIB_PATH = os.path.join(_HERE, "csrc", "libemage_hip_tools.so")   # -DEMAGE_TOOLS twin: every tile configuration + emage_set_tuning

F32, BF16, F16X3, H2 = 0, 1, 2, 3
PCM_S16, PCM_S24, PCM_S32, PCM_F32 = 0, 1, 2, 3       # EMAGE_PCM_*: the sample formats of emage_audio_resample
AUDIO_TILE = 1024                                     # EMAGE_AUDIO_TILE: outputs per tile of emage_audio_resample
AUDIO_TAPS_LDS_BYTES, AUDIO_SPAN_LDS_BYTES = 96 * 1024, 64 * 1024      # EMAGE_AUDIO_*_LDS_BYTES: the LDS budgets a rate pair must fit
REP_JOINTS = 55                                       # EMAGE_REP_JOINTS: the joints of the pose layout, (T, 165)
ABI_VERSION = 20                                     # unchanged by the gradient-norm, clip-store and validation entry points: they were ADDED, no existing prototype moved

_p, _i, _f, _l, _d = C.c_void_p, C.c_int, C.c_float, C.c_long, C.c_double

class GemmProblem(C.Structure):
    """`emage_gemm_problem` of include/emage_hip.h: one emage_gemm call's arguments (emage_gemm_grouped takes an array of them)."""
    _fields_ = ([(n, _p) for n in ("A", "W", "bias", "slope", "res", "out", "out_f32", "out_t")]
                + [(n, _i) for n in ("lda", "ldr", "res_is_f32", "res_first", "ldo", "n_store", "ldf", "t_col0", "t_rows", "t_ld",
                                     "M", "N", "Cp", "taps", "stride", "pad", "Lin", "Lout")]
                + [("a_scale", _f), ("w_scale", _f)]
                + [(n, _p) for n in ("ln_stats", "ln_c", "rs_stats", "rs_gamma", "rs_beta", "st_out")]       # the LayerNorm fold (round 6; all NULL = off)
                + [("ln_np", _i), ("rs_np", _i), ("ln_eps", _f)]
                + [("sk_ws", _p), ("sk_ws_bytes", _l), ("sk_count", _p), ("sk_tiles", _i)])             # split-K fix-up scratch (round 6; NULL = off)


class QkvAttentionProblem(C.Structure):
    """`emage_qkv_attention_problem` of include/emage_hip.h (emage_qkv_attention_grouped takes an array of them)."""
    _fields_ = ([(n, _p) for n in ("A", "W", "bias", "ln_stats", "ln_c", "out")]
                + [(n, _i) for n in ("lda", "ldo", "B")]
                + [(n, _f) for n in ("a_scale", "w_scale", "ln_eps")])


class QAttentionProblem(C.Structure):
    """`emage_q_attention_problem` of include/emage_hip.h (emage_q_attention takes one, emage_q_attention_grouped an array of them)."""
    _fields_ = ([(n, _p) for n in ("A", "W", "bias", "ln_stats", "ln_c", "k", "vt", "out")]
                + [(n, _i) for n in ("lda", "ldk", "ldvt", "vt_rows", "ldo", "B")]
                + [(n, _f) for n in ("a_scale", "w_scale", "ln_eps")])


class QmAttentionProblem(C.Structure):
    """`emage_qm_attention_problem` of include/emage_hip.h (emage_qm_attention takes one, emage_qm_attention_grouped an array of them)."""
    _fields_ = ([(n, _p) for n in ("A", "W", "bias", "ln_stats", "ln_c", "mem", "Wkv", "bias_kv", "out")]
                + [(n, _i) for n in ("lda", "ldm", "km", "kv_layers", "kv_layer", "ldo", "B")]
                + [(n, _f) for n in ("a_scale", "w_scale", "wkv_scale", "ln_eps")])


class FinalizeEntry(C.Structure):
    """`emage_finalize_entry` of include/emage_hip.h (emage_col_sum_finalize_multi takes a host array of them)."""
    _fields_ = [("partial", _p), ("out", _p), ("chunks", _i), ("C", _i), ("accumulate", _i)]


class ValEntry(C.Structure):
    """`emage_val_entry` of include/emage_hip.h (emage_val_metrics takes a host array of them)."""
    _fields_ = ([(n, _p) for n in ("rec", "latent", "logits", "index", "pred")]
                + [(n, _i) for n in ("ld_rec", "ld_latent", "ld_logits", "C", "K", "pred_rows", "tag")]
                + [("pred_ld", _l), ("l_w", _d), ("c_w", _d)])


VAL_MAX_ENTRIES, VAL_TAGS, VAL_LOSSES = 12, 3, 7       # EMAGE_VAL_*: the accumulator block of emage_val_metrics, in 8-byte words
VAL_ACC_LAST, VAL_ACC_METER, VAL_ACC_HITS, VAL_ACC_ROWS, VAL_ACC_BATCHES, VAL_ACC_STATUS, VAL_ACC_LAST_HITS, VAL_ACC_LAST_ROWS, VAL_ACC_WORDS = 0, 7, 14, 26, 27, 28, 29, 41, 48

# name -> argtypes, exactly the prototypes of include/emage_hip.h
TOOLS_SIGNATURES = {"emage_set_tuning": [_i, _i], "emage_h2_set_trace": [_p]}      # exported by the tools build only
SIGNATURES = {
    "emage_vq_argmin_f32": [_p, _i, _p, _p, _i, _l, _i, _i, _i, _p],
    "emage_argmax_logsoftmax_f32": [_p, _i, _p, _i, _l, _i, _i, _p],
    "emage_gather_rows": [_p, _p, _i, _l, _i, _p, _i, _i, _i, _i, _i, _i, _p],
    "emage_vq_quantize_train_workspace_bytes": [_i],
    "emage_vq_quantize_train": [_p, _i, _p, _p, _p, _i, _p, _i, _i, _i, _p, _p, _f, _p, _l, _i, _i, _i, _p],
    "emage_vq_quantize_backward": [_p, _i, _p, _p, _p, _i, _p, _f, _p, _i, _p, _i, _i, _i, _p],
    "emage_embedding_backward_workspace_bytes": [_i, _i],
    "emage_embedding_backward": [_p, _l, _p, _i, _i, _i, _i, _p, _l, _p, _l, _p],
    "emage_gemm": [_i, _p, _i, _p, _p, _p, _p, _i, _i, _i, _p, _i, _i, _p, _i, _p, _i, _i, _i,
                   _i, _i, _i, _i, _i, _i, _i, _i, _f, _f, _p],
    "emage_gemm_ws": [_i, _p, _i, _p, _p, _p, _p, _i, _i, _i, _p, _i, _i, _p, _i, _p, _i, _i, _i,
                      _i, _i, _i, _i, _i, _i, _i, _i, _f, _f, _p, C.c_size_t, _p],
    "emage_gemm_grouped": [_i, C.POINTER(GemmProblem), _i, _p],
    "emage_gemm_grouped_launches": [_i, C.POINTER(GemmProblem), _i],
    "emage_wav_conv_in": [_i, _p, _l, _i, _i, _l, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _p],
    "emage_audio_resample": [_i, _p, _l, _i, _l, _p, _i, _i, _i, _p, _l, _l, _i, _p],
    "emage_conv_slab": [_i, _p, _i, _p, _p, _p, _p, _i, _p, _i, _i, _i, _i, _i, _i, _f, _f, _p],
    "emage_wav_block0": [_i, _p, _l, _i, _i, _l, _i, _p, _p, _f, _p, _p, _i, _i, _i, _p, _p, _p, _i, _i, _p, _i, _i, _i, _f, _f, _p],
    "emage_attention": [_i, _p, _i, _p, _i, _p, _i, _i, _p, _i, _i, _i, _i, _i, _i, _p],
    "emage_attention_dropout": [_i, _p, _i, _p, _i, _p, _i, _i, _p, _i, _i, _i, _i, _i, _i, _p, _p],
    "emage_qkv_attention": [_i, _p, _i, _p, _p, _p, _p, _f, _p, _i, _i, _i, _i, _i, _f, _f, _p],
    "emage_qkv_attention_grouped": [_i, C.POINTER(QkvAttentionProblem), _i, _i, _i, _i, _p],
    "emage_q_attention": [_i, C.POINTER(QAttentionProblem), _i, _i, _i, _i, _p],
    "emage_q_attention_grouped": [_i, C.POINTER(QAttentionProblem), _i, _i, _i, _i, _i, _p],
    "emage_qm_attention": [_i, C.POINTER(QmAttentionProblem), _i, _i, _i, _i, _p],
    "emage_qm_attention_grouped": [_i, C.POINTER(QmAttentionProblem), _i, _i, _i, _i, _i, _p],
    "emage_bn_stats_workspace_bytes": [_i, _i],
    "emage_bn_stats": [_p, _i, _i, _i, _p, _l, _p, _p, _p, _p, _f, _p],
    "emage_bn_apply": [_p, _i, _p, _p, _p, _p, _p, _i, _p, _p, _p, _p, _f, _f, _p, _i, _i, _i, _p],
    "emage_mse_loss": [_p, _i, _p, _i, _i, _i, _f, _p, _p, _p],
    "emage_nll_loss": [_p, _i, _p, _i, _i, _f, _p, _p, _p],
    "emage_transpose_f32": [_p, _i, _p, _i, _i, _i, _p],
    "emage_col_sum": [_p, _i, _p, _i, _i, _i, _p, _i, _p, _l, _p],
    "emage_col_sum_chunks": [_i],
    "emage_col_sum_finalize_multi": [C.POINTER(FinalizeEntry), _i, _p],
    "emage_act_backward": [_p, _i, _p, _i, _f, _p, _i, _i, _i, _p],
    "emage_layernorm_backward_affine_workspace_bytes": [_i, _i, _i],
    "emage_layernorm_backward_affine": [_p, _i, _p, _p, _i, _f, _p, _i, _p, _p, _i, _i, _i, _i, _p, _l, _p],
    "emage_grad_prep": [_p, _i, _p, _i, _f, _i, _i, _f, _p, _i, _i, _p, _i, _i, _p, _i, _p, _l, _p],
    "emage_layernorm_backward": [_p, _i, _p, _p, _i, _f, _p, _i, _p, _i, _i, _i, _p],
    "emage_attention_backward": [_p, _i, _p, _i, _p, _i, _i, _p, _p, _i, _p, _i, _p, _i, _p, _i, _i, _i, _i, _i, _i, _p],
    "emage_mse_loss_grad": [_p, _i, _p, _i, _i, _i, _f, _p, _i, _p],
    "emage_nll_loss_grad": [_p, _i, _p, _i, _i, _f, _p, _i, _p],
    "emage_im2col_t": [_p, _i, _i, _i, _i, _i, _i, _i, _i, _p, _l, _p],
    "emage_im2col_t_h2": [_p, _i, _i, _i, _i, _i, _i, _i, _i, _p, _l, _p],
    "emage_col2im": [_p, _l, _i, _i, _i, _i, _i, _i, _i, _p, _i, _p],
    "emage_bn_backward": [_p, _i, _p, _p, _p, _f, _p, _i, _p, _i, _p, _p, _i, _i, _p, _l, _p],
    "emage_bn_backward_sums": [_p, _i, _p, _p, _f, _p, _i, _p, _p, _i, _i, _p, _l, _p],
    "emage_bn_backward_apply": [_p, _i, _p, _p, _p, _f, _p, _i, _p, _p, _l, _p, _i, _i, _i, _p],
    "emage_wav_conv_in_backward_workspace_bytes": [_i, _i, _i],
    "emage_wav_conv_in_backward": [_p, _i, _p, _l, _i, _i, _i, _i, _i, _i, _i, _p, _p, _l, _p],
    "emage_count_nonfinite": [_p, _l, _p, _p],
    "emage_count_nonfinite_multi": [C.POINTER(_p), C.POINTER(_l), _i, _p, _p],
    "emage_adam_step_dev": [_p, _p, _p, _p, _l, _p, _f, _f, _f, _f, _f, _p],
    "emage_adam_step": [_p, _p, _p, _p, _l, _i, _f, _f, _f, _f, _f, _p],
    "emage_adam_multi_chunk": [],
    "emage_adam_multi": [_p, _p, _p, _i, _p, _i, _f, _f, _f, _f, _f, _f, _i, _p, _p],
    "emage_adam_multi_scaled": [_p, _p, _p, _i, _p, _i, _f, _f, _f, _f, _f, _f, _p, _i, _p, _p],
    "emage_grad_norm_workspace_bytes": [_i, _i],
    "emage_grad_sumsq_multi": [_p, _p, _p, _i, _i, _d, _d, _p, _p, _p, _p, _p, _l, _p],
    "emage_scale_multi": [_p, _p, _p, _i, _p, _p],
    "emage_dropout_mask": [_p, _l, _f, C.c_ulonglong, C.c_uint, _p, _i, _p],
    "emage_gather_clips": [_p, _l, _p, _i, _i, _p, _l, _i, _i, _p, _p, _p, _p, _l, _i, _p, _l, _p, _l, _p, _l, _l, _p, _l, _l, _p, _l, _l, _p, _l, _l, _p, _p],
    "emage_motion_mask": [_p, _l, _d, _d, C.c_ulonglong, C.c_uint, _p, _p],
    "emage_gather_clip_speakers": [_p, _l, _p, _i, _i, _p, _l, _p, _l, _p, _p, _p],
    "emage_gather_windows": [_i, _p, _l, _p, _i, _i, _p, _l, _p, _p],
    "emage_copy_segments": [_p, _l, _p, _l, _p, _i, _l, _l, _p, _p],
    "emage_stream_push": [_i, _p, _l, _p, _i, _p, _l, _p, _p],
    "emage_stream_push_resample": [_p, _l, _p, _i, _p, _i, _p, _l, _p, _l, _p, _i, _p, _p],
    "emage_stream_push_hints": [_p, _l, _p, _i, _p, _p, _i, _i, _p, _p, _i, _p, _p],
    "emage_stream_windows": [_p, _l, _p, _i, _i, _p, _l, _p, _p],
    "emage_stream_commit": [_p, _i, _i, _p, _i, _i, _p, _i, _p, _i, _p, _l, _p, _i, _p, _p],
    "emage_stream_emit": [_p, _i, _i, _i, _p, _p, _p, _i, _i, _f, _p, _i, _p, _p, _p, _p, _p, _p, _p],
    "emage_val_metrics_workspace_bytes": [_i, _i],
    "emage_val_metrics": [C.POINTER(ValEntry), _i, _i, _i, _p, _p, _p, _l, _p],
    "emage_mul_add": [_p, _i, _p, _i, _i, _p, _i, _p, _i, _i, _i, _p],
    "emage_mul_add_philox": [_p, _i, _f, C.c_ulonglong, C.c_uint, _p, _i, _i, _p, _i, _p, _i, _i, _i, _p],
    "emage_layernorm": [_i, _p, _i, _p, _p, _f, _p, _i, _p, _p, _i, _i, _i, _p],
    "emage_add": [_i, _p, _i, _p, _i, _i, _p, _i, _i, _i, _p, _p, _i, _i, _i, _p],
    "emage_pack_motion": [_i, _p, _p, _l, _p, _p, _l, _i, _p, _i, _i, _i, _i, _i, _p],
    "emage_pack_motion_hints": [_i, _p, _p, _l, _i, _p, _p, _p, _l, _i, _p, _i, _i, _i, _i, _i, _p, _p],
    "emage_cast_pad": [_i, _p, _i, _p, _i, _i, _i, _i, _p],
    "emage_h2_cast": [_p, _i, _p, _i, _i, _i, _i, _f, _i, _p],
    "emage_f16x3_pack_weights": [_p, _i, _p, _i, _i, _i, _f, _p],
    "emage_rot6d_to_axis_angle": [_p, _p, _i, _p],
    "emage_axis_angle_to_rot6d": [_p, _p, _i, _p],
    "emage_merge_parts": [_p, _i, _p, _i, _p, _i, _p, _i, _p, _p, _p, _i, _p],
    "emage_velocity_to_position": [_p, _i, _i, _p, _i, _f, _p, _i, _i, _p],
    "emage_lstm_step": [_i, _p, _i, _p, _f, _f, _p, _i, _p, _i, _p, _i, _i, _i, _p],
    "emage_lstm_step_pair": [_i, _p, _p, _i, _i, _p, _p, _f, _f, _f, _p, _p, _i, _p, _p, _i, _p, _p, _i, _i, _i, _p],
    "emage_lstm_layer_sync_words": [_i, _i],
    "emage_lstm_layer_health": [_p, _i, _p, _p],
    "emage_lstm_layer": [_i, _p, _l, _i, _p, _p, _f, _f, _f, _p, _l, _i, _i, _i, _i, _p, _i, _p],
    "emage_lstm_layer_lengths": [_i, _p, _l, _i, _p, _p, _f, _f, _f, _p, _l, _i, _i, _i, _i, _p, _p, _i, _p],
    "emage_softmax2_mix": [_p, _i, _p, _i, _p, _i, _p, _i, _i, _i, _p],
    "emage_lstm_inputs": [_p, _p, _i, _p, _l, _i, _i, _p, _p, _i, _i, _i, _i, _p],
    "emage_rot6d_scatter": [_p, _i, _p, _p, _i, _i, _p],
    "emage_motion_rep": [_p, _p, _l, _f, _p, _i, _i, _p],
}
RESTYPES = {"emage_bn_stats_workspace_bytes": _l, "emage_vq_quantize_train_workspace_bytes": _l, "emage_wav_conv_in_backward_workspace_bytes": _l, "emage_layernorm_backward_affine_workspace_bytes": _l,
            "emage_grad_norm_workspace_bytes": _l, "emage_val_metrics_workspace_bytes": _l, "emage_embedding_backward_workspace_bytes": _l}

_lib = None
_tools = None
_use_tools = False


def _open(path, signatures):
    if not os.path.exists(path):
        raise ImportError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(hipcc --offload-arch=gfx950). The EMAGE path has no CPU fallback.")
    lib = C.CDLL(path)
    lib.emage_abi_version.restype = _i
    lib.emage_target_arch.restype = C.c_char_p
    if lib.emage_abi_version() != ABI_VERSION:
        raise ImportError(f"{os.path.basename(path)} ABI {lib.emage_abi_version()} != expected {ABI_VERSION}; rebuild")
    for name, args in signatures.items():
        fn = getattr(lib, name)   # AttributeError if the symbol is missing
        fn.argtypes = args
        fn.restype = RESTYPES.get(name, _i)
    return lib


def load():
    """The shared library every op launches into (loaded once, every entry point typed): the product library, or — after
    `use_tools()` — its tools twin."""
    global _lib, _tools
    if _use_tools:
        if _tools is None:
            _tools = _open(TOOLS_LIB_PATH, {**SIGNATURES, **TOOLS_SIGNATURES})
        return _tools
    if _lib is None:
        _lib = _open(LIB_PATH, SIGNATURES)
    return _lib


def use_tools(on: bool = True):
    """tools/ and the tile-configuration tests: route every launch of this process through libemage_hip_tools.so (all tile
    configurations, `emage_set_tuning`, ablation branches, phase tracer).  The product path never calls this."""
    global _use_tools
    _use_tools = bool(on)
    return load()


class EmageKernelError(RuntimeError):
    pass


def nonfinite_error(count, precision, where):
    """What every runner raises when its health counter came back non-zero: `count` non-finite values `where` ("among the network outputs
    of a tick", "in the generated motion"), computed in `precision`."""
    return FloatingPointError(f"{int(count)} non-finite values {where} (precision {precision!r}): in f16x3 an activation beyond |x| < 4094 overflows "
                              "the fp16 planes — run this checkpoint with set_precision('fp32')")


def check(code: int, what: str):
    if code != 0:
        kind = "unsupported argument (EMAGE_EINVAL)" if code < 0 else f"hipError {code}"
        raise EmageKernelError(f"{what}: {kind}")
