"""ctypes binding of libixtts_hip.so (the C ABI in include/ixtts_hip.h).

There is NO fallback: if the library is missing or fails to load, `lib()` raises.  The
product path never routes through oracle/ or any CPU implementation.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("IXTTS_LIB") or os.path.join(HERE, "libixtts_hip.so")  # IXTTS_LIB: developer builds (trace)

MAX_STAGES = 8
MAX_RESK = 4
BIGVGAN_TILE_SLOTS = 6  # IXTTS_BIGVGAN_TILE_SLOTS


class BigVGANCfg(C.Structure):
    _fields_ = [
        ("num_mels", C.c_int), ("upsample_initial_channel", C.c_int), ("n_stages", C.c_int),
        ("upsample_rates", C.c_int * MAX_STAGES), ("upsample_kernel_sizes", C.c_int * MAX_STAGES),
        ("n_resblock_kernels", C.c_int), ("resblock_kernel_sizes", C.c_int * MAX_RESK),
        ("resblock_dilations", (C.c_int * 3) * MAX_RESK), ("max_frames", C.c_int), ("fast_sin", C.c_int),
    ]


class GptCfg(C.Structure):
    _fields_ = [
        ("model_dim", C.c_int), ("layers", C.c_int), ("heads", C.c_int), ("n_mel_codes", C.c_int),
        ("n_mel_pos", C.c_int), ("n_text_tokens", C.c_int), ("n_text_pos", C.c_int),
        ("start_mel_token", C.c_int), ("stop_mel_token", C.c_int), ("max_seq", C.c_int),
        ("max_batch", C.c_int), ("weight_dtype", C.c_int),
    ]


class SamplerCfg(C.Structure):
    _fields_ = [
        ("repetition_penalty", C.c_float), ("temperature", C.c_float), ("top_k", C.c_int),
        ("top_p", C.c_float), ("do_sample", C.c_int), ("suppress_stop", C.c_int), ("seed", C.c_uint64),
        ("typical_mass", C.c_float), ("length_penalty", C.c_float),
        ("min_new_tokens", C.c_int), ("no_repeat_ngram_size", C.c_int), ("min_p", C.c_float),
        ("exp_decay_start", C.c_int), ("exp_decay_factor", C.c_double), ("epsilon_cutoff", C.c_float), ("eta_cutoff", C.c_float),
        ("renormalize_logits", C.c_int), ("forced_eos_step", C.c_int), ("n_seq_bias", C.c_int),  # n_seq_bias: the engine fills it in
    ]


NGRAM_MAX = 8  # IXTTS_NGRAM_MAX
SEQ_BIAS_MAX = 64  # IXTTS_SEQ_BIAS_MAX
SEQ_BIAS_LEN = 8  # IXTTS_SEQ_BIAS_LEN

QWEN_TOPK_MAX = 64  # IXTTS_QWEN_TOPK_MAX
QWEN_MAX_EOS = 8
QWEN_MAX_SLOTS = 4  # IXTTS_QWEN_MAX_SLOTS

RESAMPLE_TILE = 1024  # IXTTS_RESAMPLE_TILE: output samples per workgroup of the resampler (`resample_tile()` asks the library)
PCM_ENCODINGS = {"pcm_s16le": 0, "mulaw": 1, "alaw": 2}  # IXTTS_PCM_*
LOUDNESS_REQ_COLS = 6  # IXTTS_LOUDNESS_REQ_COLS: (first row, rows, start, extent, hop, first hop slot)
LOUDNESS_COEF_COLS = 24  # IXTTS_LOUDNESS_COEF_COLS: shelf b0 b1 b2 a1 a2, high-pass a1 a2, one unused, the chunk transition 4 x 4
LOUDNESS_MAX_HOP = 4800  # IXTTS_LOUDNESS_MAX_HOP
LOUDNESS_CEILING_BOUND, LOUDNESS_NO_BLOCK = 1, 2  # flags of a record
LOUDNESS_RECORD_BYTES = 24  # ixtts_loudness_record: f64 lufs, f32 gain, f32 peak, u32 flags, u32 blocks
TRUE_PEAK_TAPS = 49  # IXTTS_TRUE_PEAK_TAPS
LIMITER_TILE = 1024  # IXTTS_LIMITER_TILE: output samples per workgroup of the limiter (`limiter_tile()` asks the library)
LIMITER_MAX_W = 240  # IXTTS_LIMITER_MAX_W: the look-around at 48 kHz
LIMITER_REQ_COLS = 10  # IXTTS_LIMITER_REQ_COLS: (first row, rows, start, extent, out offset, gain index, W, window offset, mode, first partial slot)


class QwenCfg(C.Structure):
    _fields_ = [
        ("hidden_size", C.c_int), ("layers", C.c_int), ("heads", C.c_int), ("kv_heads", C.c_int), ("head_dim", C.c_int),
        ("intermediate_size", C.c_int), ("vocab_size", C.c_int), ("rms_norm_eps", C.c_float), ("rope_theta", C.c_float),
        ("tie_word_embeddings", C.c_int), ("max_seq", C.c_int), ("weight_dtype", C.c_int), ("n_eos", C.c_int),
        ("eos_ids", C.c_int * QWEN_MAX_EOS),
    ]


class QwenSampling(C.Structure):
    _fields_ = [("do_sample", C.c_int), ("temperature", C.c_float), ("top_k", C.c_int), ("top_p", C.c_float), ("seed", C.c_uint64)]


# every symbol include/ixtts_hip.h declares: name -> (restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    "ixtts_version": (C.c_char_p, []),
    "ixtts_last_error": (C.c_char_p, []),
    "ixtts_aa_snake_f32": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P]),
    "ixtts_attn_full_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "ixtts_attn_full_f32": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_long, C.c_long, C.c_long, C.c_long, C.c_long,
                                      C.c_long, C.c_float, _P, C.c_size_t, _P]),
    "ixtts_attn_full_varlen_workspace_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "ixtts_attn_full_varlen_f32": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_long, C.c_long, C.c_long, C.c_long,
                                             C.c_float, _P, C.c_size_t, _P]),
    "ixtts_attn_full_rope_f32": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_long, C.c_long, C.c_long, C.c_long,
                                           C.c_long, C.c_long, C.c_float, _P, C.c_size_t, _P]),
    "ixtts_attn_full_rope_varlen_f32": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_long, C.c_long, C.c_long,
                                                  C.c_long, C.c_float, _P, C.c_size_t, _P]),
    "ixtts_adaln_rmsnorm_f32": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_float, _P]),
    "ixtts_ln_modulate_f32": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_float, _P]),
    "ixtts_rope_qk_f32": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "ixtts_swiglu_f32": (C.c_int, [_P, _P, C.c_long, C.c_int, _P]),
    "ixtts_wn_gate_f32": (C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_long, C.c_int, _P]),
    "ixtts_wn_gate_rows_f32": (C.c_int, [_P, _P, _P, C.c_long, C.c_int, C.c_long, C.c_int, C.c_long, C.c_int, _P]),
    "ixtts_reflect_halo_rows_f32": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "ixtts_adaln_rmsnorm_varlen_f32": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_long, C.c_int, C.c_float, _P]),
    "ixtts_ln_modulate_varlen_f32": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_long, C.c_int, C.c_float, _P]),
    "ixtts_rope_qk_varlen_f32": (C.c_int, [_P, _P, _P, C.c_int, C.c_long, C.c_int, C.c_int, _P]),
    "ixtts_wn_gate_rows_varlen_f32": (C.c_int, [_P, _P, _P, C.c_long, C.c_int, _P, C.c_int, C.c_long, C.c_int, _P]),
    "ixtts_reflect_halo_rows_varlen_f32": (C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "ixtts_adaln_rmsnorm_planes_f32": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_float, _P]),
    "ixtts_adaln_rmsnorm_planes_varlen_f32": (C.c_int, [_P, _P, _P, _P, _P, C.c_int, C.c_long, C.c_int, C.c_float, _P]),
    "ixtts_gemm_x6_split_halo": (C.c_int, [_P, C.c_long, _P, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "ixtts_gemm_x6_split_halo_varlen": (C.c_int, [_P, C.c_long, _P, C.c_long, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P]),
    "ixtts_gemm_x6_packed_bytes": (C.c_size_t, [C.c_int, C.c_int]),
    "ixtts_gemm_x6_pack": (C.c_int, [_P, _P, C.c_int, C.c_int, _P]),
    "ixtts_gemm_x6_rows_padded": (C.c_long, [C.c_long]),
    "ixtts_gemm_x6_split": (C.c_int, [_P, C.c_long, _P, C.c_long, C.c_int, _P]),
    "ixtts_gemm_x6_f32": (C.c_int, [_P, C.c_long, C.c_long, _P, _P, _P, C.c_long, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "ixtts_gemm_x6_pair_f32": (C.c_int, [_P, C.c_long, C.c_long, C.c_int, _P, _P, _P, C.c_long, C.c_long, C.c_int, _P, C.c_long, C.c_int, C.c_int,
                                         C.c_int, C.c_int, C.c_int, _P]),
    "ixtts_gemm_x6_pair_gate_varlen_f32": (C.c_int, [_P, C.c_long, C.c_long, C.c_int, _P, _P, _P, C.c_long, _P, C.c_int, _P, C.c_long, C.c_int, C.c_int,
                                                     C.c_int, C.c_int, _P]),
    "ixtts_bigvgan_create": (C.c_int, [C.POINTER(_P), C.POINTER(BigVGANCfg)]),
    "ixtts_bigvgan_set_tensor": (C.c_int, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), C.c_int]),
    "ixtts_bigvgan_finalize": (C.c_int, [_P]),
    "ixtts_bigvgan_arena": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    "ixtts_bigvgan_adopt_arena": (C.c_int, [_P]),
    "ixtts_bigvgan_forward": (C.c_int, [_P, _P, C.c_int, C.c_int, _P, _P]),
    "ixtts_bigvgan_forward_varlen": (C.c_int, [_P, _P, _P, _P, C.c_int, C.c_int, _P, _P]),
    "ixtts_bigvgan_tile_launches": (C.c_int, [_P, C.POINTER(C.c_int64), C.POINTER(C.c_int)]),
    "ixtts_bigvgan_flops": (C.c_double, [_P, C.c_int, C.c_int]),
    "ixtts_bigvgan_destroy": (C.c_int, [_P]),
    "ixtts_gpt_create": (C.c_int, [C.POINTER(_P), C.POINTER(GptCfg)]),
    "ixtts_gpt_set_tensor": (C.c_int, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), C.c_int]),
    "ixtts_gpt_finalize": (C.c_int, [_P]),
    "ixtts_gpt_arena": (C.c_int, [_P, C.POINTER(_P), C.POINTER(C.c_size_t)]),
    "ixtts_gpt_adopt_arena": (C.c_int, [_P]),
    "ixtts_gpt_share_arena": (C.c_int, [_P, _P]),
    "ixtts_gpt_prefill": (C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, _P]),
    "ixtts_gpt_prefill_many": (C.c_int, [_P, C.c_int, C.POINTER(C.c_int), C.POINTER(_P), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, _P]),
    "ixtts_gpt_prefill_plan": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "ixtts_gpt_decode": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(SamplerCfg), _P]),
    "ixtts_gpt_decode_slots": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(SamplerCfg), C.POINTER(C.c_uint32), _P]),
    "ixtts_gpt_read": (C.c_int, [_P, C.c_int, _P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), _P]),
    "ixtts_gpt_read_logits": (C.c_int, [_P, C.c_int, _P, _P]),
    "ixtts_gpt_beam_begin": (C.c_int, [_P, C.c_int, _P]),
    "ixtts_gpt_beam_decode": (C.c_int, [_P, C.c_int, C.POINTER(SamplerCfg), _P]),
    "ixtts_gpt_beam_read": (C.c_int, [_P, C.c_int, _P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float), _P, _P, _P, _P]),
    "ixtts_gpt_beam_force": (C.c_int, [_P, _P, C.c_int, _P]),
    "ixtts_gpt_beam_begin_group": (C.c_int, [_P, C.c_int, C.c_int, C.c_uint64, _P]),
    "ixtts_gpt_beam_park_group": (C.c_int, [_P, C.c_int, _P]),
    "ixtts_gpt_beam_decode_groups": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(SamplerCfg), _P]),
    "ixtts_gpt_beam_decode_groups_cfg": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(SamplerCfg), _P]),
    "ixtts_gpt_beam_read_group":(C.c_int, [_P, C.c_int, C.c_int, _P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float), _P, _P, _P, _P]),
    "ixtts_gpt_beam_force_group": (C.c_int, [_P, C.c_int, _P, C.c_int, _P]),
    "ixtts_gpt_read_probs": (C.c_int, [_P, C.c_int, _P, _P]),
    "ixtts_gpt_force_next": (C.c_int, [_P, C.c_int, C.c_int32, _P]),
    "ixtts_gpt_set_bans": (C.c_int, [_P, C.c_int, _P, C.c_int, _P, C.c_int, _P]),
    "ixtts_gpt_set_sequence_bias": (C.c_int, [_P, C.c_int, _P, _P, _P, C.c_int, _P]),
    "ixtts_gpt_set_forced_eos": (C.c_int, [_P, C.c_int, _P, C.c_int, _P]),
    "ixtts_gpt_latent": (C.c_int, [_P, _P, C.c_int, _P, C.c_int, _P, _P]),
    "ixtts_gpt_latent_many": (C.c_int, [_P, C.c_int, C.POINTER(_P), C.POINTER(C.c_int), C.POINTER(_P), C.POINTER(C.c_int), C.POINTER(_P), C.c_int, _P]),
    "ixtts_gpt_latent_plan": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int)]),
    "ixtts_gpt_bench_gemv": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, _P]),
    "ixtts_gpt_step_bytes": (C.c_double, [_P, C.c_int, C.c_int]),
    "ixtts_gpt_max_batch": (C.c_int, []),
    "ixtts_gpt_max_batch_for": (C.c_int, [C.c_int]),
    "ixtts_gpt_destroy": (C.c_int, [_P]),
    "ixtts_qwen_create": (C.c_int, [C.POINTER(_P), C.POINTER(QwenCfg)]),
    "ixtts_qwen_set_tensor": (C.c_int, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), C.c_int]),
    "ixtts_qwen_finalize": (C.c_int, [_P]),
    "ixtts_qwen_prefill": (C.c_int, [_P, _P, C.c_int, _P]),
    "ixtts_qwen_step": (C.c_int, [_P, C.c_int, C.POINTER(QwenSampling), _P]),
    "ixtts_qwen_read": (C.c_int, [_P, _P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), _P]),
    "ixtts_qwen_generate": (C.c_int, [_P, C.c_int, C.POINTER(QwenSampling), _P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), _P]),
    "ixtts_qwen_read_logits": (C.c_int, [_P, _P, _P]),
    "ixtts_qwen_read_kept": (C.c_int, [_P, _P, _P, C.c_int, C.POINTER(C.c_int), _P]),
    "ixtts_qwen_draw": (C.c_int, [_P, C.c_uint64, C.c_int, _P, _P]),
    "ixtts_qwen_step_bytes": (C.c_double, [_P, C.c_int]),
    "ixtts_qwen_create_slots": (C.c_int, [C.POINTER(_P), C.POINTER(QwenCfg), C.c_int]),
    "ixtts_qwen_prefill_slots": (C.c_int, [_P, C.c_int, _P, _P, _P]),
    "ixtts_qwen_step_slots": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(QwenSampling), _P]),
    "ixtts_qwen_generate_slots": (C.c_int, [_P, C.c_int, C.c_int, C.POINTER(QwenSampling), _P]),
    "ixtts_qwen_read_slot": (C.c_int, [_P, C.c_int, _P, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), _P]),
    "ixtts_qwen_read_logits_slot": (C.c_int, [_P, C.c_int, _P, _P]),
    "ixtts_qwen_read_kept_slot": (C.c_int, [_P, C.c_int, _P, _P, C.c_int, C.POINTER(C.c_int), _P]),
    "ixtts_qwen_destroy": (C.c_int, [_P]),
    "ixtts_resample_tile": (C.c_int, []),
    "ixtts_resample_varlen_f32": (C.c_int, [_P, C.c_long, _P, C.c_long, _P, C.c_int, C.c_long, _P, C.c_long, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    "ixtts_pcm_assemble": (C.c_int, [_P, C.c_long, _P, C.c_long, _P, C.c_int, C.c_int, _P]),
    "ixtts_loudness_measure": (C.c_int, [_P, C.c_long, _P, C.c_int, _P, _P, C.c_int, C.c_long, _P, _P, C.c_long, _P]),
    "ixtts_loudness_gain": (C.c_int, [_P, _P, C.c_long, _P, _P, C.c_int, _P, _P, _P]),
    "ixtts_pcm_assemble_gain": (C.c_int, [_P, C.c_long, _P, C.c_long, _P, C.c_int, _P, C.c_int, C.c_int, _P]),
    "ixtts_limiter_tile": (C.c_int, []),
    "ixtts_true_peak": (C.c_int, [_P, C.c_long, _P, C.c_int, _P, _P, C.c_int, C.c_long, _P, _P, C.c_long, _P]),
    "ixtts_limiter": (C.c_int, [_P, C.c_long, _P, C.c_int, _P, _P, C.c_int, C.c_long, _P, C.c_long, _P, C.c_int, _P, C.c_long, _P, C.c_long, _P]),
}

_lib = None


class IxttsError(RuntimeError):
    pass


def lib():
    """Load libixtts_hip.so and bind every declared symbol; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    # torch first: its bundled HIP runtime must be the one this process initialises.  Loading libixtts_hip.so before torch
    # pulls in /opt/rocm's libamdhip64 as a second runtime, and device memory calls through it then fail with
    # "no ROCm-capable device is detected" (seen when build() ran before smoke() in one process).
    import torch  # noqa: F401

    if not os.path.exists(LIB_PATH):
        raise IxttsError(
            f"{LIB_PATH} not found: build it with `python -m voice_tts_amd.build` "
            "(there is no CPU fallback for the HIP path)")
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(L, name)  # AttributeError if the .so lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def check(rc, what=""):
    if rc != 0:
        msg = lib().ixtts_last_error().decode(errors="replace")
        raise IxttsError(f"{what} failed with code {rc}: {msg}")


def max_batch():
    """Decode slots an engine of ANY weight type can step together (a build constant of libixtts_hip.so): 16."""
    return int(lib().ixtts_gpt_max_batch())


_DTYPE_CODES = {"f32": 0, "bf16": 1, "f16": 2}  # IXTTS_DTYPE_*


def max_batch_for(dtype):
    """Decode slots an engine of weight type `dtype` ("f32" | "bf16" | "f16", or the IXTTS_DTYPE_* code) can step together:
    32 for the 16-bit types, 16 for fp32."""
    if isinstance(dtype, str):
        if dtype not in _DTYPE_CODES:
            raise ValueError(f"max_batch_for: unknown weight type {dtype!r}")
        dtype = _DTYPE_CODES[dtype]
    return int(lib().ixtts_gpt_max_batch_for(int(dtype)))


def resample_tile():
    """Output samples one workgroup of the resampler produces (a build constant of libixtts_hip.so)."""
    return int(lib().ixtts_resample_tile())


def limiter_tile():
    """Output samples one workgroup of the limiter produces (a build constant of libixtts_hip.so)."""
    return int(lib().ixtts_limiter_tile())


def current_stream_ptr():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
