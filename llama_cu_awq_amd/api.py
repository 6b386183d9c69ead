"""ctypes mirror of include/llama2_q4.h (same names / argument meaning as the reference's host functions).

Fails loudly when libllama2_q4.so is missing -- there is no CPU or PyTorch fallback on this path.
Device buffers are plain HIP allocations owned by `DevBuf`; arrays cross the boundary as numpy.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libllama2_q4.so")
# the -DQ4_PROFILING build of the same sources (ablations, launch-skip mask, tuning setters): tools/ and
# tests/prof_cases.py select it with Q4_PROFILING_BUILD=1 or use_profiling_build() before the first lib() call
PROF_LIB_PATH = os.path.join(_HERE, "libllama2_q4_prof.so")

MAX_SEQ_LEN = 128 * 1024
KV_FP16, KV_FP8 = 0, 1          # q4_set_kv_format
KV_FORMATS = {"fp16": KV_FP16, "fp8": KV_FP8}
MAX_TOP_LOGPROBS = 20           # Q4_MAX_TOP_LOGPROBS
MAX_PENALTY_WINDOW = 1024       # Q4_MAX_PENALTY_WINDOW
MAX_LOGIT_BIAS = 256            # Q4_MAX_LOGIT_BIAS
ROPE_NONE, ROPE_LINEAR, ROPE_LLAMA3, ROPE_CUSTOM, ROPE_MAX_PAIRS = 0, 1, 2, 3, 256   # Q4_ROPE_*
ROPE_KINDS = {"none": ROPE_NONE, "default": ROPE_NONE, "linear": ROPE_LINEAR, "llama3": ROPE_LLAMA3, "custom": ROPE_CUSTOM}
GUIDE_MAX_STATES, GUIDE_DEAD, GUIDE_NONE, GUIDE_OFFTRACK = 4096, 0xFFFF, -1, -2   # Q4_GUIDE_*


class Config(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("dim", "hidden_dim", "n_layers", "n_heads", "n_kv_heads", "vocab_size", "seq_len")] + [
        ("rope_theta", C.c_float)]


class QWeight(C.Structure):
    _fields_ = [("weight", C.c_void_p), ("zeros", C.c_void_p), ("scales", C.c_void_p)]


class PerLayerWeight(C.Structure):
    _fields_ = [("rms_att_weight", C.c_void_p), ("rms_ffn_weight", C.c_void_p)] + [
        (n, QWeight) for n in ("wq_q", "wq_k", "wq_v", "wq_o", "wq_gate", "wq_up", "wq_down")]


class TransformerWeights(C.Structure):
    _fields_ = [("token_embedding_table", C.c_void_p), ("wcls", C.c_void_p), ("rms_final_weight", C.c_void_p),
                ("layers", C.POINTER(PerLayerWeight)), ("num_layers", C.c_int)]


class RunState(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("x", "xb", "hb", "q", "att", "logits", "key_cache", "value_cache", "pos",
                                          "shared_data", "logits_array")]


class CliArgs(C.Structure):
    _fields_ = [("checkpoint_path", C.c_char_p), ("tokenizer_path", C.c_char_p), ("dataset_path", C.c_char_p),
                ("steps", C.c_int), ("prompt", C.c_char_p), ("perplexity", C.c_int), ("temperature", C.c_float),
                ("topp", C.c_float), ("rng_seed", C.c_ulonglong), ("mode", C.c_char_p), ("system_prompt", C.c_char_p),
                ("seed_from_time", C.c_int)]


class SnapshotInfo(C.Structure):
    """struct q4_snapshot_info"""
    _fields_ = [("n_pos", C.c_int), ("kv_format", C.c_int), ("n_layers", C.c_int), ("n_kv_heads", C.c_int), ("head_size", C.c_int),
                ("rope_theta", C.c_float), ("fingerprint", C.c_ulonglong), ("device_bytes", C.c_ulonglong), ("export_bytes", C.c_ulonglong)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class RopeScaling(C.Structure):
    """q4_rope_scaling; the default is kind NONE"""
    _fields_ = [("kind", C.c_int), ("factor", C.c_float), ("low_freq_factor", C.c_float), ("high_freq_factor", C.c_float),
                ("original_max_position", C.c_int), ("n_freqs", C.c_int), ("inv_freq", C.POINTER(C.c_float))]

    def as_dict(self):
        """the setting in Hugging Face's spelling (custom: with a copy of the frequencies); None for kind NONE"""
        if self.kind == ROPE_LINEAR:
            return {"rope_type": "linear", "factor": self.factor}
        if self.kind == ROPE_LLAMA3:
            return {"rope_type": "llama3", "factor": self.factor, "low_freq_factor": self.low_freq_factor, "high_freq_factor": self.high_freq_factor,
                    "original_max_position_embeddings": self.original_max_position}
        if self.kind == ROPE_CUSTOM:
            return {"kind": "custom", "inv_freq": np.array(self.inv_freq[:self.n_freqs], dtype=np.float32)}
        return None


def rope_scaling_struct(scaling):
    """None, the text form ("linear,factor=4", "llama3,factor=8,low=1,high=4,orig=8192", "none"), a dict in Hugging Face's rope_scaling spelling
    (rope_type or type, factor, low_freq_factor, high_freq_factor, original_max_position_embeddings), dict(kind="custom", inv_freq=array) or a
    RopeScaling -> (RopeScaling, the array it points into or None: keep it alive as long as the struct). Checked by the library, not here."""
    if scaling is None:
        return RopeScaling(), None
    if isinstance(scaling, RopeScaling):
        return scaling, None
    if isinstance(scaling, str):
        r = RopeScaling()
        if lib().q4_parse_rope_scaling(scaling.encode(), C.byref(r)):
            raise ValueError("rope_scaling: cannot use %r (none | linear,factor=F | llama3,factor=F,low=L,high=H,orig=N)" % (scaling,))
        return r, None
    if not isinstance(scaling, dict):
        raise ValueError("rope_scaling: None, a text, a dict or a RopeScaling, not %r" % (scaling,))
    kind = scaling.get("kind", scaling.get("rope_type", scaling.get("type")))
    if kind not in ROPE_KINDS:
        raise ValueError("rope_scaling: kind %r is not supported (linear, llama3, custom; yarn, longrope and dynamic are not)" % (kind,))
    r = RopeScaling(kind=ROPE_KINDS[kind])
    keep = None
    if r.kind in (ROPE_LINEAR, ROPE_LLAMA3):
        r.factor = float(scaling["factor"])
    if r.kind == ROPE_LLAMA3:
        r.low_freq_factor = float(scaling["low_freq_factor"])
        r.high_freq_factor = float(scaling["high_freq_factor"])
        r.original_max_position = int(scaling["original_max_position_embeddings"])
    if r.kind == ROPE_CUSTOM:
        keep = np.ascontiguousarray(scaling["inv_freq"], dtype=np.float32).reshape(-1)
        r.n_freqs = keep.shape[0]
        r.inv_freq = keep.ctypes.data_as(C.POINTER(C.c_float))
    return r, keep


def rope_inv_freq(scaling, head_size, theta):
    """q4_rope_inv_freq (host only): the head_size/2 float32 frequencies a model of this head size and rope_theta gets under `scaling` (any form
    Transformer(rope_scaling=...) accepts; None: the unscaled pow(theta, -2i/head_size), rounded to float)."""
    r, keep = rope_scaling_struct(scaling)
    out = np.empty(max(int(head_size) // 2, 1), dtype=np.float32)
    check(lib().q4_rope_inv_freq(C.byref(r), int(head_size), float(theta), out.ctypes.data))
    return out


def RoPERotationFreqs(q, k, num_heads, num_kv_heads, head_size, pPos, loff, inv_freq):
    """q4_rope_rotation_freqs over DevBufs: RoPERotation with the angle pos * inv_freq[i] (inv_freq: head_size/2 float32 on the device)"""
    check(lib().q4_rope_rotation_freqs(q.ptr, k.ptr, num_heads, num_kv_heads, head_size, pPos.ptr, loff, inv_freq.ptr))


class SamplingControls(C.Structure):
    """q4_sampling_controls; the defaults are the neutral values (everything off)"""
    _fields_ = [("top_k", C.c_int), ("min_p", C.c_float), ("repeat_penalty", C.c_float), ("presence_penalty", C.c_float),
                ("frequency_penalty", C.c_float), ("penalty_last_n", C.c_int)]

    def __init__(self, top_k=0, min_p=0.0, repeat_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, penalty_last_n=64):
        super().__init__(int(top_k), float(min_p), float(repeat_penalty), float(presence_penalty), float(frequency_penalty), int(penalty_last_n))

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


MAX_DRY_WINDOW = 4096
DRY_MAX_MATCH = 64
DRY_BREAKER_STRINGS = ("\n", ":", "\"", "*")


class DryControls(C.Structure):
    """q4_dry_controls; the defaults are off (multiplier 0, no n-gram ban)"""
    _fields_ = [("multiplier", C.c_float), ("base", C.c_float), ("allowed_length", C.c_int), ("last_n", C.c_int), ("no_repeat_ngram_size", C.c_int)]

    def __init__(self, multiplier=0.0, base=1.75, allowed_length=2, last_n=1024, no_repeat_ngram_size=0):
        super().__init__(float(multiplier), float(base), int(allowed_length), int(last_n), int(no_repeat_ngram_size))

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


ADAPTIVE_RECORD = 8
ADAPTIVE_RECORD_FIELDS = ("T_s", "H", "d_star", "mu", "T_m", "kept", "lse", "lse_t")


class AdaptiveControls(C.Structure):
    """q4_adaptive_controls; the defaults are off (typical_p 1, top_n_sigma 0, mirostat_tau 0)"""
    _fields_ = [("typical_p", C.c_float), ("top_n_sigma", C.c_float), ("mirostat_tau", C.c_float), ("mirostat_eta", C.c_float)]

    def __init__(self, typical_p=1.0, top_n_sigma=0.0, mirostat_tau=0.0, mirostat_eta=0.1):
        super().__init__(float(typical_p), float(top_n_sigma), float(mirostat_tau), float(mirostat_eta))

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


NOT_ADMITTED = 6                # q4_verify_tokens: nothing ran
SPEC_MAX_DRAFT = 7
# q4_drafter_fn: (ctx, tokens, n_tokens, max_draft, draft_out) -> number of ids written
DRAFTER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int))


# every symbol include/llama2_q4.h declares (tests/test_abi.py checks the .so exports all of them)
SYMBOLS = [
    "q4_status_string", "q4_last_error", "q4_set_device", "q4_stream_create", "q4_stream_create_masked", "q4_stream_destroy", "q4_set_stream",
    "q4_get_stream", "q4_stream_synchronize", "q4_device_synchronize", "q4_malloc", "q4_free", "q4_memcpy_h2d",
    "q4_memcpy_d2h", "q4_memset", "q4_rmsnorm", "q4_matmul_f16", "q4_matmul_q4", "q4_qkv_matvec", "q4_ffn_matvec_silu",
    "q4_rope_rotation", "q4_multi_head_attention", "q4_multi_head_attention_kv8", "q4_copy_embedding", "q4_convert_fp16_to_fp32", "q4_argmax",
    "q4_run_llama_network", "q4_run_transformer", "q4_run_transformer_at", "q4_wait_pos", "q4_steps_that_fit", "q4_run_transformer_steps", "q4_set_fusion", "q4_get_fusion", "q4_set_kv_format", "q4_get_kv_format", "q4_kv_format_of", "q4_ffn_pair_covers", "q4_set_use_graphs", "q4_reset_graphs", "q4_graph_captures",
    "build_sampler", "destroy_sampler", "random_u32", "random_f32", "q4_sample", "q4_build_transformer",
    "q4_free_transformer", "q4_set_quiet", "q4_transformer_new", "q4_transformer_delete", "q4_transformer_config",
    "q4_transformer_state", "q4_transformer_weights", "q4_sampler_new", "q4_sampler_delete", "q4_reset_sequence",
    "q4_shared_pos", "q4_handoff_status", "q4_handoff_timeouts", "q4_kv_stream_price", "q4_shared_token", "q4_get_logits", "q4_get_kv_row", "q4_get_logits_array", "q4_generate",
    "q4_generate_ids", "q4_chat", "q4_softmax_f32", "compute_perplexity", "q4_get_dataset_perplexity",
    "q4_parse_dataset_and_compute_perplexity", "q4_perplexity_ids", "q4_tokenizer_new", "q4_tokenizer_delete",
    "q4_tokenizer_encode", "q4_tokenizer_decode", "q4_tokenizer_max_token_length", "q4_main", "q4_parse_args",
    "q4_bench_kernel", "q4_bench_kernel_graph", "q4_bench_in_network", "q4_device_info",
    "q4_logprob_topk", "q4_set_logprobs", "q4_get_logprobs_k", "q4_get_logprobs", "q4_score_ids",
    "q4_set_greedy_screen", "q4_get_greedy_screen", "q4_screen_candidates", "q4_greedy_screen_op",
    "q4_sampler_set_controls", "q4_sampler_get_controls", "q4_sampler_set_logit_bias", "q4_parse_sampling_controls", "q4_process_logits",
    "q4_guide_new", "q4_guide_delete", "q4_set_guide", "q4_get_guide", "q4_get_guide_states", "q4_guide_mask", "q4_tokenizer_piece",
    "q4_resume_sequence", "q4_common_prefix", "q4_generate_ids_from", "q4_snapshot_new", "q4_snapshot_restore", "q4_snapshot_delete", "q4_snapshot_info",
    "q4_snapshot_tokens", "q4_snapshot_export", "q4_snapshot_import", "q4_snapshot_check", "q4_copy_runs",
    "q4_shift_context", "q4_set_context_shift", "q4_get_context_shift", "q4_parse_context_shift", "q4_get_rope_row", "q4_kv_shift",
    "q4_set_rope_scaling", "q4_get_rope_scaling", "q4_rope_scaling_of", "q4_parse_rope_scaling", "q4_rope_inv_freq", "q4_get_rope_inv_freq",
    "q4_rope_rotation_freqs",
    "q4_sampler_set_dry", "q4_sampler_get_dry", "q4_sampler_set_dry_breakers", "q4_parse_dry", "q4_dry_penalty_table", "q4_dry_penalty",
    "q4_sampler_set_adaptive", "q4_sampler_get_adaptive", "q4_parse_adaptive", "q4_get_adaptive_records", "q4_adaptive_mask",
    "q4_set_prompt_ingest", "q4_get_prompt_ingest", "q4_prompt_passes", "q4_set_pass_context", "q4_get_pass_context",
    "q4_verify_tokens", "q4_verify_covers", "q4_set_speculative", "q4_get_speculative", "q4_parse_speculative", "q4_set_drafter", "q4_spec_draft",
    "q4_spec_stats", "q4_verify_classifier", "q4_verify_accept", "q4_set_speculative_sampled", "q4_get_speculative_sampled", "q4_verify_tokens_sampled",
    "q4_verify_covers_sampled", "q4_verify_sample_rows", "q4_verify_accept_tokens", "q4_parse_speculative_sampled",
    "q4_logprob_topk_rows", "q4_set_pass_logprobs", "q4_get_pass_logprobs", "q4_set_pass_gqa", "q4_get_pass_gqa", "q4_parse_pass_gqa",
    "q4_set_pass_kv8", "q4_get_pass_kv8", "q4_parse_pass_kv8", "q4_set_pass_13b", "q4_get_pass_13b", "q4_parse_pass_13b",
    "q4_set_pass_stages", "q4_get_pass_stages", "q4_parse_pass_stages", "q4_guide_mask_rows", "q4_dry_penalty_rows", "q4_process_logits_rows",
    "q4_guide_forced_run", "q4_spec_stats_forced",
    "q4_batch_covers", "q4_batch_new", "q4_batch_delete", "q4_batch_open", "q4_batch_restore", "q4_batch_close", "q4_batch_step", "q4_batch_generate",
    "q4_batch_pos", "q4_batch_get_logits", "q4_batch_get_kv_row", "q4_batch_cache", "q4_batch_set_prefill", "q4_batch_get_prefill", "q4_batch_plan_rows",
]

_lib = None
_use_prof = os.environ.get("Q4_PROFILING_BUILD", "") == "1"


def use_profiling_build():
    global _use_prof
    assert _lib is None, "select the profiling build before the library is loaded"
    _use_prof = True


def lib():
    global _lib
    if _lib is not None:
        return _lib
    path = PROF_LIB_PATH if _use_prof else LIB_PATH
    # tools/ab.py compares builds of the library inside one gpurun call (clocks differ from box to box by several per cent)
    path = os.environ.get("Q4_LIB_OVERRIDE") or path
    if not os.path.exists(path):
        raise RuntimeError(
            "%s is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` or "
            "`make -C llama_cu_awq_amd/csrc`. There is no CPU fallback for this path." % (os.path.basename(path), path))
    L = C.CDLL(path)
    vp, i, f = C.c_void_p, C.c_int, C.c_float
    L.q4_status_string.restype = C.c_char_p
    L.q4_status_string.argtypes = [i]
    L.q4_last_error.restype = C.c_char_p
    L.q4_stream_create.argtypes = [C.POINTER(vp)]
    if hasattr(L, "q4_stream_create_masked"):      # (older builds under tools/ab.py do not have it)
        L.q4_stream_create_masked.argtypes = [C.POINTER(vp), i]
    L.q4_stream_destroy.argtypes = [vp]
    L.q4_set_stream.argtypes = [vp]
    L.q4_set_stream.restype = None
    L.q4_get_stream.restype = vp
    L.q4_malloc.argtypes = [C.POINTER(vp), C.c_size_t]
    L.q4_free.argtypes = [vp]
    L.q4_memcpy_h2d.argtypes = [vp, vp, C.c_size_t]
    L.q4_memcpy_d2h.argtypes = [vp, vp, C.c_size_t]
    L.q4_memset.argtypes = [vp, i, C.c_size_t]
    L.q4_rmsnorm.argtypes = [vp, vp, vp, i]
    L.q4_matmul_f16.argtypes = [vp, vp, vp, i, i, i, i, i, i, i, f]
    L.q4_matmul_q4.argtypes = [vp, vp, C.POINTER(QWeight), i, i, i, i, vp]
    L.q4_qkv_matvec.argtypes = [vp, vp, vp, vp, C.POINTER(QWeight), C.POINTER(QWeight), C.POINTER(QWeight), i, i, i, vp]
    L.q4_ffn_matvec_silu.argtypes = [vp, vp, C.POINTER(QWeight), C.POINTER(QWeight), i, i]
    L.q4_rope_rotation.argtypes = [vp, vp, i, i, i, vp, i, f]
    L.q4_multi_head_attention.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, vp]
    L.q4_copy_embedding.argtypes = [vp, vp, i, vp, vp]
    L.q4_convert_fp16_to_fp32.argtypes = [vp, vp, i]
    L.q4_argmax.argtypes = [vp, i, vp, vp, vp, i]
    L.q4_run_llama_network.argtypes = [vp, C.POINTER(Config), C.POINTER(RunState), C.POINTER(TransformerWeights), i]
    L.q4_run_transformer.argtypes = [i, C.POINTER(Config), C.POINTER(RunState), C.POINTER(TransformerWeights), i, vp]
    L.q4_run_transformer_at.argtypes = [i, i, C.POINTER(Config), C.POINTER(RunState), C.POINTER(TransformerWeights), i, vp]
    L.q4_set_fusion.argtypes = [i]
    L.q4_set_fusion.restype = None
    if hasattr(L, "q4_set_kv_format"):             # (older builds under tools/ab.py do not have it)
        L.q4_set_kv_format.argtypes = [i]
        L.q4_kv_format_of.argtypes = [C.POINTER(RunState)]
        L.q4_multi_head_attention_kv8.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, i, i, i, i, vp]
    if hasattr(L, "q4_kv_stream_price"):
        L.q4_kv_stream_price.restype = C.c_double
        L.q4_kv_stream_price.argtypes = [vp]
    if hasattr(L, "q4_ffn_pair_covers"):           # (older builds under tools/ab.py do not have it)
        L.q4_ffn_pair_covers.argtypes = [i, i]
    L.q4_set_use_graphs.argtypes = [i]
    L.q4_set_use_graphs.restype = None
    L.q4_reset_graphs.restype = None
    L.q4_set_quiet.argtypes = [i]
    L.q4_set_quiet.restype = None
    L.random_u32.argtypes = [C.POINTER(C.c_ulonglong)]
    L.random_u32.restype = C.c_uint
    L.random_f32.argtypes = [C.POINTER(C.c_ulonglong)]
    L.random_f32.restype = f
    L.q4_transformer_new.argtypes = [C.c_char_p, i, C.POINTER(i)]
    L.q4_transformer_new.restype = vp
    L.q4_transformer_delete.argtypes = [vp]
    L.q4_transformer_delete.restype = None
    L.q4_transformer_config.argtypes = [vp]
    L.q4_transformer_config.restype = C.POINTER(Config)
    L.q4_transformer_state.argtypes = [vp]
    L.q4_transformer_state.restype = C.POINTER(RunState)
    L.q4_transformer_weights.argtypes = [vp]
    L.q4_transformer_weights.restype = C.POINTER(TransformerWeights)
    L.q4_sampler_new.argtypes = [i, f, f, C.c_ulonglong]
    L.q4_sampler_new.restype = vp
    L.q4_sampler_delete.argtypes = [vp]
    L.q4_sampler_delete.restype = None
    L.q4_sample.argtypes = [vp, C.POINTER(RunState), i]
    L.q4_reset_sequence.argtypes = [C.POINTER(RunState), vp, i]
    L.q4_shared_pos.argtypes = [C.POINTER(RunState)]
    L.q4_shared_token.argtypes = [C.POINTER(RunState), i]
    L.q4_handoff_status.argtypes = [C.POINTER(RunState)]
    L.q4_get_logits.argtypes = [vp, vp]
    L.q4_get_kv_row.argtypes = [vp, i, i, vp, vp]
    L.q4_get_logits_array.argtypes = [vp, i, vp]
    L.q4_generate_ids.argtypes = [vp, vp, vp, i, i, vp, C.POINTER(i), C.POINTER(C.c_double)]
    L.q4_generate_ids.restype = C.c_double
    L.q4_generate.argtypes = [vp, vp, vp, C.c_char_p, i, C.POINTER(i), C.POINTER(C.c_double)]
    L.q4_generate.restype = C.c_double
    L.q4_perplexity_ids.argtypes = [vp, vp, vp, i]
    L.q4_perplexity_ids.restype = f
    L.q4_softmax_f32.argtypes = [vp, i]
    L.q4_softmax_f32.restype = None
    L.compute_perplexity.argtypes = [vp, vp, i, i]
    L.compute_perplexity.restype = f
    L.q4_tokenizer_new.argtypes = [C.c_char_p, i]
    L.q4_tokenizer_new.restype = vp
    L.q4_tokenizer_delete.argtypes = [vp]
    L.q4_tokenizer_delete.restype = None
    L.q4_tokenizer_encode.argtypes = [vp, C.c_char_p, i, i, vp, C.POINTER(i)]
    L.q4_tokenizer_decode.argtypes = [vp, i, i]
    L.q4_tokenizer_decode.restype = C.c_char_p
    L.q4_tokenizer_max_token_length.argtypes = [vp]
    L.q4_parse_args.argtypes = [i, C.POINTER(C.c_char_p), C.POINTER(CliArgs)]
    L.q4_main.argtypes = [i, C.POINTER(C.c_char_p)]
    L.q4_bench_kernel.argtypes = [i, C.POINTER(Config), C.POINTER(RunState), C.POINTER(TransformerWeights), i,
                                  C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.q4_bench_kernel.restype = C.c_double
    L.q4_bench_kernel_graph.argtypes = [i, C.POINTER(Config), C.POINTER(RunState), C.POINTER(TransformerWeights), i, i]
    L.q4_bench_kernel_graph.restype = C.c_double
    L.q4_bench_in_network.argtypes = [i, i, C.POINTER(Config), C.POINTER(RunState), C.POINTER(TransformerWeights), i,
                                      C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(i)]
    L.q4_bench_in_network.restype = C.c_double
    L.q4_device_info.argtypes = [C.c_char_p, i, C.POINTER(i), C.POINTER(C.c_size_t)]
    if hasattr(L, "q4_set_logprobs"):              # (older builds under tools/ab.py do not have it)
        L.q4_logprob_topk.argtypes = [vp, i, i, vp, vp, vp, vp, vp]
        L.q4_set_logprobs.argtypes = [vp, i]
        L.q4_get_logprobs_k.argtypes = [vp]
        L.q4_get_logprobs.argtypes = [vp, i, i, vp, vp, vp]
        L.q4_score_ids.argtypes = [vp, vp, vp, i, vp]
    if hasattr(L, "q4_set_pass_logprobs"):         # (older builds under tools/ab.py do not have it)
        L.q4_logprob_topk_rows.argtypes = [vp, i, i, i, i, vp, vp, vp, vp, vp]
        L.q4_set_pass_logprobs.argtypes = [vp, i]
        L.q4_get_pass_logprobs.argtypes = [vp]
    if hasattr(L, "q4_set_pass_gqa"):              # (older builds under tools/ab.py do not have it)
        L.q4_set_pass_gqa.argtypes = [vp, i]
        L.q4_get_pass_gqa.argtypes = [vp]
        L.q4_parse_pass_gqa.argtypes = [C.c_char_p, C.POINTER(i)]
    if hasattr(L, "q4_set_pass_13b"):              # (older builds under tools/ab.py do not have it)
        L.q4_set_pass_13b.argtypes = [vp, i]
        L.q4_get_pass_13b.argtypes = [vp]
        L.q4_parse_pass_13b.argtypes = [C.c_char_p, C.POINTER(i)]
    if hasattr(L, "q4_set_pass_kv8"):              # (older builds under tools/ab.py do not have it)
        L.q4_set_pass_kv8.argtypes = [vp, i]
        L.q4_get_pass_kv8.argtypes = [vp]
        L.q4_parse_pass_kv8.argtypes = [C.c_char_p, C.POINTER(i)]
    if hasattr(L, "q4_set_pass_stages"):           # (older builds under tools/ab.py do not have it)
        L.q4_set_pass_stages.argtypes = [vp, i]
        L.q4_get_pass_stages.argtypes = [vp]
        L.q4_parse_pass_stages.argtypes = [C.c_char_p, C.POINTER(i)]
        L.q4_guide_mask_rows.argtypes = [vp, i, vp, vp, i, i, vp, vp]
        L.q4_dry_penalty_rows.argtypes = [vp, i, C.POINTER(DryControls), vp, i, i, i, vp, vp]
        L.q4_process_logits_rows.argtypes = [vp, i, C.POINTER(SamplingControls), vp, vp, i, i, i, vp, vp]
        L.q4_guide_forced_run.argtypes = [vp, i, i, vp]
        L.q4_spec_stats_forced.argtypes = [vp, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    if hasattr(L, "q4_set_greedy_screen"):         # (older builds under tools/ab.py do not have it)
        L.q4_set_greedy_screen.argtypes = [i]
        L.q4_set_greedy_screen.restype = None
        L.q4_screen_candidates.argtypes = [vp, C.POINTER(i), C.POINTER(i), C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
        L.q4_greedy_screen_op.argtypes = [vp, vp, i, i, vp, C.POINTER(i), vp, vp, vp, C.POINTER(i)]
    if hasattr(L, "q4_set_prompt_ingest"):         # (older builds under tools/ab.py do not have it)
        L.q4_set_prompt_ingest.argtypes = [i]
        L.q4_set_prompt_ingest.restype = None
    if hasattr(L, "q4_set_pass_context"):          # (older builds under tools/ab.py do not have it)
        L.q4_set_pass_context.argtypes = [i]
        L.q4_set_pass_context.restype = None
        L.q4_get_pass_context.argtypes = []
        L.q4_get_pass_context.restype = i
    if hasattr(L, "q4_verify_tokens"):             # (older builds under tools/ab.py do not have it)
        ll = C.c_longlong
        L.q4_verify_tokens.argtypes = [vp, vp, i, vp, C.POINTER(i)]
        L.q4_verify_covers.argtypes = [vp, i, i]
        L.q4_set_speculative.argtypes = [vp, i, i, i]
        L.q4_get_speculative.argtypes = [vp, C.POINTER(i), C.POINTER(i), C.POINTER(i)]
        L.q4_parse_speculative.argtypes = [C.c_char_p, C.POINTER(i), C.POINTER(i), C.POINTER(i)]
        L.q4_set_drafter.argtypes = [vp, DRAFTER_FN, vp]
        L.q4_spec_draft.argtypes = [vp, i, i, i, i, vp]
        L.q4_spec_stats.argtypes = [vp, C.POINTER(ll), C.POINTER(ll), C.POINTER(ll)]
        L.q4_verify_classifier.argtypes = [vp, vp, vp, vp, i, i, i]
        L.q4_verify_accept.argtypes = [vp, i, i, vp, i, vp, i, vp, vp, vp, vp, vp, vp]
    if hasattr(L, "q4_verify_tokens_sampled"):     # (older builds under tools/ab.py do not have it)
        L.q4_set_speculative_sampled.argtypes = [vp, i]
        L.q4_get_speculative_sampled.argtypes = [vp]
        L.q4_parse_speculative_sampled.argtypes = [C.c_char_p, C.POINTER(i)]
        L.q4_verify_tokens_sampled.argtypes = [vp, vp, vp, i, vp, C.POINTER(i)]
        L.q4_verify_covers_sampled.argtypes = [vp, vp, i, i]
        L.q4_verify_sample_rows.argtypes = [vp, vp, i, i, vp, vp]
        L.q4_verify_accept_tokens.argtypes = [vp, i, i, vp, i, vp, vp, i, vp, vp, vp, vp, vp, vp]
    if hasattr(L, "q4_sampler_set_controls"):      # (older builds under tools/ab.py do not have it)
        L.q4_sampler_set_controls.argtypes = [vp, C.POINTER(SamplingControls)]
        L.q4_sampler_get_controls.argtypes = [vp, C.POINTER(SamplingControls)]
        L.q4_sampler_set_logit_bias.argtypes = [vp, vp, vp, i]
        L.q4_parse_sampling_controls.argtypes = [C.c_char_p, C.POINTER(SamplingControls)]
        L.q4_process_logits.argtypes = [vp, i, C.POINTER(SamplingControls), vp, vp, i, vp, vp]
    if hasattr(L, "q4_guide_new"):                 # (older builds under tools/ab.py do not have it)
        L.q4_guide_new.argtypes = [C.POINTER(vp), i, i, vp]
        L.q4_guide_delete.argtypes = [vp]
        L.q4_set_guide.argtypes = [vp, vp]
        L.q4_get_guide.argtypes = [vp]
        L.q4_get_guide.restype = vp
        L.q4_get_guide_states.argtypes = [vp, i, i, vp]
        L.q4_guide_mask.argtypes = [vp, i, vp, vp, vp, vp]
        L.q4_tokenizer_piece.argtypes = [vp, i, C.POINTER(C.c_void_p), C.POINTER(i)]
    if hasattr(L, "q4_snapshot_new"):              # (older builds under tools/ab.py do not have it)
        ll = C.c_longlong
        L.q4_resume_sequence.argtypes = [C.POINTER(RunState), vp, i, i]
        L.q4_common_prefix.argtypes = [vp, vp, i]
        L.q4_generate_ids_from.argtypes = [vp, vp, vp, i, i, i, vp, C.POINTER(i), C.POINTER(C.c_double)]
        L.q4_generate_ids_from.restype = C.c_double
        L.q4_snapshot_new.argtypes = [C.POINTER(vp), vp, i]
        L.q4_snapshot_restore.argtypes = [vp, vp]
        L.q4_snapshot_delete.argtypes = [vp]
        L.q4_snapshot_info.argtypes = [vp, C.POINTER(SnapshotInfo)]
        L.q4_snapshot_tokens.argtypes = [vp, vp]
        L.q4_snapshot_export.argtypes = [vp, vp, C.c_size_t]
        L.q4_snapshot_import.argtypes = [C.POINTER(vp), vp, C.c_size_t]
        L.q4_snapshot_check.argtypes = [vp, C.c_size_t, C.POINTER(SnapshotInfo)]
        L.q4_copy_runs.argtypes = [vp, vp, ll, ll, ll, ll]
    if hasattr(L, "q4_batch_new"):                 # (older builds under tools/ab.py do not have it)
        L.q4_batch_covers.argtypes = [vp]
        L.q4_batch_new.argtypes = [C.POINTER(vp), vp, i]
        L.q4_batch_delete.argtypes = [vp]
        L.q4_batch_open.argtypes = [vp, i, vp, i, C.c_ulonglong]
        L.q4_batch_restore.argtypes = [vp, i, vp, vp, i, C.c_ulonglong]
        L.q4_batch_close.argtypes = [vp, i]
        L.q4_batch_step.argtypes = [vp, vp, vp]
        L.q4_batch_generate.argtypes = [vp, vp, i, vp, C.POINTER(i)]
        L.q4_batch_pos.argtypes = [vp, i]
        L.q4_batch_get_logits.argtypes = [vp, i, vp]
        L.q4_batch_get_kv_row.argtypes = [vp, i, i, i, vp, vp]
        L.q4_batch_cache.argtypes = [vp, i, C.POINTER(vp), C.POINTER(vp)]
    if hasattr(L, "q4_batch_set_prefill"):         # (likewise)
        L.q4_batch_set_prefill.argtypes = [vp, i]
        L.q4_batch_get_prefill.argtypes = [vp]
        L.q4_batch_plan_rows.argtypes = [vp, vp, vp, i, i, vp]
        if _use_prof:
            L.q4_set_batch_run_form.argtypes = [i]
            L.q4_set_batch_run_form.restype = None
    if hasattr(L, "q4_shift_context"):             # (older builds under tools/ab.py do not have it)
        L.q4_shift_context.argtypes = [vp, i, i, i, i]
        L.q4_set_context_shift.argtypes = [vp, i, i]
        L.q4_get_context_shift.argtypes = [vp, C.POINTER(i), C.POINTER(i)]
        L.q4_parse_context_shift.argtypes = [C.c_char_p, C.POINTER(i), C.POINTER(i)]
        L.q4_get_rope_row.argtypes = [vp, i, vp]
        L.q4_kv_shift.argtypes = [vp, vp, vp, vp, i, i, i, i, i, i, i, i, vp]
    if hasattr(L, "q4_set_rope_scaling"):          # (older builds under tools/ab.py do not have it)
        L.q4_set_rope_scaling.argtypes = [C.POINTER(RopeScaling)]
        L.q4_get_rope_scaling.argtypes = [C.POINTER(RopeScaling)]
        L.q4_rope_scaling_of.argtypes = [vp, C.POINTER(RopeScaling)]
        L.q4_parse_rope_scaling.argtypes = [C.c_char_p, C.POINTER(RopeScaling)]
        L.q4_rope_inv_freq.argtypes = [C.POINTER(RopeScaling), i, f, vp]
        L.q4_get_rope_inv_freq.argtypes = [vp, vp]
        L.q4_rope_rotation_freqs.argtypes = [vp, vp, i, i, i, vp, i, vp]
    if hasattr(L, "q4_sampler_set_dry"):           # (older builds under tools/ab.py do not have it)
        L.q4_sampler_set_dry.argtypes = [vp, C.POINTER(DryControls)]
        L.q4_sampler_get_dry.argtypes = [vp, C.POINTER(DryControls)]
        L.q4_sampler_set_dry_breakers.argtypes = [vp, vp, i]
        L.q4_parse_dry.argtypes = [C.c_char_p, C.POINTER(DryControls)]
        L.q4_dry_penalty_table.argtypes = [C.POINTER(DryControls), vp]
        L.q4_dry_penalty.argtypes = [vp, i, C.POINTER(DryControls), vp, i, vp, vp]
    if hasattr(L, "q4_sampler_set_adaptive"):      # (older builds under tools/ab.py do not have it)
        L.q4_sampler_set_adaptive.argtypes = [vp, C.POINTER(AdaptiveControls)]
        L.q4_sampler_get_adaptive.argtypes = [vp, C.POINTER(AdaptiveControls)]
        L.q4_parse_adaptive.argtypes = [C.c_char_p, C.POINTER(AdaptiveControls)]
        L.q4_get_adaptive_records.argtypes = [vp, i, i, vp]
        L.q4_adaptive_mask.argtypes = [vp, i, C.POINTER(AdaptiveControls), f, vp, vp, vp, vp, vp]
    if _use_prof:
        for name, at in (("q4_set_gemv_tune", [i, i, i]), ("q4_set_gemv_early", [i, i]), ("q4_set_half_tail", [i]),
                         ("q4_set_ksplit", [i]), ("q4_set_ablate", [i]), ("q4_set_skip_mask", [i]),
                         ("q4_set_attention_split", [i, i]), ("q4_set_debug_buffer", [vp])):
            getattr(L, name).argtypes = at
            getattr(L, name).restype = None
    _lib = L
    return L


class Q4Error(RuntimeError):
    pass


def check(rc):
    if rc != 0:
        L = lib()
        raise Q4Error("%s (status %d) %s" % (L.q4_status_string(rc).decode(), rc, L.q4_last_error().decode()))


class DevBuf:
    """A HIP device allocation holding a numpy array's bytes."""

    def __init__(self, arr=None, nbytes=None):
        L = lib()
        if arr is not None:
            arr = np.ascontiguousarray(arr)
            nbytes = arr.nbytes
        self.nbytes = max(int(nbytes), 16)
        p = C.c_void_p()
        check(L.q4_malloc(C.byref(p), self.nbytes))
        self.ptr = p.value
        if arr is not None:
            check(L.q4_memcpy_h2d(self.ptr, arr.ctypes.data, arr.nbytes))
        else:
            check(L.q4_memset(self.ptr, 0, self.nbytes))
            check(L.q4_stream_synchronize())

    def get(self, dtype, count=None):
        dtype = np.dtype(dtype)
        n = self.nbytes // dtype.itemsize if count is None else count
        out = np.empty(n, dtype=dtype)
        check(lib().q4_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes))
        return out

    def put(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        check(lib().q4_memcpy_h2d(self.ptr, arr.ctypes.data, arr.nbytes))

    def free(self):
        if self.ptr:
            lib().q4_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DevQWeight:
    """QWeight (common.h:20-24) on the device, from (weight u32, zeros u32, scales f16) numpy arrays."""

    def __init__(self, weight, zeros, scales):
        self.bufs = [DevBuf(weight), DevBuf(zeros), DevBuf(scales)]
        self.q = QWeight(self.bufs[0].ptr, self.bufs[1].ptr, self.bufs[2].ptr)

    def ref(self):
        return C.byref(self.q)


# ---- the reference's host functions, same names and argument order (llama2_q4.cu:209-284) ----------------
def rmsnorm(o, x, weight, size):
    check(lib().q4_rmsnorm(o.ptr, x.ptr, weight.ptr, size))


def matmul(xout, x, w, n, d, batch=1, x_stride=0, w_stride=0, op_stride=0, w_row_stride=-1, alpha=1.0):
    check(lib().q4_matmul_f16(xout.ptr, x.ptr, w.ptr, n, d, batch, x_stride, w_stride, op_stride, w_row_stride, alpha))


def matmul_q4(xout, x, w, inpSize, opSize, accum=False, loff=-1, pPos=None):
    check(lib().q4_matmul_q4(xout.ptr, x.ptr, w.ref(), inpSize, opSize, int(accum), loff, pPos.ptr if pPos else None))


def qkv_matvec(q, key_cache, value_cache, x, qw, kw, vw, inpSize, opSize, loff, pPos):
    check(lib().q4_qkv_matvec(q.ptr, key_cache.ptr, value_cache.ptr, x.ptr, qw.ref(), kw.ref(), vw.ref(), inpSize, opSize,
                              loff, pPos.ptr))


def ffn_matvec_silu(xout, x, gate_w, up_w, inpSize, opSize):
    check(lib().q4_ffn_matvec_silu(xout.ptr, x.ptr, gate_w.ref(), up_w.ref(), inpSize, opSize))


def RoPERotation(q, k, num_heads, num_kv_heads, head_size, pPos, loff, rope_theta):
    check(lib().q4_rope_rotation(q.ptr, k.ptr, num_heads, num_kv_heads, head_size, pPos.ptr, loff, rope_theta))


def MultiHeadAttention(output, q, key_cache, value_cache, att, num_heads, head_size, kv_mul, max_seq_len, pPos,
                       kv_offset_bytes=0):
    check(lib().q4_multi_head_attention(output.ptr, q.ptr, key_cache.ptr + kv_offset_bytes, value_cache.ptr + kv_offset_bytes,
                                        att.ptr if att else None, num_heads, head_size, kv_mul, max_seq_len, pPos.ptr))


def logprob_topk(logits, n, top_k, target, lse, target_logprob, top_ids=None, top_logprobs=None):
    """q4_logprob_topk over DevBufs: the model's own distribution (temperature 1, no nucleus). target: a DevBuf holding one int32, or None."""
    check(lib().q4_logprob_topk(logits.ptr, n, top_k, target.ptr if target else None, lse.ptr, target_logprob.ptr,
                                top_ids.ptr if top_ids else None, top_logprobs.ptr if top_logprobs else None))


def _bias_arrays(logit_bias):
    """{id: bias} (or None) -> (ids int32, bias float32)"""
    items = sorted((logit_bias or {}).items())
    return np.array([k for k, _ in items], dtype=np.int32), np.array([v for _, v in items], dtype=np.float32)


def parse_sampling_controls(text):
    """q4_parse_sampling_controls: "top_k=40,min_p=0.05,repeat_penalty=1.1,last_n=64,presence=0,frequency=0" -> SamplingControls"""
    c = SamplingControls()
    check(lib().q4_parse_sampling_controls(text.encode(), C.byref(c)))
    return c


def process_logits(logits, n, controls=None, logit_bias=None, tokens=None, pos=None, **kw):
    """q4_process_logits over DevBufs: rewrites `logits` (n halves) in place -- bias, penalties over the window of the ring `tokens` (int32) that ends
    at the position in `pos` (one int32), top-k, min-p. controls: a SamplingControls, or its fields as keywords; logit_bias: {id: bias}."""
    c = controls if controls is not None else SamplingControls(**kw)
    ids, bias = _bias_arrays(logit_bias)
    check(lib().q4_process_logits(logits.ptr, n, C.byref(c), ids.ctypes.data, bias.ctypes.data, ids.shape[0], tokens.ptr if tokens else None,
                                  pos.ptr if pos else None))


def process_logits_rows(logits, n, ld, n_rows, view, pos_rows, controls=None, logit_bias=None, **kw):
    """q4_process_logits_rows over DevBufs: the row form -- rows r < n_rows of `logits`, ld halves apart, row r at position pos_rows[r] (int32), the window
    read from `view` (int32 tokens by absolute position: a ring prefix and the drafts behind it)."""
    c = controls if controls is not None else SamplingControls(**kw)
    ids, bias = _bias_arrays(logit_bias)
    check(lib().q4_process_logits_rows(logits.ptr, n, C.byref(c), ids.ctypes.data, bias.ctypes.data, ids.shape[0], ld, n_rows, view.ptr if view else None,
                                       pos_rows.ptr if pos_rows else None))


def parse_dry(text):
    """q4_parse_dry: "multiplier=0.8,base=1.75,allowed=2,last_n=1024,ngram=0" -> DryControls"""
    c = DryControls()
    check(lib().q4_parse_dry(text.encode(), C.byref(c)))
    return c


def dry_penalty_table(controls=None, **kw):
    """q4_dry_penalty_table (host only): pen[0 .. 64] float32 -- multiplier * powf(base, L - allowed_length) clamped to 3.0e38 from allowed_length on,
    0 below"""
    c = controls if controls is not None else DryControls(**kw)
    out = np.empty(DRY_MAX_MATCH + 1, dtype=np.float32)
    check(lib().q4_dry_penalty_table(C.byref(c), out.ctypes.data))
    return out


def _breaker_array(breakers):
    return np.ascontiguousarray(sorted(breakers) if isinstance(breakers, (set, frozenset)) else (breakers if breakers is not None else []),
                                dtype=np.int32).reshape(-1)


def dry_penalty(logits, n, controls=None, breakers=None, tokens=None, pos=None, **kw):
    """q4_dry_penalty over DevBufs: rewrites `logits` (n halves) in place -- the DRY penalty and the n-gram ban over the window of the ring `tokens`
    (int32) that ends at the position in `pos` (one int32). controls: a DryControls, or its fields as keywords; breakers: token ids."""
    c = controls if controls is not None else DryControls(**kw)
    ids = _breaker_array(breakers)
    check(lib().q4_dry_penalty(logits.ptr, n, C.byref(c), ids.ctypes.data, ids.shape[0], tokens.ptr if tokens else None, pos.ptr if pos else None))


def dry_penalty_rows(logits, n, ld, n_rows, view, pos_rows, controls=None, breakers=None, **kw):
    """q4_dry_penalty_rows over DevBufs: the row form -- rows r < n_rows of `logits`, ld halves apart, row r at position pos_rows[r] (int32), the window
    read from `view` (int32 tokens by absolute position: a ring prefix and the drafts behind it)."""
    c = controls if controls is not None else DryControls(**kw)
    ids = _breaker_array(breakers)
    check(lib().q4_dry_penalty_rows(logits.ptr, n, C.byref(c), ids.ctypes.data, ids.shape[0], ld, n_rows, view.ptr if view else None,
                                    pos_rows.ptr if pos_rows else None))


def dry_breaker_ids(tokenizer, strings=DRY_BREAKER_STRINGS):
    """the ids of every token whose piece contains one of `strings` (llama.cpp's default sequence breakers, as single tokens); a byte-fallback piece
    <0xHH> counts as its byte"""
    needles = [s.encode("utf-8") if isinstance(s, str) else bytes(s) for s in strings]
    out = []
    for i, piece in enumerate(tokenizer.pieces()):
        if len(piece) == 6 and piece.startswith(b"<0x") and piece.endswith(b">"):
            try:
                piece = bytes([int(piece[3:5], 16)])
            except ValueError:
                pass
        if any(s in piece for s in needles):
            out.append(i)
    return out


def parse_adaptive(text):
    """q4_parse_adaptive: "typical_p=0.9,top_n_sigma=1.5,mirostat_tau=5,mirostat_eta=0.1" -> AdaptiveControls"""
    c = AdaptiveControls()
    check(lib().q4_parse_adaptive(text.encode(), C.byref(c)))
    return c


def adaptive_record(raw):
    """one raw record (ADAPTIVE_RECORD float32) as a dict: T_s, H, d_star, mu, T_m, lse, lse_t floats (NaN: the stage was off), kept an int"""
    raw = np.ascontiguousarray(raw, dtype=np.float32)
    out = {k: np.float32(raw[j]) for j, k in enumerate(ADAPTIVE_RECORD_FIELDS)}
    out["kept"] = int(raw[5:6].view(np.int32)[0])
    return out


def adaptive_mask(logits, n, controls=None, temperature=1.0, mu_ring=None, side=None, tokens=None, pos=None, record=None, **kw):
    """q4_adaptive_mask over DevBufs: top-n-sigma, typical-p and Mirostat v2 write -inf over `logits` (n halves) in place. controls: an
    AdaptiveControls, or its fields as keywords. With Mirostat: mu_ring (float32 by position), side (n + 2 float32), tokens (the ring, int32), pos (one
    int32) and a temperature above 0. record: ADAPTIVE_RECORD float32 (adaptive_record reads them)."""
    c = controls if controls is not None else AdaptiveControls(**kw)
    check(lib().q4_adaptive_mask(logits.ptr, n, C.byref(c), float(temperature), mu_ring.ptr if mu_ring else None, side.ptr if side else None,
                                 tokens.ptr if tokens else None, pos.ptr if pos else None, record.ptr if record else None))


class Guide:
    """q4_guide: a token automaton on the device. table: uint16 [S, V], an entry a state or GUIDE_DEAD (llama_cu_awq_amd.guide builds them from
    choices or a regular expression). Immutable; may be attached to several models of the same vocabulary; close() fails while one still holds it."""

    def __init__(self, table):
        table = np.ascontiguousarray(table, dtype=np.uint16)
        if table.ndim != 2:
            raise ValueError("a guide's table is [states, vocabulary]")
        self.n_states, self.vocab_size = int(table.shape[0]), int(table.shape[1])
        h = C.c_void_p()
        check(lib().q4_guide_new(C.byref(h), self.n_states, self.vocab_size, table.ctypes.data))
        self.h = h.value

    def forced_run(self, state, max_draft):
        """q4_guide_forced_run: the tokens the automaton forces from `state` (each state on the way has exactly one live token), at most max_draft, ending
        behind an EOS; int32. guide.forced_run is the numpy restatement."""
        out = np.empty(max(int(max_draft), 1), dtype=np.int32)
        n = lib().q4_guide_forced_run(self.h, int(state), int(max_draft), out.ctypes.data)
        return out[:n].copy()

    def close(self):
        if getattr(self, "h", None):
            check(lib().q4_guide_delete(self.h))
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def guide_mask(logits, n, guide, state_ring, tokens, pos):
    """q4_guide_mask over DevBufs: one guide launch -- advances the automaton at the position in `pos` (one int32) from state_ring[pos - 1] and the ring
    entry tokens[pos], writes state_ring[pos] and -inf over the logits (n halves) the new state forbids."""
    check(lib().q4_guide_mask(logits.ptr, n, guide.h, state_ring.ptr, tokens.ptr, pos.ptr))


def guide_mask_rows(logits, n, ld, n_rows, guide, state_ring, view, pos_rows):
    """q4_guide_mask_rows over DevBufs: the row form -- rows r < n_rows of `logits`, ld halves apart, at positions pos_rows[r] = pos_rows[0] + r; block r walks
    the automaton from state_ring[pos_rows[0] - 1] over view[pos_rows[0] .. pos_rows[r]], writes state_ring[pos_rows[r]] and masks row r."""
    check(lib().q4_guide_mask_rows(logits.ptr, n, guide.h, state_ring.ptr, ld, n_rows, view.ptr, pos_rows.ptr))


def copy_runs(dst, src, outer, dst_stride, src_stride, run_bytes, dst_offset=0, src_offset=0):
    """q4_copy_runs over DevBufs: run r < outer moves run_bytes bytes from src + src_offset + r * src_stride to dst + dst_offset + r * dst_stride, in
    stream order (q4_kv_copy.hip: the launch that takes and restores snapshots)."""
    check(lib().q4_copy_runs(dst.ptr + dst_offset, src.ptr + src_offset, outer, dst_stride, src_stride, run_bytes))


def snapshot_check(blob):
    """q4_snapshot_check: validates a serialised snapshot without touching the GPU; the header's fields as a dict, or Q4Error"""
    blob = bytes(blob)
    info = SnapshotInfo()
    check(lib().q4_snapshot_check(blob, len(blob), C.byref(info)))
    return info.as_dict()


class Snapshot:
    """q4_snapshot: the K / V rows of positions [0, n_pos) of a model, packed on the device, with the tokens they were computed from. Immutable. Made by
    Transformer.snapshot() or Snapshot.from_bytes(); given to Transformer.restore() or generate_ids(reuse=...) of any model of the same checkpoint."""

    def __init__(self, handle):
        self.h = handle
        info = SnapshotInfo()
        check(lib().q4_snapshot_info(self.h, C.byref(info)))
        self.info = info.as_dict()
        self.n_pos = info.n_pos
        self.nbytes = info.device_bytes
        self.tokens = np.empty(self.n_pos, dtype=np.int32)
        check(lib().q4_snapshot_tokens(self.h, self.tokens.ctypes.data))

    def to_bytes(self):
        out = np.empty(self.info["export_bytes"], dtype=np.uint8)
        check(lib().q4_snapshot_export(self.h, out.ctypes.data, out.nbytes))
        return out.tobytes()

    @classmethod
    def from_bytes(cls, b):
        b = bytes(b)
        h = C.c_void_p()
        check(lib().q4_snapshot_import(C.byref(h), b, len(b)))
        return cls(h.value)

    def close(self):
        if getattr(self, "h", None):
            check(lib().q4_snapshot_delete(self.h))
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def verify_classifier(logits, x, rms_w, wcls, dim, vocab, n_rows):
    """q4_verify_classifier over DevBufs: logits [n_rows, vocab] = wcls . rmsnorm(x[r], rms_w), the verify pass's classifier launch."""
    check(lib().q4_verify_classifier(logits.ptr, x.ptr, rms_w.ptr, wcls.ptr, dim, vocab, n_rows))


def verify_accept(logits, ld, size, draft, x, dim, logits_out, x_out, ring, pos_host, pos_dev, report=None):
    """q4_verify_accept over DevBufs (draft: host ids): the verify pass's accept launch."""
    d = np.ascontiguousarray(draft, dtype=np.int32)
    check(lib().q4_verify_accept(logits.ptr, ld, size, d.ctypes.data, d.shape[0], x.ptr if x else None, dim, logits_out.ptr, x_out.ptr if x_out else None,
                                 ring.ptr, pos_host.ptr, pos_dev.ptr, report.ptr if report else None))


def verify_accept_tokens(logits, ld, size, draft, tokens, x, dim, logits_out, x_out, ring, pos_host, pos_dev, report=None):
    """q4_verify_accept_tokens over DevBufs (draft: host ids; tokens: the rows' tokens, device): the accept launch of a pass under the sampler."""
    d = np.ascontiguousarray(draft, dtype=np.int32)
    check(lib().q4_verify_accept_tokens(logits.ptr, ld, size, d.ctypes.data, d.shape[0], tokens.ptr if tokens else None, x.ptr if x else None, dim,
                                        logits_out.ptr, x_out.ptr if x_out else None, ring.ptr, pos_host.ptr, pos_dev.ptr, report.ptr if report else None))


def verify_sample_rows(sampler, logits, ld, n_rows, coins, tokens):
    """q4_verify_sample_rows over DevBufs (sampler: a q4_sampler_new handle; coins: host floats): rows normalised in place, tokens[r] sampled with coins[r]."""
    c = np.ascontiguousarray(coins, dtype=np.float32)
    check(lib().q4_verify_sample_rows(sampler, logits.ptr, ld, n_rows, c.ctypes.data, tokens.ptr))


def greedy_screen_op(x, w, n, d, rms_w=None):
    """q4_greedy_screen_op over DevBufs: (token, A [d] float32, B [d] float32, refined logits [d] float16, candidate rows)."""
    tok, cand = C.c_int(), C.c_int()
    A = np.empty(d, dtype=np.float32)
    B = np.empty(d, dtype=np.float32)
    refined = np.empty(d, dtype=np.float16)
    check(lib().q4_greedy_screen_op(x.ptr, w.ptr, n, d, rms_w.ptr if rms_w else None, C.byref(tok), A.ctypes.data, B.ctypes.data, refined.ctypes.data,
                                    C.byref(cand)))
    return tok.value, A, B, refined, cand.value


def set_greedy_screen(on):
    lib().q4_set_greedy_screen(int(on))


def set_prompt_ingest(max_tokens):
    """q4_set_prompt_ingest: positions per prompt pass of the token loop, 0 off (csrc/prompt_pass.h)."""
    lib().q4_set_prompt_ingest(int(max_tokens))


def get_prompt_ingest():
    return lib().q4_get_prompt_ingest()


def logprob_topk_rows(logits, ld, n, n_rows, top_k, targets, lse, target_logprob, top_ids=None, top_logprobs=None):
    """q4_logprob_topk_rows over DevBufs: q4_logprob_topk for n_rows rows `ld` halves apart, one block per row. targets: a DevBuf of n_rows int32, or None;
    the outputs hold n_rows (x top_k) entries."""
    check(lib().q4_logprob_topk_rows(logits.ptr, ld, n, n_rows, top_k, targets.ptr if targets else None, lse.ptr, target_logprob.ptr,
                                     top_ids.ptr if top_ids else None, top_logprobs.ptr if top_logprobs else None))


def set_pass_context(positions):
    """q4_set_pass_context: the exclusive upper bound on the positions a prompt pass or a verify pass may touch; 256 (the default) at the least."""
    lib().q4_set_pass_context(int(positions))


def get_pass_context():
    return lib().q4_get_pass_context()


def prompt_passes():
    """Prompt passes run since the library was loaded (q4_prompt_passes)."""
    return lib().q4_prompt_passes()


def spec_draft(tokens, max_draft, ngram_max, ngram_min):
    """q4_spec_draft, the built-in prompt-lookup drafter (host only): the ids that followed the most recent earlier occurrence of the ring's last g tokens,
    g from ngram_max down to ngram_min; [] for no match."""
    t = np.ascontiguousarray(tokens, dtype=np.int32)
    out = np.zeros(max(int(max_draft), 1), dtype=np.int32)
    n = lib().q4_spec_draft(t.ctypes.data, t.shape[0], int(max_draft), int(ngram_max), int(ngram_min), out.ctypes.data)
    return [int(x) for x in out[:n]]


def parse_speculative(text):
    """q4_parse_speculative: "draft=4,ngram=3,min=2" -> dict(draft, ngram, min)"""
    d, g, m = C.c_int(), C.c_int(), C.c_int()
    check(lib().q4_parse_speculative(text.encode(), C.byref(d), C.byref(g), C.byref(m)))
    return {"draft": d.value, "ngram": g.value, "min": m.value}


def synchronize():
    check(lib().q4_stream_synchronize())


def device_info():
    name = C.create_string_buffer(256)
    cu = C.c_int()
    mem = C.c_size_t()
    check(lib().q4_device_info(name, 256, C.byref(cu), C.byref(mem)))
    return name.value.decode(), cu.value, mem.value


class Transformer:
    """build_transformer / free_transformer (llama2_q4.cu:408-432) + run_transformer + sampler, by handle."""

    def __init__(self, path, perplexity=False, temperature=0.0, topp=0.9, seed=1, quiet=True, kv="fp16", logprobs=None, sampling=None,
                 logit_bias=None, guide=None, context_shift=None, rope_scaling=None, dry=None, dry_breakers=None, tokenizer=None, adaptive=None, speculative=None,
                 pass_logprobs=False, pass_gqa=False, pass_stages=False, pass_kv8=False, pass_13b=False):
        L = lib()
        L.q4_set_quiet(1 if quiet else 0)
        st = C.c_int()
        if kv not in KV_FORMATS:
            raise ValueError("kv: 'fp16' or 'fp8', not %r" % (kv,))
        # the format is a process-wide setting read by the build: set around it and restored, whatever the build does
        has = hasattr(L, "q4_set_kv_format")           # (older builds under tools/ab.py do not have it: fp16 only)
        if not has and kv != "fp16":
            raise Q4Error("this build of the library has no FP8 K / V cache")
        before = L.q4_get_kv_format() if has else KV_FP16
        # ... and so is the RoPE scaling (rope_scaling_struct lists the accepted forms)
        has_rope = hasattr(L, "q4_set_rope_scaling")   # (older builds under tools/ab.py do not have it: unscaled only)
        if not has_rope and rope_scaling is not None:
            raise Q4Error("this build of the library has no RoPE scaling")
        rope, rope_keep = rope_scaling_struct(rope_scaling) if has_rope else (None, None)
        rope_before = RopeScaling()
        if has_rope:
            check(L.q4_get_rope_scaling(C.byref(rope_before)))
            if rope_before.kind == ROPE_CUSTOM:        # (points at the library's copy, which the next call rewrites)
                rope_before_keep = np.array(rope_before.inv_freq[:rope_before.n_freqs], dtype=np.float32)
                rope_before.inv_freq = rope_before_keep.ctypes.data_as(C.POINTER(C.c_float))
            if L.q4_set_rope_scaling(C.byref(rope)):
                raise ValueError("rope_scaling: %r is refused (factor >= 1; llama3: 0 < low_freq_factor < high_freq_factor, "
                                 "original_max_position_embeddings >= 1; custom: 1 .. %d finite frequencies >= 0)" % (rope_scaling, ROPE_MAX_PAIRS))
        if has:
            check(L.q4_set_kv_format(KV_FORMATS[kv]))
        try:
            self.h = L.q4_transformer_new(path.encode(), int(perplexity), C.byref(st))
        finally:
            if has:
                L.q4_set_kv_format(before)
            if has_rope:
                L.q4_set_rope_scaling(C.byref(rope_before))
        del rope_keep
        self.kv_format = kv
        if not self.h:
            raise Q4Error("build_transformer failed: %s %s" % (L.q4_status_string(st.value).decode(), L.q4_last_error().decode()))
        # a COPY of the header: the C struct lives inside the Transformer and dies with close(); readers of
        # `config` (bench.py prints it after closing) must never see freed memory
        self.config = Config.from_buffer_copy(L.q4_transformer_config(self.h).contents)
        self.state = L.q4_transformer_state(self.h)
        self.weights = L.q4_transformer_weights(self.h)
        self.sampler = L.q4_sampler_new(self.config.vocab_size, temperature, topp, seed)
        if not self.sampler:
            raise Q4Error("build_sampler failed")
        try:
            if logprobs is not None:
                self.set_logprobs(logprobs)
            if pass_logprobs:
                self.set_pass_logprobs(True)
            if pass_gqa:
                self.set_pass_gqa(True)
            if pass_kv8:
                self.set_pass_kv8(True)
            if pass_13b:
                self.set_pass_13b(True)
            if pass_stages:
                self.set_pass_stages(True)
            if sampling is not None:
                self.set_sampling(**sampling)
            if logit_bias is not None:
                self.set_logit_bias(logit_bias)
            if guide is not None:
                self.set_guide(guide)
            if context_shift is not None:
                self.set_context_shift(*context_shift)
            if dry is not None:
                self.set_dry(**dry)
            if dry_breakers is not None:
                self.set_dry_breakers(dry_breakers, tokenizer=tokenizer)
            if adaptive is not None:
                self.set_adaptive(**adaptive)
            if speculative is not None:
                self.set_speculative(**speculative)
        except Exception:
            self.close()
            raise

    def close(self):
        L = lib()
        if getattr(self, "h", None):
            L.q4_stream_synchronize()
            L.q4_reset_graphs()
            L.q4_sampler_delete(self.sampler)
            L.q4_transformer_delete(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self, prompt_tokens):
        t = np.ascontiguousarray(prompt_tokens, dtype=np.int32)
        check(lib().q4_reset_sequence(self.state, t.ctypes.data, t.shape[0]))

    def run_transformer(self, gen_token, copy_logits=False):
        check(lib().q4_run_transformer(int(gen_token), C.byref(self.config), self.state, self.weights, int(copy_logits),
                                       self.sampler))

    def run_transformer_at(self, pos, gen_token, copy_logits=False):
        """the step with the position supplied by the caller: queued behind the previous one, nothing is read back (q4_run_transformer_at)"""
        check(lib().q4_run_transformer_at(int(pos), int(gen_token), C.byref(self.config), self.state, self.weights, int(copy_logits),
                                          self.sampler))

    def logits(self):
        out = np.empty(self.config.vocab_size, dtype=np.float16)
        check(lib().q4_get_logits(self.h, out.ctypes.data))
        return out

    def kv_row(self, layer, pos):
        kv_dim = self.config.dim * self.config.n_kv_heads // self.config.n_heads
        k = np.empty(kv_dim, dtype=np.float16)
        v = np.empty(kv_dim, dtype=np.float16)
        check(lib().q4_get_kv_row(self.h, layer, pos, k.ctypes.data, v.ctypes.data))
        return k, v

    def logits_array(self, num_pos):
        out = np.empty((num_pos, self.config.vocab_size), dtype=np.float32)
        check(lib().q4_get_logits_array(self.h, num_pos, out.ctypes.data))
        return out

    def pos(self):
        return lib().q4_shared_pos(self.state)

    def token(self, i):
        return lib().q4_shared_token(self.state, i)

    def generate_ids(self, prompt_tokens, steps, reuse=None):
        """generate() on token ids: returns (tokens ring [pos+1], tok/s, timed_tokens, seconds). reuse=True: the steps of the prompt's common prefix with
        what this model ran last are skipped, their K / V rows reused in place (common_prefix); reuse=<Snapshot>: the snapshot is restored first and the
        run starts at the common prefix of the prompt and the snapshot's tokens. timed_tokens then counts the steps that ran."""
        t = np.ascontiguousarray(prompt_tokens, dtype=np.int32)
        if reuse is None or reuse is False:
            return self.generate_ids_from(t, steps, 0)
        if reuse is True:
            return self.generate_ids_from(t, steps, self.common_prefix(t))
        self.restore(reuse)
        n = min(reuse.n_pos, t.shape[0] - 1)
        differ = np.nonzero(reuse.tokens[:n] != t[:n])[0]
        return self.generate_ids_from(t, steps, int(differ[0]) if differ.size else n)

    def generate_ids_from(self, prompt_tokens, steps, start_pos):
        """q4_generate_ids_from: generate_ids over K / V rows [0, start_pos) that are already in place (computed from prompt_tokens[:start_pos])."""
        t = np.ascontiguousarray(prompt_tokens, dtype=np.int32)
        limit = MAX_SEQ_LEN - 1 if self.context_shift()[1] > 0 else self.config.seq_len      # (a model that shifts generates past seq_len)
        if steps <= 0:                                          # the C side clamps the same way (llama2_q4.cu:690)
            steps = self.config.seq_len
        steps = min(steps, limit)
        out = np.zeros(steps + 2, dtype=np.int32)
        timed = C.c_int()
        secs = C.c_double()
        L = lib()
        if start_pos == 0:
            tps = L.q4_generate_ids(self.h, self.sampler, t.ctypes.data, t.shape[0], steps, out.ctypes.data, C.byref(timed), C.byref(secs))
        else:
            tps = L.q4_generate_ids_from(self.h, self.sampler, t.ctypes.data, t.shape[0], steps, int(start_pos), out.ctypes.data, C.byref(timed),
                                         C.byref(secs))
        if tps < 0:
            raise Q4Error("generate failed: " + L.q4_last_error().decode())
        return out[: self.pos_after(timed.value, start_pos, t) + 1], tps, timed.value, secs.value

    @staticmethod
    def pos_after(timed, start_pos, prompt):
        """the loop's final position from timed_tokens = pos - 1 - start (a prefix with an EOS inside runs from 0: q4_generate_ids_from)"""
        start = 0 if start_pos > 1 and (np.asarray(prompt[1:start_pos]) == 2).any() else start_pos
        return timed + 1 + start

    def resume(self, tokens, start_pos):
        """q4_resume_sequence: reset() that starts at start_pos over the K / V rows already there (computed from tokens[:start_pos])"""
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        check(lib().q4_resume_sequence(self.state, t.ctypes.data, t.shape[0], int(start_pos)))

    def common_prefix(self, tokens):
        """q4_common_prefix: the largest start_pos that is safe for `tokens` as the model stands; synchronises"""
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        n = lib().q4_common_prefix(self.h, t.ctypes.data, t.shape[0])
        if n < 0:
            check(-n)
        return n

    def set_context_shift(self, n_keep, n_discard):
        """q4_set_context_shift: generate_ids (and the library's other token loops) then shift at seq_len instead of stopping -- keep the first n_keep
        positions, discard the n_discard behind them, slide the rest down -- and `steps` may pass seq_len. n_discard = 0: off."""
        check(lib().q4_set_context_shift(self.h, int(n_keep), int(n_discard)))

    def context_shift(self):
        """(n_keep, n_discard) of the setting; n_discard 0: off"""
        L = lib()
        if not hasattr(L, "q4_get_context_shift"):             # (older builds under tools/ab.py do not have it)
            return 0, 0
        k, d = C.c_int(), C.c_int()
        check(L.q4_get_context_shift(self.h, C.byref(k), C.byref(d)))
        return k.value, d.value

    def shift_context(self, n_keep, n_discard, n_pos=None, n_ring=None):
        """q4_shift_context: K / V rows, ring tokens, guide states and log-probability records of positions [n_keep + n_discard, n_pos) move down by
        n_discard, the K rows rotated by as many positions, in place; the position becomes n_pos - n_discard. n_pos None: every completed position;
        n_ring None: n_pos + 1 (the ring up to the token the last step chose). The rows then hold what was computed with the discarded tokens in view:
        not what ingesting the surviving tokens would give. Synchronises."""
        if n_pos is None:
            check(lib().q4_stream_synchronize())
            n_pos = min(self.pos(), self.config.seq_len)
        check(lib().q4_shift_context(self.h, int(n_pos), int(n_keep), int(n_discard), int(n_pos + 1 if n_ring is None else n_ring)))

    @property
    def rope_scaling(self):
        """the model's RoPE scaling (q4_rope_scaling_of) in Hugging Face's spelling, dict(kind="custom", inv_freq=...) for custom frequencies, None for
        an unscaled model"""
        L = lib()
        if not hasattr(L, "q4_rope_scaling_of"):               # (older builds under tools/ab.py do not have it)
            return None
        r = RopeScaling()
        check(L.q4_rope_scaling_of(self.h, C.byref(r)))
        if r.kind == ROPE_CUSTOM:
            return {"kind": "custom", "inv_freq": self.rope_inv_freq()}
        return r.as_dict()

    def rope_inv_freq(self):
        """q4_get_rope_inv_freq: the head_size/2 float32 frequencies the model's rotation table was built from; Q4Error for an unscaled model (its
        table comes from rope_theta: it has no frequency array)"""
        out = np.empty(self.config.dim // self.config.n_heads // 2, dtype=np.float32)
        check(lib().q4_get_rope_inv_freq(self.h, out.ctypes.data))
        return out

    def rope_row(self, pos):
        """row `pos` of the model's rotation table: [head_size/2, 2] float32 (cos, sin); synchronises"""
        out = np.empty((self.config.dim // self.config.n_heads // 2, 2), dtype=np.float32)
        check(lib().q4_get_rope_row(self.h, int(pos), out.ctypes.data))
        return out

    def snapshot(self, n_pos=None):
        """q4_snapshot_new: a Snapshot of positions [0, n_pos); None: every position the device has completed"""
        if n_pos is None:
            check(lib().q4_stream_synchronize())
            n_pos = self.pos()
        h = C.c_void_p()
        check(lib().q4_snapshot_new(C.byref(h), self.h, int(n_pos)))
        return Snapshot(h.value)

    def restore(self, snap):
        """q4_snapshot_restore: the snapshot's rows back into positions [0, snap.n_pos), in stream order; the position does not move (follow with
        resume() or generate_ids_from())"""
        check(lib().q4_snapshot_restore(self.h, snap.h))

    def screen_candidates(self):
        """(last, max, total, steps) of the model's screened greedy steps (q4_screen_candidates); synchronises."""
        last, mx = C.c_int(), C.c_int()
        total, steps = C.c_longlong(), C.c_longlong()
        check(lib().q4_screen_candidates(self.h, C.byref(last), C.byref(mx), C.byref(total), C.byref(steps)))
        return last.value, mx.value, total.value, steps.value

    def set_speculative(self, draft=4, ngram=3, min=2, sampled=False):
        """q4_set_speculative: the token loops verify up to `draft` drafted tokens per pass over the weights (0: off); ngram / min: the longest and the
        shortest n-gram the built-in prompt-lookup drafter matches. Greedy runs, and with sampled=True (q4_set_speculative_sampled) runs under the
        temperature / top-p sampler too: every row is sampled with its own position's coin. The tokens are those of the run without it."""
        check(lib().q4_set_speculative(self.h, int(draft), int(ngram), int(min)))
        check(lib().q4_set_speculative_sampled(self.h, 1 if sampled else 0))

    def speculative_sampled(self):
        """q4_get_speculative_sampled: whether verify passes also run under the temperature / top-p sampler"""
        return bool(lib().q4_get_speculative_sampled(self.h))

    def verify_sampled(self, draft):
        """q4_verify_tokens_sampled at the current position under the model's sampler: (emitted tokens, n_accepted), or None where nothing ran. The
        sampler's stream must stand at the current position's coin; n_accepted + 1 coins of it are consumed."""
        d = np.ascontiguousarray(draft, dtype=np.int32)
        out = np.zeros(d.shape[0] + 1, dtype=np.int32)
        acc = C.c_int()
        rc = lib().q4_verify_tokens_sampled(self.h, self.sampler, d.ctypes.data, d.shape[0], out.ctypes.data, C.byref(acc))
        if rc == NOT_ADMITTED:
            return None
        check(rc)
        return out[: acc.value + 1].copy(), acc.value

    def verify_covers_sampled(self, pos, n_draft):
        return bool(lib().q4_verify_covers_sampled(self.h, self.sampler, int(pos), int(n_draft)))

    def speculative(self):
        d, g, m = C.c_int(), C.c_int(), C.c_int()
        check(lib().q4_get_speculative(self.h, C.byref(d), C.byref(g), C.byref(m)))
        return {"draft": d.value, "ngram": g.value, "min": m.value}

    def set_drafter(self, fn):
        """q4_set_drafter: fn(tokens, max_draft) -> ids, tokens the ring up to the current position's token as an int32 array (valid during the call only);
        None: the built-in drafter. Called from inside generate_ids; an exception inside it counts as no draft."""
        if fn is None:
            check(lib().q4_set_drafter(self.h, DRAFTER_FN(), None))
            self._drafter = None
            return

        def call(ctx, tokens, n_tokens, max_draft, out):
            try:
                ids = list(fn(np.ctypeslib.as_array(tokens, shape=(n_tokens,)), max_draft))[:max_draft]
            except Exception:
                return 0
            for k, v in enumerate(ids):
                out[k] = int(v)
            return len(ids)

        cb = DRAFTER_FN(call)
        check(lib().q4_set_drafter(self.h, cb, None))
        self._drafter = cb              # (keeps the callback alive while the model holds it)

    def verify(self, draft):
        """q4_verify_tokens at the current position: (emitted tokens, n_accepted) -- the n_accepted leading drafts the model confirms and the token
        behind them --, or None where a pass is not admitted and nothing ran (run steps instead)."""
        d = np.ascontiguousarray(draft, dtype=np.int32)
        out = np.zeros(d.shape[0] + 1, dtype=np.int32)
        acc = C.c_int()
        rc = lib().q4_verify_tokens(self.h, d.ctypes.data, d.shape[0], out.ctypes.data, C.byref(acc))
        if rc == NOT_ADMITTED:
            return None
        check(rc)
        return out[: acc.value + 1].copy(), acc.value

    def verify_covers(self, pos, n_draft):
        return bool(lib().q4_verify_covers(self.h, int(pos), int(n_draft)))

    def spec_stats(self):
        """(passes, drafted, accepted) of the model's verify passes (q4_spec_stats)"""
        a, b, c = C.c_longlong(), C.c_longlong(), C.c_longlong()
        check(lib().q4_spec_stats(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def set_sampling(self, **kw):
        """Sampling controls inside the decode step (q4_sampler_set_controls): top_k, min_p, repeat_penalty, presence_penalty, frequency_penalty,
        penalty_last_n; no keyword: off. They rewrite the logits of every generating step in front of the argmax / sampler."""
        check(lib().q4_sampler_set_controls(self.sampler, C.byref(SamplingControls(**kw)) if kw else None))

    def sampling(self):
        c = SamplingControls()
        check(lib().q4_sampler_get_controls(self.sampler, C.byref(c)))
        return c.as_dict()

    def set_logit_bias(self, logit_bias):
        """{token id: bias} added to the logits of every generating step (-inf bans a token); None or {}: cleared"""
        ids, bias = _bias_arrays(logit_bias)
        check(lib().q4_sampler_set_logit_bias(self.sampler, ids.ctypes.data, bias.ctypes.data, ids.shape[0]))

    def set_dry(self, **kw):
        """DRY and the no-repeat-n-gram ban inside the decode step (q4_sampler_set_dry): multiplier, base, allowed_length, last_n,
        no_repeat_ngram_size; no keyword: off. They rewrite the logits of every generating step behind the guide and in front of the sampling controls."""
        check(lib().q4_sampler_set_dry(self.sampler, C.byref(DryControls(**kw)) if kw else None))

    def dry(self):
        c = DryControls()
        check(lib().q4_sampler_get_dry(self.sampler, C.byref(c)))
        return c.as_dict()

    def set_dry_breakers(self, breakers, tokenizer=None):
        """the single-token sequence breakers of DRY: token ids, None or [] to clear, or "default" with a Tokenizer (dry_breaker_ids)"""
        if isinstance(breakers, str):
            if breakers != "default" or tokenizer is None:
                raise ValueError('dry_breakers: token ids, or "default" together with tokenizer=<Tokenizer>')
            breakers = dry_breaker_ids(tokenizer)
        ids = _breaker_array(breakers)
        check(lib().q4_sampler_set_dry_breakers(self.sampler, ids.ctypes.data, ids.shape[0]))

    def set_adaptive(self, **kw):
        """typical-p, top-n-sigma and Mirostat v2 inside the decode step (q4_sampler_set_adaptive): typical_p, top_n_sigma, mirostat_tau, mirostat_eta;
        no keyword: off. They mask the logits of every generating step behind the sampling controls and in front of the argmax / sampler."""
        check(lib().q4_sampler_set_adaptive(self.sampler, C.byref(AdaptiveControls(**kw)) if kw else None))

    def adaptive(self):
        c = AdaptiveControls()
        check(lib().q4_sampler_get_adaptive(self.sampler, C.byref(c)))
        return c.as_dict()

    def adaptive_records(self, first_pos, n):
        """the launch's records at positions first_pos .. first_pos + n - 1 as float32 [n, ADAPTIVE_RECORD] (adaptive_record reads a row); synchronises"""
        out = np.empty((n, ADAPTIVE_RECORD), dtype=np.float32)
        check(lib().q4_get_adaptive_records(self.h, first_pos, n, out.ctypes.data))
        return out

    def set_guide(self, guide):
        """Guided decoding (q4_set_guide): a Guide, or None for off. Every generating step then masks what the automaton's state forbids; the state
        is kept on the device by position and starts at 0 behind the prompt."""
        check(lib().q4_set_guide(self.h, guide.h if guide is not None else None))
        self._guide = guide             # (keeps the handle alive while the model holds it)

    def guide_states(self, first_pos, n):
        """the automaton's state at positions first_pos .. first_pos + n - 1 (GUIDE_NONE: no guided step ran there); synchronises"""
        out = np.empty(n, dtype=np.int32)
        check(lib().q4_get_guide_states(self.h, first_pos, n, out.ctypes.data))
        return out

    def set_logprobs(self, top_k):
        """Per-token log-probability records inside the decode step: None / -1 off, 0 the chosen or target token only, K <= 20 also the top K."""
        check(lib().q4_set_logprobs(self.h, -1 if top_k is None else int(top_k)))

    def set_pass_logprobs(self, on):
        """q4_set_pass_logprobs: prompt passes, verify passes and score_ids' passes also while the records are on (off by default: records keep the steps).
        Records, tokens, K / V rows and logits are the per-token run's, byte for byte."""
        check(lib().q4_set_pass_logprobs(self.h, 1 if on else 0))

    def pass_logprobs(self):
        """q4_get_pass_logprobs"""
        return bool(lib().q4_get_pass_logprobs(self.h))

    def set_pass_gqa(self, on):
        """q4_set_pass_gqa: prompt and verify passes also for the grouped-query 4096-wide shape (dim 4096, 128-wide heads, four query heads per K / V
        head, hidden 14336: Mistral-7B, Llama-3-8B); off by default. Tokens, K / V rows, logits and records are the per-token run's, byte for byte."""
        check(lib().q4_set_pass_gqa(self.h, 1 if on else 0))

    def pass_gqa(self):
        """q4_get_pass_gqa"""
        return bool(lib().q4_get_pass_gqa(self.h))

    def set_pass_kv8(self, on):
        """q4_set_pass_kv8: prompt and verify passes also for a model built with kv="fp8" (of a shape they admit with the fp16 cache); off by default"""
        check(lib().q4_set_pass_kv8(self.h, 1 if on else 0))

    def pass_kv8(self):
        """q4_get_pass_kv8"""
        return bool(lib().q4_get_pass_kv8(self.h))

    def set_pass_13b(self, on):
        """q4_set_pass_13b: prompt and verify passes also for Llama-2-13B's shape (dim 5120, forty 128-wide heads, multi-head, hidden 13824, fp16
        cache); off by default. Tokens, K / V rows, logits and records are the per-token run's, byte for byte."""
        check(lib().q4_set_pass_13b(self.h, 1 if on else 0))

    def pass_13b(self):
        """q4_get_pass_13b"""
        return bool(lib().q4_get_pass_13b(self.h))

    def set_pass_stages(self, on):
        """q4_set_pass_stages: verify passes also with a guide, DRY or the sampling controls on (their row forms), prompt passes also with a guide or the
        adaptive truncation on, and the guide's forced tokens as drafts in the token loop; off by default. Tokens, K / V rows, logits, rng_state and the
        guide's states below the position are the per-token run's, byte for byte."""
        check(lib().q4_set_pass_stages(self.h, 1 if on else 0))

    def pass_stages(self):
        """q4_get_pass_stages"""
        return bool(lib().q4_get_pass_stages(self.h))

    def spec_stats_forced(self):
        """(drafted, accepted) of the drafts the guide's forced run gave the token loop (q4_spec_stats_forced); they are part of spec_stats' totals"""
        a, b = C.c_longlong(), C.c_longlong()
        check(lib().q4_spec_stats_forced(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def logprobs_k(self):
        return lib().q4_get_logprobs_k(self.h)

    def logprobs(self, first_pos, n):
        """(token_logprob [n], top_ids [n, K], top_logprobs [n, K]) of records first_pos .. first_pos + n - 1; synchronises. Record p describes step p's
        logits and the token at ring index p + 1, under the model's own distribution (temperature 1, no nucleus)."""
        k = max(self.logprobs_k(), 0)
        tok = np.empty(n, dtype=np.float32)
        ids = np.empty((n, k), dtype=np.int32)
        top = np.empty((n, k), dtype=np.float32)
        check(lib().q4_get_logprobs(self.h, first_pos, n, tok.ctypes.data, ids.ctypes.data if k else None, top.ctypes.data if k else None))
        return tok, ids, top

    def score_ids(self, tokens_with_bos):
        """Teacher-forced log-probabilities of tokens_with_bos[1:] (no logits_array needed: works on a perplexity=False build)."""
        t = np.ascontiguousarray(tokens_with_bos, dtype=np.int32)
        out = np.empty(t.shape[0] - 1, dtype=np.float32)
        check(lib().q4_score_ids(self.h, self.sampler, t.ctypes.data, t.shape[0] - 1, out.ctypes.data))
        return out

    def perplexity_ids(self, tokens_with_bos):
        t = np.ascontiguousarray(tokens_with_bos, dtype=np.int32)
        return lib().q4_perplexity_ids(self.h, self.sampler, t.ctypes.data, t.shape[0] - 1)

    def bench_kernel(self, kernel_id, iters):
        mn = C.c_double()
        mx = C.c_double()
        avg = lib().q4_bench_kernel(kernel_id, C.byref(self.config), self.state, self.weights, iters, C.byref(mn), C.byref(mx))
        if avg < 0:
            raise Q4Error("bench_kernel failed: " + lib().q4_last_error().decode())
        return avg, mn.value, mx.value


    def bench_in_network(self, report_mask, tokens=8, time_mask=127):
        """(avg, min, max us, launches) of one launch class inside the eager decode network, from the current position."""
        mn = C.c_double()
        mx = C.c_double()
        n = C.c_int()
        avg = lib().q4_bench_in_network(time_mask, report_mask, C.byref(self.config), self.state, self.weights, tokens, C.byref(mn),
                                        C.byref(mx), C.byref(n))
        if avg < 0:
            raise Q4Error("bench_in_network failed: " + lib().q4_last_error().decode())
        return avg, mn.value, mx.value, n.value

    def bench_kernel_graph(self, kernel_id, iters=32, reps=20):
        us = lib().q4_bench_kernel_graph(kernel_id, C.byref(self.config), self.state, self.weights, iters, reps)
        if us < 0:
            raise Q4Error("bench_kernel_graph failed: " + lib().q4_last_error().decode())
        return us


BATCH_MAX_SLOTS = 8


class Batch:
    """q4_batch: up to BATCH_MAX_SLOTS sequences over one Transformer's weights, every open one advanced by one position per pass over the weights
    (csrc/q4_batch.h). A slot's tokens, K / V rows and logits are byte for byte those of the same checkpoint running that sequence alone with the slot's
    seed. The model's sampler decides greedy or temperature / top-p; its own sequence is not touched. delete() the batch before the Transformer closes."""

    def __init__(self, transformer, slots, prefill_rows=1):
        self.t = transformer
        self.slots = int(slots)
        h = C.c_void_p()
        check(lib().q4_batch_new(C.byref(h), transformer.h, self.slots))
        self.h = h.value
        if int(prefill_rows) != 1:
            self.set_prefill(prefill_rows)

    def set_prefill(self, n):
        """q4_batch_set_prefill: a slot inside its prompt takes up to `n` rows (consecutive positions) of a pass that has rows to spare; 1: one per slot"""
        check(lib().q4_batch_set_prefill(self.h, int(n)))

    def prefill(self):
        return lib().q4_batch_get_prefill(self.h)

    @staticmethod
    def plan_rows(open_, pos, n_prompt, max_rows_per_slot):
        """q4_batch_plan_rows, the schedule of one pass (host arithmetic, no device): (rows in the pass, int32 rows per slot)"""
        o, p, n = (np.ascontiguousarray(x, dtype=np.int32) for x in (open_, pos, n_prompt))
        rows = np.zeros(len(o), dtype=np.int32)
        total = lib().q4_batch_plan_rows(o.ctypes.data, p.ctypes.data, n.ctypes.data, len(o), int(max_rows_per_slot), rows.ctypes.data)
        if total < 0:
            check(-total)
        return total, rows

    def run(self, requests, max_new_tokens, eos=None, seeds=None):
        """A host loop over step(): `requests` (token lists) are opened in free slots in order as slots fall free, each generates until it emits `eos`
        (kept as its last token) or has max_new_tokens, then its slot is closed and the next request takes it. Returns each request's generated tokens in
        request order. ValueError, nothing opened: a seed list of another length, max_new_tokens below 1, an empty request or one that does not fit the
        context with its new tokens. Every slot of the batch must be closed going in (an open one: Q4Error from the first open that meets it). However
        the loop ends -- also on a pass that raises, e.g. a row where no row form exists -- the slots this call opened are closed again."""
        requests = [[int(x) for x in r] for r in requests]
        seeds = [1] * len(requests) if seeds is None else [int(s) for s in seeds]
        new = int(max_new_tokens)
        if len(seeds) != len(requests):
            raise ValueError("Batch.run: %d seeds for %d requests" % (len(seeds), len(requests)))
        if new < 1:
            raise ValueError("Batch.run: max_new_tokens must be at least 1")
        for r in requests:
            if not r or len(r) + new > self.t.config.seq_len + 1:
                raise ValueError("Batch.run: a request of %d tokens and %d new ones does not fit the context" % (len(r), new))
        out = [[] for _ in requests]
        owner = [None] * self.slots
        queued = 0
        try:
            while queued < len(requests) or any(o is not None for o in owner):
                for slot in range(self.slots):
                    if owner[slot] is None and queued < len(requests):
                        self.open(slot, requests[queued], seed=seeds[queued])
                        owner[slot] = queued
                        queued += 1
                toks = self.step()
                for slot, req in enumerate(owner):
                    if req is None or toks[slot] < 0:
                        continue
                    out[req].append(int(toks[slot]))
                    if len(out[req]) >= new or (eos is not None and int(toks[slot]) == int(eos)):
                        self.close(slot)
                        owner[slot] = None
        finally:
            for slot, req in enumerate(owner):
                if req is not None:
                    self.close(slot)
        return out

    @staticmethod
    def covers(transformer):
        return bool(lib().q4_batch_covers(transformer.h))

    def open(self, slot, prompt, seed=1):
        """q4_batch_open: the slot starts at position 0 on `prompt`; seed: its coin stream (Transformer(seed=...) of the run alone)"""
        p = np.ascontiguousarray(prompt, dtype=np.int32)
        check(lib().q4_batch_open(self.h, int(slot), p.ctypes.data, p.shape[0], int(seed)))

    def restore(self, slot, snap, prompt, seed=1):
        """q4_batch_restore: the slot starts at position snap.n_pos behind the snapshot's rows; `prompt` begins with the snapshot's tokens and is longer"""
        p = np.ascontiguousarray(prompt, dtype=np.int32)
        check(lib().q4_batch_restore(self.h, int(slot), snap.h, p.ctypes.data, p.shape[0], int(seed)))

    def step(self):
        """q4_batch_step: one pass; int32 [BATCH_MAX_SLOTS], the generated token per slot or -1 (closed, or still inside its prompt)"""
        out = np.empty(BATCH_MAX_SLOTS, dtype=np.int32)
        check(lib().q4_batch_step(self.h, self.t.sampler, out.ctypes.data))
        return out

    def generate(self, steps):
        """q4_batch_generate: up to `steps` passes queued back to back, one synchronise; int32 [passes run, BATCH_MAX_SLOTS]"""
        out = np.empty((int(steps), BATCH_MAX_SLOTS), dtype=np.int32)
        n = C.c_int()
        check(lib().q4_batch_generate(self.h, self.t.sampler, int(steps), out.ctypes.data, C.byref(n)))
        return out[: n.value]

    def pos(self, slot):
        n = lib().q4_batch_pos(self.h, int(slot))
        if n < 0:
            check(-n)
        return n

    def logits(self, slot):
        out = np.empty(self.t.config.vocab_size, dtype=np.float16)
        check(lib().q4_batch_get_logits(self.h, int(slot), out.ctypes.data))
        return out

    def kv_row(self, slot, layer, pos):
        cfg = self.t.config
        kv_dim = cfg.dim * cfg.n_kv_heads // cfg.n_heads
        k = np.empty(kv_dim, dtype=np.float16)
        v = np.empty(kv_dim, dtype=np.float16)
        check(lib().q4_batch_get_kv_row(self.h, int(slot), int(layer), int(pos), k.ctypes.data, v.ctypes.data))
        return k, v

    def cache(self, slot):
        """(key_cache, value_cache) device addresses of the slot's caches, each [n_layers][seq_len][kv_dim] halves"""
        k, v = C.c_void_p(), C.c_void_p()
        check(lib().q4_batch_cache(self.h, int(slot), C.byref(k), C.byref(v)))
        return k.value, v.value

    def close(self, slot):
        """q4_batch_close: the slot's rows and logits stay readable until it is opened again"""
        check(lib().q4_batch_close(self.h, int(slot)))

    def delete(self):
        """q4_batch_delete: the whole batch, every slot's cache with it"""
        if getattr(self, "h", None):
            check(lib().q4_batch_delete(self.h))
            self.h = None

    def __del__(self):
        try:
            self.delete()
        except Exception:
            pass


class Tokenizer:
    def __init__(self, path, vocab_size):
        self.h = lib().q4_tokenizer_new(path.encode(), vocab_size)
        self.vocab_size = vocab_size
        if not self.h:
            raise Q4Error("couldn't load %s" % path)

    def encode(self, text, bos=1, eos=0):
        b = text.encode("utf-8") if isinstance(text, str) else text
        toks = np.zeros(len(b) + 3, dtype=np.int32)
        n = C.c_int()
        check(lib().q4_tokenizer_encode(self.h, b, bos, eos, toks.ctypes.data, C.byref(n)))
        return toks[: n.value].tolist()

    def decode(self, prev, tok):
        return lib().q4_tokenizer_decode(self.h, prev, tok)

    def piece(self, tok):
        """the raw bytes of a vocabulary entry, as the file holds them (q4_tokenizer_piece)"""
        p, n = C.c_void_p(), C.c_int()
        check(lib().q4_tokenizer_piece(self.h, int(tok), C.byref(p), C.byref(n)))
        return C.string_at(p.value, n.value) if n.value else b""

    def pieces(self):
        return [self.piece(i) for i in range(self.vocab_size)]

    def close(self):
        if self.h:
            lib().q4_tokenizer_delete(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
