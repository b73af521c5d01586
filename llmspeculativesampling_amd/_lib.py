"""ctypes binding of libspecdec.so (the C ABI declared in include/specdec.h).

There is no CPU fallback: if the shared object is missing or fails to load the
import raises, and every entry point converts a negative sd_status into the
Python exception the reference raises at the same place (Errors).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SD_LIBSPECDEC") or os.path.join(_HERE, "libspecdec.so")   # (override: kernel-variant experiments)

SD_OK, SD_ERR_INVALID, SD_ERR_NORM_LOGITS, SD_ERR_PROB, SD_ERR_HIP, SD_ERR_CAPACITY = 0, -1, -2, -3, -4, -5
SD_F32, SD_BF16, SD_F16 = 0, 1, 2
SD_W12_QKV, SD_W12_GATE_UP, SD_W12_DOWN = 0, 1, 2          # matrices sd_model_set_w12 takes 12-bit records for
SD_NORM_ROUND_BF16, SD_NORM_ROUND_F16, SD_NORM_DT_BF16, SD_NORM_DT_F16 = 1, 2, 16, 32
N_PROFILE_CLASSES = 8
PROFILE_CLASS_NAMES = ["gemm", "attention", "norm_residual", "qkv_rope_append", "activation", "embed",
                       "logits", "other"]


class SdAcceptResult(C.Structure):
    _fields_ = [("n_accepted", C.c_int32), ("n", C.c_int32), ("next_token", C.c_int32), ("flags", C.c_int32),
                ("p_at", C.c_float * 16), ("q_at", C.c_float * 16), ("drafted", C.c_int32 * 16)]


class SdNormRow(C.Structure):
    _fields_ = [("probs_out", C.c_void_p), ("err", C.c_void_p), ("exp_noise", C.c_void_p), ("philox_seed", C.c_uint64),
                ("draw_index", C.c_uint64), ("tok_out", C.c_void_p), ("sample_err", C.c_void_p)]


class SdRowSampling(C.Structure):
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float)]


class SdAcceptItem(C.Structure):
    _fields_ = [("p_hist", C.c_void_p), ("q_hist", C.c_void_p), ("seq", C.c_void_p), ("L", C.c_int32),
                ("r", C.c_void_p), ("exp_noise", C.c_void_p), ("philox_seed", C.c_uint64), ("draw_scan", C.c_uint64),
                ("draw_resample", C.c_uint64), ("res", C.c_void_p), ("err_flags", C.c_void_p), ("n_err", C.c_int32)]


class SdMultiResult(C.Structure):
    _fields_ = [("chosen", SdAcceptResult), ("choice", C.c_int32), ("n_uniform", C.c_int32), ("width", C.c_int32),
                ("gamma", C.c_int32), ("p_at", C.c_float * 256), ("q_at", C.c_float * 256)]


class SdMultiItem(C.Structure):
    _fields_ = [("p_hist", C.c_void_p), ("q_hist", C.c_void_p), ("seq", C.c_void_p)]


class SdMultiAdoptItem(C.Structure):
    _fields_ = [("draft_kv", C.c_void_p), ("target_kv", C.c_void_p), ("seq", C.c_void_p)]


class SdMultiReplica(C.Structure):
    _fields_ = [("draft", C.c_void_p), ("target", C.c_void_p), ("seq", C.c_void_p), ("q_hist", C.c_void_p),
                ("p_hist", C.c_void_p)]


class SdBatchStream(C.Structure):
    _fields_ = [("draft", C.c_void_p), ("target", C.c_void_p), ("seq", C.c_void_p), ("q_hist", C.c_void_p),
                ("p_hist", C.c_void_p), ("err_words", C.c_void_p), ("res_dev", C.c_void_p), ("res_host", C.c_void_p),
                ("host_seq", C.c_void_p), ("len", C.c_int32), ("T", C.c_int32), ("ori_eos_cnt", C.c_int32),
                ("draft_len", C.c_int32), ("target_len", C.c_int32), ("seed", C.c_uint64), ("draw", C.c_uint64),
                ("done", C.c_int32), ("calls", C.c_int32), ("acc_len_out", C.c_void_p), ("p_at_out", C.c_void_p),
                ("q_at_out", C.c_void_p)]


class SdQueuePrompt(C.Structure):
    _fields_ = [("tokens", C.c_void_p), ("L", C.c_int32), ("T", C.c_int32), ("ori_eos_cnt", C.c_int32), ("seed", C.c_uint64),
                ("host_seq", C.c_void_p), ("acc_len_out", C.c_void_p), ("p_at_out", C.c_void_p), ("q_at_out", C.c_void_p),
                ("len", C.c_int32), ("calls", C.c_int32), ("admit_iter", C.c_int32), ("finish_iter", C.c_int32)]


class SdQueuePass(C.Structure):
    _fields_ = [("act0", C.c_int32), ("n_act", C.c_int32), ("chunk0", C.c_int32), ("n_chunks", C.c_int32)]


class SdQueueChunk(C.Structure):
    _fields_ = [("joiner", C.c_int32), ("row0", C.c_int32), ("rows", C.c_int32)]


class SdKvCopyItem(C.Structure):
    _fields_ = [("dst", C.c_void_p), ("lo", C.c_int32), ("hi", C.c_int32)]


class SdArStream(C.Structure):
    _fields_ = [("session", C.c_void_p), ("seq", C.c_void_p), ("probs", C.c_void_p), ("err_words", C.c_void_p),
                ("host_seq", C.c_void_p), ("len", C.c_int32), ("T", C.c_int32), ("cache_len", C.c_int32),
                ("seed", C.c_uint64), ("draw", C.c_uint64), ("done", C.c_int32), ("steps", C.c_int32)]


class SdSampling(C.Structure):
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float), ("V", C.c_int32), ("ld", C.c_long),
                ("eos_token_id", C.c_int32)]


class SdHeadScratch(C.Structure):
    _fields_ = [("logits", C.c_void_p), ("ld_logits", C.c_long), ("norm_mode", C.c_int32)]


class SdSpecStream(C.Structure):
    _fields_ = SdBatchStream._fields_[:8]                  # the device side of one stream, as sd_batch_stream starts


class SdSpecScratch(C.Structure):
    _fields_ = [("draft", SdHeadScratch), ("target", SdHeadScratch), ("norm_workspace", C.c_void_p),
                ("max_rows_per_forward", C.c_int32)]


class SdLockstepLog(C.Structure):
    _fields_ = [("verify_ms_out", C.c_void_p), ("verify_streams_out", C.c_void_p), ("verify_ctx_out", C.c_void_p),
                ("max_iters_log", C.c_int32), ("n_iters", C.c_int32), ("err", C.c_int32)]


class SdSeqState(C.Structure):
    _fields_ = [("host_seq", C.c_void_p), ("len", C.c_int32), ("T", C.c_int32), ("ori_eos_cnt", C.c_int32),
                ("draft_len", C.c_int32), ("target_len", C.c_int32), ("seed", C.c_uint64), ("draw", C.c_uint64),
                ("max_iters", C.c_int32), ("acc_len_out", C.c_void_p), ("p_at_out", C.c_void_p), ("q_at_out", C.c_void_p),
                ("draft_ms_out", C.c_void_p), ("target_ms_out", C.c_void_p), ("n_iters", C.c_int32), ("err", C.c_int32)]


class SdArLog(C.Structure):
    _fields_ = [("step_ms_out", C.c_void_p), ("step_streams_out", C.c_void_p), ("max_steps_log", C.c_int32),
                ("n_steps", C.c_int32), ("err", C.c_int32)]


class SdLogprobItem(C.Structure):
    _fields_ = [("logits", C.c_void_p), ("ld", C.c_long), ("rows", C.c_int32), ("tokens", C.c_void_p), ("res", C.c_void_p),
                ("out", C.c_void_p)]


class SdLogprobBlock(C.Structure):
    _fields_ = [("dev", C.c_void_p), ("host", C.c_void_p), ("logprob_out", C.POINTER(C.c_void_p))]


class SdScoreItem(C.Structure):
    _fields_ = [("logits", C.c_void_p), ("ld", C.c_long), ("rows", C.c_int32), ("tokens", C.c_void_p), ("logprob", C.c_void_p),
                ("rank", C.c_void_p), ("top_ids", C.c_void_p), ("top_logprobs", C.c_void_p)]


class SdScoreOut(C.Structure):
    _fields_ = [("logprob", C.c_void_p), ("rank", C.c_void_p), ("top_ids", C.c_void_p), ("top_logprobs", C.c_void_p)]


SD_SCORE_MAX_TOP, SD_SCORE_MAX_ROWS = 20, 80             # sd_score_rows: top_n and rows per item


class SdPenalty(C.Structure):
    _fields_ = [("repetition", C.c_float), ("frequency", C.c_float), ("presence", C.c_float)]


class SdPenaltyItem(C.Structure):
    _fields_ = [("in", C.c_void_p), ("out", C.c_void_p), ("ld_in", C.c_long), ("ld_out", C.c_long), ("rows", C.c_int32),
                ("seq", C.c_void_p), ("hist0", C.c_int32), ("prompt_len", C.c_int32), ("pen", SdPenalty)]


class SdPenaltyBlock(C.Structure):
    _fields_ = [("rows", C.c_void_p), ("ld", C.c_long), ("max_rows", C.c_int32), ("params", C.POINTER(SdPenalty))]


class SdLogitEdit(C.Structure):
    _fields_ = [("bias_ids", C.c_void_p), ("bias_vals", C.c_void_p), ("n_bias", C.c_int32), ("allowed", C.c_void_p),
                ("min_tokens", C.c_int32)]


class SdLogitEditItem(C.Structure):
    _fields_ = SdPenaltyItem._fields_ + [("edit", SdLogitEdit), ("eos_token_id", C.c_int32)]


class SdLogitEditBlock(C.Structure):
    _fields_ = [("rows", C.c_void_p), ("ld", C.c_long), ("max_rows", C.c_int32), ("params", C.POINTER(SdLogitEdit))]


class SdLoopOpts(C.Structure):                          # the loops' optional last argument; every member may be NULL
    _fields_ = [("row_params", C.POINTER(SdRowSampling)), ("logprobs", C.POINTER(SdLogprobBlock)),
                ("penalties", C.POINTER(SdPenaltyBlock)), ("edits", C.POINTER(SdLogitEditBlock))]


class SdGrammar(C.Structure):                            # a token automaton; device tables, caller-owned
    _fields_ = [("masks", C.c_void_p), ("next", C.c_void_p), ("cls", C.c_void_p), ("n_states", C.c_int32), ("n_classes", C.c_int32),
                ("start", C.c_int32)]


class SdGrammarItem(C.Structure):                        # one item of sd_grammar_rows: sd_edit_rows' item, the grammar, the state cache
    _fields_ = [("row", SdLogitEditItem), ("grammar", C.POINTER(SdGrammar)), ("states", C.c_void_p)]


class SdLookupItem(C.Structure):                         # one stream of sd_lookup_propose
    _fields_ = [("seq", C.c_void_p), ("L", C.c_int32), ("q_hist", C.c_void_p), ("info", C.c_void_p)]


SD_EDIT_MAX_BIAS = 1024                                  # bias entries per request
SD_LOOKUP_MAX_NGRAM = 8                                  # the longest key the prompt-lookup proposer matches
LOGPROB_SLICE, LOGPROB_STREAMS = 17, 16                  # sd_logprob_block: 16 streams x 17 floats, device and pinned host


class SdBatchItem(C.Structure):
    _fields_ = [("session", C.c_void_p), ("seq", C.c_void_p), ("pos0", C.c_int32), ("n_new", C.c_int32),
                ("n_logits", C.c_int32)]


class SdModelConfig(C.Structure):
    _fields_ = [("arch", C.c_int32), ("dtype", C.c_int32), ("vocab", C.c_int32), ("hidden", C.c_int32),
                ("inter", C.c_int32), ("n_layers", C.c_int32), ("n_heads", C.c_int32), ("n_kv_heads", C.c_int32),
                ("head_dim", C.c_int32), ("max_pos", C.c_int32), ("opt_pre_ln", C.c_int32),
                ("opt_proj_dim", C.c_int32), ("norm_eps", C.c_float), ("logits_bf16_round", C.c_int32),
                ("fused_layout", C.c_int32)]


SD_GN_GATHER, SD_GN_ROWMAJOR, SD_GN_FUSED, SD_GN_QKV, SD_GN_ONE_SLAB = 1, 2, 4, 8, 16      # what a GEMM call needs of its route
SD_GEMM_NONE, SD_GEMM_STREAM, SD_GEMM_STREAM_W16, SD_GEMM_ROWS, SD_GEMM_MM = 0, 1, 2, 3, 4


class SdGemmRouteInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("kind", "S", "ksp", "mtw", "NG", "grid", "nwn", "nwk", "nld", "inst_mt", "inst_ntw",
                                         "inst_unroll", "inst_ch", "inst_wbm", "inst_nt", "lds_bytes")] + [("part_floats", C.c_uint64)]


_VP = C.c_void_p
_VPP = C.POINTER(C.c_void_p)


class SdModelWeights(C.Structure):
    _fields_ = [("embed", _VP), ("pos_embed", _VP), ("project_in", _VP), ("project_out", _VP),
                ("final_norm_w", _VP), ("final_norm_b", _VP), ("lm_head", _VP), ("rope_cos", _VP), ("rope_sin", _VP),
                ("wqkv", _VPP), ("bqkv", _VPP), ("wo", _VPP), ("bo", _VPP), ("w_gate_up", _VPP), ("b_fc1", _VPP),
                ("w_down", _VPP), ("b_fc2", _VPP), ("norm1_w", _VPP), ("norm1_b", _VPP), ("norm2_w", _VPP),
                ("norm2_b", _VPP)]


# every struct include/specdec.h declares, by its C name
C_STRUCTS = {"sd_accept_result": SdAcceptResult, "sd_norm_row": SdNormRow, "sd_row_sampling": SdRowSampling,
             "sd_accept_item": SdAcceptItem,
             "sd_multi_result": SdMultiResult, "sd_multi_item": SdMultiItem, "sd_multi_adopt_item": SdMultiAdoptItem,
             "sd_multi_replica": SdMultiReplica, "sd_batch_stream": SdBatchStream, "sd_queue_prompt": SdQueuePrompt,
             "sd_queue_pass": SdQueuePass, "sd_queue_chunk": SdQueueChunk, "sd_kv_copy_item": SdKvCopyItem,
             "sd_ar_stream": SdArStream, "sd_sampling": SdSampling, "sd_head_scratch": SdHeadScratch,
             "sd_spec_stream": SdSpecStream, "sd_spec_scratch": SdSpecScratch, "sd_lockstep_log": SdLockstepLog, "sd_seq_state": SdSeqState,
             "sd_ar_log": SdArLog, "sd_batch_item": SdBatchItem,
             "sd_logprob_item": SdLogprobItem, "sd_logprob_block": SdLogprobBlock, "sd_score_item": SdScoreItem,
             "sd_score_out": SdScoreOut, "sd_penalty": SdPenalty,
             "sd_penalty_item": SdPenaltyItem, "sd_penalty_block": SdPenaltyBlock, "sd_logit_edit": SdLogitEdit,
             "sd_logit_edit_item": SdLogitEditItem, "sd_logit_edit_block": SdLogitEditBlock, "sd_loop_opts": SdLoopOpts,
             "sd_lookup_item": SdLookupItem, "sd_grammar": SdGrammar, "sd_grammar_item": SdGrammarItem,
             "sd_model_config": SdModelConfig,
             "sd_gemm_route_info": SdGemmRouteInfo, "sd_model_weights": SdModelWeights}

# every symbol include/specdec.h declares: (name, restype, argtypes)
_F, _I, _L, _U64 = C.c_float, C.c_int, C.c_long, C.c_uint64
_P = C.POINTER
SYMBOLS = [
    ("sd_version", _I, []),
    ("sd_last_error", C.c_char_p, []),
    ("sd_norm_probs", _I, [_VP, _I, _I, _L, _F, _I, _F, _I, _VP, _L, _VP, _VP, _VP]),
    ("sd_topk_topp_filter", _I, [_VP, _I, _I, _L, _I, _F, _I, _VP, _L, _VP]),
    ("sd_norm_workspace_bytes", C.c_size_t, [_I]),
    ("sd_norm_sample", _I, [_VP, _I, _F, _I, _F, _I, _VP, _VP, _VP, _U64, _U64, _VP, _VP, _VP, _VP]),
    ("sd_norm_batch", _I, [_VP, _I, _I, _L, _F, _I, _F, _I, C.POINTER(SdNormRow), _I, _VP, _VP]),
    ("sd_norm_batch_rows", _I, [_VP, _I, _I, _L, C.POINTER(SdRowSampling), _I, C.POINTER(SdNormRow), _I, _VP, _VP]),
    ("sd_norm_batch_rows_debug", _I, [_VP, _I, _I, _L, C.POINTER(SdRowSampling), _I, C.POINTER(SdNormRow), _I, _VP, _VP, _VP, _VP,
                                      _VP]),                                 # test hook
    ("sd_accept_batch", _I, [C.POINTER(SdAcceptItem), _I, _L, _I, _I, _I, _VP]),
    ("sd_accept_multi", _I, [C.POINTER(SdMultiItem), _I, _L, _I, _I, _VP, _U64, _U64, _VP, _VP]),
    ("sd_multi_resample", _I, [_VP, _VP, _L, _I, _VP, _I, _VP, _U64, _U64, _VP, _I, _VP]),
    ("sd_multi_accept_resample", _I, [C.POINTER(SdMultiItem), _I, _L, _I, _I, _I, _VP, _U64, _U64, _U64, _VP, _I, _VP]),   # internal
    ("sd_multi_adopt", _I, [C.POINTER(SdMultiAdoptItem), _I, _VP, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _VP]),
    ("sd_spec_multi_block_bytes", C.c_size_t, [_I, _I]),
    ("sd_spec_multi_generate", _I, [_P(SdMultiReplica), _I, _I, _I, _P(SdSampling), _U64, _VP, _P(SdSpecScratch), _VP, _VP,
                                    _P(SdSeqState), _VP]),
    ("sd_sample", _I, [_VP, _I, _VP, _U64, _U64, _VP, _VP, _I, _VP]),
    ("sd_philox_exp", _I, [_U64, _U64, _I, _VP, _VP]),
    ("sd_philox_uniform", _I, [_U64, _U64, _I, _VP, _VP]),
    ("sd_max_fn", _I, [_VP, _VP, _I, _VP, _I, _VP]),
    ("sd_accept_scan", _I, [_VP, _VP, _L, _VP, _I, _I, _VP, _U64, _U64, _VP, _VP]),
    ("sd_resample", _I, [_VP, _VP, _L, _I, _VP, _I, _I, _VP, _U64, _U64, _VP, _VP, _I, _VP]),
    ("sd_model_create", _I, [C.POINTER(SdModelConfig), C.POINTER(SdModelWeights), C.POINTER(_VP)]),
    ("sd_model_destroy", _I, [_VP]),
    ("sd_model_max_rows", _I, [_VP]),
    ("sd_model_max_pass_rows", _I, [_VP]),
    ("sd_pack_weight_bf16", _I, [_VP, _VP, _I, _I, _VP]),
    ("sd_w12_bytes", _I, [_I, _I, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    ("sd_pack_weight_w12", _I, [_VP, _VP, _VP, _I, _I, _VP, _VP]),
    ("sd_unpack_weight_w12", _I, [_VP, _VP, _VP, _I, _I, _VP]),
    ("sd_model_set_w12", _I, [_VP, _I, _I, _VP, _VP]),
    ("sd_session_w12_launches", _I, [_VP]),
    ("sd_pack_activation_bf16", _I, [_VP, _VP, _I, _I, _VP]),
    ("sd_gemm_bf16", _I, [_VP, _VP, _I, _I, _I, _I, _VP, C.c_size_t, _VP, C.POINTER(C.c_int), _VP]),
    ("sd_gemm_route", _I, [_I, _I, _I, _I, C.POINTER(SdGemmRouteInfo)]),
    ("sd_gemm_bf16_need", _I, [_VP, _VP, _I, _I, _I, _I, _VP, C.c_size_t, _VP, C.POINTER(C.c_int), _VP]),
    ("sd_session_kv_bytes", C.c_size_t, [_VP, _I]),
    ("sd_session_scratch_bytes", C.c_size_t, [_VP, _I]),
    ("sd_session_part_floats", C.c_size_t, [_VP, _I]),
    ("sd_session_create", _I, [_VP, _I, _I, _VP, _VP, C.POINTER(_VP)]),
    ("sd_session_destroy", _I, [_VP]),
    ("sd_session_set_kv_fp8", _I, [_VP, _VP]),
    ("sd_session_prefill_attn_launches", _I, [_VP]),
    ("sd_session_prefill_attn_blocked_launches", _I, [_VP]),
    ("sd_prefill_attn_plan", _I, [_I, _I, _I, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_long)]),
    ("sd_prefill_attn_route", _I, [_I, _I, _I, _I, _I, _I, C.POINTER(C.c_int)]),
    ("sd_session_forward", _I, [_VP, _VP, _I, _I, _I, _VP, _L, _VP]),
    ("sd_session_forward_tree", _I, [_VP, _VP, C.POINTER(C.c_int32), C.POINTER(C.c_uint64), _I, _I, _VP, _L, _VP]),
    ("sd_session_compact_kv", _I, [_VP, _I, _VP, _I, _VP]),
    ("sd_session_fused_status", _I, [_VP, _VP]),
    ("sd_session_test_skew_wait", _I, [_VP, _I]),
    ("sd_session_ao_stamps", _I, [_VP, _VP, _I]),
    ("sd_cand_list_bytes", C.c_size_t, [_I]),
    ("sd_norm_probs_lists", _I, [_VP, _I, _I, _L, _F, _I, _F, _I, _VP, _L, _VP, _VP, _VP, _VP]),
    ("sd_accept_resample", _I, [_VP, _VP, _L, _I, _VP, _I, _I, _VP, _U64, _U64, _U64, _VP, _VP, _I, _I, _VP, _VP]),
    ("sd_norm_probs_debug", _I, [_VP, _I, _I, _L, _F, _I, _F, _I, _VP, _L, _VP, _VP, _VP, _VP, _VP, _I, _I, _VP, _U64, _U64,
                                 _VP, _VP, _VP]),                                     # test hook
    ("sd_accept_resample_batch", _I, [C.POINTER(SdAcceptItem), _I, _L, _I, _I, _I, _VPP, _VP]),   # internal
    ("sd_spec_batch_generate", _I, [_P(SdBatchStream), _I, _I, _P(SdSampling), _U64, _VP, _P(SdSpecScratch), _P(SdLockstepLog), _VP,
                                    _P(SdLoopOpts)]),
    ("sd_spec_queue_generate", _I, [_P(SdBatchStream), _I, _I, _P(SdQueuePrompt), _I, _I, _I, _P(SdSampling), _U64, _VP,
                                    _P(SdSpecScratch), _P(SdLockstepLog), _VP, _VP, _VP, _VP, _I, _P(SdLoopOpts)]),
    ("sd_session_copy_kv", _I, [_VP, C.POINTER(SdKvCopyItem), _I, _VP]),
    ("sd_spec_queue_plan", _I, [_I, _I, C.POINTER(C.c_int32), _I, _I, C.POINTER(C.c_int32), _I, _I, _I, C.POINTER(SdQueuePass), _I,
                                C.POINTER(SdQueueChunk), _I, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("sd_spec_generate", _I, [_P(SdSpecStream), _I, _P(SdSampling), _P(SdSpecScratch), _P(SdSeqState), _U64, _VP, _VP,
                              _P(SdLoopOpts)]),
    ("sd_ar_block_bytes", C.c_size_t, [_I]),
    ("sd_ar_batch_generate", _I, [_P(SdArStream), _I, _P(SdSampling), _P(SdHeadScratch), _VP, _VP, _VP, _P(SdArLog), _VP,
                                  _P(SdLoopOpts)]),
    ("sd_token_logprobs", _I, [_P(SdLogprobItem), _I, _I, _I, _VP]),
    ("sd_score_rows", _I, [_P(SdScoreItem), _I, _I, _I, _I, _VP]),
    ("sd_score_sequence", _I, [_VP, _VP, _I, _I, _I, _VP, _L, _I, _P(SdScoreOut), _VP]),
    ("sd_penalize_rows", _I, [_P(SdPenaltyItem), _I, _I, _I, _VP]),
    ("sd_edit_rows", _I, [_P(SdLogitEditItem), _I, _I, _I, _VP]),
    ("sd_session_set_grammar", _I, [_VP, _P(SdGrammar), _VP, C.c_int32]),
    ("sd_grammar_rows", _I, [_P(SdGrammarItem), _I, _I, _I, _VP]),
    ("sd_lookup_propose", _I, [_P(SdLookupItem), _I, _I, _L, _I, _I, _I, _VP]),
    ("sd_lookup_generate", _I, [_P(SdSpecStream), _I, _I, _I, _P(SdSampling), _P(SdSpecScratch), _P(SdSeqState), _VP, _VP]),
    ("sd_lookup_batch_generate", _I, [_P(SdBatchStream), _I, _I, _I, _I, _P(SdSampling), _P(SdSpecScratch), _P(SdLockstepLog), _VPP,
                                      _VP]),
    ("sd_batch_forward", _I, [C.POINTER(SdBatchItem), _I, _VP, _L, _VP]),
    ("sd_batch_prefill", _I, [C.POINTER(SdBatchItem), _I, _VP]),
    ("sd_tp_unique_id", _I, [_VP]),
    ("sd_tp_create_rccl", _I, [_I, _I, _VP, C.POINTER(_VP)]),
    ("sd_tp_create_loopback", _I, [_I, C.POINTER(_VP)]),
    ("sd_tp_destroy", _I, [_VP]),
    ("sd_session_set_tp", _I, [_VP, _VP]),
    ("sd_comm_probe", _I, []),
    ("sd_comm_unique_id", _I, [_VP]),
    ("sd_comm_init", _I, [_I, _I, _VP, C.POINTER(_VP)]),
    ("sd_comm_all_gather_tokens", _I, [_VP, _VP, _VP, _I, _I, _VP]),
    ("sd_comm_rank", _I, [_VP, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("sd_comm_destroy", _I, [_VP]),
    ("sd_profile_enable", _I, [_VP, _I]),
    ("sd_profile_read", _I, [_VP, C.POINTER(C.c_float), C.POINTER(C.c_int)]),
]


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m llmspeculativesampling_amd._build` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the HIP path.")
    # torch first: it brings its own copy of the HIP runtime (torch/lib/libamdhip64.so), and libspecdec.so must bind to THAT
    # instance - loaded before torch it would pull in /opt/rocm's copy, the process would hold two runtimes, and the first
    # kernel launch on torch's device pointers would fail with "no ROCm-capable device is detected"
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)          # AttributeError here = header and library disagree
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


class SpecDecError(RuntimeError):
    pass


def check(rc: int, what: str = "") -> None:
    """Negative sd_status -> the reference's exception at that point."""
    if rc == SD_OK:
        return
    msg = lib.sd_last_error().decode(errors="replace")
    if rc == SD_ERR_NORM_LOGITS:
        raise RuntimeError("norm logits error")          # reference utils.py:207
    if rc == SD_ERR_PROB:
        raise RuntimeError("prob error")                 # reference utils.py:224
    if rc == SD_ERR_CAPACITY:
        raise SpecDecError(f"{what}: capacity exceeded: {msg}")
    if rc == SD_ERR_INVALID:
        raise ValueError(f"{what}: {msg}")
    raise SpecDecError(f"{what}: HIP failure: {msg}")
