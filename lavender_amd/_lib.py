"""ctypes binding of liblavender_hip.so (the C ABI declared in include/lavender_hip.h).

The product path has NO fallback: if the shared library is missing or a symbol is absent, importing
this module raises.  Build it with ``python -c "import __graft_entry__ as g; g.build()"`` or ``make``.
"""
import ctypes as C
import os

import torch  # noqa: F401  -- BEFORE the CDLL below: the streams and device memory this library is handed come from torch's copy of the
#                              HIP runtime; loaded first, that copy is the libamdhip64 our .so binds to (loaded after ours, the process holds two
#                              runtimes and the first launch fails with "no ROCm-capable device is detected": __graft_entry__.build() + smoke())

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liblavender_hip.so")


class LavenderHipError(RuntimeError):
    pass


if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: the MI355X kernels are not built (run `make` or __graft_entry__.build()). "
        "lavender_amd has no CPU or eager fallback.")

lib = C.CDLL(LIB_PATH)

vp, i32, i64, f32, u32 = C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_uint32


class GemmEpilogue(C.Structure):
    _fields_ = [("bias", vp), ("act", i32), ("preact", vp), ("ldp", i64), ("gelu_in", vp), ("ldg", i64),
                ("dropout_p", f32), ("seed", u32), ("row_scale", vp), ("rows_per_group", i32), ("residual", vp),
                ("ldr", i64), ("colsum", vp), ("alpha", f32), ("out_mode", i32), ("k_keep", vp),
                ("k_rows_per_group", i32), ("rowsum_a", vp), ("preact_is_grad", i32), ("gelu_in_is_grad", i32),
                ("residual_f32", i32), ("a_rowmap", vp), ("res_rowmap", vp),
                ("res_ln_mean", vp), ("res_ln_rstd", vp), ("res_ln_gamma", vp), ("res_ln_beta", vp), ("hm_heads", i32), ("hm_head_dim", i32), ("hm_rows", i64), ("c_pad_writable", i32), ("assign", i32)]


class GemmTnJob(C.Structure):             # struct lav_gemm_tn_job
    _fields_ = [("M", i32), ("N", i32), ("K", i32), ("A", vp), ("lda", i64), ("B", vp), ("ldb", i64), ("C", vp), ("ldc", i64),
                ("rowsum_a", vp), ("k_keep", vp), ("k_rows_per_group", i32), ("alpha", f32), ("fallback_splits", i32), ("assign", i32)]


class GemmLaunchInfo(C.Structure):        # struct lav_gemm_launch_info (lav_gemm_plan / lav_gemm_tn_grouped_plan)
    _fields_ = [("kernel", C.c_char_p), ("tile_rows", i32), ("tile_cols", i32), ("grid", u32), ("block", u32)]


class LnGather(C.Structure):
    _fields_ = [("mode", i32), ("H", i32), ("W", i32), ("C0", i32)]


class LnBwdExtra(C.Structure):
    _fields_ = [("dx2", vp), ("lddx2", i64), ("row_scale", vp), ("rows_per_group", i32), ("dropout_p", f32),
                ("seed", u32), ("colsum", vp), ("x_f32", i32)]


class LnF32(C.Structure):
    _fields_ = [("x_f32", i32), ("y32", vp), ("ldy32", i64)]


class AttnDesc(C.Structure):
    _fields_ = [("mode", i32), ("heads", i32), ("head_dim", i32), ("B", i32), ("D", i32), ("H", i32), ("W", i32),
                ("wd", i32), ("wh", i32), ("ww", i32), ("sd", i32), ("sh", i32), ("sw", i32), ("cfg_wh", i32),
                ("cfg_ww", i32), ("cfg_wd", i32), ("bias_table", vp), ("n_seq", i32), ("L", i32), ("key_mask", vp),
                ("dropout_p", f32), ("seed", u32), ("scale", f32), ("tok_table", vp), ("win_type", vp), ("type_region", vp),
                ("n_types", i32), ("comb", vp), ("combT", vp), ("causal_from", i32), ("qkv_headmajor", i32), ("bias_map", vp)]


class AttnLaunchInfo(C.Structure):        # struct lav_attn_launch_info (lav_attention_plan)
    _fields_ = [("kernel", C.c_char_p), ("route", C.c_char_p), ("grid_x", u32), ("grid_y", u32), ("block", u32), ("lds_bytes", u32), ("split", i32),
                ("delta_negated", i32)]


class BertLayerDesc(C.Structure):          # struct lav_bert_layer_desc (stage-level entries)
    _fields_ = ([(n, i32) for n in ("n_seq", "L", "hidden", "heads", "ffn")] + [(n, f32) for n in ("p_hidden", "p_attn", "ln_eps")] +
                [(n, u32) for n in ("seed_attn", "seed1", "seed2")] + [("causal_from", i32)] +
                [(n, vp) for n in ("key_mask", "w_qkv", "b_qkv", "w_ao", "b_ao", "ln1_gamma", "ln1_beta", "w_ff1", "b_ff1", "w_ff2", "b_ff2",
                                   "ln2_gamma", "ln2_beta", "x", "res_pre", "res_mean", "res_rstd", "res_gamma", "res_beta", "qkv", "cx", "lse",
                                   "pre1", "mean1", "rstd1", "x1", "h_pre", "h", "pre2", "mean2", "rstd2", "y")] + [("stream_f16", i32), ("ln2_eps", f32)])


class BertLayerBwdDesc(C.Structure):       # struct lav_bert_layer_bwd_desc
    _fields_ = ([("f", BertLayerDesc)] + [(n, vp) for n in ("dy", "wt_qkv", "wt_ao", "wt_ff1", "wt_ff2")] +
                [(n, i64) for n in ("ldt_qkv", "ldt_ao", "ldt_ff1", "ldt_ff2")] +
                [(n, vp) for n in ("g_w_qkv", "g_b_qkv", "g_w_ao", "g_b_ao", "g_ln1_gamma", "g_ln1_beta", "g_w_ff1", "g_b_ff1", "g_w_ff2", "g_b_ff2",
                                   "g_ln2_gamma", "g_ln2_beta")] +
                [(n, i32) for n in ("splits_qkv", "splits_ao", "splits_ff1", "splits_ff2")] +
                [(n, vp) for n in ("d_pre2", "d_dense2", "dh", "d_x1", "d_pre1", "d_dense1", "d_cx", "dqkv", "dx")] + [("group_splits", i32), ("assign_mask", i32)])


class SwinBlockDesc(C.Structure):          # struct lav_swin_block_desc
    _fields_ = ([(n, i32) for n in ("rows", "C", "heads", "rows_per_group", "qkv_headmajor")] + [("ln_eps", f32)] +
                [(n, vp) for n in ("attn", "ln1_gamma", "ln1_beta", "w_qkv", "b_qkv", "w_proj", "b_proj", "ln2_gamma", "ln2_beta", "w_fc1", "b_fc1",
                                   "w_fc2", "b_fc2", "dp_attn", "dp_mlp", "x", "y1", "mean1", "rstd1", "qkv", "ao", "lse", "x_mid", "y2", "mean2",
                                   "rstd2", "h_pre", "h", "out")])


class SwinBlockBwdDesc(C.Structure):       # struct lav_swin_block_bwd_desc
    _fields_ = ([("f", SwinBlockDesc), ("dy", vp), ("alpha_attn", f32), ("alpha_mlp", f32)] +
                [(n, vp) for n in ("wt_qkv", "wt_proj", "wt_fc1", "wt_fc2")] + [(n, i64) for n in ("ldt_qkv", "ldt_proj", "ldt_fc1", "ldt_fc2")] +
                [(n, vp) for n in ("g_ln1_gamma", "g_ln1_beta", "g_w_qkv", "g_b_qkv", "g_bias_table", "g_w_proj", "g_b_proj", "g_ln2_gamma", "g_ln2_beta",
                                   "g_w_fc1", "g_b_fc1", "g_w_fc2", "g_b_fc2")] +
                [(n, i32) for n in ("splits_qkv", "splits_proj", "splits_fc1", "splits_fc2")] +
                [(n, vp) for n in ("dh", "d_y2", "d_mid", "d_ao", "dqkv", "d_y1", "dx")] + [("group_splits", i32), ("assign_mask", i32)])


class AttnDecodeDesc(C.Structure):         # struct lav_attn_decode_desc
    _fields_ = ([(n, i32) for n in ("B", "heads", "head_dim", "q_len", "Lv", "n_cached", "n_append", "max_len")] + [("scale", f32)] +
                [("prefix_qkv", vp), ("ld_prefix", i64), ("key_mask", vp), ("qkv_new", vp), ("ld_new", i64), ("cache_k", vp), ("cache_v", vp),
                 ("out", vp), ("ldo", i64), ("partials", vp), ("partials_capacity", i64)])


class BertLayerDecodeDesc(C.Structure):    # struct lav_bert_layer_decode_desc
    _fields_ = ([(n, i32) for n in ("B", "q_len", "hidden", "heads", "ffn", "Lv", "n_cached", "n_append", "max_len")] +
                [(n, f32) for n in ("ln_eps", "ln2_eps")] +
                [(n, vp) for n in ("key_mask", "w_qkv", "b_qkv", "w_ao", "b_ao", "ln1_gamma", "ln1_beta", "w_ff1", "b_ff1", "w_ff2", "b_ff2",
                                   "ln2_gamma", "ln2_beta", "prefix_qkv", "cache_k", "cache_v", "x", "x_res")] + [("x_res_bf16", i32)] +
                [(n, vp) for n in ("qkv", "cx", "pre1", "x1", "x1_32", "h", "pre2", "ln_stats", "y", "y32", "attn_partials")] +
                [("attn_partials_capacity", i64)])


class BeamSelectDesc(C.Structure):         # struct lav_beam_select_desc
    _fields_ = ([(n, i32) for n in ("clips", "beams", "keep", "V", "cur", "max_len", "early_stopping")] + [(n, f32) for n in ("cur_norm", "max_norm")] +
                [(n, i64) for n in ("eos_id", "pad_id")] +
                [("cand_score", vp), ("cand_word", vp), ("beam_scores", vp), ("ids", vp), ("ld_ids", i64), ("next_ids", vp), ("ld_next", i64),
                 ("parent", vp), ("hyp_ids", vp), ("hyp_score", vp), ("hyp_seq", vp), ("state", vp), ("worst", vp)])


REPARENT_MAX_LAYERS = 24                    # LAV_REPARENT_MAX_LAYERS


class BeamReparentDesc(C.Structure):       # struct lav_beam_reparent_desc
    _fields_ = ([(n, i32) for n in ("layers", "rows", "heads", "n_pos", "max_len")] + [("parent", vp)] +
                [(n, vp * REPARENT_MAX_LAYERS) for n in ("src_k", "src_v", "dst_k", "dst_v")])



class BertLayerRowsDesc(C.Structure):      # struct lav_bert_layer_rows_desc (retrieval pair scorer)
    _fields_ = ([(n, i32) for n in ("n_seq", "L", "hidden", "heads", "ffn")] + [(n, f32) for n in ("ln_eps", "ln2_eps")] +
                [(n, vp) for n in ("key_mask", "q_row", "w_qkv", "b_qkv", "w_ao", "b_ao", "ln1_gamma", "ln1_beta", "w_ff1", "b_ff1", "w_ff2", "b_ff2",
                                   "ln2_gamma", "ln2_beta", "x", "x_rowmap", "res")] + [("ldr", i64), ("res_dtype", i32)] +
                [(n, vp) for n in ("res_rowmap", "res_mean", "res_rstd", "res_gamma", "res_beta", "qkv", "cx", "pre1", "mean1", "rstd1", "x1", "h",
                                   "pre2", "mean2", "rstd2", "y", "y32")])


class MlmPairReadoutDesc(C.Structure):     # struct lav_mlm_pair_readout_desc
    _fields_ = ([(n, i32) for n in ("n", "hidden", "vocab", "true_id", "false_id")] + [("ln_eps", f32), ("x", vp), ("ldx", i64)] +
                [(n, vp) for n in ("w_dense", "b_dense", "ln_gamma", "ln_beta", "w_dec")] + [("ldw_dec", i64)] +
                [(n, vp) for n in ("b_dec", "t", "out_row", "out_col", "scores")] + [("ld_scores", i64), ("score_rows", i32), ("score_cols", i32),
                                                                                     ("logits", vp)])

P = C.POINTER
_SIGS = {
    "lav_last_error": (C.c_char_p, []),
    "lav_abi_version": (i32, []),
    "lav_gemm_bf16": (i32, [vp, i32, i32, i32, i32, vp, i64, vp, i64, vp, i64, P(GemmEpilogue), i32]),
    "lav_gemm_select": (i32, [i32, i32]),
    "lav_winl_select": (i32, [i32]),
    "lav_probe_win_prof": (None, [vp]),
    "lav_gemm_tn_grouped": (i32, [vp, i32, P(GemmTnJob), i32]),
    "lav_gemm_plan": (i32, [i32, i32, i32, i32, i64, i64, i64, P(GemmEpilogue), i32, P(GemmLaunchInfo), i32]),
    "lav_gemm_tn_grouped_plan": (i32, [i32, P(GemmTnJob), i32, P(GemmLaunchInfo), i32]),
    "lav_gemm_splits": (i32, [i32, i32, i32, i32, i64, i64, i64, P(GemmEpilogue), i32, P(C.c_size_t)]),
    "lav_gemm_tn_splits": (i32, [i32, P(GemmTnJob), i32, P(C.c_size_t)]),
    "lav_bert_layer_fwd": (i32, [vp, P(BertLayerDesc)]),
    "lav_bert_layer_bwd": (i32, [vp, vp, P(BertLayerBwdDesc)]),
    "lav_swin_block_fwd": (i32, [vp, P(SwinBlockDesc)]),
    "lav_swin_block_bwd": (i32, [vp, vp, P(SwinBlockBwdDesc)]),
    "lav_layernorm_set_defer": (i32, [vp, i32]),
    "lav_layernorm_flush": (i32, [vp]),
    "lav_layernorm_flush_all": (i32, [vp]),
    "lav_workspace_bytes": (C.c_size_t, [i32]),
    "lav_set_workspace": (i32, [vp, i32, vp, C.c_size_t]),
    "lav_layernorm_fwd": (i32, [vp, i32, i32, vp, i64, P(LnGather), vp, vp, f32, vp, i64, vp, vp, P(LnF32)]),
    "lav_layernorm_bwd": (i32, [vp, i32, i32, vp, i64, vp, i64, P(LnGather), vp, vp, vp, vp, i64, vp, i64, vp, vp,
                                P(LnBwdExtra)]),
    "lav_scale_mask_rows": (i32, [vp, i32, i32, vp, i64, vp, i64, vp, i32, f32, u32, vp, vp, i64]),
    "lav_colsum_bf16": (i32, [vp, i32, i32, vp, i64, vp]),
    "lav_attention_fwd": (i32, [vp, P(AttnDesc), vp, vp, vp]),
    "lav_attention_bwd": (i32, [vp, P(AttnDesc), vp, vp, vp, vp, vp, vp]),
    "lav_attention_bwd_bias": (i32, [vp, P(AttnDesc), vp, vp, vp, vp]),
    "lav_attention_bias_split": (i32, [P(AttnDesc)]),
    "lav_attention_lse_elems": (C.c_size_t, [P(AttnDesc)]),
    "lav_attention_plan": (i32, [P(AttnDesc), i32, P(AttnLaunchInfo), i32]),
    "lav_attention_build_bias_map": (i32, [vp, P(AttnDesc)]),
    "lav_attention_build_bias": (i32, [vp, P(AttnDesc)]),
    "lav_patch_im2col": (i32, [vp, vp, i32, i32, i32, i32, i32, vp]),
    "lav_video_embed_fwd": (i32, [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, f32, vp, i64, vp, vp]),
    "lav_video_embed_bwd": (i32, [vp, i32, i32, i32, i32, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "lav_text_embed_fwd": (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, f32, f32, u32, vp, vp, vp]),
    "lav_text_embed_bwd": (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, f32, u32, vp, vp, vp, vp, vp]),
    "lav_text_embed_pre_fwd": (i32, [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, f32, f32, u32, vp, i64, vp, vp, vp]),
    "lav_text_embed_pre_bwd": (i32, [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, f32, u32, vp, vp, vp, vp, vp, i64, vp, i32]),
    "lav_gather_rows": (i32, [vp, i32, i32, vp, i64, vp, vp, i64]),
    "lav_gather_sum_rows": (i32, [vp, i32, i32, vp, i64, vp, vp, vp, i64]),
    "lav_pair_key_mask": (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp]),
    "lav_cross_entropy_fwd_bwd": (i32, [vp, i32, i32, vp, i64, vp, vp, f32, i32]),
    "lav_scale_by_count": (i32, [vp, i64, vp, vp, f32]),
    "lav_scale_by_scalar": (i32, [vp, i64, vp, i32, vp]),
    "lav_cross_entropy_f32_fwd_bwd": (i32, [vp, i32, i32, vp, i64, vp, vp, f32, i32]),
    "lav_caption_loss_fwd_bwd": (i32, [vp, i32, i32, vp, i64, vp, f32, i32, i32, vp, vp, vp, vp, vp, i32]),
    "lav_transpose_bf16_batched": (i32, [vp, i32, vp, i32, vp, vp]),
    "lav_pair_score_fwd": (i32, [vp, i32, i32, vp, i64, vp, vp, f32, i32, vp, i64]),
    "lav_pair_score_bwd": (i32, [vp, i32, i32, vp, i64, i32, f32, vp, i64, vp, i64, vp, vp, i64, vp, vp]),
    "lav_sumsq_f32": (i32, [vp, i64, vp, vp]),
    "lav_adamw_step": (i32, [vp, i64, vp, vp, vp, vp, vp, vp, P(f32), P(f32), f32, f32, f32, i32, vp, f32, f32]),
    "lav_cast_f32_to_bf16": (i32, [vp, i64, vp, vp]),
    "lav_cast_bf16_to_f32": (i32, [vp, i64, vp, vp]),
    "lav_zero_blocks": (i32, [vp, vp, vp, i64, i32]),
    "lav_fill_droppath": (i32, [vp, i32, i32, vp, u32, vp]),
    # caption decoding (csrc/decode.hip, csrc/stages.cpp)
    "lav_gemm_skinny_bf16": (i32, [vp, i32, i32, i32, vp, i64, vp, i64, vp, i32, vp, i64, i32, vp, i64]),
    "lav_attention_decode_splits": (i32, [P(AttnDecodeDesc)]),
    "lav_attention_decode": (i32, [vp, P(AttnDecodeDesc)]),
    "lav_text_embed_rows_fwd": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, f32, vp]),
    "lav_greedy_step": (i32, [vp, i32, i32, vp, i64, vp, i64, i32, f32, vp, vp, vp, i64, i64, vp, i64]),
    "lav_bert_layer_decode": (i32, [vp, P(BertLayerDecodeDesc)]),
    # beam search (csrc/decode.hip, csrc/stages.cpp)
    "lav_attention_decode_beam": (i32, [vp, P(AttnDecodeDesc), i32]),
    "lav_bert_layer_decode_beam": (i32, [vp, P(BertLayerDecodeDesc), i32]),
    "lav_beam_step": (i32, [vp, i32, i32, i32, vp, i64, vp, i64, i32, f32, vp, vp, vp]),
    "lav_beam_select": (i32, [vp, P(BeamSelectDesc)]),
    "lav_beam_reparent": (i32, [vp, P(BeamReparentDesc)]),
    # retrieval evaluation (csrc/retrieval.hip, csrc/stages.cpp)
    "lav_attention_rows": (i32, [vp, i32, i32, i32, i32, vp, i64, vp, vp, f32, vp, i64]),
    "lav_bert_layer_fwd_rows": (i32, [vp, P(BertLayerRowsDesc)]),
    "lav_mlm_pair_readout": (i32, [vp, P(MlmPairReadoutDesc)]),
    "lav_retrieval_rank": (i32, [vp, i32, i32, vp, i64, vp, vp]),
    # video-QA read-out (csrc/qa.hip)
    "lav_answer_readout_workspace_bytes": (C.c_size_t, [i32, i32]),
    "lav_answer_readout": (i32, [vp, i32, i32, vp, i64, i32, vp, vp, vp, i32, i32, vp, C.c_size_t, vp, vp, vp]),
    "lav_match_readout": (i32, [vp, i32, i32, vp, i64, i32, vp, i64, i32, i32, vp, vp, vp, vp]),
    # fp32-I/O validation mode (csrc/validate.hip)
    "lav_v_gemm_f32": (i32, [vp, i32, i32, i32, vp, i64, vp, i64, vp, i64, vp, i32, vp, i64]),
    "lav_v_attention_f32": (i32, [vp, P(AttnDesc), vp, vp, vp]),
    "lav_v_im2col_f32": (i32, [vp, vp, i32, i32, i32, i32, i32, vp]),
    "lav_v_video_embed_f32": (i32, [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, f32, vp, i64]),
    "lav_v_text_embed_f32": (i32, [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, f32, vp]),
    "lav_v_gather_rows_f32": (i32, [vp, i32, i32, vp, i64, vp, vp, i64]),
}


class FrameXform(C.Structure):               # struct lav_frame_xform (include/lavender_pipeline.h)
    _fields_ = [("pad_left", i32), ("pad_top", i32), ("resize_w", i32), ("resize_h", i32), ("crop_x", i32), ("crop_y", i32),
                ("out_index", i64)]


# input pipeline (include/lavender_pipeline.h)
_PIPE_SIGS = {
    "lav_tsv_open": (vp, [C.c_char_p, C.c_char_p]),
    "lav_tsv_rows": (i64, [vp]),
    "lav_tsv_row_offset": (i64, [vp, i64]),
    "lav_tsv_fields": (i32, [vp, i64, i32, P(vp), P(i64)]),
    "lav_tsv_close": (None, [vp]),
    "lav_jpeg_peek": (i32, [vp, i64, P(i32), P(i32)]),
    "lav_decoder_create": (vp, [i32]),
    "lav_decoder_destroy": (None, [vp]),
    "lav_decoder_decode": (i32, [vp, vp, i32, P(vp), P(i64), P(FrameXform), i32, i32, P(f32), P(f32), vp]),
    "lav_decoder_failed_frames": (i32, [vp, P(i32), i32]),
    "lav_decoder_read_rgb": (i32, [vp, i32, vp, i64, P(i32), P(i32)]),
}
class MatDesc(C.Structure):                  # struct lav_mat_desc
    _fields_ = [("src_off", C.c_long), ("dst_off", C.c_long), ("rows", C.c_int), ("cols", C.c_int), ("ld_dst", C.c_int),
                ("tile0", C.c_int)]


EXPORTS = tuple(_SIGS)
PIPELINE_EXPORTS = tuple(_PIPE_SIGS)

for _name, (_res, _args) in {**_SIGS, **_PIPE_SIGS}.items():
    try:
        _f = getattr(lib, _name)
    except AttributeError as e:  # pragma: no cover
        raise ImportError(f"{LIB_PATH} does not export {_name}; rebuild it") from e
    _f.restype = _res
    _f.argtypes = _args


ABI_VERSION = 7
if lib.lav_abi_version() != ABI_VERSION:  # pragma: no cover
    raise ImportError(f"{LIB_PATH} has ABI version {lib.lav_abi_version()}, this package binds version {ABI_VERSION} (descriptor layouts differ): "
                      "rebuild it with `make -C <repo root>` or `python -c 'import __graft_entry__ as g; g.build()'`")


def check(rc, what=""):
    if rc != 0:
        msg = lib.lav_last_error()
        raise LavenderHipError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")
