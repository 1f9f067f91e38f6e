"""ctypes binding of libmode_hip.so (C-ABI declared in include/mode_hip.h).

The HIP library IS the product: there is no CPU / PyTorch fallback.  If the shared object is missing or a symbol is
absent, loading fails loudly (``ModeHipUnavailable``) and every operator that needs it raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MODE_HIP_LIB", os.path.join(_HERE, "libmode_hip.so"))

MODE_BF16, MODE_F32 = 0, 1
EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_RESIDUAL, EPI_SWIGLU, EPI_RESIDUAL_NORM = 0, 1, 2, 3, 4, 5
ABI_VERSION = 13
GEMM_SKINNY_OK, GEMM_W_KN, GEMM_A_KM, GEMM_UNIFORM_GROUPS, GEMM_SMALL_ROWS, GEMM_IDENTITY_ROWS = 1, 2, 4, 8, 16, 32

c_i32, c_i64, c_f32, c_vp, c_sz = C.c_int32, C.c_int64, C.c_float, C.c_void_p, C.c_size_t


class ModeHipUnavailable(RuntimeError):
    pass


class ModeAdamWFuse(C.Structure):
    """AdamW in the epilogue of a weight-gradient GEMM (include/mode_hip.h, ABI 11): arena base pointers (same element offsets as the gradient
    arena), the step's hyper-parameters, optional per-workgroup sums of squares of the gradient."""
    _fields_ = [("grad_base", c_vp), ("param_base", c_vp), ("exp_avg_base", c_vp), ("exp_avg_sq_base", c_vp), ("lp_base", c_vp), ("ema_base", c_vp),
                ("ema_rate", c_f32), ("lr", c_f32), ("beta1", c_f32), ("beta2", c_f32), ("eps", c_f32), ("weight_decay", c_f32), ("step", c_i32),
                ("grad_scale", c_f32), ("gsq", c_vp), ("gsq_capacity", c_i64), ("side_stream", c_vp), ("side_events", c_vp)]


class ModeGemmDesc(C.Structure):
    _fields_ = [("dtype", c_i32), ("epilogue", c_i32), ("out_dtype", c_i32), ("M", c_i32), ("N", c_i32), ("K", c_i32),
                ("A", c_vp), ("lda", c_i64), ("W", c_vp), ("ldw", c_i64), ("w_expert_stride", c_i64),
                ("bias", c_vp), ("bias_expert_stride", c_i64), ("resid", c_vp), ("ldr", c_i64), ("C", c_vp), ("ldc", c_i64),
                ("a_rows", c_vp), ("expert_offsets", c_vp), ("num_experts", c_i32), ("split_k", c_i32), ("split_stride", c_i64), ("k_group_offsets", c_vp), ("num_k_groups", c_i32),
                ("c_group_stride", c_i64), ("flags", c_i32), ("w_rows", c_vp),
                ("C2", c_vp), ("ldc2", c_i64), ("gain", c_vp), ("row_ss_out", c_vp), ("row_ss", c_vp), ("row_ss_n", c_i32), ("row_eps", c_f32),
                ("w_tap_cols", c_i32), ("w_rows_tap_stride", c_i64), ("a_tap_cols", c_i32), ("a_rows_tap_stride", c_i64),
                ("adamw", C.POINTER(ModeAdamWFuse)),
                ("touch0", c_vp), ("touch0_bytes", c_i64), ("touch1", c_vp), ("touch1_bytes", c_i64)]      # weight run-ahead ranges (a hint; zero = none)


class ModeEmbedDesc(C.Structure):
    _fields_ = [("B", c_i32), ("T", c_i32), ("D", c_i32), ("A_len", c_i32), ("A_dim", c_i32), ("n_img", c_i32),
                ("use_noise_token", c_i32), ("emb_t", c_vp), ("emb_row_stride", c_i64), ("goal_e", c_vp), ("img_e", c_vp),
                ("actions", c_vp), ("c_in", c_vp), ("c_in_stride", c_i64), ("w_act", c_vp), ("pos", c_vp), ("g", c_vp),
                ("cond", c_vp), ("cond_row_stride", c_i64), ("eps", c_f32), ("x", c_vp), ("h", c_vp), ("h_dtype", c_i32)]


class ModeHeadDesc(C.Structure):
    _fields_ = [("B", c_i32), ("T", c_i32), ("D", c_i32), ("A_len", c_i32), ("A_dim", c_i32), ("k", c_i32),
                ("u", c_vp), ("Y", c_vp), ("y_dtype", c_i32), ("y_splits", c_i32), ("y_split_stride", c_i64), ("pos", c_vp), ("posw", c_vp), ("g", c_vp), ("eps", c_f32),
                ("w_out", c_vp), ("b_out", c_vp), ("x_a", c_vp), ("scal", c_vp), ("scal_stride", c_i64),
                ("F", c_vp), ("denoised", c_vp), ("x_next", c_vp), ("u_ss", c_vp), ("u_ss_n", c_i32), ("u_gain", c_vp), ("den_prev", c_vp), ("lin", c_vp), ("aux1", c_vp), ("aux2", c_vp)]


class ModeDims(C.Structure):
    _fields_ = [("D", c_i32), ("H", c_i32), ("L", c_i32), ("E", c_i32), ("k", c_i32), ("T", c_i32), ("A_len", c_i32),
                ("A_dim", c_i32), ("O", c_i32), ("G", c_i32), ("n_img", c_i32), ("use_noise_token", c_i32),
                ("router_normalize", c_i32), ("eps", c_f32)]


class ModeLayerWeights(C.Structure):
    _fields_ = [("ln1_g", c_vp), ("ln2_g", c_vp), ("qn_g", c_vp), ("kn_g", c_vp), ("wqkv", c_vp), ("bqkv", c_vp),
                ("wo", c_vp), ("r_w0", c_vp), ("r_b0", c_vp), ("r_w3", c_vp), ("r_b3", c_vp), ("w1", c_vp), ("b1", c_vp),
                ("w2", c_vp)]


class ModeModelWeights(C.Structure):
    _fields_ = [("pos", c_vp), ("w_se", c_vp), ("b_se", c_vp), ("w_sl", c_vp), ("w_tok", c_vp), ("w_goal", c_vp),
                ("w_act", c_vp), ("ln_g", c_vp), ("w_out", c_vp), ("b_out", c_vp), ("layers", C.POINTER(ModeLayerWeights))]


class ModeMetaLayout(C.Structure):
    _fields_ = [("counts", c_i32), ("offsets", c_i32), ("perm", c_i32), ("pos", c_i32), ("posw", c_i32), ("poffsets", c_i32), ("prow", c_i32),
                ("total_words", c_i32), ("padded_rows", c_i32)]


c_u64, c_u32 = C.c_uint64, C.c_uint32


class ModeStashLayout(C.Structure):
    _fields_ = [(n, c_u64) for n in ("x0", "h1", "qkv", "yattn", "x1", "ub", "P", "Hd", "Y", "layer_stride", "xL", "yL", "u_tmp", "tr_hid", "tr_logits", "global_bytes",
                                     "total_bytes")]


class ModeGroupedMlpDesc(C.Structure):
    _fields_ = [("dtype", c_i32), ("N", c_i32), ("D", c_i32), ("E", c_i32), ("k", c_i32), ("x", c_vp), ("perm", c_vp), ("offsets", c_vp),
                ("w1", c_vp), ("b1", c_vp), ("w2", c_vp), ("p", c_vp), ("h", c_vp), ("y", c_vp), ("y_dtype", c_i32), ("seed", c_u32),
                ("p_drop", c_f32), ("dy", c_vp), ("dxs", c_vp), ("dw1", c_vp), ("db1", c_vp), ("dw2", c_vp)]


class ModeTrainArgs(C.Structure):
    _fields_ = [("B", c_i32), ("dtype", c_i32), ("seed", c_u32), ("attn_pdrop", c_f32), ("mlp_pdrop", c_f32), ("sigma", c_vp), ("e1", c_vp),
                ("emb_t", c_vp), ("cond", c_vp), ("goal_in_cond", c_i32), ("state_images", c_vp), ("goals", c_vp), ("goal_e", c_vp),
                ("img_e", c_vp), ("actions", c_vp), ("c_in", c_vp), ("c_in_stride", c_i64), ("actions_scaled", c_vp), ("act_rows", c_vp),
                ("meta", c_vp), ("meta_layer_stride", c_i64), ("topk_idx", c_vp), ("topk_layer_stride", c_i64), ("idx_per_token", c_i32),
                ("probs", c_vp), ("r_pre", c_vp), ("F", c_vp), ("layer_events", c_vp), ("shifted", c_vp), ("aux_lb_coef", c_vp), ("aux_z_coef", c_vp),
                ("d_state_images", c_vp), ("d_goals", c_vp), ("token_routing", c_i32), ("tr_pre", c_vp), ("tr_shifted", c_vp), ("tr_topk_idx", c_vp),
                ("tr_topk_w", c_vp), ("fuse_adamw", C.POINTER(ModeAdamWFuse))]


class ModeLayerGrads(C.Structure):
    _fields_ = [(n, c_vp) for n in ("ln1_g", "ln2_g", "qn_g", "kn_g", "wqkv", "bqkv", "wo", "r_w0", "r_b0", "r_w3", "r_b3", "w1", "b1", "w2")]


class ModeModelGrads(C.Structure):
    _fields_ = [(n, c_vp) for n in ("pos", "w_se", "b_se", "w_sl", "w_tok", "w_goal", "w_act", "ln_g", "w_out", "b_out")] + \
               [("layers", C.POINTER(ModeLayerGrads))]


class ModeLayerWeightsT(C.Structure):
    _fields_ = [(n, c_vp) for n in ("wqkvT", "woT", "w1T", "w2T")]


class ModeModelWeightsT(C.Structure):
    _fields_ = [("w_outT", c_vp), ("layers", C.POINTER(ModeLayerWeightsT))]


class ModeForwardArgs(C.Structure):
    _fields_ = [("B", c_i32), ("dtype", c_i32), ("emb_t", c_vp), ("emb_row_stride", c_i64), ("cond", c_vp),
                ("cond_row_stride", c_i64), ("meta", c_vp), ("meta_layer_stride", c_i64), ("goal_e", c_vp), ("img_e", c_vp),
                ("actions", c_vp), ("c_in", c_vp), ("c_in_stride", c_i64), ("scal", c_vp), ("scal_stride", c_i64),
                ("F", c_vp), ("denoised", c_vp), ("x_next", c_vp), ("topk_idx_out", c_vp), ("uniform_routing", c_i32), ("den_prev", c_vp), ("lin", c_vp), ("aux1", c_vp), ("aux2", c_vp)]


class ModeEmbedGuidedDesc(C.Structure):
    """mode_embed_tokens_fwd for classifier-free guidance pairs (include/mode_hip.h, an addition to ABI 13): emb.B pairs, 2 * emb.B * T rows written."""
    _fields_ = [("emb", ModeEmbedDesc)]


class ModeHeadGuidedDesc(C.Structure):
    """mode_head_ddim_fwd for pairs: den = den_u + scale[0] * (den_c - den_u) ahead of the solver update; ``scale`` a device fp32 scalar."""
    _fields_ = [("head", ModeHeadDesc), ("scale", c_vp)]


class ModeGuidedArgs(C.Structure):
    """mode_dit_forward for pairs: fwd.B pairs at an internal batch of 2 * fwd.B (what every field means then: include/mode_hip.h)."""
    _fields_ = [("fwd", ModeForwardArgs), ("scale", c_vp)]


class ModeQkvAttnDesc(C.Structure):
    _fields_ = [("dtype", c_i32), ("B", c_i32), ("T", c_i32), ("H", c_i32), ("D", c_i32), ("h", c_vp), ("ldh", c_i64), ("wqkv", c_vp), ("ldw", c_i64),
                ("bqkv", c_vp), ("q_gain", c_vp), ("k_gain", c_vp), ("eps", c_f32), ("y", c_vp), ("ldy", c_i64)]


class ModeConvBnDesc(C.Structure):
    _fields_ = [("x", c_vp), ("ldx", c_i64), ("idx", c_vp), ("idx_tap_stride", c_i64), ("taps", c_i32), ("w", c_vp), ("ldw", c_i64), ("y", c_vp), ("ldy", c_i64),
                ("M", c_i32), ("Cin", c_i32), ("Cout", c_i32), ("bn_mean", c_vp), ("bn_var", c_vp), ("bn_weight", c_vp), ("bn_bias", c_vp), ("bn_eps", c_f32),
                ("residual", c_vp), ("ldr", c_i64), ("relu", c_i32), ("pre_gamma", c_vp), ("pre_beta", c_vp), ("post_gamma", c_vp), ("post_beta", c_vp),
                ("rows_per_sample", c_i32), ("stat_sum", c_vp), ("stat_sq", c_vp)]


class ModeBnFilmDesc(C.Structure):
    _fields_ = [("N", c_i32), ("C", c_i32), ("HW", c_i32), ("dtype", c_i32), ("x", c_vp), ("scale", c_vp), ("shift", c_vp), ("pre_gamma", c_vp),
                ("pre_beta", c_vp), ("residual", c_vp), ("relu", c_i32), ("post_gamma", c_vp), ("post_beta", c_vp), ("y", c_vp),
                ("bn_weight", c_vp), ("bn_bias", c_vp), ("bn_mean", c_vp), ("bn_var", c_vp), ("bn_eps", c_f32), ("channels_last", c_i32)]


class ModeStemConvDesc(C.Structure):
    _fields_ = [("x", c_vp), ("x_dtype", c_i32), ("sxn", c_i64), ("sxc", c_i64), ("sxh", c_i64), ("sxw", c_i64), ("N", c_i32), ("H", c_i32), ("W", c_i32),
                ("Cin", c_i32), ("kh", c_i32), ("kw", c_i32), ("sh", c_i32), ("sw", c_i32), ("ph", c_i32), ("pw", c_i32), ("Cout", c_i32), ("w", c_vp),
                ("y", c_vp), ("bn_mean", c_vp), ("bn_var", c_vp), ("bn_weight", c_vp), ("bn_bias", c_vp), ("bn_eps", c_f32), ("relu", c_i32), ("dy", c_vp),
                ("dw_part", c_vp)]


MODE_ENV_MAX = 1024


class ModeEnvPoolDesc(C.Structure):
    """Commit + emit of a vectorised rollout's control step (include/mode_hip.h, ABI 13)."""
    _fields_ = [("num_envs", c_i32), ("W", c_i32), ("A", c_i32), ("multistep", c_i32), ("ctrl", c_vp), ("chunk", c_vp), ("plan", c_vp),
                ("counter", c_vp), ("draws", c_vp), ("out", c_vp), ("active", c_u32 * (MODE_ENV_MAX // 32))]


class ModeEnvEnsDesc(C.Structure):
    """Commit + emit with temporal ensembling over a ring of each environment's last K plans (include/mode_hip.h, an addition to ABI 13)."""
    _fields_ = [("pool", ModeEnvPoolDesc), ("ring", c_vp), ("birth", c_vp), ("t", c_vp), ("weights", c_vp), ("K", c_i32)]


class ModeEnvSelectDesc(C.Structure):
    """Selection among the N candidate plans of every replanning row (include/mode_hip.h, an addition to ABI 13)."""
    _fields_ = [("rows", c_vp), ("has_prev", c_vp), ("count", c_vp), ("chunk", c_vp), ("plan", c_vp), ("weights", c_vp), ("chosen", c_vp),
                ("selected", c_vp), ("scores", c_vp), ("m_b", c_i32), ("num_envs", c_i32), ("W", c_i32), ("A", c_i32), ("shift", c_i32), ("N", c_i32)]


class ModeEnvBidDesc(C.Structure):
    """Selection with forward contrast among N strong candidates, against M weak ones (include/mode_hip.h, an addition to ABI 13)."""
    _fields_ = [("rows", c_vp), ("has_prev", c_vp), ("count", c_vp), ("chunk", c_vp), ("plan", c_vp), ("weights", c_vp), ("chosen", c_vp),
                ("selected", c_vp), ("scores", c_vp), ("lambda_", c_vp), ("bc", c_vp), ("fc", c_vp), ("m_b", c_i32), ("num_envs", c_i32),
                ("W", c_i32), ("A", c_i32), ("shift", c_i32), ("N", c_i32), ("M", c_i32), ("K", c_i32)]


class ModeEnvFramesCam(C.Structure):
    """One camera of mode_env_gather_frames (include/mode_hip.h, ABI 13)."""
    _fields_ = [("src", c_vp), ("src_stride", c_i64), ("row_elems", c_i64), ("dst", c_vp), ("src_dtype", c_i32), ("dst_dtype", c_i32)]


class ModeEnvFramesDesc(C.Structure):
    """Gather of the replanning environments' camera frames into the encoders' input (include/mode_hip.h, ABI 13)."""
    _fields_ = [("rows", c_vp), ("m_b", c_i32), ("num_envs", c_i32), ("cam", ModeEnvFramesCam * 2)]


class ModeFramePrepCam(C.Structure):
    """One camera of mode_frames_preprocess (include/mode_hip.h, an addition to ABI 13)."""
    _fields_ = [("src", c_vp), ("src_stride", c_i64), ("dst", c_vp), ("shifts", c_vp), ("T", c_i32), ("H", c_i32), ("W", c_i32), ("OH", c_i32),
                ("OW", c_i32), ("dst_dtype", c_i32), ("pad", c_i32), ("mean", c_f32 * 3), ("inv_std", c_f32 * 3)]


class ModeFramePrepDesc(C.Structure):
    """uint8 HWC camera frames -> resized, shifted, normalised NCHW encoder input, both cameras in one launch (include/mode_hip.h)."""
    _fields_ = [("rows", c_vp), ("m_b", c_i32), ("num_envs", c_i32), ("cam", ModeFramePrepCam * 2)]


class ModeDataStreamDesc(C.Structure):
    """mode_data_sample_windows (include/mode_hip.h, an addition to ABI 13): the store's tables, the draw's (seed, step) and the batch's outputs."""
    _fields_ = [("actions", c_vp), ("ep_begin", c_vp), ("starts", c_vp), ("goals", c_vp), ("lo", c_vp), ("scale", c_vp), ("S", c_i32), ("E", c_i32),
                ("A", c_i32), ("G", c_i32), ("W", c_i32), ("B", c_i32), ("n_total", c_i32), ("seed", c_u32), ("step", c_u32), ("out_actions", c_vp),
                ("action_mask", c_vp), ("latent_goal", c_vp), ("index", c_vp), ("episode", c_vp), ("noise", c_vp), ("u", c_vp), ("shifts", c_vp * 2),
                ("shift_pad", c_i32 * 2)]


MODE_ORDER_EPOCH, MODE_ORDER_WEIGHTED = 1, 2


class ModeDataOrderDesc(C.Structure):
    """mode_data_sample_windows_ordered (include/mode_hip.h, an addition to ABI 13): a ModeDataStreamDesc, the mode, the int64 cut table of a weighted
    mixture and the int64 epoch / position outputs of an epoch order."""
    _fields_ = [("s", ModeDataStreamDesc), ("mode", c_i32), ("cut", c_vp), ("epoch", c_vp), ("position", c_vp)]


class ModeDataSweepDesc(C.Structure):
    """mode_data_sweep_windows (include/mode_hip.h, an addition to ABI 13): the store's tables, the enumeration's (stride, first), the noise's
    (seed, draw, noise_scale) and the batch's outputs."""
    _fields_ = [("actions", c_vp), ("ep_begin", c_vp), ("starts", c_vp), ("goals", c_vp), ("lo", c_vp), ("scale", c_vp), ("S", c_i32), ("E", c_i32),
                ("A", c_i32), ("G", c_i32), ("W", c_i32), ("B", c_i32), ("n_total", c_i32), ("stride", c_i32), ("first", c_i32), ("seed", c_u32),
                ("draw", c_u32), ("noise_scale", c_f32), ("out_actions", c_vp), ("action_mask", c_vp), ("latent_goal", c_vp), ("index", c_vp),
                ("episode", c_vp), ("valid", c_vp), ("window", c_vp), ("noise", c_vp)]


class ModeActionErrorDesc(C.Structure):
    """mode_action_error (include/mode_hip.h, an addition to ABI 13): two [B, W, A] chunks, the optional mask / weight / unit factors and the fp64
    accumulators."""
    _fields_ = [("pred", c_vp), ("target", c_vp), ("mask", c_vp), ("weight", c_vp), ("unit", c_vp), ("sq", c_vp), ("ab", c_vp), ("cnt", c_vp),
                ("B", c_i32), ("W", c_i32), ("A", c_i32), ("accumulate", c_i32)]


class ModeDataGoalDesc(C.Structure):
    """mode_data_relabel_goals (include/mode_hip.h, an addition to ABI 13): the store's per-step goal embeddings, the index / episode a sampling
    launch wrote, the draws' (ids, seed, step, lo, hi, thresh) and the relabelled outputs."""
    _fields_ = [("step_goals", c_vp), ("ep_begin", c_vp), ("index", c_vp), ("episode", c_vp), ("ids", c_vp), ("thresh", C.c_uint64),
                ("goal_dtype", c_i32), ("S", c_i32), ("E", c_i32), ("G", c_i32), ("B", c_i32), ("seed", c_u32), ("step", c_u32), ("lo", c_i32),
                ("hi", c_i32), ("latent_goal", c_vp), ("goal_index", c_vp), ("goal_offset", c_vp), ("goal_kind", c_vp)]


class ModeValLevelsDesc(C.Structure):
    """mode_val_noise_levels (include/mode_hip.h, an addition to ABI 13): a swept batch's actions / noise / window, the sigma table and the draw;
    the rows' level, sigma and noised input."""
    _fields_ = [("actions", c_vp), ("noise", c_vp), ("window", c_vp), ("sigmas", c_vp), ("B", c_i32), ("W", c_i32), ("A", c_i32), ("K", c_i32),
                ("draw", c_u32), ("level", c_vp), ("sigma", c_vp), ("x", c_vp)]


class ModeLevelErrorDesc(C.Structure):
    """mode_level_error (include/mode_hip.h, an addition to ABI 13): mode_action_error's chunks and factors, a level per row and the fp64
    accumulators per level."""
    _fields_ = [("pred", c_vp), ("target", c_vp), ("mask", c_vp), ("weight", c_vp), ("level", c_vp), ("sq", c_vp), ("cnt", c_vp), ("B", c_i32),
                ("W", c_i32), ("A", c_i32), ("K", c_i32), ("accumulate", c_i32)]


MODE_GRAD_CHUNK = 16384


class ModeGradChunk(C.Structure):
    """One chunk of mode_grad_sumsq (include/mode_hip.h, an addition to ABI 13): at most MODE_GRAD_CHUNK elements of ONE tensor, lo 16-byte aligned."""
    _fields_ = [("lo", c_i64), ("n", c_i32), ("tensor", c_i32)]


class ModeGradClipState(C.Structure):
    """Device-side result of mode_grad_clip_finish, read by mode_adamw_step_clipped (include/mode_hip.h)."""
    _fields_ = [("total_norm", c_f32), ("coef", c_f32), ("scale", c_f32), ("nonfinite", c_i32), ("skip", c_i32), ("skipped", c_i32), ("pad", c_i32 * 2)]


MODE_LORA_MAX_RANK = 64


class ModeLoraDesc(C.Structure):
    """One LoRA target of mode_lora_merge / mode_lora_grad (include/mode_hip.h, an addition to ABI 13): G matrices [rows, cols], w_stride elements apart."""
    _fields_ = [("G", c_i32), ("rows", c_i32), ("cols", c_i32), ("r", c_i32), ("w_stride", c_i64), ("W", c_vp), ("A", c_vp), ("B", c_vp), ("scale", c_vp),
                ("out", c_vp), ("out_dtype", c_i32), ("accumulate", c_i32), ("dW", c_vp), ("dA", c_vp), ("dB", c_vp)]


class ModeLoraFactDesc(C.Structure):
    """mode_lora_fact_grad (include/mode_hip.h, an addition to ABI 13): dA / dB of G matrices [rows, cols] from the bf16 operands X [M, cols] and
    dY [M, rows] of the dense weight-gradient GEMM, grouped by row offsets."""
    _fields_ = [("G", c_i32), ("rows", c_i32), ("cols", c_i32), ("r", c_i32), ("M", c_i32), ("dtype", c_i32), ("X", c_vp), ("ld_x", c_i64),
                ("x_rows", c_vp), ("dY", c_vp), ("ld_dy", c_i64), ("group_offsets", c_vp), ("A", c_vp), ("B", c_vp), ("scale", c_vp),
                ("dA", c_vp), ("dB", c_vp)]


LORA_KINDS = ("wqkv", "wo", "w1", "w2")                          # the [kind] order of ModeLoraTrain's tables


class ModeLoraTrain(C.Structure):
    """mode_dit_backward_lora: per kind a table of per-layer A / B / dA / dB pointers (NULL table = kind not adapted) and the factored workspace."""
    _fields_ = [("r", c_i32), ("reserved", c_i32), ("scale", c_vp), ("A", c_vp * 4), ("B", c_vp * 4), ("dA", c_vp * 4), ("dB", c_vp * 4),
                ("workspace", c_vp), ("workspace_bytes", c_sz)]


P = C.POINTER
# name -> (restype, argtypes): every symbol include/mode_hip.h declares
PROTOTYPES = {
    "mode_hip_version": (C.c_int, []),
    "mode_hip_status_string": (C.c_char_p, [C.c_int]),
    "mode_set_option": (C.c_int, [C.c_char_p, C.c_int]),
    "mode_probe_mfma_burn": (C.c_int, [c_vp, c_vp, C.c_int, C.c_int, P(C.c_double), c_vp]),
    "mode_hip_sizeof": (c_sz, [C.c_char_p]),
    "mode_gemm": (C.c_int, [P(ModeGemmDesc), c_vp]),
    "mode_rmsnorm_cond_fwd": (C.c_int, [c_vp, c_vp, c_vp, C.c_int, C.c_int, C.c_int, c_f32, c_vp, c_vp, C.c_int, c_vp]),
    "mode_attn_block_fwd": (C.c_int, [c_vp, c_vp, c_vp, c_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_f32, C.c_uint32, c_f32, c_vp]),
    "mode_qkv_attn_fwd": (C.c_int, [C.POINTER(ModeQkvAttnDesc), c_vp]),
    "mode_conv_bn_act_fwd": (C.c_int, [C.POINTER(ModeConvBnDesc), c_vp]),
    "mode_attn_block_bwd": (C.c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_f32, C.c_uint32,
                                      c_f32, c_vp]),
    "mode_sigma_embed": (C.c_int, [c_vp, c_vp, c_vp, c_vp, C.c_int, C.c_int, c_vp]),
    "mode_moe_route_topk_f32": (C.c_int, [c_vp, C.c_int, C.c_int, C.c_int, C.c_int, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "mode_moe_dispatch_meta": (C.c_int, [c_vp, c_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "mode_moe_combine_norm_fwd": (C.c_int, [c_vp, c_vp, C.c_int, C.c_int, c_i64, c_vp, c_vp, C.c_int, C.c_int, C.c_int, c_vp, c_vp, C.c_int,
                                            c_f32, c_vp, c_vp, C.c_int, c_vp]),
    "mode_moe_combine_norm_fused_fwd": (C.c_int, [c_vp, c_vp, C.c_int, c_vp, c_vp, C.c_int, C.c_int, c_i64, c_vp, c_vp, C.c_int, C.c_int, C.c_int, c_vp,
                                                  c_vp, C.c_int, c_f32, c_vp, c_vp, C.c_int, c_vp]),
    "mode_embed_tokens_fwd": (C.c_int, [P(ModeEmbedDesc), c_vp]),
    "mode_head_ddim_fwd": (C.c_int, [P(ModeHeadDesc), c_vp]),
    "mode_ddim_edm_step": (C.c_int, [c_vp, c_vp, c_vp, c_i64, C.c_int, C.c_int, c_vp, c_vp, c_vp]),
    "mode_transpose": (C.c_int, [c_vp, c_i64, C.c_int, C.c_int, c_vp, c_i64, c_vp, c_vp, C.c_int, c_vp]),
    "mode_colsum_workspace_bytes": (c_sz, [C.c_int, C.c_int, C.c_int]),
    "mode_colsum": (C.c_int, [c_vp, c_i64, C.c_int, C.c_int, C.c_int, c_vp, C.c_int, C.c_int, c_vp, C.c_int, c_vp, c_sz, c_vp]),
    "mode_swiglu_fwd": (C.c_int, [c_vp, c_vp, c_i64, C.c_int, C.c_int, C.c_uint32, c_f32, c_vp]),
    "mode_swiglu_bwd": (C.c_int, [c_vp, c_vp, c_vp, c_i64, C.c_int, C.c_int, C.c_uint32, c_f32, c_vp]),
    "mode_rmsnorm_bwd": (C.c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, C.c_int, C.c_int, C.c_int, c_f32, c_vp, C.c_int, c_vp, c_vp, c_vp, C.c_int, c_vp]),
    "mode_rowcopy_f32": (C.c_int, [c_vp, c_i64, C.c_int, C.c_int, c_vp, c_vp, c_i64, C.c_int, C.c_int, c_vp, c_vp, c_i64, C.c_int, C.c_int, c_vp]),
    "mode_gelu_fwd": (C.c_int, [c_vp, c_vp, c_i64, c_vp]),
    "mode_gelu_bwd": (C.c_int, [c_vp, c_vp, c_vp, c_i64, c_vp]),
    "mode_moe_router_bwd": (C.c_int, [c_vp, c_vp, c_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_vp, c_vp]),
    "mode_moe_router_bwd_aux": (C.c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_vp, c_vp]),
    "mode_edm_noise_scale": (C.c_int, [c_vp, c_vp, c_vp, c_f32, C.c_int, C.c_int, c_vp, c_vp]),
    "mode_edm_loss": (C.c_int, [c_vp, c_vp, c_vp, c_vp, c_f32, C.c_int, C.c_int, c_vp, c_vp, c_vp]),
    "mode_sigma_embed_bwd": (C.c_int, [c_vp, c_vp, C.c_int, C.c_int, c_vp, c_vp, c_vp]),
    "mode_moe_combine_bwd": (C.c_int, [c_vp, c_vp, C.c_int, c_vp, c_vp, C.c_int, C.c_int, C.c_int, c_vp, c_vp, c_vp]),
    "mode_moe_meta_layout": (C.c_int, [C.c_int, C.c_int, C.c_int, P(ModeMetaLayout)]),
    "mode_dit_dispatch": (C.c_int, [c_vp, c_vp, C.c_int, c_i64, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_vp, c_vp]),
    "mode_dit_workspace_bytes": (c_sz, [P(ModeDims), C.c_int, C.c_int, C.c_int]),
    "mode_dit_sigma_embed": (C.c_int, [P(ModeDims), P(ModeModelWeights), c_vp, C.c_int, c_vp, c_vp, c_sz, c_vp]),
    "mode_dit_embed_obs": (C.c_int, [P(ModeDims), P(ModeModelWeights), c_vp, c_vp, C.c_int, c_vp, c_vp, c_vp]),
    "mode_dit_route": (C.c_int, [P(ModeDims), P(ModeModelWeights), c_vp, C.c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "mode_moe_weights_from_idx": (C.c_int, [c_vp, c_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_vp, c_vp]),
    "mode_moe_sample_experts": (C.c_int, [c_vp, c_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_vp, c_vp, c_vp]),
    "mode_moe_aux_stats": (C.c_int, [c_vp, c_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_vp, C.c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "mode_dit_train_stash_layout": (C.c_int, [P(ModeDims), C.c_int, C.c_int, P(ModeStashLayout)]),
    "mode_dit_train_workspace_bytes": (c_sz, [P(ModeDims), C.c_int, C.c_int]),
    "mode_dit_forward_train": (C.c_int, [P(ModeDims), P(ModeModelWeights), P(ModeTrainArgs), c_vp, c_sz, c_vp]),
    "mode_dit_forward_train_layer": (C.c_int, [P(ModeDims), P(ModeModelWeights), P(ModeTrainArgs), c_vp, c_sz, c_i32, c_i32, c_vp]),
    "mode_moe_grouped_mlp_workspace_bytes": (c_sz, [c_i32, c_i32, c_i32, c_i32, c_i32]),
    "mode_moe_grouped_mlp_fwd": (C.c_int, [P(ModeGroupedMlpDesc), c_vp]),
    "mode_moe_grouped_mlp_bwd": (C.c_int, [P(ModeGroupedMlpDesc), c_vp, c_sz, c_vp]),
    "mode_rmsnorm_cond_bwd_workspace_bytes": (c_sz, [c_i32, c_i32, c_i32]),
    "mode_rmsnorm_cond_bwd": (C.c_int, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_f32, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "mode_swiglu_bwd_bias_workspace_bytes": (c_sz, [c_i64, c_i32, c_i32]),
    "mode_swiglu_bwd_bias": (C.c_int, [c_vp, c_vp, c_vp, c_i64, c_i32, c_i32, c_u32, c_f32, c_vp, c_i32, c_vp, c_vp, c_sz, c_vp]),
    "mode_pos_emb_bwd": (C.c_int, [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "mode_router_logits": (C.c_int, [c_vp, c_i64, c_vp, c_i64, c_vp, c_i64, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "mode_router_mlp_bwd": (C.c_int, [c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "mode_iota_i32": (C.c_int, [c_vp, c_i32, c_i32, c_vp]),
    "mode_adamw_step": (C.c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, c_i32, C.c_float, c_vp, c_vp,
                                  C.c_float, c_vp]),
    "mode_ema_update": (C.c_int, [c_vp, c_vp, c_i64, C.c_float, c_vp]),
    "mode_grad_sumsq": (C.c_int, [c_vp, c_vp, c_i32, c_i32, c_vp, c_vp]),
    "mode_grad_clip_finish": (C.c_int, [c_vp, c_vp, c_i32, C.c_float, C.c_float, c_i32, c_vp, c_vp, c_vp]),
    "mode_adamw_step_clipped": (C.c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, c_i32, c_vp, c_vp,
                                          C.c_float, c_vp, c_vp]),
    # (p, g, m_bf16, v_bf16, n, elem_base, lr, beta1, beta2, eps, weight_decay, step, round_seed, grad_scale, lp_bf16, ema, ema_rate, st, stream)
    "mode_adamw_step_lp": (C.c_int, [c_vp, c_vp, c_vp, c_vp, c_i64, c_i64, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, c_i32, C.c_uint32,
                                     C.c_float, c_vp, c_vp, C.c_float, c_vp, c_vp]),
    "mode_adamw_fuse_gsq_floats": (c_i64, [P(ModeDims)]),
    "mode_dit_backward": (C.c_int, [P(ModeDims), P(ModeModelWeights), P(ModeModelWeightsT), P(ModeTrainArgs), c_vp, c_vp, P(ModeModelGrads),
                                    c_vp, c_sz, c_vp]),
    "mode_dit_forward": (C.c_int, [P(ModeDims), P(ModeModelWeights), P(ModeForwardArgs), c_vp, c_sz, c_vp]),
    "mode_bn_film_act_fwd": (C.c_int, [P(ModeBnFilmDesc), c_vp]),
    "mode_bn_workspace_bytes": (c_sz, [c_i32, c_i32, c_i32, c_i32, c_i32]),
    "mode_bn_stats": (C.c_int, [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "mode_bn_prepare": (C.c_int, [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, C.c_float, C.c_float, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz,
                                  c_vp]),
    "mode_bn_prepare_partials": (C.c_int, [c_vp, c_vp, c_i32, C.c_double, c_i32, c_vp, c_vp, C.c_float, C.c_float, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "mode_bn_film_act_bwd": (C.c_int, [P(ModeBnFilmDesc), c_vp, c_vp, c_vp, c_i32, c_i32, c_f32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "mode_stem_conv_fwd": (C.c_int, [P(ModeStemConvDesc), c_vp]),
    "mode_stem_conv_wgrad_slabs": (C.c_int, [P(ModeStemConvDesc)]),
    "mode_stem_conv_wgrad": (C.c_int, [P(ModeStemConvDesc), c_vp]),
    "mode_maxpool_nhwc_fwd": (C.c_int, [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp]),
    "mode_maxpool_nhwc_bwd": (C.c_int, [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp]),
    "mode_env_gather_noise": (C.c_int, [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, c_i32, c_f32, c_vp]),
    "mode_env_gather_warm": (C.c_int, [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_f32, c_vp]),
    "mode_env_gather_noise_cand": (C.c_int, [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, c_i32, c_f32, c_i32, c_vp]),
    "mode_env_gather_warm_cand": (C.c_int, [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_f32,
                                            c_i32, c_vp]),
    "mode_env_select": (C.c_int, [P(ModeEnvSelectDesc), c_vp]),
    "mode_env_gather_noise_bid": (C.c_int, [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, c_i32, c_f32, c_i32, c_i32, c_vp]),
    "mode_env_gather_warm_bid": (C.c_int, [c_vp, c_i32, c_i32, c_vp, c_vp, c_vp, c_i64, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_i32, c_i32, c_i32, c_f32,
                                           c_i32, c_i32, c_vp]),
    "mode_env_select_bid": (C.c_int, [P(ModeEnvBidDesc), c_vp]),
    "mode_env_commit_emit": (C.c_int, [P(ModeEnvPoolDesc), c_vp]),
    "mode_env_gather_frames": (C.c_int, [P(ModeEnvFramesDesc), c_vp]),
    "mode_env_commit_emit_ens": (C.c_int, [P(ModeEnvEnsDesc), c_vp]),
    "mode_embed_tokens_guided_fwd": (C.c_int, [P(ModeEmbedGuidedDesc), c_vp]),
    "mode_head_ddim_guided_fwd": (C.c_int, [P(ModeHeadGuidedDesc), c_vp]),
    "mode_dit_forward_guided": (C.c_int, [P(ModeDims), P(ModeModelWeights), P(ModeGuidedArgs), c_vp, c_sz, c_vp]),
    "mode_frames_preprocess": (C.c_int, [P(ModeFramePrepDesc), c_vp]),
    "mode_data_sample_windows": (C.c_int, [P(ModeDataStreamDesc), c_vp]),
    "mode_data_sample_windows_ordered": (C.c_int, [P(ModeDataOrderDesc), c_vp]),
    "mode_data_sweep_windows": (C.c_int, [P(ModeDataSweepDesc), c_vp]),
    "mode_action_error": (C.c_int, [P(ModeActionErrorDesc), c_vp]),
    "mode_data_relabel_goals": (C.c_int, [P(ModeDataGoalDesc), c_vp]),
    "mode_val_noise_levels": (C.c_int, [P(ModeValLevelsDesc), c_vp]),
    "mode_level_error": (C.c_int, [P(ModeLevelErrorDesc), c_vp]),
    "mode_edm_loss_masked": (C.c_int, [c_vp, c_vp, c_vp, c_vp, c_f32, C.c_int, C.c_int, C.c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "mode_lora_merge": (C.c_int, [P(ModeLoraDesc), c_vp]),
    "mode_lora_grad_workspace_bytes": (c_sz, [P(ModeLoraDesc)]),
    "mode_lora_grad": (C.c_int, [P(ModeLoraDesc), c_vp, c_sz, c_vp]),
    "mode_lora_fact_workspace_bytes": (c_sz, [P(ModeLoraFactDesc)]),
    "mode_lora_fact_grad": (C.c_int, [P(ModeLoraFactDesc), c_vp, c_sz, c_vp]),
    "mode_dit_backward_lora_workspace_bytes": (c_sz, [P(ModeDims), C.c_int, C.c_int]),
    "mode_dit_backward_lora": (C.c_int, [P(ModeDims), P(ModeModelWeights), P(ModeModelWeightsT), P(ModeTrainArgs), c_vp, c_vp, P(ModeModelGrads),
                                         P(ModeLoraTrain), c_vp, c_sz, c_vp]),
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load (once) and type every entry point.  Raises ModeHipUnavailable if the library or any symbol is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ModeHipUnavailable(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` or "
            f"`make -C mode_diffusion_policy_amd/csrc`. There is no CPU fallback for the MoDE denoising path.")
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as e:  # missing ROCm runtime etc.
        raise ModeHipUnavailable(f"cannot load {LIB_PATH}: {e}") from e
    for name, (res, args) in PROTOTYPES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise ModeHipUnavailable(f"{LIB_PATH} lacks symbol {name}") from e
        fn.restype, fn.argtypes = res, args
    if lib.mode_hip_version() != ABI_VERSION:
        raise ModeHipUnavailable(f"ABI version mismatch: library {lib.mode_hip_version()} != binding {ABI_VERSION}")
    for kv in filter(None, os.environ.get("MODE_HIP_OPTS", "").split(",")):     # tuning knobs of mode_set_option, e.g. "fuse_ln2=0,dn_split_k=1"
        key, _, val = kv.partition("=")
        if lib.mode_set_option(key.strip().encode(), int(val)) != 0:
            raise ValueError(f"MODE_HIP_OPTS: unknown or invalid option {kv!r}")
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().mode_hip_status_string(rc).decode()
        raise RuntimeError(f"libmode_hip {what} failed: {msg} (status {rc})")
