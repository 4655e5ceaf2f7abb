"""ctypes binding of include/bsarec_hip.h.  Fails loudly: there is no CPU or PyTorch fallback."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BSAREC_LIB") or os.path.join(HERE, "libbsarec_hip.so")   # BSAREC_LIB: another build of the same ABI
MAX_LAYERS = 16
ABI_VERSION = 10
TOPK_MAX = 1024                                  # BSAREC_TOPK_MAX: the largest k of bsarec_topk_seen
NEG_MAX = 1024                                   # BSAREC_NEG_MAX: the most negatives per row of bsarec_sampled_rank
NEG_MAX_DRAWS = 1 << 20                          # BSAREC_NEG_MAX_DRAWS: draws examined before a row fails
TRAIN_NEG_MAX = 8192                             # BSAREC_TRAIN_NEG_MAX: the most candidates of the sampled-softmax head
TRAIN_NEG_SITE = 0x4E454753                      # BSAREC_TRAIN_NEG_SITE: Philox counter word 2 of its draws
CLOZE_SITE = 0x434C4F5A                          # BSAREC_CLOZE_SITE: Philox counter word 2 of BERT4Rec's masking draws

(BUF_LAYER_OUT, BUF_LOGITS, BUF_LOSS, BUF_DSP, BUF_HMIX, BUF_PROBS, BUF_DLAYER_IN, BUF_LOSS_ROWS, BUF_CTX,
 BUF_DLOGITS, BUF_TRAIN_CAND, BUF_TRAIN_CORR, BUF_TRAIN_LOGITS, BUF_TRAIN_DLOGITS, BUF_DROP_BITS) = range(15)
K_NONE, K_FFN1, K_FFN2, K_QKV, K_LOGITS, K_DU, K_DW1, K_FUSED_FWD, K_FUSED_BWD = range(9)

LAYER_FIELDS = ["sqrt_beta", "filter_ln_w", "filter_ln_b", "query_w", "query_b", "key_w", "key_b", "value_w", "value_b",
                "dense_w", "dense_b", "attn_ln_w", "attn_ln_b", "ffn1_w", "ffn1_b", "ffn2_w", "ffn2_b", "ffn_ln_w",
                "ffn_ln_b"]
# C field name -> state_dict suffix under item_encoder.blocks.{l}.
LAYER_KEYS = {
    "sqrt_beta": "layer.filter_layer.sqrt_beta",
    "filter_ln_w": "layer.filter_layer.LayerNorm.weight", "filter_ln_b": "layer.filter_layer.LayerNorm.bias",
    "query_w": "layer.attention_layer.query.weight", "query_b": "layer.attention_layer.query.bias",
    "key_w": "layer.attention_layer.key.weight", "key_b": "layer.attention_layer.key.bias",
    "value_w": "layer.attention_layer.value.weight", "value_b": "layer.attention_layer.value.bias",
    "dense_w": "layer.attention_layer.dense.weight", "dense_b": "layer.attention_layer.dense.bias",
    "attn_ln_w": "layer.attention_layer.LayerNorm.weight", "attn_ln_b": "layer.attention_layer.LayerNorm.bias",
    "ffn1_w": "feed_forward.dense_1.weight", "ffn1_b": "feed_forward.dense_1.bias",
    "ffn2_w": "feed_forward.dense_2.weight", "ffn2_b": "feed_forward.dense_2.bias",
    "ffn_ln_w": "feed_forward.LayerNorm.weight", "ffn_ln_b": "feed_forward.LayerNorm.bias",
}
OPTIONAL_LAYER_KEYS = {"filter_cw": "layer.filter_layer.complex_weight"}      # sibling model FMLPRec only
TOP_KEYS = {"item_emb": "item_embeddings.weight", "pos_emb": "position_embeddings.weight",
            "ln_w": "LayerNorm.weight", "ln_b": "LayerNorm.bias"}


class Config(C.Structure):
    _fields_ = [("batch", C.c_int), ("seq_len", C.c_int), ("hidden", C.c_int), ("heads", C.c_int), ("layers", C.c_int),
                ("item_size", C.c_int), ("cutoff_bins", C.c_int), ("alpha", C.c_float), ("ln_eps", C.c_float),
                ("p_hidden", C.c_float), ("p_attn", C.c_float), ("filter_kind", C.c_int),
                # per-plan options, 0 = default (include/bsarec_hip.h)
                ("hidden_act", C.c_int), ("storage", C.c_int), ("no_fused", C.c_int), ("no_prune_top", C.c_int),
                ("dw_tiled", C.c_int), ("splits", C.c_int), ("top_slabs", C.c_int), ("separate_embed", C.c_int),
                ("separate_top", C.c_int), ("chain_kernels", C.c_int), ("x3_products", C.c_int),
                # sampled-softmax training head (0 = full-catalogue CE)
                ("train_negatives", C.c_int), ("train_sampler", C.c_int), ("train_no_logq", C.c_int),
                # lazy (sparse) Adam for the item table under the sampled head (0 = dense Adam)
                ("train_lazy_adam", C.c_int),
                # fp32 fused block kernels read the Linear weights from their fragment-ordered image (csrc/wimage.h)
                ("weight_image", C.c_int)]


TRAIN_FIELDS = ("train_negatives", "train_sampler", "train_no_logq")
TRAIN_SAMPLERS = {"uniform": 0, "popularity": 1}


OPTION_FIELDS = ("storage", "no_fused", "no_prune_top", "dw_tiled", "splits", "top_slabs", "separate_embed", "separate_top", "chain_kernels", "x3_products",
                 "weight_image")
# options a plan takes through a setter after its creation, not through bsarec_config_t (bsarec_plan_set_drop_bits)
PLAN_SETTERS = ("drop_bits",)
HIDDEN_ACTS = {"gelu": 0, "relu": 1, "swish": 2, "tanh": 3, "sigmoid": 4}      # src/model/_modules.py:38-45

# Plan options the HOST gives to plans it creates from now on.  The C ABI has no process-wide state: these are Python
# defaults (test / bench shims and the environment knobs of INTEGRATION.md), copied into bsarec_config_t per plan.
_defaults = {k: 0 for k in OPTION_FIELDS + PLAN_SETTERS}
_defaults["weight_image"] = 1        # on wherever the library can use it (fp32 plans at the fused shape), ignored elsewhere
_defaults["drop_bits"] = 1           # fused plans: the backward reads the forward's dropout keep bits (csrc/drop_bits.h)


def _env_defaults():
    e = os.environ
    d = {}
    if e.get("BSAREC_DW") == "tiled":
        d["dw_tiled"] = 1
    if e.get("BSAREC_PRUNE_TOP") == "0":
        d["no_prune_top"] = 1
    if e.get("BSAREC_EMBED_IN_BLOCK") == "0":
        d["separate_embed"] = 1
    if e.get("BSAREC_TOP_TAIL") == "0":
        d["separate_top"] = 1
    if e.get("BSAREC_FUSED") == "0":
        d["no_fused"] = 1
    if e.get("BSAREC_BLOCK_KERNELS") == "chain":
        d["chain_kernels"] = 1
    if e.get("BSAREC_PRODUCTS") == "bf16x3":
        d["x3_products"] = 1
    for env, key, hi in (("BSAREC_TOP_SLABS", "top_slabs", 16), ("BSAREC_SPLITS", "splits", 1024)):
        if e.get(env, "").isdigit() and 1 <= int(e[env]) <= hi:
            d[key] = int(e[env])
    if e.get("BSAREC_STORAGE") == "bf16":
        d["storage"] = 1
    if e.get("BSAREC_WEIGHT_IMAGE") == "0":
        d["weight_image"] = 0
    if e.get("BSAREC_DROP_BITS") == "0":
        d["drop_bits"] = 0
    return d


def set_default_options(**kw):
    """Test / bench shim: options of the plans created after this call (e.g. ``no_prune_top=1``).  Returns the
    previous values of the keys it changed."""
    old = {}
    for k, v in kw.items():
        if k not in _defaults:
            raise KeyError(k)
        old[k] = _defaults[k]
        _defaults[k] = int(v)
    return old


def default_options():
    d = dict(_defaults)
    d.update(_env_defaults())
    return d


class Layer(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in LAYER_FIELDS] + [("filter_cw", C.c_void_p)]


class Tensors(C.Structure):
    _fields_ = [("item_emb", C.c_void_p), ("pos_emb", C.c_void_p), ("ln_w", C.c_void_p), ("ln_b", C.c_void_p),
                ("layer", Layer * MAX_LAYERS)]


class Adam(C.Structure):
    """bsarec_adam_t"""
    _fields_ = [("params", C.c_void_p), ("grads", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("n", C.c_long), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("weight_decay", C.c_float), ("grad_scale", C.c_float), ("shadow_bf16", C.c_void_p), ("shadow_from", C.c_long),
                ("grads2", C.c_void_p), ("grads2_n", C.c_long), ("n_grad_srcs", C.c_int), ("grad_srcs", C.c_void_p * 8),
                ("wimage_plan", C.c_void_p)]


class Comm(C.Structure):
    """bsarec_comm_t (include/bsarec_comm.h)"""
    _fields_ = [("rank", C.c_int), ("world", C.c_int), ("flags", C.c_void_p * 8), ("epoch", C.c_void_p),
                ("error", C.c_void_p), ("timeout_ms", C.c_int)]


class GruConfig(C.Structure):
    """bsarec_gru_config_t"""
    _fields_ = [("batch", C.c_int), ("seq_len", C.c_int), ("input_size", C.c_int), ("hidden_size", C.c_int),
                ("num_layers", C.c_int), ("out_size", C.c_int)]


class Gru4RecConfig(C.Structure):
    """bsarec_gru4rec_config_t"""
    _fields_ = [("gru", GruConfig), ("item_size", C.c_int), ("dropout", C.c_float)]


class Gru4RecHead(C.Structure):
    """bsarec_gru4rec_head_t"""
    _fields_ = [("loss", C.c_int), ("candidates", C.c_int), ("bpreg", C.c_float)]


class CaserConfig(C.Structure):
    """bsarec_caser_config_t"""
    _fields_ = [("batch", C.c_int), ("seq_len", C.c_int), ("width", C.c_int), ("n_h", C.c_int), ("n_v", C.c_int)]


class CaserStepConfig(C.Structure):
    """bsarec_caser_step_config_t"""
    _fields_ = [("conv", CaserConfig), ("item_size", C.c_int), ("dropout", C.c_float)]


class CaserUserStepConfig(C.Structure):
    """bsarec_caser_user_step_config_t"""
    _fields_ = [("step", CaserStepConfig), ("num_users", C.c_int)]


class FeaAttnConfig(C.Structure):
    """bsarec_fea_attn_config_t"""
    _fields_ = [("batch", C.c_int), ("seq_len", C.c_int), ("width", C.c_int), ("lo", C.c_int), ("hi", C.c_int),
                ("topk", C.c_int), ("train", C.c_int)]


class LruConfig(C.Structure):
    """bsarec_lru_config_t"""
    _fields_ = [("batch", C.c_int), ("seq_len", C.c_int), ("width", C.c_int)]


class LruRecConfig(C.Structure):
    """bsarec_lrurec_config_t"""
    _fields_ = [("lru", LruConfig), ("layers", C.c_int), ("item_size", C.c_int), ("dropout", C.c_float), ("ln_eps", C.c_float)]


class MambaConfig(C.Structure):
    """bsarec_mamba_config_t"""
    _fields_ = [("batch", C.c_int), ("seq_len", C.c_int), ("width", C.c_int), ("expand", C.c_int), ("d_state", C.c_int),
                ("d_conv", C.c_int), ("dt_rank", C.c_int)]


class Mamba4RecConfig(C.Structure):
    """bsarec_mamba4rec_config_t"""
    _fields_ = [("mamba", MambaConfig), ("layers", C.c_int), ("item_size", C.c_int), ("dropout", C.c_float), ("ln_eps", C.c_float)]


GRU4REC_CAND_MAX = 8192                        # BSAREC_GRU4REC_CAND_MAX: the most candidate columns of a GRU4Rec head
GRU4REC_LOSSES = {"ce": 1, "top1": 2, "bpr_max": 3}                 # bsarec_gru4rec_head_t.loss
GRU4REC_CANDIDATES = {"in_batch": 1, "in_batch+sampled": 2}         # bsarec_gru4rec_head_t.candidates

HOOK = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)          # bsarec_hook_t


EXPORTS = {
    "bsarec_abi_version": (C.c_int, []),
    "bsarec_workspace_bytes": (C.c_size_t, [C.POINTER(Config)]),
    "bsarec_plan_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(Config), C.POINTER(Tensors), C.POINTER(Tensors),
                                     C.POINTER(Tensors), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bsarec_shadow_refresh": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bsarec_wimage_refresh": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bsarec_wimage_floats": (C.c_long, [C.POINTER(Config)]),
    "bsarec_wimage_offset": (C.c_long, [C.c_int] * 5),
    "bsarec_plan_set_dense_grad_hook": (C.c_int, [C.c_void_p, HOOK, C.c_void_p, C.c_void_p]),
    "bsarec_plan_set_train_sampler": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bsarec_plan_set_drop_bits": (C.c_int, [C.c_void_p, C.c_int]),
    "bsarec_plan_set_bidirectional": (C.c_int, [C.c_void_p, C.c_int]),
    "bsarec_drop_bits_bytes": (C.c_long, [C.POINTER(Config)]),
    "bsarec_drop_bits_hidden_bit": (C.c_long, [C.c_int, C.c_long, C.c_long, C.c_int]),
    "bsarec_drop_bits_attn_bit": (C.c_long, [C.c_long, C.c_int, C.c_long, C.c_int, C.c_int, C.c_int]),
    "bsarec_buffer_is_bf16": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "bsarec_plan_is_fused": (C.c_int, [C.c_void_p]),
    "bsarec_config_is_fused": (C.c_int, [C.c_void_p]),
    "bsarec_plan_destroy": (None, [C.c_void_p]),
    "bsarec_buffer_offset": (C.c_long, [C.c_void_p, C.c_int, C.c_int]),
    "bsarec_step_begin": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bsarec_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "bsarec_forward_last": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "bsarec_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "bsarec_loss_bce": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bsarec_loss_logsig": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bsarec_logits": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bsarec_backward": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bsarec_backward_seq": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "bsarec_backward_seq_multi": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "bsarec_adam_step": (C.c_int, [C.POINTER(Adam), C.c_void_p, C.c_void_p]),
    "bsarec_train_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Adam), C.c_void_p]),
    "bsarec_gather_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "bsarec_train_step_indexed": (C.c_int, [C.c_void_p] * 4 + [C.c_long] + [C.c_void_p] * 3 + [C.POINTER(Adam), C.c_void_p]),
    "bsarec_grad_step_indexed": (C.c_int, [C.c_void_p] * 4 + [C.c_long] + [C.c_void_p] * 3 + [C.c_float] * 3 + [C.c_void_p]),
    "bsarec_adam_apply": (C.c_int, [C.POINTER(Adam), C.c_void_p, C.c_void_p]),
    "bsarec_mask_seen": (C.c_int, [C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bsarec_topk_seen": (C.c_int, [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "bsarec_sampled_rank": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5 +
                            [C.c_int, C.c_uint64, C.c_uint32] + [C.c_void_p] * 4),
    "bsarec_topk_full_workspace_bytes": (C.c_long, [C.c_int] * 5),
    "bsarec_topk_full": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3 +
                         [C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bsarec_topk_full_range": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_int, C.c_long, C.c_int] + [C.c_void_p] * 3 +
                               [C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bsarec_answer_rank": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 7),
    "bsarec_answer_rank_range": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_int, C.c_long, C.c_int] +
                                 [C.c_void_p] * 8),
    "bsarec_answer_score_range": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_int, C.c_long, C.c_int] +
                                  [C.c_void_p] * 6),
    "bsarec_info_nce_workspace_bytes": (C.c_long, [C.c_int] * 3),
    "bsarec_info_nce_fwd": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_float, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]),
    "bsarec_info_nce_bwd": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_float, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bsarec_ce_head_workspace_bytes": (C.c_long, [C.c_int] * 3),
    "bsarec_ce_head_fwd": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]),
    "bsarec_ce_head_bwd": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bsarec_ce_head_range_workspace_bytes": (C.c_long, [C.c_int] * 3),
    "bsarec_ce_head_range_stats": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_int, C.c_long, C.c_long, C.c_int,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]),
    "bsarec_ce_head_range_merge": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    "bsarec_ce_head_range_bwd": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_int, C.c_long, C.c_long, C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bsarec_cloze_mask": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int64] + [C.c_void_p] * 6),
    "bsarec_cloze_head_workspace_bytes": (C.c_long, [C.c_int] * 3),
    "bsarec_cloze_head_fwd": (C.c_int, [C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_int, C.c_int, C.c_int] +
                              [C.c_void_p] * 6 + [C.c_long, C.c_void_p]),
    "bsarec_cloze_head_bwd": (C.c_int, [C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_int, C.c_int, C.c_int] +
                              [C.c_void_p] * 5 + [C.c_long, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bsarec_gru_weight_floats": (C.c_long, [C.POINTER(GruConfig)]),
    "bsarec_gru_workspace_bytes": (C.c_long, [C.POINTER(GruConfig), C.c_int]),
    "bsarec_gru_fwd": (C.c_int, [C.POINTER(GruConfig), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_long,
                                 C.c_void_p]),
    "bsarec_gru_bwd": (C.c_int, [C.POINTER(GruConfig), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p,
                                 C.c_void_p, C.c_void_p]),
    "bsarec_gru4rec_workspace_bytes": (C.c_long, [C.POINTER(Gru4RecConfig)]),
    "bsarec_gru4rec_loss_grad": (C.c_int, [C.POINTER(Gru4RecConfig)] + [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 4 +
                                 [C.c_long, C.c_void_p]),
    "bsarec_gru4rec_train_step": (C.c_int, [C.POINTER(Gru4RecConfig)] + [C.c_void_p] * 3 + [C.POINTER(Adam)] * 2 +
                                  [C.c_void_p] * 3 + [C.c_long, C.c_void_p]),
    "bsarec_gru4rec_cand_head_workspace_bytes": (C.c_long, [C.c_int, C.c_int, C.POINTER(Gru4RecHead)]),
    "bsarec_gru4rec_cand_head": (C.c_int, [C.c_void_p] * 4 + [C.c_int] * 3 + [C.POINTER(Gru4RecHead)] + [C.c_void_p] * 4 +
                                 [C.c_long, C.c_void_p]),
    "bsarec_gru4rec_cand_workspace_bytes": (C.c_long, [C.POINTER(Gru4RecConfig), C.POINTER(Gru4RecHead)]),
    "bsarec_gru4rec_cand_loss_grad": (C.c_int, [C.POINTER(Gru4RecConfig)] + [C.c_void_p] * 6 + [C.c_int] + [C.c_void_p] * 4 +
                                      [C.c_long, C.c_void_p, C.POINTER(Gru4RecHead)]),
    "bsarec_gru4rec_cand_train_step": (C.c_int, [C.POINTER(Gru4RecConfig)] + [C.c_void_p] * 3 + [C.POINTER(Adam)] * 2 +
                                       [C.c_void_p] * 3 + [C.c_long, C.c_void_p, C.POINTER(Gru4RecHead)]),
    "bsarec_caser_weight_floats": (C.c_long, [C.POINTER(CaserConfig)]),
    "bsarec_caser_workspace_bytes": (C.c_long, [C.POINTER(CaserConfig), C.c_int]),
    "bsarec_caser_fwd": (C.c_int, [C.POINTER(CaserConfig), C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_long,
                                   C.c_void_p]),
    "bsarec_caser_bwd": (C.c_int, [C.POINTER(CaserConfig), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p,
                                   C.c_void_p, C.c_void_p]),
    "bsarec_caser_fc_floats": (C.c_long, [C.POINTER(CaserConfig)]),
    "bsarec_caser_fc_workspace_bytes": (C.c_long, [C.c_int] * 3),
    "bsarec_caser_fc_fwd": (C.c_int, [C.c_int] * 3 + [C.c_void_p] * 3 + [C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_long,
                                      C.c_void_p]),
    "bsarec_caser_fc_bwd": (C.c_int, [C.c_int] * 3 + [C.c_void_p] * 5 + [C.c_int, C.c_float] + [C.c_void_p] * 3 +
                            [C.c_long, C.c_void_p]),
    "bsarec_caser_step_workspace_bytes": (C.c_long, [C.POINTER(CaserStepConfig)]),
    "bsarec_caser_loss_grad": (C.c_int, [C.POINTER(CaserStepConfig)] + [C.c_void_p] * 7 + [C.c_int] + [C.c_void_p] * 5 +
                               [C.c_long, C.c_void_p]),
    "bsarec_caser_train_step": (C.c_int, [C.POINTER(CaserStepConfig)] + [C.c_void_p] * 3 + [C.POINTER(Adam)] * 3 +
                                [C.c_void_p] * 3 + [C.c_long, C.c_void_p]),
    "bsarec_caser_fc2_floats": (C.c_long, [C.POINTER(CaserConfig)]),
    "bsarec_caser_user_step_workspace_bytes": (C.c_long, [C.POINTER(CaserUserStepConfig)]),
    "bsarec_caser_user_loss_grad": (C.c_int, [C.POINTER(CaserUserStepConfig)] + [C.c_void_p] * 10 + [C.c_int] +
                                    [C.c_void_p] * 7 + [C.c_long, C.c_void_p]),
    "bsarec_caser_user_train_step": (C.c_int, [C.POINTER(CaserUserStepConfig)] + [C.c_void_p] * 4 + [C.POINTER(Adam)] * 5 +
                                     [C.c_void_p] * 3 + [C.c_long, C.c_void_p]),
    "bsarec_fea_attn_workspace_bytes": (C.c_long, [C.POINTER(FeaAttnConfig)]),
    "bsarec_fea_attn_fwd": (C.c_int, [C.POINTER(FeaAttnConfig)] + [C.c_void_p] * 5 + [C.c_long, C.c_void_p]),
    "bsarec_fea_attn_bwd": (C.c_int, [C.POINTER(FeaAttnConfig)] + [C.c_void_p] * 5 + [C.c_long] + [C.c_void_p] * 4),
    "bsarec_lru_weight_floats": (C.c_long, [C.POINTER(LruConfig)]),
    "bsarec_lru_workspace_bytes": (C.c_long, [C.POINTER(LruConfig), C.c_int]),
    "bsarec_lru_fwd": (C.c_int, [C.POINTER(LruConfig)] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]),
    "bsarec_lru_bwd": (C.c_int, [C.POINTER(LruConfig)] + [C.c_void_p] * 5 + [C.c_long] + [C.c_void_p] * 3),
    "bsarec_lrurec_weight_floats": (C.c_long, [C.POINTER(LruRecConfig)]),
    "bsarec_lrurec_workspace_bytes": (C.c_long, [C.POINTER(LruRecConfig)]),
    "bsarec_lrurec_loss_grad": (C.c_int, [C.POINTER(LruRecConfig)] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 4 +
                                [C.c_long, C.c_void_p]),
    "bsarec_lrurec_train_step": (C.c_int, [C.POINTER(LruRecConfig)] + [C.c_void_p] * 2 + [C.POINTER(Adam)] * 2 +
                                 [C.c_void_p] * 3 + [C.c_long, C.c_void_p]),
    "bsarec_mamba_weight_floats": (C.c_long, [C.POINTER(MambaConfig)]),
    "bsarec_mamba_workspace_bytes": (C.c_long, [C.POINTER(MambaConfig), C.c_int]),
    "bsarec_mamba_fwd": (C.c_int, [C.POINTER(MambaConfig)] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]),
    "bsarec_mamba_bwd": (C.c_int, [C.POINTER(MambaConfig)] + [C.c_void_p] * 5 + [C.c_long] + [C.c_void_p] * 3),
    "bsarec_mamba4rec_weight_floats": (C.c_long, [C.POINTER(Mamba4RecConfig)]),
    "bsarec_mamba4rec_workspace_bytes": (C.c_long, [C.POINTER(Mamba4RecConfig)]),
    "bsarec_mamba4rec_loss_grad": (C.c_int, [C.POINTER(Mamba4RecConfig)] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 4 +
                                   [C.c_long, C.c_void_p]),
    "bsarec_mamba4rec_train_step": (C.c_int, [C.POINTER(Mamba4RecConfig)] + [C.c_void_p] * 2 + [C.POINTER(Adam)] * 2 +
                                    [C.c_void_p] * 3 + [C.c_long, C.c_void_p]),
    "bsarec_freq_layer_fwd": (C.c_int, [C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_float, C.c_float, C.c_void_p, C.c_int,
                                                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bsarec_freq_layer_bwd_scratch_floats": (C.c_long, [C.c_int, C.c_int, C.c_int]),
    "bsarec_freq_layer_bwd": (C.c_int, [C.c_void_p] * 7 + [C.c_int] * 4 + [C.c_float, C.c_void_p, C.c_int] +
                              [C.c_void_p] * 6),
    "bsarec_profile_select": (C.c_int, [C.c_void_p, C.c_int]),
    "bsarec_debug_stamps": (C.c_int, [C.c_void_p, C.c_void_p]),
    "bsarec_profile_read": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "bsarec_profile_event_overhead": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double)]),
}

# include/bsarec_comm.h
COMM_EXPORTS = {
    "bsarec_comm_alloc": (C.c_int, [C.POINTER(C.c_void_p), C.c_size_t, C.c_int]),
    "bsarec_comm_free": (C.c_int, [C.c_void_p]),
    "bsarec_comm_export": (C.c_int, [C.c_void_p, C.c_char_p]),
    "bsarec_comm_import": (C.c_int, [C.c_char_p, C.POINTER(C.c_void_p)]),
    "bsarec_comm_release": (C.c_int, [C.c_void_p]),
    "bsarec_comm_barrier": (C.c_int, [C.POINTER(Comm), C.c_void_p]),
}

# include/bsarec_shard.h
PTRS8 = C.c_void_p * 8
SHARD_EXPORTS = {
    "bsarec_shard_gather_rows": (C.c_int, [C.c_void_p, C.c_long, C.POINTER(PTRS8), C.c_int, C.c_long, C.c_long, C.c_int,
                                           C.c_void_p, C.c_void_p, C.c_void_p]),
    "bsarec_shard_logits": (C.c_int, [C.c_void_p, C.c_long, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_long,
                                      C.c_void_p]),
    "bsarec_shard_ce_stats": (C.c_int, [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_long, C.c_void_p,
                                        C.c_void_p]),
    "bsarec_shard_ce_grad": (C.c_int, [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_long, C.c_void_p,
                                       C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bsarec_shard_head_bwd_scratch_floats": (C.c_long, [C.c_int, C.c_int, C.c_int]),
    "bsarec_shard_head_bwd": (C.c_int, [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bsarec_shard_scatter_rows": (C.c_int, [C.c_void_p, C.c_long, C.c_int, C.POINTER(PTRS8), C.c_long, C.c_long, C.c_long,
                                            C.c_int, C.c_void_p, C.c_void_p]),
    # sampled-softmax head of the sharded step, lazy Adam of the shard
    "bsarec_shard_ssm_draw": (C.c_int, [C.c_uint64, C.c_void_p, C.c_int, C.c_long, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]),
    "bsarec_shard_ssm_gather": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(PTRS8), C.c_int, C.c_long, C.c_long,
                                          C.c_int, C.c_void_p, C.c_void_p]),
    "bsarec_shard_ssm_head": (C.c_int, [C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_int, C.c_long, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "bsarec_shard_ssm_loss": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
    "bsarec_shard_ssm_bwd_scratch_floats": (C.c_long, [C.c_int, C.c_int, C.c_int]),
    "bsarec_shard_ssm_bwd": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p,
                                       C.c_long, C.c_void_p, C.c_void_p, C.c_void_p]),
    "bsarec_shard_ssm_pull": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(PTRS8), C.c_long, C.c_long,
                                        C.c_long, C.c_int, C.c_void_p, C.c_void_p]),
    "bsarec_shard_lazy_mark": (C.c_int, [C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_long, C.c_long,
                                         C.c_long, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "bsarec_shard_lazy_adam": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float,
                                         C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]),
}

_lib = None


def source_sha16() -> str:
    """First 16 hex digits of the sha256 over the library's sources (csrc/ + the header): the tag that ties an offline
    rocprofv3 profile under profiles/ to the build it was taken with."""
    import hashlib
    h = hashlib.sha256()
    src = os.path.join(HERE, "csrc")
    for f in sorted(os.listdir(src)) + [os.path.join(os.path.dirname(HERE), "include", "bsarec_hip.h"),
                                         os.path.join(HERE, "build.py")]:          # (build.py: the compiler flags)
        with open(f if os.path.isabs(f) else os.path.join(src, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def load():
    """dlopen the HIP library and bind every symbol of the header.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m bsarec_amd.build` (hipcc, gfx950). "
            "bsarec_amd has no fallback path.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in list(EXPORTS.items()) + list(COMM_EXPORTS.items()) + list(SHARD_EXPORTS.items()):
        fn = getattr(lib, name)       # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    if lib.bsarec_abi_version() != ABI_VERSION:
        raise RuntimeError("libbsarec_hip.so ABI version mismatch: rebuild with `python -m bsarec_amd.build --force`")
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        kind = "invalid argument / unsupported shape" if rc < 0 else "hipError_t"
        raise RuntimeError(f"{what} failed: {kind} {rc}")
