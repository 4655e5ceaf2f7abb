"""Training driver with the reference's command line (src/main.py:10-70, flags of src/utils.py:51-127).

    python -m bsarec_amd.main --data_dir /path/to/data/ --data_name Beauty --lr 0.0005 --alpha 0.7 --c 5 \\
        --num_attention_heads 1 --train_name BSARec_Beauty

Same flow as the reference: read `<data_dir><data_name>.txt`, build the train / valid / test splits, train with
early stopping on validation NDCG@20 (patience epochs without improvement), reload the best parameters, report the
six test metrics.  Everything numeric runs in libbsarec_hip.so; batches come from the device-resident sample table.
"""
from __future__ import annotations

import argparse
import datetime
import logging
import os
import random
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

from . import data as D
from .caser import CaserModel
from .model import MODEL_DICT as _MODEL_DICT

# --model_type -> class: the table of model.py and Caser (bsarec_amd/caser.py).  Caser is registered HERE: the key set of
# bsarec_amd.model.MODEL_DICT is pinned (tests/test_gru_cpu.py), so that table stays as it is
MODEL_DICT = dict(_MODEL_DICT, caser=CaserModel)
# ... and MODEL_DICT's key set is pinned too (tests/test_caser_cpu.py): later siblings register in a table of their own, which
# model_class consults after MODEL_DICT
from .bert4rec import BERT4RecModel
SIBLING_MODELS = {"bert4rec": BERT4RecModel}
# ... as is SIBLING_MODELS' (tests/test_cloze_cpu.py).  MODEL_REGISTRY is the open table: tests check membership in it, never its
# key set, so the next sibling adds a key here
from .fearec import FEARecModel
from .lrurec import LRURecModel
from .mamba4rec import Mamba4RecModel
MODEL_REGISTRY = {"fearec": FEARecModel, "lrurec": LRURecModel, "mamba4rec": Mamba4RecModel}
from .trainer import Trainer


def model_class(model_type: str):
    """--model_type -> class (case-insensitive): MODEL_DICT, then SIBLING_MODELS, then MODEL_REGISTRY."""
    key = model_type.lower()
    for table in (MODEL_DICT, SIBLING_MODELS, MODEL_REGISTRY):
        if key in table:
            return table[key]
    raise KeyError(model_type)


def ratio_value(lo_open: bool):
    """--global_ratio (0, 1] / --spatial_ratio [0, 1]."""
    def parse(text: str) -> float:
        try:
            r = float(text)
        except ValueError:
            raise argparse.ArgumentTypeError(f"not a number: {text!r}") from None
        if not ((0.0 < r if lo_open else 0.0 <= r) and r <= 1.0):                # (NaN fails)
            raise argparse.ArgumentTypeError(f"{r} outside {'(0' if lo_open else '[0'}, 1]")
        return r
    return parse


def positive_value(text: str) -> float:
    """--fea_topk_factor: a finite number > 0."""
    try:
        r = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a number: {text!r}") from None
    if not 0.0 < r < float("inf"):
        raise argparse.ArgumentTypeError(f"{r} is not a finite number > 0")
    return r


def radius_value(text: str) -> float:
    """--lru_r_min / --lru_r_max: a ring radius in [0, 1)."""
    try:
        r = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a number: {text!r}") from None
    if not 0.0 <= r < 1.0:                                                       # (NaN fails)
        raise argparse.ArgumentTypeError(f"{r} outside [0, 1)")
    return r


def int_choice(what: str, allowed):
    """--mamba_d_state / --mamba_d_conv / --mamba_expand / --mamba_dt_rank: an integer out of ``allowed``."""
    def parse(text: str) -> int:
        try:
            v = int(text)
        except ValueError:
            raise argparse.ArgumentTypeError(f"not an integer: {text!r}") from None
        if v not in allowed:
            raise argparse.ArgumentTypeError(f"{v}: expected {what}")
        return v
    return parse


def bool_value(text: str) -> bool:
    """--fredom: True / False."""
    if text not in ("True", "False"):
        raise argparse.ArgumentTypeError(f"expected True or False, got {text!r}")
    return text == "True"


def mask_ratio_value(text: str) -> float:
    """--mask_ratio: a share in (0, 1]."""
    try:
        r = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a number: {text!r}") from None
    if not 0.0 < r <= 1.0:
        raise argparse.ArgumentTypeError(f"{r} outside (0, 1]")
    return r


def cutoff_list(text: str) -> tuple:
    """--extra_ks: comma list of evaluation cutoffs in 1 .. BSAREC_TOPK_MAX (duplicates dropped, order kept)."""
    from ._lib import TOPK_MAX
    out = []
    for tok in (t.strip() for t in text.split(",")):
        if not tok:
            continue
        try:
            k = int(tok)
        except ValueError:
            raise argparse.ArgumentTypeError(f"not an integer cutoff: {tok!r}") from None
        if not 1 <= k <= TOPK_MAX:
            raise argparse.ArgumentTypeError(f"cutoff {k} outside 1..{TOPK_MAX}")
        if k not in out:
            out.append(k)
    return tuple(out)


def negatives_count(text: str) -> int:
    """--eval_negatives: 0 (full-catalogue ranking) .. BSAREC_NEG_MAX."""
    from ._lib import NEG_MAX
    try:
        n = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not an integer: {text!r}") from None
    if not 0 <= n <= NEG_MAX:
        raise argparse.ArgumentTypeError(f"{n} outside 0..{NEG_MAX}")
    return n


def train_negatives_count(text: str) -> int:
    """--train_negatives: 0 (full-catalogue cross-entropy) .. BSAREC_TRAIN_NEG_MAX."""
    from ._lib import TRAIN_NEG_MAX
    try:
        n = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not an integer: {text!r}") from None
    if not 0 <= n <= TRAIN_NEG_MAX:
        raise argparse.ArgumentTypeError(f"{n} outside 0..{TRAIN_NEG_MAX}")
    return n


def seed_value(text: str) -> int:
    """--eval_seed: an unsigned 64-bit integer."""
    try:
        n = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not an integer: {text!r}") from None
    if not 0 <= n < 1 << 64:
        raise argparse.ArgumentTypeError(f"{n} outside 0..2^64-1")
    return n


def parse_args(argv=None):
    """The reference's flag names and defaults (src/utils.py:53-96); BSARec-specific --c / --alpha included."""
    p = argparse.ArgumentParser()
    p.add_argument("--data_dir", default="./data/", type=str)
    p.add_argument("--output_dir", default="output/", type=str)
    p.add_argument("--data_name", default="Beauty", type=str)
    p.add_argument("--do_eval", action="store_true")
    p.add_argument("--load_model", default=None, type=str)
    p.add_argument("--train_name", default=datetime.datetime.now().strftime('%b-%d-%Y_%H-%M-%S'), type=str)
    p.add_argument("--lr", default=0.001, type=float)
    p.add_argument("--batch_size", default=256, type=int)
    p.add_argument("--epochs", default=200, type=int)
    p.add_argument("--no_cuda", action="store_true")
    p.add_argument("--log_freq", default=1, type=int)
    p.add_argument("--patience", default=10, type=int)
    p.add_argument("--num_workers", default=4, type=int)          # accepted, unused: batches are device-resident
    p.add_argument("--seed", default=42, type=int)
    p.add_argument("--weight_decay", default=0.0, type=float)
    p.add_argument("--adam_beta1", default=0.9, type=float)
    p.add_argument("--adam_beta2", default=0.999, type=float)
    p.add_argument("--gpu_id", default="0", type=str)
    p.add_argument("--model_type", default="BSARec", type=str)
    p.add_argument("--max_seq_length", default=50, type=int)
    p.add_argument("--hidden_size", default=64, type=int)
    p.add_argument("--num_hidden_layers", default=2, type=int)
    p.add_argument("--hidden_act", default="gelu", type=str)
    p.add_argument("--num_attention_heads", default=2, type=int)
    p.add_argument("--attention_probs_dropout_prob", default=0.5, type=float)
    p.add_argument("--hidden_dropout_prob", default=0.5, type=float)
    p.add_argument("--initializer_range", default=0.02, type=float)
    p.add_argument("--c", default=3, type=int)
    p.add_argument("--alpha", default=0.9, type=float)
    # not a reference flag: HR@k / NDCG@k at these cutoffs too, logged after the reference's six metrics
    p.add_argument("--extra_ks", default=(), type=cutoff_list, help="extra evaluation cutoffs, e.g. 50,100 (<= 1024)")
    # not reference flags: sampled-candidate evaluation (each answer against N sampled unseen items) instead of the full
    # ranking.  Absent unless given (argparse.SUPPRESS), so that a run without them logs the same arguments as before;
    # readers use trainer.sampled_protocol(args)
    p.add_argument("--eval_negatives", default=argparse.SUPPRESS, type=negatives_count,
                   help="rank each answer against this many sampled unseen items (0..1024; 0 = full ranking, the default)")
    p.add_argument("--eval_sampler", default=argparse.SUPPRESS, choices=("uniform", "popularity"),
                   help="how the negatives are drawn: uniform over the catalogue (default) or by training-set popularity")
    p.add_argument("--eval_seed", default=argparse.SUPPRESS, type=seed_value, help="seed of the negative draws (default: --seed)")
    # not a reference flag: how the full ranking is computed -- dense (full_logits + bsarec_topk_seen, the default) or fused
    # (bsarec_topk_full: no B x V score matrix, the same lists) or rank (bsarec_answer_rank: the answers' ranks without lists,
    # the same six metrics plus MRR).  Absent unless given, as the --eval_* flags above
    p.add_argument("--eval_full_rank", default=argparse.SUPPRESS, choices=("dense", "fused", "rank"),
                   help="full-ranking path: dense score matrix + top-k (default), fused scoring + top-k without the matrix, or "
                        "the answers' exact ranks without lists (adds MRR)")
    # not reference flags: the sampled-softmax training head (the answer against N candidates shared by the batch, logQ-corrected)
    # instead of the full-catalogue cross-entropy.  Absent unless given (argparse.SUPPRESS), as the --eval_* flags are
    p.add_argument("--train_negatives", default=argparse.SUPPRESS, type=train_negatives_count,
                   help="train with a sampled softmax over this many candidates per step (0..8192; 0 = full CE, the default)")
    p.add_argument("--train_sampler", default=argparse.SUPPRESS, choices=("uniform", "popularity"),
                   help="how the training candidates are drawn: uniform over the catalogue (default) or by training popularity")
    p.add_argument("--train_no_logq", default=argparse.SUPPRESS, action="store_true",
                   help="no logQ correction of the sampled logits")
    p.add_argument("--train_lazy_adam", default=argparse.SUPPRESS, action="store_true",
                   help="lazy (sparse) Adam for the item table: each step updates only the rows it touches (needs --train_negatives)")
    # DuoRec's flags (src/utils.py:106-111)
    p.add_argument("--tau", default=1.0, type=float)
    p.add_argument("--lmd", default=0.1, type=float)
    p.add_argument("--lmd_sem", default=0.1, type=float)
    p.add_argument("--ssl", default="us_x", type=str)
    p.add_argument("--sim", default="dot", type=str)
    # not a reference flag: DuoRec's InfoNCE terms through the HIP head (bsarec_info_nce_fwd / _bwd) instead of the restated
    # torch head.  Absent unless given (argparse.SUPPRESS), as the --eval_* flags are
    p.add_argument("--duorec_head", default=argparse.SUPPRESS, choices=("torch", "hip"),
                   help="DuoRec's contrastive head: the reference's torch code restated (default) or the HIP kernels")
    # likewise: DuoRec's supervised full-catalogue cross-entropy through bsarec_ce_head_fwd / _bwd (no B x V logits)
    p.add_argument("--duorec_ce_head", default=argparse.SUPPRESS, choices=("torch", "hip"),
                   help="DuoRec's supervised cross-entropy: torch.matmul + F.cross_entropy (default) or the HIP kernels")
    # not a reference flag: width of GRU4Rec's recurrent state (--model_type GRU4Rec).  Absent unless given, as the flags above
    p.add_argument("--gru_hidden_size", default=argparse.SUPPRESS, type=int, choices=(32, 64, 96, 128),
                   help="GRU4Rec: hidden size of the GRU layers (default 64)")
    p.add_argument("--gru_step", default=argparse.SUPPRESS, choices=("torch", "fused"),
                   help="GRU4Rec: step through autograd and torch.optim.Adam (default) or through the one-call HIP step "
                        "(lookup, Philox dropout, BPR head, item-table gradient and Adam in the library)")
    p.add_argument("--gru_loss", default=argparse.SUPPRESS, choices=("bpr", "ce", "top1", "bpr_max"),
                   help="GRU4Rec: pairwise BPR against one negative per row (default), or cross-entropy, TOP1 or BPR-max over "
                        "candidates shared by the batch (--gru_negatives)")
    p.add_argument("--gru_negatives", default=argparse.SUPPRESS, choices=("pair", "in_batch", "in_batch+sampled"),
                   help="GRU4Rec: a row's negatives -- its own sampled negative (default, with --gru_loss bpr), the other rows' "
                        "answers, or those and every row's sampled negative")
    p.add_argument("--gru_bpreg", default=argparse.SUPPRESS, type=float,
                   help="GRU4Rec: weight of BPR-max's score regulariser (default 1.0)")
    # not reference flags: the filter counts of Caser's convolution block (--model_type Caser).  Absent unless given
    p.add_argument("--caser_nh", default=argparse.SUPPRESS, type=int, choices=(4, 8, 16, 32),
                   help="Caser: horizontal filters per height (default 16)")
    p.add_argument("--caser_nv", default=argparse.SUPPRESS, type=int,
                   help="Caser: vertical filters, 1..16 (default 4)")
    p.add_argument("--caser_step", default=argparse.SUPPRESS, choices=("torch", "fused"),
                   help="Caser: step through autograd and torch.optim.Adam (default) or through the one-call HIP step "
                        "(lookup, convolutions, fc1 with Philox dropout, BPR head, item-table gradient and Adam in the library)")
    p.add_argument("--caser_user", default=argparse.SUPPRESS, action="store_true",
                   help="Caser: the personalised model -- a user embedding and a second Linear + ReLU on [z1 | P[user]] "
                        "(valid with either --caser_step)")
    # not reference flags: BERT4Rec's cloze task (--model_type BERT4Rec).  Absent unless given
    p.add_argument("--mask_ratio", default=argparse.SUPPRESS, type=mask_ratio_value,
                   help="BERT4Rec: share of the real positions replaced by the mask token in a training step (default 0.2)")
    p.add_argument("--bert_mask_slots", default=argparse.SUPPRESS, type=int,
                   help="BERT4Rec: loss positions kept per sequence (default min(L, 2 ceil(mask_ratio L)))")
    # not reference-checked flags: FEARec's layer and loss (--model_type FEARec).  Absent unless given
    p.add_argument("--global_ratio", default=argparse.SUPPRESS, type=ratio_value(True),
                   help="FEARec: share of the rfft bins in a layer's band, in (0, 1] (default 0.6)")
    p.add_argument("--spatial_ratio", default=argparse.SUPPRESS, type=ratio_value(False),
                   help="FEARec: weight of the causal softmax attention beside the autocorrelation attention, in [0, 1] (default 0.1)")
    p.add_argument("--fredom", default=argparse.SUPPRESS, type=bool_value,
                   help="FEARec: True / False, the frequency-domain regulariser of the us_x loss (default True)")
    p.add_argument("--fredom_type", default=argparse.SUPPRESS, choices=("un", "su", "us_x"),
                   help="FEARec: which views the frequency-domain regulariser compares (default us_x)")
    p.add_argument("--fea_topk_factor", default=argparse.SUPPRESS, type=positive_value,
                   help="FEARec: the layer keeps int(factor ln L) delays, clamped to 1 .. min(L, 32) (default 1.0)")
    # not reference-checked flags: the ring of LRURec's initial eigenvalues (--model_type LRURec).  Absent unless given
    p.add_argument("--lru_r_min", default=argparse.SUPPRESS, type=radius_value,
                   help="LRURec: smallest initial |lambda|, 0 <= r_min < r_max (default 0.8)")
    p.add_argument("--lru_r_max", default=argparse.SUPPRESS, type=radius_value,
                   help="LRURec: largest initial |lambda|, r_min < r_max < 1 (default 0.99)")
    p.add_argument("--lru_step", default=argparse.SUPPRESS, choices=("torch", "fused"),
                   help="LRURec: step through autograd and torch.optim.Adam (default) or through the one-call HIP step "
                        "(lookup, LayerNorms, recurrent layers, feed-forward nets with Philox dropout, CE head, item-table "
                        "gradient and Adam in the library)")
    # not reference-checked flags: the state-space layer of Mamba4Rec (--model_type Mamba4Rec).  Absent unless given
    p.add_argument("--mamba_d_state", default=argparse.SUPPRESS, type=int_choice("4, 8, 16 or 32", (4, 8, 16, 32)),
                   help="Mamba4Rec: states per channel, 4, 8, 16 or 32 (default 16)")
    p.add_argument("--mamba_d_conv", default=argparse.SUPPRESS, type=int_choice("2..4", range(2, 5)),
                   help="Mamba4Rec: taps of the causal depthwise convolution, 2..4 (default 4)")
    p.add_argument("--mamba_expand", default=argparse.SUPPRESS, type=int_choice("1 or 2", (1, 2)),
                   help="Mamba4Rec: d_inner / hidden_size, 1 or 2 (default 2)")
    p.add_argument("--mamba_dt_rank", default=argparse.SUPPRESS, type=int_choice("a multiple of 4 in 4..64", range(4, 65, 4)),
                   help="Mamba4Rec: rank of the step-size projection, a multiple of 4 in 4..64 (default 4 ceil(hidden_size / 64))")
    p.add_argument("--mamba_step", default=argparse.SUPPRESS, choices=("torch", "fused"),
                   help="Mamba4Rec: step through autograd and torch.optim.Adam (default) or through the one-call HIP step "
                        "(lookup, LayerNorms, state-space layers, feed-forward nets with Philox dropout, CE head, item-table "
                        "gradient and Adam in the library)")
    args = p.parse_args(argv)
    if not getattr(args, "lru_r_min", 0.8) < getattr(args, "lru_r_max", 0.99):
        p.error("--lru_r_min / --lru_r_max: expected 0 <= r_min < r_max < 1")
    n = getattr(args, "eval_negatives", 0)
    if n > 0 and hasattr(args, "eval_full_rank"):
        p.error("--eval_full_rank: applies to the full ranking, not to --eval_negatives > 0")
    if n > 0 and args.extra_ks and max(args.extra_ks) > n + 1:
        p.error(f"--extra_ks: cutoff {max(args.extra_ks)} exceeds the {n + 1} candidates of --eval_negatives {n}")
    return args


NDCG20 = 5        # position of NDCG@20 in the evaluation scores; extra cutoffs come after the reference's six values


def monitored_score(scores) -> np.ndarray:
    """What early stopping monitors: NDCG@20 (src/main.py:57), whatever extra cutoffs follow it."""
    return np.array(scores[NDCG20:NDCG20 + 1])


class EarlyStopping:
    """src/utils.py:129-176: stop after `patience` validations without an improvement of the monitored score
    (NDCG@20); the best parameters are kept (in memory, and on disk when a path is given)."""

    def __init__(self, checkpoint_path, logger, patience=10):
        self.checkpoint_path, self.logger, self.patience = checkpoint_path, logger, patience
        self.counter, self.best_score, self.best_state, self.early_stop = 0, None, None, False

    def __call__(self, score, model):
        if self.best_score is None or np.any(score > self.best_score):
            self.best_score = score
            self.best_state = {k: v.detach().clone() for k, v in model.state_dict().items()}
            if self.checkpoint_path:
                torch.save({k: v.cpu() for k, v in self.best_state.items()}, self.checkpoint_path)
            self.counter = 0
        else:
            self.counter += 1
            self.logger.info(f"EarlyStopping counter: {self.counter} out of {self.patience}")
            self.early_stop = self.counter >= self.patience


def run(args, user_seq, logger=None, checkpoint_path=None):
    """Train + test on the given user sequences.  Returns (test scores, info string, epochs run, seconds)."""
    logger = logger or logging.getLogger("bsarec_amd")
    random.seed(args.seed); np.random.seed(args.seed); torch.manual_seed(args.seed)
    max_item = max(max(s) for s in user_seq)
    args.item_size = max_item + 1                                   # src/main.py:23
    args.num_users = len(user_seq) + 1
    L, dev = args.max_seq_length, torch.device("cuda", torch.cuda.current_device())
    u, x, a = D.train_table(user_seq, L)
    train_dl = D.DeviceBatches(u, x, a, args.batch_size, dev, shuffle=True, seed=args.seed)
    eval_dl = D.DeviceBatches(*D.eval_table(user_seq, L, "valid"), args.batch_size, dev, shuffle=False)
    test_dl = D.DeviceBatches(*D.eval_table(user_seq, L, "test"), args.batch_size, dev, shuffle=False)
    n_users = len(user_seq)
    for split in ("valid", "test"):
        indptr, cols = D.seen_csr(user_seq, split)
        setattr(args, f"{split}_rating_matrix", sp.csr_matrix((np.ones(len(cols)), cols, indptr), shape=(n_users, args.item_size)))
    if (getattr(args, "eval_negatives", 0) > 0 and getattr(args, "eval_sampler", "uniform") == "popularity") or \
            (getattr(args, "train_negatives", 0) > 0 and getattr(args, "train_sampler", "uniform") == "popularity"):
        args.item_popularity = D.item_popularity(user_seq, args.item_size)    # training part only: one table for both splits
    model = model_class(args.model_type)(args=args)
    if getattr(model, "needs_negatives", False):
        train_dl.enable_negatives(user_seq, args.item_size)
    if getattr(model, "needs_same_target", False):
        train_dl.enable_same_target()
    model.set_seed(args.seed)
    trainer = Trainer(model, train_dl, eval_dl, test_dl, args, logger)
    if args.do_eval:
        if args.load_model is None:
            logger.info("No model input!")
            return None
        trainer.load(os.path.join(args.output_dir, args.load_model + ".pt"))
        scores, info = trainer.test(0)
        return scores, info, 0, 0.0
    stopper = EarlyStopping(checkpoint_path, logger, patience=args.patience)
    t0 = time.time()
    epochs = 0
    for epoch in range(args.epochs):
        trainer.train(epoch)
        scores, _ = trainer.valid(epoch)
        stopper(monitored_score(scores), trainer.model)             # monitors NDCG@20 (src/main.py:57)
        epochs = epoch + 1
        if stopper.early_stop:
            logger.info("Early stopping")
            break
    secs = time.time() - t0
    logger.info("---------------Test Score---------------")
    trainer.model.load_state_dict(stopper.best_state)
    scores, info = trainer.test(0)
    logger.info(args.train_name)
    logger.info(info)
    return scores, info, epochs, secs


def main(argv=None):
    args = parse_args(argv)
    os.environ["CUDA_VISIBLE_DEVICES"] = args.gpu_id
    os.makedirs(args.output_dir, exist_ok=True)
    logger = logging.getLogger("bsarec_amd." + args.train_name)      # one log file per run (src/utils.py:9-28)
    logger.setLevel(logging.INFO)
    logger.propagate = False
    fmt = logging.Formatter("%(asctime)s - %(message)s")
    for h in (logging.FileHandler(os.path.join(args.output_dir, args.train_name + ".log")), logging.StreamHandler(sys.stderr)):
        h.setFormatter(fmt)
        logger.addHandler(h)
    user_seq, _, _ = D.read_user_seqs(args.data_dir + args.data_name + ".txt")
    logger.info(str(args))
    return run(args, user_seq, logger, os.path.join(args.output_dir, args.train_name + ".pt"))


if __name__ == "__main__":
    main()
