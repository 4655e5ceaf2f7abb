/* bsarec_hip.h -- C ABI of the MI355X (gfx950) BSARec training hot path.
 *
 * The reference (Sun-Sir/BSARec) is pure Python/PyTorch and has no FFI: the seam this library
 * slots under is the Python object protocol between Trainer and the model
 * (src/trainers.py:94-116 -> src/model/bsarec.py:16-37).  Each entry point below names the
 * reference code it replaces.  Conventions:
 *   - plain pointers and sizes only; every device buffer is allocated and owned by the caller
 *     (PyTorch in the shipped host code); the library never allocates or frees device memory;
 *   - all work is enqueued on the caller's hipStream_t (passed as void*), never synchronises, and
 *     can therefore be captured into a hipGraph (the two exceptions say so: bsarec_plan_create
 *     synchronises once, bsarec_profile_read waits for its own events);
 *   - no process-wide mutable state: every option is a field of bsarec_config_t and belongs to the
 *     plan, profiling / diagnostic state is per plan; two plans with different options may be
 *     driven from different threads;
 *   - return value: 0 = OK, < 0 = invalid argument / unsupported shape (nothing was launched),
 *     > 0 = hipError_t of a failed launch;
 *   - fp32 arithmetic and fp32 tensors by default (the reference's arithmetic type); cfg.storage = 1 keeps the
 *     saved activations / inter-block gradients / a shadow of the Linear weights in bf16 and multiplies with
 *     bf16 MFMAs (fp32 accumulation, fp32 masters, LayerNorm / softmax / loss / Adam in fp32) at the fused
 *     shape, and multiplies with bf16 MFMAs on operands rounded while they are staged (fp32 tensors) at every
 *     other shape; ids and answers are int64 as produced by the reference DataLoader (src/dataset.py:108-115).
 */
#ifndef BSAREC_HIP_H
#define BSAREC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSAREC_MAX_LAYERS 16
#define BSAREC_ABI_VERSION 10

/* Hyper-parameters the reference model reads from `args`
 * (src/utils.py:83-96; src/model/bsarec.py:71-88; src/model/_modules.py:79-87). */
typedef struct {
    int batch;          /* B: sequences per call (src/utils.py:67) */
    int seq_len;        /* L = max_seq_length */
    int hidden;         /* d = hidden_size, multiple of 4, <= 256 */
    int heads;          /* num_attention_heads; d/heads multiple of 4 */
    int layers;         /* num_hidden_layers, <= BSAREC_MAX_LAYERS */
    int item_size;      /* V = max item id + 1 (row 0 = padding, still a class) */
    int cutoff_bins;    /* min(c//2 + 1, L//2 + 1): rFFT bins kept by FrequencyLayer */
    float alpha;        /* BSARecLayer mix (src/model/bsarec.py:78) */
    float ln_eps;       /* 1e-12 */
    float p_hidden;     /* hidden_dropout_prob */
    float p_attn;       /* attention_probs_dropout_prob */
    int filter_kind;    /* 0: BSARec's FrequencyLayer (low-pass + beta^2 high-pass, src/model/bsarec.py:90-104);
                         * 1: FMLPRec's learnable complex filter irfft(rfft(x) * W) (src/model/fmlprec.py:96-113): the
                         *    layer's filter_cw tensor is used, cutoff_bins must be L/2 + 1, generic kernels only */
    /* ---- per-plan options; 0 selects the default everywhere, so a zero-filled tail is a valid configuration ---- */
    int hidden_act;     /* FeedForward activation (src/model/_modules.py:38-59, ACT2FN): 0 gelu (erf form, the default), 1 relu,
                         * 2 swish, 3 tanh, 4 sigmoid.  Non-default activations run on the generic tiled kernels */
    int storage;        /* 0: fp32 everywhere (the reference's arithmetic); 1 (config C2 / the bf16 half of C3): bf16 MFMA with fp32
                         *    accumulation, fp32 master weights, fp32 LayerNorm / softmax / loss head / Adam.  At the fused shape
                         *    (hidden = 64, L <= 64) the saved activations, the inter-block gradients and a shadow of the Linear weights
                         *    are STORED as bf16; at every other shape (generic tiled kernels) all tensors stay fp32 and the operands of
                         *    every matrix product of the block stack are rounded to bf16 as they are staged into LDS
                         *    (bsarec_buffer_is_bf16 = 0 everywhere, `shadow` unused) */
    int no_fused;       /* 1: never take the fused per-sequence block kernels (hidden = 64, L <= 64, cutoff_bins <= 8) */
    int no_prune_top;   /* 1: bsarec_forward_last evaluates the full top block (no one-row evaluation) */
    int dw_tiled;       /* 1: LDS-tiled grouped weight-gradient kernel at the fused shape too (default: direct split-K) */
    int splits;         /* split-K slab slices of the weight-gradient products (0: 32 at the fused shape, 40 elsewhere) */
    int top_slabs;      /* slab slices of the one-row top block's weight-gradient products (0: 2) */
    int separate_embed; /* 1: the embedding front-end runs as its own kernel on the fused path too */
    int separate_top;   /* 1: the one-row top block of the loss path runs as its own kernels instead of as the tail /
                         * head of the launches of the block below it */
    int chain_kernels;  /* 1: the register-chain forward block kernel (fused_chain.h: lane = token, accumulators chained as MFMA
                         * operands, LDS weight ring) instead of the LDS-phase kernel (fused_layer.h) at the fused shape in
                         * fp32; measured equal in speed on MI355X, kept selectable */
    int x3_products;    /* 1: the fused block kernels evaluate every fp32 product of their matrix multiplications on the bf16
                         * matrix cores as six bf16 x bf16 partial products of the operands' exact three-way bf16 splits
                         * (fp32 accumulation; error <= 2^-26 per product, below fp32 rounding; fp32 tensors, fp32 storage).
                         * 0 (default): v_mfma_f32_32x32x2_f32.  Ignored under storage = 1 */
    int train_negatives;  /* 0: the loss is the full-catalogue CE.  1 .. BSAREC_TRAIN_NEG_MAX: the sampled-softmax head (below) for
                           * every entry point that runs the loss (bsarec_loss, bsarec_train_step, bsarec_train_step_indexed,
                           * bsarec_grad_step_indexed); bsarec_logits stays full-catalogue.  fp32 only (storage = 1 is refused) */
    int train_sampler;    /* sampled head: 0 uniform over [1, V); 1 popularity (bsarec_plan_set_train_sampler) */
    int train_no_logq;    /* sampled head: 1 = no logQ correction */
    int train_lazy_adam;  /* sampled head: 1 = lazy (sparse) Adam for the item table in bsarec_train_step and
                           * bsarec_train_step_indexed (below); 0 (default): dense Adam.  Needs train_negatives > 0 */
    int weight_image;     /* 1: the fp32 fused block kernels read the Linear weights from a second copy in the order of their MFMA
                           * operand fragments, the fragment image (one coalesced 16-byte-per-lane load per fragment; same
                           * values, same registers, same results bit for bit).  Takes effect at the fused shape with storage = 0,
                           * x3_products = 0, chain_kernels = 0, filter_kind = 0 (bsarec_wimage_floats > 0) and is ignored
                           * elsewhere.  The image is the caller's memory (bsarec_plan_create, `shadow`); bsarec_train_step and
                           * bsarec_train_step_indexed keep it current themselves, bsarec_adam_step / _apply through
                           * bsarec_adam_t.wimage_plan; after any other change of the masters the caller runs
                           * bsarec_wimage_refresh before the next forward.  0: the kernels read the masters */
} bsarec_config_t;

/* The 19 tensors of one BSARecBlock, in state_dict order (+ the sibling model's filter weight)
 * (item_encoder.blocks.{l}.layer.filter_layer.* , .attention_layer.* , .feed_forward.*). */
typedef struct {
    float *sqrt_beta, *filter_ln_w, *filter_ln_b;
    float *query_w, *query_b, *key_w, *key_b, *value_w, *value_b, *dense_w, *dense_b;
    float *attn_ln_w, *attn_ln_b;
    float *ffn1_w, *ffn1_b, *ffn2_w, *ffn2_b, *ffn_ln_w, *ffn_ln_b;
    float *filter_cw;   /* filter_kind 1 only: complex_weight [L/2+1, d, 2] (re, im) as the reference stores it; else null */
} bsarec_layer_t;

/* All 4 + 19 N tensors (parameters, or their gradients) as device pointers.  Linear weights are
 * [out, in] row-major exactly as nn.Linear stores them. */
typedef struct {
    float *item_emb;    /* [V, d]  item_embeddings.weight */
    float *pos_emb;     /* [L, d]  position_embeddings.weight */
    float *ln_w, *ln_b; /* [d]     LayerNorm.{weight,bias} */
    bsarec_layer_t layer[BSAREC_MAX_LAYERS];
} bsarec_tensors_t;

/* Named device buffers inside the workspace (byte offsets via bsarec_buffer_offset). */
enum {
    BSAREC_BUF_LAYER_OUT = 0,  /* [B,L,d]   output of layer l-1 (l = 0: embedding output), l in [0, N] */
    BSAREC_BUF_LOGITS = 1,     /* [B,Vp]    full-catalogue logits, Vp = 4*ceil(V/4), pad columns = 0 */
    BSAREC_BUF_LOSS = 2,       /* [1]       mean cross-entropy */
    BSAREC_BUF_DSP = 3,        /* [B,L,d]   FrequencyLayer output of layer l (generic path only; stays on chip in the fused path) */
    BSAREC_BUF_HMIX = 4,       /* [B,L,d]   alpha*dsp + (1-alpha)*gsp of layer l */
    BSAREC_BUF_PROBS = 5,      /* [B,h,L,Lp] attention probabilities of layer l (before dropout) */
    BSAREC_BUF_DLAYER_IN = 6,  /* [B,L,d]   gradient w.r.t. layer output l (ping-pong pair: only l = 0, 1 survive backward; on the fused path l = 0 is never materialised: the bottom block emits the embedding gradient directly) */
    BSAREC_BUF_LOSS_ROWS = 7,  /* [B]       per-sequence cross-entropy */
    BSAREC_BUF_CTX = 8,        /* [B,L,d]   attention context of layer l */
    BSAREC_BUF_DLOGITS = 9,    /* [B,Vp]    d loss / d logits = (softmax - onehot(answer)) / B, pad columns = 0 (after bsarec_loss) */
    /* sampled-softmax head (cfg.train_negatives = N > 0 only; -1 otherwise), after the loss: */
    BSAREC_BUF_TRAIN_CAND = 10,    /* int32 [N]     the step's candidates n_0 .. n_N-1 */
    BSAREC_BUF_TRAIN_CORR = 11,    /* [N]           their corrections c(n_j) */
    BSAREC_BUF_TRAIN_LOGITS = 12,  /* [B, N+1]      x_b0 (answer), x_b1 .. x_bN (candidates; -inf on an accidental hit) */
    BSAREC_BUF_TRAIN_DLOGITS = 13, /* [B, N+1]      d loss / d x = (softmax - onehot_0) / B (exactly 0 on a hit) */
    BSAREC_BUF_DROP_BITS = 14      /* bytes: keep bits of layer l's dropout masks after a training forward (bsarec_drop_bits_bytes;
                                    * -1 where the plan keeps none) */
};

typedef struct bsarec_plan bsarec_plan_t;   /* host-side launch plan (no device memory of its own) */

int bsarec_abi_version(void);

/* Bytes of device workspace a plan for `cfg` needs (activations kept for backward, scratch,
 * split-K slabs, reduction job table).  0 if cfg is unsupported. */
size_t bsarec_workspace_bytes(const bsarec_config_t *cfg);

/* Device step state: 8 x uint64.  [0] seed of the Philox dropout stream, [1] forward-step counter,
 * [2] Adam step t, [3] two packed floats written by bsarec_adam_step ({lr/bc1, sqrt(bc2)}), [4] ticket counter of
 * the Adam kernel (uint32), [5], [6] beta1^t, beta2^t as doubles, [7] reserved.  The caller zero-initialises it and
 * sets [0]; kernels read/advance it on the device so a captured graph replays correctly; t = 0 restarts Adam. */
#define BSAREC_STATE_BYTES 64

/* Build a launch plan.  `params`/`grads` hold device pointers (copied into the plan); `workspace`
 * must hold bsarec_workspace_bytes(cfg) bytes, 256-byte aligned; `twiddle` is the float[2L] table
 * (cos, sin)(2 pi j / L) built on the host in double precision.  Enqueues one small H2D copy of the
 * reduction job table on `stream` and waits for it (the one synchronising call of the training path).
 * `shadow` (cfg.storage = 1 at the fused shape only, else null / ignored): the same tensor set as `params` but as bf16 arrays (uint16_t behind the
 * float* fields) -- the bf16 shadow of the fp32 masters that the MFMA products read; only the six Linear weights of
 * every layer are used.  The caller keeps it current: bsarec_shadow_refresh after it changes the masters itself, or
 * bsarec_adam_t.shadow_bf16 so that the fused Adam writes both.
 * cfg.weight_image = 1 where it takes effect (bsarec_wimage_floats(cfg) > 0): `shadow->layer[0].query_w` is instead the
 * fragment image, bsarec_wimage_floats(cfg) floats, 256-byte aligned, shared by every plan of the same parameters; no
 * other field of `shadow` is read.  Its content is the caller's to initialise (bsarec_wimage_refresh).
 * Replaces: model construction wiring of src/model/bsarec.py:8-14. */
int bsarec_plan_create(bsarec_plan_t **out, const bsarec_config_t *cfg, const bsarec_tensors_t *params,
                       const bsarec_tensors_t *grads, const bsarec_tensors_t *shadow, void *workspace,
                       size_t workspace_bytes, void *state, const float *twiddle, void *stream);
/* cfg.storage = 1: bf16 shadow <- fp32 masters for the Linear weights of every layer (one launch per layer). */
int bsarec_shadow_refresh(bsarec_plan_t *plan, void *stream);
/* cfg.weight_image = 1: fragment image <- fp32 masters for the Linear weights of every layer (one launch; nothing where the
 * plan keeps no image). */
int bsarec_wimage_refresh(bsarec_plan_t *plan, void *stream);
/* Floats of the fragment image a plan for `cfg` reads (layer after layer); 0: such a plan reads the masters; < 0: bad cfg. */
long bsarec_wimage_floats(const bsarec_config_t *cfg);
/* The image's index map: where element [n][k] of Linear weight `which` (0..5 = query, key, value, dense, dense_1, dense_2;
 * [out][in] row-major) of hidden size d lives inside a layer's image, transposed = 0 for the forward (F) and 1 for the
 * backward (T) orientation; -1 on a bad argument.  Host arithmetic only. */
long bsarec_wimage_offset(int which, int transposed, int d, int n, int k);
/* Element type of a named workspace buffer under this plan: 0 = fp32, 1 = bf16 (cfg.storage = 1: every saved
 * activation of the block stack except the last layer's output; logits, loss and the statistics stay fp32). */
int bsarec_buffer_is_bf16(const bsarec_plan_t *plan, int buffer, int layer);

/* 1 if the plan resolved to the fused per-sequence block kernels (hidden = 64, L <= 64, ...), 0 for the generic tiled kernels. */
int bsarec_plan_is_fused(const bsarec_plan_t *plan);
/* The same question before a plan exists (does cfg.storage = 1 need a `shadow`?): 1 fused, 0 generic, < 0 invalid cfg. */
int bsarec_config_is_fused(const bsarec_config_t *cfg);
void bsarec_plan_destroy(bsarec_plan_t *plan);

/* Data-parallel bucketing: the dense part of the item-table gradient, dE = dlogits^T . h_last, is complete
 * right after the logits backward -- long before the rest of the gradient.  `hook` (may be null) is called by
 * bsarec_backward / bsarec_*_step_indexed on the calling thread as soon as that kernel is ENQUEUED on `stream`, so that
 * the host can start exchanging grads->item_emb on a side stream under the whole encoder backward (record an event on
 * `stream`, let the side stream wait for it).  `lookup_grad` (may be null): [V, d] buffer that then receives the
 * lookup-path rows (the embedding scatter at the END of the backward) instead of grads->item_emb, so that the early
 * exchange is not disturbed; hand it to the update as bsarec_adam_t.grads2. */
typedef void (*bsarec_hook_t)(void *user, void *stream);
int bsarec_plan_set_dense_grad_hook(bsarec_plan_t *plan, bsarec_hook_t hook, void *user, float *lookup_grad);

/* Sampled-softmax training head (cfg.train_negatives = N > 0), opt-in beside the full-catalogue CE for large catalogues
 * (Jean et al. 2015; Yi et al. 2019).
 *   Draws: each step draws N items with replacement, shared by all B rows.  Philox4x32-10 call j = 0, 1, ... has key
 *   (lo32(state[0]), hi32(state[0])) -- the dropout key -- and counter (lo32(j), hi32(j), BSAREC_TRAIN_NEG_SITE, lo32(state[1]))
 *   -- the dropout stream's layout at a site no dropout mask uses, with the step value this step's masks use (read on the
 *   device: a captured graph replays with fresh candidates).  Uniform (train_sampler 0): draw 4j + m takes word w_m,
 *   n = 1 + ((uint64)w_m * (V - 1) >> 32).  Popularity (1): draw 2j + m takes x = w_2m | (uint64)w_2m+1 << 32, r = the high 64
 *   bits of x * T, n = the smallest i with pop_cum[i] > r (the table format of bsarec_sampled_rank: int64[V], non-decreasing,
 *   pop_cum[0] = 0, T = pop_cum[V - 1] >= 1; items of count 0 are never drawn).  Candidates depend on (seed, step, N, V, table)
 *   only.
 *   Logits: x_b0 = h_b . E[a_b] - c(a_b), x_bj = h_b . E[n_j] - c(n_j) (j = 1 .. N, candidate n_j-1), h_b = the last layer's
 *   output at position L-1, fp32 dot products; c(i) = log(N q_i), q_i = (pop_cum[i] - pop_cum[i-1]) / T, under popularity
 *   sampling with logQ on, else 0 (uniform: a constant that cancels).  Accidental hit n_j == a_b: x_bj = -inf.
 *   Loss: loss_rows[b] = logsumexp_j x_bj - x_b0 -> BSAREC_BUF_LOSS_ROWS, their mean over B -> BSAREC_BUF_LOSS.
 *   Backward (bsarec_backward and the steps): g = (softmax(x_b) - onehot_0) / B; d(h_b) = sum_c g_bc E[c]; dE[c] += g_bc h_b for
 *   every candidate column, the answers included, summed as 64-bit fixed point (2^-40) so that the step is bit-deterministic;
 *   rows that are no candidate get no head gradient (the item table's gradient is then the head rows plus the lookup rows;
 *   Adam stays dense unless train_lazy_adam = 1).
 *   Refusals (< 0 before anything is launched): storage = 1 (at plan creation); a dense-gradient hook or lookup_grad;
 *   bsarec_backward_seq / _multi; train_sampler = 1 without a table. */
#define BSAREC_TRAIN_NEG_MAX 8192
#define BSAREC_TRAIN_NEG_SITE 0x4E454753u
/* Lazy (sparse) Adam for the item table (cfg.train_lazy_adam = 1, with the sampled head), the optimiser of torch.optim.SparseAdam
 * and of LazyAdam: a step's update of the item table costs what the rows it touches cost, not V d.
 *   Touched set of a step: T = { ids[b][l] != 0 } u { answers[b] } u { n_0 .. n_N-1 } (BSAREC_BUF_TRAIN_CAND), at most
 *   min(V, B L + B + N) rows; ids and answers clamped to [0, V) as the kernels read them.
 *   Row r in T: g_r = the item-table gradient row of the sampled head (candidate and answer rows plus lookup rows, the
 *   fixed-point sum converted to float), then the arithmetic of the dense update with the same t and bias corrections
 *   (state[3]): g += wd w when weight_decay != 0, m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g^2,
 *   w -= step_size m / (sqrt(v) / bc2s + eps).  Once per step however often r occurs in T, and even when g_r is exactly 0:
 *   presence in T counts, not the value.
 *   Row r not in T: w, m and v unchanged bit for bit (no weight decay), its gradient row not written.
 *   Every other tensor of the arena: the dense update, as without the flag.
 *   Gradient arena after a lazy step: item rows of T hold this step's gradient; other item rows keep what they held before.
 *   T, its size and its resets live on the device: a captured step replays with a fresh T.  Steps stay bit-deterministic
 *   (T is listed in arbitrary order; each row's update is independent of the others).
 *   Only bsarec_train_step and bsarec_train_step_indexed update lazily; bsarec_loss / bsarec_backward on such a plan compute
 *   and store exactly what they do without the flag.  The plan-less bsarec_adam_step / bsarec_adam_apply are unchanged.
 *   Refusals (< 0 before anything is launched): train_lazy_adam = 1 with train_negatives = 0 (at plan creation; the workspace
 *   size is 0); bsarec_grad_step_indexed on such a plan; a step whose bsarec_adam_t does not hold the item table inside
 *   its flat arena, or has grads2, grad_srcs or shadow_bf16.
 *   Workspace: int32[V] row marks + int32[min(V, B L + B + N)] row list; nothing without the flag. */

/* The popularity table of train_sampler = 1: int64[V] on the device, kept valid by the caller while the plan trains (null
 * clears it).  < 0 on a plan without train_negatives > 0 and train_sampler = 1. */
int bsarec_plan_set_train_sampler(bsarec_plan_t *plan, const int64_t *pop_cum);

/* Keep bits of the dropout masks (plan option drop_bits).  At the fused shape, in fp32 and bf16 storage (not with
 * x3_products, chain_kernels or filter_kind = 1), the forward block kernels of a training step leave one bit per element of
 * every dropout mask in BSAREC_BUF_DROP_BITS of their layer -- 1 = kept -- and the matching backward reads the bits instead of
 * evaluating the Philox stream a second time; results are the same bit for bit.  On by default; bsarec_plan_set_drop_bits(plan, 0)
 * makes the backward evaluate Philox again (and the forward store nothing).  Change it between steps, not between a forward
 * and its backward.  Eval forwards and sites with p = 0 touch no bits.
 * bsarec_drop_bits_bytes: bytes of one layer's buffer for `cfg` (0: such a plan keeps none; < 0: bad cfg).
 * The index map, host arithmetic only (bit i of the buffer = bit i & 7 of byte i >> 3; -1 on a bad argument):
 *   bsarec_drop_bits_hidden_bit: element (token, column) of hidden-size site `slot` (0 embedding -- layer 0 only --, 1 the
 *     FrequencyLayer's, 2 the attention output's, 3 the feed-forward's dropout) among `tokens` = B L tokens;
 *   bsarec_drop_bits_attn_bit: element (b, head, query, key) of the attention-probability dropout.
 * After bsarec_forward_last with a pruned top block the top layer holds row / query L - 1 only. */
int bsarec_plan_set_drop_bits(bsarec_plan_t *plan, int on);
long bsarec_drop_bits_bytes(const bsarec_config_t *cfg);
long bsarec_drop_bits_hidden_bit(int slot, long tokens, long token, int column);
long bsarec_drop_bits_attn_bit(long tokens, int heads, long b, int head, int query, int key);

/* Attention without the causal term (plan option bidirectional; the encoder of the BERT4Rec sibling model).
 *   on = 0 (default): mask(q, k) = (k <= q && ids[b, k] > 0) ? 0 : -10000 -- the reference's causal + padding mask;
 *   on = 1:           mask(q, k) = ids[b, k] > 0 ? 0 : -10000 -- the padding mask alone.
 * Either is added in fp32 before the row maximum.  A run-time argument of the three forward kernels that form the mask (the
 * LDS-phase block kernel, the register-chain block kernel, the generic path's softmax epilogue): no kernel is instantiated for
 * it, and a causal plan computes the bits it always did.  The backward kernels read the saved probabilities and form no mask;
 * the one-row top block of bsarec_forward_last looks at the last row, where both masks agree.  Change it between steps, not
 * between a forward and its backward. */
int bsarec_plan_set_bidirectional(bsarec_plan_t *plan, int on);

/* Byte offset of a named buffer inside the workspace, or -1. */
long bsarec_buffer_offset(const bsarec_plan_t *plan, int buffer, int layer);

/* Advance the forward-step counter (new dropout masks).  Call once per training step. */
int bsarec_step_begin(bsarec_plan_t *plan, void *stream);

/* BSARecModel.forward(input_ids, all_sequence_output=True)   (src/model/bsarec.py:16-28):
 * ids int64[B,L] (left-padded with 0) -> layer outputs in BSAREC_BUF_LAYER_OUT[0..N].
 * train != 0 applies dropout (model.train()), 0 is model.eval(). */
int bsarec_forward(bsarec_plan_t *plan, const int64_t *ids, int train, void *stream);

/* The rest of BSARecModel.calculate_loss (src/model/bsarec.py:32-35) on the forward's result:
 * logits = h[:, -1, :] @ E^T, mean CE against answers int64[B]; also prepares dlogits. */
int bsarec_loss(bsarec_plan_t *plan, const int64_t *answers, void *stream);

/* bsarec_forward for callers that consume only position L-1 of the last layer -- bsarec_loss, bsarec_logits and
 * bsarec_backward, i.e. calculate_loss (src/model/bsarec.py:30-37) and Trainer.predict_full of the last position
 * (src/trainers.py:126-129).  At the fused shape with >= 2 layers the top block is then evaluated on that row only
 * (it still attends to all positions) and its backward uses the exact one-row structure of the upstream gradient;
 * loss, logits and all parameter gradients are those of bsarec_forward.  Other rows of BSAREC_BUF_LAYER_OUT[N] are
 * left unspecified.  cfg.no_prune_top = 1 makes this identical to bsarec_forward. */
int bsarec_forward_last(bsarec_plan_t *plan, const int64_t *ids, int train, void *stream);

/* Sibling model SASRec (src/model/sasrec.py:41-63): the BCE head on one positive and one negative item at the last
 * position, over the rows with pos_ids != 0, instead of the full-catalogue CE.  Run it on a plan created with
 * alpha = 0 (then a BSARecBlock is exactly the reference's TransformerBlock, src/model/_modules.py:142-151).  Loss ->
 * BSAREC_BUF_LOSS; bsarec_backward then back-propagates this head (pos_ids / neg_ids must stay valid until then). */
int bsarec_loss_bce(bsarec_plan_t *plan, const int64_t *pos_ids, const int64_t *neg_ids, void *stream);
/* Sibling model FMLPRec's head (src/model/fmlprec.py:41-62): mean over ALL rows of
 * -log(sigmoid(x_pos) + 1e-24) - log(1 - sigmoid(x_neg) + 1e-24); otherwise as bsarec_loss_bce. */
int bsarec_loss_logsig(bsarec_plan_t *plan, const int64_t *pos_ids, const int64_t *neg_ids, void *stream);

/* logits only (Trainer.predict_full, src/trainers.py:62-68). */
int bsarec_logits(bsarec_plan_t *plan, void *stream);

/* loss.backward() (src/trainers.py:106): gradients of all tensors -> `grads` (overwritten, not
 * accumulated).  Must follow bsarec_forward(train as given there) + bsarec_loss on the same plan. */
int bsarec_backward(bsarec_plan_t *plan, void *stream);

/* Backward of BSARecModel.forward itself (src/model/bsarec.py:16-28 as an autograd graph): `d_out` = gradient w.r.t.
 * the LAST layer's output on ALL positions, fp32 [B, L, d].  Must follow bsarec_forward (not _forward_last) on the
 * same plan.  Gradients of all tensors -> `grads` (overwritten); the item table receives its lookup-path rows only
 * (there is no logits product on this path).  What sibling models with their own heads on the sequence output need
 * (DuoRec's contrastive terms, src/model/duorec.py:95-127). */
int bsarec_backward_seq(bsarec_plan_t *plan, const float *d_out, void *stream);

/* The same with an upstream gradient for EVERY element of forward(all_sequence_output=True)'s list
 * (src/model/bsarec.py:46-54: index 0 = embedding output, index l = output of block l - 1, index N = the last layer):
 * d_outs[0..N], fp32 [B, L, d] each; d_outs[N] must be given, d_outs[l < N] may be NULL (no gradient for that output). */
int bsarec_backward_seq_multi(bsarec_plan_t *plan, const float *const *d_outs, void *stream);

/* torch.optim.Adam (src/trainers.py:27-28,107) over flat arenas: one struct for every entry point that updates. */
typedef struct {
    float *params;            /* [n] fp32 master parameters (n % 4 == 0) */
    const float *grads;       /* [n] gradients (written by bsarec_backward through the plan's `grads` pointers) */
    float *exp_avg, *exp_avg_sq;   /* [n] Adam moments */
    long n;
    float lr, beta1, beta2, eps, weight_decay;
    float grad_scale;         /* g is scaled by this first (1/world_size after a summing all-reduce; else 1) */
    void *shadow_bf16;        /* null, or bf16[n] mirror of params (cfg.storage = 1): the update also writes the rounded */
    long shadow_from;         /*   parameter to shadow_bf16[i] for i >= shadow_from (the tensors after the item table) */
    /* ---- data-parallel gradient sources (all optional; zero-filled = g is `grads`) ---- */
    float *grads2;            /* a second arena ADDED to the first grads2_n elements of g and zeroed by the update: the   */
    long grads2_n;            /*   lookup-path rows of the item table when its dense part was exchanged early (buckets)    */
    int n_grad_srcs;          /* > 0: g = sum of grad_srcs[0 .. n) in index order (`grads` ignored) -- the one-shot       */
    const float *grad_srcs[8];/*   peer-to-peer exchange of bsarec_comm.h: every rank's arena in RANK order, so that every */
                              /*   replica forms the identical sum                                                        */
    bsarec_plan_t *wimage_plan; /* bsarec_adam_step / _apply only: null, or a plan of `params` that reads the fragment image  */
                              /*   (cfg.weight_image): bsarec_wimage_refresh(wimage_plan) is launched right behind the update */
} bsarec_adam_t;

/* Advance Adam's t / bias corrections in `state`, then update. */
int bsarec_adam_step(const bsarec_adam_t *adam, void *state, void *stream);
/* The parameter update alone (t and the bias corrections were already advanced by bsarec_grad_step_indexed(lr > 0)). */
int bsarec_adam_apply(const bsarec_adam_t *adam, void *state, void *stream);

/* Trainer.iteration's per-batch body (src/trainers.py:100-107) in one call:
 * step_begin + forward(train) + loss + backward + Adam. */
int bsarec_train_step(bsarec_plan_t *plan, const int64_t *ids, const int64_t *answers, const bsarec_adam_t *adam,
                      void *stream);

/* Device-side batch assembly from a resident sample table (replaces RandomSampler + DataLoader collation,
 * src/dataset.py:207-211): ids_out[b,:] = table[perm[*cursor + b], :], answers_out[b] = answers_table[perm[*cursor + b]].
 * `cursor` is one int64 on the device. */
int bsarec_gather_batch(const int64_t *table, const int64_t *answers_table, const int64_t *perm, long n_samples,
                        const void *cursor, int B, int L, int64_t *ids_out, int64_t *answers_out, void *stream);

/* bsarec_train_step fed from the resident table: the embedding kernel assembles the batch at *cursor (and fills
 * ids_buf / answers_buf), forward + loss + backward + Adam; the closing block of the gradient reduction ends the step
 * (mean loss, forward-step index += 1, *cursor += B).  A captured graph of this call replays a whole epoch with no
 * host work.  The dropout step counter is used as it stands and advanced at the END (bsarec_train_step /
 * bsarec_step_begin advance it BEFORE use): call bsarec_step_begin once between a begin-style step and this one. */
int bsarec_train_step_indexed(bsarec_plan_t *plan, const int64_t *table, const int64_t *answers_table,
                              const int64_t *perm, long n_samples, void *cursor, int64_t *ids_buf, int64_t *answers_buf,
                              const bsarec_adam_t *adam, void *stream);

/* The data-parallel half of the above: gather + forward + loss + backward (no Adam).  The caller then exchanges the
 * flat gradient arena (RCCL all-reduce, or the peer-to-peer read of bsarec_comm.h) and calls
 * bsarec_adam_step(grad_scale = 1/world) -- or, when lr > 0 is given here, the step's closing block also advances
 * Adam's t and publishes the bias corrections, and the caller follows the exchange with bsarec_adam_apply (one launch
 * fewer per step).  lr <= 0: no Adam bookkeeping here. */
int bsarec_grad_step_indexed(bsarec_plan_t *plan, const int64_t *table, const int64_t *answers_table,
                             const int64_t *perm, long n_samples, void *cursor, int64_t *ids_buf, int64_t *answers_buf,
                             float lr, float beta1, float beta2, void *stream);

/* Evaluation branch of Trainer.iteration (src/trainers.py:134): scores[b][indices[j]] = 0 (not -inf) for every item j
 * of the CSR row indptr[users[b]] .. indptr[users[b] + 1] -- the items user b has already seen (the reference's
 * train_matrix, src/dataset.py:126-168, uploaded as int64 CSR).  scores: [B][ld] on the device. */
int bsarec_mask_seen(float *scores, long ld, int B, const int64_t *users, const int64_t *indptr,
                     const int64_t *indices, void *stream);

/* The same masking AND the reference's top-k (src/trainers.py:134-149: argpartition of the 20 best + argsort) in one
 * launch, one workgroup per user: scores[b][seen items] = 0 (written back), then out_idx[b][0..k) = the columns of the k
 * best scores of scores[b][0..V) in descending order, out_val (nullable) their scores exactly as stored.  Columns [V, ld)
 * are never read.  indptr == NULL: no masking.  1 <= k <= BSAREC_TOPK_MAX, k <= V <= ld.
 * The order is total: NaN ranks above +inf and all NaNs are equal, -0.0 equals +0.0, and among equal scores the smaller
 * column comes first -- a stable descending sort with NaN as the largest value; every index is < V. */
#define BSAREC_TOPK_MAX 1024
int bsarec_topk_seen(float *scores, long ld, int B, int V, const int64_t *users, const int64_t *indptr,
                     const int64_t *indices, int k, int64_t *out_idx, float *out_val, void *stream);

/* Sampled-candidate evaluation: the protocol of the SASRec / BERT4Rec papers, opt-in beside the full ranking above.  Row b
 * ranks its answer a = answers[b] against n_neg items drawn for user u = users[b] that u has not seen.  One launch, one
 * workgroup per row; enqueued on `stream` and capturable.
 *   Draw stream: Philox4x32-10 call j = 0, 1, ... has counter (j, lo32(u), hi32(u), tag), key (lo32(seed), hi32(seed)) and
 *   returns words w0..w3.  pop_cum == NULL (uniform): draw 4j + m takes w_m, item = 1 + ((uint64)w_m * (V - 1) >> 32).
 *   pop_cum != NULL (popularity): int64[V], non-decreasing, pop_cum[0] = 0, T = pop_cum[V - 1] >= 1; draw 2j + m takes
 *   x = w_2m | (uint64)w_2m+1 << 32, r = the high 64 bits of the 128-bit product x * T, item = the smallest i with
 *   pop_cum[i] > r (items of count 0 are never drawn).
 *   Acceptance, in stream order: a draw is accepted iff its item is not in the seen set (CSR row u of indptr / indices,
 *   sorted ascending; indptr == NULL: nothing is seen), is not a, and was not accepted before.  Sampling stops at n_neg
 *   accepted; a row that has not got them after BSAREC_NEG_MAX_DRAWS draws has failed.  a may itself be a seen item (a
 *   repeated item): it is still the positive.
 *   Candidates: [a, n_1 .. n_n_neg] in acceptance order; they depend on (u, tag, seed) only.
 *   Scores: s_c = sum_k h[b * ldh + k] * item_emb[c * d + k] in fp32, one code path for the answer and the negatives.
 *   Rank: the number of negatives whose score is > s_a, == s_a or NaN (ties count against the model); n_neg if s_a is
 *   NaN; -1 for a failed row or an answer outside [1, V).
 * rank_out: int32[B].  cand_out / score_out (nullable): [B][n_neg + 1], the candidates and their scores; a failed row has
 * a in column 0, 0 after its accepted negatives, and NaN scores.  Limits (else < 0 before any HIP call): B >= 1, V >= 2,
 * 4 <= d <= 256, d % 4 == 0, ldh >= d, 1 <= n_neg <= BSAREC_NEG_MAX, item_emb 16-byte aligned, h / item_emb / users /
 * answers / rank_out non-null, indices non-null when indptr is given. */
#define BSAREC_NEG_MAX 1024
#define BSAREC_NEG_MAX_DRAWS (1 << 20)
int bsarec_sampled_rank(const float *h, long ldh, const float *item_emb, int B, int V, int d, const int64_t *users,
                        const int64_t *answers, const int64_t *indptr, const int64_t *indices, const int64_t *pop_cum,
                        int n_neg, uint64_t seed, uint32_t tag, int32_t *rank_out, int64_t *cand_out, float *score_out,
                        void *stream);

/* Full-catalogue top-k without the B x V score matrix: opt-in beside bsarec_logits + bsarec_topk_seen, same result.
 *   Scores: s(b, j) = acc after acc = 0, acc = fmaf(h[b * ldh + i], item_emb[j * d + i], acc) for i = 0 .. d-1 in fp32 --
 *   an fmaf chain in ascending i, which v_mfma_f32_32x32x2_f32 computes bit for bit.  A score depends only on those two rows:
 *   not on B, V, k, cand_cap, the row's or the item's position, the workspace or the launch.
 *   Result: the seen items of row b (CSR row users[b] of indptr / indices; indptr == NULL: none; entries outside [0, V) are
 *   ignored) score 0.0, not -inf, exactly as in bsarec_topk_seen.  out_idx[b][0..k) = the top k under bsarec_topk_seen's total
 *   order (NaN above +inf and all NaNs equal, -0 equal to +0, ties to the smaller column, column 0 ranked like any other);
 *   out_val (nullable) their scores, +0.0 for a seen item.  For the same scores the lists are exactly those of
 *   bsarec_topk_seen on the materialised matrix, for every input (ties, all-zero tables, NaN rows, heavily seen rows):
 *   there is no approximate mode.
 *   Execution: a fixed sequence of 8 launches on `stream`: no host synchronisation, no allocation; capturable in a graph.
 *   Working memory: the caller's workspace of bsarec_topk_full_workspace_bytes(B, V, d, k, cand_cap) bytes, O(B (s + cap))
 *   with s ~ 4 sqrt(k V) sampled columns and cap candidates per row, never O(B V).
 *   Limits (else < 0 before any HIP call): B >= 1, 1 <= k <= BSAREC_TOPK_MAX, k <= V < 2^31, 4 <= d <= 256, d % 4 == 0,
 *   ldh >= d, h / item_emb / workspace 16-byte aligned and non-null, out_idx non-null, workspace_bytes >= the query, users and
 *   indices non-null when indptr is given.  cand_cap == 0: the default capacity; > 0: the per-row candidate capacity
 *   (k <= cand_cap <= 2^30), for tests that force the overflow paths -- the result does not depend on it.
 * bsarec_topk_full_workspace_bytes: host only, no HIP call; < 0 for arguments bsarec_topk_full would refuse. */
long bsarec_topk_full_workspace_bytes(int B, int V, int d, int k, int cand_cap);
int bsarec_topk_full(const float *h, long ldh, const float *item_emb, int B, int V, int d, const int64_t *users,
                     const int64_t *indptr, const int64_t *indices, int k, int cand_cap, void *workspace, long workspace_bytes,
                     int64_t *out_idx, float *out_val, void *stream);
/* bsarec_topk_full over a contiguous item range: item_rows holds rows [col_base, col_base + Vs) of a larger catalogue (one
 * shard of a catalogue split by rows).  bsarec_topk_full is the col_base = 0 case of the same code.
 *   Scores: the same fmaf chain of the h row and the item row: the score of an item does not depend on the range it is in.
 *   Seen items: the CSR indices are GLOBAL item ids; an entry applies (score +0.0) iff col_base <= id < col_base + Vs, every
 *   other entry (another range's items, negative padding) is ignored.
 *   Result: out_idx are GLOBAL ids (col_base + the row of item_rows), in bsarec_topk_seen's total order; equal scores go to
 *   the smaller global id.  So the top-k of a catalogue cut into contiguous ranges is the merge, under that order, of the
 *   ranges' top-min(k, Vs) lists.
 *   Execution, workspace (bsarec_topk_full_workspace_bytes(B, Vs, d, k, cand_cap)) and limits: those of bsarec_topk_full with
 *   V := Vs, and col_base >= 0, col_base + Vs <= 2^31 - 1 (else < 0 before any HIP call). */
int bsarec_topk_full_range(const float *h, long ldh, const float *item_rows, int B, int Vs, long col_base, int d,
                           const int64_t *users, const int64_t *indptr, const int64_t *indices, int k, int cand_cap,
                           void *workspace, long workspace_bytes, int64_t *out_idx, float *out_val, void *stream);

/* The answer's exact place in the full-catalogue order -- the one integer per row that HR@k, NDCG@k and MRR are functions
 * of -- without a score matrix, a threshold, a candidate list or a sort, and at any depth (no BSAREC_TOPK_MAX).
 *   Scores: s(b, j) is the fmaf chain of bsarec_topk_full.  The effective score e(b, j) is +0.0 when GLOBAL id j occurs in CSR
 *   row users[b] (indptr == NULL: nothing is seen), else s(b, j).  CSR entries are global ids as in bsarec_topk_full_range:
 *   entries outside the range are ignored, rows need not be sorted, may repeat an id (a distinct item counts once) and may
 *   be of any length.
 *   Rank: with a = answers[b] and t = e(b, a), rank_out[b] = the number of items j != a of the range that stand before (t, a)
 *   in bsarec_topk_seen's total order: topk key of e(b, j) above that of t, or equal keys and global j < a (NaN above +inf,
 *   -0 = +0, column 0 like any other).  An answer that is itself seen has t = +0.0.  Over the whole catalogue rank_out[b] is
 *   the index of a in the list bsarec_topk_seen would give with k = V, for every input: there is no approximate mode.
 *   bsarec_answer_rank: the col_base = 0, answer_score = NULL case.  score_out[b] (nullable) = t.  A row whose answer is
 *   outside [0, V) gets rank -1 and score NaN.
 *   bsarec_answer_rank_range, answer_score == NULL: the same over [col_base, col_base + Vs).  answer_score given:
 *   t = answer_score[b] as it is, and a -- any id in [0, 2^31), in this range or another -- serves the tie order and the j != a
 *   exclusion only (a outside [0, 2^31): -1 and NaN).  So the ranks of the contiguous ranges of a catalogue add up to the rank
 *   in the whole catalogue.
 *   bsarec_answer_score_range: score_out[b] = e(b, a) for the rows whose answer lies in the range; the other rows are left
 *   untouched.  Zero the array and sum it over the ranges: the sum is t (x + 0 = x; -0 and +0 share a key).
 *   Execution: two launches on `stream` (one for the score call): no host synchronisation, no allocation, no workspace;
 *   capturable; integer adds only, so bit-deterministic.
 *   Limits (else < 0 before any HIP call): B >= 1, 1 <= V, Vs < 2^31, col_base >= 0, col_base + Vs <= 2^31 - 1, 4 <= d <= 256,
 *   d % 4 == 0, ldh >= d, h and the item rows 16-byte aligned and non-null, answers and rank_out non-null (score_out for the
 *   score call), users and indices non-null when indptr is given. */
int bsarec_answer_rank(const float *h, long ldh, const float *item_emb, int B, int V, int d, const int64_t *users,
                       const int64_t *indptr, const int64_t *indices, const int64_t *answers, int32_t *rank_out,
                       float *score_out, void *stream);
int bsarec_answer_rank_range(const float *h, long ldh, const float *item_rows, int B, int Vs, long col_base, int d,
                             const int64_t *users, const int64_t *indptr, const int64_t *indices, const int64_t *answers,
                             const float *answer_score, int32_t *rank_out, float *score_out, void *stream);
int bsarec_answer_score_range(const float *h, long ldh, const float *item_rows, int B, int Vs, long col_base, int d,
                              const int64_t *users, const int64_t *indptr, const int64_t *indices, const int64_t *answers,
                              float *score_out, void *stream);

/* DuoRec's contrastive head (src/model/duorec.py:47-78 + F.cross_entropy): InfoNCE between two batches of B rows, loss and
 * gradient, without the 2B x 2B score matrix.  z = [z_i; z_j], n = 2B rows; pos(r) = (r + B) mod n.
 *   u_r  = z_r (sim = 0, dot)  or  z_r / max(|z_r|, 1e-8) (sim = 1, cos: each norm clamped on its own)
 *   s_rc = u_r . u_c * inv_tau
 *   lse_r = log sum_{c != r} exp(s_rc)       the diagonal excluded, the positive included once; the maximum is subtracted
 *                                            before every exp, so scores above 88 are fine
 *   row_r = lse_r - s_{r, pos(r)}            rows_out[r] (nullable, float[2B])
 *   loss  = mean_r row_r                     loss_out[0]: what F.cross_entropy(*info_nce(z_i, z_j, 1 / inv_tau, B, sim)) returns
 *   Backward for the upstream scalar g = gout[0] (DEVICE memory, read on the device): with W_rc = exp(s_rc - lse_r) +
 *   exp(s_rc - lse_c) for c != r and W_rr = 0,
 *     du_r = g inv_tau / n * (sum_c W_rc u_c - 2 u_pos(r))
 *     dot: dz_r = du_r.   cos: dz_r = (du_r - u_r (u_r . du_r)) / |z_r| when |z_r| > 1e-8, else du_r / 1e-8 (autograd through
 *     the clamp).  dz_i, dz_j: contiguous [B, d].  B = 1 gives loss 0 and dz 0 exactly.
 *   bsarec_info_nce_bwd reads the statistics (lse, the clamped norms) that bsarec_info_nce_fwd left in `workspace` for the SAME
 *   z_i, z_j, B, d, inv_tau, sim: call the forward first and keep workspace and inputs unchanged in between.
 *   Workspace: bsarec_info_nce_workspace_bytes(B, d, sim) bytes (host-only query, no HIP call), linear in B: per-row statistics,
 *   per-split partial (max, sum) pairs, and the backward's S <= 8 key-split slabs of [2B, d] floats with S * 2B <= 16384 + 2B.
 *   Execution: two launches on `stream` forward (three for cos), two backward; no host synchronisation, no allocation, no
 *   atomics: capturable, and every sum has ONE order, so loss, rows and gradients are bit-deterministic -- also between a strided
 *   view and its contiguous copy.  Inputs are read-only and may alias each other; outputs may not alias inputs or the workspace.
 *   Limits (else < 0 before any HIP call): 1 <= B <= 4096; 4 <= d <= 256, d % 4 == 0; ld_i, ld_j >= d and % 4 == 0 (row
 *   strides in floats); z_i, z_j, workspace, dz_i, dz_j non-null and 16-byte aligned; loss_out, gout non-null; inv_tau finite
 *   and > 0; sim in {0, 1}; workspace_bytes at least the queried size. */
long bsarec_info_nce_workspace_bytes(int B, int d, int sim);
int bsarec_info_nce_fwd(const float *z_i, long ld_i, const float *z_j, long ld_j, int B, int d, float inv_tau, int sim,
                        float *loss_out, float *rows_out, void *workspace, long workspace_bytes, void *stream);
int bsarec_info_nce_bwd(const float *z_i, long ld_i, const float *z_j, long ld_j, int B, int d, float inv_tau, int sim,
                        const float *gout, void *workspace, long workspace_bytes, float *dz_i, float *dz_j, void *stream);

/* Full-catalogue cross-entropy on an external hidden state, loss and gradient, without the B x V logits: what
 * F.cross_entropy(h @ item_emb.T, answers) and its autograd compute, with nothing of size B x V stored.  No plan.
 *   s(b, j) = the fmaf chain of bsarec_topk_full: acc = 0, then acc = fmaf(h[b * ldh + i], item_emb[j * d + i], acc), i ascending
 *             (training and evaluation see the same logits); one score routine serves the forward and every backward kernel
 *   a_b     = answers[b] clamped to [0, V); item 0 (the padding row) is a class like any other
 *   lse_b   = m_b + log sum_{j < V} exp(s(b, j) - m_b), m_b the row maximum: scores above 88 are fine
 *   row_b   = lse_b - s(b, a_b)                rows_out[b] (nullable, float[B])
 *   loss    = mean_b row_b                     loss_out[0].  V = 1 gives loss 0 and zero gradients exactly.
 *   Backward for the upstream scalar g = gout[0] (DEVICE memory, read on the device): G_bj = g / B * (exp(s(b, j) - lse_b) -
 *   [j == a_b]),  dh[b] = sum_j G_bj item_emb[j]  (contiguous [B, d]),  d_item_emb[j] = sum_b G_bj h[b]  (contiguous [V, d], every
 *   row overwritten).  g / B is applied to the finished sums.
 *   The row statistics are kept as the pair (m_b, log l_b), l_b the sum above: row_b is formed as (m_b - s(b, a_b)) + log l_b and
 *   the backward's exponent as (s(b, j) - m_b) - log l_b, which do not round at the magnitude of m_b as m_b + log l_b would.
 *   bsarec_ce_head_bwd reads the row statistics that bsarec_ce_head_fwd left in `workspace` for the SAME h, item_emb, answers,
 *   B, V, d: call the forward first and keep workspace and inputs unchanged in between.
 *   Workspace: bsarec_ce_head_workspace_bytes(B, V, d) bytes (host-only query, no HIP call): m[B], log l[B], the (max, sum) pairs of the
 *   S splits of the catalogue, and the backward's S slabs of [B, d] floats, added in split order; S B <= 16384 + B, so the size
 *   is at most (16384 + 2B) * (d + 8) * 4 bytes for every V and stops growing with V.
 *   Execution: two launches on `stream` forward, three backward; no host synchronisation, no allocation, no atomics: capturable,
 *   and every sum has ONE order, so loss, rows, dh and d_item_emb are bit-deterministic -- also between a strided h (the
 *   [:, -1, :] view, ldh = L * d) and its contiguous copy.  Inputs are read-only; outputs may not alias inputs or the workspace.
 *   Limits (else < 0 before any HIP call): 1 <= B <= 65536; 1 <= V < 2^31; 4 <= d <= 256, d % 4 == 0; ldh >= d and % 4 == 0 (row
 *   stride in floats); h, item_emb, workspace, dh, d_item_emb non-null and 16-byte aligned; answers, loss_out, gout non-null;
 *   workspace_bytes at least the queried size. */
long bsarec_ce_head_workspace_bytes(int B, int V, int d);
int bsarec_ce_head_fwd(const float *h, long ldh, const float *item_emb, int B, int V, int d, const int64_t *answers,
                       float *loss_out, float *rows_out, void *workspace, long workspace_bytes, void *stream);
int bsarec_ce_head_bwd(const float *h, long ldh, const float *item_emb, int B, int V, int d, const int64_t *answers,
                       const float *gout, void *workspace, long workspace_bytes, float *dh, float *d_item_emb, void *stream);
/* The same head over a catalogue split by rows into contiguous ranges, one per rank (the catalogue-sharded step,
 * bsarec_shard.h): exact full-catalogue CE, d(h) and dE with no [Bg, Vs] buffer.  item_rows holds rows [col_base, col_base + Vs)
 * of a catalogue of item_size rows; h, answers and every output cover ALL Bg rows of the global batch.  bsarec_ce_head_fwd /
 * _bwd are the col_base = 0, Vs = item_size case of the same kernels.
 *   Scores: the same fmaf chain of the h row and the item row; a score does not depend on the range the item is in.
 *   Answers: clamped to [0, item_size) GLOBALLY; a range owns a_b iff col_base <= a_b < col_base + Vs.
 *   bsarec_ce_head_range_stats: stats[3][Bg] in the layout of bsarec_shard_ce_stats -- row 0 the row maximum over the owned
 *     items, row 1 sum exp(s - max) over them, row 2 s(b, a_b) if owned, else 0.  Vs = 0 reports (-inf, 0, 0) and launches
 *     nothing over items.  Two launches.
 *   The caller gathers every range's stats into stats_all[world][3][Bg], in range order (an all-gather).
 *   bsarec_ce_head_range_merge: one launch of one workgroup; per row the `world` (max, sum) pairs merged in range order (a
 *     (-inf, 0) pair is neutral), target = the sum of row 2 over the ranges (one owner, the others wrote 0); m_b and log l_b of
 *     the WHOLE catalogue go into this range's `workspace` where the backward reads them; loss_rows[b] = (m_b - target) +
 *     log l_b, loss[0] = their mean.  Every range that merges the same stats_all gets the same bits.  With world = 1 over the
 *     whole table, loss and loss_rows are those of bsarec_ce_head_fwd bit for bit.
 *   bsarec_ce_head_range_bwd: G_bj = g / Bg * (exp((s(b, j) - m_b) - log l_b) - [col_base + j == a_b]) for the owned j;
 *     dh_part[Bg, d] = sum over the owned j of G_bj item_rows[j] -- the ranges' parts add up to d(h) (an all-reduce);
 *     dE_rows[Vs, d] = sum_b G_bj h[b], every row overwritten, one writer per row, one order.  Vs = 0 zeroes dh_part and
 *     touches nothing else.  Three launches.  With world = 1 over the whole table: the bits of bsarec_ce_head_bwd.
 *   Call stats, merge and bwd in that order with the SAME workspace, h, item_rows and answers; the workspace is
 *   bsarec_ce_head_range_workspace_bytes(Bg, Vs, d) = bsarec_ce_head_workspace_bytes(Bg, max(Vs, 1), d) bytes (host only).
 *   Execution: as bsarec_ce_head_fwd / _bwd -- the caller's stream, no host synchronisation, no allocation, no atomics,
 *   capturable, bit-deterministic, h through its row stride.
 *   Limits (else < 0 before any HIP call): those of bsarec_ce_head_fwd / _bwd with B := Bg, V := Vs (Vs = 0 allowed);
 *   0 <= col_base, col_base + Vs <= item_size < 2^31; 1 <= world <= 8; stats, stats_all, loss_rows, loss non-null;
 *   merge: workspace 16-byte aligned and at least 8 Bg bytes. */
long bsarec_ce_head_range_workspace_bytes(int Bg, int Vs, int d);
int bsarec_ce_head_range_stats(const float *h, long ldh, const float *item_rows, int Bg, int Vs, long col_base, long item_size,
                               int d, const int64_t *answers, float *stats, void *workspace, long workspace_bytes, void *stream);
int bsarec_ce_head_range_merge(const float *stats_all, int world, int Bg, void *workspace, long workspace_bytes,
                               float *loss_rows, float *loss, void *stream);
int bsarec_ce_head_range_bwd(const float *h, long ldh, const float *item_rows, int Bg, int Vs, long col_base, long item_size,
                             int d, const int64_t *answers, const float *gout, void *workspace, long workspace_bytes,
                             float *dh_part, float *dE_rows, void *stream);

/* BERT4Rec's masking step (csrc/cloze.h): which tokens of a batch are replaced by the mask token, and the compacted list of
 * the positions that carry a loss term, for bsarec_cloze_head_fwd / _bwd.  No plan.
 *   Draw: token e = b * L + t takes word e & 3 of Philox4x32-10 call (lo32(e >> 2), hi32(e >> 2), BSAREC_CLOZE_SITE,
 *   lo32(state[1])) keyed by state[0] -- the dropout stream at a site no dropout mask uses; threshold floor(ratio * 2^32),
 *   at most 2^32 - 1.
 *   drawn(b, t) = ids[b, t] > 0 && word < threshold; a row that draws nothing while ids[b, L - 1] > 0 draws position L - 1,
 *   so every sequence that ends in an item gives at least one row.
 *   masked_ids[b, t] = drawn ? mask_token : ids[b, t]                                   int64 [B, L]
 *   The loss positions of row b are its LAST min(count_b, slots) drawn positions; earlier drawn ones stay masked in the input
 *   and carry no loss.  rows[R], R = B * slots: the token indices b * L + t of all loss positions, ascending, no gaps;
 *   targets[r] = ids at that token; count[0] = n, the number of live rows; rows = -1 and targets = 0 at r >= n.
 *   Every output element is written; the outputs depend on (ids, ratio, slots, state[0], state[1]) only.  `state` (u64[8], as
 *   a plan's) is read, not advanced.
 *   Execution: two launches on `stream`; no atomics, no allocation, no host synchronisation: capturable, and a replay reads the
 *   state's current step.  rows doubles as the staging area of the compaction.
 *   Limits (else < 0 before any HIP call): 1 <= B <= 65536; 1 <= L <= 256; 1 <= slots <= L; B * slots <= 65536;
 *   0 <= ratio <= 1 (NaN refused); every pointer non-null, ids / masked_ids / targets / state 8-byte aligned, rows / count
 *   4-byte aligned. */
#define BSAREC_CLOZE_SITE 0x434C4F5Au
int bsarec_cloze_mask(const int64_t *ids, int B, int L, float ratio, int slots, int64_t mask_token, const void *state,
                      int64_t *masked_ids, int32_t *rows, int64_t *targets, int32_t *count, void *stream);

/* The cloze loss: bsarec_ce_head_fwd / _bwd on the rows of h that a row list names, of which the first n are live -- the SAME
 * kernels with a row list and a live count (csrc/ce_head.h), nothing of size rows x V.  No plan.
 *   h: [T, d] with row stride ldh (the encoder's [B, L, d] output: T = B * L).  rows[R], targets[R], count[1] as
 *   bsarec_cloze_mask writes them; n = min(count[0], R) (< 0 counts as 0), read on the device.
 *   For r < n: row_r = lse_r - s(r, a_r) over the items j < V, the scores those of h[rows[r]] through the fmaf chain of
 *   bsarec_ce_head_fwd, a_r = targets[r] clamped to [0, V).  loss_out[0] = (sum_{r < n} row_r) / max(n, 1).  rows_out
 *   (nullable, float[R]): row_r, and 0 at r >= n.
 *   Backward for the device scalar g = gout[0]: G_rj = g / max(n, 1) * (softmax_rj - [j == a_r]);  dh is contiguous [T, d] and
 *   every float of it is written: row rows[r] holds sum_j G_rj item_emb[j], every other row 0;  d_item_emb [V, d], every row
 *   overwritten with sum_{r < n} G_rj h[rows[r]].  n = 0: loss 0 and all-zero gradients.
 *   rows[r < n] are distinct and inside [0, T) -- the caller's contract, which bsarec_cloze_mask keeps; entries at r >= n are
 *   never read as indices.  item_emb may be the first V rows of a larger table (BERT4Rec's has V + 1: the mask token is no class).
 *   The splits, the grids and the workspace (bsarec_cloze_head_workspace_bytes = bsarec_ce_head_workspace_bytes(R, V, d)) are
 *   sized by the capacity R on the host; row tiles at or behind n exit at once, so the time follows n.
 *   Execution: as bsarec_ce_head_fwd / _bwd (the backward adds one memset node for dh); capturable, bit-deterministic.
 *   Limits (else < 0 before any HIP call): those of bsarec_ce_head_fwd / _bwd with B := R; 1 <= T < 2^31 / d; rows, targets,
 *   count non-null, rows / count 4-byte and targets 8-byte aligned. */
long bsarec_cloze_head_workspace_bytes(int R, int V, int d);
int bsarec_cloze_head_fwd(const float *h, long ldh, long T, const float *item_emb, int R, int V, int d, const int32_t *rows,
                          const int64_t *targets, const int32_t *count, float *loss_out, float *rows_out, void *workspace,
                          long workspace_bytes, void *stream);
int bsarec_cloze_head_bwd(const float *h, long ldh, long T, const float *item_emb, int R, int V, int d, const int32_t *rows,
                          const int64_t *targets, const int32_t *count, const float *gout, void *workspace,
                          long workspace_bytes, float *dh, float *d_item_emb, void *stream);

/* GRU stack of the GRU4Rec sibling model (csrc/gru.h): num_layers bias-free GRU layers in torch's gate order (r, z, n), h_0 = 0,
 * no dropout between layers, and an optional Linear on top -- what nn.GRU(input_size, hidden_size, num_layers, bias=False,
 * batch_first=True) followed by nn.Linear(hidden_size, out_size) and their autograd compute, in fp32.  No plan.
 *   One layer, with a_t = W_ih x_t and b_t = W_hh h_{t-1} (three gate blocks of hidden_size rows each):
 *     r = sigmoid(a_r + b_r), z = sigmoid(a_z + b_z), n = tanh(a_n + r * b_n), h_t = n + z * (h_{t-1} - n);
 *   layer k > 0 reads layer k - 1's h; y = the top layer's h; out = y . w_out^T + b_out, or y itself when out_size is 0.
 *   Every position is computed: the caller masks nothing.
 *   weights: ONE flat array of bsarec_gru_weight_floats(cfg) floats, row-major tensors in this order:
 *     w_ih_l0 [3H, I] | w_hh_l0 [3H, H] | w_ih_l1 [3H, H] | w_hh_l1 [3H, H] | ... | w_out [O, H] | b_out [O]
 *   (I = input_size, H = hidden_size, O = out_size; the last two are empty when O is 0).  dweights has the same layout.
 *   x is [B, L, I]; out is [B, L, O'] with O' = O, or H when O is 0; with last_only != 0 out is [B, O'], position L - 1 alone,
 *   the bits of that row of the full output.  train = 0 gives the bits of train = 1 and keeps nothing for a backward.
 *   bsarec_gru_bwd: dout has out's shape; with last_only != 0 it is [B, O'], the gradient at position L - 1, zero elsewhere.
 *   dx [B, L, I] and every float of dweights are overwritten.  It reads what bsarec_gru_fwd(train = 1) left in the SAME
 *   workspace for the same cfg, x and weights: call the forward first and keep all three unchanged in between.
 *   Launches, all on `stream`: forward, per layer one product a = in . W_ih^T of all L B rows (the library's tiled fp32 MFMA
 *   product) and one sequence kernel -- ceil(B / 16) workgroups, each owning 16 sequences for all L steps with W_hh resident in
 *   registers, no communication between workgroups --, then the projection (on B rows with last_only).  Backward, per layer
 *   from the top: one sequence kernel (t descending; writes da [L B, 3H] and db_n [L B, H]), then d(in) = da . W_ih,
 *   dW_ih = da^T . in and dW_hh = db^T . h_prev as split-K products into slabs added in split order; before them the
 *   projection's d(y), dw_out, db_out.  No atomics, no allocation, no host synchronisation: capturable, and every sum has ONE
 *   order that depends on the shape alone, so all outputs are bit-deterministic; a sequence's forward bits do not depend on B
 *   or on its place in the batch.
 *   Workspace: bsarec_gru_workspace_bytes(cfg, train) bytes (host-only query, no HIP call).  Activations are kept time-major,
 *   [L][B][.].  In floats, with T = L B: a / da [T, 3H] | y_k [T, H] for k < N (train = 0: min(N, 2)) | and with train != 0:
 *   (r, z, n, b_n)_k [T, 4H] for k < N | db_n [T, H] | two d(y) [T, H] | x time-major [T, I] | dout time-major [T, O] |
 *   S slabs of max(3H max(I, H), O H) | S x O bias partials; S <= 64: a product over K rows is split into at most min(64, ceil(K / 256))
 *   slices of a multiple of 32 rows.
 *   Limits (else < 0 before any HIP call): 1 <= batch <= 65536; 1 <= seq_len <= 256; 4 <= input_size <= 256, % 4 == 0;
 *   hidden_size in {32, 64, 96, 128}; 1 <= num_layers <= 4; out_size 0, or 4 <= out_size <= 256, % 4 == 0; every pointer
 *   non-null and 16-byte aligned; workspace_bytes at least the queried size (bsarec_gru_bwd: that of train = 1).  Inputs are
 *   read-only; outputs may not alias inputs, each other or the workspace. */
typedef struct {
    int batch, seq_len, input_size, hidden_size, num_layers;
    int out_size;                      /* 0: no projection */
} bsarec_gru_config_t;
long bsarec_gru_weight_floats(const bsarec_gru_config_t *cfg);
long bsarec_gru_workspace_bytes(const bsarec_gru_config_t *cfg, int train);
int bsarec_gru_fwd(const bsarec_gru_config_t *cfg, const float *x, const float *weights, int train, int last_only, float *out,
                   void *workspace, long workspace_bytes, void *stream);
int bsarec_gru_bwd(const bsarec_gru_config_t *cfg, const float *x, const float *weights, int last_only, const float *dout,
                   void *workspace, long workspace_bytes, float *dx, float *dweights, void *stream);

/* One GRU4Rec training step (csrc/pair_step.h): with E = item_emb [V, d], x = Dropout_p(E[ids]) [B, L, d], s = the GRU stack's
 * output at position L - 1 (bsarec_gru_fwd, last_only) and
 *   diff_b = s_b . E[answers_b] - s_b . E[neg_answers_b],  loss = mean_b -log(sigmoid(diff_b) + 1e-10),
 * bsarec_gru4rec_loss_grad writes the loss (one float) and the gradient of every parameter: d_item_emb [V, d] -- the lookup rows
 * dE[ids[b, t]] += dx[b, t] * mask plus the head's 2 B rows; EVERY float is written, zero where no row was touched -- and dweights
 * in the layout of bsarec_gru_fwd's weights.  Id 0 is an ordinary row (nn.Embedding without padding_idx).  The sigmoid gives 0 or 1
 * exactly for large |diff| and never NaN.
 *   Dropout is the library's Philox stream, site 0, element index (b L + t) d + c, keyed by the device-resident step state
 * (`state`: u64[8], [0] = seed, [1] = forward-step counter, [2] = Adam t, [3..6] owned by the library).  A call with train != 0
 * advances the step counter FIRST and draws with the new value, as bsarec_train_step does; train = 0 draws nothing (the result of
 * dropout = 0) and touches no counter.  The mask is regenerated in the backward, not stored.
 *   bsarec_gru4rec_train_step is the above with train = 1 followed by Adam on both arrays, Adam's t advanced ONCE:
 * adam_items->params / grads are E / dE with n = V d, adam_weights->params / grads the GRU flat array and its gradient with
 * n = bsarec_gru_weight_floats(&cfg->gru); grads are written, then read.  lr, beta1 and beta2 of the two must agree (one t and one
 * pair of bias corrections serve both); shadow_bf16, grads2, grads2_n, n_grad_srcs and wimage_plan must be null / 0.
 *   Launches, all on `stream`, one after the other: the step counter (train != 0), lookup + dropout, bsarec_gru_fwd, the BPR
 * rows, bsarec_gru_bwd, the item-table gradient, its flush with the mean loss (and Adam's t) in a closing block, then one Adam
 * launch per array.  No allocation, no host synchronisation: capturable, and a replay of a captured bsarec_gru4rec_train_step is
 * the NEXT step -- a fresh mask, the next t.  Every output is bit-deterministic: the item-table gradient is summed in 64-bit fixed
 * point (2^-40 units, exact while |sum| < 2^22, the range of the BSARec lookup path), the mean loss in one fixed order.  The result
 * does not depend on what the workspace holds on entry.
 *   Workspace: bsarec_gru4rec_workspace_bytes(cfg) bytes (host-only query, no HIP call).  In floats, with T = L B: the GRU
 * workspace of train = 1 | x [T, d] | s [B, d] | ds [B, d] | dx [T, d] | c [B, rounded up to 4] | loss rows [B, rounded up to 4] |
 * the accumulator, V d 64-bit words.
 *   Limits (else < 0 before any HIP call): cfg->gru inside the limits of bsarec_gru_workspace_bytes with input_size == out_size;
 * item_size >= 2; 0 <= dropout < 1 (NaN refused); every pointer non-null; the float arrays (Adam's four included) and the
 * workspace 16-byte aligned, ids / answers / neg_answers / state 8-byte, loss_out 4-byte; workspace_bytes at least the queried
 * size; adam_*->n as above.  ids, answers and neg_answers inside [0, V) are the caller's contract.  Outputs may not alias
 * inputs, each other or the workspace. */
typedef struct {
    bsarec_gru_config_t gru;           /* input_size == out_size == d, the embedding width */
    int item_size;                     /* V >= 2 */
    float dropout;                     /* p in [0, 1) */
} bsarec_gru4rec_config_t;
long bsarec_gru4rec_workspace_bytes(const bsarec_gru4rec_config_t *cfg);
int bsarec_gru4rec_loss_grad(const bsarec_gru4rec_config_t *cfg, const float *item_emb, const float *weights,
                             const int64_t *ids, const int64_t *answers, const int64_t *neg_answers,
                             void *state, int train, float *loss_out, float *d_item_emb, float *dweights,
                             void *workspace, long workspace_bytes, void *stream);
int bsarec_gru4rec_train_step(const bsarec_gru4rec_config_t *cfg, const int64_t *ids, const int64_t *answers,
                              const int64_t *neg_answers, const bsarec_adam_t *adam_items,
                              const bsarec_adam_t *adam_weights, void *state, float *loss_out,
                              void *workspace, long workspace_bytes, void *stream);

/* GRU4Rec heads over candidates shared by the batch (csrc/gru4rec_cand.h), beside the pairwise head above.  The candidates are
 * c_0 .. c_C-1: candidates = 1: C = B, c_j = answers[j]; candidates = 2: C = 2 B, c_j = answers[j] for j < B and
 * c_{B+k} = neg_answers[k].  With r_bj = s_b . E[c_j], row b's positive is column b and its negatives are
 * M_b = { j : c_j != answers[b] }, m_b = |M_b| (every column holding the row's own target is left out; duplicates that are not the
 * target each count).  loss = mean_b loss_b over all B rows; a row with m_b = 0 has loss 0 and gradient 0 exactly:
 *   loss = 1 (cross-entropy)  loss_b = logsumexp_{j in {b} + M_b} r_bj - r_bb
 *   loss = 2 (TOP1)           loss_b = (1 / m_b) sum_{M_b} [sigmoid(r_bj - r_bb) + sigmoid(r_bj^2)]
 *   loss = 3 (BPR-max)        p = softmax of r_bj over M_b;  loss_b = -log(sum_j p_bj sigmoid(r_bb - r_bj) + 1e-10)
 *                                                                     + bpreg sum_j p_bj r_bj^2
 * Every softmax subtracts its maximum; the sigmoid is the pairwise head's (0 or 1 exactly for large arguments, never NaN).
 *   bsarec_gru4rec_cand_head is the head alone: s [B, width], item_emb [item_size, width] -> the loss (one float), ds [B, width] =
 * G . E_c and dEc [C, width] = G^T . s with G = d(loss) / d(r); dEc[j] is the gradient of item_emb's row c_j through column j (the
 * caller adds rows of equal items).  bsarec_gru4rec_cand_loss_grad / _cand_train_step are bsarec_gru4rec_loss_grad /
 * _train_step with this head in place of the pairwise rows: the same arguments, then the head; the item-table gradient takes
 * T + C rows (the lookup rows, then dEc[j] into row c_j) through the same fixed-point accumulator, flush, closing block and Adam
 * launches.
 *   Launches, all on `stream`, one after the other: the scores R [B, C] in 64 x 64 tiles; one workgroup per row (the row's
 * statistics, loss_b, G_b written over R_b); one grid that forms dEc and ds, each split over its summed dimension into
 * nslab slabs (nslab = min(16, ceil(C / 64)), lowered while nslab (B + C) width would pass 2^26 floats: a function of the shape
 * alone); with nslab > 1 one launch that adds the slabs in slab order; the head alone closes with the mean loss.  No floating-point atomics, no allocation, no host synchronisation: capturable, bit-deterministic, and independent of
 * what the workspace holds on entry.
 *   Workspace (host-only queries, no HIP call), in floats: R [B, C] (rounded up to 4) | nslab slabs [C, width] | nslab slabs
 * [B, width] (both absent when nslab is 1); bsarec_gru4rec_cand_head_workspace_bytes: those, then loss rows [B, rounded up to 4];
 * bsarec_gru4rec_cand_workspace_bytes: the workspace of bsarec_gru4rec_workspace_bytes, then those, then dEc [C, width].
 *   Limits (else < 0 before any HIP call): those of bsarec_gru4rec_loss_grad / _train_step (the head alone: 1 <= batch <= 65536,
 * 4 <= width <= 256, % 4 == 0, item_size >= 2); head non-null, loss in 1..3, candidates in 1..2, bpreg >= 0 (NaN refused);
 * C <= BSAREC_GRU4REC_CAND_MAX; every pointer non-null (neg_answers too when candidates is 1), float arrays and the workspace
 * 16-byte aligned, answers / neg_answers 8-byte, loss_out 4-byte; workspace_bytes at least the queried size.  answers and
 * neg_answers inside [0, item_size) are the caller's contract (a value outside is never dereferenced: it is no column of any row,
 * and a row whose answer is outside has loss 0).  Outputs may not alias inputs, each other or the workspace. */
#define BSAREC_GRU4REC_CAND_MAX 8192
typedef struct {
    int loss;                          /* 1 cross-entropy, 2 TOP1, 3 BPR-max */
    int candidates;                    /* 1 the batch's answers, 2 the answers and the negatives */
    float bpreg;                       /* BPR-max: the weight of the score regulariser, >= 0; ignored by the others */
} bsarec_gru4rec_head_t;
long bsarec_gru4rec_cand_head_workspace_bytes(int batch, int width, const bsarec_gru4rec_head_t *head);
int bsarec_gru4rec_cand_head(const float *s, const float *item_emb, const int64_t *answers, const int64_t *neg_answers,
                             int batch, int width, int item_size, const bsarec_gru4rec_head_t *head, float *loss_out,
                             float *ds, float *dEc, void *workspace, long workspace_bytes, void *stream);
long bsarec_gru4rec_cand_workspace_bytes(const bsarec_gru4rec_config_t *cfg, const bsarec_gru4rec_head_t *head);
int bsarec_gru4rec_cand_loss_grad(const bsarec_gru4rec_config_t *cfg, const float *item_emb, const float *weights,
                                  const int64_t *ids, const int64_t *answers, const int64_t *neg_answers,
                                  void *state, int train, float *loss_out, float *d_item_emb, float *dweights,
                                  void *workspace, long workspace_bytes, void *stream, const bsarec_gru4rec_head_t *head);
int bsarec_gru4rec_cand_train_step(const bsarec_gru4rec_config_t *cfg, const int64_t *ids, const int64_t *answers,
                                   const int64_t *neg_answers, const bsarec_adam_t *adam_items,
                                   const bsarec_adam_t *adam_weights, void *state, float *loss_out,
                                   void *workspace, long workspace_bytes, void *stream, const bsarec_gru4rec_head_t *head);

/* Stand-alone FrequencyLayer (src/model/bsarec.py:90-104) for per-op parity tests:
 * y = LN(Drop(low + beta^2 (x - low)) + x); backward given dy. */
int bsarec_freq_layer_fwd(const float *x, const float *sqrt_beta, const float *ln_w, const float *ln_b,
                          const float *twiddle, int B, int L, int d, int cutoff_bins, float eps, float p_drop,
                          const void *state, int site, float *y, float *xhat, float *rstd, void *stream);
long bsarec_freq_layer_bwd_scratch_floats(int B, int L, int d);
int bsarec_freq_layer_bwd(const float *x, const float *dy, const float *xhat, const float *rstd,
                          const float *sqrt_beta, const float *ln_w, const float *twiddle, int B, int L, int d,
                          int cutoff_bins, float p_drop, const void *state, int site,
                          float *scratch /* bsarec_freq_layer_bwd_scratch_floats(B,L,d) floats */,
                          float *dx, float *dsqrt_beta, float *dln_w, float *dln_b, void *stream);

/* Convolution block of the Caser sibling model (csrc/caser.h): with x [B, L, d] (d = width),
 *   vertical    zv[b, c, j]   = sum_t Wv[c, t] x[b, t, j] + bv[c],                                c < n_v, at z[b][c d + j]
 *   horizontal  c_h[b, f, t]  = sum_{i < h, j < d} Wh_h[f, i, j] x[b, t + i, j] + bh_h[f],        h = 1 .. L, t = 0 .. L - h
 *               zh[b, h-1, f] = max(0, max_t c_h[b, f, t]),                                       at z[b][n_v d + (h-1) n_h + f]
 * z [B, F], F = n_v d + n_h L: what nn.Conv2d(1, n_v, (L, 1)) and, per height, nn.Conv2d(1, n_h, (h, d)) -> ReLU -> max over t
 * compute on x.unsqueeze(1), concatenated.  All arithmetic is fp32 (v_mfma_f32_16x16x4_f32 in the horizontal forward).
 *   weights: ONE flat array of bsarec_caser_weight_floats(cfg) floats, row-major tensors in this order, EACH at an offset rounded
 * up to a multiple of 4 floats: conv_v.weight [n_v, L], conv_v.bias [n_v], then for h = 1 .. L conv_h.{h-1}.weight [n_h, h, d]
 * and conv_h.{h-1}.bias [n_h].  The gaps are never read; bsarec_caser_bwd writes 0 into them in dweights.
 *   bsarec_caser_bwd is the true derivative: a cell (b, h, f) passes dz only if its maximum is > 0, and to the window at the
 * LOWEST t that attains the maximum (torch's CPU max-pool rule).  dx [B, L, d] and every float of dweights are overwritten.  It
 * reads what bsarec_caser_fwd(train = 1) left in the SAME workspace: the winning t per cell as int [B][L][n_h], -1 for a cell
 * that passes nothing.  With train = 0 the forward keeps nothing and gives the same z bits.
 *   One reduction order per (h, f), whatever t and b: bit-identical windows give bit-identical c_h, so exact ties (left-padded
 * sequences repeat a row) resolve by the rule above, and a sequence's z bits do not depend on the rest of the batch.  Every
 * gradient sum runs in a fixed order (b rising; per dx element the cells (h, f) rising): no atomics, bit-deterministic.
 *   Launches, all on `stream`: forward 2 (vertical, horizontal), backward 3 (dx, dWh + dbh, dWv + dbv + gaps).  No allocation, no
 * host synchronisation, no scratch: capturable.  Dynamic LDS of the dx launch is 6 L n_h bytes (<= 48 KB).
 *   Workspace: bsarec_caser_workspace_bytes(cfg, train) bytes (host-only query, no HIP call).
 *   Limits (else < 0 before any HIP call): 1 <= batch <= 65536, 1 <= seq_len <= 256, width in 4 .. 256 and a multiple of 4,
 * n_h in {4, 8, 16, 32}, 1 <= n_v <= 16; every pointer non-null and 16-byte aligned; workspace_bytes at least the queried size
 * (bsarec_caser_bwd: that of train = 1).  Inputs are assumed finite. */
typedef struct {
    int batch, seq_len, width, n_h, n_v;
} bsarec_caser_config_t;
long bsarec_caser_weight_floats(const bsarec_caser_config_t *cfg);
long bsarec_caser_workspace_bytes(const bsarec_caser_config_t *cfg, int train);
int bsarec_caser_fwd(const bsarec_caser_config_t *cfg, const float *x, const float *weights, int train, float *z,
                     void *workspace, long workspace_bytes, void *stream);
int bsarec_caser_bwd(const bsarec_caser_config_t *cfg, const float *x, const float *weights, const float *dz,
                     void *workspace, long workspace_bytes, float *dx, float *dweights, void *stream);

/* fc1 of the Caser model alone (csrc/caser_step.h), for per-op parity: with z [batch, features] (features = F), fc = W1
 * [width, F] followed by b1 [width] (bsarec_caser_fc_floats(cfg) = width F + width floats for a convolution config),
 *   forward   zd = z (.) m,  s = max(0, zd W1^T + b1) [batch, width];  m = keep / (1 - dropout) of the library's Philox stream,
 *             site 0, element index b F + k, keyed by state[0] = seed and state[1] = the step counter, which this call READS
 *             (it advances nothing).  train = 0 or dropout = 0: m = 1, no draw.
 *   backward  du = ds where s > 0, else 0 (an s of exactly 0 passes nothing);  dfc = [dW1 = du^T zd | db1 = sum_b du];
 *             dz = (du W1) (.) m [batch, F].  Every float of dz and dfc is overwritten.
 * A masked forward (train != 0 and dropout > 0) leaves zd in the workspace and bsarec_caser_fc_bwd with the same arguments reads
 * it from the SAME workspace; the mask of dz is regenerated.  Without a mask the workspace is not touched (zd is z).
 *   All products run on v_mfma_f32_16x16x4_f32 in fp32.  Every sum has one order that is a function of the shape alone (the
 * forward splits F over eight waves, four at width > 128, the weight gradient the batch over four; the waves' parts are added in
 * wave order): no atomics, equal bits
 * on every run, and a row of s does not depend on the other rows of the batch.  Launches on `stream`: forward 1, backward 2
 * (dz; dW1 + db1).  No allocation, no host synchronisation, no scratch: capturable.
 *   Workspace: bsarec_caser_fc_workspace_bytes(batch, features, width) = 4 batch F bytes (host-only query).
 *   Limits (else < 0 before any HIP call): 1 <= batch <= 65536; features in 4 .. 12288 and a multiple of 4; width in 4 .. 256
 * and a multiple of 4; 0 <= dropout < 1 (NaN refused); every pointer non-null, float arrays and the workspace 16-byte aligned,
 * state 8-byte; workspace_bytes at least the queried size.  Outputs may not alias inputs, each other or the workspace.
 *
 * One Caser training step: with E = item_emb [V, d], x = E[ids] [B, L, d] (no mask on x), z = bsarec_caser_fwd(x),
 * s = the forward above with dropout = cfg->dropout, and
 *   diff_b = s_b . E[answers_b] - s_b . E[neg_answers_b],  loss = mean_b -log(sigmoid(diff_b) + 1e-10),
 * bsarec_caser_loss_grad writes the loss (one float) and the gradient of every parameter: d_item_emb [V, d] -- the lookup rows
 * dE[ids[b, t]] += dx[b, t] plus the head's 2 B rows; EVERY float is written, zero where no row was touched -- dweights in the
 * layout of bsarec_caser_fwd's weights and dfc in the layout of fc.  Id 0 is an ordinary row.  The head, the fixed-point row
 * scatter (2^-40 units, exact while |sum| < 2^22), the flush and the closing block are those of bsarec_gru4rec_loss_grad.
 *   `state` is u64[8] as there: [0] = seed, [1] = forward-step counter, [2] = Adam t.  A call with train != 0 advances the step
 * counter FIRST and draws with the new value; train = 0 draws nothing (the result of dropout = 0) and touches no counter.
 *   bsarec_caser_train_step is the above with train = 1 followed by Adam on the three arrays, Adam's t advanced ONCE:
 * adam_items->params / grads are E / dE with n = V d, adam_weights the convolution's flat array with
 * n = bsarec_caser_weight_floats(&cfg->conv), adam_fc the fc array with n = bsarec_caser_fc_floats(&cfg->conv); grads are written,
 * then read.  lr, beta1 and beta2 of the three must agree (one t and one pair of bias corrections serve all); shadow_bf16,
 * grads2, grads2_n, n_grad_srcs and wimage_plan must be null / 0.
 *   Launches, all on `stream`, one after the other: the step counter (train != 0), the lookup (which also clears the
 * accumulator), bsarec_caser_fwd(train = 1), the fc forward, the BPR rows, the fc backward, bsarec_caser_bwd, the item-table
 * gradient over L B + 2 B rows, its flush with the mean loss (and Adam's t) in a closing block, then one Adam launch per array.
 * No allocation, no host synchronisation: capturable, and a replay of a captured bsarec_caser_train_step is the NEXT step -- a
 * fresh mask, the next t.  Every output is bit-deterministic, and the result does not depend on what the workspace holds on entry.
 *   Workspace: bsarec_caser_step_workspace_bytes(cfg) bytes (host-only query).  In floats, with T = L B and F as above: the
 * convolution workspace of train = 1 | x [T, d] | z [B, F] | zd [B, F] | s [B, d] | ds [B, d] | dz [B, F] | dx [T, d] |
 * c [B, rounded up to 4] | loss rows [B, rounded up to 4] | the accumulator, V d 64-bit words.
 *   Limits (else < 0 before any HIP call): cfg->conv inside the limits of bsarec_caser_workspace_bytes; item_size >= 2;
 * 0 <= dropout < 1 (NaN refused); every pointer non-null; the float arrays (Adam's four included) and the workspace 16-byte
 * aligned, ids / answers / neg_answers / state 8-byte, loss_out 4-byte; workspace_bytes at least the queried size; adam_*->n as
 * above.  ids, answers and neg_answers inside [0, V) are the caller's contract (a value outside is never dereferenced).  Outputs
 * may not alias inputs, each other or the workspace. */
typedef struct {
    bsarec_caser_config_t conv;
    int item_size;                     /* V >= 2 */
    float dropout;                     /* p in [0, 1), on z */
} bsarec_caser_step_config_t;
long bsarec_caser_fc_floats(const bsarec_caser_config_t *cfg);
long bsarec_caser_fc_workspace_bytes(int batch, int features, int width);
int bsarec_caser_fc_fwd(int batch, int features, int width, const float *z, const float *fc, const void *state, int train,
                        float dropout, float *s, void *workspace, long workspace_bytes, void *stream);
int bsarec_caser_fc_bwd(int batch, int features, int width, const float *z, const float *fc, const float *s, const float *ds,
                        const void *state, int train, float dropout, float *dz, float *dfc,
                        void *workspace, long workspace_bytes, void *stream);
long bsarec_caser_step_workspace_bytes(const bsarec_caser_step_config_t *cfg);
int bsarec_caser_loss_grad(const bsarec_caser_step_config_t *cfg, const float *item_emb, const float *weights, const float *fc,
                           const int64_t *ids, const int64_t *answers, const int64_t *neg_answers,
                           void *state, int train, float *loss_out, float *d_item_emb, float *dweights, float *dfc,
                           void *workspace, long workspace_bytes, void *stream);
int bsarec_caser_train_step(const bsarec_caser_step_config_t *cfg, const int64_t *ids, const int64_t *answers,
                            const int64_t *neg_answers, const bsarec_adam_t *adam_items, const bsarec_adam_t *adam_weights,
                            const bsarec_adam_t *adam_fc, void *state, float *loss_out,
                            void *workspace, long workspace_bytes, void *stream);

/* The personalised Caser step (csrc/caser_user.h): the step above with a user table P = user_emb [U, d] and a second
 * Linear + ReLU, fc2 = W2 [d, 2 d] followed by b2 [d] (bsarec_caser_fc2_floats(cfg) = 2 d d + d floats).  With z1 the s of the
 * step above (relu(fc1(Dropout(z))), [B, d]) and users int64 [B]:
 *   x2 = [ z1 | P[users] ] [B, 2 d];   s = max(0, x2 W2^T + b2) [B, d];   the BPR head of the step above on this s.
 * bsarec_caser_user_loss_grad writes the loss and the gradient of every parameter: d_item_emb, dweights and dfc as above,
 * d_user_emb [U, d] -- row u is the sum of dx2[b, d:2d] over the rows b with users[b] = u, duplicates included; EVERY float is
 * written, exactly zero where no row names the user -- and dfc2 in the layout of fc2.  A user id is the 0-based index of the
 * user; id 0 is an ordinary row; an id outside [0, U) is never dereferenced: its half of x2 is zero and it adds nothing.
 *   fc2 runs on the launches of bsarec_caser_fc_fwd / _bwd with features = 2 d and no mask (the sums and their orders are those
 * documented there).  The user rows are summed by the fixed-point row scatter of the item table (2^-40 units, exact while
 * |sum| < 2^22) into an accumulator of their own, which the concatenation launch clears.  `state` and `train` as above.
 *   bsarec_caser_user_train_step is the above with train = 1 followed by Adam on the five arrays, Adam's t advanced ONCE:
 * adam_items (n = V d), adam_users (n = U d), adam_weights, adam_fc as above, adam_fc2 (n = bsarec_caser_fc2_floats).  lr, beta1
 * and beta2 of the five must agree; shadow_bf16, grads2, grads2_n, n_grad_srcs and wimage_plan must be null / 0.
 *   Launches, all on `stream`, one after the other: the step counter (train != 0), the item lookup, bsarec_caser_fwd (2), the
 * fc1 forward, the concatenation, the fc2 forward, the BPR rows on s, the fc2 backward (2), the user gradient with the split of
 * dx2, the fc1 backward (2), bsarec_caser_bwd (3), the item-table gradient, the user flush, the item flush with the mean loss
 * (and Adam's t) in its closing block, then one Adam launch per array.  No allocation, no host synchronisation: capturable, a
 * replay is the NEXT step.  Every output is bit-deterministic (no floating-point atomics, every sum in an order that is a
 * function of the shape alone) and does not depend on what the workspace holds on entry.
 *   Workspace: bsarec_caser_user_step_workspace_bytes(cfg) bytes (host-only query).  In floats: the regions of
 * bsarec_caser_step_workspace_bytes(&cfg->step) in their order -- its s region holds z1, its ds region d(z1) -- then
 * x2 [B, 2 d] | s [B, d] | ds [B, d] | dx2 [B, 2 d] | the user accumulator, U d 64-bit words.
 *   Limits (else < 0 before any HIP call): those of bsarec_caser_loss_grad / _train_step for cfg->step and every argument they
 * share; num_users >= 1; user_emb, fc2, d_user_emb and dfc2 (Adam's four included) non-null and 16-byte aligned, users 8-byte;
 * workspace_bytes at least the queried size. */
typedef struct {
    bsarec_caser_step_config_t step;
    int num_users;                     /* U >= 1 */
} bsarec_caser_user_step_config_t;
long bsarec_caser_fc2_floats(const bsarec_caser_config_t *cfg);
long bsarec_caser_user_step_workspace_bytes(const bsarec_caser_user_step_config_t *cfg);
int bsarec_caser_user_loss_grad(const bsarec_caser_user_step_config_t *cfg, const float *item_emb, const float *user_emb,
                                const float *weights, const float *fc, const float *fc2, const int64_t *ids,
                                const int64_t *users, const int64_t *answers, const int64_t *neg_answers,
                                void *state, int train, float *loss_out, float *d_item_emb, float *d_user_emb,
                                float *dweights, float *dfc, float *dfc2,
                                void *workspace, long workspace_bytes, void *stream);
int bsarec_caser_user_train_step(const bsarec_caser_user_step_config_t *cfg, const int64_t *ids, const int64_t *users,
                                 const int64_t *answers, const int64_t *neg_answers, const bsarec_adam_t *adam_items,
                                 const bsarec_adam_t *adam_users, const bsarec_adam_t *adam_weights,
                                 const bsarec_adam_t *adam_fc, const bsarec_adam_t *adam_fc2, void *state, float *loss_out,
                                 void *workspace, long workspace_bytes, void *stream);

/* Band-limited autocorrelation attention of the FEARec sibling model (csrc/fea_attn.h): with q, k, v [B, L, D] (D = width),
 * F = L / 2 + 1 and a band lo <= f < hi of rfft bins,
 *   Qf[b, c, f] = sum_t q[b, t, c] e^{-2 pi i f t / L} (Kf alike),  S[b, f] = sum_c Qf[b, c, f] conj(Kf[b, c, f]),
 *   m[b, tau]   = 1 / (D L) sum_{f in band} w_f Re(S[b, f] e^{+2 pi i f tau / L}),  tau = 0 .. L - 1;  w_f = 1 at f = 0 and at
 *                 f = L / 2 of an even L, else 2 -- irfft(n = L) of the band-masked cross-spectrum, averaged over channels,
 *   idx         = the topk delays with the largest g[tau] = mean_b m[b, tau], ONE set for the batch (train != 0), or with the
 *                 largest m[b, .] per sequence (train = 0); equal values go to the lower tau,
 *   p[b, i]     = softmax_i(m[b, idx_i]),  out[b, t, c] = sum_i p[b, i] v[b, (t + idx_i) mod L, c].
 * bsarec_fea_attn_bwd is the true derivative with idx held fixed (nothing flows through g): every float of dq, dk and dv is
 * overwritten.  It reads what bsarec_fea_attn_fwd left in the SAME workspace with the same cfg.  The kernels evaluate m in its
 * equivalent time-domain form (the Gram matrix's diagonal sums against the band's impulse response, csrc/fea_attn.h), so no
 * spectrum is stored or recomputed.  All arithmetic is fp32 (v_mfma_f32_16x16x4_f32 in the products), the impulse response is
 * summed in fp64.
 *   Every sum has one order that is a function of the shape alone: no atomics, equal bits on every run, and with train = 0
 * nothing of a sequence depends on the rest of the batch.  Launches, all on `stream`, one after the other: forward 3 (4 with
 * train != 0), backward 3.  No allocation, no host synchronisation: capturable.
 *   Workspace: bsarec_fea_attn_workspace_bytes(cfg) bytes (host-only query, no HIP call).  In 4-byte words, each part at an
 * offset rounded up to a multiple of 4: m [B, L] float at 0 | idx int32, [topk] (train != 0) or [B, topk], at
 * round_up(B L, 4) | p [B, topk] | the impulse response [L] | cv [B, L] (backward only).
 *   Limits (else < 0 before any HIP call, nothing written): 1 <= batch <= 65536, 2 <= seq_len <= 256, width in 4 .. 256 and a
 * multiple of 4, 0 <= lo < hi <= seq_len / 2 + 1, 1 <= topk <= min(seq_len, 32); every pointer non-null and 16-byte aligned;
 * workspace_bytes at least the queried size.  Outputs may not alias inputs, each other or the workspace.  Inputs are assumed
 * finite. */
typedef struct {
    int batch, seq_len, width, lo, hi, topk, train;
} bsarec_fea_attn_config_t;
long bsarec_fea_attn_workspace_bytes(const bsarec_fea_attn_config_t *cfg);
int bsarec_fea_attn_fwd(const bsarec_fea_attn_config_t *cfg, const float *q, const float *k, const float *v, float *out,
                        void *workspace, long workspace_bytes, void *stream);
int bsarec_fea_attn_bwd(const bsarec_fea_attn_config_t *cfg, const float *q, const float *k, const float *v, const float *dout,
                        void *workspace, long workspace_bytes, float *dq, float *dk, float *dv, void *stream);

/* Linear recurrent unit layer of the LRURec sibling model (csrc/lru.h): with x [B, L, d] (d = width), ids [B, L] (int64, 0 is
 * padding; a null pointer means no padding) and m_t = (ids[b, t] != 0),
 *   lambda = exp(-exp(nu_log)) (cos(exp(theta_log)) + i sin(exp(theta_log))),
 *   u_t = in_proj.weight x_t + in_proj.bias (first d entries the real part, last d the imaginary part),
 *   v_t = m_t exp(gamma_log) u_t,  h_t = lambda h_{t-1} + v_t (h_{-1} = 0),
 *   y_t = out_proj.weight [Re h_t | Im h_t] + out_proj.bias, y [B, L, d].
 * `weights` is ONE flat fp32 array, every tensor at a multiple of 4 floats: nu_log [d] | theta_log [d] | gamma_log [d] |
 * in_proj.weight [2d, d] | in_proj.bias [2d] | out_proj.weight [d, 2d] | out_proj.bias [d]; bsarec_lru_weight_floats is their
 * sum, 4 d d + 6 d.  bsarec_lru_bwd is the true derivative: every float of dx [B, L, d] and of dweights (the layout of weights)
 * is overwritten.  It reads what bsarec_lru_fwd(train = 1) left in the SAME workspace with the same cfg, ids and weights: v and
 * [Re h | Im h], [B, L, 2d] each.  train = 0 keeps nothing and gives the same y, bit for bit.
 *   The products run in the GEMM core (v_mfma_f32, split-K slabs added in slice order, bias gradients as column sums), the
 * recurrence as a chunked scan over time (csrc/lru.h).  A masked step is selected to 0, so nothing at an item's position depends
 * on what x holds under the padding; a row of padding alone gives y = out_proj.bias bit for bit and dx = 0.  With seq_len = 1,
 * dnu_log and dtheta_log are exact zeros.  Every sum has one order that is a function of the shape alone: no atomics, equal bits
 * on every run, and a sequence's y and dx do not depend on the batch or on its place in it.  Launches, all on `stream`, one after
 * the other: forward 4, backward 11.  No allocation, no host synchronisation, static LDS only: capturable.
 *   Workspace: bsarec_lru_workspace_bytes(cfg, train) bytes (host-only query, no HIP call); train != 0 asks for no less.
 *   Limits (else < 0 before any HIP call, nothing written): 1 <= batch <= 65536, 1 <= seq_len <= 256, width in 4 .. 256 and a
 * multiple of 4; every float pointer non-null and 16-byte aligned; workspace_bytes at least the queried size.  Outputs may not
 * alias inputs, each other or the workspace.  Inputs are assumed finite. */
typedef struct {
    int batch, seq_len, width;
} bsarec_lru_config_t;
long bsarec_lru_weight_floats(const bsarec_lru_config_t *cfg);
long bsarec_lru_workspace_bytes(const bsarec_lru_config_t *cfg, int train);
int bsarec_lru_fwd(const bsarec_lru_config_t *cfg, const float *x, const int64_t *ids, const float *weights, int train, float *y,
                   void *workspace, long workspace_bytes, void *stream);
int bsarec_lru_bwd(const bsarec_lru_config_t *cfg, const float *x, const int64_t *ids, const float *weights, const float *dy,
                   void *workspace, long workspace_bytes, float *dx, float *dweights, void *stream);

/* Selective state-space layer of the Mamba4Rec sibling model (csrc/mamba.h): with x [B, L, d] (d = width), d_inner = expand d,
 * N = d_state, K = d_conv, R = dt_rank, ids [B, L] (int64, 0 is padding; a null pointer means no padding) and
 * m_t = (ids[b, t] != 0),
 *   [xs_t | z_t] = in_proj.weight x_t,
 *   c_t[j] = conv1d.bias[j] + sum_{k<K} conv1d.weight[j, k] (m_s xs_s[j]), s = t - K + 1 + k, terms with s < 0 are 0,
 *   u_t = silu(c_t),  [delta_t | B_t | C_t] = x_proj.weight u_t,  Delta_t = softplus(dt_proj.weight delta_t + dt_proj.bias),
 *   A = -exp(A_log),
 *   m_t = 1: h_t[j, n] = exp(Delta_t[j] A[j, n]) h_{t-1}[j, n] + Delta_t[j] B_t[n] u_t[j];  m_t = 0: h_t = h_{t-1};  h_{-1} = 0,
 *   s_t[j] = sum_n C_t[n] h_t[j, n] + D[j] u_t[j],  y_t = m_t ? s_t silu(z_t) : 0,  out_t = out_proj.weight y_t, out [B, L, d].
 * `weights` is ONE flat fp32 array, every tensor at a multiple of 4 floats: in_proj.weight [2 d_inner, d] | conv1d.weight
 * [d_inner, K] | conv1d.bias [d_inner] | x_proj.weight [R + 2N, d_inner] | dt_proj.weight [d_inner, R] | dt_proj.bias [d_inner] |
 * A_log [d_inner, N] | D [d_inner] | out_proj.weight [d, d_inner]; bsarec_mamba_weight_floats is their sum.  bsarec_mamba_bwd is
 * the true derivative: every float of dx [B, L, d] and of dweights (the layout of weights) is overwritten.  It reads what
 * bsarec_mamba_fwd(train = 1) left in the SAME workspace with the same cfg, ids and weights: the [B, L, .] activations and the
 * state after every 8th step (never the state of every step).  train = 0 keeps nothing and gives the same out, bit for bit.
 *   The products run in the GEMM core (v_mfma_f32, split-K slabs added in slice order, dt_proj.bias's gradient as column sums),
 * the convolution and the scan in csrc/mamba.h.  Padding is a selection: the state is exactly 0 until a sequence's first item, a
 * padded position gives out = 0 and dx = 0 whatever x holds there and adds nothing to any weight gradient.  Every sum has one
 * order that is a function of the shape alone: no atomics, equal bits on every run, and a sequence's out and dx do not depend on
 * the batch or on its place in it.  Launches, all on `stream`, one after the other: forward 7, backward 18.  No allocation, no
 * host synchronisation, static LDS only: capturable.
 *   Workspace: bsarec_mamba_workspace_bytes(cfg, train) bytes (host-only query, no HIP call); train != 0 asks for no less.
 *   Limits (else < 0 before any HIP call, nothing written): 1 <= batch <= 65536, 1 <= seq_len <= 256, width in 4 .. 256 and a
 * multiple of 4, expand 1 or 2, d_state 4, 8, 16 or 32, d_conv in 2 .. 4, dt_rank a multiple of 4 in 4 .. 64; every float
 * pointer non-null and 16-byte aligned; workspace_bytes at least the queried size; no output (out; dx, dweights) overlapping an
 * input, the workspace or the other output.  Inputs are assumed finite. */
typedef struct {
    int batch, seq_len, width, expand, d_state, d_conv, dt_rank;
} bsarec_mamba_config_t;
long bsarec_mamba_weight_floats(const bsarec_mamba_config_t *cfg);
long bsarec_mamba_workspace_bytes(const bsarec_mamba_config_t *cfg, int train);
int bsarec_mamba_fwd(const bsarec_mamba_config_t *cfg, const float *x, const int64_t *ids, const float *weights, int train,
                     float *out, void *workspace, long workspace_bytes, void *stream);
int bsarec_mamba_bwd(const bsarec_mamba_config_t *cfg, const float *x, const int64_t *ids, const float *weights, const float *dout,
                     void *workspace, long workspace_bytes, float *dx, float *dweights, void *stream);

/* One LRURec training step (csrc/lrurec_step.h): with E = item_emb [V, d], T = B L rows and N = layers blocks,
 *   x_0 = Drop_0(LN(E[ids])),
 *   per block k < N:  z = LRU_k(x_k, ids) (bsarec_lru_fwd),  a = LN(Drop_{1+2k}(z) + x_k),
 *                     x_{k+1} = LN(Drop_{2+2k}(dense_2(gelu(dense_1(a)))) + a)       (4 d inner, the erf gelu),
 *   loss = mean_b cross_entropy(x_N[b, L - 1] . E^T, answers_b)                      (bsarec_ce_head_fwd with ldh = L d),
 * LayerNorm TF style with ln_eps inside the root.  Id 0 is an ordinary table row (nn.Embedding without padding_idx); it is masked
 * only inside the recurrent layer.  bsarec_lrurec_loss_grad writes the loss (one float) and the gradient of every parameter:
 * d_item_emb [V, d] -- the CE head's dense dE, which overwrites every row, plus the T lookup rows dE[ids[b, t]] += de[b, t] -- and
 * dweights in the layout of weights.
 *   `weights` is ONE flat fp32 array in the model's state_dict order, every tensor at a multiple of 4 floats:
 *   LayerNorm.weight [d] | LayerNorm.bias [d], then per block the 4 d d + 6 d array of bsarec_lru_fwd | lru.LayerNorm.weight,
 *   .bias [d] | dense_1.weight [4d, d] | dense_1.bias [4d] | dense_2.weight [d, 4d] | dense_2.bias [d] |
 *   feed_forward.LayerNorm.weight, .bias [d];  bsarec_lrurec_weight_floats is their sum, 2 d + N (12 d d + 15 d).
 *   Dropout is the library's Philox stream: site 0 on the embeddings, 1 + 2 k behind block k's recurrent layer, 2 + 2 k behind
 * its dense_2; element index row d + c (oracle dropout_keep(B L d, p, seed, step, site)), keyed by the device-resident step state
 * (`state`: u64[8], [0] = seed, [1] = forward-step counter, [2] = Adam t, [3..6] owned by the library).  A call with train != 0
 * advances the step counter FIRST and draws with the new value; train = 0 draws nothing (the result of dropout = 0) and touches
 * no counter.  Masks are regenerated in the backward, not stored.
 *   Backward: the gradient entering the top block is the head's dh at position L - 1 and zero elsewhere; per block the
 * feed-forward LayerNorm, du with the gelu' epilogue, da with the residual gradient added in the epilogue, dW1, dW2 and both bias
 * gradients as split-K TN products whose slabs are added in slice order (dW2 takes gelu(u) on load), the LayerNorm behind the
 * recurrent layer, bsarec_lru_bwd -- its dweights go straight into the block's slice of the flat gradient -- and dx = its dx + the
 * residual gradient.  Every LayerNorm's d(weight), d(bias) partials are added in one fixed order.  The lookup rows are summed in
 * 64-bit fixed point (2^-40 units, exact while |sum| < 2^22) and added onto the head's dE by one flush: every output is
 * bit-deterministic and does not depend on the order in which rows arrive.
 *   bsarec_lrurec_train_step is the above with train = 1 followed by Adam on both arrays, Adam's t advanced ONCE:
 * adam_items->params / grads are E / dE with n = V d, adam_weights->params / grads the flat array and its gradient with
 * n = bsarec_lrurec_weight_floats(cfg); grads are written, then read.  lr, beta1 and beta2 of the two must agree (one t and one
 * pair of bias corrections serve both); shadow_bf16, grads2, grads2_n, n_grad_srcs and wimage_plan must be null / 0.
 *   Launches, all on `stream`, one after the other: 11 + 28 N for a loss and its gradients (the step counter adds one when
 * train != 0), then one Adam launch per array -- 70 for a training step at N = 2.  No allocation, no host synchronisation, no float
 * atomics, static or launch-sized LDS: capturable, and a replay of a captured bsarec_lrurec_train_step is the NEXT step -- fresh
 * masks, the next t.  The result does not depend on what the workspace holds on entry.
 *   Workspace: bsarec_lrurec_workspace_bytes(cfg) bytes (host-only query, no HIP call).  In floats, with T = L B and T4 = T
 * rounded up to 4: one [4] | xhat0 [T, d] | rstd0 [T4] | x_0 .. x_N [N + 1][T, d] | z [T, d] | per block: the workspace of
 * bsarec_lru_fwd(train = 1), a [T, d], xhat_a [T, d], rstd_a [T4], u [T, 4d], xhat_f [T, d], rstd_f [T4] | dy, dz, dt [T, d] each |
 * du [T, 4d] | da, dxl [T, d] each | dh [B, d] | the workspace of bsarec_ce_head_fwd | slabs of dW1 [ns][4d, d], of dW2
 * [ns][d, 4d], of db1 [ns][4d], of db2 [ns][d] (ns split-K slices, a function of T) | LayerNorm partials [2 N + 1][2][nb][d]
 * (nb <= 256) | the accumulator, V d 64-bit words.
 *   Limits (else < 0 before any HIP call): cfg->lru inside the limits of bsarec_lru_workspace_bytes; 1 <= layers <=
 * BSAREC_MAX_LAYERS; item_size >= 2; 0 <= dropout < 1 and ln_eps > 0 (NaN refused); every pointer non-null; the float arrays
 * (Adam's four included) and the workspace 16-byte aligned, ids / answers / state 8-byte, loss_out 4-byte; workspace_bytes at
 * least the queried size; adam_*->n as above.  ids and answers inside [0, V) are the caller's contract (an id outside is never
 * dereferenced: its table row reads as zeros and its gradient row is dropped).  Outputs may not alias inputs, each other or the
 * workspace. */
typedef struct {
    bsarec_lru_config_t lru;           /* batch B, seq_len L, width d: the limits of bsarec_lru_workspace_bytes */
    int layers;                        /* N, 1 .. BSAREC_MAX_LAYERS */
    int item_size;                     /* V >= 2 */
    float dropout;                     /* p in [0, 1), NaN refused */
    float ln_eps;                      /* > 0; 1e-12 in the model */
} bsarec_lrurec_config_t;
long bsarec_lrurec_weight_floats(const bsarec_lrurec_config_t *cfg);
long bsarec_lrurec_workspace_bytes(const bsarec_lrurec_config_t *cfg);
int bsarec_lrurec_loss_grad(const bsarec_lrurec_config_t *cfg, const float *item_emb, const float *weights,
                            const int64_t *ids, const int64_t *answers, void *state, int train, float *loss_out,
                            float *d_item_emb, float *dweights, void *workspace, long workspace_bytes, void *stream);
int bsarec_lrurec_train_step(const bsarec_lrurec_config_t *cfg, const int64_t *ids, const int64_t *answers,
                             const bsarec_adam_t *adam_items, const bsarec_adam_t *adam_weights, void *state,
                             float *loss_out, void *workspace, long workspace_bytes, void *stream);

/* One Mamba4Rec training step: the LRURec step above with the selective state-space layer inside a block.  The two steps run
 * through ONE host driver (csrc/bsarec_hip.hip, "Block-model training step") that takes the layer as a description -- its weight
 * floats, its train = 1 workspace floats, its forward and its backward call -- and the same six row kernels (csrc/lrurec_step.h).
 * With E = item_emb [V, d], T = B L rows and N = layers blocks,
 *   x_0 = Drop_0(LN(E[ids])),
 *   per block k < N:  z = Mamba_k(x_k, ids) (bsarec_mamba_fwd),  a = LN(Drop_{1+2k}(z) + x_k),
 *                     x_{k+1} = LN(Drop_{2+2k}(dense_2(gelu(dense_1(a)))) + a)       (4 d inner, the erf gelu),
 *   loss = mean_b cross_entropy(x_N[b, L - 1] . E^T, answers_b)                      (bsarec_ce_head_fwd with ldh = L d).
 *   `weights` is ONE flat fp32 array in the model's state_dict order -- but for A_log and D, which stay at their place in the
 *   layer's array --, every tensor at a multiple of 4 floats:
 *   LayerNorm.weight [d] | LayerNorm.bias [d], then per block the M = bsarec_mamba_weight_floats array of bsarec_mamba_fwd,
 *   unchanged | mamba.LayerNorm.weight, .bias [d] | dense_1.weight [4d, d] | dense_1.bias [4d] | dense_2.weight [d, 4d] |
 *   dense_2.bias [d] | feed_forward.LayerNorm.weight, .bias [d];  bsarec_mamba4rec_weight_floats is their sum,
 *   2 d + N (M + 8 d d + 9 d).
 *   Everything else is the contract of bsarec_lrurec_loss_grad / bsarec_lrurec_train_step word for word: id 0 an ordinary table
 * row masked only inside the layer, the Philox dropout stream (element row d + c) and its sites 0, 1 + 2 k, 2 + 2 k, the device
 * `state` u64[8], train != 0 advancing the step counter first and train = 0 drawing nothing and touching no counter, masks
 * regenerated in the backward, the backward of a block with bsarec_mamba_bwd in the layer's place -- its dweights go straight
 * into the block's slice of the flat gradient --, the lookup rows summed in 64-bit fixed point and added onto the head's dense dE
 * by one flush, Adam's t advanced once in the closing block, the Adam structs (n = V d and n = bsarec_mamba4rec_weight_floats).
 *   Launches, all on `stream`, one after the other: 11 + 38 N for a loss and its gradients -- per block 7 + 3 forward and
 * 10 + 18 backward -- (the step counter adds one when train != 0), then one Adam launch per array: 14 + 38 N, 90 for a training
 * step at N = 2.  No allocation, no host synchronisation, no float atomics, static or launch-sized LDS: capturable as one linear
 * chain without parallel branches, and a replay of a captured bsarec_mamba4rec_train_step is the NEXT step.  The result does not
 * depend on what the workspace holds on entry.
 *   Workspace: bsarec_mamba4rec_workspace_bytes(cfg) bytes (host-only query, no HIP call).  In floats, with T = L B and T4 = T
 * rounded up to 4: one [4] | xhat0 [T, d] | rstd0 [T4] | x_0 .. x_N [N + 1][T, d] | z [T, d] | per block: the whole workspace of
 * bsarec_mamba_fwd(train = 1), its backward scratch included, a [T, d], xhat_a [T, d], rstd_a [T4], u [T, 4d], xhat_f [T, d],
 * rstd_f [T4] | dy, dz, dt [T, d] each | du [T, 4d] | da, dxl [T, d] each | dh [B, d] | the workspace of bsarec_ce_head_fwd |
 * slabs of dW1 [ns][4d, d], of dW2 [ns][d, 4d], of db1 [ns][4d], of db2 [ns][d] (ns split-K slices, a function of T) | LayerNorm
 * partials [2 N + 1][2][nb][d] (nb <= 256) | the accumulator, V d 64-bit words.
 *   Limits (else < 0 before any HIP call): cfg->mamba inside the limits of bsarec_mamba_workspace_bytes; the rest as for
 * bsarec_lrurec_*: 1 <= layers <= BSAREC_MAX_LAYERS; item_size >= 2; 0 <= dropout < 1 and ln_eps > 0 (NaN refused); every pointer
 * non-null; the float arrays (Adam's four included) and the workspace 16-byte aligned, ids / answers / state 8-byte, loss_out
 * 4-byte; workspace_bytes at least the queried size; adam_*->n as above.  Outputs may not alias inputs, each other or the
 * workspace. */
typedef struct {
    bsarec_mamba_config_t mamba;       /* B, L, d, expand, d_state, d_conv, dt_rank: the limits of bsarec_mamba_workspace_bytes */
    int layers;                        /* N, 1 .. BSAREC_MAX_LAYERS */
    int item_size;                     /* V >= 2 */
    float dropout;                     /* p in [0, 1), NaN refused */
    float ln_eps;                      /* > 0; 1e-12 in the model */
} bsarec_mamba4rec_config_t;
long bsarec_mamba4rec_weight_floats(const bsarec_mamba4rec_config_t *cfg);
long bsarec_mamba4rec_workspace_bytes(const bsarec_mamba4rec_config_t *cfg);
int bsarec_mamba4rec_loss_grad(const bsarec_mamba4rec_config_t *cfg, const float *item_emb, const float *weights,
                               const int64_t *ids, const int64_t *answers, void *state, int train, float *loss_out,
                               float *d_item_emb, float *dweights, void *workspace, long workspace_bytes, void *stream);
int bsarec_mamba4rec_train_step(const bsarec_mamba4rec_config_t *cfg, const int64_t *ids, const int64_t *answers,
                                const bsarec_adam_t *adam_items, const bsarec_adam_t *adam_weights, void *state,
                                float *loss_out, void *workspace, long workspace_bytes, void *stream);

/* Tag kernel launches of one id with hipEvents for in-process roofline timing (bench.py):
 * when set, every launch of kernel class `kclass` (see BSAREC_K_*) on the next calls of THIS plan is bracketed
 * by hipEventRecord on the launch stream; bsarec_profile_read returns the summed milliseconds and
 * launch count, then resets.  Not for use under graph capture. */
enum { BSAREC_K_NONE = 0, BSAREC_K_FFN1 = 1, BSAREC_K_FFN2 = 2, BSAREC_K_QKV = 3, BSAREC_K_LOGITS = 4,
       BSAREC_K_DU = 5, BSAREC_K_DW1 = 6, BSAREC_K_FUSED_FWD = 7, BSAREC_K_FUSED_BWD = 8 };
int bsarec_profile_select(bsarec_plan_t *plan, int kclass);
/* Diagnostic: device buffer of 32*2*layers int64 that receives per-phase shader-clock stamps of workgroup 0
 * of this plan's fused kernels (null disables). */
int bsarec_debug_stamps(bsarec_plan_t *plan, void *dev_buf);
/* Waits for the plan's recorded event pairs (the one call besides bsarec_plan_create that blocks the host). */
int bsarec_profile_read(bsarec_plan_t *plan, double *ms_total, int *launches);
/* Milliseconds one such hipEvent bracket reads with NO kernel inside it (average of `reps` back-to-back pairs on
 * `stream`): the marker-packet cost bench.py subtracts so that its per-launch time agrees with rocprofv3's. */
int bsarec_profile_event_overhead(void *stream, int reps, double *ms_avg);

#ifdef __cplusplus
}
#endif
#endif /* BSAREC_HIP_H */
