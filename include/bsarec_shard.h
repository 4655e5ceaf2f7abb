/* bsarec_shard.h -- catalogue-sharded head of the BSARec training step (configuration C5: V = 10 M items).
 *
 * New functionality: the reference is single-device (src/main.py:19); what is sharded here is its full-catalogue head
 *     logits = seq_output[:, -1, :] @ item_embeddings.weight^T ;  loss = CrossEntropyLoss(logits, answers)
 * (src/model/bsarec.py:32-35) and the item-embedding lookup (src/model/_abstract_model.py:14-24).  At C5 a replicated
 * table costs 41 GB per GPU (weights + gradient + Adam moments) and a dense 10.24 GB gradient all-reduce per step; with
 * the catalogue rows sharded W ways (rank r owns rows [r*rows_per, (r+1)*rows_per), their gradient and their moments)
 * the table gradient never crosses a link.  The encoder (everything but the item table) stays a data-parallel
 * replica.  One step, per rank (host side: bsarec_amd/catalogue.py):
 *
 *   bsarec_shard_gather_rows      lookup rows of the local batch, read out of the owners' shards (IPC-mapped, xGMI)
 *   bsarec_forward                the ordinary encoder plan over the staging table (item_size = B*L + 1)
 *   all-gather h_last, answers    [Bg, d] + [Bg]  (Bg = W*B; torch.distributed)
 *   bsarec_shard_logits           partial logits of all Bg sequences against the owned rows
 *   bsarec_shard_ce_stats         per-row (max, sum exp, target logit) of the owned slice
 *   all-gather stats              [W, 3, Bg]
 *   bsarec_shard_ce_grad          lse / loss from everybody's statistics; d loss / d logits of the owned slice
 *   bsarec_shard_head_bwd         dE of the owned rows (complete, local) + partial d h_last of all Bg sequences
 *   reduce-scatter d h_last       [Bg, d] -> [B, d]
 *   bsarec_backward_seq           encoder backward; the staging table's gradient = one row per token
 *   bsarec_comm_barrier           (bsarec_comm.h)
 *   bsarec_shard_scatter_rows     owners pull the token rows of their items out of every rank's staging gradient
 *   bsarec_adam_step / _apply     encoder: sum of every rank's gradient arena (grad_srcs); shard: local dE
 *
 * Sampled-softmax head (opt-in, the single-GPU head of bsarec_hip.h, train_negatives = N > 0, over the shards; host side:
 * ShardedCatalogue with train_negatives): the all-gather of h_last, the logits / statistics / head backward of the owned
 * rows and the all-reduce of d h_last are replaced by, per rank (B local rows, Bg = world*B):
 *
 *   bsarec_shard_ssm_draw         the step's N candidates: the same on every rank, no communication
 *   bsarec_shard_ssm_gather       (after the step's first barrier) the B answer rows and the N candidate rows from the owners
 *   bsarec_shard_ssm_head         logits [B, N+1], loss rows, d loss / d logits = (softmax - onehot_0) / Bg of the local rows
 *   all-gather loss rows          [Bg] -> bsarec_shard_ssm_loss: the mean over the global batch in rank order
 *   bsarec_shard_ssm_bwd          complete d h_last of the local rows; the head gradient rows [B+N, hidden] (IPC-exported)
 *   bsarec_backward_seq, barrier  as above
 *   bsarec_shard_ssm_pull         owners add every rank's answer rows and the rank-ordered sum of the candidate partials
 *   bsarec_shard_scatter_rows     as above
 *   Adam                          dense (bsarec_adam_apply over the shard; dE zeroed once per step), or lazy:
 *                                 bsarec_shard_lazy_mark + bsarec_shard_lazy_adam over the owned rows the step touched
 *
 * Full-catalogue CE without the partial logits (opt-in, ShardedCatalogue with shard_ce_head = "fused"): bsarec_shard_logits,
 * bsarec_shard_ce_stats, bsarec_shard_ce_grad and bsarec_shard_head_bwd are replaced by bsarec_ce_head_range_stats, the same
 * all-gather of the statistics, bsarec_ce_head_range_merge and bsarec_ce_head_range_bwd (bsarec_hip.h): the same loss, dE and
 * partial d h_last with no [Bg, Vs] buffer.
 *
 * Same conventions as bsarec_hip.h: plain pointers and sizes, caller-owned memory, caller's stream, no synchronisation,
 * return 0 / <0 invalid argument / >0 hipError_t.  fp32.  hidden % 4 == 0, world <= 8.
 */
#ifndef BSAREC_SHARD_H
#define BSAREC_SHARD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Staging table of one rank's batch.  ids[n] are catalogue ids of the n = B*L tokens; shards[r] is rank r's table
 * shard [rows_per_shard, hidden] (device pointers valid in THIS process: the local shard and IPC mappings of the
 * peers').  stage[(n+1), hidden]: row 0 = E[0], row j+1 = E[ids[j]]; local_ids[j] = j+1, or 0 where ids[j] == 0.
 * Ids outside [0, item_size) are clamped like everywhere else in the library. */
int bsarec_shard_gather_rows(const int64_t *ids, long n, const float *const *shards, int world, long rows_per_shard,
                             long item_size, int hidden, float *stage, int64_t *local_ids, void *stream);

/* logits[b, v] = h[b, :] . E_shard[v, :] for b < Bg, v < Vs; row stride ld >= Vs, ld % 4 == 0.  h has row stride ldh. */
int bsarec_shard_logits(const float *h, long ldh, int Bg, const float *E_shard, int Vs, int hidden, float *logits, long ld,
                        void *stream);

/* stats[3][Bg] = per row: max over the owned slice, sum exp(x - max), logits[b, answers[b] - lo] if this rank owns the
 * answer else 0.  (An empty slice reports -inf, 0, 0.) */
int bsarec_shard_ce_stats(const float *logits, long ld, int Bg, int Vs, const int64_t *answers, long lo, long item_size,
                          float *stats, void *stream);

/* stats_all[world][3][Bg] (every rank's stats, rank order) -> loss_rows[Bg] = lse - target logit, loss[0] = their mean
 * (identical on every rank), and logits := (softmax - onehot) / Bg in place over the owned slice (columns Vs..ld-1 := 0). */
int bsarec_shard_ce_grad(float *logits, long ld, int Bg, int Vs, const int64_t *answers, long lo, long item_size,
                         const float *stats_all, int world, float *loss_rows, float *loss, void *stream);

/* dE_shard[Vs, hidden] = dlogits^T . h (overwritten: the dense part of the owned rows' gradient, complete);
 * dh[Bg, hidden] = dlogits . E_shard (this rank's partial sum over its rows; split-K slabs in `scratch`). */
long bsarec_shard_head_bwd_scratch_floats(int Bg, int Vs, int hidden);
int bsarec_shard_head_bwd(const float *dlogits, long ld, int Bg, int Vs, const float *h, long ldh, const float *E_shard,
                          int hidden, float *dE_shard, float *dh, float *scratch, void *stream);

/* Lookup-path gradient: ids_all[world][n] (every rank's token ids, rank order), stage_grads[r] = rank r's staging-table
 * gradient [(n+1), hidden] (row j+1 = token j; IPC mappings for the peers).  dE_shard[id - lo] += row for every token
 * whose id is owned (lo <= id < lo + Vs) and not the padding id.  Float atomics: the order of additions is not fixed. */
int bsarec_shard_scatter_rows(const int64_t *ids_all, long n, int world, const float *const *stage_grads, long lo, long Vs,
                              long item_size, int hidden, float *dE_shard, void *stream);

/* ---- sampled-softmax head of the sharded step (1 <= N <= BSAREC_TRAIN_NEG_MAX = 8192) ----------------------------------
 * Draws: the stream of bsarec_hip.h's train_negatives contract with key = `key` (the single-GPU head's state[0]) and step =
 * lo32(state[1]), read on the device (a replayed graph draws afresh).  pop_cum: int64[item_size] cumulative popularity
 * (the popularity sampler; null: uniform over [1, item_size)).  cand[N] (int32) and corr[N] = c(n_j) = log(N q_j) if
 * logq and pop_cum, else 0.  lazy_count (nullable): set to 0 (a lazy-Adam step's row count, before anything marks).
 * With the same key, step, sampler and N the candidates equal those of ONE bsarec_plan training on the global batch. */
int bsarec_shard_ssm_draw(uint64_t key, const uint64_t *state, int N, long item_size, const int64_t *pop_cum, int logq,
                          int *cand, float *corr, int *lazy_count, void *stream);

/* rows[(B + N), hidden]: row b = E[answers[b]] (b < B), row B + j = E[cand[j]], read out of the owners' shards as
 * bsarec_shard_gather_rows reads them (ids clamped to [0, item_size)). */
int bsarec_shard_ssm_gather(const int64_t *answers, int B, const int *cand, int N, const float *const *shards, int world,
                            long rows_per_shard, long item_size, int hidden, float *rows, void *stream);

/* The head of the B local rows: h[b] = h[b * ldh ..] (ldh >= hidden, % 4 == 0); rows from bsarec_shard_ssm_gather; cand /
 * corr from bsarec_shard_ssm_draw.  logits[B, N+1]: x_b0 = h_b . E[a_b] - c(a_b), x_bj = h_b . E[n_j] - c(n_j), -inf where
 * n_j == a_b; loss_rows[B] = logsumexp - x_b0; dlogits[B, N+1] = (softmax - onehot_0) / Bg (Bg: the global batch). */
int bsarec_shard_ssm_head(const float *h, long ldh, int B, int Bg, const float *rows, const int64_t *answers, const int *cand,
                          const float *corr, int N, long item_size, const int64_t *pop_cum, int logq, int hidden,
                          float *logits, float *dlogits, float *loss_rows, void *stream);

/* loss[0] = mean of loss_rows_all[Bg] (every rank's loss rows in rank order: the same value on every rank). */
int bsarec_shard_ssm_loss(const float *loss_rows_all, int Bg, float *loss, void *stream);

/* Head backward of the B local rows.  dh[b * lddh + k] = sum_c dlogits[b, c] rows[c'] (c' = b for c = 0, else B + c - 1):
 * complete for these rows (no exchange); grad_rows[(B + N), hidden] (overwritten): row b = dlogits[b, 0] h_b (the answer
 * row), row B + j = sum_b dlogits[b, 1 + j] h_b (this rank's partial of candidate j).  Split-K slabs of dh in `scratch`. */
long bsarec_shard_ssm_bwd_scratch_floats(int B, int N, int hidden);
int bsarec_shard_ssm_bwd(const float *dlogits, int B, int N, const float *h, long ldh, const float *rows, int hidden,
                         float *dh, long lddh, float *grad_rows, float *scratch, void *stream);

/* Owner pull of the head gradient (after a barrier that follows every rank's bsarec_shard_ssm_bwd): grad_rows[r] = rank r's
 * grad_rows (IPC mappings for the peers), cand[N] the step's candidates, answers_all[world * B] every rank's answers in
 * rank order.  For every candidate slot j with lo <= n_j < lo + Vs: dE_shard[n_j - lo] += sum over r in rank order of
 * grad_rows[r][B + j]; for every owned answers_all[t]: dE_shard[a - lo] += grad_rows[t / B][t % B].  Float atomics where a
 * row is hit more than once: the order of those additions is not fixed. */
int bsarec_shard_ssm_pull(const int64_t *answers_all, int B, int world, const int *cand, int N, const float *const *grad_rows,
                          long lo, long Vs, long item_size, int hidden, float *dE_shard, void *stream);

/* Lazy Adam of the shard (train_lazy_adam).  mark[Vs] (int32, zero between steps), rows[cap], count[1]: the touched owned
 * rows T_own of the step -- ids_all[nids] != 0 (every rank's token ids), answers_all[Bg] and cand[N], clamped to
 * [0, item_size), with lo <= id < lo + Vs -- are marked and listed at their local index (count reset by
 * bsarec_shard_ssm_draw of the same step).  cap = min(Vs, nids + Bg + N). */
int bsarec_shard_lazy_mark(const int64_t *ids_all, long nids, const int64_t *answers_all, int Bg, const int *cand, int N,
                           long lo, long Vs, long item_size, int *mark, int *rows, int *count, int cap, void *stream);

/* Adam on the rows of T_own only (the step's list of bsarec_shard_lazy_mark): E_shard / m / v [Vs, hidden] with gradient
 * dE_shard, the arithmetic of bsarec_adam_apply with the step's t and bias corrections (state[3], advanced by the
 * encoder's bsarec_adam_step), weight decay on these rows only; then their dE rows := 0 and their marks cleared.  Rows
 * outside T_own are not read or written.  The grid is sized by cap, not by Vs. */
int bsarec_shard_lazy_adam(float *E_shard, float *dE_shard, float *m, float *v, int hidden, float beta1, float beta2, float eps,
                           float weight_decay, int *mark, const int *rows, const int *count, int cap, const void *state,
                           void *stream);

#ifdef __cplusplus
}
#endif
#endif /* BSAREC_SHARD_H */
