// MI355X (gfx950) BSARec training hot path: launch plan + C ABI.  See include/bsarec_hip.h.
#include <cmath>
#include "../../include/bsarec_hip.h"
#include "../../include/bsarec_shard.h"
#include "epilogues.h"
#include "kernels.h"
#include "fused_layer.h"
#include "dw_direct.h"
#include "fused_top.h"
#include "fused_chain.h"
#include "comm.h"
#include "catalogue_shard.h"
#include "rank.h"
#include "sampled_rank.h"
#include "full_rank.h"
#include "answer_rank.h"
#include "info_nce.h"
#include "ce_head.h"
#include "cloze.h"
#include "sampled_softmax.h"
#include "lazy_adam.h"
#include "gru.h"
#include "pair_step.h"
#include "gru4rec_cand.h"
#include "caser.h"
#include "caser_step.h"
#include "caser_user.h"
#include "fea_attn.h"
#include "lru.h"
#include "mamba.h"
#include "lrurec_step.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <algorithm>

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return (int)e_; } while (0)
#define RET(x) do { int r_ = (x); if (r_ != 0) return r_; } while (0)

// Dry run: walk the launch sequence, set per-kernel attributes (large dynamic LDS), launch nothing.
// bsarec_plan_create does one dry pass so that the first real pass may already be under graph capture.
static thread_local bool g_dry = false;
#define LAUNCH(...) do { if (!g_dry) hipLaunchKernelGGL(__VA_ARGS__); } while (0)

// Every option lives in bsarec_config_t and belongs to the plan (no process-wide knobs).  Defaults of the 0 values:
//   top_slabs 2  (slab slices of the pruned top block's weight-gradient products, K = B or B*h rows only; measured
//                 1/2/4/8 slabs: 0.2115 / 0.2095 / 0.2122 / 0.2130 ms per step)
//   splits    32 at the fused shape, 40 elsewhere (slab slices of the full-block weight-gradient products)
struct bsarec_plan;
static thread_local bsarec_plan* t_plan = nullptr;   // plan of the C call this thread is inside (ProfScope, stamps)

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }
static inline long rup(long a, long b) { return (a + b - 1) / b * b; }

// ---------------------------------------------------------------------------------------------
// in-process kernel timing (bench.py roofline): hipEvent pairs around one kernel class
// ---------------------------------------------------------------------------------------------
struct ProfState {                    // per plan (bsarec_profile_select / _read)
    int kclass = BSAREC_K_NONE;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
    size_t used = 0;
    ~ProfState() { for (auto& e : events) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); } }
};

// ---------------------------------------------------------------------------------------------
// plan
// ---------------------------------------------------------------------------------------------
struct LayerBufs {
    float *dsp, *xhat_f, *rstd_f, *q, *k, *v, *probs, *ctx, *xhat_a, *rstd_a, *hmix, *u, *xhat_ff, *rstd_ff;
    float* gp;       // fused path: gelu'(pre-activation) [T, 4d]; there `u` holds gelu(pre-activation) (one-row top block: u itself)
};

struct bsarec_plan {
    bsarec_config_t cfg;
    bsarec_tensors_t P, G, S;                  // parameters, gradients, bf16 shadow of the parameters (storage = 1)
    bool bf;                                   // cfg.storage == 1 at the fused shape: bf16 storage + bf16 MFMA in the block kernels
    bool bf_products;                          // cfg.storage == 1 elsewhere: fp32 tensors, bf16 products in the tiled GEMMs (gemm.h)
    char* ws; size_t ws_bytes;
    uint64_t* state;
    const float* twiddle;
    int T, Lp, Vp, dh, nblk, rows_pb, nsplit, kchunk, vsplit, vchunk;
    bool fused;        // fused per-sequence block kernels (decided at plan creation)
    bool train;        // mode of the last forward
    // activations kept for backward
    int* ids32;
    float* X[BSAREC_MAX_LAYERS + 1];
    float *xhat0, *rstd0;
    LayerBufs lb[BSAREC_MAX_LAYERS];
    float *logits, *dlogits, *loss_rows, *loss;
    // backward scratch (shared by all layers)
    float *dXa, *dXb, *dz, *dT, *dU, *dH, *dXacc, *dO, *dF, *dC, *dS, *dq, *dk, *dv, *dXtmp, *dlast_slab;
    float *slab_wL[BSAREC_MAX_LAYERS], *slab_bL[BSAREC_MAX_LAYERS], *part_lnL[BSAREC_MAX_LAYERS], *part_betaL[BSAREC_MAX_LAYERS];
    float *part_ln0, *part_pos, *trash;
    int pos_slices;
    ReduceJob* jobs; int jobs_per_layer;
    ReduceJob* jobs_pruned;                    // same table with the top layer's key / value bias jobs fed from partials
    bool prune_ok;                             // the loss path may run the pruned top block (fused shape, >= 2 layers)
    bool pruned;                               // mode of the last forward
    int loss_kind;                             // head of the last loss call: 0 = full-catalogue CE, 1 = SASRec's BCE pair,
                                               // 2 = sampled softmax (cfg.train_negatives > 0)
    const float* ext_dy = nullptr;             // bsarec_backward_seq: upstream gradient of the last layer's output, all positions
    const float* ext_mid[BSAREC_MAX_LAYERS] = {};   // bsarec_backward_seq_multi: upstream gradients of layer outputs 0 .. N-1 (null: none)
    const int64_t *bce_pos, *bce_neg;
    float *part_kvb, *slab_dummy;
    float* part_cwL[BSAREC_MAX_LAYERS];        // FMLPRec: per-sequence d(complex_weight) [B][cb][d][2]
    float *top_dq, *top_dO, *top_dT, *top_dU, *top_ak, *top_rk, *top_av, *top_rv;              // [2][B][d] key / value bias partials of the pruned top block; [nsplit][4d] sink
    int* blockmap; int red_blocks;           // flat block -> (job, chunk) table of the final gradient reduction
    long red_elems; const float *red_lo, *red_hi;   // what the reduction jobs write: element count, address range
    // options resolved from cfg (0 = default there)
    int top_slabs; bool embed_in_block, direct_dw;
    bool scatter_in_block;                     // fused path: the embedding-gradient scatter rides in block 0's weight-gradient launch
    ProfState prof;
    long long* stamps = nullptr;             // diagnostic stamp buffer (bsarec_debug_stamps)
    bsarec_hook_t dense_hook = nullptr; void* dense_hook_user = nullptr;   // bsarec_plan_set_dense_grad_hook
    float* lookup_grad = nullptr;            // target of the embedding scatter when the dense dE is exchanged early
    unsigned long long* lookup_acc = nullptr;  // [V][d] fixed-point sum of the scatter (kernels.h), zero between steps
    // sampled-softmax head (cfg.train_negatives > 0; sampled_softmax.h)
    int* ssm_cand = nullptr; float *ssm_corr = nullptr, *ssm_logits = nullptr, *ssm_dlogits = nullptr;
    const int64_t* pop_cum = nullptr;          // bsarec_plan_set_train_sampler (train_sampler = 1)
    const int64_t* ssm_answers = nullptr;      // answers of the last sampled loss (the backward reads them)
    int ssm_nslab = 0;                         // split-K slabs of d(h_last) (ssm_split with the cap of plan_ssm_params)
    // lazy Adam (cfg.train_lazy_adam = 1; lazy_adam.h): the touched-row marks and list, used while a step runs lazily
    LazyRows lazy = {};
    bool lazy_now = false;                     // set by bsarec_train_step / _indexed around their launches (LazyStep)
    // fragment image of the Linear weights (cfg.weight_image; wimage.h): [layers][wimage_layer_floats(d)], the caller's
    // memory (bsarec_plan_create); null = the block kernels read the masters
    float* wimg = nullptr;
    // keep bits of the dropout masks (drop_bits.h): one buffer per layer, written by the forward block kernels of a training
    // step and read by the matching backward; carved wherever drop_bits_wanted(cfg), used while drop_bits is set
    // (bsarec_plan_set_drop_bits; on by default)
    unsigned char* dbitsL[BSAREC_MAX_LAYERS] = {};
    bool drop_bits = true;
    bool bidir = false;                        // attention without the causal term (bsarec_plan_set_bidirectional)
};
struct PlanScope {                           // marks the plan a C call works on for this thread (nesting-safe)
    bsarec_plan* prev;
    explicit PlanScope(bsarec_plan* p) : prev(t_plan) { t_plan = p; }
    ~PlanScope() { t_plan = prev; }
};

struct ProfScope {
    hipStream_t s; bool on; hipEvent_t stop;
    ProfScope(int kclass, hipStream_t st) : s(st), on(false) {
        ProfState* ps = t_plan ? &t_plan->prof : nullptr;
        on = ps && kclass != BSAREC_K_NONE && kclass == ps->kclass;
        if (!on) return;
        if (ps->used == ps->events.size()) {
            hipEvent_t a, b;
            (void)hipEventCreate(&a); (void)hipEventCreate(&b);
            ps->events.push_back({a, b});
        }
        (void)hipEventRecord(ps->events[ps->used].first, s);
        stop = ps->events[ps->used].second;
        ++ps->used;
    }
    ~ProfScope() { if (on) (void)hipEventRecord(stop, s); }
};

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
// Launch of a kernel with dynamic LDS: raises the kernel's limit when smem exceeds the 48 KiB default and the largest size
// this instantiation has asked for so far, then launches unless this is the dry pass.  The raise must not first happen under
// graph capture: bsarec_plan_create's dry pass walks every launch sequence a step of that plan can take.
template <auto Kernel, class... A>
static int launch_lds(dim3 grid, dim3 block, size_t smem, hipStream_t s, const A&... a) {
    static size_t raised = 0;
    if (smem > 48 * 1024 && smem > raised) {
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        raised = smem;
    }
    if (g_dry) return 0;
    hipLaunchKernelGGL(Kernel, grid, block, smem, s, a...);
    return (int)hipGetLastError();
}

static GemmP gemm_defaults(int M, int N, int K) {
    GemmP P;
    memset(&P, 0, sizeof(P));
    P.M = M; P.N = N; P.K = K; P.Nb = N; P.Kv = K;
    P.nseg = 1; P.nprob = 1; P.nsplit = 1; P.kchunk = K; P.nh = 1;
    return P;
}

template <int BM, int BN, int WM, int WN, bool AKM, bool BKM, int AXF, int BXF, bool BG, bool BF, class Epi>
static int launch_gemm_as(const GemmP& P, const XformP& X, const Epi& epi, float* bgrad, int nbatch, hipStream_t s, int kclass) {
    if (P.M <= 0 || P.N <= 0) return 0;
    const dim3 grid(cdiv(P.M, BM), cdiv(P.N, BN), nbatch * P.nprob * P.nsplit);
    ProfScope prof(g_dry ? BSAREC_K_NONE : kclass, s);
    return launch_lds<gemm_kernel<BM, BN, WM, WN, AKM, BKM, AXF, BXF, BG, BF, Epi>>(grid, dim3(64 * WM * WN),
                                                                                  GemmSmem<BM, BN, AKM, BKM, BF>::BYTES, s, P, X, epi, bgrad);
}

// fp32_only: the products of the loss head (logits and their backward) stay fp32 in the bf16-product mode, as they do under
// the fused bf16 storage
template <int BM, int BN, int WM, int WN, bool AKM, bool BKM, int AXF, int BXF, bool BG, class Epi>
static int launch_gemm(const GemmP& P, const XformP& X, const Epi& epi, float* bgrad, int nbatch, hipStream_t s,
                       int kclass = BSAREC_K_NONE, bool fp32_only = false) {
    if (!fp32_only && t_plan && t_plan->bf_products) {
        // token-parallel products (M = B L rows, one problem): a 64 x 64 tile issues ~120 instructions and 16 KB of fp32 operand
        // loads per 0.26 MFLOP k-step, which is what bounds it once the matrix time is gone -- 128 x 128 tiles quarter that
        if constexpr (BM == 64 && BN == 64 && !BG)
            if (P.M >= 8192 && P.N >= 128 && nbatch == 1)
                return launch_gemm_as<128, 128, WM, WN, AKM, BKM, AXF, BXF, BG, true, Epi>(P, X, epi, bgrad, nbatch, s, kclass);
        return launch_gemm_as<BM, BN, WM, WN, AKM, BKM, AXF, BXF, BG, true, Epi>(P, X, epi, bgrad, nbatch, s, kclass);
    }
    // fp32, 256-wide tiles (LayerNorm / softmax / dS epilogues at hidden or L > 128): 8 waves as 2 x 4 -- the 92 KB of
    // fp32 staging allow one workgroup per CU, and four waves at 344 registers left every SIMD with a single wave
    if constexpr (BN == 256 && WM * WN == 4)
        return launch_gemm_as<BM, BN, 2, 4, AKM, BKM, AXF, BXF, BG, false, Epi>(P, X, epi, bgrad, nbatch, s, kclass);
    else
        return launch_gemm_as<BM, BN, WM, WN, AKM, BKM, AXF, BXF, BG, false, Epi>(P, X, epi, bgrad, nbatch, s, kclass);
}

static XformP no_xform() { XformP X; memset(&X, 0, sizeof(X)); return X; }

template <bool BIAS, bool ADD, bool GGRAD>
static EpiLinear<BIAS, ADD, GGRAD> epi_linear(float* C, long ldc) {
    EpiLinear<BIAS, ADD, GGRAD> e;
    memset(&e, 0, sizeof(e));
    e.C[0] = C; e.ldc = ldc;
    return e;
}

// ---------------------------------------------------------------------------------------------
// plan: configuration checks, derived sizes, workspace carve, creation
// ---------------------------------------------------------------------------------------------
struct Carver {
    char* base; size_t off;
    explicit Carver(char* b) : base(b), off(0) {}
    template <class T> T* take(size_t n) {
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += rup((long)(n * sizeof(T)), 256);
        return p;
    }
};

static int check_cfg(const bsarec_config_t& c) {
    if (c.batch < 1 || c.seq_len < 1 || c.seq_len > 256) return -1;
    if (c.hidden < 4 || c.hidden > 256 || c.hidden % 4) return -2;
    if (c.heads < 1 || c.hidden % c.heads || (c.hidden / c.heads) % 4) return -3;
    if (c.layers < 1 || c.layers > BSAREC_MAX_LAYERS) return -4;
    if (c.item_size < 2) return -5;
    if (c.cutoff_bins < 1 || c.cutoff_bins > c.seq_len / 2 + 1) return -6;
    if ((long)c.cutoff_bins * c.hidden > 8192) return -7;      // spectrum must fit the LDS carve
    if (c.p_hidden < 0.f || c.p_hidden >= 1.f || c.p_attn < 0.f || c.p_attn >= 1.f) return -8;
    if (c.filter_kind != 0 && c.filter_kind != 1) return -9;
    if (c.filter_kind == 1 && c.cutoff_bins != c.seq_len / 2 + 1) return -9;     // the learnable filter has every rFFT bin
    if (c.hidden_act < 0 || c.hidden_act > 4) return -14;
    if (c.storage < 0 || c.storage > 1) return -15;
    if (c.splits < 0 || c.splits > 1024 || c.top_slabs < 0 || c.top_slabs > 16) return -16;
    if (c.train_negatives < 0 || c.train_negatives > BSAREC_TRAIN_NEG_MAX) return -17;
    if (c.train_sampler < 0 || c.train_sampler > 1 || c.train_no_logq < 0 || c.train_no_logq > 1) return -17;
    if (c.train_negatives > 0 && c.storage != 0) return -18;      // the sampled head is fp32 only
    if (c.train_lazy_adam < 0 || c.train_lazy_adam > 1 || (c.train_lazy_adam && c.train_negatives == 0)) return -19;
    if (c.weight_image < 0 || c.weight_image > 1) return -20;
    return 0;
}

static bool fused_shape_ok(const bsarec_config_t& c);
// fragment image: only where the fp32 LDS-phase block kernels run (the bf16 / x3 / chain / FMLPRec variants read the masters)
static bool wimage_wanted(const bsarec_config_t& c) {
    return c.weight_image && fused_shape_ok(c) && c.storage == 0 && !c.x3_products && !c.chain_kernels && c.filter_kind == 0;
}

// keep bits: where the LDS-phase BSARec block kernels run both directions in fp32 or bf16 storage (the x3, chain and FMLPRec
// variants evaluate Philox in both) and the embedding front-end rides in the bottom block (derive: embed_in_block)
static bool drop_bits_wanted(const bsarec_config_t& c) {
    return fused_shape_ok(c) && c.filter_kind == 0 && (c.storage == 1 || (!c.x3_products && !c.chain_kernels && !c.separate_embed));
}

static bool fused_shape_ok(const bsarec_config_t& c) {
    const int dh = c.hidden / c.heads;
    if (c.no_fused || c.hidden_act != 0 || c.hidden != 64 || c.seq_len > 64 || !(dh == 16 || dh == 32 || dh == 64)) return false;
    // filter_kind 1 (the sibling model FMLPRec: learnable complex filter over all L/2 + 1 bins, no attention branch) has its own
    // instantiation of the block kernels, fp32 storage only
    if (c.filter_kind == 1) return c.storage == 0 && c.alpha == 1.0f && c.cutoff_bins <= 36;
    return c.cutoff_bins <= FUSED_MAX_CB;
}

// sampled head: d(h_last) split-K over the candidates, at most cap (<= SSM_SLAB_MAX) slabs of >= 256 candidate columns
#define SSM_SLAB_MAX 32
static void ssm_split(int N, int cap, int* nslab, int* chunk) {
    const int want = std::max(1, std::min(cap, N / 256));
    *chunk = (int)rup(cdiv(N, want), SSM_KS);
    *nslab = cdiv(N, *chunk);
}

static void derive(bsarec_plan& p) {
    const bsarec_config_t& c = p.cfg;
    p.fused = fused_shape_ok(c);
    p.bf = c.storage == 1 && p.fused;
    p.bf_products = c.storage == 1 && !p.fused;
    p.T = c.batch * c.seq_len;
    p.Lp = (int)rup(c.seq_len, 4);
    p.Vp = (int)rup(c.item_size, 4);
    p.dh = c.hidden / c.heads;
    // LayerNorm gamma/beta partials: one row per 64-token block, or one per sequence on the fused path
    p.nblk = p.fused ? c.batch : cdiv(p.T, 64);
    p.rows_pb = p.fused ? c.seq_len : 64;
    // split-K over tokens for the weight-gradient products: 32 / 40 slab slices (below), 32-aligned chunks (the direct kernel of
    // the fused shape cuts every slice into 4 more quarters inside a workgroup)
    // fused shape, C1 (12 weight-gradient units): 32 slices = 384 workgroups leave 128 of the kernel's 512 slots to the
    // embedding scatter blocks from the first cycle.  Re-measured with the per-workgroup record (tools/dw_stamps.py):
    // 40 slices (two workgroups on 224 of the 256 CUs, 10 whole k-blocks per wave) end the big workgroups 2 us sooner,
    // but the scatter blocks then start up to 17 us into the launch and the final reduction reads 8 more slabs:
    // 32 / 40 slices = 0.1533 / 0.1551 ms per step (three runs each, alternating), so 32 stays
    const int want_splits = c.splits > 0 ? c.splits : (p.fused ? 32 : 40);
    p.top_slabs = c.top_slabs > 0 ? c.top_slabs : 2;
    p.embed_in_block = !c.separate_embed || p.bf;     // bf16 storage: X[0] is written by the block kernel only
    p.direct_dw = !c.dw_tiled && (long)p.T * 4 * c.hidden * 4 < (1L << 31);      // its operands sit behind 32-bit buffer offsets
    p.scatter_in_block = p.fused && p.direct_dw && !c.separate_embed;
    // (bf16 storage: 64-aligned chunks -- a wave's quarter is then whole 16-row k-blocks of the bf16 matrix instruction)
    long ch = rup(cdiv(p.T, want_splits), p.bf ? 2 * GEMM_BK : GEMM_BK);
    if (ch < 64) ch = 64;
    if (ch > 2048) ch = 2048;
    p.kchunk = (int)ch;
    p.nsplit = cdiv(p.T, p.kchunk);
    // split-K over the catalogue for d(h_last) = dlogits . E
    long vc = rup(cdiv(p.Vp, p.fused ? 32 : 16), GEMM_BK);     // 32 catalogue slices for the direct kernel of the fused shape
    if (vc < 64) vc = 64;
    p.vchunk = (int)vc;
    p.vsplit = cdiv(p.Vp, p.vchunk);
    // sampled head: at most vsplit slabs, so the readers' slab count holds
    int chunk;
    if (c.train_negatives > 0) ssm_split(c.train_negatives, std::min(p.vsplit, SSM_SLAB_MAX), &p.ssm_nslab, &chunk);
}

static void carve(bsarec_plan& p, char* base, size_t* total) {
    const bsarec_config_t& c = p.cfg;
    const long T = p.T, d = c.hidden, B = c.batch, L = c.seq_len, h = c.heads, N = c.layers;
    const long Td = T * d;
    Carver cv(base);
    p.jobs = cv.take<ReduceJob>((size_t)(N * 20 + 3));
    p.jobs_pruned = cv.take<ReduceJob>((size_t)(N * 20 + 3));
    p.blockmap = cv.take<int>((size_t)(N * (12 * cdiv(d * d, 64) + 16 * cdiv(4 * d, 64) + cdiv((long)c.cutoff_bins * d * 2, 64)) +
                                       cdiv(L * d, 64) + 2 * cdiv(d, 64) + 64));
    p.ids32 = cv.take<int>(T);
    for (int l = 0; l <= N; ++l) p.X[l] = cv.take<float>(Td);
    p.xhat0 = cv.take<float>(Td); p.rstd0 = cv.take<float>(T);
    for (int l = 0; l < N; ++l) {
        LayerBufs& b = p.lb[l];
        b.dsp = cv.take<float>(Td); b.xhat_f = cv.take<float>(Td); b.rstd_f = cv.take<float>(T);
        b.q = cv.take<float>(Td); b.k = cv.take<float>(Td); b.v = cv.take<float>(Td);
        b.probs = cv.take<float>(B * h * L * p.Lp); b.ctx = cv.take<float>(Td);
        b.xhat_a = cv.take<float>(Td); b.rstd_a = cv.take<float>(T); b.hmix = cv.take<float>(Td);
        b.u = cv.take<float>(4 * Td); b.xhat_ff = cv.take<float>(Td); b.rstd_ff = cv.take<float>(T);
        b.gp = p.fused ? cv.take<float>(4 * Td) : nullptr;
    }
    p.logits = cv.take<float>(B * p.Vp); p.dlogits = cv.take<float>(B * p.Vp);
    p.loss_rows = cv.take<float>(B); p.loss = cv.take<float>(4);
    p.dXa = cv.take<float>(Td); p.dXb = cv.take<float>(Td); p.dz = cv.take<float>(Td); p.dT = cv.take<float>(Td);
    p.dU = cv.take<float>(4 * Td); p.dH = cv.take<float>(Td); p.dXacc = cv.take<float>(Td); p.dO = cv.take<float>(Td);
    p.dF = cv.take<float>(Td); p.dC = cv.take<float>(Td); p.dS = cv.take<float>(B * h * L * p.Lp);
    p.dq = cv.take<float>(Td); p.dk = cv.take<float>(Td); p.dv = cv.take<float>(Td); p.dXtmp = cv.take<float>(Td);
    p.dlast_slab = cv.take<float>((long)p.vsplit * B * d);
    for (int l = 0; l < N; ++l) {                                // per layer, so that ONE reduction launch ends the backward
        p.slab_wL[l] = cv.take<float>((long)p.nsplit * 12 * d * d);  // wq wk wv wo (d*d each) + w1 w2 (4 d*d each)
        p.slab_bL[l] = cv.take<float>((long)p.nsplit * 9 * d);       // bq bk bv bo (d) + b1 (4d) + b2 (d)
        p.part_lnL[l] = cv.take<float>((long)p.nblk * 6 * d);        // gamma/beta partials of the 3 LayerNorms
        p.part_betaL[l] = cv.take<float>(B * d);
    }
    p.part_ln0 = cv.take<float>((long)p.nblk * 2 * d);
    p.pos_slices = cdiv(B, 64);
    p.part_pos = cv.take<float>((long)p.pos_slices * L * d);
    p.trash = cv.take<float>(1024);
    p.lookup_acc = cv.take<unsigned long long>((long)c.item_size * d);
    p.part_kvb = cv.take<float>(2 * B * d);
    for (int l = 0; l < N; ++l) p.part_cwL[l] = c.filter_kind == 1 ? cv.take<float>(B * c.cutoff_bins * d * 2) : nullptr;
    // pruned top block: its last-row gradient operands and the rank-1 key / value operands live in their own compact
    // buffers ([B][d], [B][4d], [B*h][d]) so that they survive the next block's backward and ride in ITS weight-gradient launch
    p.top_dq = cv.take<float>(B * d); p.top_dO = cv.take<float>(B * d); p.top_dT = cv.take<float>(B * d);
    p.top_dU = cv.take<float>(4 * B * d);
    p.top_ak = cv.take<float>(B * h * d); p.top_rk = cv.take<float>(B * h * d);
    p.top_av = cv.take<float>(B * h * d); p.top_rv = cv.take<float>(B * h * d);
    p.slab_dummy = cv.take<float>((long)p.nsplit * 4 * d);
    if (c.train_negatives > 0) {                                 // (a zero tail carves exactly what it always did)
        const long Nn = c.train_negatives;
        p.ssm_cand = cv.take<int>(Nn); p.ssm_corr = cv.take<float>(Nn);
        p.ssm_logits = cv.take<float>(B * (Nn + 1)); p.ssm_dlogits = cv.take<float>(B * (Nn + 1));
    }
    if (c.train_lazy_adam) {                                     // (nothing without the flag)
        p.lazy.cap = (int)std::min<long>(c.item_size, T + B + c.train_negatives);
        p.lazy.d4 = (int)(d / 4);
        p.lazy.mark = cv.take<int>(c.item_size); p.lazy.rows = cv.take<int>(p.lazy.cap); p.lazy.count = cv.take<int>(1);
    }
    if (drop_bits_wanted(c))
        for (int l = 0; l < N; ++l) p.dbitsL[l] = cv.take<unsigned char>((size_t)drop_bits_layer_bytes(B, L, c.heads));
    // (no guard pad: the direct weight-gradient kernels prefetch past a slice without predicates, but through buffer
    // descriptors sized to their operand -- dw_direct.h)
    *total = cv.off;
}

extern "C" int bsarec_abi_version(void) { return BSAREC_ABI_VERSION; }

extern "C" size_t bsarec_workspace_bytes(const bsarec_config_t* cfg) {
    if (!cfg || check_cfg(*cfg) != 0) return 0;
    bsarec_plan p;
    p.cfg = *cfg;
    derive(p);
    size_t total = 0;
    carve(p, nullptr, &total);
    return total;
}

// slab sub-offsets (floats) inside a layer's slab_wL / slab_bL, per split-K slice
struct SlabMap { long wq, wk, wv, wo, w1, w2, wtot, bq, bk, bv, bo, b1, b2, btot; };
static SlabMap slab_map(long d) {
    SlabMap m;
    m.wq = 0; m.wk = d * d; m.wv = 2 * d * d; m.wo = 3 * d * d; m.w1 = 4 * d * d; m.w2 = 8 * d * d; m.wtot = 12 * d * d;
    m.bq = 0; m.bk = d; m.bv = 2 * d; m.bo = 3 * d; m.b1 = 4 * d; m.b2 = 8 * d; m.btot = 9 * d;
    return m;
}

// Split-K slabs are stored [tensor][split][elements] so that one reduce job reads a fixed stride.
static float* slab_w_ptr(const bsarec_plan& p, int l, long tensor_off) { return p.slab_wL[l] + tensor_off * p.nsplit; }
static float* slab_b_ptr(const bsarec_plan& p, int l, long tensor_off) { return p.slab_bL[l] + tensor_off * p.nsplit; }

// LayerNorm gamma / beta partials, planes of [nblk][d]: six per layer in part_lnL[l] (feed-forward, attention, filter), two of
// the embedding LayerNorm in part_ln0
enum LnPart { LN_FF_G, LN_FF_B, LN_A_G, LN_A_B, LN_F_G, LN_F_B };
enum Ln0Part { LN_E_G, LN_E_B };
static float* ln_part(const bsarec_plan& p, int l, LnPart k) { return p.part_lnL[l] + (long)k * p.nblk * p.cfg.hidden; }
static float* ln0_part(const bsarec_plan& p, Ln0Part k) { return p.part_ln0 + (long)k * p.nblk * p.cfg.hidden; }

// h_last: row L-1 of every sequence of the last layer's output [B][L][d], as a [B][d] matrix of row stride L d
static const float* h_last(const bsarec_plan& p) { return p.X[p.cfg.layers] + (long)(p.cfg.seq_len - 1) * p.cfg.hidden; }
static long h_last_stride(const bsarec_plan& p) { return (long)p.cfg.seq_len * p.cfg.hidden; }

// fragment image (wimage.h): one weight's F / T image of layer l, and a layer's Linear weights as their images
static float* wimage_weight(const bsarec_plan& p, int l, int which, bool transposed) {
    const long d = p.cfg.hidden;
    return p.wimg + l * wimage_layer_floats(d) + (transposed ? 12 * d * d : 0) + wimage_weight_off(which, d);
}
static bsarec_layer_t wimage_layer(const bsarec_plan& p, int l, bool transposed) {
    bsarec_layer_t w;
    memset(&w, 0, sizeof(w));
    w.query_w = wimage_weight(p, l, WIMAGE_WQ, transposed); w.key_w = wimage_weight(p, l, WIMAGE_WK, transposed);
    w.value_w = wimage_weight(p, l, WIMAGE_WV, transposed); w.dense_w = wimage_weight(p, l, WIMAGE_WO, transposed);
    w.ffn1_w = wimage_weight(p, l, WIMAGE_W1, transposed); w.ffn2_w = wimage_weight(p, l, WIMAGE_W2, transposed);
    return w;
}

extern "C" int bsarec_plan_create(bsarec_plan_t** out, const bsarec_config_t* cfg, const bsarec_tensors_t* params,
                                  const bsarec_tensors_t* grads, const bsarec_tensors_t* shadow, void* workspace,
                                  size_t workspace_bytes, void* state, const float* twiddle, void* stream) {
    if (!out || !cfg || !params || !workspace || !state || !twiddle) return -10;
    RET(check_cfg(*cfg));
    if (cfg->storage == 1 && fused_shape_ok(*cfg) && !shadow) return -15;     // (the generic path rounds its operands itself)
    if (wimage_wanted(*cfg) && (!shadow || !shadow->layer[0].query_w || ((uintptr_t)shadow->layer[0].query_w & 255))) return -15;
    if (((uintptr_t)workspace & 255) != 0) return -11;
    bsarec_plan* p = new bsarec_plan();
    p->cfg = *cfg;
    p->P = *params;
    if (grads) p->G = *grads; else memset(&p->G, 0, sizeof(p->G));
    if (shadow) p->S = *shadow; else memset(&p->S, 0, sizeof(p->S));
    p->ws = (char*)workspace; p->ws_bytes = workspace_bytes;
    p->state = (uint64_t*)state; p->twiddle = twiddle; p->train = false;
    p->wimg = wimage_wanted(*cfg) ? shadow->layer[0].query_w : nullptr;
    derive(*p);
    size_t total = 0;
    carve(*p, p->ws, &total);
    if (total > workspace_bytes) { delete p; return -12; }
    if (hipMemset(p->lookup_acc, 0, (size_t)cfg->item_size * cfg->hidden * sizeof(unsigned long long)) != hipSuccess) {
        delete p; return -12;
    }
    if (cfg->train_lazy_adam && (hipMemset(p->lazy.mark, 0, (size_t)cfg->item_size * sizeof(int)) != hipSuccess ||
                                 hipMemset(p->lazy.count, 0, sizeof(int)) != hipSuccess)) {
        delete p; return -12;
    }

    // reduction job table: per layer 19 jobs (state_dict order), then the 2 embedding LayerNorm jobs
    const long d = cfg->hidden;
    const SlabMap sm = slab_map(d);
    std::vector<ReduceJob> jobs;
    auto add = [&](const float* src, float* dst, int nsplit, long len) {
        ReduceJob j; j.src = src; j.dst = dst; j.nsplit = nsplit; j.len = (int)len; j.stride = len; j.scale = 1.f; j.pad = 0;
        jobs.push_back(j);
    };
    const int ns = p->nsplit, nb = p->nblk;
    auto add_w = [&](int l, int which, const float* src, float* dst) {       // a Linear weight: the job also names its image
        add(src, dst, ns, (which >= WIMAGE_W1 ? 4 : 1) * d * d);
        if (!p->wimg) return;
        ReduceJob& j = jobs.back();
        j.img_f = wimage_weight(*p, l, which, false); j.img_t = wimage_weight(*p, l, which, true);
        j.wn = (int)(which == WIMAGE_W1 ? 4 * d : d); j.wk = (int)(which == WIMAGE_W2 ? 4 * d : d);
    };
    for (int l = 0; l < cfg->layers; ++l) {
        const bsarec_layer_t& g = p->G.layer[l];
        add(p->part_betaL[l], g.sqrt_beta, cfg->batch, d);
        add(ln_part(*p, l, LN_F_G), g.filter_ln_w, nb, d);
        add(ln_part(*p, l, LN_F_B), g.filter_ln_b, nb, d);
        add_w(l, WIMAGE_WQ, slab_w_ptr(*p, l, sm.wq), g.query_w); add(slab_b_ptr(*p, l, sm.bq), g.query_b, ns, d);
        add_w(l, WIMAGE_WK, slab_w_ptr(*p, l, sm.wk), g.key_w);   add(slab_b_ptr(*p, l, sm.bk), g.key_b, ns, d);
        add_w(l, WIMAGE_WV, slab_w_ptr(*p, l, sm.wv), g.value_w); add(slab_b_ptr(*p, l, sm.bv), g.value_b, ns, d);
        add_w(l, WIMAGE_WO, slab_w_ptr(*p, l, sm.wo), g.dense_w); add(slab_b_ptr(*p, l, sm.bo), g.dense_b, ns, d);
        add(ln_part(*p, l, LN_A_G), g.attn_ln_w, nb, d);
        add(ln_part(*p, l, LN_A_B), g.attn_ln_b, nb, d);
        add_w(l, WIMAGE_W1, slab_w_ptr(*p, l, sm.w1), g.ffn1_w); add(slab_b_ptr(*p, l, sm.b1), g.ffn1_b, ns, 4 * d);
        add_w(l, WIMAGE_W2, slab_w_ptr(*p, l, sm.w2), g.ffn2_w); add(slab_b_ptr(*p, l, sm.b2), g.ffn2_b, ns, d);
        add(ln_part(*p, l, LN_FF_G), g.ffn_ln_w, nb, d);
        add(ln_part(*p, l, LN_FF_B), g.ffn_ln_b, nb, d);
    }
    add(ln0_part(*p, LN_E_G), p->G.ln_w, nb, d);
    add(ln0_part(*p, LN_E_B), p->G.ln_b, nb, d);
    if (p->scatter_in_block) {   // the position gradient = sum over the batch of the embedding gradient rows the block kernel wrote
        ReduceJob j; j.src = p->dz; j.dst = p->G.pos_emb; j.nsplit = cfg->batch; j.len = (int)((long)cfg->seq_len * d);
        j.stride = (long)cfg->seq_len * d; j.scale = 1.f; j.pad = 0;
        jobs.push_back(j);
    } else add(p->part_pos, p->G.pos_emb, p->pos_slices, (long)cfg->seq_len * d);
    if (cfg->filter_kind == 1)                 // FMLPRec: d(complex_weight) of every layer, summed over the sequences
        for (int l = 0; l < cfg->layers; ++l)
            add(p->part_cwL[l], p->G.layer[l].filter_cw, cfg->batch, (long)cfg->cutoff_bins * d * 2);
    p->jobs_per_layer = 19;
    p->prune_ok = p->fused && cfg->layers >= 2 && !cfg->no_prune_top && cfg->filter_kind == 0;      // (the FMLPRec block keeps its full kernels)
    p->pruned = false;
    p->loss_kind = 0; p->bce_pos = nullptr; p->bce_neg = nullptr;
    std::vector<ReduceJob> jobs_pr = jobs;          // key_b is job 6, value_b job 8 of a layer's 19 (state_dict order)
    {
        const size_t base = (size_t)(cfg->layers - 1) * 19;
        ReduceJob& jk = jobs_pr[base + 6]; jk.src = p->part_kvb; jk.nsplit = cfg->batch; jk.stride = d;
        ReduceJob& jv = jobs_pr[base + 8]; jv.src = p->part_kvb + (long)cfg->batch * d; jv.nsplit = cfg->batch; jv.stride = d;
        for (int j : {3, 4, 5, 7, 9, 10, 13, 14, 15, 16})      // weights and the other biases: the pruned products fill TOP_SLABS slabs
            jobs_pr[base + j].nsplit = std::min(p->top_slabs, ns);
    }
    std::vector<int> bmap;
    for (size_t j = 0; j < jobs.size(); ++j)
        for (int ch = 0; ch < cdiv(jobs[j].len, 64); ++ch) bmap.push_back((int)(j << 16) | ch);
    p->red_blocks = (int)bmap.size();
    p->red_elems = 0; p->red_lo = nullptr; p->red_hi = nullptr;
    for (const ReduceJob& j : jobs) {
        p->red_elems += j.len;
        if (!p->red_lo || j.dst < p->red_lo) p->red_lo = j.dst;
        if (!p->red_hi || j.dst + j.len > p->red_hi) p->red_hi = j.dst + j.len;
    }
    hipError_t e = hipMemcpyAsync(p->jobs, jobs.data(), jobs.size() * sizeof(ReduceJob), hipMemcpyHostToDevice,
                                  (hipStream_t)stream);
    if (e == hipSuccess) e = hipMemcpyAsync(p->blockmap, bmap.data(), bmap.size() * sizeof(int), hipMemcpyHostToDevice,
                                            (hipStream_t)stream);
    if (e == hipSuccess) e = hipMemcpyAsync(p->jobs_pruned, jobs_pr.data(), jobs_pr.size() * sizeof(ReduceJob),
                                            hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);   // jobs vector is host-temporary
    if (e != hipSuccess) { delete p; return (int)e; }
    // dry pass: sets every kernel's dynamic-LDS attribute for this shape without launching anything
    g_dry = true;
    int rc = 0;
    for (int last = 0; last < 2 && rc == 0; ++last) {
        rc = last ? bsarec_forward_last(p, reinterpret_cast<const int64_t*>(p->ws), 1, stream)
                  : bsarec_forward(p, reinterpret_cast<const int64_t*>(p->ws), 1, stream);
        if (rc == 0) rc = bsarec_loss(p, reinterpret_cast<const int64_t*>(p->ws), stream);
        if (rc == 0 && p->G.item_emb) rc = bsarec_backward(p, stream);
    }
    g_dry = false;
    p->pruned = false;
    p->train = false;
    if (rc != 0) { delete p; return rc; }
    *out = p;
    return 0;
}

extern "C" void bsarec_plan_destroy(bsarec_plan_t* plan) { delete plan; }

extern "C" long bsarec_buffer_offset(const bsarec_plan_t* p, int buffer, int layer) {
    if (!p) return -1;
    const int N = p->cfg.layers;
    const void* ptr = nullptr;
    if (buffer >= BSAREC_BUF_TRAIN_CAND && buffer <= BSAREC_BUF_TRAIN_DLOGITS && p->cfg.train_negatives == 0) return -1;
    switch (buffer) {
        case BSAREC_BUF_LAYER_OUT: if (layer < 0 || layer > N) return -1; ptr = p->X[layer]; break;
        case BSAREC_BUF_LOGITS: ptr = p->logits; break;
        case BSAREC_BUF_DLOGITS: ptr = p->dlogits; break;
        case BSAREC_BUF_LOSS: ptr = p->loss; break;
        case BSAREC_BUF_LOSS_ROWS: ptr = p->loss_rows; break;
        case BSAREC_BUF_DSP: if (layer < 0 || layer >= N) return -1; ptr = p->lb[layer].dsp; break;
        case BSAREC_BUF_HMIX: if (layer < 0 || layer >= N) return -1; ptr = p->lb[layer].hmix; break;
        case BSAREC_BUF_PROBS: if (layer < 0 || layer >= N) return -1; ptr = p->lb[layer].probs; break;
        case BSAREC_BUF_CTX: if (layer < 0 || layer >= N) return -1; ptr = p->lb[layer].ctx; break;
        case BSAREC_BUF_DLAYER_IN: if (layer < 0 || layer > N) return -1; ptr = (layer & 1) ? p->dXb : p->dXa; break;
        case BSAREC_BUF_TRAIN_CAND: ptr = p->ssm_cand; break;
        case BSAREC_BUF_TRAIN_CORR: ptr = p->ssm_corr; break;
        case BSAREC_BUF_TRAIN_LOGITS: ptr = p->ssm_logits; break;
        case BSAREC_BUF_TRAIN_DLOGITS: ptr = p->ssm_dlogits; break;
        case BSAREC_BUF_DROP_BITS: if (layer < 0 || layer >= N || !p->dbitsL[layer]) return -1; ptr = p->dbitsL[layer]; break;
        default: return -1;
    }
    return (long)((const char*)ptr - p->ws);
}

extern "C" int bsarec_plan_set_dense_grad_hook(bsarec_plan_t* p, bsarec_hook_t hook, void* user, float* lookup_grad) {
    if (!p) return -10;
    if (p->cfg.train_negatives > 0 && (hook || lookup_grad)) return -22;     // the sampled head has no dense part to exchange early
    p->dense_hook = hook; p->dense_hook_user = user; p->lookup_grad = lookup_grad;
    return 0;
}

extern "C" int bsarec_plan_set_drop_bits(bsarec_plan_t* p, int on) {
    if (!p || on < 0 || on > 1) return -10;
    p->drop_bits = on != 0;
    return 0;
}
extern "C" int bsarec_plan_set_bidirectional(bsarec_plan_t* p, int on) {
    if (!p || on < 0 || on > 1) return -10;
    p->bidir = on != 0;
    return 0;
}
extern "C" long bsarec_drop_bits_bytes(const bsarec_config_t* cfg) {
    if (!cfg || check_cfg(*cfg) != 0) return -1;
    return drop_bits_wanted(*cfg) ? drop_bits_layer_bytes(cfg->batch, cfg->seq_len, cfg->heads) : 0;
}
extern "C" long bsarec_drop_bits_hidden_bit(int slot, long tokens, long token, int column) {
    if (slot < 0 || slot >= DB_SLOTS || tokens < 1 || token < 0 || token >= tokens || column < 0 || column >= 64) return -1;
    return drop_bits_hidden_bit(slot, tokens, token, column);
}
extern "C" long bsarec_drop_bits_attn_bit(long tokens, int heads, long b, int head, int query, int key) {
    if (tokens < 1 || heads < 1 || b < 0 || head < 0 || head >= heads || query < 0 || query >= 64 || key < 0 || key >= 64) return -1;
    return drop_bits_attn_bit(tokens, heads, b, head, query, key);
}

extern "C" int bsarec_plan_set_train_sampler(bsarec_plan_t* p, const int64_t* pop_cum) {
    if (!p) return -10;
    if (p->cfg.train_negatives == 0 || p->cfg.train_sampler != 1) return -22;
    p->pop_cum = pop_cum;
    return 0;
}

// The sampled head's refusals, checked by every entry point that runs the loss before it launches anything.
static int sampled_refusal(const bsarec_plan& p) {
    if (p.cfg.train_negatives == 0) return 0;
    if (p.dense_hook || p.lookup_grad) return -22;
    if (p.cfg.train_sampler == 1 && !p.pop_cum && !g_dry) return -23;
    return 0;
}

// split-K slabs of d(h_last) the head's backward leaves for the top block
static int head_nsplit(const bsarec_plan& p) { return p.loss_kind == 1 ? 1 : (p.loss_kind == 2 ? p.ssm_nslab : p.vsplit); }

extern "C" int bsarec_plan_is_fused(const bsarec_plan_t* p) { return p && p->fused ? 1 : 0; }
extern "C" int bsarec_config_is_fused(const bsarec_config_t* cfg) {
    if (!cfg) return -10;
    RET(check_cfg(*cfg));
    return fused_shape_ok(*cfg) ? 1 : 0;
}

extern "C" int bsarec_buffer_is_bf16(const bsarec_plan_t* p, int buffer, int layer) {
    if (!p || !p->bf) return 0;
    switch (buffer) {
        case BSAREC_BUF_LAYER_OUT: return layer < p->cfg.layers ? 1 : 0;     // the last layer's output stays fp32
        case BSAREC_BUF_HMIX: case BSAREC_BUF_PROBS: case BSAREC_BUF_CTX: return 1;
        case BSAREC_BUF_DLAYER_IN: return 1;
        default: return 0;
    }
}

extern "C" int bsarec_wimage_refresh(bsarec_plan_t* p, void* stream) {
    if (!p) return -10;
    if (!p->wimg) return 0;
    WImageP W;
    memset(&W, 0, sizeof(W));
    for (int l = 0; l < p->cfg.layers; ++l) {
        const bsarec_layer_t& w = p->P.layer[l];
        const float* src[WIMAGE_NW] = {w.query_w, w.key_w, w.value_w, w.dense_w, w.ffn1_w, w.ffn2_w};
        for (int i = 0; i < WIMAGE_NW; ++i) W.w[l][i] = src[i];
    }
    W.img = p->wimg; W.d = p->cfg.hidden;
    LAUNCH(wimage_refresh_kernel, dim3(cdiv(12L * W.d * W.d, ROW_THREADS), p->cfg.layers), dim3(ROW_THREADS), 0, (hipStream_t)stream, W);
    return g_dry ? 0 : (int)hipGetLastError();
}

extern "C" long bsarec_wimage_floats(const bsarec_config_t* cfg) {
    if (!cfg || check_cfg(*cfg) != 0) return -10;
    return wimage_wanted(*cfg) ? cfg->layers * wimage_layer_floats(cfg->hidden) : 0;
}

extern "C" long bsarec_wimage_offset(int which, int transposed, int d, int n, int k) {
    if (which < 0 || which >= WIMAGE_NW || d < 32 || d % 32 || transposed < 0 || transposed > 1) return -1;
    const int wn = which == WIMAGE_W1 ? 4 * d : d, wk = which == WIMAGE_W2 ? 4 * d : d;
    if (n < 0 || n >= wn || k < 0 || k >= wk) return -1;
    return (transposed ? 12L * d * d : 0) + wimage_weight_off(which, d) + (transposed ? wimage_off(k, n, wn) : wimage_off(n, k, wk));
}

extern "C" int bsarec_shadow_refresh(bsarec_plan_t* p, void* stream) {
    if (!p) return -10;
    if (!p->bf) return 0;
    const long d = p->cfg.hidden;
    for (int l = 0; l < p->cfg.layers; ++l) {
        const bsarec_layer_t& w = p->P.layer[l];
        const bsarec_layer_t& sh = p->S.layer[l];
        CastJobs6 J;
        const float* src[6] = {w.query_w, w.key_w, w.value_w, w.dense_w, w.ffn1_w, w.ffn2_w};
        float* dst[6] = {sh.query_w, sh.key_w, sh.value_w, sh.dense_w, sh.ffn1_w, sh.ffn2_w};
        for (int i = 0; i < 6; ++i) { J.src[i] = src[i]; J.dst[i] = (unsigned short*)dst[i]; J.n4[i] = (i < 4 ? d * d : 4 * d * d) / 4; }
        hipLaunchKernelGGL(cast_bf16_kernel, dim3(cdiv(4 * d * d / 4, ROW_THREADS), 6), dim3(ROW_THREADS), 0, (hipStream_t)stream, J);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------
// helpers
// ---------------------------------------------------------------------------------------------
static uint32_t drop_thresh(float p) {
    double t = (double)p * 4294967296.0;
    if (t <= 0) return 0;
    if (t >= 4294967295.0) return 0xFFFFFFFFu;
    return (uint32_t)t;
}
static DropP make_drop(const bsarec_plan& p, float prob, int site, bool train) {
    DropP d;
    d.thresh = train ? drop_thresh(prob) : 0;
    d.scale = (train && prob > 0.f) ? (float)(1.0 / (1.0 - (double)prob)) : 1.0f;
    d.rng = p.state; d.site = (uint32_t)site;
    return d;
}
static int lpr_for(int d) { return d <= 64 ? 16 : (d <= 128 ? 32 : 64); }

#define DISPATCH_LPR(d, ...) \
    do { switch (lpr_for(d)) { case 16: { constexpr int LPR = 16; __VA_ARGS__; } break; \
                               case 32: { constexpr int LPR = 32; __VA_ARGS__; } break; \
                               default: { constexpr int LPR = 64; __VA_ARGS__; } break; } } while (0)

// tiles whose epilogue needs a whole row of width n (<= 256): pick BN
#define DISPATCH_BN(n, ...) \
    do { if ((n) <= 64) { constexpr int BN = 64; __VA_ARGS__; } \
         else if ((n) <= 128) { constexpr int BN = 128; __VA_ARGS__; } \
         else { constexpr int BN = 256; __VA_ARGS__; } } while (0)

static size_t freq_smem(int L, int d, int cb, int nsrc, int kc = FREQ_KC) {
    return (size_t)(rup(2 * L, 4) + (long)nsrc * cb * 2 * d + (long)nsrc * kc * 2048) * 4;
}
#define LDS_BYTES_MAX 163840     // LDS one workgroup can have on gfx950 (160 KiB per CU)

template <int LPR>
static int launch_freq_fwd(const float* X, const float* sb, const float* g, const float* be, float eps, DropP drop,
                           const float* tw, int B, int L, int d, int cb, float* dsp, float* xhat, float* rstd, hipStream_t s,
                           const float* cw = nullptr) {
    return launch_lds<freq_fwd_kernel<LPR>>(dim3(B), dim3(ROW_THREADS), freq_smem(L, d, cb, 1), s, X, sb, g, be, eps, drop, tw, L, d,
                                            cb, dsp, xhat, rstd, cw);
}

template <int LPR>
static int launch_freq_bwd(const float* X, const float* dF, const float* dXin, const float* sb, const float* tw, int B, int L,
                           int d, int cb, float* dX, float* pbeta, hipStream_t s, const float* cw = nullptr, float* pcw = nullptr) {
    // two spectra plus the four-bin exchange buffer outgrow the LDS once cutoff_bins * hidden > 6,144 - L / 2 (198,656 bytes at
    // check_cfg's limit, cutoff_bins * hidden = 8192 with L = 256): one bin per pass there, 149,504 bytes at that limit
    if (freq_smem(L, d, cb, 2) > LDS_BYTES_MAX)
        return launch_lds<freq_bwd_kernel<LPR, 1>>(dim3(B), dim3(ROW_THREADS), freq_smem(L, d, cb, 2, 1), s, X, dF, dXin, sb, tw, L, d, cb,
                                                   dX, pbeta, cw, pcw);
    return launch_lds<freq_bwd_kernel<LPR>>(dim3(B), dim3(ROW_THREADS), freq_smem(L, d, cb, 2), s, X, dF, dXin, sb, tw, L, d, cb, dX,
                                            pbeta, cw, pcw);
}

// Host-side check of everything a direct (buffer-descriptor) kernel is about to dereference.  These kernels prefetch
// without predicates and rely on the descriptor's range check; a descriptor whose BASE is null with a non-zero range
// reads virtual address 0 + offset -- a memory fault (which on this pool can reset the node), not a wrong number.
// Round 2 saw exactly such a fault ("address (nil)") from an experimental 8-wave variant of the logits backward whose
// source was not kept; whatever its cause was, a launch with a null or oversized operand is now refused here
// (return < 0, nothing enqueued) instead of being found by the GPU.
static bool dw_problem_ok(const DwProblem& q) {
    if (!q.A || !q.B || !q.slab) return false;
    if (q.K < 1 || q.M < 1 || q.N < 1 || q.kchunk < 8 || (q.kchunk & 7) || q.nslab < 1) return false;
    if (q.lda < q.M || q.ldb < q.N) return false;
    const long esz = q.bf16 ? 2 : 4;
    if (((long)(q.K - 1) * q.lda + q.M) * esz >= (1L << 31) || ((long)(q.K - 1) * q.ldb + q.N) * esz >= (1L << 31)) return false;
    return true;
}
static bool dh_problem_ok(const DhP& h) {
    if (!h.A || !h.E || !h.slab) return false;
    if (h.B < 1 || h.V < 1 || h.kchunk < 8 || (h.kchunk & 7) || h.nsplit < 1 || h.lda < h.V) return false;
    if ((long)h.B * h.lda * 4 >= (1L << 31) || (long)h.V * 256 >= (1L << 31)) return false;
    return true;
}

// head size (x storage x product mode) of the block kernels as the compile-time constants DH (, BF, X3)
#define DISPATCH_DH(dh, ...) \
    do { switch (dh) { case 16: { constexpr int DH = 16; __VA_ARGS__; } break; \
                       case 32: { constexpr int DH = 32; __VA_ARGS__; } break; \
                       default: { constexpr int DH = 64; __VA_ARGS__; } break; } } while (0)
#define DISPATCH_BLOCK(p, ...) \
    do { if ((p).bf) { constexpr bool BF = true, X3 = false; DISPATCH_DH((p).dh, __VA_ARGS__); } \
         else if ((p).cfg.x3_products) { constexpr bool BF = false, X3 = true; DISPATCH_DH((p).dh, __VA_ARGS__); } \
         else { constexpr bool BF = false, X3 = false; DISPATCH_DH((p).dh, __VA_ARGS__); } } while (0)

// What the parameter structs of the four block kernels (FusedFwdP, TopFwdP, FusedBwdP, TopBwdP: same field names) share:
// block l's weights (wm: where the Linear weights come from), saved activations, shape, dropout sites and stamp slot.
// Everything else is zero; `u` and whatever one kernel alone reads are the caller's to set.
template <bool FWD, class BlockP>
static void fill_block(const bsarec_plan& p, int l, bool tr, const bsarec_layer_t& wm, BlockP& F) {
    const bsarec_config_t& c = p.cfg;
    const bsarec_layer_t& w = p.P.layer[l];
    const LayerBufs& b = p.lb[l];
    memset(&F, 0, sizeof(F));
    F.X = p.X[l];
    F.sqrt_beta = w.sqrt_beta; F.f_g = w.filter_ln_w; F.wq = wm.query_w; F.wk = wm.key_w; F.wv = wm.value_w; F.wo = wm.dense_w;
    F.a_g = w.attn_ln_w; F.w1 = wm.ffn1_w; F.w2 = wm.ffn2_w; F.ff_g = w.ffn_ln_w; F.tw = p.twiddle;
    F.xhat_f = b.xhat_f; F.rstd_f = b.rstd_f; F.q = b.q; F.k = b.k; F.v = b.v; F.probs = b.probs;
    F.xhat_a = b.xhat_a; F.rstd_a = b.rstd_a; F.xhat_ff = b.xhat_ff; F.rstd_ff = b.rstd_ff;
    F.L = c.seq_len; F.Lp = p.Lp; F.cb = c.cutoff_bins; F.heads = c.heads;
    F.alpha = c.alpha; F.oma = (float)(1.0 - (double)c.alpha);
    F.drop_f = make_drop(p, c.p_hidden, 1 + 4 * l, tr); F.drop_p = make_drop(p, c.p_attn, 2 + 4 * l, tr);
    F.drop_o = make_drop(p, c.p_hidden, 3 + 4 * l, tr); F.drop_ff = make_drop(p, c.p_hidden, 4 + 4 * l, tr);
    F.stamps = p.stamps ? p.stamps + 32 * (2 * l + (FWD ? 0 : 1)) : nullptr;
    F.dbits = p.drop_bits ? p.dbitsL[l] : nullptr;             // (null where the plan carved none)
    if constexpr (FWD) {       // the forward alone: the output, the biases and LayerNorm betas, the activations it saves
        F.Xout = p.X[l + 1];
        F.f_b = w.filter_ln_b; F.bq = w.query_b; F.bk = w.key_b; F.bv = w.value_b; F.bo = w.dense_b; F.a_b = w.attn_ln_b;
        F.b1 = w.ffn1_b; F.b2 = w.ffn2_b; F.ff_b = w.ffn_ln_b;
        F.ids32 = p.ids32; F.ctx = b.ctx; F.hmix = b.hmix; F.u = b.u;
        F.eps = c.ln_eps;
    }
}

// the backward's LayerNorm / sqrt_beta partials of block l (FusedBwdP, TopBwdP)
template <class BlockP>
static void fill_block_partials(const bsarec_plan& p, int l, BlockP& F) {
    F.pg_ff = ln_part(p, l, LN_FF_G); F.pb_ff = ln_part(p, l, LN_FF_B); F.pg_a = ln_part(p, l, LN_A_G);
    F.pb_a = ln_part(p, l, LN_A_B); F.pg_f = ln_part(p, l, LN_F_G); F.pb_f = ln_part(p, l, LN_F_B);
    F.pbeta = p.part_betaL[l];
}

static void fill_top_fwd(bsarec_plan& p, int l, bool tr, TopFwdP& F) {
    fill_block<true>(p, l, tr, p.P.layer[l], F);
    F.low = p.lb[l].dsp;
    F.wk_sh = p.S.layer[l].key_w; F.wv_sh = p.S.layer[l].value_w;
}

static int launch_fused_fwd(bsarec_plan& p, int l, bool tr, hipStream_t s, const int64_t* ids = nullptr, const GatherP* gp = nullptr,
                            bool top_tail = false /* block l + 1 is the pruned top block: run it as this launch's tail */) {
    const bsarec_config_t& c = p.cfg;
    FusedFwdP F;
    // MFMA operands: bf16 shadow of the Linear weights (storage = 1), their fragment image (cfg.weight_image), or the masters
    fill_block<true>(p, l, tr, p.bf ? p.S.layer[l] : p.wimg ? wimage_layer(p, l, false) : p.P.layer[l], F);
    F.xout_f32 = (l == c.layers - 1);
    F.gp = p.lb[l].gp;
    F.dsp = nullptr;          // FrequencyLayer output stays in LDS on the fused path (BSAREC_BUF_DSP is generic-path only)
    if (l == 0 && gp) {       // the embedding front-end rides in the bottom block's phase 0
        F.e_E = p.P.item_emb; F.e_pos = p.P.pos_emb; F.e_g = p.P.ln_w; F.e_b = p.P.ln_b; F.e_ids = ids; F.e_gp = *gp;
        F.e_drop = make_drop(p, c.p_hidden, 0, tr); F.e_V = c.item_size;
        F.e_X0 = p.X[0]; F.e_xhat = p.xhat0; F.e_rstd = p.rstd0; F.e_ids32 = p.ids32;
    }
    F.trash = p.trash;
    F.q_or = p.bidir ? 255 : 0;            // L <= 64: query | 255 is behind every key
    TopFwdP TF;
    if (top_tail) {
        fill_top_fwd(p, l + 1, tr, TF);
        if (p.wimg) { TF.wk_sh = wimage_weight(p, l + 1, WIMAGE_WK, false); TF.wv_sh = wimage_weight(p, l + 1, WIMAGE_WV, false); }
    }
    const dim3 grid(c.batch), block(512);
    ProfScope prof(BSAREC_K_FUSED_FWD, s);
    if (c.filter_kind == 1) {        // FMLPRec block: whole-spectrum complex filter + feed-forward (no attention branch)
        F.filter_cw = p.P.layer[l].filter_cw;
        return launch_lds<fused_layer_fwd_kernel<32, false, NoTail, false, true>>(grid, block, fused_fwd_smem_bytes(), s, F, NoTail());
    }
    int rc = 0;
    if (!p.bf && c.chain_kernels && !c.x3_products) {
        // register-chain forward (fused_chain.h): one wave per 16-token tile, two workgroup barriers
        const size_t csm = fused_chain_fwd_smem_bytes(top_tail);
        DISPATCH_DH(p.dh, rc = top_tail ? launch_lds<fused_chain_fwd_kernel<DH, TopFwdP>>(grid, block, csm, s, F, TF)
                                        : launch_lds<fused_chain_fwd_kernel<DH, NoTail>>(grid, block, csm, s, F, NoTail()));
        return rc;
    }
    const size_t smem = fused_fwd_smem_bytes();
    if (p.wimg) {
        DISPATCH_DH(p.dh, rc = top_tail ? launch_lds<fused_layer_fwd_kernel<DH, false, TopFwdP, false, false, true>>(grid, block, smem, s, F, TF)
                                        : launch_lds<fused_layer_fwd_kernel<DH, false, NoTail, false, false, true>>(grid, block, smem, s, F, NoTail()));
        return rc;
    }
    DISPATCH_BLOCK(p, rc = top_tail ? launch_lds<fused_layer_fwd_kernel<DH, BF, TopFwdP, X3>>(grid, block, smem, s, F, TF)
                                    : launch_lds<fused_layer_fwd_kernel<DH, BF, NoTail, X3>>(grid, block, smem, s, F, NoTail()));
    return rc;
}

static int launch_fused_bwd(bsarec_plan& p, int l, bool tr, const float* dY, float* dXout, hipStream_t s, bool top,
                            const TopBwdP* head = nullptr /* the pruned top block's backward runs as this launch's head */) {
    const bsarec_config_t& c = p.cfg;
    FusedBwdP F;
    fill_block<false>(p, l, tr, p.bf ? p.S.layer[l] : p.wimg ? wimage_layer(p, l, true) : p.P.layer[l], F);
    fill_block_partials(p, l, F);
    F.dY = dY; F.dX = dXout;
    F.u = p.lb[l].gp;
    if (top) { F.dh_slabs = p.dlast_slab; F.dh_nsplit = head_nsplit(p); F.dh_stride = (long)c.batch * c.hidden; }
    if (l == 0) {       // the embedding front-end's backward (Drop + LayerNorm) rides in the bottom block's epilogue
        F.e_dz = p.dz; F.e_xhat = p.xhat0; F.e_rstd = p.rstd0; F.e_g = p.P.ln_w;
        F.e_pg = ln0_part(p, LN_E_G); F.e_pb = ln0_part(p, LN_E_B); F.e_drop = make_drop(p, c.p_hidden, 0, tr);
        F.e_dx_extra = p.ext_dy ? p.ext_mid[0] : nullptr;
    }
    F.dT = p.dT; F.dU = p.dU; F.dO = p.dO; F.dq = p.dq; F.dk = p.dk; F.dv = p.dv;
    F.trash = p.trash;
    const dim3 grid(c.batch), block(512);
    const size_t smem = fused_bwd_smem_bytes();
    ProfScope prof(BSAREC_K_FUSED_BWD, s);
    if (c.filter_kind == 1) {
        F.filter_cw = p.P.layer[l].filter_cw; F.pcw = p.part_cwL[l];
        return launch_lds<fused_layer_bwd_kernel<32, false, NoTail, false, true>>(grid, block, smem, s, F, NoTail());
    }
    int rc = 0;
    if (F.dbits) {      // the forward left keep bits (drop_bits.h): the instantiations without Philox; fp32 (image or masters) / bf16
        if (p.wimg)
            DISPATCH_DH(p.dh, rc = head ? launch_lds<fused_layer_bwd_kernel<DH, false, TopBwdP, false, false, true, true>>(grid, block, smem, s, F, *head)
                                        : launch_lds<fused_layer_bwd_kernel<DH, false, NoTail, false, false, true, true>>(grid, block, smem, s, F, NoTail()));
        else if (p.bf)
            DISPATCH_DH(p.dh, rc = head ? launch_lds<fused_layer_bwd_kernel<DH, true, TopBwdP, false, false, false, true>>(grid, block, smem, s, F, *head)
                                        : launch_lds<fused_layer_bwd_kernel<DH, true, NoTail, false, false, false, true>>(grid, block, smem, s, F, NoTail()));
        else
            DISPATCH_DH(p.dh, rc = head ? launch_lds<fused_layer_bwd_kernel<DH, false, TopBwdP, false, false, false, true>>(grid, block, smem, s, F, *head)
                                        : launch_lds<fused_layer_bwd_kernel<DH, false, NoTail, false, false, false, true>>(grid, block, smem, s, F, NoTail()));
        return rc;
    }
    if (p.wimg) {
        DISPATCH_DH(p.dh, rc = head ? launch_lds<fused_layer_bwd_kernel<DH, false, TopBwdP, false, false, true>>(grid, block, smem, s, F, *head)
                                    : launch_lds<fused_layer_bwd_kernel<DH, false, NoTail, false, false, true>>(grid, block, smem, s, F, NoTail()));
        return rc;
    }
    DISPATCH_BLOCK(p, rc = head ? launch_lds<fused_layer_bwd_kernel<DH, BF, TopBwdP, X3>>(grid, block, smem, s, F, *head)
                                : launch_lds<fused_layer_bwd_kernel<DH, BF, NoTail, X3>>(grid, block, smem, s, F, NoTail()));
    return rc;
}

static int launch_top_fwd(bsarec_plan& p, int l, bool tr, hipStream_t s) {
    TopFwdP F;
    fill_top_fwd(p, l, tr, F);
    int rc = 0;
    DISPATCH_BLOCK(p, rc = launch_lds<top_fwd_kernel<DH, BF>>(dim3(p.cfg.batch), dim3(256), top_fwd_smem_bytes(), s, F));
    return rc;
}

static void fill_top_bwd(bsarec_plan& p, int l, bool tr, float* dXout, TopBwdP& F) {
    const bsarec_config_t& c = p.cfg;
    fill_block<false>(p, l, tr, p.P.layer[l], F);
    fill_block_partials(p, l, F);
    F.dX = dXout;
    F.u = p.lb[l].u; F.low = p.lb[l].dsp;
    F.dh_slabs = p.dlast_slab; F.dh_nsplit = head_nsplit(p); F.dh_stride = (long)c.batch * c.hidden;
    F.dT = p.top_dT; F.dU = p.top_dU; F.dO = p.top_dO; F.dq = p.top_dq;
    F.ak = p.top_ak; F.rk = p.top_rk; F.av = p.top_av; F.rv = p.top_rv;
    F.pbk = p.part_kvb; F.pbv = p.part_kvb + (long)c.batch * c.hidden;
}

static int launch_top_bwd(bsarec_plan& p, int l, bool tr, float* dXout, hipStream_t s) {
    TopBwdP F;
    fill_top_bwd(p, l, tr, dXout, F);
    int rc = 0;
    if (F.dbits) {
        if (p.bf) DISPATCH_DH(p.dh, rc = launch_lds<top_bwd_kernel<DH, true, true>>(dim3(p.cfg.batch), dim3(256), top_bwd_smem_bytes(), s, F));
        else DISPATCH_DH(p.dh, rc = launch_lds<top_bwd_kernel<DH, false, true>>(dim3(p.cfg.batch), dim3(256), top_bwd_smem_bytes(), s, F));
        return rc;
    }
    DISPATCH_BLOCK(p, rc = launch_lds<top_bwd_kernel<DH, BF>>(dim3(p.cfg.batch), dim3(256), top_bwd_smem_bytes(), s, F));
    return rc;
}

extern "C" int bsarec_debug_stamps(bsarec_plan_t* p, void* dev_buf) { if (!p) return -10; p->stamps = (long long*)dev_buf; return 0; }

#ifdef BSAREC_DW_STAMPS
// diagnostic build only: the per-workgroup record of the last dw_direct_kernel launch (dw_direct.h), n rows of 8 words
extern "C" int bsarec_debug_dw_stamps(long long* host_out, int n) {
    if (!host_out || n < 1 || n > DW_STAMP_MAX) return -10;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_dw_stamps), (size_t)n * 8 * sizeof(long long)));
    return 0;
}
#endif

extern "C" int bsarec_step_begin(bsarec_plan_t* p, void* stream) {
    if (!p) return -10;
    LAUNCH(step_begin_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, p->state, (long long*)nullptr, 0);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------
static int forward_impl(bsarec_plan_t* p, const int64_t* ids, int train, void* stream, const GatherP& gp, bool last_only);

extern "C" int bsarec_forward(bsarec_plan_t* p, const int64_t* ids, int train, void* stream) {
    GatherP none;
    memset(&none, 0, sizeof(none));
    return forward_impl(p, ids, train, stream, none, false);
}

extern "C" int bsarec_forward_last(bsarec_plan_t* p, const int64_t* ids, int train, void* stream) {
    GatherP none;
    memset(&none, 0, sizeof(none));
    return forward_impl(p, ids, train, stream, none, true);
}

// Block l on the generic path: FrequencyLayer, attention and feed-forward as tiled GEMMs with fused epilogues
static int generic_layer_fwd(bsarec_plan& p, int l, bool tr, hipStream_t s) {
    const bsarec_config_t& c = p.cfg;
    const int T = p.T, d = c.hidden, L = c.seq_len, B = c.batch, h = c.heads, dh = p.dh, Lp = p.Lp;
    const bsarec_layer_t& w = p.P.layer[l];
    LayerBufs& b = p.lb[l];
    const float* X = p.X[l];
    const XformP nox = no_xform();
    // K2 FrequencyLayer
    DISPATCH_LPR(d, RET(launch_freq_fwd<LPR>(X, w.sqrt_beta, w.filter_ln_w, w.filter_ln_b, c.ln_eps,
                                             make_drop(p, c.p_hidden, 1 + 4 * l, tr), p.twiddle, B, L, d,
                                             c.cutoff_bins, b.dsp, b.xhat_f, b.rstd_f, s,
                                             c.filter_kind == 1 ? w.filter_cw : nullptr)));
    // K3 Q, K, V projections (one launch, 3 problems)
    {
        GemmP g = gemm_defaults(T, d, d);
        g.nprob = 3; g.lda = d; g.ldb = d;
        g.A[0] = g.A[1] = g.A[2] = X;
        g.B[0] = w.query_w; g.B[1] = w.key_w; g.B[2] = w.value_w;
        auto e = epi_linear<true, false, false>(b.q, d);
        e.C[1] = b.k; e.C[2] = b.v;
        e.bias[0] = w.query_b; e.bias[1] = w.key_b; e.bias[2] = w.value_b;
        RET((launch_gemm<64, 64, 2, 2, false, false, XF_NONE, XF_NONE, false>(g, nox, e, nullptr, 1, s, BSAREC_K_QKV)));
    }
    // K4a scores + mask + softmax -> probs
    {
        GemmP g = gemm_defaults(L, Lp, dh);
        g.Nb = L; g.lda = d; g.ldb = d; g.nh = h;
        g.A[0] = b.q; g.B[0] = b.k;
        g.a_sb = (long)L * d; g.a_sh = dh; g.b_sb = (long)L * d; g.b_sh = dh;
        EpiSoftmax e; e.ids = p.ids32; e.L = L; e.Lp = Lp; e.sqrt_dh = sqrtf((float)dh); e.P = b.probs; e.bidir = p.bidir;
        DISPATCH_BN(Lp, RET((launch_gemm<64, BN, 2, 2, false, false, XF_NONE, XF_NONE, false>(g, nox, e, nullptr, B * h, s))));
    }
    // K4b context = Drop(probs) . V
    {
        GemmP g = gemm_defaults(L, dh, Lp);
        g.Kv = L; g.lda = Lp; g.ldb = d; g.nh = h;
        g.A[0] = b.probs; g.B[0] = b.v;
        g.a_sb = (long)h * L * Lp; g.a_sh = (long)L * Lp; g.b_sb = (long)L * d; g.b_sh = dh;
        XformP xf = nox; xf.drop = make_drop(p, c.p_attn, 2 + 4 * l, tr); xf.L = L; xf.Lp = Lp;
        auto e = epi_linear<false, false, false>(b.ctx, d);
        e.c_sb = (long)L * d; e.c_sh = dh;
        RET((launch_gemm<64, 64, 2, 2, false, true, XF_DROP, XF_NONE, false>(g, xf, e, nullptr, B * h, s)));
    }
    // K5 dense + dropout + residual + LayerNorm + alpha mix
    {
        GemmP g = gemm_defaults(T, d, d);
        g.lda = d; g.ldb = d; g.A[0] = b.ctx; g.B[0] = w.dense_w;
        EpiLN<true> e;
        e.bias = w.dense_b; e.R = X; e.drop = make_drop(p, c.p_hidden, 3 + 4 * l, tr);
        e.gamma = w.attn_ln_w; e.beta = w.attn_ln_b; e.eps = c.ln_eps;
        e.Y = b.hmix; e.xhat = b.xhat_a; e.rstd = b.rstd_a;
        e.dsp = b.dsp; e.alpha = c.alpha; e.oma = (float)(1.0 - (double)c.alpha);
        DISPATCH_BN(d, RET((launch_gemm<64, BN, 2, 2, false, false, XF_NONE, XF_NONE, false>(g, nox, e, nullptr, 1, s))));
    }
    // K6a dense_1
    {
        GemmP g = gemm_defaults(T, 4 * d, d);
        g.lda = d; g.ldb = d; g.A[0] = b.hmix; g.B[0] = w.ffn1_w;
        auto e = epi_linear<true, false, false>(b.u, 4 * d);
        e.bias[0] = w.ffn1_b;
        RET((launch_gemm<64, 64, 2, 2, false, false, XF_NONE, XF_NONE, false>(g, nox, e, nullptr, 1, s, BSAREC_K_FFN1)));
    }
    // K6b gelu + dense_2 + dropout + residual + LayerNorm
    {
        GemmP g = gemm_defaults(T, d, 4 * d);
        g.lda = 4 * d; g.ldb = 4 * d; g.A[0] = b.u; g.B[0] = w.ffn2_w;
        EpiLN<false> e;
        e.bias = w.ffn2_b; e.R = b.hmix; e.drop = make_drop(p, c.p_hidden, 4 + 4 * l, tr);
        e.gamma = w.ffn_ln_w; e.beta = w.ffn_ln_b; e.eps = c.ln_eps;
        e.Y = p.X[l + 1]; e.xhat = b.xhat_ff; e.rstd = b.rstd_ff;
        e.dsp = nullptr; e.alpha = 0.f; e.oma = 1.f;
        XformP xa = nox; xa.act = c.hidden_act;
        DISPATCH_BN(d, RET((launch_gemm<64, BN, 2, 2, false, false, XF_GELU, XF_NONE, false>(g, xa, e, nullptr, 1, s, BSAREC_K_FFN2))));
    }
    return 0;
}

static int forward_impl(bsarec_plan_t* p, const int64_t* ids, int train, void* stream, const GatherP& gp, bool last_only) {
    if (!p || (!ids && !gp.table)) return -10;
    PlanScope scope(p);
    hipStream_t s = (hipStream_t)stream;
    const bsarec_config_t& c = p->cfg;
    const int T = p->T, d = c.hidden, L = c.seq_len;
    const bool tr = train != 0;
    p->train = tr;
    p->pruned = last_only && p->prune_ok;

    const bool embed_in_block = p->fused && p->embed_in_block;
    if (!embed_in_block)
    DISPATCH_LPR(d, {
        constexpr int RPB = ROW_THREADS / LPR;
        LAUNCH(embed_fwd_kernel<LPR>, dim3(cdiv(T, RPB)), dim3(ROW_THREADS), 0, s, ids, gp, p->P.item_emb,
                           p->P.pos_emb, p->P.ln_w, p->P.ln_b, c.ln_eps, make_drop(*p, c.p_hidden, 0, tr), T, L, d,
                           c.item_size, p->X[0], p->xhat0, p->rstd0, p->ids32);
        HIPCHK(hipGetLastError());
    });

    const bool tail = p->pruned && c.layers >= 2 && !c.separate_top;     // top block = tail of the launch below it
    for (int l = 0; l < c.layers; ++l) {
        if (!p->fused) RET(generic_layer_fwd(*p, l, tr, s));
        else if (p->pruned && l == c.layers - 1) { if (!tail) RET(launch_top_fwd(*p, l, tr, s)); }
        else RET(launch_fused_fwd(*p, l, tr, s, ids, (l == 0 && embed_in_block) ? &gp : nullptr, tail && l == c.layers - 2));
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------
// logits / loss
// ---------------------------------------------------------------------------------------------
extern "C" int bsarec_logits(bsarec_plan_t* p, void* stream) {
    if (!p) return -10;
    PlanScope scope(p);
    hipStream_t s = (hipStream_t)stream;
    const bsarec_config_t& c = p->cfg;
    const int d = c.hidden;
    // hidden = 64 and a small problem: straight from global memory into the MFMA operands (dw_direct.h).  Measured on one box:
    // C1 (B = 256, V = 3,417) 0.1569 -> 0.1551 ms/step; at B = 256 x V = 12,102 and 1,024 x 20,034 the direct form LOSES (every
    // 32-row block re-reads the whole table, 4-byte stores: 0.134 -> 0.140 and 0.661 -> 0.687 ms) -- those keep the tiled GEMM
    if (p->fused && d == 64 && p->Vp <= 4096 && c.batch <= 512 && !g_dry) {
        LogitsP G;
        G.H = h_last(*p); G.ldh = h_last_stride(*p); G.E = p->P.item_emb; G.C = p->logits;
        G.B = c.batch; G.V = c.item_size; G.Vp = p->Vp;
        const long units = (long)cdiv(c.batch, 32) * cdiv(p->Vp, 32);
        ProfScope prof(BSAREC_K_LOGITS, s);
        hipLaunchKernelGGL(logits_direct_kernel, dim3((unsigned)cdiv(units, 4)), dim3(256), 0, s, G);
        return (int)hipGetLastError();
    }
    GemmP g = gemm_defaults(c.batch, p->Vp, d);
    g.Nb = c.item_size; g.lda = h_last_stride(*p); g.ldb = d;
    g.A[0] = h_last(*p); g.B[0] = p->P.item_emb;
    auto e = epi_linear<false, false, false>(p->logits, p->Vp);
    return launch_gemm<64, 64, 2, 2, false, false, XF_NONE, XF_NONE, false>(g, no_xform(), e, nullptr, 1, s, BSAREC_K_LOGITS, true);
}

// The head's parameters (sampled_softmax.h): B of the Bg rows of the global batch against the item rows E, d(h_last) in at
// most slab_cap slabs.  The output buffers, the gradient sink and the stream state are the caller's to add.
static SsmP ssm_params(const float* h, long ldh, int B, int Bg, const float* E, const int64_t* answers, const int* cand,
                       const float* corr, int N, long V, const int64_t* pop_cum, int logq, int d, int slab_cap) {
    SsmP P;
    memset(&P, 0, sizeof(P));
    P.H = h; P.ldh = ldh; P.E = E; P.answers = answers; P.pop_cum = pop_cum;
    P.B = B; P.V = (int)V; P.d = d; P.N = N; P.logq = logq ? 1 : 0; P.inv_b = 1.0f / (float)Bg;
    P.cand = const_cast<int*>(cand); P.corr = const_cast<float*>(corr);
    ssm_split(N, slab_cap, &P.nslab, &P.chunk);
    const int dt = cdiv(d, SSM_TILE);
    P.tilesA = cdiv(N, SSM_TILE) * dt;
    P.tilesB = P.nslab * cdiv(B, SSM_TILE) * dt;
    return P;
}

static SsmP plan_ssm_params(const bsarec_plan& p, const int64_t* answers) {
    const bsarec_config_t& c = p.cfg;
    SsmP P = ssm_params(h_last(p), h_last_stride(p), c.batch, c.batch, p.P.item_emb, answers, p.ssm_cand, p.ssm_corr,
                        c.train_negatives, c.item_size, c.train_sampler == 1 ? p.pop_cum : nullptr, !c.train_no_logq, c.hidden,
                        std::min(p.vsplit, SSM_SLAB_MAX));
    P.state = p.state; P.logits = p.ssm_logits; P.dlogits = p.ssm_dlogits; P.loss_rows = p.loss_rows;
    P.slab = p.dlast_slab; P.acc = p.lookup_acc;
    if (p.lazy_now) {                          // lazy Adam step: reset the row count in the loss, mark T in the backward
        P.lazy = p.lazy; P.ids32 = p.ids32; P.nids = p.T;
        P.tilesM = (int)std::min<long>(cdiv((long)p.T + c.batch + c.train_negatives, ROW_THREADS), 64);
    }
    return P;
}

static int loss_impl(bsarec_plan_t* p, const int64_t* answers, void* stream, bool with_mean) {
    if (!p || !answers) return -10;
    hipStream_t s = (hipStream_t)stream;
    if (p->cfg.train_negatives > 0) {          // sampled softmax (sampled_softmax.h): draws + logits, then the rows' CE
        RET(sampled_refusal(*p));
        p->loss_kind = 2; p->ssm_answers = answers;
        const SsmP P = plan_ssm_params(*p, answers);
        LAUNCH(ssm_logits_kernel<false>, dim3(cdiv(P.N, SSM_TILE), cdiv(P.B, SSM_TILE)), dim3(ROW_THREADS), 0, s, P);
        HIPCHK(hipGetLastError());
        LAUNCH(ssm_ce_kernel<false>, dim3(P.B), dim3(ROW_THREADS), 0, s, P);
        HIPCHK(hipGetLastError());
        if (with_mean) LAUNCH(loss_mean_kernel, dim3(1), dim3(ROW_THREADS), 0, s, p->loss_rows, P.B, p->loss);
        return (int)hipGetLastError();
    }
    RET(bsarec_logits(p, stream));
    p->loss_kind = 0;
    const bsarec_config_t& c = p->cfg;
    // up to 4,096 classes: scalar row in registers (C1); up to 24,576: float4 row in registers (C2's Beauty, C4's Yelp catalogue);
    // beyond: streamed in three passes (C5: 40 MB rows)
    const int V = c.item_size;
    const float inv_b = 1.0f / (float)c.batch;
#define CE_VEC(N4) LAUNCH(ce_rows_vec_kernel<N4>, dim3(c.batch), dim3(ROW_THREADS), 0, s, p->logits, answers, V, p->Vp, inv_b, p->dlogits, p->loss_rows)
    if (V <= CE_MAX_PER_THREAD * ROW_THREADS || V > 24 * 4 * ROW_THREADS)
        LAUNCH(ce_rows_kernel, dim3(c.batch), dim3(ROW_THREADS), 0, s, p->logits, answers, V, p->Vp, inv_b, p->dlogits, p->loss_rows);
    else if (V <= 8 * 4 * ROW_THREADS) CE_VEC(8);
    else if (V <= 12 * 4 * ROW_THREADS) CE_VEC(12);
    else if (V <= 16 * 4 * ROW_THREADS) CE_VEC(16);
    else if (V <= 20 * 4 * ROW_THREADS) CE_VEC(20);
    else CE_VEC(24);
#undef CE_VEC
    HIPCHK(hipGetLastError());
    if (with_mean) LAUNCH(loss_mean_kernel, dim3(1), dim3(ROW_THREADS), 0, s, p->loss_rows, c.batch, p->loss);
    return (int)hipGetLastError();
}

extern "C" int bsarec_loss(bsarec_plan_t* p, const int64_t* answers, void* stream) { return loss_impl(p, answers, stream, true); }

static int loss_pair(bsarec_plan_t* p, const int64_t* pos_ids, const int64_t* neg_ids, void* stream, int logsig);

// SASRec's head (sibling model on the same encoder; run the plan with alpha = 0): src/model/sasrec.py:41-63
extern "C" int bsarec_loss_bce(bsarec_plan_t* p, const int64_t* pos_ids, const int64_t* neg_ids, void* stream) {
    return loss_pair(p, pos_ids, neg_ids, stream, 0);
}
// FMLPRec's head: src/model/fmlprec.py:41-62
extern "C" int bsarec_loss_logsig(bsarec_plan_t* p, const int64_t* pos_ids, const int64_t* neg_ids, void* stream) {
    return loss_pair(p, pos_ids, neg_ids, stream, 1);
}

static int loss_pair(bsarec_plan_t* p, const int64_t* pos_ids, const int64_t* neg_ids, void* stream, int logsig) {
    if (!p || !pos_ids || !neg_ids) return -10;
    hipStream_t s = (hipStream_t)stream;
    const bsarec_config_t& c = p->cfg;
    p->loss_kind = 1; p->bce_pos = pos_ids; p->bce_neg = neg_ids;
    LAUNCH(bce_rows_kernel, dim3(1), dim3(ROW_THREADS), 0, s, h_last(*p), h_last_stride(*p), p->P.item_emb,
           pos_ids, neg_ids, c.batch, c.hidden, c.item_size, p->dlogits, p->loss, logsig);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------------------
static int backward_impl(bsarec_plan_t* p, void* stream, const TickP& tick, const bsarec_adam_t* fuse_adam = nullptr);

extern "C" int bsarec_backward(bsarec_plan_t* p, void* stream) {
    TickP none;
    memset(&none, 0, sizeof(none));
    return backward_impl(p, stream, none);
}

extern "C" int bsarec_backward_seq(bsarec_plan_t* p, const float* d_out, void* stream) {
    if (!p || !d_out) return -10;
    if (p->pruned) return -13;                 // the forward kept only the last row of the top block: run bsarec_forward
    if (p->cfg.train_negatives > 0) return -22;     // a plan with the sampled head runs that head's backward only
    TickP none;
    memset(&none, 0, sizeof(none));
    p->ext_dy = d_out;
    const int rc = backward_impl(p, stream, none);
    p->ext_dy = nullptr;
    return rc;
}

extern "C" int bsarec_backward_seq_multi(bsarec_plan_t* p, const float* const* d_outs, void* stream) {
    if (!p || !d_outs) return -10;
    const int N = p->cfg.layers;
    if (!d_outs[N]) return -10;                // the last layer's gradient is always given (zeros if the caller has none)
    if (p->pruned) return -13;                 // the forward kept only the last row of the top block: run bsarec_forward
    for (int l = 0; l < N; ++l) p->ext_mid[l] = d_outs[l];
    const int rc = bsarec_backward_seq(p, d_outs[N], stream);
    for (int l = 0; l < N; ++l) p->ext_mid[l] = nullptr;
    return rc;
}

// Can the final gradient reduction and Adam be one launch (reduce_adam_kernel)?  Needs the direct weight-gradient
// launch of block 0 to host the step tick, plain single-GPU gradient sources, and every gradient tensor inside the flat
// arena the update walks (item table + the reduction jobs' targets = the whole arena).
static bool can_fuse_adam(const bsarec_plan& p, const bsarec_adam_t& a) {
    if (!p.fused || !p.direct_dw || p.loss_kind == 1) return false;
    if (a.grads2 || a.n_grad_srcs > 0 || a.grad_scale != 1.0f) return false;
    if (!p.G.item_emb || p.G.item_emb < a.grads) return false;
    const long item = (long)p.cfg.item_size * p.cfg.hidden;
    const long off = p.G.item_emb - a.grads;
    if (off < 0 || off + item > a.n || (off & 3) || (item & 3)) return false;
    return p.red_elems + item == a.n && p.red_lo >= a.grads && p.red_hi <= a.grads + a.n;
}

// The head's backward, by the head of the last loss call: the dense part of the item table's gradient into G.item_emb (or the
// candidate rows into lookup_acc) and the head_nsplit(p) split-K slabs of d(h_last) into dlast_slab.  With an external
// upstream gradient there is no head: the item table gets its lookup rows only.
static int head_bwd(bsarec_plan& p, hipStream_t s) {
    const bsarec_config_t& c = p.cfg;
    const int d = c.hidden, B = c.batch;
    const float* hlast = h_last(p);
    const long ldh = h_last_stride(p);
    const XformP nox = no_xform();
    const bool direct_logits = p.fused && p.direct_dw && p.loss_kind == 0 && (long)B * p.Vp * 4 < (1L << 30) &&
                               (long)c.item_size * d * 4 < (1L << 31);
    if (p.ext_dy) {             // backward of forward(): no head on this path, the item table gets its lookup rows only
        if (!g_dry) HIPCHK(hipMemsetAsync(p.G.item_emb, 0, (size_t)c.item_size * d * sizeof(float), s));
    } else if (p.loss_kind == 1) {     // SASRec's BCE pair: two embedding rows per sequence instead of the dense logits path
        if (!g_dry) HIPCHK(hipMemsetAsync(p.G.item_emb, 0, (size_t)c.item_size * d * sizeof(float), s));
        LAUNCH(bce_bwd_kernel, dim3(B), dim3(64), 0, s, hlast, ldh, p.P.item_emb, p.bce_pos, p.bce_neg, p.dlogits, B, d,
               c.item_size, p.dlast_slab, p.G.item_emb);
        HIPCHK(hipGetLastError());
    } else if (p.loss_kind == 2) {
        // sampled softmax: candidate and answer rows of dE into the fixed-point accumulator (the item table's dense part is
        // zero: the final reduction writes the accumulator over it), and the slabs of d(h_last)
        const SsmP P = plan_ssm_params(p, p.ssm_answers);
        const int tilesC = std::max(1, std::min(cdiv((long)B * d, ROW_THREADS), 64));
        LAUNCH(ssm_bwd_kernel<false>, dim3(P.tilesA + P.tilesB + tilesC + P.tilesM), dim3(ROW_THREADS), 0, s, P);
        HIPCHK(hipGetLastError());
    } else if (direct_logits) {
        // fused shape: dE = dlogits^T . h_last (K = B rows, written straight into the gradient buffer) and the split-K
        // slabs of d(h_last) = dlogits . E by the direct kernels (dw_direct.h), one launch
        DwProblem q;
        memset(&q, 0, sizeof(q));
        q.A = p.dlogits; q.B = hlast; q.lda = p.Vp; q.ldb = ldh; q.M = c.item_size; q.N = d; q.K = B;
        q.kchunk = (int)rup(B, 32); q.nslab = 1; q.slab = p.G.item_emb; q.bslab = nullptr; q.gelu = 0;
        DhP H;
        memset(&H, 0, sizeof(H));
        H.A = p.dlogits; H.lda = p.Vp; H.E = p.P.item_emb; H.B = B; H.V = c.item_size; H.kchunk = p.vchunk;
        H.nsplit = p.vsplit; H.slab = p.dlast_slab;
        const int tiles = cdiv(c.item_size, 64);
        if (!dw_problem_ok(q) || !dh_problem_ok(H)) return -21;
        const dim3 lb_grid(tiles + cdiv(cdiv(B, 32) * p.vsplit, 4));
        if (p.bf) LAUNCH(logits_bwd_direct_kernel<true>, lb_grid, dim3(256), 0, s, q, tiles, H);
        else LAUNCH(logits_bwd_direct_kernel<false>, lb_grid, dim3(256), 0, s, q, tiles, H);
        HIPCHK(hipGetLastError());
    } else {
        // dE (dense, logits path) = dlogits^T . h_last  [V, d] (overwrites the gradient buffer) and the split-K slabs of
        // d(h_last) = dlogits . E -- one launch
        PairP G;
        memset(&G, 0, sizeof(G));
        G.A = gemm_defaults(c.item_size, d, B);
        G.A.lda = p.Vp; G.A.ldb = ldh; G.A.A[0] = p.dlogits; G.A.B[0] = hlast;
        G.EA = epi_linear<false, false, false>(p.G.item_emb, d);
        G.B = gemm_defaults(B, d, p.Vp);
        G.B.Kv = c.item_size; G.B.lda = p.Vp; G.B.ldb = d; G.B.A[0] = p.dlogits; G.B.B[0] = p.P.item_emb;
        G.B.nsplit = p.vsplit; G.B.kchunk = p.vchunk;
        G.EB = epi_linear<false, false, false>(p.dlast_slab, d);
        G.EB.c_split = (long)B * d;
        G.tilesA = cdiv(c.item_size, 64) * cdiv(d, 64);
        G.tilesB_m = cdiv(B, 64);
        if (d <= 64) {
            constexpr size_t smem = GemmSmem<64, 64, true, true>::BYTES > GemmSmem<64, 64, false, true>::BYTES
                                        ? GemmSmem<64, 64, true, true>::BYTES : GemmSmem<64, 64, false, true>::BYTES;
            LAUNCH(gemm_logits_bwd_kernel, dim3(G.tilesA + G.tilesB_m * p.vsplit), dim3(GEMM_THREADS), smem, s, G);
            HIPCHK(hipGetLastError());
        } else {                                   // wider hidden sizes: two plain launches (N needs several tiles)
            RET((launch_gemm<64, 64, 2, 2, true, true, XF_NONE, XF_NONE, false>(G.A, nox, G.EA, nullptr, 1, s, BSAREC_K_NONE, true)));
            RET((launch_gemm<64, 64, 2, 2, false, true, XF_NONE, XF_NONE, false>(G.B, nox, G.EB, nullptr, 1, s, BSAREC_K_NONE, true)));
        }
    }
    return 0;
}

// The upstream gradient of the top layer's output, in or instead of the loop's first buffer dY: the caller's tensor
// (bsarec_backward_seq), or on the generic path h_last's gradient summed from the head's slabs into row L-1 of zeros.
static int top_grad(bsarec_plan& p, float*& dY, hipStream_t s) {
    const bsarec_config_t& c = p.cfg;
    const int T = p.T, d = c.hidden;
    if (p.ext_dy) {
        if (p.bf) {      // the block kernels read inter-block gradients as bf16: convert the caller's fp32 tensor once
            CastJobs6 J;
            memset(&J, 0, sizeof(J));
            J.src[0] = p.ext_dy; J.dst[0] = (unsigned short*)dY; J.n4[0] = (long)T * d / 4;
            LAUNCH(cast_bf16_kernel, dim3(cdiv((long)T * d / 4, ROW_THREADS), 1), dim3(ROW_THREADS), 0, s, J);
            HIPCHK(hipGetLastError());
        } else dY = const_cast<float*>(p.ext_dy);
    } else if (!p.fused) {      // the fused top-layer backward synthesises this gradient from the slabs itself
        LAUNCH(dlast_kernel, dim3(cdiv((long)T * d / 4, ROW_THREADS)), dim3(ROW_THREADS), 0, s, p.dlast_slab,
               head_nsplit(p), (long)c.batch * d, T, c.seq_len, d, dY);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

// Block l's backward on the generic path up to dXtmp: feed-forward, the two LayerNorms of the mix, attention.  Leaves the
// weight-gradient operands (dT, dU, dO, dq, dk, dv) and dF / dXtmp for the FrequencyLayer backward that completes dX.
static int generic_layer_bwd(bsarec_plan& p, int l, const float* dY, hipStream_t s) {
    const bsarec_config_t& c = p.cfg;
    const int T = p.T, d = c.hidden, L = c.seq_len, B = c.batch, h = c.heads, dh = p.dh, Lp = p.Lp, nb = p.nblk;
    const bool tr = p.train;
    const bsarec_layer_t& w = p.P.layer[l];
    const LayerBufs& b = p.lb[l];
    const XformP nox = no_xform();
    // ---- FeedForward backward
    {
        LnBranch a; memset(&a, 0, sizeof(a));
        a.xhat = b.xhat_ff; a.rstd = b.rstd_ff; a.gamma = w.ffn_ln_w; a.in_scale = 1.f;
        a.drop = make_drop(p, c.p_hidden, 4 + 4 * l, tr); a.dT = p.dT;
        a.pgamma = ln_part(p, l, LN_FF_G); a.pbeta = ln_part(p, l, LN_FF_B);
        DISPATCH_LPR(d, LAUNCH((ln_bwd_kernel<LPR, 0>), dim3(nb), dim3(ROW_THREADS), 0, s, dY, a, a, p.dz, T, d, p.rows_pb));
        HIPCHK(hipGetLastError());
    }
    {   // dU = (dT2 . W2) * gelu'(U)
        GemmP g = gemm_defaults(T, 4 * d, d);
        g.lda = d; g.ldb = 4 * d; g.A[0] = p.dT; g.B[0] = w.ffn2_w;
        auto e = epi_linear<false, false, true>(p.dU, 4 * d);
        e.U = b.u; e.ldu = 4 * d; e.act = c.hidden_act;
        RET((launch_gemm<64, 64, 2, 2, false, true, XF_NONE, XF_NONE, false>(g, nox, e, nullptr, 1, s, BSAREC_K_DU)));
    }
    {   // dH = dU . W1 + dz
        GemmP g = gemm_defaults(T, d, 4 * d);
        g.lda = 4 * d; g.ldb = d; g.A[0] = p.dU; g.B[0] = w.ffn1_w;
        auto e = epi_linear<false, true, false>(p.dH, d);
        e.R = p.dz; e.ldr = d;
        RET((launch_gemm<64, 64, 2, 2, false, true, XF_NONE, XF_NONE, false>(g, nox, e, nullptr, 1, s)));
    }
    // ---- mix + the two LayerNorms (attention branch scaled by 1-alpha, filter branch by alpha)
    {
        LnBranch a; memset(&a, 0, sizeof(a));
        a.xhat = b.xhat_a; a.rstd = b.rstd_a; a.gamma = w.attn_ln_w; a.in_scale = (float)(1.0 - (double)c.alpha);
        a.drop = make_drop(p, c.p_hidden, 3 + 4 * l, tr); a.dT = p.dO;
        a.pgamma = ln_part(p, l, LN_A_G); a.pbeta = ln_part(p, l, LN_A_B);
        LnBranch f; memset(&f, 0, sizeof(f));
        f.xhat = b.xhat_f; f.rstd = b.rstd_f; f.gamma = w.filter_ln_w; f.in_scale = c.alpha;
        f.drop = make_drop(p, c.p_hidden, 1 + 4 * l, tr); f.dT = p.dF;
        f.pgamma = ln_part(p, l, LN_F_G); f.pbeta = ln_part(p, l, LN_F_B);
        DISPATCH_LPR(d, LAUNCH((ln_bwd_kernel<LPR, 1>), dim3(nb), dim3(ROW_THREADS), 0, s, p.dH, a, f, p.dXacc, T, d, p.rows_pb));
        HIPCHK(hipGetLastError());
    }
    // ---- attention backward
    {   // dC = dO . Wo
        GemmP g = gemm_defaults(T, d, d);
        g.lda = d; g.ldb = d; g.A[0] = p.dO; g.B[0] = w.dense_w;
        auto e = epi_linear<false, false, false>(p.dC, d);
        RET((launch_gemm<64, 64, 2, 2, false, true, XF_NONE, XF_NONE, false>(g, nox, e, nullptr, 1, s)));
    }
    XformP xfa = nox; xfa.drop = make_drop(p, c.p_attn, 2 + 4 * l, tr); xfa.L = L; xfa.Lp = Lp;
    {   // dS = P * (dA - rowsum(dA P)) / sqrt(dh),  dA = (dC . V^T) * keep/(1-p)
        GemmP g = gemm_defaults(L, Lp, dh);
        g.Nb = L; g.lda = d; g.ldb = d; g.nh = h; g.A[0] = p.dC; g.B[0] = b.v;
        g.a_sb = (long)L * d; g.a_sh = dh; g.b_sb = (long)L * d; g.b_sh = dh;
        EpiDS e; e.P = b.probs; e.drop = xfa.drop; e.L = L; e.Lp = Lp; e.sqrt_dh = sqrtf((float)dh); e.dS = p.dS;
        DISPATCH_BN(Lp, RET((launch_gemm<64, BN, 2, 2, false, false, XF_NONE, XF_NONE, false>(g, nox, e, nullptr, B * h, s))));
    }
    {   // dV = Drop(P)^T . dC
        GemmP g = gemm_defaults(L, dh, L);
        g.lda = Lp; g.ldb = d; g.nh = h; g.A[0] = b.probs; g.B[0] = p.dC;
        g.a_sb = (long)h * L * Lp; g.a_sh = (long)L * Lp; g.b_sb = (long)L * d; g.b_sh = dh;
        auto e = epi_linear<false, false, false>(p.dv, d);
        e.c_sb = (long)L * d; e.c_sh = dh;
        RET((launch_gemm<64, 64, 2, 2, true, true, XF_DROP, XF_NONE, false>(g, xfa, e, nullptr, B * h, s)));
    }
    {   // dK = dS^T . Q
        GemmP g = gemm_defaults(L, dh, L);
        g.lda = Lp; g.ldb = d; g.nh = h; g.A[0] = p.dS; g.B[0] = b.q;
        g.a_sb = (long)h * L * Lp; g.a_sh = (long)L * Lp; g.b_sb = (long)L * d; g.b_sh = dh;
        auto e = epi_linear<false, false, false>(p.dk, d);
        e.c_sb = (long)L * d; e.c_sh = dh;
        RET((launch_gemm<64, 64, 2, 2, true, true, XF_NONE, XF_NONE, false>(g, nox, e, nullptr, B * h, s)));
    }
    {   // dQ = dS . K
        GemmP g = gemm_defaults(L, dh, Lp);
        g.Kv = L; g.lda = Lp; g.ldb = d; g.nh = h; g.A[0] = p.dS; g.B[0] = b.k;
        g.a_sb = (long)h * L * Lp; g.a_sh = (long)L * Lp; g.b_sb = (long)L * d; g.b_sh = dh;
        auto e = epi_linear<false, false, false>(p.dq, d);
        e.c_sb = (long)L * d; e.c_sh = dh;
        RET((launch_gemm<64, 64, 2, 2, false, true, XF_NONE, XF_NONE, false>(g, nox, e, nullptr, B * h, s)));
    }
    {   // dXtmp = dQ.Wq + dK.Wk + dV.Wv + (dzA + dzF)
        GemmP g = gemm_defaults(T, d, d);
        g.lda = d; g.ldb = d; g.nseg = 3;
        g.A[0] = p.dq; g.A[1] = p.dk; g.A[2] = p.dv;
        g.B[0] = w.query_w; g.B[1] = w.key_w; g.B[2] = w.value_w;
        auto e = epi_linear<false, true, false>(p.dXtmp, d);
        e.R = p.dXacc; e.ldr = d;
        RET((launch_gemm<64, 64, 2, 2, false, true, XF_NONE, XF_NONE, false>(g, nox, e, nullptr, 1, s)));
    }
    return 0;
}

// tile size of the grouped tiled kernel (the direct kernel has its own units): 128 for bf16 products at hidden >= 128 (C3:
// 405 -> 337 us per launch); the fp32 form needs 296 registers at 128 x 128 = one wave per SIMD and loses (765 -> 987 us)
static int dw_tile(const bsarec_plan& p) { return (p.bf_products && p.cfg.hidden >= 128) ? 128 : 64; }

// The six weight-gradient problems (and bias gradients) of block l as split-K products into the layer's slabs
static void build_dw_problems(const bsarec_plan& p, int l, bool top_pruned, GroupedTN& G) {
    const bsarec_config_t& c = p.cfg;
    const int T = p.T, d = c.hidden, L = c.seq_len, B = c.batch, h = c.heads, N = c.layers, ns = p.nsplit;
    const SlabMap sm = slab_map(d);
    const LayerBufs& b = p.lb[l];
    const float* X = p.X[l];
    memset(&G, 0, sizeof(G));
    struct Spec { const float* A; long lda; const float* B; long ldb; int M, N; long woff, boff; int gelu; };
    const Spec sp[6] = {
        {p.dq, d, X, d, d, d, sm.wq, sm.bq, 0},        {p.dk, d, X, d, d, d, sm.wk, sm.bk, 0},
        {p.dv, d, X, d, d, d, sm.wv, sm.bv, 0},        {p.dO, d, b.ctx, d, d, d, sm.wo, sm.bo, 0},
        {p.dU, 4 * d, b.hmix, d, 4 * d, d, sm.w1, sm.b1, 0},
        // dW2 = dT2^T . act(u): the full fused forward already saved gelu(u) in `u`; elsewhere apply it while loading
        {p.dT, d, b.u, 4 * d, d, 4 * d, sm.w2, sm.b2, (p.fused && !top_pruned) ? 0 : 1}};
    int tiles = 0;
    const int gts = dw_tile(p);
    // Top block: only position L-1 of each sequence carries an upstream gradient (bsarec.py:32), so dq, dO, dU
    // and dT2 are zero on every other row: their four products reduce over the B last positions only
    // (row stride L*ld), exactly; dk and dv still reduce over all tokens.
    const bool top = (l == N - 1) && !p.ext_dy;       // (an external upstream gradient has every row)
    for (int i = 0; i < 6; ++i) {
        const bool last_only = top && i != 1 && i != 2;
        GemmP g = gemm_defaults(sp[i].M, sp[i].N, last_only ? B : T);
        g.lda = sp[i].lda; g.ldb = sp[i].ldb; g.A[0] = sp[i].A; g.B[0] = sp[i].B; g.nsplit = ns; g.kchunk = p.kchunk;
        if (last_only) {
            // row L-1 of every sequence (element offsets: the operands are bf16 tensors under storage = 1)
            const long esz = p.bf ? 2 : 4;
            g.A[0] = (const float*)((const char*)g.A[0] + (long)(L - 1) * sp[i].lda * esz);
            g.B[0] = (const float*)((const char*)g.B[0] + (long)(L - 1) * sp[i].ldb * esz);
            g.lda *= L; g.ldb *= L;
            g.kchunk = (int)rup(cdiv(B, ns), GEMM_BK);           // slices beyond ceil(B / kchunk) write zero slabs
            if (top_pruned) {                                    // gradient rows come compact ([B][M]) from top_bwd_kernel
                g.A[0] = i == 0 ? p.top_dq : i == 3 ? p.top_dO : i == 4 ? p.top_dU : p.top_dT;
                g.lda = sp[i].M;
                g.nsplit = std::min(p.top_slabs, ns); g.kchunk = (int)rup(cdiv(B, g.nsplit), GEMM_BK);
            }
        }
        // pruned top block: dK, dV are rank-1 per (sequence, head) -> dWk = AK^T RK, dWv = AV^T RV over B*h rows
        // (fused_top.h); their bias gradients come from per-sequence partials, the slab output is discarded
        const bool compact = top_pruned && (i == 1 || i == 2);
        if (compact) {
            g = gemm_defaults(d, d, B * h);
            g.A[0] = i == 1 ? p.top_ak : p.top_av; g.B[0] = i == 1 ? p.top_rk : p.top_rv; g.lda = d; g.ldb = d;
            g.nsplit = std::min(p.top_slabs, ns); g.kchunk = (int)rup(cdiv(B * h, g.nsplit), GEMM_BK);
        }
        G.P[i] = g;
        G.E[i] = epi_linear<false, false, false>(slab_w_ptr(p, l, sp[i].woff), sp[i].N);
        G.E[i].c_split = (long)sp[i].M * sp[i].N;
        G.bgrad[i] = compact ? p.slab_dummy : slab_b_ptr(p, l, sp[i].boff);
        G.tile0[i] = tiles;
        G.tiles_n[i] = cdiv(sp[i].N, gts);
        G.b_gelu[i] = sp[i].gelu;
        tiles += cdiv(sp[i].M, gts) * G.tiles_n[i];
    }
    G.tile0[6] = tiles; G.nprob = 6; G.act = c.hidden_act;
}

// What the layer loop carries from the pruned top block to the block below it on the direct path: the top block's six
// (tiny) weight-gradient problems wait in DW (np problems, nu units so far) and its backward in top_head; both ride in the
// launches of the block below.
struct DwPending { DwP DW; int np, nu; TopBwdP top_head; bool have_head; };

// Direct launch of block l's problems (and of those waiting in Q).  tick: the step tick to run in this launch (null: none).
static int launch_dw_direct(bsarec_plan& p, int l, bool top_pruned, const GroupedTN& G, DwPending& Q, const TickP* tick,
                            hipStream_t s) {
    const int T = p.T, ns = p.nsplit;
    // hidden = 64: direct split-K products, one workgroup per (problem, 64x64 tile, slab slice) -- dw_direct.h.
    // The pruned top block's six (tiny) problems are not launched on their own: they wait in DW and ride in
    // the next block's launch.
    for (int i = 0; i < 6; ++i) {
        const GemmP& g = G.P[i];
        DwProblem& q = Q.DW.P[Q.np];
        q.A = g.A[0]; q.B = g.B[0]; q.lda = g.lda; q.ldb = g.ldb; q.M = g.M; q.N = g.N; q.K = g.K;
        q.kchunk = g.kchunk; q.nslab = g.nsplit; q.slab = G.E[i].C[0]; q.bslab = G.bgrad[i]; q.gelu = G.b_gelu[i];
        q.bf16 = p.bf ? 1 : 0;
        for (int m0 = 0; m0 < q.M; m0 += 64)
            for (int n0 = 0; n0 < q.N; n0 += 64) Q.DW.U[Q.nu++] = DwUnit{(short)Q.np, (short)m0, (short)n0, 0};
        ++Q.np;
    }
    if (top_pruned) { Q.DW.nsmall = Q.nu; Q.DW.small_slabs = std::min(p.top_slabs, ns); }
    else {
        Q.DW.nunits = Q.nu; Q.DW.nslab = ns;
        TickP tk_here;                     // the step tick rides in block 0's launch when Adam is fused into the reduction
        memset(&tk_here, 0, sizeof(tk_here));
        if (tick) tk_here = *tick;
        ScatterP sc;                       // ... and so does the embedding-gradient scatter (block 0's launch: dz is complete)
        memset(&sc, 0, sizeof(sc));
        if (p.scatter_in_block && l == 0) {
            sc.de = p.dz; sc.ids32 = p.ids32; sc.T = T; sc.dA = p.lookup_acc;
            sc.nblocks = cdiv(T, SCATTER_FLOATS / 64);
        }
        for (int i = 0; i < Q.np; ++i) if (!dw_problem_ok(Q.DW.P[i])) return -21;
        if (sc.nblocks && (!sc.de || !sc.ids32 || !sc.dA)) return -21;
        ProfScope prof(BSAREC_K_DW1, s);
        const dim3 dw_grid(8 * cdiv(ns, 8) * (Q.nu - Q.DW.nsmall) + Q.DW.nsmall * Q.DW.small_slabs + sc.nblocks + (tk_here.state ? 1 : 0));
        LAUNCH(dw_direct_kernel, dw_grid, dim3(256), 0, s, Q.DW, tk_here, sc);
        HIPCHK(hipGetLastError());
        Q.np = 0; Q.nu = 0; Q.DW.nsmall = 0; Q.DW.small_slabs = 0;
    }
    return 0;
}

// Grouped tiled launch of block l's problems
static int launch_dw_grouped(const bsarec_plan& p, const GroupedTN& G, hipStream_t s) {
    ProfScope prof(BSAREC_K_DW1, s);
    const dim3 grid(G.tile0[6], p.nsplit), block(GEMM_THREADS);
    if (!p.bf_products)
        return launch_lds<gemm_grouped_tn_kernel<false, 64>>(grid, block, GemmSmem<64, 64, true, true, false>::BYTES, s, G);
    if (dw_tile(p) == 128)
        return launch_lds<gemm_grouped_tn_kernel<true, 128>>(grid, block, GemmSmem<128, 128, true, true, true>::BYTES, s, G);
    return launch_lds<gemm_grouped_tn_kernel<true, 64>>(grid, block, GemmSmem<64, 64, true, true, true>::BYTES, s, G);
}

// Embedding front-end backward: LayerNorm + dropout into dz (fused path: done by the bottom block's backward kernel), then the
// scatter of dz's rows into lookup_acc and the position partials (unless that rode in block 0's weight-gradient launch)
static int embed_bwd(bsarec_plan& p, const float* dY, hipStream_t s) {
    const bsarec_config_t& c = p.cfg;
    const int T = p.T, d = c.hidden, L = c.seq_len, B = c.batch;
    if (!p.fused) {
        LnBranch a; memset(&a, 0, sizeof(a));
        a.xhat = p.xhat0; a.rstd = p.rstd0; a.gamma = p.P.ln_w; a.in_scale = 1.f;
        a.drop = make_drop(p, c.p_hidden, 0, p.train); a.dT = nullptr;
        a.pgamma = ln0_part(p, LN_E_G); a.pbeta = ln0_part(p, LN_E_B);
        DISPATCH_LPR(d, LAUNCH((ln_bwd_kernel<LPR, 2>), dim3(p.nblk), dim3(ROW_THREADS), 0, s, dY, a, a, p.dz, T, d, p.rows_pb));
        HIPCHK(hipGetLastError());
    }
    if (!p.scatter_in_block)
    DISPATCH_LPR(d, {
        constexpr int CHUNK = SCATTER_FLOATS / (LPR * 4);
        const int sb = cdiv(T, CHUNK);
        RET(launch_lds<embed_bwd_kernel<LPR>>(dim3(sb + L * p.pos_slices), dim3(ROW_THREADS), fix_scatter_lds_bytes(LPR), s,
                                              p.dz, p.ids32, B, L, d, p.lookup_acc, p.part_pos, sb));
    });
    return 0;
}

// Does this Adam update the plan's own masters (same arena layout as its gradients)?  Only then do the masters change
// under the plan's fragment image.
static bool adam_on_masters(const bsarec_plan& p, const bsarec_adam_t& a) {
    return p.G.item_emb && a.params + (p.G.item_emb - a.grads) == p.P.item_emb;
}
// after an Adam launch that does not write the image itself (adam_kernel, lazy_adam_kernel): rebuild it, one small launch
static int wimage_after_adam(bsarec_plan& p, const bsarec_adam_t& a, hipStream_t s) {
    return (p.wimg && !a.wimage_plan && adam_on_masters(p, a)) ? bsarec_wimage_refresh(&p, s) : 0;
}

// ONE deterministic second-stage reduction for every split-K slab and LayerNorm / beta partial (no empty blocks: flat block
// map); its extra last block closes the optimisation step when asked to (the lookup-path sum of the item-table gradient
// joins its target here: after every scatter block has finished).  fuse_adam: the same launch also runs Adam over the arena.
static int final_reduce(bsarec_plan& p, const TickP& tick, const bsarec_adam_t* fuse_adam, hipStream_t s) {
    const bsarec_config_t& c = p.cfg;
    LookupAcc la;
    memset(&la, 0, sizeof(la));
    la.acc = p.lookup_acc; la.dst = p.lookup_grad ? p.lookup_grad : p.G.item_emb; la.n4 = (long)c.item_size * c.hidden / 4;
    la.nblocks = (int)std::min<long>(cdiv(la.n4, ROW_THREADS), 1024);
    la.dense_zero = (!p.ext_dy && p.loss_kind == 2) ? 1 : 0;
    const bool lazy = p.lazy_now && !p.ext_dy && p.loss_kind == 2;
    if (lazy) {                        // lazy Adam: the rows of T only, in a grid sized to the list's capacity
        la.lazy = p.lazy;
        la.nblocks = (int)std::min<long>(cdiv((long)p.lazy.cap * p.lazy.d4, ROW_THREADS), 1024);
    }
    const ReduceJob* jobs = p.pruned ? p.jobs_pruned : p.jobs;
    if (fuse_adam) {
        const bsarec_adam_t& a = *fuse_adam;
        AdamFuseP A;
        memset(&A, 0, sizeof(A));
        A.w = a.params; A.g = const_cast<float*>(a.grads); A.m = a.exp_avg; A.v = a.exp_avg_sq;
        A.b1 = a.beta1; A.b2 = a.beta2; A.eps = a.eps; A.wd = a.weight_decay;
        A.shadow = (unsigned short*)a.shadow_bf16; A.shadow_from = a.shadow_bf16 ? a.shadow_from : a.n;
        A.item_off = p.G.item_emb - a.grads; A.item_n4 = la.n4; A.lookup_acc = la.acc;
        A.dense_zero = la.dense_zero;
        A.wimage = (p.wimg && adam_on_masters(p, a)) ? 1 : 0;
        if (lazy) A.lazy = p.lazy;
        int ab = lazy ? la.nblocks : cdiv(A.item_n4, ROW_THREADS);
        if (ab > 1024) ab = 1024;
        LAUNCH(reduce_adam_kernel, dim3(p.red_blocks + ab), dim3(ROW_THREADS), 0, s, jobs, p.blockmap, p.red_blocks,
               (const uint64_t*)p.state, A);
    } else
        LAUNCH(multi_reduce_flat_kernel, dim3(p.red_blocks + la.nblocks + (tick.state ? 1 : 0)), dim3(ROW_THREADS), 0, s, jobs,
               p.blockmap, p.red_blocks, tick, la);
    return (int)hipGetLastError();
}

static int backward_impl(bsarec_plan_t* p, void* stream, const TickP& tick, const bsarec_adam_t* fuse_adam) {
    if (!p) return -10;
    if (!p->G.item_emb) return -13;
    // fused Adam reads the item table's gradient from the arena, where the lookup sum must land: refuse before anything is
    // launched (an early return after the scatter would leave its sums in lookup_acc for the next step)
    if (fuse_adam && p->lookup_grad) return -21;
    PlanScope scope(p);
    hipStream_t s = (hipStream_t)stream;
    const bsarec_config_t& c = p->cfg;
    const int T = p->T, d = c.hidden, L = c.seq_len, B = c.batch, N = c.layers;
    const bool tr = p->train;

    RET(head_bwd(*p, s));
    // the dense item-table gradient is complete (enqueued): a data-parallel host may start exchanging it now
    if (p->dense_hook && !g_dry && !p->ext_dy) p->dense_hook(p->dense_hook_user, stream);
    float* dY = (N & 1) ? p->dXb : p->dXa;       // gradient w.r.t. X[l+1]; ping-pong so that dX[0] lands in dXa
    RET(top_grad(*p, dY, s));

    DwPending pend;
    memset(&pend, 0, sizeof(pend));
    for (int l = N - 1; l >= 0; --l) {
        float* dXout = (dY == p->dXa) ? p->dXb : p->dXa;
        const bool top_pruned = p->fused && p->pruned && l == N - 1;
        if (top_pruned) {
            // rides in the next launch -- when this layer's weight-gradient products do too (the direct kernel defers them; the
            // tiled fallback launches them inside this iteration and needs the top block's operands now)
            if (N >= 2 && !c.separate_top && p->direct_dw) { fill_top_bwd(*p, l, tr, dXout, pend.top_head); pend.have_head = true; }
            else RET(launch_top_bwd(*p, l, tr, dXout, s));
        } else if (p->fused) {
            RET(launch_fused_bwd(*p, l, tr, dY, dXout, s, l == N - 1 && !p->ext_dy,
                                 (pend.have_head && l == N - 2) ? &pend.top_head : nullptr));
        } else RET(generic_layer_bwd(*p, l, dY, s));
        // all six weight gradients + bias gradients of the block: one split-K launch (the step tick rides in block 0's direct
        // launch when Adam is fused into the reduction)
        GroupedTN G;
        build_dw_problems(*p, l, top_pruned, G);
        if (p->fused && p->direct_dw) RET(launch_dw_direct(*p, l, top_pruned, G, pend, (fuse_adam && l == 0) ? &tick : nullptr, s));
        else RET(launch_dw_grouped(*p, G, s));
        // ---- FrequencyLayer backward: completes dX of this layer
        if (!p->fused) {
            const bsarec_layer_t& w = p->P.layer[l];
            DISPATCH_LPR(d, RET(launch_freq_bwd<LPR>(p->X[l], p->dF, p->dXtmp, w.sqrt_beta, p->twiddle, B, L, d, c.cutoff_bins,
                                                     dXout, p->part_betaL[l], s, c.filter_kind == 1 ? w.filter_cw : nullptr,
                                                     c.filter_kind == 1 ? p->part_cwL[l] : nullptr)));
        }
        dY = dXout;
        // forward(all_sequence_output=True): layer output l may carry an upstream gradient of its own -- it joins the gradient
        // coming down from the blocks above (the fused bottom block adds output 0's inside its epilogue: its dX never
        // reaches memory)
        if (p->ext_dy && p->ext_mid[l] && !(p->fused && l == 0)) {
            const long n4 = (long)T * d / 4;
            LAUNCH(grad_join_kernel, dim3((unsigned)std::min<long>(cdiv(n4, ROW_THREADS), 2048)), dim3(ROW_THREADS), 0, s, dXout,
                   p->ext_mid[l], n4, p->bf ? 1 : 0);
            HIPCHK(hipGetLastError());
        }
    }
    RET(embed_bwd(*p, dY, s));
    return final_reduce(*p, tick, fuse_adam, s);
}

// ---------------------------------------------------------------------------------------------
// Adam / fused step
// ---------------------------------------------------------------------------------------------
static TickP make_tick(void* state, int adam, float lr, float b1, float b2, const float* loss_rows, int B, float* loss_out,
                       void* cursor, int advance, int bump_step) {
    TickP t;
    memset(&t, 0, sizeof(t));
    t.state = (uint64_t*)state; t.adam = adam; t.lr = lr; t.b1 = b1; t.b2 = b2;
    t.loss_rows = loss_rows; t.B = B; t.loss_out = loss_out;
    t.cursor = (long long*)cursor; t.advance = advance; t.bump_step = bump_step;
    return t;
}

static int adam_check(const bsarec_adam_t* a) {
    if (!a || !a->params || !a->grads || !a->exp_avg || !a->exp_avg_sq || a->n <= 0 || (a->n & 3)) return -10;
    if (a->shadow_bf16 && (a->shadow_from < 0 || (a->shadow_from & 3))) return -10;
    if (a->grads2 && (a->grads2_n < 0 || a->grads2_n > a->n || (a->grads2_n & 3))) return -10;
    if (a->n_grad_srcs < 0 || a->n_grad_srcs > 8) return -10;
    for (int r = 0; r < a->n_grad_srcs; ++r) if (!a->grad_srcs[r]) return -10;
    return 0;
}

static int adam_launch(const bsarec_adam_t& a, void* state, hipStream_t s) {
    const long n4 = a.n / 4;
    int blocks = cdiv(n4, ROW_THREADS);
    if (blocks > 2048) blocks = 2048;
    GradSrcs S;
    memset(&S, 0, sizeof(S));
    S.nsrc = a.n_grad_srcs;
    for (int r = 0; r < a.n_grad_srcs; ++r) S.src[r] = a.grad_srcs[r];
    S.g2 = a.grads2; S.n2_4 = a.grads2 ? a.grads2_n / 4 : 0;
    LAUNCH(adam_kernel, dim3(blocks), dim3(ROW_THREADS), 0, s, a.params, a.grads, a.exp_avg, a.exp_avg_sq, n4,
           (const uint64_t*)state, a.beta1, a.beta2, a.eps, a.weight_decay, a.grad_scale, (unsigned short*)a.shadow_bf16,
           a.shadow_bf16 ? a.shadow_from / 4 : n4, S);
    HIPCHK(hipGetLastError());
    // adam_kernel walks the arena as float4 groups without knowing its tensors: the fragment image is rebuilt by a launch of
    // its own right behind it (same stream, so inside the same captured graph)
    return a.wimage_plan ? bsarec_wimage_refresh(a.wimage_plan, s) : 0;
}

extern "C" int bsarec_adam_step(const bsarec_adam_t* a, void* state, void* stream) {
    RET(adam_check(a));
    if (!state) return -10;
    hipStream_t s = (hipStream_t)stream;
    LAUNCH(adam_tick_kernel, dim3(1), dim3(ROW_THREADS), 0, s, make_tick(state, 1, a->lr, a->beta1, a->beta2, nullptr, 0, nullptr, nullptr, 0, 0));
    HIPCHK(hipGetLastError());
    return adam_launch(*a, state, s);
}

extern "C" int bsarec_adam_apply(const bsarec_adam_t* a, void* state, void* stream) {
    RET(adam_check(a));
    if (!state) return -10;
    return adam_launch(*a, state, (hipStream_t)stream);
}

// Lazy Adam (cfg.train_lazy_adam): the flat arena must hold the item table (the rows of T are addressed through it), with
// no data-parallel gradient sources and no bf16 shadow (the lazy head is single-GPU fp32).
static int lazy_check(const bsarec_plan& p, const bsarec_adam_t& a) {
    if (!p.cfg.train_lazy_adam) return 0;
    if (a.grads2 || a.n_grad_srcs > 0 || a.shadow_bf16) return -24;
    const long item = (long)p.cfg.item_size * p.cfg.hidden;
    if (!p.G.item_emb || p.G.item_emb < a.grads) return -24;
    const long off = p.G.item_emb - a.grads;
    if (off + item > a.n || (off & 3)) return -24;
    return 0;
}

// The plan-aware Adam of a lazy step (lazy_adam_kernel): dense over the arena without the item table, lazy over T.
// Adam's t / bias corrections were advanced by the step's gradient reduction.
static int lazy_adam_launch(const bsarec_plan& p, const bsarec_adam_t& a, hipStream_t s) {
    LazyAdamP A;
    memset(&A, 0, sizeof(A));
    A.w = a.params; A.g = a.grads; A.m = a.exp_avg; A.v = a.exp_avg_sq;
    A.n = a.n; A.item_off = p.G.item_emb - a.grads; A.item_n = (long)p.cfg.item_size * p.cfg.hidden;
    A.b1 = a.beta1; A.b2 = a.beta2; A.eps = a.eps; A.wd = a.weight_decay; A.gscale = a.grad_scale;
    A.T = p.lazy;
    A.dense_blocks = (int)std::max<long>(1, std::min<long>(cdiv((A.n - A.item_n) / 4, ROW_THREADS), 2048));
    const int lb = (int)std::min<long>(cdiv((long)p.lazy.cap * p.lazy.d4, ROW_THREADS), 1024);
    LAUNCH(lazy_adam_kernel, dim3(A.dense_blocks + lb), dim3(ROW_THREADS), 0, s, (const uint64_t*)p.state, A);
    return (int)hipGetLastError();
}

struct LazyStep {                              // a lazy plan's step runs lazily for the duration of one entry point
    bsarec_plan* p;
    explicit LazyStep(bsarec_plan* q) : p(q) { p->lazy_now = p->cfg.train_lazy_adam != 0; }
    ~LazyStep() { p->lazy_now = false; }
};

extern "C" int bsarec_gather_batch(const int64_t* table, const int64_t* answers_table, const int64_t* perm, long n_samples,
                                   const void* cursor, int B, int L, int64_t* ids_out, int64_t* answers_out, void* stream) {
    if (!table || !answers_table || !perm || !cursor || !ids_out || !answers_out || B < 1 || L < 1) return -10;
    LAUNCH(gather_batch_kernel, dim3(cdiv((long)B * L, ROW_THREADS)), dim3(ROW_THREADS), 0, (hipStream_t)stream, table,
           answers_table, perm, n_samples, (const long long*)cursor, B, L, ids_out, answers_out);
    return (int)hipGetLastError();
}

extern "C" int bsarec_train_step_indexed(bsarec_plan_t* p, const int64_t* table, const int64_t* answers_table,
                                         const int64_t* perm, long n_samples, void* cursor, int64_t* ids_buf,
                                         int64_t* answers_buf, const bsarec_adam_t* a, void* stream) {
    if (!p) return -10;
    RET(adam_check(a));
    RET(sampled_refusal(*p));
    RET(lazy_check(*p, *a));
    hipStream_t s = (hipStream_t)stream;
    if (!table || !answers_table || !perm || !cursor || !ids_buf || !answers_buf) return -10;
    LazyStep lazy(p);
    GatherP gp{table, answers_table, perm, n_samples, (const long long*)cursor, ids_buf, answers_buf};
    RET(forward_impl(p, ids_buf, 1, stream, gp, true));       // batch assembly rides in the embedding kernel
    RET(loss_impl(p, answers_buf, stream, false));
    // the extra block of the final gradient reduction closes the step: mean loss, Adam t and bias corrections, next
    // forward-step index, cursor += B
    const TickP tk = make_tick(p->state, 1, a->lr, a->beta1, a->beta2, p->loss_rows, p->cfg.batch, p->loss, cursor, p->cfg.batch, 1);
    if (can_fuse_adam(*p, *a) && !p->cfg.separate_embed)       // 7 launches: the last one reduces and updates
        return backward_impl(p, stream, tk, a);
    RET(backward_impl(p, stream, tk));
    RET(p->lazy_now ? lazy_adam_launch(*p, *a, s) : adam_launch(*a, p->state, s));
    return wimage_after_adam(*p, *a, s);
}

extern "C" int bsarec_grad_step_indexed(bsarec_plan_t* p, const int64_t* table, const int64_t* answers_table,
                                        const int64_t* perm, long n_samples, void* cursor, int64_t* ids_buf,
                                        int64_t* answers_buf, float lr, float b1, float b2, void* stream) {
    if (!p || !table || !answers_table || !perm || !cursor || !ids_buf || !answers_buf) return -10;
    RET(sampled_refusal(*p));
    if (p->cfg.train_lazy_adam) return -22;    // a lazy plan's item-table update needs the step's T: its Adam runs inside the step
    GatherP gp{table, answers_table, perm, n_samples, (const long long*)cursor, ids_buf, answers_buf};
    RET(forward_impl(p, ids_buf, 1, stream, gp, true));
    RET(bsarec_loss(p, answers_buf, stream));
    // same convention as bsarec_train_step_indexed: the step index / cursor advance when the step is done
    return backward_impl(p, stream, make_tick(p->state, lr > 0.f ? 1 : 0, lr, b1, b2, nullptr, 0, nullptr, cursor, p->cfg.batch, 1));
}

extern "C" int bsarec_train_step(bsarec_plan_t* p, const int64_t* ids, const int64_t* answers, const bsarec_adam_t* a,
                                 void* stream) {
    if (!p) return -10;
    RET(adam_check(a));
    RET(sampled_refusal(*p));
    RET(lazy_check(*p, *a));
    if (p->cfg.train_lazy_adam) {
        // lazy: the gradient reduction's extra block advances Adam's t (as bsarec_adam_step's tick would), then the dense
        // update of the rest of the arena and the lazy one of T in one launch
        LazyStep lazy(p);
        RET(bsarec_step_begin(p, stream));
        RET(bsarec_forward_last(p, ids, 1, stream));
        RET(bsarec_loss(p, answers, stream));
        TickP tk = make_tick(p->state, 1, a->lr, a->beta1, a->beta2, nullptr, 0, nullptr, nullptr, 0, 0);
        RET(backward_impl(p, stream, tk));
        RET(lazy_adam_launch(*p, *a, (hipStream_t)stream));
        return wimage_after_adam(*p, *a, (hipStream_t)stream);
    }
    RET(bsarec_step_begin(p, stream));
    RET(bsarec_forward_last(p, ids, 1, stream));
    RET(bsarec_loss(p, answers, stream));
    RET(bsarec_backward(p, stream));
    RET(bsarec_adam_step(a, p->state, stream));
    return wimage_after_adam(*p, *a, (hipStream_t)stream);
}

extern "C" int bsarec_mask_seen(float* scores, long ld, int B, const int64_t* users, const int64_t* indptr,
                                const int64_t* indices, void* stream) {
    if (!scores || !users || !indptr || !indices || B < 1 || ld < 1) return -10;
    hipLaunchKernelGGL(mask_seen_kernel, dim3(B), dim3(ROW_THREADS), 0, (hipStream_t)stream, scores, ld, users, indptr, indices);
    return (int)hipGetLastError();
}

extern "C" int bsarec_topk_seen(float* scores, long ld, int B, int V, const int64_t* users, const int64_t* indptr,
                                const int64_t* indices, int k, int64_t* out_idx, float* out_val, void* stream) {
    static_assert(BSAREC_TOPK_MAX == TOPK_MAX && ROW_THREADS == 256, "topk_seen_kernel: one thread per digit bin");
    if (!scores || !out_idx || B < 1 || V < 1 || ld < V || k < 1 || k > BSAREC_TOPK_MAX || k > V) return -10;
    if (indptr && (!users || !indices)) return -10;
    hipLaunchKernelGGL(topk_seen_kernel, dim3(B), dim3(ROW_THREADS), 0, (hipStream_t)stream, scores, ld, V, users, indptr, indices, k,
                       out_idx, out_val);
    return (int)hipGetLastError();
}

// Argument conditions the catalogue entry points share: a row of d floats is read as float4s, d <= 256 bounds the LDS tiles;
// E holds rows [col_base, col_base + V) of a catalogue whose ids fit an int.
static bool row_dim_ok(int d) { return d >= 4 && d <= 256 && d % 4 == 0; }
static bool aligned_to(const void* p, uintptr_t a) { return p && (uintptr_t)p % a == 0; }
static bool col_range_ok(long col_base, int V) { return col_base >= 0 && col_base + V <= 0x7fffffffL; }
// the pointers of an entry point: p16 aligned to 16 bytes, p8 to 8, p4 to 4, none null (aligned_to fails a null pointer)
static int ptrs_check(std::initializer_list<const void*> p16, std::initializer_list<const void*> p8 = {},
                      std::initializer_list<const void*> p4 = {}) {
    for (const void* p : p16)
        if (!aligned_to(p, 16)) return -10;
    for (const void* p : p8)
        if (!aligned_to(p, 8)) return -10;
    for (const void* p : p4)
        if (!aligned_to(p, 4)) return -10;
    return 0;
}
// what the plan-less sequence layers share: B <= 65536 sequences of min_len .. 256 positions; a dropout rate in [0, 1)
static bool seq_shape_ok(int batch, int seq_len, int min_len) {
    return batch >= 1 && batch <= 65536 && seq_len >= min_len && seq_len <= 256;
}
static bool dropout_ok(float p) { return p >= 0.f && p < 1.f; }           // NaN fails both comparisons

// A score-tile kernel's h tile is rows x (d + 4) floats: up to 133 KB of the 160 KB LDS (128 rows, d = 256), past the 64 KB a
// launch gets without asking.  Once per process (`done` is the family's flag) every kernel's limit is raised to its largest tile.
static size_t tile_smem(int rows, int d) { return (size_t)rows * (d + 4) * sizeof(float); }
struct TileKernel { const void* fn; int rows; };
static int tile_lds_once(bool& done, std::initializer_list<TileKernel> kernels) {
    if (done) return 0;
    for (const TileKernel& k : kernels) {
        const hipError_t e = hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tile_smem(k.rows, 256));
        if (e != hipSuccess) return (int)e;
    }
    done = true;
    return 0;
}
// The grid of the filter and of the count kernel: (row tiles, item groups), about 1024 workgroups.
static dim3 fr_tile_grid(int B, int V) {
    const int tiles = (B + FR_ROWS - 1) / FR_ROWS, nblk = (V + FR_ITEMS - 1) / FR_ITEMS;
    const int groups = (1024 + tiles - 1) / tiles;
    return dim3(tiles, groups > nblk ? nblk : groups);
}

extern "C" int bsarec_sampled_rank(const float* h, long ldh, const float* item_emb, int B, int V, int d, const int64_t* users,
                                   const int64_t* answers, const int64_t* indptr, const int64_t* indices, const int64_t* pop_cum,
                                   int n_neg, uint64_t seed, uint32_t tag, int32_t* rank_out, int64_t* cand_out, float* score_out,
                                   void* stream) {
    static_assert(BSAREC_NEG_MAX == NEG_MAX && BSAREC_NEG_MAX_DRAWS == NEG_MAX_DRAWS, "sampled_rank_kernel: the header's limits");
    if (!h || !item_emb || !users || !answers || !rank_out || (indptr && !indices)) return -10;
    if (B < 1 || V < 2 || !row_dim_ok(d) || ldh < d || n_neg < 1 || n_neg > BSAREC_NEG_MAX) return -10;
    if (!aligned_to(item_emb, 16)) return -10;                        // float4 row loads
    hipLaunchKernelGGL(sampled_rank_kernel, dim3(B), dim3(ROW_THREADS), 0, (hipStream_t)stream, h, ldh, item_emb, V, d, users, answers,
                       indptr, indices, pop_cum, n_neg, (uint32_t)seed, (uint32_t)(seed >> 32), tag, rank_out, cand_out, score_out);
    return (int)hipGetLastError();
}

// Full-catalogue top-k without the score matrix (full_rank.h).  Sizes of one call: s sampled columns per row (a function of
// k and V only), cap list entries per row (cand_cap, or by default about 4 k V / s: expected survivors ~ k V / s = cap / 4); s ~ 4 sqrt(k V).
struct FrShape { long s, stride, cap; };
static bool fr_shape(int B, int V, int d, int k, int cand_cap, FrShape* out) {
    if (B < 1 || k < 1 || k > BSAREC_TOPK_MAX || V < k || !row_dim_ok(d)) return false;
    if (cand_cap < 0 || (cand_cap > 0 && cand_cap < k) || cand_cap > (1 << 30)) return false;
    const long kv = (long)k * V;
    long s = 4 * (long)std::sqrt((double)kv);
    if (s < 4L * k) s = 4L * k;
    if (s > V) s = V;
    long cap = cand_cap;
    if (cap == 0) {
        cap = (4 * kv + s - 1) / s;
        cap = (cap + 255) / 256 * 256;
        if (cap < k) cap = k;
    }
    out->s = s; out->stride = V / s; out->cap = cap;
    return true;
}
static long fr_align(long x) { return (x + 255) / 256 * 256; }

extern "C" long bsarec_topk_full_workspace_bytes(int B, int V, int d, int k, int cand_cap) {
    FrShape f;
    if (!fr_shape(B, V, d, k, cand_cap, &f)) return -10;
    return fr_align((long)B * 8) + fr_align((long)B * 4) + fr_align((long)B * f.s * 4) + (long)B * f.cap * 8;
}

// One code path: bsarec_topk_full is the col_base = 0 case.  item_emb holds rows [col_base, col_base + V) of the catalogue;
// the CSR entries and out_idx are global ids (full_rank.h).
extern "C" int bsarec_topk_full_range(const float* h, long ldh, const float* item_emb, int B, int V, long col_base, int d,
                                      const int64_t* users, const int64_t* indptr, const int64_t* indices, int k, int cand_cap,
                                      void* workspace, long workspace_bytes, int64_t* out_idx, float* out_val, void* stream) {
    static_assert(BSAREC_TOPK_MAX == TOPK_MAX && ROW_THREADS == 256 && FR_ROWS == 128, "full_rank.h: the header's limits");
    FrShape f;
    if (!fr_shape(B, V, d, k, cand_cap, &f)) return -10;
    if (!col_range_ok(col_base, V)) return -10;
    if (!h || !item_emb || !workspace || !out_idx || ldh < d || (indptr && (!users || !indices))) return -10;
    if (!aligned_to(h, 16) || !aligned_to(item_emb, 16) || !aligned_to(workspace, 16)) return -10;
    if (workspace_bytes < bsarec_topk_full_workspace_bytes(B, V, d, k, cand_cap)) return -10;
    char* ws = (char*)workspace;
    unsigned long long* tau = (unsigned long long*)ws;           ws += fr_align((long)B * 8);
    unsigned* count = (unsigned*)ws;                             ws += fr_align((long)B * 4);
    unsigned* skeys = (unsigned*)ws;                             ws += fr_align((long)B * f.s * 4);
    unsigned long long* list = (unsigned long long*)ws;
    const int cap = (int)f.cap;
    hipStream_t st = (hipStream_t)stream;
    static bool raised = false;
    RET(tile_lds_once(raised, {{(const void*)full_rank_filter_kernel, FR_ROWS}}));
    hipLaunchKernelGGL(full_rank_sample_kernel, dim3(B), dim3(ROW_THREADS), 0, st, h, ldh, item_emb, V, col_base, d, users, indptr,
                       indices, k, (int)f.s, (int)f.stride, skeys, tau, count);
    for (int round = 0; round <= FR_ROUNDS; ++round) {
        if (round > 0)
            hipLaunchKernelGGL(full_rank_rethreshold_kernel, dim3(B), dim3(ROW_THREADS), 0, st, k, cap, tau, count, list);
        hipLaunchKernelGGL(full_rank_filter_kernel, fr_tile_grid(B, V), dim3(ROW_THREADS), tile_smem(FR_ROWS, d), st, h, ldh, item_emb, B,
                           V, d, cap, tau, count, list);
    }
    hipLaunchKernelGGL(full_rank_select_kernel, dim3(B), dim3(ROW_THREADS), 0, st, V, col_base, k, cap, users, indptr, indices, count,
                       list, out_idx, out_val);
    hipLaunchKernelGGL(full_rank_fallback_kernel, dim3(B), dim3(ROW_THREADS), 0, st, h, ldh, item_emb, V, col_base, d, k, cap, users,
                       indptr, indices, count, out_idx, out_val);
    return (int)hipGetLastError();
}

extern "C" int bsarec_topk_full(const float* h, long ldh, const float* item_emb, int B, int V, int d, const int64_t* users,
                                const int64_t* indptr, const int64_t* indices, int k, int cand_cap, void* workspace,
                                long workspace_bytes, int64_t* out_idx, float* out_val, void* stream) {
    return bsarec_topk_full_range(h, ldh, item_emb, B, V, 0, d, users, indptr, indices, k, cand_cap, workspace, workspace_bytes,
                                  out_idx, out_val, stream);
}

// The answer's rank without a list (answer_rank.h): the per-row launch, then the count launch; no workspace.
static int answer_rank_check(const float* h, long ldh, const float* E, int B, int V, long col_base, int d, const int64_t* users,
                             const int64_t* indptr, const int64_t* indices, const int64_t* answers, const void* out) {
    if (B < 1 || V < 1 || !row_dim_ok(d) || ldh < d) return -10;
    if (!col_range_ok(col_base, V)) return -10;
    if (!h || !E || !answers || !out || (indptr && (!users || !indices))) return -10;
    if (!aligned_to(h, 16) || !aligned_to(E, 16)) return -10;
    return 0;
}

extern "C" int bsarec_answer_rank_range(const float* h, long ldh, const float* item_rows, int B, int Vs, long col_base, int d,
                                        const int64_t* users, const int64_t* indptr, const int64_t* indices, const int64_t* answers,
                                        const float* answer_score, int32_t* rank_out, float* score_out, void* stream) {
    RET(answer_rank_check(h, ldh, item_rows, B, Vs, col_base, d, users, indptr, indices, answers, rank_out));
    hipStream_t st = (hipStream_t)stream;
    static bool raised = false;
    RET(tile_lds_once(raised, {{(const void*)answer_rank_count_kernel, FR_ROWS}}));
    hipLaunchKernelGGL(answer_rank_row_kernel<false>, dim3(B), dim3(ROW_THREADS), 0, st, h, ldh, item_rows, Vs, col_base, d, users,
                       indptr, indices, answers, answer_score, rank_out, score_out);
    hipLaunchKernelGGL(answer_rank_count_kernel, fr_tile_grid(B, Vs), dim3(ROW_THREADS), tile_smem(FR_ROWS, d), st, h, ldh, item_rows, B,
                       Vs, col_base, d, users, indptr, indices, answers, answer_score, (const float*)score_out, rank_out);
    return (int)hipGetLastError();
}

extern "C" int bsarec_answer_rank(const float* h, long ldh, const float* item_emb, int B, int V, int d, const int64_t* users,
                                  const int64_t* indptr, const int64_t* indices, const int64_t* answers, int32_t* rank_out,
                                  float* score_out, void* stream) {
    return bsarec_answer_rank_range(h, ldh, item_emb, B, V, 0, d, users, indptr, indices, answers, nullptr, rank_out, score_out,
                                    stream);
}

extern "C" int bsarec_answer_score_range(const float* h, long ldh, const float* item_rows, int B, int Vs, long col_base, int d,
                                         const int64_t* users, const int64_t* indptr, const int64_t* indices,
                                         const int64_t* answers, float* score_out, void* stream) {
    RET(answer_rank_check(h, ldh, item_rows, B, Vs, col_base, d, users, indptr, indices, answers, score_out));
    hipLaunchKernelGGL(answer_rank_row_kernel<true>, dim3(B), dim3(ROW_THREADS), 0, (hipStream_t)stream, h, ldh, item_rows, Vs,
                       col_base, d, users, indptr, indices, answers, (const float*)nullptr, (int32_t*)nullptr, score_out);
    return (int)hipGetLastError();
}

// DuoRec's contrastive head (info_nce.h): plan-less, everything on the caller's stream, no allocation.
static int info_nce_shape_check(int B, int d, int sim) {
    if (B < 1 || B > 4096 || !row_dim_ok(d) || (sim != 0 && sim != 1)) return -10;
    return 0;
}

extern "C" long bsarec_info_nce_workspace_bytes(int B, int d, int sim) {
    if (info_nce_shape_check(B, d, sim)) return -10;
    return nce_workspace_floats(B, d) * (long)sizeof(float);
}

static int info_nce_params(NceP& P, const float* z_i, long ld_i, const float* z_j, long ld_j, int B, int d, float inv_tau, int sim,
                           void* workspace, long workspace_bytes) {
    RET(info_nce_shape_check(B, d, sim));
    if (ld_i < d || ld_j < d || ld_i % 4 != 0 || ld_j % 4 != 0) return -10;
    if (!(inv_tau > 0.f) || !std::isfinite(inv_tau)) return -10;
    if (!z_i || !z_j || !workspace || !aligned_to(z_i, 16) || !aligned_to(z_j, 16) || !aligned_to(workspace, 16)) return -10;
    if (workspace_bytes < bsarec_info_nce_workspace_bytes(B, d, sim)) return -10;
    const long n = 2L * B;
    P.zi = z_i; P.zj = z_j; P.ldi = ld_i; P.ldj = ld_j;
    P.B = B; P.n = (int)n; P.d = d; P.cos = sim; P.S = nce_splits((int)n); P.T = cdiv(n, NCE_TILE);
    P.inv_tau = inv_tau;
    float* w = (float*)workspace;
    P.lse = w; P.spos = w + n; P.norm = w + 2 * n; P.pm = w + 3 * n; P.pl = P.pm + P.S * n; P.slab = w + nce_stat_floats(n, P.S);
    return 0;
}

extern "C" int bsarec_info_nce_fwd(const float* z_i, long ld_i, const float* z_j, long ld_j, int B, int d, float inv_tau, int sim,
                                   float* loss_out, float* rows_out, void* workspace, long workspace_bytes, void* stream) {
    NceP P;
    RET(info_nce_params(P, z_i, ld_i, z_j, ld_j, B, d, inv_tau, sim, workspace, workspace_bytes));
    if (!loss_out) return -10;
    hipStream_t st = (hipStream_t)stream;
    if (P.cos) hipLaunchKernelGGL(nce_norm_kernel, dim3(cdiv(P.n, ROW_THREADS / 64)), dim3(ROW_THREADS), 0, st, P);
    hipLaunchKernelGGL(nce_fwd_kernel, dim3(P.S, P.T), dim3(ROW_THREADS), 0, st, P);
    hipLaunchKernelGGL(nce_stat_kernel, dim3(1), dim3(1024), 0, st, P, loss_out, rows_out);
    return (int)hipGetLastError();
}

extern "C" int bsarec_info_nce_bwd(const float* z_i, long ld_i, const float* z_j, long ld_j, int B, int d, float inv_tau, int sim,
                                   const float* gout, void* workspace, long workspace_bytes, float* dz_i, float* dz_j,
                                   void* stream) {
    NceP P;
    RET(info_nce_params(P, z_i, ld_i, z_j, ld_j, B, d, inv_tau, sim, workspace, workspace_bytes));
    if (!gout || !dz_i || !dz_j || !aligned_to(dz_i, 16) || !aligned_to(dz_j, 16)) return -10;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(P.S, P.T);
    switch (cdiv(d, NCE_TILE)) {
        case 1: hipLaunchKernelGGL(nce_bwd_kernel<1>, grid, dim3(ROW_THREADS), 0, st, P); break;
        case 2: hipLaunchKernelGGL(nce_bwd_kernel<2>, grid, dim3(ROW_THREADS), 0, st, P); break;
        case 3: hipLaunchKernelGGL(nce_bwd_kernel<3>, grid, dim3(ROW_THREADS), 0, st, P); break;
        default: hipLaunchKernelGGL(nce_bwd_kernel<4>, grid, dim3(ROW_THREADS), 0, st, P); break;
    }
    hipLaunchKernelGGL(nce_dz_kernel, dim3(cdiv(P.n, ROW_THREADS / 64)), dim3(ROW_THREADS), 0, st, P, gout, dz_i, dz_j);
    return (int)hipGetLastError();
}

// Full-catalogue cross-entropy on an external hidden state (ce_head.h): plan-less, everything on the caller's stream, no allocation.
static int ce_head_shape_check(int B, int V, int d) {
    if (B < 1 || B > 65536 || V < 1 || !row_dim_ok(d)) return -10;
    return 0;
}

extern "C" long bsarec_ce_head_workspace_bytes(int B, int V, int d) {
    if (ce_head_shape_check(B, V, d)) return -10;
    return ce_workspace_floats(B, V, d) * (long)sizeof(float);
}

// A range without rows (Vs = 0) keeps the workspace of one row.
extern "C" long bsarec_ce_head_range_workspace_bytes(int Bg, int Vs, int d) {
    if (Vs < 0) return -10;
    return bsarec_ce_head_workspace_bytes(Bg, Vs > 1 ? Vs : 1, d);
}

// item_emb: rows [base, base + V) of a catalogue of N rows (the single-table entry points: base 0, N = V >= 1)
static int ce_head_params(CeP& P, const float* h, long ldh, const float* item_emb, int B, int V, long base, long N, int d,
                          const int64_t* answers, void* workspace, long workspace_bytes) {
    if (V < 0 || base < 0 || base + V > N || N > 2147483647L) return -10;
    RET(ce_head_shape_check(B, V > 1 ? V : 1, d));
    if (ldh < d || ldh % 4 != 0) return -10;
    if (!h || !item_emb || !answers || !workspace) return -10;
    if (!aligned_to(h, 16) || !aligned_to(item_emb, 16) || !aligned_to(workspace, 16)) return -10;
    if (workspace_bytes < bsarec_ce_head_range_workspace_bytes(B, V, d)) return -10;
    P.h = h; P.ldh = ldh; P.E = item_emb; P.ans = answers;
    P.B = B; P.V = V; P.d = d; P.S = ce_splits(B, V); P.nblk = ce_nblk(V);
    P.N = (int)N; P.base = base;
    P.rows = nullptr; P.count = nullptr;          // the identity, all B rows live
    float* w = (float*)workspace;
    P.m = w; P.logl = w + B; P.pm = w + 2L * B; P.pl = P.pm + (long)P.S * B; P.slab = w + ce_stat_floats(B, P.S);
    return 0;
}

static int ce_head_attributes() {
    static bool raised = false;
    return tile_lds_once(raised, {{(const void*)ce_fwd_kernel, CE_ROWS},
                                  {(const void*)ce_dh_kernel<4, 1>, 128}, {(const void*)ce_dh_kernel<4, 2>, 128},
                                  {(const void*)ce_dh_kernel<2, 4>, 64}, {(const void*)ce_dh_kernel<1, 8>, 32},
                                  {(const void*)ce_de_kernel<1>, CE_ROWS}, {(const void*)ce_de_kernel<2>, CE_ROWS},
                                  {(const void*)ce_de_kernel<4>, CE_ROWS}, {(const void*)ce_de_kernel<8>, CE_ROWS}});
}

extern "C" int bsarec_ce_head_fwd(const float* h, long ldh, const float* item_emb, int B, int V, int d, const int64_t* answers,
                                  float* loss_out, float* rows_out, void* workspace, long workspace_bytes, void* stream) {
    CeP P;
    if (V < 1) return -10;
    RET(ce_head_params(P, h, ldh, item_emb, B, V, 0, V, d, answers, workspace, workspace_bytes));
    if (!loss_out) return -10;
    RET(ce_head_attributes());
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ce_fwd_kernel, dim3(P.S, cdiv(B, CE_ROWS)), dim3(ROW_THREADS), tile_smem(CE_ROWS, d), st, P);
    hipLaunchKernelGGL(ce_stat_kernel<false>, dim3(1), dim3(1024), 0, st, P, loss_out, rows_out);
    return (int)hipGetLastError();
}

// d(h) of P's rows of E (the slabs in split order, times g / B) and dE of those rows, from the m and log l in the workspace
static int ce_head_bwd_launch(const CeP& P, const float* gout, float* dh, float* d_item_emb, hipStream_t st) {
    if (!gout || !dh || !d_item_emb || !aligned_to(dh, 16) || !aligned_to(d_item_emb, 16)) return -10;
    RET(ce_head_attributes());
    const int ndc = ce_ndc(P.d), rows = 32 * ce_dh_rb(ndc);
    const dim3 grid(P.S, cdiv(P.B, rows)), wg(ROW_THREADS);
    const size_t smem_dh = tile_smem(rows, P.d), smem_de = tile_smem(CE_ROWS, P.d);
    switch (ndc) {
        case 1: hipLaunchKernelGGL((ce_dh_kernel<4, 1>), grid, wg, smem_dh, st, P); break;
        case 2: hipLaunchKernelGGL((ce_dh_kernel<4, 2>), grid, wg, smem_dh, st, P); break;
        case 4: hipLaunchKernelGGL((ce_dh_kernel<2, 4>), grid, wg, smem_dh, st, P); break;
        default: hipLaunchKernelGGL((ce_dh_kernel<1, 8>), grid, wg, smem_dh, st, P); break;
    }
    hipLaunchKernelGGL(ce_dh_sum_kernel, dim3(cdiv((long)P.B * P.d / 4, ROW_THREADS)), wg, 0, st, P, gout, dh);
    switch (ndc) {
        case 1: hipLaunchKernelGGL(ce_de_kernel<1>, dim3(P.nblk), wg, smem_de, st, P, gout, d_item_emb); break;
        case 2: hipLaunchKernelGGL(ce_de_kernel<2>, dim3(P.nblk), wg, smem_de, st, P, gout, d_item_emb); break;
        case 4: hipLaunchKernelGGL(ce_de_kernel<4>, dim3(P.nblk), wg, smem_de, st, P, gout, d_item_emb); break;
        default: hipLaunchKernelGGL(ce_de_kernel<8>, dim3(P.nblk), wg, smem_de, st, P, gout, d_item_emb); break;
    }
    return (int)hipGetLastError();
}

extern "C" int bsarec_ce_head_bwd(const float* h, long ldh, const float* item_emb, int B, int V, int d, const int64_t* answers,
                                  const float* gout, void* workspace, long workspace_bytes, float* dh, float* d_item_emb,
                                  void* stream) {
    CeP P;
    if (V < 1) return -10;
    RET(ce_head_params(P, h, ldh, item_emb, B, V, 0, V, d, answers, workspace, workspace_bytes));
    return ce_head_bwd_launch(P, gout, dh, d_item_emb, (hipStream_t)stream);
}

// The cloze head (BERT4Rec): the same kernels over a row list of capacity R with a live count on the device (ce_head.h).
extern "C" long bsarec_cloze_head_workspace_bytes(int R, int V, int d) { return bsarec_ce_head_workspace_bytes(R, V, d); }

static int cloze_head_params(CeP& P, const float* h, long ldh, long T, const float* item_emb, int R, int V, int d,
                             const int32_t* rows, const int64_t* targets, const int32_t* count, void* workspace,
                             long workspace_bytes) {
    if (V < 1 || T < 1 || !row_dim_ok(d) || T > 2147483647L / d) return -10;
    if (!rows || !count || !aligned_to(rows, 4) || !aligned_to(count, 4) || !aligned_to(targets, 8)) return -10;
    RET(ce_head_params(P, h, ldh, item_emb, R, V, 0, V, d, targets, workspace, workspace_bytes));
    P.rows = rows; P.count = count;
    return 0;
}

extern "C" int bsarec_cloze_head_fwd(const float* h, long ldh, long T, const float* item_emb, int R, int V, int d,
                                     const int32_t* rows, const int64_t* targets, const int32_t* count, float* loss_out,
                                     float* rows_out, void* workspace, long workspace_bytes, void* stream) {
    CeP P;
    RET(cloze_head_params(P, h, ldh, T, item_emb, R, V, d, rows, targets, count, workspace, workspace_bytes));
    if (!loss_out) return -10;
    RET(ce_head_attributes());
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ce_fwd_kernel, dim3(P.S, cdiv(R, CE_ROWS)), dim3(ROW_THREADS), tile_smem(CE_ROWS, d), st, P);
    hipLaunchKernelGGL(ce_stat_kernel<false>, dim3(1), dim3(1024), 0, st, P, loss_out, rows_out);
    return (int)hipGetLastError();
}

extern "C" int bsarec_cloze_head_bwd(const float* h, long ldh, long T, const float* item_emb, int R, int V, int d,
                                     const int32_t* rows, const int64_t* targets, const int32_t* count, const float* gout,
                                     void* workspace, long workspace_bytes, float* dh, float* d_item_emb, void* stream) {
    CeP P;
    RET(cloze_head_params(P, h, ldh, T, item_emb, R, V, d, rows, targets, count, workspace, workspace_bytes));
    if (!gout || !dh || !d_item_emb || !aligned_to(dh, 16) || !aligned_to(d_item_emb, 16)) return -10;
    RET((int)hipMemsetAsync(dh, 0, (size_t)T * d * sizeof(float), (hipStream_t)stream));      // the rows outside the list
    return ce_head_bwd_launch(P, gout, dh, d_item_emb, (hipStream_t)stream);
}

// BERT4Rec's masking step (cloze.h)
extern "C" int bsarec_cloze_mask(const int64_t* ids, int B, int L, float ratio, int slots, int64_t mask_token, const void* state,
                                 int64_t* masked_ids, int32_t* rows, int64_t* targets, int32_t* count, void* stream) {
    if (B < 1 || B > 65536 || L < 1 || L > 256 || slots < 1 || slots > L || (long)B * slots > 65536) return -10;
    if (!(ratio >= 0.0f && ratio <= 1.0f)) return -10;                          // (NaN fails both comparisons)
    if (!ids || !state || !masked_ids || !rows || !targets || !count) return -10;
    if (!aligned_to(ids, 8) || !aligned_to(state, 8) || !aligned_to(masked_ids, 8) || !aligned_to(targets, 8) ||
        !aligned_to(rows, 4) || !aligned_to(count, 4)) return -10;
    ClozeP P;
    P.ids = ids; P.B = B; P.L = L; P.slots = slots; P.mask_token = mask_token; P.state = (const uint64_t*)state;
    const double th = (double)ratio * 4294967296.0;                              // oracle.dropout_threshold
    P.thresh = th >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)th;
    P.masked_ids = masked_ids; P.rows = rows; P.targets = targets; P.count = count;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cloze_draw_kernel, dim3(cdiv(B, CLOZE_THREADS / 64)), dim3(CLOZE_THREADS), 0, st, P);
    hipLaunchKernelGGL(cloze_compact_kernel, dim3(1), dim3(1024), 0, st, P);
    return (int)hipGetLastError();
}

// Range form of the head: one shard of a catalogue split by rows (ce_head.h).  stats -> (the caller's exchange) -> merge -> bwd.
extern "C" int bsarec_ce_head_range_stats(const float* h, long ldh, const float* item_rows, int Bg, int Vs, long col_base,
                                          long item_size, int d, const int64_t* answers, float* stats, void* workspace,
                                          long workspace_bytes, void* stream) {
    CeP P;
    RET(ce_head_params(P, h, ldh, item_rows, Bg, Vs, col_base, item_size, d, answers, workspace, workspace_bytes));
    if (!stats) return -10;
    hipStream_t st = (hipStream_t)stream;
    if (Vs > 0) {
        RET(ce_head_attributes());
        hipLaunchKernelGGL(ce_fwd_kernel, dim3(P.S, cdiv(Bg, CE_ROWS)), dim3(ROW_THREADS), tile_smem(CE_ROWS, d), st, P);
    }
    hipLaunchKernelGGL(ce_stat_kernel<true>, dim3(1), dim3(1024), 0, st, P, (float*)nullptr, stats);      // Vs = 0: S = 0
    return (int)hipGetLastError();
}

extern "C" int bsarec_ce_head_range_merge(const float* stats_all, int world, int Bg, void* workspace, long workspace_bytes,
                                          float* loss_rows, float* loss, void* stream) {
    if (world < 1 || world > 8 || Bg < 1 || Bg > 65536) return -10;
    if (!stats_all || !workspace || !aligned_to(workspace, 16) || !loss_rows || !loss) return -10;
    if (workspace_bytes < 2L * Bg * (long)sizeof(float)) return -10;          // m[Bg] | logl[Bg]: the head of every layout
    float* w = (float*)workspace;
    hipLaunchKernelGGL(ce_merge_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, stats_all, world, Bg, w, w + Bg, loss_rows, loss);
    return (int)hipGetLastError();
}

extern "C" int bsarec_ce_head_range_bwd(const float* h, long ldh, const float* item_rows, int Bg, int Vs, long col_base,
                                        long item_size, int d, const int64_t* answers, const float* gout, void* workspace,
                                        long workspace_bytes, float* dh_part, float* dE_rows, void* stream) {
    CeP P;
    RET(ce_head_params(P, h, ldh, item_rows, Bg, Vs, col_base, item_size, d, answers, workspace, workspace_bytes));
    if (Vs == 0) {
        if (!gout || !dh_part || !aligned_to(dh_part, 16)) return -10;
        return (int)hipMemsetAsync(dh_part, 0, (size_t)Bg * d * sizeof(float), (hipStream_t)stream);
    }
    return ce_head_bwd_launch(P, gout, dh_part, dE_rows, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// Dense products of the plan-less layers (the GRU stack, the LRU and Mamba layers, the LRURec step): fp32 products on 64 x 64
// tiles of the GEMM core, on the caller's stream.  A weight gradient is a split-K product into slabs that the caller owns, and
// one sum over the slabs.
// ---------------------------------------------------------------------------------------------
// split-K of a weight-gradient product over K rows: slices of >= 256 rows, 64 at the most; a function of K alone
static void split_k(long K, int* nsplit, int* kchunk) {
    long ns = (K + 255) / 256;
    ns = ns < 1 ? 1 : (ns > 64 ? 64 : ns);
    const long kc = rup((K + ns - 1) / ns, GEMM_BK);
    *kchunk = (int)kc;
    *nsplit = kc > 0 ? (int)((K + kc - 1) / kc) : 1;
    if (*nsplit < 1) *nsplit = 1;
}
// C (+ bias); P, Q != 0: row r = p Q + q of the product is stored at row q P + p
static EpiGru dense_epi(float* C, long ldc, const float* bias = nullptr, int P = 0, int Q = 0) {
    EpiGru e;
    e.C = C; e.ldc = ldc; e.c_split = 0; e.bias = bias; e.P = P; e.Q = Q;
    return e;
}
// C[M, N] = A[M, K] . W[N, K]^T through the epilogue e
template <class Epi>
static int dense_nt(const float* A, const float* W, int M, int N, int K, const Epi& e, hipStream_t s) {
    GemmP g = gemm_defaults(M, N, K);
    g.lda = K; g.ldb = K; g.A[0] = A; g.B[0] = W;
    return launch_gemm<64, 64, 2, 2, false, false, XF_NONE, XF_NONE, false>(g, no_xform(), e, nullptr, 1, s, BSAREC_K_NONE, true);
}
// C[M, N] = A[M, K] . W[K, N] through the epilogue e
template <class Epi>
static int dense_nn(const float* A, const float* W, int M, int N, int K, const Epi& e, hipStream_t s) {
    GemmP g = gemm_defaults(M, N, K);
    g.lda = K; g.ldb = N; g.A[0] = A; g.B[0] = W;
    return launch_gemm<64, 64, 2, 2, false, true, XF_NONE, XF_NONE, false>(g, no_xform(), e, nullptr, 1, s, BSAREC_K_NONE, true);
}
// out[M, N] = A[K, M]^T . Bm[K, N] in split-K slabs at slab + coff, M x Nfull each (the caller sums them); bpart: the column
// sums of A per split, [ns][M]
static int dense_tn(const float* A, long lda, const float* Bm, int M, int N, long K, float* slab, long slab_floats, long coff,
                    float* bpart, hipStream_t s) {
    int ns, kc;
    split_k(K, &ns, &kc);
    GemmP g = gemm_defaults(M, N, (int)K);
    g.lda = lda; g.ldb = N; g.A[0] = A; g.B[0] = Bm; g.nsplit = ns; g.kchunk = kc;
    EpiGru e = dense_epi(slab + coff, N);
    e.c_split = slab_floats;
    if (bpart) return launch_gemm<64, 64, 2, 2, true, true, XF_NONE, XF_NONE, true>(g, no_xform(), e, bpart, 1, s, BSAREC_K_NONE, true);
    return launch_gemm<64, 64, 2, 2, true, true, XF_NONE, XF_NONE, false>(g, no_xform(), e, nullptr, 1, s, BSAREC_K_NONE, true);
}
// out[floats] = the sum of the split_k(K) slabs of `floats` floats each
static void slab_sum(const float* slab, long K, long floats, float* out, hipStream_t s) {
    int ns, kc;
    split_k(K, &ns, &kc);
    hipLaunchKernelGGL(gru_slab_sum_kernel, dim3(cdiv(floats / 4, 256)), dim3(256), 0, s, slab, ns, floats / 4, out);
}
// The backward of Y[rows, out] = X[rows, in] . W[out, in]^T (+ b), four launches at the most, in this order:
// dX = dY . W through dx_epi;  dW = dY^T . X summed over the split-K slabs;  db (null: none) = the column sums of dY.
// slab holds split_k(rows) slabs of out x in floats, bpart (read only with db) as many of `out` floats; both are scratch
static int linear_bwd(const float* dY, const float* X, const float* W, long rows, int out, int in, const EpiGru& dx_epi,
                      float* slab, float* bpart, float* dW, float* db, hipStream_t s) {
    const long wfloats = (long)out * in;
    RET(dense_nn(dY, W, (int)rows, in, out, dx_epi, s));
    RET(dense_tn(dY, out, X, out, in, rows, slab, wfloats, 0, db ? bpart : nullptr, s));
    slab_sum(slab, rows, wfloats, dW, s);
    if (db) slab_sum(bpart, rows, out, db, s);
    return 0;
}

// ---------------------------------------------------------------------------------------------
// GRU stack (gru.h): plan-less, everything on the caller's stream, no allocation
// ---------------------------------------------------------------------------------------------
static int gru_check(const bsarec_gru_config_t* c) {
    if (!c) return -10;
    if (!seq_shape_ok(c->batch, c->seq_len, 1)) return -10;
    if (!row_dim_ok(c->input_size)) return -10;
    if (c->hidden_size != 32 && c->hidden_size != 64 && c->hidden_size != 96 && c->hidden_size != 128) return -10;
    if (c->num_layers < 1 || c->num_layers > 4) return -10;
    if (c->out_size != 0 && !row_dim_ok(c->out_size)) return -10;
    return 0;
}

// Workspace, in floats (every region a multiple of 4): A / da [T][3H] | Y_k [T][H], k < NY | S_k [T][4H] | db_n [T][H] |
// dY ping [T][H] | dY pong [T][H] | x time-major [T][I] | dout time-major [T][O] | slabs [ns][max(3H max(I, H), O H)] |
// bias partials [ns][O]; T = L B, NY = N in training, else min(N, 2); everything behind Y_k in training only
struct GruWs {
    long a, y, s, dbn, dya, dyb, xt, dot, slab, bpart, total;
    int ny, ns;        // ns: the most slabs any of the backward's split-K products writes
};
static GruWs gru_ws(const bsarec_gru_config_t& c, bool train) {
    const long T = (long)c.batch * c.seq_len, H = c.hidden_size, I = c.input_size, O = c.out_size, N = c.num_layers;
    GruWs w;
    memset(&w, 0, sizeof(w));
    for (long K : {T, T - c.batch, (long)c.batch}) {        // the K of every split-K product of the backward
        int ns, kc;
        split_k(K, &ns, &kc);
        w.ns = std::max(w.ns, ns);
    }
    w.ny = train ? (int)N : (int)(N < 2 ? N : 2);
    long off = 0;
    w.a = off; off += T * 3 * H;
    w.y = off; off += w.ny * T * H;
    if (train) {
        w.s = off; off += N * T * 4 * H;
        w.dbn = off; off += T * H;
        w.dya = off; off += T * H;
        w.dyb = off; off += T * H;
        w.xt = off; off += T * I;
        w.dot = off; off += T * O;
        const long big = std::max(3 * H * std::max(I, H), O * H);
        w.slab = off; off += w.ns * big;
        w.bpart = off; off += (long)w.ns * O;
    }
    w.total = off;
    return w;
}

// offsets (floats) into the flat weight array: w_ih_l0 | w_hh_l0 | w_ih_l1 | ... | w_out | b_out
struct GruW { long ih[4], hh[4], out, bout, total; };
static GruW gru_weights(const bsarec_gru_config_t& c) {
    GruW w;
    long off = 0;
    for (int k = 0; k < c.num_layers; ++k) {
        w.ih[k] = off; off += 3L * c.hidden_size * (k == 0 ? c.input_size : c.hidden_size);
        w.hh[k] = off; off += 3L * c.hidden_size * c.hidden_size;
    }
    w.out = off; off += (long)c.out_size * c.hidden_size;
    w.bout = off; off += c.out_size;
    w.total = off;
    return w;
}

extern "C" long bsarec_gru_weight_floats(const bsarec_gru_config_t* cfg) {
    if (gru_check(cfg)) return -10;
    return gru_weights(*cfg).total;
}

extern "C" long bsarec_gru_workspace_bytes(const bsarec_gru_config_t* cfg, int train) {
    if (gru_check(cfg)) return -10;
    return gru_ws(*cfg, train != 0).total * (long)sizeof(float);
}

static void gru_swap(const float* src, float* dst, long P, long Q, int W, hipStream_t s) {
    hipLaunchKernelGGL(gru_swap_rows_kernel, dim3(cdiv(P * Q * (W / 4), 256)), dim3(256), 0, s, src, dst, P, Q, W / 4);
}
#define GRU_DISPATCH(H, KERNEL, ...) \
    switch ((H) / 32) { \
        case 1: hipLaunchKernelGGL(KERNEL<1>, __VA_ARGS__); break; \
        case 2: hipLaunchKernelGGL(KERNEL<2>, __VA_ARGS__); break; \
        case 3: hipLaunchKernelGGL(KERNEL<3>, __VA_ARGS__); break; \
        default: hipLaunchKernelGGL(KERNEL<4>, __VA_ARGS__); break; \
    }

extern "C" int bsarec_gru_fwd(const bsarec_gru_config_t* cfg, const float* x, const float* weights, int train, int last_only,
                              float* out, void* workspace, long workspace_bytes, void* stream) {
    RET(gru_check(cfg));
    RET(ptrs_check({x, weights, out, workspace}));
    if (workspace_bytes < gru_ws(*cfg, train != 0).total * (long)sizeof(float)) return -10;
    const bsarec_gru_config_t& c = *cfg;
    const int B = c.batch, L = c.seq_len, I = c.input_size, H = c.hidden_size, N = c.num_layers, O = c.out_size;
    const long T = (long)B * L;
    const GruWs ws = gru_ws(c, train != 0);
    const GruW wo = gru_weights(c);
    float* w = (float*)workspace;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(cdiv(B, GRU_ROWS)), wg(2 * H);
    const float* y = nullptr;
    for (int k = 0; k < N; ++k) {
        // a = in . W_ih^T, time-major: x's rows (b, t) go through the row map, a layer output is time-major already
        if (k == 0) RET(dense_nt(x, weights + wo.ih[0], (int)T, 3 * H, I, dense_epi(w + ws.a, 3 * H, nullptr, B, L), s));
        else RET(dense_nt(y, weights + wo.ih[k], (int)T, 3 * H, H, dense_epi(w + ws.a, 3 * H), s));
        GruFwdP P;
        P.A = w + ws.a; P.Whh = weights + wo.hh[k]; P.B = B; P.L = L;
        P.Y = w + ws.y + (long)(train ? k : (k & 1)) * T * H;
        P.S = train ? w + ws.s + (long)k * T * 4 * H : nullptr;
        GRU_DISPATCH(H, gru_seq_fwd_kernel, grid, wg, 0, s, P);
        y = P.Y;
    }
    const float* ylast = y + (long)(L - 1) * B * H;
    if (O > 0) {
        if (last_only) RET(dense_nt(ylast, weights + wo.out, B, O, H, dense_epi(out, O, weights + wo.bout), s));
        else RET(dense_nt(y, weights + wo.out, (int)T, O, H, dense_epi(out, O, weights + wo.bout, L, B), s));
    } else {
        if (last_only) gru_swap(ylast, out, 1, B, H, s);
        else gru_swap(y, out, L, B, H, s);
    }
    return (int)hipGetLastError();
}

extern "C" int bsarec_gru_bwd(const bsarec_gru_config_t* cfg, const float* x, const float* weights, int last_only, const float* dout,
                              void* workspace, long workspace_bytes, float* dx, float* dweights, void* stream) {
    RET(gru_check(cfg));
    RET(ptrs_check({x, weights, dout, workspace, dx, dweights}));
    if (workspace_bytes < gru_ws(*cfg, true).total * (long)sizeof(float)) return -10;
    const bsarec_gru_config_t& c = *cfg;
    const int B = c.batch, L = c.seq_len, I = c.input_size, H = c.hidden_size, N = c.num_layers, O = c.out_size;
    const long T = (long)B * L;
    const GruWs ws = gru_ws(c, true);
    const GruW wo = gru_weights(c);
    float* w = (float*)workspace;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(cdiv(B, GRU_ROWS)), wg(2 * H);
    float* slab = w + ws.slab;
    const float* ytop = w + ws.y + (long)(N - 1) * T * H;
    // the top layer's dY (time-major, or the B rows of t = L - 1) and the projection's gradients
    const float* dy = w + ws.dya;
    float* dy_next = w + ws.dyb;
    if (O > 0) {
        const float* d = dout;                    // rows in the order of y's rows
        const float* yrows = ytop + (last_only ? (long)(L - 1) * B * H : 0);
        const long K = last_only ? B : T;
        if (!last_only) { gru_swap(dout, w + ws.dot, B, L, O, s); d = w + ws.dot; }
        RET(linear_bwd(d, yrows, weights + wo.out, K, O, H, dense_epi(w + ws.dya, H), slab, w + ws.bpart, dweights + wo.out,
                       dweights + wo.bout, s));
    } else if (last_only) {
        dy = dout;
    } else {
        gru_swap(dout, w + ws.dya, B, L, H, s);
    }
    gru_swap(x, w + ws.xt, B, L, I, s);
    for (int k = N - 1; k >= 0; --k) {
        const int Ik = k == 0 ? I : H;
        const float* yk = w + ws.y + (long)k * T * H;
        const float* in = k == 0 ? w + ws.xt : w + ws.y + (long)(k - 1) * T * H;
        GruBwdP P;
        P.S = w + ws.s + (long)k * T * 4 * H; P.Y = yk; P.Whh = weights + wo.hh[k]; P.dY = dy;
        P.da = w + ws.a; P.dbn = w + ws.dbn; P.B = B; P.L = L; P.dy_last = (last_only && k == N - 1) ? 1 : 0;
        GRU_DISPATCH(H, gru_seq_bwd_kernel, grid, wg, 0, s, P);
        // d(in) = da . W_ih: the layer below's dY, or dx through the row map;  dW_ih = da^T . in over all T rows
        const EpiGru din = k > 0 ? dense_epi(dy_next, H) : dense_epi(dx, I, nullptr, L, B);
        RET(linear_bwd(P.da, in, weights + wo.ih[k], T, 3 * H, Ik, din, slab, nullptr, dweights + wo.ih[k], nullptr, s));
        if (k > 0) {
            const float* t = dy_next;
            dy_next = (dy == dout) ? w + ws.dya : const_cast<float*>(dy);
            dy = t;
        }
        // dW_hh = (da_r, da_z | db_n)[t >= 1]^T . y[t - 1]: rows 0 .. 2H from da, rows 2H .. 3H from db_n, over (L - 1) B rows
        const long K = T - B;
        RET(dense_tn(P.da + 3L * B * H, 3 * H, yk, 2 * H, H, K, slab, 3L * H * H, 0, nullptr, s));
        RET(dense_tn(P.dbn + (long)B * H, H, yk, H, H, K, slab, 3L * H * H, 2L * H * H, nullptr, s));
        slab_sum(slab, K, 3L * H * H, dweights + wo.hh[k], s);
    }
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Caser convolution block (caser.h): plan-less, everything on the caller's stream, no allocation
// ---------------------------------------------------------------------------------------------
static int caser_check(const bsarec_caser_config_t* c) {
    if (!c) return -10;
    if (!seq_shape_ok(c->batch, c->seq_len, 1)) return -10;
    if (!row_dim_ok(c->width)) return -10;
    if (c->n_h != 4 && c->n_h != 8 && c->n_h != 16 && c->n_h != 32) return -10;
    if (c->n_v < 1 || c->n_v > 16) return -10;
    return 0;
}

// offsets (floats) into the flat weight array, every tensor at a multiple of 4: conv_v.weight [n_v][L] | conv_v.bias [n_v] |
// conv_h.{h-1}.weight [n_h][h][d], conv_h.{h-1}.bias [n_h] for h = 1 .. L (n_h and d are multiples of 4: no gaps among these)
struct CaserW { long bv, h0, total, F; };
static CaserW caser_weights(const bsarec_caser_config_t& c) {
    CaserW w;
    const long L = c.seq_len, d = c.width;
    w.bv = rup((long)c.n_v * L, 4);
    w.h0 = w.bv + rup((long)c.n_v, 4);
    w.total = w.h0 + (long)c.n_h * d * (L * (L + 1) / 2) + (long)c.n_h * L;
    w.F = (long)c.n_v * d + (long)c.n_h * L;
    return w;
}
// workspace: the winning window per cell, int [B][L][n_h] (training); 16 bytes that nothing touches otherwise
static long caser_ws_bytes(const bsarec_caser_config_t& c, bool train) {
    return train ? rup((long)c.batch * c.seq_len * c.n_h * (long)sizeof(int), 16) : 16;
}

extern "C" long bsarec_caser_weight_floats(const bsarec_caser_config_t* cfg) {
    if (caser_check(cfg)) return -10;
    return caser_weights(*cfg).total;
}

extern "C" long bsarec_caser_workspace_bytes(const bsarec_caser_config_t* cfg, int train) {
    if (caser_check(cfg)) return -10;
    return caser_ws_bytes(*cfg, train != 0);
}

extern "C" int bsarec_caser_fwd(const bsarec_caser_config_t* cfg, const float* x, const float* weights, int train, float* z,
                                void* workspace, long workspace_bytes, void* stream) {
    RET(caser_check(cfg));
    RET(ptrs_check({x, weights, z, workspace}));
    if (workspace_bytes < caser_ws_bytes(*cfg, train != 0)) return -10;
    const bsarec_caser_config_t& c = *cfg;
    const CaserW wo = caser_weights(c);
    hipStream_t s = (hipStream_t)stream;
    CaserP P;
    P.x = x; P.w = weights; P.z = z; P.win = train ? (int*)workspace : nullptr;
    P.B = c.batch; P.L = c.seq_len; P.d = c.width; P.nh = c.n_h; P.nv = c.n_v;
    P.F = wo.F; P.bv_off = wo.bv; P.h_off = wo.h0;
    hipLaunchKernelGGL(caser_v_fwd_kernel, dim3(cdiv((long)c.batch * (c.width / 4), 256)), dim3(256), 0, s, P);
    const dim3 grid((c.seq_len + 1) / 2, cdiv(c.batch, 4));
    if (c.n_h <= 16) hipLaunchKernelGGL(caser_h_fwd_kernel<1>, grid, dim3(256), 0, s, P);
    else hipLaunchKernelGGL(caser_h_fwd_kernel<2>, grid, dim3(256), 0, s, P);
    return (int)hipGetLastError();
}

extern "C" int bsarec_caser_bwd(const bsarec_caser_config_t* cfg, const float* x, const float* weights, const float* dz,
                                void* workspace, long workspace_bytes, float* dx, float* dweights, void* stream) {
    RET(caser_check(cfg));
    RET(ptrs_check({x, weights, dz, workspace, dx, dweights}));
    if (workspace_bytes < caser_ws_bytes(*cfg, true)) return -10;
    const bsarec_caser_config_t& c = *cfg;
    const CaserW wo = caser_weights(c);
    hipStream_t s = (hipStream_t)stream;
    CaserBwdP P;
    P.x = x; P.w = weights; P.dz = dz; P.win = (const int*)workspace; P.dx = dx; P.dw = dweights;
    P.B = c.batch; P.L = c.seq_len; P.d = c.width; P.nh = c.n_h; P.nv = c.n_v;
    P.F = wo.F; P.bv_off = wo.bv; P.h_off = wo.h0;
    const int quads = c.seq_len * (c.width / 4), cells = c.seq_len * c.n_h;
    hipLaunchKernelGGL(caser_dx_kernel, dim3(c.batch, cdiv(quads, 256)), dim3(256), (size_t)cells * 6, s, P);
    hipLaunchKernelGGL(caser_dwh_kernel, dim3(cells, cdiv(quads, 256)), dim3(256), 0, s, P);
    hipLaunchKernelGGL(caser_dv_kernel, dim3(c.seq_len + 1, c.n_v), dim3(64), 0, s, P);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// FEARec autocorrelation attention (fea_attn.h): plan-less, one linear chain on the caller's stream, no allocation
// ---------------------------------------------------------------------------------------------
static int fea_check(const bsarec_fea_attn_config_t* c) {
    if (!c) return -10;
    if (!seq_shape_ok(c->batch, c->seq_len, 2)) return -10;
    if (!row_dim_ok(c->width)) return -10;
    if (c->lo < 0 || c->lo >= c->hi || c->hi > c->seq_len / 2 + 1) return -10;
    if (c->topk < 1 || c->topk > 32 || c->topk > c->seq_len) return -10;
    return 0;
}

// workspace, in 4-byte words, every part at a multiple of 4: m [B][L] | idx (train: [k], else [B][k]) | p [B][k] | h [L] | cv [B][L]
struct FeaWs { long m, idx, p, h, cv, total; };
static FeaWs fea_ws(const bsarec_fea_attn_config_t& c) {
    FeaWs w;
    const long B = c.batch, L = c.seq_len, k = c.topk;
    w.m = 0;
    w.idx = rup(B * L, 4);
    w.p = w.idx + rup(c.train ? k : B * k, 4);
    w.h = w.p + rup(B * k, 4);
    w.cv = w.h + rup(L, 4);
    w.total = w.cv + rup(B * L, 4);
    return w;
}

extern "C" long bsarec_fea_attn_workspace_bytes(const bsarec_fea_attn_config_t* cfg) {
    if (fea_check(cfg)) return -10;
    return fea_ws(*cfg).total * 4;
}

static FeaP fea_params(const bsarec_fea_attn_config_t& c, void* workspace) {
    const FeaWs w = fea_ws(c);
    float* f = (float*)workspace;
    FeaP P = {};
    P.m = f + w.m; P.idx = (int*)(f + w.idx); P.p = f + w.p; P.h = f + w.h; P.cv = f + w.cv;
    P.B = c.batch; P.L = c.seq_len; P.D = c.width; P.lo = c.lo; P.hi = c.hi; P.topk = c.topk; P.train = c.train != 0;
    return P;
}

extern "C" int bsarec_fea_attn_fwd(const bsarec_fea_attn_config_t* cfg, const float* q, const float* k, const float* v, float* out,
                                   void* workspace, long workspace_bytes, void* stream) {
    RET(fea_check(cfg));
    RET(ptrs_check({q, k, v, out, workspace}));
    if (workspace_bytes < fea_ws(*cfg).total * 4) return -10;
    const bsarec_fea_attn_config_t& c = *cfg;
    hipStream_t s = (hipStream_t)stream;
    FeaP P = fea_params(c, workspace);
    P.q = q; P.k = k; P.v = v; P.out = out;
    hipLaunchKernelGGL(fea_band_kernel, dim3(1), dim3(256), 0, s, P);
    hipLaunchKernelGGL(fea_corr_kernel, dim3(c.batch), dim3(256), 0, s, P);
    if (P.train) hipLaunchKernelGGL(fea_select_kernel, dim3(1), dim3(1024), 0, s, P);
    hipLaunchKernelGGL(fea_shift_kernel<true>, dim3(c.batch, cdiv((long)c.seq_len * (c.width / 4), 256)), dim3(256), 0, s, P);
    return (int)hipGetLastError();
}

extern "C" int bsarec_fea_attn_bwd(const bsarec_fea_attn_config_t* cfg, const float* q, const float* k, const float* v,
                                   const float* dout, void* workspace, long workspace_bytes, float* dq, float* dk, float* dv,
                                   void* stream) {
    RET(fea_check(cfg));
    RET(ptrs_check({q, k, v, dout, workspace, dq, dk, dv}));
    if (workspace_bytes < fea_ws(*cfg).total * 4) return -10;
    const bsarec_fea_attn_config_t& c = *cfg;
    hipStream_t s = (hipStream_t)stream;
    FeaP P = fea_params(c, workspace);
    P.q = q; P.k = k; P.v = v; P.dout = dout; P.dq = dq; P.dk = dk; P.dv = dv;
    hipLaunchKernelGGL(fea_dp_kernel, dim3(c.batch), dim3(256), 0, s, P);
    hipLaunchKernelGGL(fea_shift_kernel<false>, dim3(c.batch, cdiv((long)c.seq_len * (c.width / 4), 256)), dim3(256), 0, s, P);
    hipLaunchKernelGGL(fea_dqk_kernel, dim3(c.batch, 2), dim3(256), 0, s, P);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Linear recurrent unit layer (lru.h): plan-less, one linear chain on the caller's stream, no allocation
// ---------------------------------------------------------------------------------------------
static int lru_check(const bsarec_lru_config_t* c) {
    if (!c) return -10;
    if (!seq_shape_ok(c->batch, c->seq_len, 1)) return -10;
    if (!row_dim_ok(c->width)) return -10;
    return 0;
}

// offsets (floats) into the flat weight array: nu_log | theta_log | gamma_log | in_proj.weight [2d][d] | in_proj.bias [2d] |
// out_proj.weight [d][2d] | out_proj.bias [d]
struct LruW { long win, bin, wout, bout, total; };
static LruW lru_weights(const bsarec_lru_config_t& c) {
    const long d = c.width;
    LruW w;
    w.win = 3 * d; w.bin = w.win + 2 * d * d; w.wout = w.bin + 2 * d; w.bout = w.wout + 2 * d * d; w.total = w.bout + d;
    return w;
}

// Workspace, in floats (every region a multiple of 4): V [T][2d] | H [T][2d] | lambda, gamma [3d] | G [T][2d] |
// slabs [ns][2 d d] | bias partials [ns][2d] | scan partials [workgroups][3d]; T = B L; everything behind lambda in training only
struct LruWs { long v, h, lam, g, slab, bpart, part, total; int ns, nwg; };
static LruWs lru_ws(const bsarec_lru_config_t& c, bool train) {
    const long T = (long)c.batch * c.seq_len, d = c.width;
    LruWs w;
    memset(&w, 0, sizeof(w));
    int kc;
    split_k(T, &w.ns, &kc);
    w.nwg = cdiv(c.batch, lru_geom(c.width).seqs);
    long off = 0;
    w.v = off; off += T * 2 * d;
    w.h = off; off += T * 2 * d;
    w.lam = off; off += 3 * d;
    if (train) {
        w.g = off; off += T * 2 * d;
        w.slab = off; off += w.ns * 2 * d * d;
        w.bpart = off; off += w.ns * 2 * d;
        w.part = off; off += w.nwg * 3 * d;
    }
    w.total = off;
    return w;
}

extern "C" long bsarec_lru_weight_floats(const bsarec_lru_config_t* cfg) {
    if (lru_check(cfg)) return -10;
    return lru_weights(*cfg).total;
}

extern "C" long bsarec_lru_workspace_bytes(const bsarec_lru_config_t* cfg, int train) {
    if (lru_check(cfg)) return -10;
    return lru_ws(*cfg, train != 0).total * (long)sizeof(float);
}

extern "C" int bsarec_lru_fwd(const bsarec_lru_config_t* cfg, const float* x, const int64_t* ids, const float* weights, int train,
                              float* y, void* workspace, long workspace_bytes, void* stream) {
    RET(lru_check(cfg));
    RET(ptrs_check({x, weights, y, workspace}));
    if (workspace_bytes < lru_ws(*cfg, train != 0).total * (long)sizeof(float)) return -10;
    const bsarec_lru_config_t& c = *cfg;
    const int B = c.batch, L = c.seq_len, d = c.width;
    const long T = (long)B * L;
    const LruWs ws = lru_ws(c, train != 0);
    const LruW wo = lru_weights(c);
    float* w = (float*)workspace;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(lru_lambda_kernel, dim3(cdiv(d, 256)), dim3(256), 0, s, weights, w + ws.lam, d);
    RET(dense_nt(x, weights + wo.win, (int)T, 2 * d, d, dense_epi(w + ws.v, 2 * d, weights + wo.bin), s));
    LruFwdP P;
    P.V = w + ws.v; P.H = w + ws.h; P.ids = ids; P.lam = w + ws.lam; P.B = B; P.L = L; P.d = d; P.save_v = train != 0;
    hipLaunchKernelGGL(lru_scan_fwd_kernel, dim3(ws.nwg), dim3(LRU_THREADS), 0, s, P);
    RET(dense_nt(w + ws.h, weights + wo.wout, (int)T, d, 2 * d, dense_epi(y, d, weights + wo.bout), s));
    return (int)hipGetLastError();
}

extern "C" int bsarec_lru_bwd(const bsarec_lru_config_t* cfg, const float* x, const int64_t* ids, const float* weights, const float* dy,
                              void* workspace, long workspace_bytes, float* dx, float* dweights, void* stream) {
    RET(lru_check(cfg));
    RET(ptrs_check({x, weights, dy, workspace, dx, dweights}));
    if (workspace_bytes < lru_ws(*cfg, true).total * (long)sizeof(float)) return -10;
    const bsarec_lru_config_t& c = *cfg;
    const int B = c.batch, L = c.seq_len, d = c.width;
    const long T = (long)B * L;
    const LruWs ws = lru_ws(c, true);
    const LruW wo = lru_weights(c);
    float* w = (float*)workspace;
    hipStream_t s = (hipStream_t)stream;
    float* slab = w + ws.slab;
    hipLaunchKernelGGL(lru_lambda_kernel, dim3(cdiv(d, 256)), dim3(256), 0, s, weights, w + ws.lam, d);
    // g = dy . W_out;  dW_out = dy^T . [Re h | Im h], db_out = its column sums
    RET(linear_bwd(dy, w + ws.h, weights + wo.wout, T, d, 2 * d, dense_epi(w + ws.g, 2 * d), slab, w + ws.bpart,
                   dweights + wo.wout, dweights + wo.bout, s));
    LruBwdP P;
    P.G = w + ws.g; P.V = w + ws.v; P.H = w + ws.h; P.ids = ids; P.lam = w + ws.lam; P.part = w + ws.part; P.B = B; P.L = L; P.d = d;
    hipLaunchKernelGGL(lru_scan_bwd_kernel, dim3(ws.nwg), dim3(LRU_THREADS), 0, s, P);
    hipLaunchKernelGGL(lru_param_grad_kernel, dim3(d / 4), dim3(256), 0, s, w + ws.part, ws.nwg, weights, w + ws.lam, d, dweights);
    // dx = du . W_in;  dW_in = du^T . x, db_in = its column sums
    RET(linear_bwd(w + ws.g, x, weights + wo.win, T, 2 * d, d, dense_epi(dx, d), slab, w + ws.bpart, dweights + wo.win,
                   dweights + wo.bin, s));
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Selective state-space layer (mamba.h): plan-less, one linear chain on the caller's stream, no allocation
// ---------------------------------------------------------------------------------------------
static int mamba_check(const bsarec_mamba_config_t* c) {
    if (!c) return -10;
    if (!seq_shape_ok(c->batch, c->seq_len, 1)) return -10;
    if (!row_dim_ok(c->width)) return -10;
    if (c->expand < 1 || c->expand > 2) return -10;
    if (c->d_state != 4 && c->d_state != 8 && c->d_state != 16 && c->d_state != 32) return -10;
    if (c->d_conv < 2 || c->d_conv > 4) return -10;
    if (c->dt_rank < 4 || c->dt_rank > 64 || c->dt_rank % 4) return -10;
    return 0;
}

// offsets (floats) into the flat weight array: in_proj.weight [2 di][d] | conv1d.weight [di][K] | conv1d.bias [di] |
// x_proj.weight [R + 2N][di] | dt_proj.weight [di][R] | dt_proj.bias [di] | A_log [di][N] | D [di] | out_proj.weight [d][di]
struct MambaW { long win, wconv, bconv, wx, wdt, bdt, alog, dd, wout, total; };
static MambaW mamba_weights(const bsarec_mamba_config_t& c) {
    const long d = c.width, di = d * c.expand, N = c.d_state, K = c.d_conv, R = c.dt_rank;
    MambaW w;
    w.win = 0; w.wconv = w.win + 2 * di * d; w.bconv = w.wconv + di * K; w.wx = w.bconv + di; w.wdt = w.wx + (R + 2 * N) * di;
    w.bdt = w.wdt + di * R; w.alog = w.bdt + di; w.dd = w.alog + di * N; w.wout = w.dd + di; w.total = w.wout + d * di;
    return w;
}

// Workspace, in floats (every region a multiple of 4), T = B L: xz [T][2 di] | u [T][di] | delta [T][R] | bc [T][2N] |
// dt [T][di] | y [T][di] | c [T][di] | s [T][di] | checkpoints [B][nck][di][N] | dy, du_scan, du_proj, ddt [T][di] each |
// dxz [T][2 di] | dxdbl [T][R + 2N] | dB dC partials [slices][T][2N] | dA_log dD partials [G][di N + di] |
// convolution partials [conv workgroups][di K + di] | slabs [ns][largest weight] | bias partials [ns][di]; everything behind y
// in training only
struct MambaWs {
    long xz, u, delta, bc, dt, y, c, s, hck, dy, du1, du2, ddt, dxz, dxdbl, bcp, adp, cvp, slab, bpart, total, slab_floats;
    int ns, nck, nslice, groups, conv_rows, conv_wgs;
};
static MambaWs mamba_ws(const bsarec_mamba_config_t& c, bool train) {
    const long T = (long)c.batch * c.seq_len, d = c.width, di = d * c.expand, N = c.d_state, K = c.d_conv, R = c.dt_rank;
    MambaWs w;
    memset(&w, 0, sizeof(w));
    int kc;
    split_k(T, &w.ns, &kc);
    w.nck = cdiv(c.seq_len, MAMBA_CK) - 1;
    w.nslice = cdiv((int)di, MAMBA_THREADS / (int)N);
    w.groups = c.batch < 1024 ? c.batch : 1024;
    w.conv_rows = cdiv(T, 1024L);                     // at most 1024 partial rows
    w.conv_wgs = (int)cdiv(T, (long)w.conv_rows);
    long off = 0;
    w.xz = off; off += T * 2 * di;
    w.u = off; off += T * di;
    w.delta = off; off += T * R;
    w.bc = off; off += T * 2 * N;
    w.dt = off; off += T * di;
    w.y = off; off += T * di;
    if (train) {
        w.c = off; off += T * di;
        w.s = off; off += T * di;
        w.hck = off; off += (long)c.batch * w.nck * di * N;
        w.dy = off; off += T * di;
        w.du1 = off; off += T * di;
        w.du2 = off; off += T * di;
        w.ddt = off; off += T * di;
        w.dxz = off; off += T * 2 * di;
        w.dxdbl = off; off += T * (R + 2 * N);
        w.bcp = off; off += w.nslice * T * 2 * N;
        w.adp = off; off += w.groups * (di * N + di);
        w.cvp = off; off += w.conv_wgs * (di * K + di);
        w.slab_floats = 2 * di * d;
        if ((R + 2 * N) * di > w.slab_floats) w.slab_floats = (R + 2 * N) * di;
        w.slab = off; off += w.ns * w.slab_floats;
        w.bpart = off; off += w.ns * di;
    }
    w.total = off;
    return w;
}

extern "C" long bsarec_mamba_weight_floats(const bsarec_mamba_config_t* cfg) {
    if (mamba_check(cfg)) return -10;
    return mamba_weights(*cfg).total;
}

extern "C" long bsarec_mamba_workspace_bytes(const bsarec_mamba_config_t* cfg, int train) {
    if (mamba_check(cfg)) return -10;
    return mamba_ws(*cfg, train != 0).total * (long)sizeof(float);
}

struct MambaSpan { const void* p; long bytes; };
// whether one of the first `nout` spans (the outputs) overlaps any other span
static bool spans_overlap(const MambaSpan* spans, int n, int nout) {
    for (int i = 0; i < nout; ++i)
        for (int k = 0; k < n; ++k) {
            const uintptr_t a0 = (uintptr_t)spans[i].p, b0 = (uintptr_t)spans[k].p;
            if (k != i && a0 < b0 + (uintptr_t)spans[k].bytes && b0 < a0 + (uintptr_t)spans[i].bytes) return true;
        }
    return false;
}

#define MAMBA_DISPATCH(N, KERNEL, ...) \
    switch (N) { \
        case 4: hipLaunchKernelGGL(KERNEL<4>, __VA_ARGS__); break; \
        case 8: hipLaunchKernelGGL(KERNEL<8>, __VA_ARGS__); break; \
        case 16: hipLaunchKernelGGL(KERNEL<16>, __VA_ARGS__); break; \
        default: hipLaunchKernelGGL(KERNEL<32>, __VA_ARGS__); break; \
    }

extern "C" int bsarec_mamba_fwd(const bsarec_mamba_config_t* cfg, const float* x, const int64_t* ids, const float* weights, int train,
                                float* out, void* workspace, long workspace_bytes, void* stream) {
    RET(mamba_check(cfg));
    const bsarec_mamba_config_t& c = *cfg;
    const int B = c.batch, L = c.seq_len, d = c.width, di = d * c.expand, N = c.d_state, K = c.d_conv, R = c.dt_rank;
    const long T = (long)B * L, fb = sizeof(float);
    const MambaW wo = mamba_weights(c);
    const MambaSpan spans[] = {{out, T * d * fb}, {workspace, workspace_bytes}, {x, T * d * fb}, {weights, wo.total * fb}};
    const MambaWs ws = mamba_ws(c, train != 0);
    RET(ptrs_check({out, workspace, x, weights}));
    if (workspace_bytes < ws.total * fb || spans_overlap(spans, 4, 2)) return -10;
    float* w = (float*)workspace;
    hipStream_t s = (hipStream_t)stream;
    RET(dense_nt(x, weights + wo.win, (int)T, 2 * di, d, dense_epi(w + ws.xz, 2 * di), s));
    MambaConvP C;
    memset(&C, 0, sizeof(C));
    C.XZ = w + ws.xz; C.ids = ids; C.W = weights + wo.wconv; C.C = train ? w + ws.c : nullptr; C.U = w + ws.u;
    C.T = T; C.L = L; C.di = di; C.K = K;
    hipLaunchKernelGGL(mamba_conv_fwd_kernel, dim3((unsigned)cdiv(T * (di / 4), 256L)), dim3(256), 0, s, C);
    RET(dense_nt(w + ws.u, weights + wo.wx, (int)T, R, di, dense_epi(w + ws.delta, R), s));
    RET(dense_nt(w + ws.u, weights + wo.wx + (long)R * di, (int)T, 2 * N, di, dense_epi(w + ws.bc, 2 * N), s));
    RET(dense_nt(w + ws.delta, weights + wo.wdt, (int)T, di, R, dense_epi(w + ws.dt, di, weights + wo.bdt), s));
    MambaScanP P;
    memset(&P, 0, sizeof(P));
    P.XZ = w + ws.xz; P.U = w + ws.u; P.DTR = w + ws.dt; P.BC = w + ws.bc; P.Alog = weights + wo.alog; P.D = weights + wo.dd;
    P.ids = ids; P.Y = w + ws.y; P.S = train ? w + ws.s : nullptr; P.HCK = train && ws.nck > 0 ? w + ws.hck : nullptr;
    P.B = B; P.L = L; P.di = di; P.nck = ws.nck;
    MAMBA_DISPATCH(N, mamba_scan_fwd_kernel, dim3(B, ws.nslice), dim3(MAMBA_THREADS), 0, s, P);
    RET(dense_nt(w + ws.y, weights + wo.wout, (int)T, d, di, dense_epi(out, d), s));
    return (int)hipGetLastError();
}

extern "C" int bsarec_mamba_bwd(const bsarec_mamba_config_t* cfg, const float* x, const int64_t* ids, const float* weights,
                                const float* dout, void* workspace, long workspace_bytes, float* dx, float* dweights, void* stream) {
    RET(mamba_check(cfg));
    const bsarec_mamba_config_t& c = *cfg;
    const int B = c.batch, L = c.seq_len, d = c.width, di = d * c.expand, N = c.d_state, K = c.d_conv, R = c.dt_rank, X = R + 2 * N;
    const long T = (long)B * L, fb = sizeof(float);
    const MambaW wo = mamba_weights(c);
    const MambaSpan spans[] = {{dx, T * d * fb}, {dweights, wo.total * fb}, {workspace, workspace_bytes}, {x, T * d * fb},
                               {weights, wo.total * fb}, {dout, T * d * fb}};
    const MambaWs ws = mamba_ws(c, true);
    RET(ptrs_check({dx, dweights, workspace, x, weights, dout}));
    if (workspace_bytes < ws.total * fb || spans_overlap(spans, 6, 3)) return -10;
    float* w = (float*)workspace;
    hipStream_t s = (hipStream_t)stream;
    float* slab = w + ws.slab;
    // dy = dout . W_out;  dW_out = dout^T . y
    RET(linear_bwd(dout, w + ws.y, weights + wo.wout, T, d, di, dense_epi(w + ws.dy, di), slab, nullptr, dweights + wo.wout,
                   nullptr, s));
    MambaScanP P;
    memset(&P, 0, sizeof(P));
    P.XZ = w + ws.xz; P.U = w + ws.u; P.DTR = w + ws.dt; P.BC = w + ws.bc; P.Alog = weights + wo.alog; P.D = weights + wo.dd;
    P.ids = ids; P.S = w + ws.s; P.HCK = w + ws.hck; P.DY = w + ws.dy; P.DU = w + ws.du1; P.DDT = w + ws.ddt; P.DXZ = w + ws.dxz;
    P.BCP = w + ws.bcp; P.ADP = w + ws.adp; P.B = B; P.L = L; P.di = di; P.nck = ws.nck;
    MAMBA_DISPATCH(N, mamba_scan_bwd_kernel, dim3(ws.groups, ws.nslice), dim3(MAMBA_THREADS), 0, s, P);
    hipLaunchKernelGGL(mamba_rows_sum_kernel, dim3((di * N + di) / 4), dim3(256), 0, s, w + ws.adp, ws.groups, (long)di * N + di,
                       dweights + wo.alog);
    // dxdbl = [ddt . W_dt | dB | dC];  dW_dt = ddt^T . delta, db_dt = its column sums
    // (dB | dC land in columns R .. X, the product in columns < R: the two writers of dxdbl do not meet)
    hipLaunchKernelGGL(mamba_bc_sum_kernel, dim3((unsigned)cdiv(T * (2 * N / 4), 256L)), dim3(256), 0, s, w + ws.bcp, ws.nslice, T,
                       2 * N, w + ws.dxdbl, X, R);
    RET(linear_bwd(w + ws.ddt, w + ws.delta, weights + wo.wdt, T, di, R, dense_epi(w + ws.dxdbl, X), slab, w + ws.bpart,
                   dweights + wo.wdt, dweights + wo.bdt, s));
    // du_proj = dxdbl . W_x;  dW_x = dxdbl^T . u
    RET(linear_bwd(w + ws.dxdbl, w + ws.u, weights + wo.wx, T, X, di, dense_epi(w + ws.du2, di), slab, nullptr, dweights + wo.wx,
                   nullptr, s));
    MambaConvP C;
    memset(&C, 0, sizeof(C));
    C.XZ = w + ws.xz; C.ids = ids; C.W = weights + wo.wconv; C.C = w + ws.c; C.DU1 = w + ws.du1; C.DU2 = w + ws.du2;
    C.DXZ = w + ws.dxz; C.part = w + ws.cvp; C.T = T; C.L = L; C.di = di; C.K = K; C.rows = ws.conv_rows;
    hipLaunchKernelGGL(mamba_conv_bwd_kernel, dim3(ws.conv_wgs), dim3(256), 0, s, C);
    hipLaunchKernelGGL(mamba_rows_sum_kernel, dim3((di * K + di) / 4), dim3(256), 0, s, w + ws.cvp, ws.conv_wgs, (long)di * K + di,
                       dweights + wo.wconv);
    // dx = dxz . W_in;  dW_in = dxz^T . x
    RET(linear_bwd(w + ws.dxz, x, weights + wo.win, T, 2 * di, d, dense_epi(dx, d), slab, nullptr, dweights + wo.win, nullptr, s));
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// The shell of a pairwise step (pair_step.h), once for the GRU4Rec, Caser and personalised Caser steps: a driver fills one
// PairStep and calls pair_begin_embed, pair_bpr (or its own head), pair_item_grad and pair_flush_tick around its encoder's
// launches.  Behind them the argument checks that the entry points of the three steps share.
// ---------------------------------------------------------------------------------------------
// dropout site 0 of a step (GRU4Rec: the token rows; Caser: z in front of fc1); train = false: no mask, whatever p
static DropP site0_drop(float p, const void* state, bool train) {
    DropP d;
    d.thresh = train ? drop_thresh(p) : 0;
    d.scale = (train && p > 0.f) ? (float)(1.0 / (1.0 - (double)p)) : 1.0f;
    d.rng = (const uint64_t*)state; d.site = 0;
    return d;
}

struct PairStep {
    int B, d, V; long T;                                 // rows, width, items, tokens
    const float* E; const int64_t* ids; const int64_t* answers; const int64_t* neg_answers;
    void* state; int train;
    DropP drop;                                          // of the token rows
    float* x; float* dx; float* c; float* rows;          // workspace: [T][d], [T][d], [B], the loss rows [B]
    unsigned long long* acc;                             // workspace: the fixed-point accumulator [V][d]
    float* dE; float* loss_out;
    const bsarec_adam_t* tick_adam;                      // null, or the Adam whose t the closing block advances (a *_train_step)
    hipStream_t s;
};

// a training step moves the step counter first; then x = E[ids] (times the mask), and the same launch clears the accumulator
static void pair_begin_embed(const PairStep& p) {
    if (p.train) hipLaunchKernelGGL(step_begin_kernel, dim3(1), dim3(1), 0, p.s, (uint64_t*)p.state, (long long*)nullptr, 0);
    PairEmbedP pe;
    pe.E = p.E; pe.ids = p.ids; pe.x = p.x; pe.T = p.T; pe.d = p.d; pe.V = p.V; pe.drop = p.drop;
    pe.acc = p.acc; pe.acc_n2 = (long)p.V * p.d / 2;
    DISPATCH_LPR(p.d, hipLaunchKernelGGL(pair_embed_kernel<LPR>, dim3(std::min(cdiv(p.T, ROW_THREADS / LPR), 4096)),
                                         dim3(ROW_THREADS), 0, p.s, pe));
}

// the BPR rows on the encoder's state sv [B][d]: ds [B][d], c and the loss rows are written
static void pair_bpr(const PairStep& p, const float* sv, float* ds) {
    PairBprP pb;
    pb.s = sv; pb.E = p.E; pb.ans = p.answers; pb.neg = p.neg_answers; pb.B = p.B; pb.d = p.d; pb.V = p.V;
    pb.ds = ds; pb.c = p.c; pb.loss_rows = p.rows;
    DISPATCH_LPR(p.d, hipLaunchKernelGGL(pair_bpr_kernel<LPR>, dim3(cdiv(p.B, ROW_THREADS / LPR)), dim3(ROW_THREADS), 0, p.s, pb));
}

// dE's rows into the accumulator: the T token rows, then the head's -- 2 B pairwise rows with head_rows = the sv of pair_bpr
// (C = 0), or C candidate rows with head_rows = the dEc [C][d] of g4c_launch
static void pair_item_grad(const PairStep& p, const float* head_rows, int C = 0) {
    PairGradP pg;
    pg.dx = p.dx; pg.ids = p.ids; pg.ans = p.answers; pg.neg = p.neg_answers;
    pg.T = p.T; pg.B = p.B; pg.C = C; pg.d = p.d; pg.V = p.V; pg.drop = p.drop; pg.dA = p.acc;
    pg.head_rows = head_rows; pg.c = p.c;
    const long n_head = C ? C : 2L * p.B;
    DISPATCH_LPR(p.d, {
        const dim3 grid(cdiv(p.T + n_head, SCATTER_FLOATS / (4 * LPR)));
        if (C) hipLaunchKernelGGL(g4c_item_grad_kernel<LPR>, grid, dim3(ROW_THREADS), 0, p.s, pg);
        else hipLaunchKernelGGL(pair_item_grad_kernel<LPR>, grid, dim3(ROW_THREADS), 0, p.s, pg);
    });
}

// the flush of a table's accumulator [n] into every float of dst
static LookupAcc pair_flush_acc(unsigned long long* acc, float* dst, long n) {
    LookupAcc la;
    memset(&la, 0, sizeof(la));
    la.acc = acc; la.dst = dst; la.n4 = n / 4; la.dense_zero = 1;
    la.nblocks = std::min(cdiv(la.n4, ROW_THREADS), 1024);
    return la;
}

// accumulator -> dE, and the one closing block of the step: the mean loss and, with tick_adam, Adam's t
static int pair_flush_tick(const PairStep& p) {
    const LookupAcc la = pair_flush_acc(p.acc, p.dE, (long)p.V * p.d);
    const bsarec_adam_t* a = p.tick_adam;
    const TickP tk = a ? make_tick(p.state, 1, a->lr, a->beta1, a->beta2, p.rows, p.B, p.loss_out, nullptr, 0, 0)
                       : make_tick(p.state, 0, 0.f, 0.f, 0.f, p.rows, p.B, p.loss_out, nullptr, 0, 0);
    hipLaunchKernelGGL(pair_flush_kernel, dim3(la.nblocks + 1), dim3(ROW_THREADS), 0, p.s, la, tk);
    return (int)hipGetLastError();
}

// an Adam of a step: fp32 arrays only, one gradient source, 16-byte aligned, n floats
struct StepAdam { const bsarec_adam_t* a; long n; };
static int pair_adam_check(const bsarec_adam_t* a, long n) {
    RET(adam_check(a));
    if (a->n != n) return -10;
    if (a->shadow_bf16 || a->grads2 || a->grads2_n || a->n_grad_srcs || a->wimage_plan) return -10;
    for (const void* p : {(const void*)a->params, (const void*)a->grads, (const void*)a->exp_avg, (const void*)a->exp_avg_sq})
        if (!aligned_to(p, 16)) return -10;
    return 0;
}
// every Adam of a *_train_step: one t and one pair of bias corrections in `state` serve them all, so lr and the betas are
// the first's
template <int N>
static int pair_adams_check(const StepAdam (&adams)[N]) {
    for (const StepAdam& x : adams) RET(pair_adam_check(x.a, x.n));
    const bsarec_adam_t* a0 = adams[0].a;
    for (const StepAdam& x : adams)
        if (x.a->lr != a0->lr || x.a->beta1 != a0->beta1 || x.a->beta2 != a0->beta2) return -10;
    return 0;
}
template <int N>
static int pair_adams_launch(const StepAdam (&adams)[N], void* state, hipStream_t s) {
    for (const StepAdam& x : adams) RET(adam_launch(*x.a, state, s));
    return 0;
}
static float* adam_grads(const bsarec_adam_t* a) { return const_cast<float*>(a->grads); }

// ---------------------------------------------------------------------------------------------
// GRU4Rec training step: lookup + dropout, the GRU stack, the BPR head, every gradient, Adam -- plan-less, one linear chain of
// launches on the caller's stream, no allocation, no host synchronisation
// ---------------------------------------------------------------------------------------------
static int gru4rec_check(const bsarec_gru4rec_config_t* c) {
    if (!c) return -10;
    RET(gru_check(&c->gru));
    if (c->gru.input_size != c->gru.out_size) return -10;
    if (c->item_size < 2) return -10;
    if (!dropout_ok(c->dropout)) return -10;
    return 0;
}

// Workspace, in floats (every region a multiple of 4): the GRU workspace of train = 1 | x [T][d] | s [B][d] | ds [B][d] |
// dx [T][d] | c [B up to 4] | loss rows [B up to 4] | the fixed-point accumulator [V][d] of 64-bit words
struct Gru4RecWs { long gru, x, s, ds, dx, c, rows, acc, total; long gru_bytes; };
static Gru4RecWs gru4rec_ws(const bsarec_gru4rec_config_t& c) {
    const long B = c.gru.batch, T = B * c.gru.seq_len, d = c.gru.input_size;
    Gru4RecWs w;
    long off = 0;
    w.gru = off; off += gru_ws(c.gru, true).total;
    w.gru_bytes = off * (long)sizeof(float);
    w.x = off; off += T * d;
    w.s = off; off += B * d;
    w.ds = off; off += B * d;
    w.dx = off; off += T * d;
    w.c = off; off += rup(B, 4);
    w.rows = off; off += rup(B, 4);
    w.acc = off; off += 2L * c.item_size * d;
    w.total = off;
    return w;
}

extern "C" long bsarec_gru4rec_workspace_bytes(const bsarec_gru4rec_config_t* cfg) {
    if (gru4rec_check(cfg)) return -10;
    return gru4rec_ws(*cfg).total * (long)sizeof(float);
}

// The heads over candidates shared by the batch (gru4rec_cand.h; bsarec_gru4rec_cand_*): in a step, scores, rows, backward (and
// slab sum) stand where the BPR rows do, and the item-table gradient runs over T + C rows
static int g4c_head_check(const bsarec_gru4rec_head_t* h, long B) {
    if (!h) return -10;
    if (h->loss < G4C_CE || h->loss > G4C_BPR_MAX || h->candidates < 1 || h->candidates > 2) return -10;
    if (!(h->bpreg >= 0.f)) return -10;                                 // NaN fails the comparison
    if (B < 1 || B * h->candidates > G4C_MAX) return -10;
    return 0;
}

// The head's own regions, in floats from `off` (every one a multiple of 4): R / G [B][C] | slabs of dEc [nslab][C][d] | slabs of
// ds [nslab][B][d] (both empty when nslab is 1).  A slab of dEc sums chunkB rows, one of ds chunkC candidates.  The products are
// bound by the latency of their 16-deep k-slices (about 3 us each, measured), not by their flops, so the summed dimension is cut
// short: nslab = min(16, ceil(C / 64)), i.e. at least 64 candidates per slab of ds, lowered while the slabs would pass 2^26 floats.
struct G4cWs { long R, slabE, slabS, end; int C, nslab, chunkB, chunkC; };
static G4cWs g4c_ws(long B, int candidates, long d, long off) {
    G4cWs w;
    w.C = (int)(B * candidates);
    w.nslab = std::min(16, cdiv(w.C, SSM_TILE));
    while (w.nslab > 1 && w.nslab * (B + w.C) * d > (1L << 26)) --w.nslab;
    w.chunkB = (int)rup(cdiv(B, w.nslab), SSM_KS);
    w.chunkC = (int)rup(cdiv(w.C, w.nslab), SSM_TILE);
    w.R = off; off += rup(B * w.C, 4);
    w.slabE = off; off += w.nslab > 1 ? w.nslab * (long)w.C * d : 0;
    w.slabS = off; off += w.nslab > 1 ? w.nslab * B * d : 0;
    w.end = off;
    return w;
}

// scores, rows, backward (+ slab sum): loss_rows [B], ds [B][d] and dEc [C][d] are written
static void g4c_launch(const G4cWs& g, float* w, const float* sv, const float* E, const int64_t* answers, const int64_t* neg_answers,
                       int B, int d, int V, const bsarec_gru4rec_head_t& head, float* loss_rows, float* ds, float* dEc,
                       hipStream_t s) {
    Gru4RecCandP P;
    memset(&P, 0, sizeof(P));
    P.s = sv; P.E = E; P.ans = answers; P.neg = neg_answers; P.B = B; P.C = g.C; P.d = d; P.V = V; P.loss = head.loss;
    P.bpreg = head.bpreg; P.R = w + g.R; P.loss_rows = loss_rows;
    P.nslab = g.nslab; P.chunkB = g.chunkB; P.chunkC = g.chunkC;
    const bool direct = g.nslab == 1;
    P.outE = direct ? dEc : w + g.slabE; P.strideE = (long)g.C * d;
    P.outS = direct ? ds : w + g.slabS; P.strideS = (long)B * d;
    const int dt = cdiv(d, SSM_TILE), ct = cdiv(g.C, SSM_TILE), rt = cdiv(B, SSM_TILE);
    P.tilesA = ct * dt * g.nslab;
    hipLaunchKernelGGL(g4c_scores_kernel, dim3(ct, rt), dim3(ROW_THREADS), 0, s, P);
    hipLaunchKernelGGL(g4c_rows_kernel, dim3(B), dim3(ROW_THREADS), 0, s, P);
    hipLaunchKernelGGL(g4c_bwd_kernel, dim3(P.tilesA + rt * dt * g.nslab), dim3(ROW_THREADS), 0, s, P);
    if (!direct) {
        const long nE4 = (long)g.C * d / 4, nS4 = (long)B * d / 4;
        hipLaunchKernelGGL(g4c_slab_sum_kernel, dim3(cdiv(nE4 + nS4, ROW_THREADS)), dim3(ROW_THREADS), 0, s, w + g.slabE,
                           w + g.slabS, g.nslab, nE4, nS4, dEc, ds);
    }
}

// a candidate step's workspace: the step's (gru4rec_ws; its c region is not used), then the head's regions, then dEc [C][d]
static G4cWs g4c_step_ws(const bsarec_gru4rec_config_t& c, const bsarec_gru4rec_head_t& h, long* dEc, long* total) {
    const G4cWs g = g4c_ws(c.gru.batch, h.candidates, c.gru.input_size, gru4rec_ws(c).total);
    *dEc = g.end;
    *total = g.end + (long)g.C * c.gru.input_size;
    return g;
}

// tick_adam: null, or the Adam whose t the step's closing block advances (bsarec_gru4rec_train_step); head: null (the BPR rows
// against one negative per row), or the head over shared candidates
static int gru4rec_run(const bsarec_gru4rec_config_t& c, const float* E, const float* weights, const int64_t* ids,
                       const int64_t* answers, const int64_t* neg_answers, void* state, int train, float* loss_out, float* dE,
                       float* dweights, void* workspace, const bsarec_adam_t* tick_adam, const bsarec_gru4rec_head_t* head,
                       hipStream_t s) {
    const int B = c.gru.batch, d = c.gru.input_size;
    const Gru4RecWs ws = gru4rec_ws(c);
    float* w = (float*)workspace;
    const PairStep p = {B, d, c.item_size, (long)B * c.gru.seq_len, E, ids, answers, neg_answers, state, train,
                        site0_drop(c.dropout, state, train != 0), w + ws.x, w + ws.dx, w + ws.c, w + ws.rows,
                        reinterpret_cast<unsigned long long*>(w + ws.acc), dE, loss_out, tick_adam, s};
    pair_begin_embed(p);
    RET(bsarec_gru_fwd(&c.gru, p.x, weights, 1, 1, w + ws.s, w + ws.gru, ws.gru_bytes, s));
    long dEc = 0, total = 0;
    G4cWs g = {};
    if (head) {
        g = g4c_step_ws(c, *head, &dEc, &total);
        g4c_launch(g, w, w + ws.s, E, answers, neg_answers, B, d, p.V, *head, p.rows, w + ws.ds, w + dEc, s);
    } else {
        pair_bpr(p, w + ws.s, w + ws.ds);
    }
    RET(bsarec_gru_bwd(&c.gru, p.x, weights, 1, w + ws.ds, w + ws.gru, ws.gru_bytes, p.dx, dweights, s));
    pair_item_grad(p, head ? w + dEc : w + ws.s, g.C);
    return pair_flush_tick(p);
}

extern "C" long bsarec_gru4rec_cand_workspace_bytes(const bsarec_gru4rec_config_t* cfg, const bsarec_gru4rec_head_t* head) {
    if (gru4rec_check(cfg) || g4c_head_check(head, cfg->gru.batch)) return -10;
    long dEc, total;
    g4c_step_ws(*cfg, *head, &dEc, &total);
    return total * (long)sizeof(float);
}

// head: null, or checked here with the larger workspace it needs
static int gru4rec_loss_grad(const bsarec_gru4rec_config_t* cfg, const float* item_emb, const float* weights, const int64_t* ids,
                             const int64_t* answers, const int64_t* neg_answers, void* state, int train, float* loss_out,
                             float* d_item_emb, float* dweights, void* workspace, long workspace_bytes,
                             const bsarec_adam_t* tick_adam, const bsarec_gru4rec_head_t* head, hipStream_t s) {
    RET(gru4rec_check(cfg));
    RET(ptrs_check({item_emb, weights, d_item_emb, dweights, workspace}, {ids, answers, neg_answers, state}, {loss_out}));
    if (workspace_bytes < gru4rec_ws(*cfg).total * (long)sizeof(float)) return -10;
    if (head) {
        RET(g4c_head_check(head, cfg->gru.batch));
        if (workspace_bytes < bsarec_gru4rec_cand_workspace_bytes(cfg, head)) return -10;
    }
    return gru4rec_run(*cfg, item_emb, weights, ids, answers, neg_answers, state, train, loss_out, d_item_emb, dweights, workspace,
                       tick_adam, head, s);
}

extern "C" int bsarec_gru4rec_loss_grad(const bsarec_gru4rec_config_t* cfg, const float* item_emb, const float* weights,
                                        const int64_t* ids, const int64_t* answers, const int64_t* neg_answers, void* state,
                                        int train, float* loss_out, float* d_item_emb, float* dweights, void* workspace,
                                        long workspace_bytes, void* stream) {
    return gru4rec_loss_grad(cfg, item_emb, weights, ids, answers, neg_answers, state, train, loss_out, d_item_emb, dweights,
                             workspace, workspace_bytes, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int bsarec_gru4rec_cand_loss_grad(const bsarec_gru4rec_config_t* cfg, const float* item_emb, const float* weights,
                                             const int64_t* ids, const int64_t* answers, const int64_t* neg_answers, void* state,
                                             int train, float* loss_out, float* d_item_emb, float* dweights, void* workspace,
                                             long workspace_bytes, void* stream, const bsarec_gru4rec_head_t* head) {
    if (!head) return -10;
    return gru4rec_loss_grad(cfg, item_emb, weights, ids, answers, neg_answers, state, train, loss_out, d_item_emb, dweights,
                             workspace, workspace_bytes, nullptr, head, (hipStream_t)stream);
}

static int gru4rec_train_step(const bsarec_gru4rec_config_t* cfg, const int64_t* ids, const int64_t* answers,
                              const int64_t* neg_answers, const bsarec_adam_t* adam_items, const bsarec_adam_t* adam_weights,
                              void* state, float* loss_out, void* workspace, long workspace_bytes,
                              const bsarec_gru4rec_head_t* head, void* stream) {
    RET(gru4rec_check(cfg));
    const StepAdam adams[] = {{adam_items, (long)cfg->item_size * cfg->gru.input_size},
                              {adam_weights, gru_weights(cfg->gru).total}};
    RET(pair_adams_check(adams));
    hipStream_t s = (hipStream_t)stream;
    RET(gru4rec_loss_grad(cfg, adam_items->params, adam_weights->params, ids, answers, neg_answers, state, 1, loss_out,
                          adam_grads(adam_items), adam_grads(adam_weights), workspace, workspace_bytes, adam_items, head, s));
    return pair_adams_launch(adams, state, s);
}

extern "C" int bsarec_gru4rec_train_step(const bsarec_gru4rec_config_t* cfg, const int64_t* ids, const int64_t* answers,
                                         const int64_t* neg_answers, const bsarec_adam_t* adam_items,
                                         const bsarec_adam_t* adam_weights, void* state, float* loss_out, void* workspace,
                                         long workspace_bytes, void* stream) {
    return gru4rec_train_step(cfg, ids, answers, neg_answers, adam_items, adam_weights, state, loss_out, workspace, workspace_bytes,
                              nullptr, stream);
}

extern "C" int bsarec_gru4rec_cand_train_step(const bsarec_gru4rec_config_t* cfg, const int64_t* ids, const int64_t* answers,
                                              const int64_t* neg_answers, const bsarec_adam_t* adam_items,
                                              const bsarec_adam_t* adam_weights, void* state, float* loss_out, void* workspace,
                                              long workspace_bytes, void* stream, const bsarec_gru4rec_head_t* head) {
    if (!head) return -10;
    return gru4rec_train_step(cfg, ids, answers, neg_answers, adam_items, adam_weights, state, loss_out, workspace, workspace_bytes,
                              head, stream);
}

// ---------------------------------------------------------------------------------------------
// Block-model training step (lrurec_step.h), once for LRURec and Mamba4Rec: lookup + LayerNorm + dropout, N blocks of a sequence
// layer and a feed-forward net, the CE head at position L - 1, every gradient, Adam -- plan-less, one linear chain of launches on
// the caller's stream, no allocation, no host synchronisation.  The layer is a description (LrrLayer): its weight and train
// workspace floats and its two calls.  Launches: 11 + N (21 + the layer's forward and backward) for a loss and its gradients
// (one more when train != 0: the step counter), and two Adam launches behind them in a training step.
// ---------------------------------------------------------------------------------------------
// the layer inside a block: z = fwd(x, ids, w) with train = 1, and its true derivative reading what fwd left in ws
struct LrrLayer {
    const void* cfg;
    long weights, ws;                                       // floats of a block's weight array / of the train = 1 workspace
    int (*fwd)(const void* cfg, const float* x, const int64_t* ids, const float* w, float* z, void* ws, long ws_bytes, hipStream_t s);
    int (*bwd)(const void* cfg, const float* x, const int64_t* ids, const float* w, const float* dz, void* ws, long ws_bytes,
               float* dx, float* dw, hipStream_t s);
};
// a checked step: the shape, and the layer
struct LrrStep { int B, L, d, layers, item_size; float dropout, ln_eps; LrrLayer layer; };

// what the two steps' configs share behind their layer's own check
static int lrr_check(int layers, int item_size, float dropout, float ln_eps) {
    if (layers < 1 || layers > BSAREC_MAX_LAYERS) return -10;
    if (item_size < 2) return -10;
    if (!dropout_ok(dropout)) return -10;
    if (!(ln_eps > 0.f)) return -10;                                    // NaN fails it
    return 0;
}

static int lrurec_step(const bsarec_lrurec_config_t* c, LrrStep* st) {
    if (!c) return -10;
    RET(lru_check(&c->lru));
    RET(lrr_check(c->layers, c->item_size, c->dropout, c->ln_eps));
    *st = {c->lru.batch, c->lru.seq_len, c->lru.width, c->layers, c->item_size, c->dropout, c->ln_eps,
           {&c->lru, lru_weights(c->lru).total, lru_ws(c->lru, true).total,
            [](const void* cfg, const float* x, const int64_t* ids, const float* w, float* z, void* ws, long n, hipStream_t s) {
                return bsarec_lru_fwd((const bsarec_lru_config_t*)cfg, x, ids, w, 1, z, ws, n, s);
            },
            [](const void* cfg, const float* x, const int64_t* ids, const float* w, const float* dz, void* ws, long n, float* dx,
               float* dw, hipStream_t s) { return bsarec_lru_bwd((const bsarec_lru_config_t*)cfg, x, ids, w, dz, ws, n, dx, dw, s); }}};
    return 0;
}

static int mamba4rec_step(const bsarec_mamba4rec_config_t* c, LrrStep* st) {
    if (!c) return -10;
    RET(mamba_check(&c->mamba));
    RET(lrr_check(c->layers, c->item_size, c->dropout, c->ln_eps));
    *st = {c->mamba.batch, c->mamba.seq_len, c->mamba.width, c->layers, c->item_size, c->dropout, c->ln_eps,
           {&c->mamba, mamba_weights(c->mamba).total, mamba_ws(c->mamba, true).total,
            [](const void* cfg, const float* x, const int64_t* ids, const float* w, float* z, void* ws, long n, hipStream_t s) {
                return bsarec_mamba_fwd((const bsarec_mamba_config_t*)cfg, x, ids, w, 1, z, ws, n, s);
            },
            [](const void* cfg, const float* x, const int64_t* ids, const float* w, const float* dz, void* ws, long n, float* dx,
               float* dw, hipStream_t s) { return bsarec_mamba_bwd((const bsarec_mamba_config_t*)cfg, x, ids, w, dz, ws, n, dx, dw, s); }}};
    return 0;
}

// offsets (floats) into the flat weight array: LayerNorm.weight | LayerNorm.bias, then per block (`first` + k `stride`) the array
// of the layer | its LayerNorm w, b | dense_1 w [4d][d], b [4d] | dense_2 w [d][4d], b [d] | feed_forward.LayerNorm w, b
struct LrrW { long first, stride, layer_ln, w1, b1, w2, b2, ff_ln, total; };
static LrrW lrr_weights(const LrrStep& c) {
    const long d = c.d;
    LrrW w;
    w.first = 2 * d;
    w.layer_ln = c.layer.weights;
    w.w1 = w.layer_ln + 2 * d; w.b1 = w.w1 + 4 * d * d;
    w.w2 = w.b1 + 4 * d; w.b2 = w.w2 + 4 * d * d;
    w.ff_ln = w.b2 + d; w.stride = w.ff_ln + 2 * d;
    w.total = w.first + c.layers * w.stride;
    return w;
}

// Workspace, in floats (every region a multiple of 4), T = B L, T4 = T rounded up to 4:
//   one [4] | xhat0 [T][d] | rstd0 [T4] | x_0 .. x_N [N + 1][T][d] | z [T][d] |
//   per block (`blk` + k `blk_stride`): the layer's workspace of train = 1 | a [T][d] | xhat_a [T][d] | rstd_a [T4] |
//     u [T][4d] | xhat_f [T][d] | rstd_f [T4] |
//   dy [T][d] | dz [T][d] | dt [T][d] | du [T][4d] | da [T][d] | dxl [T][d] | dh [B][d] | the CE head's workspace |
//   slabs of dW1 [ns][4d][d] | of dW2 [ns][d][4d] | of db1 [ns][4d] | of db2 [ns][d] | LayerNorm partials [2 N + 1][2][nb][d] |
//   the fixed-point accumulator [V][d] of 64-bit words
// ns: the split-K slices of a product over T rows (split_k); nb blocks of rows_pb rows: the grid of ln_bwd_kernel
struct LrrWs {
    long one, xhat0, rstd0, x, z, blk, blk_stride, dy, dz, dt, du, da, dxl, dh, ce, slab1, slab2, bp1, bp2, lnpart, acc, total;
    long b_a, b_xhat_a, b_rstd_a, b_u, b_xhat_f, b_rstd_f;        // inside a block's region, behind the layer's workspace at 0
    long layer_bytes, ce_bytes;
    int ns, kc, nb, rows_pb;
};
static LrrWs lrr_ws(const LrrStep& c) {
    const long B = c.B, T = B * c.L, d = c.d, N = c.layers, T4 = rup(T, 4);
    LrrWs w;
    memset(&w, 0, sizeof(w));
    split_k(T, &w.ns, &w.kc);
    w.nb = std::min(cdiv(T, 64), 256);
    w.rows_pb = (int)rup(cdiv(T, w.nb), 16);
    w.nb = cdiv(T, w.rows_pb);
    const long layer = c.layer.ws, ce = ce_workspace_floats((int)B, c.item_size, (int)d);
    w.layer_bytes = layer * (long)sizeof(float); w.ce_bytes = ce * (long)sizeof(float);
    long off = 0;
    w.one = off; off += 4;
    w.xhat0 = off; off += T * d;
    w.rstd0 = off; off += T4;
    w.x = off; off += (N + 1) * T * d;
    w.z = off; off += T * d;
    long b = layer;
    w.b_a = b; b += T * d;
    w.b_xhat_a = b; b += T * d;
    w.b_rstd_a = b; b += T4;
    w.b_u = b; b += T * 4 * d;
    w.b_xhat_f = b; b += T * d;
    w.b_rstd_f = b; b += T4;
    w.blk = off; w.blk_stride = b; off += N * b;
    w.dy = off; off += T * d;
    w.dz = off; off += T * d;
    w.dt = off; off += T * d;
    w.du = off; off += T * 4 * d;
    w.da = off; off += T * d;
    w.dxl = off; off += T * d;
    w.dh = off; off += B * d;
    w.ce = off; off += rup(ce, 4);
    w.slab1 = off; off += w.ns * 4 * d * d;
    w.slab2 = off; off += w.ns * 4 * d * d;
    w.bp1 = off; off += w.ns * 4 * d;
    w.bp2 = off; off += w.ns * d;
    w.lnpart = off; off += (2 * N + 1) * 2 * w.nb * d;
    w.acc = off; off += 2L * c.item_size * d;
    w.total = off;
    return w;
}

extern "C" long bsarec_lrurec_weight_floats(const bsarec_lrurec_config_t* cfg) {
    LrrStep st;
    return lrurec_step(cfg, &st) ? -10 : lrr_weights(st).total;
}

extern "C" long bsarec_lrurec_workspace_bytes(const bsarec_lrurec_config_t* cfg) {
    LrrStep st;
    return lrurec_step(cfg, &st) ? -10 : lrr_ws(st).total * (long)sizeof(float);
}

extern "C" long bsarec_mamba4rec_weight_floats(const bsarec_mamba4rec_config_t* cfg) {
    LrrStep st;
    return mamba4rec_step(cfg, &st) ? -10 : lrr_weights(st).total;
}

extern "C" long bsarec_mamba4rec_workspace_bytes(const bsarec_mamba4rec_config_t* cfg) {
    LrrStep st;
    return mamba4rec_step(cfg, &st) ? -10 : lrr_ws(st).total * (long)sizeof(float);
}

// dropout site `site` of a step; train = false: no mask, whatever p
static DropP lrr_drop(const LrrStep& c, const void* state, bool train, int site) {
    DropP d = site0_drop(c.dropout, state, train);
    d.site = (uint32_t)site;
    return d;
}

// ln_bwd_kernel over the step's T rows, MODE 0 (y = LN(Drop(z) + res): dz and dt = dz times the mask) or MODE 2 (y = Drop(LN(e)):
// dz = de); the d(gamma), d(beta) partials go to LayerNorm j's slot of the workspace
template <int MODE>
static void lrr_ln_bwd(const LrrWs& ws, float* w, int j, const float* dy, const float* xhat, const float* rstd, const float* gamma,
                          const DropP& drop, float* dz, float* dt, long T, int d, hipStream_t s) {
    LnBranch a;
    memset(&a, 0, sizeof(a));
    a.xhat = xhat; a.rstd = rstd; a.gamma = gamma; a.in_scale = 1.f; a.drop = drop; a.dT = dt;
    a.pgamma = w + ws.lnpart + (long)j * 2 * ws.nb * d; a.pbeta = a.pgamma + (long)ws.nb * d;
    DISPATCH_LPR(d, hipLaunchKernelGGL((ln_bwd_kernel<LPR, MODE>), dim3(ws.nb), dim3(ROW_THREADS), 0, s, dy, a, a, dz, (int)T, d,
                                       ws.rows_pb));
}

// tick_adam: null, or the Adam whose t the step's closing block advances (a *_train_step)
static int lrr_run(const LrrStep& c, const float* E, const float* weights, const int64_t* ids,
                      const int64_t* answers, void* state, int train, float* loss_out, float* dE, float* dweights, void* workspace,
                      const bsarec_adam_t* tick_adam, hipStream_t s) {
    const int B = c.B, L = c.L, d = c.d, N = c.layers, V = c.item_size;
    const long T = (long)B * L, Td = T * d;
    const bool tr = train != 0;
    const LrrWs ws = lrr_ws(c);
    const LrrW wo = lrr_weights(c);
    float* w = (float*)workspace;
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(w + ws.acc);
    const XformP nox = no_xform();
    const dim3 wg(ROW_THREADS);
    const dim3 flat_grid(std::min(cdiv(Td / 4, ROW_THREADS), 4096));
    auto X = [&](int k) { return w + ws.x + (long)k * Td; };
    auto blk = [&](int k) { return w + ws.blk + (long)k * ws.blk_stride; };
    auto Wb = [&](int k) { return weights + wo.first + (long)k * wo.stride; };

    // ---- forward
    if (tr) hipLaunchKernelGGL(step_begin_kernel, dim3(1), dim3(1), 0, s, (uint64_t*)state, (long long*)nullptr, 0);
    {
        LrrEmbedP P;
        P.E = E; P.ids = ids; P.gamma = weights; P.beta = weights + d; P.eps = c.ln_eps; P.drop = lrr_drop(c, state, tr, 0);
        P.T = T; P.d = d; P.V = V; P.x = X(0); P.xhat = w + ws.xhat0; P.rstd = w + ws.rstd0;
        P.acc = acc; P.acc_n2 = (long)V * d / 2; P.one = w + ws.one;
        DISPATCH_LPR(d, hipLaunchKernelGGL(lrr_embed_kernel<LPR>, dim3(std::min(cdiv(T, ROW_THREADS / LPR), 4096)), wg, 0, s, P));
    }
    for (int k = 0; k < N; ++k) {
        float* bw = blk(k);
        const float* wk = Wb(k);
        RET(c.layer.fwd(c.layer.cfg, X(k), ids, wk, w + ws.z, bw, ws.layer_bytes, s));
        {   // a = LN(Drop(z) + x)
            LrrAddLnP P;
            P.z = w + ws.z; P.x = X(k); P.gamma = wk + wo.layer_ln; P.beta = wk + wo.layer_ln + d; P.eps = c.ln_eps;
            P.drop = lrr_drop(c, state, tr, 1 + 2 * k); P.T = T; P.d = d;
            P.a = bw + ws.b_a; P.xhat = bw + ws.b_xhat_a; P.rstd = bw + ws.b_rstd_a;
            DISPATCH_LPR(d, hipLaunchKernelGGL(lrr_add_ln_kernel<LPR>, dim3(std::min(cdiv(T, ROW_THREADS / LPR), 4096)), wg, 0, s, P));
        }
        {   // u = dense_1(a)
            auto e = epi_linear<true, false, false>(bw + ws.b_u, 4 * d);
            e.bias[0] = wk + wo.b1;
            RET(dense_nt(bw + ws.b_a, wk + wo.w1, (int)T, 4 * d, d, e, s));
        }
        {   // x_{k+1} = LN(Drop(dense_2(gelu(u))) + a)
            GemmP g = gemm_defaults((int)T, d, 4 * d);
            g.lda = 4 * d; g.ldb = 4 * d; g.A[0] = bw + ws.b_u; g.B[0] = wk + wo.w2;
            EpiLN<false> e;
            e.bias = wk + wo.b2; e.R = bw + ws.b_a; e.drop = lrr_drop(c, state, tr, 2 + 2 * k);
            e.gamma = wk + wo.ff_ln; e.beta = wk + wo.ff_ln + d; e.eps = c.ln_eps;
            e.Y = X(k + 1); e.xhat = bw + ws.b_xhat_f; e.rstd = bw + ws.b_rstd_f;
            e.dsp = nullptr; e.alpha = 0.f; e.oma = 1.f;
            XformP xa = nox; xa.act = 0;
            DISPATCH_BN(d, RET((launch_gemm<64, BN, 2, 2, false, false, XF_GELU, XF_NONE, false>(g, xa, e, nullptr, 1, s, BSAREC_K_NONE,
                                                                                                  true))));
        }
    }
    // ---- the CE head on position L - 1 of x_N: the loss, dh [B][d] and the dense part of dE (every row written)
    const float* hlast = X(N) + (long)(L - 1) * d;
    RET(bsarec_ce_head_fwd(hlast, (long)L * d, E, B, V, d, answers, loss_out, nullptr, w + ws.ce, ws.ce_bytes, s));
    RET(bsarec_ce_head_bwd(hlast, (long)L * d, E, B, V, d, answers, w + ws.one, w + ws.ce, ws.ce_bytes, w + ws.dh, dE, s));
    hipLaunchKernelGGL(lrr_top_fill_kernel, flat_grid, wg, 0, s, w + ws.dh, w + ws.dy, Td / 4, L, d / 4);
    // ---- the blocks, top down; dy is the gradient of x_{k+1}
    for (int k = N - 1; k >= 0; --k) {
        float* bw = blk(k);
        const float* wk = Wb(k);
        float* dwk = dweights + wo.first + (long)k * wo.stride;
        lrr_ln_bwd<0>(ws, w, 2 + 2 * k, w + ws.dy, bw + ws.b_xhat_f, bw + ws.b_rstd_f, wk + wo.ff_ln,
                         lrr_drop(c, state, tr, 2 + 2 * k), w + ws.dz, w + ws.dt, T, d, s);
        {   // du = (dt . W2) * gelu'(u)
            auto e = epi_linear<false, false, true>(w + ws.du, 4 * d);
            e.U = bw + ws.b_u; e.ldu = 4 * d; e.act = 0;
            RET(dense_nn(w + ws.dt, wk + wo.w2, (int)T, 4 * d, d, e, s));
        }
        {   // da = du . W1 + dz
            auto e = epi_linear<false, true, false>(w + ws.da, d);
            e.R = w + ws.dz; e.ldr = d;
            RET(dense_nn(w + ws.du, wk + wo.w1, (int)T, d, 4 * d, e, s));
        }
        {   // dW1 = du^T . a, dW2 = dt^T . gelu(u), db1 and db2 the column sums of du and dt: split-K slabs in one grouped launch
            GroupedTN G;
            memset(&G, 0, sizeof(G));
            struct Spec { const float* A; long lda; const float* B; long ldb; int M, N; float* slab; float* bpart; int gelu; };
            const Spec sp[2] = {{w + ws.du, 4L * d, bw + ws.b_a, d, 4 * d, d, w + ws.slab1, w + ws.bp1, 0},
                                {w + ws.dt, d, bw + ws.b_u, 4L * d, d, 4 * d, w + ws.slab2, w + ws.bp2, 1}};
            int tiles = 0;
            for (int i = 0; i < 2; ++i) {
                GemmP g = gemm_defaults(sp[i].M, sp[i].N, (int)T);
                g.lda = sp[i].lda; g.ldb = sp[i].ldb; g.A[0] = sp[i].A; g.B[0] = sp[i].B; g.nsplit = ws.ns; g.kchunk = ws.kc;
                G.P[i] = g;
                G.E[i] = epi_linear<false, false, false>(sp[i].slab, sp[i].N);
                G.E[i].c_split = (long)sp[i].M * sp[i].N;
                G.bgrad[i] = sp[i].bpart;
                G.tile0[i] = tiles;
                G.tiles_n[i] = cdiv(sp[i].N, 64);
                G.b_gelu[i] = sp[i].gelu;
                tiles += cdiv(sp[i].M, 64) * G.tiles_n[i];
            }
            G.tile0[2] = tiles; G.nprob = 2; G.act = 0;
            RET((launch_lds<gemm_grouped_tn_kernel<false, 64>>(dim3(tiles, ws.ns), dim3(GEMM_THREADS),
                                                               GemmSmem<64, 64, true, true, false>::BYTES, s, G)));
            slab_sum(w + ws.slab1, T, 4L * d * d, dwk + wo.w1, s);
            slab_sum(w + ws.bp1, T, 4L * d, dwk + wo.b1, s);
            slab_sum(w + ws.slab2, T, 4L * d * d, dwk + wo.w2, s);
            slab_sum(w + ws.bp2, T, d, dwk + wo.b2, s);
        }
        lrr_ln_bwd<0>(ws, w, 1 + 2 * k, w + ws.da, bw + ws.b_xhat_a, bw + ws.b_rstd_a, wk + wo.layer_ln,
                         lrr_drop(c, state, tr, 1 + 2 * k), w + ws.dz, w + ws.dt, T, d, s);
        RET(c.layer.bwd(c.layer.cfg, X(k), ids, wk, w + ws.dt, bw, ws.layer_bytes, w + ws.dxl, dwk, s));
        hipLaunchKernelGGL(lrr_add_kernel, flat_grid, wg, 0, s, w + ws.dxl, w + ws.dz, w + ws.dy, Td / 4);
    }
    // ---- the embedding: de = LNbwd(dy times the mask), every LayerNorm's parameter gradient, the lookup rows onto dE
    lrr_ln_bwd<2>(ws, w, 0, w + ws.dy, w + ws.xhat0, w + ws.rstd0, weights, lrr_drop(c, state, tr, 0), w + ws.dz, nullptr, T, d, s);
    {
        LrrLnSumP P;
        P.part = w + ws.lnpart; P.nb = ws.nb; P.d = d; P.dw = dweights;
        P.first = wo.first; P.stride = wo.stride; P.at_layer = wo.layer_ln; P.at_ff = wo.ff_ln;
        hipLaunchKernelGGL(lrr_ln_sum_kernel, dim3(2 * N + 1), wg, 0, s, P);
    }
    {
        LrrItemGradP P;
        P.de = w + ws.dz; P.ids = ids; P.T = T; P.d = d; P.V = V; P.dA = acc;
        DISPATCH_LPR(d, hipLaunchKernelGGL(lrr_item_grad_kernel<LPR>, dim3(cdiv(T, SCATTER_FLOATS / (4 * LPR))), wg, 0, s, P));
    }
    // the accumulator is ADDED onto the head's dense dE; the closing block of a training step advances Adam's t
    LookupAcc la = pair_flush_acc(acc, dE, (long)V * d);
    la.dense_zero = 0;
    const bsarec_adam_t* a = tick_adam;
    const TickP tk = a ? make_tick(state, 1, a->lr, a->beta1, a->beta2, nullptr, 0, nullptr, nullptr, 0, 0)
                       : make_tick(state, 0, 0.f, 0.f, 0.f, nullptr, 0, nullptr, nullptr, 0, 0);
    hipLaunchKernelGGL(pair_flush_kernel, dim3(la.nblocks + (a ? 1 : 0)), wg, 0, s, la, tk);
    return (int)hipGetLastError();
}

static int lrr_loss_grad(const LrrStep& st, const float* item_emb, const float* weights, const int64_t* ids, const int64_t* answers,
                         void* state, int train, float* loss_out, float* d_item_emb, float* dweights, void* workspace,
                         long workspace_bytes, const bsarec_adam_t* tick_adam, hipStream_t s) {
    RET(ptrs_check({item_emb, weights, d_item_emb, dweights, workspace}, {ids, answers, state}, {loss_out}));
    if (workspace_bytes < lrr_ws(st).total * (long)sizeof(float)) return -10;
    return lrr_run(st, item_emb, weights, ids, answers, state, train, loss_out, d_item_emb, dweights, workspace, tick_adam, s);
}

static int lrr_train_step(const LrrStep& st, const int64_t* ids, const int64_t* answers, const bsarec_adam_t* adam_items,
                          const bsarec_adam_t* adam_weights, void* state, float* loss_out, void* workspace, long workspace_bytes,
                          hipStream_t s) {
    const StepAdam adams[] = {{adam_items, (long)st.item_size * st.d}, {adam_weights, lrr_weights(st).total}};
    RET(pair_adams_check(adams));
    RET(lrr_loss_grad(st, adam_items->params, adam_weights->params, ids, answers, state, 1, loss_out, adam_grads(adam_items),
                      adam_grads(adam_weights), workspace, workspace_bytes, adam_items, s));
    return pair_adams_launch(adams, state, s);
}

extern "C" int bsarec_lrurec_loss_grad(const bsarec_lrurec_config_t* cfg, const float* item_emb, const float* weights,
                                       const int64_t* ids, const int64_t* answers, void* state, int train, float* loss_out,
                                       float* d_item_emb, float* dweights, void* workspace, long workspace_bytes, void* stream) {
    LrrStep st;
    RET(lrurec_step(cfg, &st));
    return lrr_loss_grad(st, item_emb, weights, ids, answers, state, train, loss_out, d_item_emb, dweights, workspace,
                         workspace_bytes, nullptr, (hipStream_t)stream);
}

extern "C" int bsarec_lrurec_train_step(const bsarec_lrurec_config_t* cfg, const int64_t* ids, const int64_t* answers,
                                        const bsarec_adam_t* adam_items, const bsarec_adam_t* adam_weights, void* state,
                                        float* loss_out, void* workspace, long workspace_bytes, void* stream) {
    LrrStep st;
    RET(lrurec_step(cfg, &st));
    return lrr_train_step(st, ids, answers, adam_items, adam_weights, state, loss_out, workspace, workspace_bytes,
                          (hipStream_t)stream);
}

extern "C" int bsarec_mamba4rec_loss_grad(const bsarec_mamba4rec_config_t* cfg, const float* item_emb, const float* weights,
                                          const int64_t* ids, const int64_t* answers, void* state, int train, float* loss_out,
                                          float* d_item_emb, float* dweights, void* workspace, long workspace_bytes, void* stream) {
    LrrStep st;
    RET(mamba4rec_step(cfg, &st));
    return lrr_loss_grad(st, item_emb, weights, ids, answers, state, train, loss_out, d_item_emb, dweights, workspace,
                         workspace_bytes, nullptr, (hipStream_t)stream);
}

extern "C" int bsarec_mamba4rec_train_step(const bsarec_mamba4rec_config_t* cfg, const int64_t* ids, const int64_t* answers,
                                           const bsarec_adam_t* adam_items, const bsarec_adam_t* adam_weights, void* state,
                                           float* loss_out, void* workspace, long workspace_bytes, void* stream) {
    LrrStep st;
    RET(mamba4rec_step(cfg, &st));
    return lrr_train_step(st, ids, answers, adam_items, adam_weights, state, loss_out, workspace, workspace_bytes,
                          (hipStream_t)stream);
}

static int g4c_alone_check(int B, int d, int V, const bsarec_gru4rec_head_t* head) {
    if (B < 1 || B > 65536 || d < 4 || d > 256 || d % 4 || V < 2) return -10;
    return g4c_head_check(head, B);
}

// the head alone: its regions, then the loss rows [B up to 4]
extern "C" long bsarec_gru4rec_cand_head_workspace_bytes(int batch, int width, const bsarec_gru4rec_head_t* head) {
    if (g4c_alone_check(batch, width, 2, head)) return -10;
    return (g4c_ws(batch, head->candidates, width, 0).end + rup(batch, 4)) * (long)sizeof(float);
}

extern "C" int bsarec_gru4rec_cand_head(const float* s, const float* item_emb, const int64_t* answers, const int64_t* neg_answers,
                                        int batch, int width, int item_size, const bsarec_gru4rec_head_t* head, float* loss_out,
                                        float* ds, float* dEc, void* workspace, long workspace_bytes, void* stream) {
    RET(g4c_alone_check(batch, width, item_size, head));
    RET(ptrs_check({s, item_emb, ds, dEc, workspace}, {answers, neg_answers}, {loss_out}));
    if (workspace_bytes < bsarec_gru4rec_cand_head_workspace_bytes(batch, width, head)) return -10;
    const G4cWs g = g4c_ws(batch, head->candidates, width, 0);
    float* w = (float*)workspace;
    hipStream_t st = (hipStream_t)stream;
    g4c_launch(g, w, s, item_emb, answers, neg_answers, batch, width, item_size, *head, w + g.end, ds, dEc, st);
    hipLaunchKernelGGL(adam_tick_kernel, dim3(1), dim3(ROW_THREADS), 0, st,
                       make_tick(nullptr, 0, 0.f, 0.f, 0.f, w + g.end, batch, loss_out, nullptr, 0, 0));
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Caser training step (caser_step.h): fc1 in both directions alone, and the whole step -- lookup, bsarec_caser_fwd, fc1, the BPR
// head, every gradient, Adam -- plan-less, one linear chain of launches on the caller's stream, no allocation, no host
// synchronisation
// ---------------------------------------------------------------------------------------------
static bool caser_fc_shape_ok(int B, int F, int d) {
    return B >= 1 && B <= 65536 && F >= 4 && F <= 12288 && F % 4 == 0 && row_dim_ok(d);
}

extern "C" long bsarec_caser_fc_floats(const bsarec_caser_config_t* cfg) {
    if (caser_check(cfg)) return -10;
    return (caser_weights(*cfg).F + 1) * cfg->width;
}

// zd [B][F]: the dropped-out z of a masked forward, read by the backward
extern "C" long bsarec_caser_fc_workspace_bytes(int batch, int features, int width) {
    if (!caser_fc_shape_ok(batch, features, width)) return -10;
    return (long)batch * features * (long)sizeof(float);
}

// z, fc, the drop and the shape are set; the masked forward leaves zd in `zd`, and the backward reads it there (z otherwise)
static CaserFcP caser_fc_params(int B, int F, int d, const float* z, const float* fc, const DropP& drop, float* zd) {
    CaserFcP P;
    memset(&P, 0, sizeof(P));
    P.z = z; P.w = fc; P.B = B; P.F = F; P.d = d; P.drop = drop;
    P.zd_out = drop.thresh ? zd : nullptr;
    P.zd = drop.thresh ? zd : z;
    return P;
}

static void caser_fc_fwd_launch(const CaserFcP& P, hipStream_t s) {
    const dim3 grid(cdiv(P.B, 16));
    const int nt = P.d <= 64 ? 4 : (P.d <= 128 ? 8 : 16), nw = nt <= 8 ? 8 : 4;
    const size_t lds = (size_t)(nw - 1) * 16 * (16 * nt + CASER_FC_LDS_PAD) * sizeof(float);      // 30,464 / 59,136 / 49,920 bytes
    if (nt == 4) hipLaunchKernelGGL((caser_fc_fwd_kernel<4, 8>), grid, dim3(512), lds, s, P);
    else if (nt == 8) hipLaunchKernelGGL((caser_fc_fwd_kernel<8, 8>), grid, dim3(512), lds, s, P);
    else hipLaunchKernelGGL((caser_fc_fwd_kernel<16, 4>), grid, dim3(256), lds, s, P);
}

static void caser_fc_bwd_launch(const CaserFcP& P, hipStream_t s) {
    hipLaunchKernelGGL(caser_fc_dz_kernel, dim3(cdiv(P.F, 256), cdiv(P.B, 16)), dim3(256), 0, s, P);
    hipLaunchKernelGGL(caser_fc_dw_kernel, dim3(cdiv(P.F, 64), cdiv(P.d, 64)), dim3(256), 0, s, P);
}

extern "C" int bsarec_caser_fc_fwd(int batch, int features, int width, const float* z, const float* fc, const void* state,
                                   int train, float dropout, float* s, void* workspace, long workspace_bytes, void* stream) {
    if (!caser_fc_shape_ok(batch, features, width) || !dropout_ok(dropout)) return -10;
    RET(ptrs_check({z, fc, s, workspace}, {state}));
    if (workspace_bytes < bsarec_caser_fc_workspace_bytes(batch, features, width)) return -10;
    CaserFcP P = caser_fc_params(batch, features, width, z, fc, site0_drop(dropout, state, train != 0), (float*)workspace);
    P.s_out = s;
    caser_fc_fwd_launch(P, (hipStream_t)stream);
    return (int)hipGetLastError();
}

extern "C" int bsarec_caser_fc_bwd(int batch, int features, int width, const float* z, const float* fc, const float* s,
                                   const float* ds, const void* state, int train, float dropout, float* dz, float* dfc,
                                   void* workspace, long workspace_bytes, void* stream) {
    if (!caser_fc_shape_ok(batch, features, width) || !dropout_ok(dropout)) return -10;
    RET(ptrs_check({z, fc, s, ds, dz, dfc, workspace}, {state}));
    if (workspace_bytes < bsarec_caser_fc_workspace_bytes(batch, features, width)) return -10;
    CaserFcP P = caser_fc_params(batch, features, width, z, fc, site0_drop(dropout, state, train != 0), (float*)workspace);
    P.s = s; P.ds = ds; P.dz = dz; P.dw = dfc;
    caser_fc_bwd_launch(P, (hipStream_t)stream);
    return (int)hipGetLastError();
}

static int caser_step_check(const bsarec_caser_step_config_t* c) {
    if (!c) return -10;
    RET(caser_check(&c->conv));
    if (c->item_size < 2 || !dropout_ok(c->dropout)) return -10;
    return 0;
}

// Workspace, in floats (every region a multiple of 4): the convolution workspace of train = 1 | x [T][d] | z [B][F] | zd [B][F] |
// s [B][d] | ds [B][d] | dz [B][F] | dx [T][d] | c [B up to 4] | loss rows [B up to 4] | the fixed-point accumulator [V][d] of
// 64-bit words
struct CaserStepWs { long conv, x, z, zd, s, ds, dz, dx, c, rows, acc, total; long conv_bytes; };
static CaserStepWs caser_step_ws(const bsarec_caser_step_config_t& c) {
    const long B = c.conv.batch, T = B * c.conv.seq_len, d = c.conv.width, F = caser_weights(c.conv).F;
    CaserStepWs w;
    long off = 0;
    w.conv = off; w.conv_bytes = caser_ws_bytes(c.conv, true); off += w.conv_bytes / (long)sizeof(float);
    w.x = off; off += T * d;
    w.z = off; off += B * F;
    w.zd = off; off += B * F;
    w.s = off; off += B * d;
    w.ds = off; off += B * d;
    w.dz = off; off += B * F;
    w.dx = off; off += T * d;
    w.c = off; off += rup(B, 4);
    w.rows = off; off += rup(B, 4);
    w.acc = off; off += 2L * c.item_size * d;
    w.total = off;
    return w;
}

extern "C" long bsarec_caser_step_workspace_bytes(const bsarec_caser_step_config_t* cfg) {
    if (caser_step_check(cfg)) return -10;
    return caser_step_ws(*cfg).total * (long)sizeof(float);
}

// ---------------------------------------------------------------------------------------------
// Personalised Caser step (caser_user.h): the step above with a user table and fc2 = Linear(2 d, d) behind fc1.  fc2 runs on
// fc1's launches; the chain is linear on the caller's stream, no allocation, no host synchronisation.  Both steps run through
// one driver, caser_run, with the user part absent or present
// ---------------------------------------------------------------------------------------------
static int caser_user_check(const bsarec_caser_user_step_config_t* c) {
    if (!c) return -10;
    RET(caser_step_check(&c->step));
    if (c->num_users < 1) return -10;
    return 0;
}

extern "C" long bsarec_caser_fc2_floats(const bsarec_caser_config_t* cfg) {
    if (caser_check(cfg)) return -10;
    return (2L * cfg->width + 1) * cfg->width;
}

// Workspace, in floats: the regions of caser_step_ws (its s holds z1, its ds holds dz1) | x2 [B][2 d] | s [B][d] | ds [B][d] |
// dx2 [B][2 d] | the fixed-point accumulator [U][d] of 64-bit words
struct CaserUserWs { CaserStepWs st; long x2, s, ds, dx2, uacc, total; };
static CaserUserWs caser_user_ws(const bsarec_caser_user_step_config_t& c) {
    const long B = c.step.conv.batch, d = c.step.conv.width;
    CaserUserWs w;
    w.st = caser_step_ws(c.step);
    long off = w.st.total;
    w.x2 = off; off += 2 * B * d;
    w.s = off; off += B * d;
    w.ds = off; off += B * d;
    w.dx2 = off; off += 2 * B * d;
    w.uacc = off; off += 2L * c.num_users * d;
    w.total = off;
    return w;
}

extern "C" long bsarec_caser_user_step_workspace_bytes(const bsarec_caser_user_step_config_t* cfg) {
    if (caser_user_check(cfg)) return -10;
    return caser_user_ws(*cfg).total * (long)sizeof(float);
}

// what the personalised step has beyond the item-only one: its arrays, and in ws its regions of the workspace
struct CaserUserPart { int U; const int64_t* users; const float* P; const float* fc2; float* dP; float* dfc2; CaserUserWs ws; };

// tick_adam: null, or the Adam whose t the step's closing block advances (a *_train_step); u: null, or the user part
static int caser_run(const bsarec_caser_step_config_t& c, const CaserUserPart* u, const float* E, const float* weights,
                     const float* fc, const int64_t* ids, const int64_t* answers, const int64_t* neg_answers, void* state, int train,
                     float* loss_out, float* dE, float* dweights, float* dfc, void* workspace, const bsarec_adam_t* tick_adam,
                     hipStream_t s) {
    const int B = c.conv.batch, d = c.conv.width, F = (int)caser_weights(c.conv).F;
    const CaserStepWs ws = caser_step_ws(c);
    float* w = (float*)workspace;
    const DropP none = site0_drop(0.f, state, false);  // the token rows and fc2 carry no mask
    const PairStep p = {B, d, c.item_size, (long)B * c.conv.seq_len, E, ids, answers, neg_answers, state, train, none,
                        w + ws.x, w + ws.dx, w + ws.c, w + ws.rows, reinterpret_cast<unsigned long long*>(w + ws.acc), dE, loss_out,
                        tick_adam, s};
    pair_begin_embed(p);
    RET(bsarec_caser_fwd(&c.conv, p.x, weights, 1, w + ws.z, w + ws.conv, ws.conv_bytes, s));

    CaserFcP pf = caser_fc_params(B, F, d, w + ws.z, fc, site0_drop(c.dropout, state, train != 0), w + ws.zd);
    pf.s_out = w + ws.s; pf.s = w + ws.s; pf.ds = w + ws.ds; pf.dz = w + ws.dz; pf.dw = dfc;      // with u: s = z1, ds = dz1
    caser_fc_fwd_launch(pf, s);

    float* sv = w + (u ? u->ws.s : ws.s);               // the state the head reads, and its gradient
    float* dsv = w + (u ? u->ws.ds : ws.ds);
    CaserUserP pu;
    CaserFcP p2;
    if (u) {                                            // x2 = [z1 | P[users]], the state = relu(fc2(x2))
        memset(&pu, 0, sizeof(pu));
        pu.z1 = w + ws.s; pu.P = u->P; pu.users = u->users; pu.x2 = w + u->ws.x2; pu.dx2 = w + u->ws.dx2; pu.dz1 = w + ws.ds;
        pu.B = B; pu.d = d; pu.U = u->U; pu.acc_n2 = (long)u->U * d / 2;
        pu.acc = reinterpret_cast<unsigned long long*>(w + u->ws.uacc);
        DISPATCH_LPR(d, hipLaunchKernelGGL(caser_user_concat_kernel<LPR>, dim3(std::min(cdiv(B, ROW_THREADS / LPR), 4096)),
                                           dim3(ROW_THREADS), 0, s, pu));
        p2 = caser_fc_params(B, 2 * d, d, pu.x2, u->fc2, none, nullptr);
        p2.s_out = sv; p2.s = sv; p2.ds = dsv; p2.dz = w + u->ws.dx2; p2.dw = u->dfc2;
        caser_fc_fwd_launch(p2, s);
    }
    pair_bpr(p, sv, dsv);

    if (u) {                                            // fc2 backwards; dx2 -> the user rows and dz1
        caser_fc_bwd_launch(p2, s);
        DISPATCH_LPR(d, {
            pu.scatter_blocks = cdiv(B, SCATTER_FLOATS / (4 * LPR));
            hipLaunchKernelGGL(caser_user_grad_kernel<LPR>, dim3(pu.scatter_blocks + cdiv(B, ROW_THREADS / LPR)), dim3(ROW_THREADS),
                               0, s, pu);
        });
    }
    caser_fc_bwd_launch(pf, s);
    RET(bsarec_caser_bwd(&c.conv, p.x, weights, w + ws.dz, w + ws.conv, ws.conv_bytes, p.dx, dweights, s));
    pair_item_grad(p, sv);

    if (u) {                                            // a grid of exactly nblocks: no closing block, the tick is not read
        const LookupAcc lu = pair_flush_acc(pu.acc, u->dP, (long)u->U * d);
        hipLaunchKernelGGL(pair_flush_kernel, dim3(lu.nblocks), dim3(ROW_THREADS), 0, s, lu,
                           make_tick(nullptr, 0, 0.f, 0.f, 0.f, nullptr, 0, nullptr, nullptr, 0, 0));
    }
    return pair_flush_tick(p);
}

static int caser_loss_grad(const bsarec_caser_step_config_t* cfg, const CaserUserPart* u, const float* item_emb,
                           const float* weights, const float* fc, const int64_t* ids, const int64_t* answers,
                           const int64_t* neg_answers, void* state, int train, float* loss_out, float* d_item_emb, float* dweights,
                           float* dfc, void* workspace, long workspace_bytes, const bsarec_adam_t* tick_adam, hipStream_t s) {
    RET(caser_step_check(cfg));
    RET(ptrs_check({item_emb, weights, fc, d_item_emb, dweights, dfc, workspace}, {ids, answers, neg_answers, state}, {loss_out}));
    if (u) RET(ptrs_check({u->P, u->fc2, u->dP, u->dfc2}, {u->users}));
    if (workspace_bytes < (u ? u->ws.total : caser_step_ws(*cfg).total) * (long)sizeof(float)) return -10;
    return caser_run(*cfg, u, item_emb, weights, fc, ids, answers, neg_answers, state, train, loss_out, d_item_emb, dweights, dfc,
                     workspace, tick_adam, s);
}

extern "C" int bsarec_caser_loss_grad(const bsarec_caser_step_config_t* cfg, const float* item_emb, const float* weights,
                                      const float* fc, const int64_t* ids, const int64_t* answers, const int64_t* neg_answers,
                                      void* state, int train, float* loss_out, float* d_item_emb, float* dweights, float* dfc,
                                      void* workspace, long workspace_bytes, void* stream) {
    return caser_loss_grad(cfg, nullptr, item_emb, weights, fc, ids, answers, neg_answers, state, train, loss_out, d_item_emb,
                           dweights, dfc, workspace, workspace_bytes, nullptr, (hipStream_t)stream);
}

extern "C" int bsarec_caser_train_step(const bsarec_caser_step_config_t* cfg, const int64_t* ids, const int64_t* answers,
                                       const int64_t* neg_answers, const bsarec_adam_t* adam_items,
                                       const bsarec_adam_t* adam_weights, const bsarec_adam_t* adam_fc, void* state,
                                       float* loss_out, void* workspace, long workspace_bytes, void* stream) {
    RET(caser_step_check(cfg));
    const CaserW wo = caser_weights(cfg->conv);
    const StepAdam adams[] = {{adam_items, (long)cfg->item_size * cfg->conv.width}, {adam_weights, wo.total},
                              {adam_fc, (wo.F + 1) * cfg->conv.width}};
    RET(pair_adams_check(adams));
    hipStream_t s = (hipStream_t)stream;
    RET(caser_loss_grad(cfg, nullptr, adam_items->params, adam_weights->params, adam_fc->params, ids, answers, neg_answers, state,
                        1, loss_out, adam_grads(adam_items), adam_grads(adam_weights), adam_grads(adam_fc), workspace,
                        workspace_bytes, adam_items, s));
    return pair_adams_launch(adams, state, s);
}

extern "C" int bsarec_caser_user_loss_grad(const bsarec_caser_user_step_config_t* cfg, const float* item_emb,
                                           const float* user_emb, const float* weights, const float* fc, const float* fc2,
                                           const int64_t* ids, const int64_t* users, const int64_t* answers,
                                           const int64_t* neg_answers, void* state, int train, float* loss_out,
                                           float* d_item_emb, float* d_user_emb, float* dweights, float* dfc, float* dfc2,
                                           void* workspace, long workspace_bytes, void* stream) {
    RET(caser_user_check(cfg));
    const CaserUserPart u = {cfg->num_users, users, user_emb, fc2, d_user_emb, dfc2, caser_user_ws(*cfg)};
    return caser_loss_grad(&cfg->step, &u, item_emb, weights, fc, ids, answers, neg_answers, state, train, loss_out, d_item_emb,
                           dweights, dfc, workspace, workspace_bytes, nullptr, (hipStream_t)stream);
}

extern "C" int bsarec_caser_user_train_step(const bsarec_caser_user_step_config_t* cfg, const int64_t* ids,
                                            const int64_t* users, const int64_t* answers, const int64_t* neg_answers,
                                            const bsarec_adam_t* adam_items, const bsarec_adam_t* adam_users,
                                            const bsarec_adam_t* adam_weights, const bsarec_adam_t* adam_fc,
                                            const bsarec_adam_t* adam_fc2, void* state, float* loss_out, void* workspace,
                                            long workspace_bytes, void* stream) {
    RET(caser_user_check(cfg));
    const bsarec_caser_config_t& cv = cfg->step.conv;
    const CaserW wo = caser_weights(cv);
    const StepAdam adams[] = {{adam_items, (long)cfg->step.item_size * cv.width}, {adam_users, (long)cfg->num_users * cv.width},
                              {adam_weights, wo.total}, {adam_fc, (wo.F + 1) * cv.width},
                              {adam_fc2, (2L * cv.width + 1) * cv.width}};
    RET(pair_adams_check(adams));
    hipStream_t s = (hipStream_t)stream;
    const CaserUserPart u = {cfg->num_users, users, adam_users->params, adam_fc2->params, adam_grads(adam_users),
                             adam_grads(adam_fc2), caser_user_ws(*cfg)};
    RET(caser_loss_grad(&cfg->step, &u, adam_items->params, adam_weights->params, adam_fc->params, ids, answers, neg_answers, state,
                        1, loss_out, adam_grads(adam_items), adam_grads(adam_weights), adam_grads(adam_fc), workspace,
                        workspace_bytes, adam_items, s));
    return pair_adams_launch(adams, state, s);
}

// ---------------------------------------------------------------------------------------------
// stand-alone FrequencyLayer (per-op parity tests)
// ---------------------------------------------------------------------------------------------
static DropP standalone_drop(float p, const void* state, int site) {
    DropP d;
    d.thresh = drop_thresh(p);
    d.scale = p > 0.f ? (float)(1.0 / (1.0 - (double)p)) : 1.f;
    d.rng = (const uint64_t*)state; d.site = (uint32_t)site;
    return d;
}

extern "C" int bsarec_freq_layer_fwd(const float* x, const float* sqrt_beta, const float* ln_w, const float* ln_b,
                                     const float* twiddle, int B, int L, int d, int cb, float eps, float p_drop,
                                     const void* state, int site, float* y, float* xhat, float* rstd, void* stream) {
    if (!x || !y || d % 4 || d > 256 || L > 256 || (long)cb * d > 8192 || (p_drop > 0.f && !state)) return -10;
    DISPATCH_LPR(d, RET(launch_freq_fwd<LPR>(x, sqrt_beta, ln_w, ln_b, eps, standalone_drop(p_drop, state, site), twiddle,
                                             B, L, d, cb, y, xhat, rstd, (hipStream_t)stream)));
    return 0;
}

extern "C" long bsarec_freq_layer_bwd_scratch_floats(int B, int L, int d) {
    const long T = (long)B * L;
    return 3 * T * d + (long)B * d + 2L * cdiv(T, 64) * d + 64;
}

extern "C" int bsarec_freq_layer_bwd(const float* x, const float* dy, const float* xhat, const float* rstd,
                                     const float* sqrt_beta, const float* ln_w, const float* twiddle, int B, int L, int d,
                                     int cb, float p_drop, const void* state, int site, float* scratch, float* dx,
                                     float* dsqrt_beta, float* dln_w, float* dln_b, void* stream) {
    if (!x || !dy || !scratch || d % 4 || d > 256 || L > 256 || (long)cb * d > 8192 || (p_drop > 0.f && !state)) return -10;
    hipStream_t s = (hipStream_t)stream;
    const int T = B * L, nb = cdiv(T, 64);
    float* dz = scratch; float* dF = dz + (long)T * d; float* pbeta = dF + (long)T * d;
    float* pg = pbeta + (long)B * d; float* pb = pg + (long)nb * d;
    LnBranch a; memset(&a, 0, sizeof(a));
    a.xhat = xhat; a.rstd = rstd; a.gamma = ln_w; a.in_scale = 1.f; a.drop = standalone_drop(p_drop, state, site);
    a.dT = dF; a.pgamma = pg; a.pbeta = pb;
    DISPATCH_LPR(d, LAUNCH((ln_bwd_kernel<LPR, 0>), dim3(nb), dim3(ROW_THREADS), 0, s, dy, a, a, dz, T, d, 64));
    HIPCHK(hipGetLastError());
    // y = LN(Drop(f(x)) + x): the residual contributes dz directly
    DISPATCH_LPR(d, RET(launch_freq_bwd<LPR>(x, dF, dz, sqrt_beta, twiddle, B, L, d, cb, dx, pbeta, s)));
    ReduceJobs3 hj;                      // the three jobs travel in the kernarg block: no staging copy, no synchronisation
    hj.j[0] = ReduceJob{pbeta, dsqrt_beta, B, d, d, 1.f, 0};
    hj.j[1] = ReduceJob{pg, dln_w, nb, d, d, 1.f, 0};
    hj.j[2] = ReduceJob{pb, dln_b, nb, d, d, 1.f, 0};
    LAUNCH(multi_reduce3_kernel, dim3(cdiv(d, 64), 3), dim3(ROW_THREADS), 0, s, hj);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// profiling hooks
// ---------------------------------------------------------------------------------------------
extern "C" int bsarec_profile_select(bsarec_plan_t* p, int kclass) {
    if (!p) return -10;
    p->prof.kclass = kclass;
    p->prof.used = 0;
    return 0;
}

extern "C" int bsarec_profile_read(bsarec_plan_t* p, double* ms_total, int* launches) {
    if (!p) return -10;
    ProfState& ps = p->prof;
    double tot = 0.0;
    for (size_t i = 0; i < ps.used; ++i) {
        HIPCHK(hipEventSynchronize(ps.events[i].second));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, ps.events[i].first, ps.events[i].second));
        tot += ms;
    }
    if (ms_total) *ms_total = tot;
    if (launches) *launches = (int)ps.used;
    ps.used = 0;
    return 0;
}

extern "C" int bsarec_profile_event_overhead(void* stream, int reps, double* ms_avg) {
    hipStream_t s = (hipStream_t)stream;
    hipEvent_t a, b;
    HIPCHK(hipEventCreate(&a)); HIPCHK(hipEventCreate(&b));
    double tot = 0.0;
    for (int i = 0; i < reps; ++i) {
        HIPCHK(hipEventRecord(a, s)); HIPCHK(hipEventRecord(b, s));
        HIPCHK(hipEventSynchronize(b));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, a, b));
        tot += ms;
    }
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    if (ms_avg) *ms_avg = reps > 0 ? tot / reps : 0.0;
    return 0;
}

// ---------------------------------------------------------------------------------------------
// catalogue-sharded head (include/bsarec_shard.h, catalogue_shard.h)
// ---------------------------------------------------------------------------------------------
static int shard_ptrs(ShardPtrs& S, const float* const* p, int world) {
    if (!p || world < 1 || world > 8) return -10;
    memset(&S, 0, sizeof(S));
    for (int r = 0; r < world; ++r) { if (!p[r]) return -10; S.p[r] = p[r]; }
    return 0;
}

extern "C" int bsarec_shard_gather_rows(const int64_t* ids, long n, const float* const* shards, int world, long rows_per,
                                        long V, int d, float* stage, int64_t* local_ids, void* stream) {
    if (!ids || !stage || !local_ids || n < 1 || rows_per < 1 || V < 1 || d < 4 || (d & 3)) return -10;
    if ((V + rows_per - 1) / rows_per > world) return -11;
    ShardPtrs S;
    RET(shard_ptrs(S, shards, world));
    const int d4 = d / 4;
    LAUNCH(shard_gather_rows_kernel, dim3(cdiv((n + 1) * d4, 256)), dim3(256), 0, (hipStream_t)stream, ids, n, S, rows_per, V, d4,
           stage, local_ids);
    return (int)hipGetLastError();
}

extern "C" int bsarec_shard_logits(const float* h, long ldh, int Bg, const float* E, int Vs, int d, float* logits, long ld,
                                   void* stream) {
    if (!h || !logits || Bg < 1 || Vs < 0 || d < 4 || (d & 3) || ld < Vs || (ld & 3) || ldh < d) return -10;
    if (Vs == 0) return 0;
    if (!E) return -10;
    GemmP g = gemm_defaults(Bg, (int)ld, d);
    g.Nb = Vs; g.lda = ldh; g.ldb = d;
    g.A[0] = h; g.B[0] = E;
    auto e = epi_linear<false, false, false>(logits, ld);
    return launch_gemm<64, 64, 2, 2, false, false, XF_NONE, XF_NONE, false>(g, no_xform(), e, nullptr, 1, (hipStream_t)stream);
}

extern "C" int bsarec_shard_ce_stats(const float* logits, long ld, int Bg, int Vs, const int64_t* answers, long lo, long V,
                                     float* stats, void* stream) {
    if (!logits || !answers || !stats || Bg < 1 || Vs < 0 || ld < Vs || (ld & 3)) return -10;
    LAUNCH(shard_ce_stats_kernel, dim3(Bg), dim3(ROW_THREADS), 0, (hipStream_t)stream, logits, ld, Vs, answers, lo, V, stats, Bg);
    return (int)hipGetLastError();
}

extern "C" int bsarec_shard_ce_grad(float* logits, long ld, int Bg, int Vs, const int64_t* answers, long lo, long V,
                                    const float* stats_all, int world, float* loss_rows, float* loss, void* stream) {
    if (!logits || !answers || !stats_all || !loss_rows || Bg < 1 || Vs < 0 || ld < Vs || (ld & 3) || world < 1 || world > 8)
        return -10;
    hipStream_t s = (hipStream_t)stream;
    LAUNCH(shard_ce_grad_kernel, dim3(Bg), dim3(ROW_THREADS), 0, s, logits, ld, Vs, answers, lo, V, stats_all, world, Bg,
           1.0f / (float)Bg, loss_rows);
    HIPCHK(hipGetLastError());
    if (loss) LAUNCH(loss_mean_kernel, dim3(1), dim3(ROW_THREADS), 0, s, loss_rows, Bg, loss);
    return (int)hipGetLastError();
}

// split-K over the owned rows for d h_last: enough slices to fill the chip at small Bg, chunks of >= 4096 rows
static void shard_split(int Bg, int Vs, int d, int* nsplit, int* kchunk) {
    const long tiles = (long)cdiv(Bg, 64) * cdiv(d, 64);
    long want = (1024 + tiles - 1) / tiles;
    if (want < 1) want = 1;
    if (want > 64) want = 64;
    long ch = rup(cdiv(Vs > 0 ? Vs : 1, want), GEMM_BK);
    if (ch < 256) ch = 256;
    *kchunk = (int)ch;
    *nsplit = cdiv(Vs > 0 ? Vs : 1, ch);
}

extern "C" long bsarec_shard_head_bwd_scratch_floats(int Bg, int Vs, int d) {
    if (Bg < 1 || Vs < 0 || d < 4) return -10;
    int ns, kc;
    shard_split(Bg, Vs, d, &ns, &kc);
    return (long)ns * Bg * d;
}

extern "C" int bsarec_shard_head_bwd(const float* dlogits, long ld, int Bg, int Vs, const float* h, long ldh, const float* E,
                                     int d, float* dE, float* dh, float* scratch, void* stream) {
    if (!dlogits || !h || !dh || !scratch || Bg < 1 || Vs < 0 || d < 4 || (d & 3) || ld < Vs || (ld & 3) || ldh < d) return -10;
    hipStream_t s = (hipStream_t)stream;
    if (Vs == 0) { if (!g_dry) HIPCHK(hipMemsetAsync(dh, 0, (size_t)Bg * d * sizeof(float), s)); return 0; }
    if (!E || !dE) return -10;
    const XformP nox = no_xform();
    {       // dE[v, :] = sum_b dlogits[b, v] h[b, :]
        GemmP g = gemm_defaults(Vs, d, Bg);
        g.lda = ld; g.ldb = ldh; g.A[0] = dlogits; g.B[0] = h;
        auto e = epi_linear<false, false, false>(dE, d);
        RET((launch_gemm<64, 64, 2, 2, true, true, XF_NONE, XF_NONE, false>(g, nox, e, nullptr, 1, s)));
    }
    int ns, kc;
    shard_split(Bg, Vs, d, &ns, &kc);
    {       // dh[b, :] = sum_v dlogits[b, v] E[v, :]
        GemmP g = gemm_defaults(Bg, d, (int)ld);
        g.Kv = Vs; g.lda = ld; g.ldb = d; g.A[0] = dlogits; g.B[0] = E;
        g.nsplit = ns; g.kchunk = kc;
        auto e = epi_linear<false, false, false>(scratch, d);
        e.c_split = (long)Bg * d;
        RET((launch_gemm<64, 64, 2, 2, false, true, XF_NONE, XF_NONE, false>(g, nox, e, nullptr, 1, s)));
    }
    LAUNCH(shard_slab_sum_kernel, dim3(cdiv((long)Bg * d / 4, ROW_THREADS)), dim3(ROW_THREADS), 0, s, scratch, ns, Bg, d / 4, dh,
           (long)d);
    return (int)hipGetLastError();
}

extern "C" int bsarec_shard_scatter_rows(const int64_t* ids_all, long n, int world, const float* const* stage_grads, long lo,
                                         long Vs, long V, int d, float* dE, void* stream) {
    if (!ids_all || n < 1 || Vs < 0 || d < 4 || (d & 3)) return -10;
    if (Vs == 0) return 0;
    if (!dE) return -10;
    ShardPtrs G;
    RET(shard_ptrs(G, stage_grads, world));
    const int d4 = d / 4;
    LAUNCH(shard_scatter_rows_kernel, dim3(cdiv(n * world * d4, 256)), dim3(256), 0, (hipStream_t)stream, ids_all, n, world, G, lo,
           Vs, V, d4, dE);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// sampled-softmax head of the catalogue-sharded step (include/bsarec_shard.h; sampled_softmax.h, catalogue_shard.h,
// lazy_adam.h)
// ---------------------------------------------------------------------------------------------
extern "C" int bsarec_shard_ssm_draw(uint64_t key, const uint64_t* state, int N, long V, const int64_t* pop_cum, int logq,
                                     int* cand, float* corr, int* lazy_count, void* stream) {
    if (!state || !cand || !corr || N < 1 || N > SSM_NEG_MAX || V < 2 || V > INT32_MAX) return -10;
    SsmP P = ssm_params(nullptr, 0, 1, 1, nullptr, nullptr, cand, corr, N, V, pop_cum, logq, 4, SSM_SLAB_MAX);
    P.state = state;
    LAUNCH(shard_ssm_draw_kernel, dim3(cdiv(N, ROW_THREADS)), dim3(ROW_THREADS), 0, (hipStream_t)stream, P, key, lazy_count);
    return (int)hipGetLastError();
}

extern "C" int bsarec_shard_ssm_gather(const int64_t* answers, int B, const int* cand, int N, const float* const* shards, int world,
                                       long rows_per, long V, int d, float* rows, void* stream) {
    if (!answers || !cand || !rows || B < 1 || N < 1 || N > SSM_NEG_MAX || rows_per < 1 || V < 1 || d < 4 || (d & 3)) return -10;
    if ((V + rows_per - 1) / rows_per > world) return -11;
    ShardPtrs S;
    RET(shard_ptrs(S, shards, world));
    const int d4 = d / 4;
    LAUNCH(shard_ssm_gather_kernel, dim3(cdiv(((long)B + N) * d4, 256)), dim3(256), 0, (hipStream_t)stream, answers, B, cand, N, S,
           rows_per, V, d4, rows);
    return (int)hipGetLastError();
}

extern "C" int bsarec_shard_ssm_head(const float* h, long ldh, int B, int Bg, const float* rows, const int64_t* answers,
                                     const int* cand, const float* corr, int N, long V, const int64_t* pop_cum, int logq, int d,
                                     float* logits, float* dlogits, float* loss_rows, void* stream) {
    if (!h || !rows || !answers || !cand || !corr || !logits || !dlogits || !loss_rows) return -10;
    if (B < 1 || Bg < B || N < 1 || N > SSM_NEG_MAX || V < 2 || V > INT32_MAX || d < 4 || (d & 3) || ldh < d) return -10;
    hipStream_t s = (hipStream_t)stream;
    SsmP P = ssm_params(h, ldh, B, Bg, rows, answers, cand, corr, N, V, pop_cum, logq, d, SSM_SLAB_MAX);
    P.logits = logits; P.dlogits = dlogits; P.loss_rows = loss_rows;
    LAUNCH(ssm_logits_kernel<true>, dim3(cdiv(N, SSM_TILE), cdiv(B, SSM_TILE)), dim3(ROW_THREADS), 0, s, P);
    HIPCHK(hipGetLastError());
    LAUNCH(ssm_ce_kernel<true>, dim3(B), dim3(ROW_THREADS), 0, s, P);
    return (int)hipGetLastError();
}

extern "C" int bsarec_shard_ssm_loss(const float* loss_rows_all, int Bg, float* loss, void* stream) {
    if (!loss_rows_all || !loss || Bg < 1) return -10;
    LAUNCH(loss_mean_kernel, dim3(1), dim3(ROW_THREADS), 0, (hipStream_t)stream, loss_rows_all, Bg, loss);
    return (int)hipGetLastError();
}

extern "C" long bsarec_shard_ssm_bwd_scratch_floats(int B, int N, int d) {
    if (B < 1 || N < 1 || N > SSM_NEG_MAX || d < 4) return -10;
    int ns, ch;
    ssm_split(N, SSM_SLAB_MAX, &ns, &ch);
    return (long)ns * B * d;
}

extern "C" int bsarec_shard_ssm_bwd(const float* dlogits, int B, int N, const float* h, long ldh, const float* rows, int d,
                                    float* dh, long lddh, float* grad_rows, float* scratch, void* stream) {
    if (!dlogits || !h || !rows || !dh || !grad_rows || !scratch) return -10;
    if (B < 1 || N < 1 || N > SSM_NEG_MAX || d < 4 || (d & 3) || ldh < d || lddh < d || (lddh & 3)) return -10;
    hipStream_t s = (hipStream_t)stream;
    SsmP P = ssm_params(h, ldh, B, B, rows, nullptr, nullptr, nullptr, N, 2, nullptr, 0, d, SSM_SLAB_MAX);
    P.dlogits = const_cast<float*>(dlogits); P.slab = scratch; P.G = grad_rows;
    const int tilesC = std::max(1, std::min(cdiv((long)B * d, ROW_THREADS), 64));
    LAUNCH(ssm_bwd_kernel<true>, dim3(P.tilesA + P.tilesB + tilesC), dim3(ROW_THREADS), 0, s, P);
    HIPCHK(hipGetLastError());
    LAUNCH(shard_slab_sum_kernel, dim3(cdiv((long)B * d / 4, ROW_THREADS)), dim3(ROW_THREADS), 0, s, scratch, P.nslab, B, d / 4, dh,
           lddh);
    return (int)hipGetLastError();
}

extern "C" int bsarec_shard_ssm_pull(const int64_t* answers_all, int B, int world, const int* cand, int N,
                                     const float* const* grad_rows, long lo, long Vs, long V, int d, float* dE, void* stream) {
    if (!answers_all || !cand || B < 1 || N < 1 || N > SSM_NEG_MAX || Vs < 0 || lo < 0 || V < 1 || d < 4 || (d & 3)) return -10;
    ShardPtrs G;
    RET(shard_ptrs(G, grad_rows, world));
    if (Vs == 0) return 0;
    if (!dE) return -10;
    const int d4 = d / 4;
    LAUNCH(shard_ssm_pull_kernel, dim3(cdiv(((long)N + (long)world * B) * d4, 256)), dim3(256), 0, (hipStream_t)stream, answers_all,
           B, world, cand, N, G, lo, Vs, V, d4, dE);
    return (int)hipGetLastError();
}

extern "C" int bsarec_shard_lazy_mark(const int64_t* ids_all, long nids, const int64_t* answers_all, int Bg, const int* cand, int N,
                                      long lo, long Vs, long V, int* mark, int* rows, int* count, int cap, void* stream) {
    if (!ids_all || !answers_all || !cand || nids < 0 || Bg < 1 || N < 1 || N > SSM_NEG_MAX || Vs < 0 || lo < 0 || V < 1) return -10;
    if (Vs == 0) return 0;
    if (!mark || !rows || !count || cap < (int)std::min<long>(Vs, nids + Bg + N)) return -10;
    LazyRows T;
    memset(&T, 0, sizeof(T));
    T.mark = mark; T.rows = rows; T.count = count; T.cap = cap;
    const int nb = (int)std::max<long>(1, std::min<long>(cdiv(nids + Bg + N, ROW_THREADS), 256));
    LAUNCH(shard_lazy_mark_kernel, dim3(nb), dim3(ROW_THREADS), 0, (hipStream_t)stream, ids_all, nids, answers_all, Bg, cand, N, lo,
           Vs, V, T);
    return (int)hipGetLastError();
}

extern "C" int bsarec_shard_lazy_adam(float* E, float* dE, float* m, float* v, int d, float b1, float b2, float eps, float wd,
                                      int* mark, const int* rows, const int* count, int cap, const void* state, void* stream) {
    if (!state || d < 4 || (d & 3) || cap < 0) return -10;
    if (cap == 0) return 0;
    if (!E || !dE || !m || !v || !mark || !rows || !count) return -10;
    ShardLazyAdamP A;
    memset(&A, 0, sizeof(A));
    A.w = E; A.g = dE; A.m = m; A.v = v; A.b1 = b1; A.b2 = b2; A.eps = eps; A.wd = wd;
    A.T.mark = mark; A.T.rows = const_cast<int*>(rows); A.T.count = const_cast<int*>(count); A.T.cap = cap; A.T.d4 = d / 4;
    const int nb = (int)std::min<long>(cdiv((long)cap * A.T.d4, ROW_THREADS), 1024);
    LAUNCH(shard_lazy_adam_kernel, dim3(nb), dim3(ROW_THREADS), 0, (hipStream_t)stream, (const uint64_t*)state, A);
    return (int)hipGetLastError();
}
