/*
 * rlt_hip.h - C ABI of librlt_hip.so: the MI355X (gfx950) implementation of the
 * ranked-list-truncation forward/backward hot path.
 *
 * The reference (Woody5962/Ranked-List-Truncation) has no FFI: its hot path sits behind Python
 * classes (models/__init__.py:1-12, utils/losses.py, utils/metrics.py).  This header is the
 * boundary those classes are re-implemented on: every entry point below replaces the arithmetic
 * of the reference lines it cites, and the Python mirror of the reference's classes
 * (ranked-list-truncation_amd/{models,utils}) binds exactly these symbols through ctypes.
 *
 * Conventions
 *   - all tensors are fp32 device pointers owned by the caller (labels are fp32 0/1 like the
 *     reference's), contiguous unless a leading dimension is given; nothing is allocated or
 *     freed here, workspaces are passed in; no host synchronisation, everything is ordered on
 *     `stream` (a hipStream_t passed as void*; NULL = the default stream);
 *   - return value: 0 ok; <0 argument error (RLT_E_*); >0 a hipError_t from the launch;
 *   - "position-major" activations: token row index t = s*B + b (position s outermost, list b
 *     innermost), i.e. a (S, B, E) tensor.  The reference keeps (B, S, E) and lets
 *     nn.TransformerEncoderLayer(batch_first=False) attend over axis 0 = the B lists at each
 *     position (models/AttnCut.py:9,17-18); position-major makes that attention axis contiguous.
 *     User-facing inputs/outputs stay in the reference's (B, S, F) / (B, S, 1) layout.
 */
#ifndef RLT_HIP_H
#define RLT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RLT_E_ARG      (-1)   /* null pointer / non-positive dimension            */
#define RLT_E_SHAPE    (-2)   /* dimension outside what the kernels support        */
#define RLT_E_WORKSPACE (-3)  /* workspace too small                               */
#define RLT_E_ALIGN    (-4)   /* pointer / leading dimension not 16-byte aligned   */

#define RLT_ABI_VERSION 5
int rlt_abi_version(void);
/* Precision of the MFMA contractions (the rlt_gemm* family, rlt_list_attention_*, the BiLSTM recurrences); inputs, outputs,
 * softmax, LayerNorm, gate nonlinearities, losses and every accumulator are fp32 in all modes.
 *   RLT_PRECISION_FP32   exact fp32 products on the f32 MFMA (157 TFLOP/s peak) - bit-for-bit fp32 fma chains
 *   RLT_PRECISION_BF16X6 fp32-FAITHFUL products on the bf16 MFMA (the split and the order of the products are implemented
 *                        once, in csrc/split6.h): every operand split exactly into three bf16 values
 *                        (8 + 8 + 8 significand bits: all 24 operand bits enter), six of the nine partial products kept,
 *                        each exact in the matrix pipe, fp32 accumulation; what is dropped is < 2^-23 of the product
 *                        in the worst case (under one fp32 ulp; 2^-29 typical).  Held to the FP32 mode's tolerances in
 *                        the tests.  Measured against fp64 (tools/gpu_probe.py x6_adversarial, profiles/r05_notes.md): at
 *                        or below the f32 MFMA kernels' error on random operands and on the adversarial classes `ones`
 *                        (low significand bits all ones, one sign) and `cancel` (sums cancelling by 1e4); on operands
 *                        that all share the SAME worst-case low bits (`worst-split`: 0x7F40, one sign) the roundings of
 *                        the small plane products into one running sum add coherently - 17x the f32 MFMA kernels' error
 *                        in a K ~ 10^6 contraction of the GEMM family, always inside the a-priori bound K 2^-24 of an
 *                        fp32 chain and two orders inside BASELINE.json's 1e-4; list attention keeps those products in an
 *                        accumulator of their own (head dim 16: all kernels; head dim 64: the forward at 512 lists and
 *                        more) and stays at or below the f32 kernels on that class too, its head-dim-64 gradients within
 *                        2x on every class (asserted; 4-8x until ABI 4).  Head dim 128 and shapes off the tile grid
 *                        run the exact-fp32 kernels in this mode.  THE DEFAULT: the reference computes in fp32 end to
 *                        end (models/AttnCut.py:8-14).
 *   RLT_PRECISION_BF16X3 opt-in fast mode: every operand split into bf16 hi + bf16 lo, a*b = hi*hi + hi*lo + lo*hi
 *                        (16 operand bits, ~2^-16 relative error per product, ~2x faster end to end; inside
 *                        BASELINE.json's 1e-4 bound but narrower than the reference's arithmetic)
 * Every entry point whose arithmetic or buffer layout depends on the mode takes an `int precision` argument: one of the
 * three codes above for THAT call, or RLT_PRECISION_DEFAULT = the process default (environment variable
 * RLT_PRECISION=fp32|bf16x6|bf16x3 at first use, else BF16X6; rlt_set_precision changes it and does nothing else).
 * The calls are re-entrant: two models in one process - or two threads - may run different modes side by side.  A
 * backward call and the workspace queries of a forward / backward pair must be given the forward call's precision (the
 * stash and workspace layouts depend on it).  Any other code: RLT_E_ARG (workspace queries: 0 bytes). */
#define RLT_PRECISION_DEFAULT (-1)
#define RLT_PRECISION_FP32   0
#define RLT_PRECISION_BF16X3 1
#define RLT_PRECISION_BF16X6 2
int rlt_set_precision(int mode);    /* sets the process default (not RLT_PRECISION_DEFAULT) */
int rlt_get_precision(void);        /* the process default */
/* human-readable name of an RLT_E_* / hipError_t code (static storage) */
const char* rlt_error_string(int code);

/* ------------------------------------------------------------------ reward losses (L1-L6)
 * utils/losses.py:48-68 (ChoopyLoss), :71-96 (AttnCutLoss), :194-233 (DivLoss) with the
 * reward matrix of :57-65/:81-89/:217-225 built from utils/metrics.py:85-101 in closed form
 * (prefix sums), fused: one pass over p and labels yields the per-list loss terms and
 * d(loss)/dp.
 *   p, labels: (B,S).  metric: RLT_METRIC_*.  kind: RLT_LOSS_*.  tau: reward temperature
 *   (DivLoss: 0.85 augmented / 1.0; AttnCutLoss: 0.95; ignored for EXPECT).
 *   dcg_coef: S floats log2(j+2) (utils/metrics.py:7), required for RLT_METRIC_DCG.
 *   loss_per_list: (B) un-normalised per-list terms; *loss_out = sum(loss_per_list)/B
 *   (KLDivLoss 'batchmean' / the reference's .div(B)).
 *   dp: (B,S) or NULL; receives d(loss_out)/dp (already divided by B).  With dp == NULL the call computes the loss only.
 *   S <= 1024 (RLT_E_SHAPE beyond).
 *   Alignment: when S % 4 == 0 every form of the pass reads and writes its rows 16 bytes at a time, so p, labels and each
 *   (B,S) output that is present - dp here, r_out / q_out of rlt_reward_matrix[_ex] - must be 16-byte aligned: RLT_E_ALIGN
 *   before any launch otherwise (also for rlt_loss_metrics).  Other S: 4-byte alignment suffices.
 */
#define RLT_METRIC_F1  0
#define RLT_METRIC_DCG 1
#define RLT_LOSS_EXPECT 0   /* ChoopyLoss:  -E_p[r]                 */
#define RLT_LOSS_CE     1   /* AttnCutLoss: -sum q log p            */
#define RLT_LOSS_KL     2   /* DivLoss kl:  KL(q || p)              */
#define RLT_LOSS_JS     3   /* DivLoss js:  JS(q, p)                */
int rlt_reward_loss(const float* p, const float* labels, const float* dcg_coef, int B, int S,
                    int metric, int kind, float tau,
                    float* loss_per_list, float* loss_out, float* dp, void* stream);
/* the same with the `penalty` argument of Metric_for_Loss.dcg (utils/metrics.py:94): the DCG gain of a non-relevant
 * document is penalty / log2(j+2); rlt_reward_loss is this call with the reference's default -1.  Ignored for F1. */
int rlt_reward_loss_ex(const float* p, const float* labels, const float* dcg_coef, int B, int S,
                       int metric, float penalty, int kind, float tau,
                       float* loss_per_list, float* loss_out, float* dp, void* stream);
/* reward matrix r (B,S) and its distribution q = softmax(r/tau) (either may be NULL):
 * the B*S python loop of utils/losses.py:217-228 on its own (tests, plots). */
int rlt_reward_matrix(const float* labels, const float* dcg_coef, int B, int S, int metric, float tau,
                      float* r_out, float* q_out, void* stream);
int rlt_reward_matrix_ex(const float* labels, const float* dcg_coef, int B, int S, int metric, float penalty, float tau,
                         float* r_out, float* q_out, void* stream);
/* Training-step form (run.py:126 + :141-145 in ONE pass over p and labels): everything rlt_reward_loss_ex produces, plus
 * the cut metrics of rlt_cut_metrics_ex on the same rows while they are in registers - k_out (B) int32 = argmax_j p + 1 (first
 * maximum), f1_out / dcg_out (B) float64 (DCG with `metric_penalty`, utils/metrics.py:27), sums[0..1] = their batch sums.
 * loss_out = (sum of the per-list terms)/B from a float64 sum.  All outputs required except dp.  Two launches: the pass
 * (when S % 4 == 0, S <= 384 and dp is given: two ranked lists per wavefront - one per 32-lane half - or four - one per
 * 16-lane row, where rounds of 64 positions waste fewer lanes than rounds of 128: S in 1..64, 129..192 and, for F1, 257..320;
 * one list per wavefront otherwise; a grid
 * sized to the chip striding over the lists; every wavefront leaves its float64 partial sums in ws) and a one-workgroup
 * fixed-order reduction of those partials (deterministic).  The float64 DCG coefficients 1/log2(j+2) (utils/metrics.py:7) and
 * their prefix sums are read from `dcg_table`, CALLER memory of rlt_dcg_table_bytes() bytes (8-byte aligned) that
 * rlt_dcg_table_init has filled once (one small launch on `stream`; the table does not depend on B, S or the metric and may be
 * shared by every later call on that device): like every entry point of this library the call allocates nothing, never
 * synchronises with the host and may be captured into a graph.  (ABI 3 built the table itself on first use: a hidden
 * hipMalloc + synchronous copy.)
 * ws: rlt_loss_metrics_workspace(B) bytes.
 * Algorithmic bytes per list: read p, labels 8S, write dp 4S + 24 B of results (3.6 KB at S = 300). */
size_t rlt_dcg_table_bytes(void);
int rlt_dcg_table_init(void* table, size_t table_bytes, void* stream);
size_t rlt_loss_metrics_workspace(int B);
int rlt_loss_metrics(const float* p, const float* labels, const float* dcg_coef, int B, int S,
                     int metric, float penalty, int kind, float tau, double metric_penalty,
                     float* loss_per_list, float* loss_out, float* dp,
                     int32_t* k_out, double* f1_out, double* dcg_out, double* sums,
                     const void* dcg_table, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ reward losses for any cut reward (csrc/reward_any.hip)
 * The reward r[b,k] - the value of cutting list b after position k, k = 1..S - as an ARGUMENT: a spec whose reward is built
 * from the labels in registers, or a (B,S) matrix the caller supplies.  The F1 / DCG entry points above are not touched.
 *
 * rlt_reward_spec is a HOST struct, read at call time; its scalars travel as kernel arguments.
 *   grade g_j: the label rounded to the nearest integer and clamped to 0..n_grades-1; NaN gives 0.
 *   RLT_REWARD_FBETA: a document is relevant iff label >= 1; c_k = relevant documents among the first k, N = in the list;
 *     r_k = (1 + beta^2) c_k / (beta^2 N + k), 0 when c_k == 0 (F_beta of precision c_k / k and recall c_k / N).
 *   RLT_REWARD_GAIN: cum_k = sum_{j<=k} gain[g_j] d_j, a float64 prefix sum; r_k = cum_k, or with `normalize`
 *     r_k = cum_k / ideal (0 when ideal <= 0), ideal = sum_g gain[g] (D[a_g + n_g] - D[a_g]) over the grades of positive gain in
 *     descending gain (ties: the higher grade first), n_g = the list's documents of grade g, a_g = those of the grades taken
 *     before it, D = the float64 prefix sum of d: the value of the list sorted by gain, which is the largest value of any
 *     ordering when d is non-negative and non-increasing.  gain = {penalty, 1} with discount == NULL is Metric_for_Loss.dcg.
 *   Both are formed in float64 and rounded to fp32 once.
 * Graded labels enter through THIS interface only: the F1 / DCG kernels above test label == 1, where a grade 2 reads as
 * non-relevant.
 *
 * rlt_reward_spec_matrix: r_out and / or q_out = softmax(r / tau) as (B,S) fp32 (the counterpart of rlt_reward_matrix_ex).
 * rlt_reward_any_loss: the loss of rlt_reward_loss_ex (kind RLT_LOSS_*, the same definitions and / B scaling) on that reward.
 *   Exactly one reward source: labels + spec (the reward is never written), or r_in, (B,S) fp32, assumed finite and not checked
 *   (labels and spec NULL); anything else RLT_E_ARG.  q = softmax(r / tau) with the row maximum subtracted; q, the loss terms
 *   and dp are formed in float64 and rounded to fp32 where they are stored.  dp (B,S) may be NULL.  Per-list outputs, each
 *   may be NULL: loss_per_list fp32; k_out int32 = first maximum of p, plus 1; r_k fp32 = the reward at that cut; r_best fp32
 *   and best_k int32 = the row's largest reward over k = 1..S and its first position.  sums: 4 float64 or NULL = sum r_k, sum
 *   r_best, the number of lists with r_k == r_best, B.  loss_out (or NULL) = (sum of the per-list terms) / B from a float64 sum.
 *   dcg_table: as for rlt_loss_metrics; read only by a GAIN spec with discount == NULL (may be NULL otherwise).
 *   ws: rlt_reward_any_workspace(B) bytes, 8-byte aligned (0 for B <= 0; never smaller for a larger B).
 * Layout as rlt_loss_metrics: a wavefront owns whole lists, four, two or one by S and S % 4; rows of S % 4 == 0 floats are read
 * and written 16 bytes at a time, so p, labels, r_in, dp, r_out and q_out must then be 16-byte aligned (RLT_E_ALIGN).  S in
 * 1..1024 (RLT_E_SHAPE beyond).  Two launches: the pass (every workgroup leaves one float64 record in ws) and a one-workgroup
 * fixed-order reduction.  No atomics, no allocation, no host synchronisation: two calls give the same bits.  Errors before any
 * launch: RLT_E_ARG (p, ws or both / neither reward source; non-positive B or S; kind or family outside their codes; beta <= 0;
 * n_grades outside 2..8; a non-finite gain; tau <= 0; a GAIN spec with neither discount nor dcg_table), RLT_E_SHAPE,
 * RLT_E_ALIGN, RLT_E_WORKSPACE.
 * Algorithmic bytes per list: read 8 S, write dp 4 S + up to 20 B of results. */
#define RLT_REWARD_FBETA 0
#define RLT_REWARD_GAIN  1
#define RLT_REWARD_MAX_GRADES 8
typedef struct {
    int   family;       /* RLT_REWARD_*                                                        */
    int   n_grades;     /* GAIN: 2..8                                                          */
    int   normalize;    /* GAIN: 1 = divide by the list's ideal value                          */
    float beta;         /* FBETA: > 0                                                          */
    float gain[RLT_REWARD_MAX_GRADES];   /* GAIN: gain of a document of grade g                */
    const float* discount;               /* GAIN: device, S floats d_j, or NULL = 1/log2(j+2)
                                            taken from dcg_table                               */
} rlt_reward_spec;
int rlt_reward_spec_matrix(const float* labels, int B, int S, const rlt_reward_spec* spec, float tau, const void* dcg_table,
                           float* r_out, float* q_out, void* stream);
size_t rlt_reward_any_workspace(int B);
int rlt_reward_any_loss(const float* p, const float* labels, const rlt_reward_spec* spec, const float* r_in, int B, int S,
                        int kind, float tau, float* loss_per_list, float* loss_out, float* dp,
                        int32_t* k_out, float* r_k, float* r_best, int32_t* best_k, double* sums,
                        const void* dcg_table, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ evaluation in any cut reward (csrc/reward_eval.hip)
 * What the truncation baselines, the cut report, the cut sweep and the paired comparison need from a reward row, in one pass.
 * The reward: exactly one source, as for rlt_reward_any_loss - labels + spec, or r_in (B,S) fp32 (labels and spec NULL).
 *   r[b,k], k = 1..S, is bit for bit the fp32 value rlt_reward_spec_matrix writes for the same labels and spec (one device
 *   text builds both: csrc/reward_form.h), or r_in itself; r[b,0] = 0: cutting before the first document keeps nothing, the
 *   k = 0 entry of rlt_truncation_curves.
 * Cuts: k_in (B,T) int32, row-major, 0 <= T <= 64; T = 0 (k_in is then not read) means no cuts.  The T columns are the cuts of
 *   T rules or systems on the same lists: the (B,T) output of rlt_cut_sweep, or the k of rlt_cut_report.  A cut outside 0..S is
 *   clamped into that range and counted.
 * Per-list outputs (each may be NULL):
 *   r_at (B,T) fp32 = r[b, k_in[b,t]];
 *   better (B,T) int32 = the number of cuts k in kmin..S with r[b,k] strictly greater than r_at[b,t]; kmin = 0 with allow_empty,
 *   otherwise 1;
 *   best (B) fp32 and best_k (B) int32 = the row's largest reward over kmin..S and its first position: np.argmax on the
 *   (S+1)-entry row, so k = 0 wins a tie with allow_empty.
 * Split outputs (float64, 8-byte aligned, each may be NULL; accumulate = 1 ADDS this batch, 0 overwrites):
 *   curve (S+1) = sum over lists of r[b,k], k = 0..S (entry 0 is 0): Fixed-k at every k at once, and Greedy-k;
 *   best_hist (S+1) = counts of best_k;
 *   sums (3 + 3T): [0] the number of lists, [1] sum best, [2] the number of clamped cuts, then per t: sum r_at,
 *   #(r_at == best), sum better.
 * dcg_table: as for rlt_reward_any_loss.  ws: rlt_reward_eval_workspace(B, S, T) bytes, 8-byte aligned (0 for B <= 0, S outside
 * 1..1024 or T outside 0..64; never smaller for a larger B).
 * Layout as rlt_reward_any_loss: a wavefront owns whole lists, four, two or one by S and S % 4; rows of S % 4 == 0 floats are
 * read 16 bytes at a time, so labels and r_in must then be 16-byte aligned.  The reward row stays in registers, the sums per
 * position are kept per lane, the cuts are served from a copy of the row in LDS.  Two launches (one without split outputs): the
 * pass (every workgroup leaves one float64 record in ws) and a fixed-order column reduction.  No atomics, no allocation, no host
 * synchronisation: two calls give the same bits.  Errors before any launch, in this order: RLT_E_ARG (both or neither reward
 * source; non-positive B or S; T outside 0..64; T > 0 with k_in NULL; r_at or better with T = 0; every output NULL; a spec
 * outside its ranges, a GAIN spec with neither discount nor dcg_table; ws NULL), RLT_E_SHAPE (S > 1024), RLT_E_ALIGN (rows; 8
 * bytes for curve, best_hist, sums, ws and the table; 4 for the rest), RLT_E_WORKSPACE.
 * Algorithmic bytes per list: read 4 S + 4 T, write up to 8 T + 8. */
size_t rlt_reward_eval_workspace(int B, int S, int T);
int rlt_reward_eval(const float* labels, const rlt_reward_spec* spec, const float* r_in, int B, int S,
                    const int32_t* k_in, int T, int allow_empty, const void* dcg_table, int accumulate,
                    float* r_at, int32_t* better, float* best, int32_t* best_k,
                    double* curve, double* best_hist, double* sums,
                    void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ multi-task terms (L7-L8)
 * utils/losses.py:99-141 (RerankLoss) and nn.BCELoss of :177,:187 (MtCutLoss).
 * rlt_mt_terms: one pass over the rerank scores and/or class probabilities (either may be NULL)
 * accumulating the batch-wide sums; then finalises on device (no host sync):
 *   terms[0] = rerank hinge  max(0, mean_{y==0} s - mean_{y==1} s + margin), 0 if a class is empty
 *   terms[1] = BCE mean over B*S (log clamped at -100 like torch)
 *   terms[2] = d hinge / d s for y==1 entries (= -1/n_pos if active else 0)
 *   terms[3] = d hinge / d s for y==0 entries (= +1/n_neg if active else 0)
 * ws: at least rlt_mt_terms_workspace(B,S) bytes.
 * rlt_mt_terms_bwd: d_rerank (B,S) = w_r * terms[2|3]; d_class (B,S) = w_c * dBCE/dc / (B*S);
 * both scaled by *gscale (device scalar, NULL = 1).
 */
size_t rlt_mt_terms_workspace(int B, int S);
int rlt_mt_terms(const float* rerank, const float* cls, const float* labels, int B, int S, float margin,
                 float* terms, void* ws, size_t ws_bytes, void* stream);
int rlt_mt_terms_bwd(const float* cls, const float* labels, const float* terms, int B, int S,
                     float w_rerank, float w_class, const float* gscale,
                     float* d_rerank, float* d_class, void* stream);
/* out[0] = sum_i w[i] * x[i] for n <= 8 device scalars (combining cut / rerank / class terms) */
int rlt_weighted_sum(const float* const* x, const float* w, int n, float* out, void* stream);

/* ------------------------------------------------------------------ cut metrics (E1-E3)
 * run.py:137-142 (k = argmax+1) and utils/metrics.py:15-38 (Metric.f1 / Metric.dcg at k).
 * p, labels: (B,S).  k_out (B) int32; f1_out, dcg_out (B) float64 per list (the reference
 * averages them over the batch on the host); any output may be NULL.
 * If k_in != NULL the metrics are evaluated at those cut positions instead of the argmax.
 * sums (2 doubles, may be NULL) receives sum_i f1_i, sum_i dcg_i.
 */
int rlt_cut_metrics(const float* p, const float* labels, const int32_t* k_in, int B, int S,
                    int32_t* k_out, double* f1_out, double* dcg_out, double* sums, void* stream);
/* the same with Metric.dcg's `penalty` argument (utils/metrics.py:27; rlt_cut_metrics uses the default -1) */
int rlt_cut_metrics_ex(const float* p, const float* labels, const int32_t* k_in, int B, int S, double penalty,
                       int32_t* k_out, double* f1_out, double* dcg_out, double* sums, void* stream);

/* Task metrics of utils/metrics.py:40-76 (section 8f row N4), per list in float64:
 *   dcg_out[b] = taskr_metric's DCG of list b re-ordered by descending pred (relevant +1/log2(i+2), else -1/log2(i+2));
 *   auc_out[b] = taskc_metric's ROC AUC of pred against labels (ties 1/2), or -1 for a list with a single class (the
 *                reference skips those);
 *   sums (3 doubles, may be NULL) = sum of dcg_out, sum of the valid auc_out, number of valid lists.
 * labels, pred (B,S), S <= 1024. */
int rlt_task_metrics(const float* labels, const float* pred, int B, int S,
                     double* dcg_out, double* auc_out, double* sums, void* stream);

/* ------------------------------------------------------------------ rerank, then truncate (csrc/rerank.hip)
 * A stable per-list sort by descending pred (B,S) that carries up to four companion (B,S) fp32 arrays along - the labels, the
 * retrieval score, the cut distribution, the class probability - so that every evaluation pass above and below runs unchanged
 * on the re-ranked lists.
 * The order of list b is exactly that of np.argsort(-pred[b], kind="stable") on float32: values descend; equal values keep
 * their original order, and +0.0 == -0.0 is a tie; every NaN comes after every number, in original order; +inf is first and
 * -inf last among the numbers.  This is a TOTAL order - every element is sorted by one 64-bit key, (an integer image of the
 * value, NaN mapped behind -inf) << 32 | original index, and the keys of a list are distinct - so perm is a permutation and
 * rank its inverse for ANY input bits.  (The `pi > pj || (pi == pj && i < j)` rank inside rlt_task_metrics is not a
 * permutation when NaNs are present; on NaN-free input the two orders agree.)
 * Outputs (each may be NULL, but not all of them with n == 0):
 *   perm (B,S) int32: perm[b,i] = original index of the document at new position i;
 *   rank (B,S) int32: rank[b,j] = new position of original document j, the inverse of perm;
 *   sorted_pred (B,S): sorted_pred[b,i] = pred[b,perm[b,i]], the same bits (NaN payloads and the sign of zero included);
 *   dst[t] (B,S), t < n: dst[t][b,i] = src[t][b,perm[b,i]], the same bits.
 * src, dst: HOST arrays of n device pointers, 0 <= n <= 4 (not read for n == 0).  No dst[t] or sorted_pred may overlap pred or
 * any src[t]: the caller's duty, not checked.
 * S in 1..1024, any B >= 1 (64-bit element offsets).  A group of 16, 32 or 64 lanes owns a list (S <= 64: four lists per
 * wavefront, S <= 128: two, else one), four wavefronts per workgroup; the keys stay in registers through a bitonic network
 * (exchanges inside a lane and between lanes), perm goes through the wavefront's LDS and the companions are gathered through it.
 * One launch, no workspace, no atomics, no allocation, no host synchronisation: two calls give the same bits.
 * Errors before any launch, in this order: RLT_E_ARG (pred NULL; non-positive B or S; n outside 0..4; n > 0 with src or dst
 * NULL, or a NULL entry among their first n; nothing to write), RLT_E_SHAPE (S > 1024), RLT_E_ALIGN (any pointer off 4 bytes:
 * rows are read and written 4 bytes at a time, no 16-byte requirement).
 * Algorithmic bytes per list: read 4 S (1 + n), write up to 4 S (3 + n). */
int rlt_rerank_lists(const float* pred, int B, int S, const float* const* src, float* const* dst, int n,
                     int32_t* perm, int32_t* rank, float* sorted_pred, void* stream);

/* ------------------------------------------------------------------ pairwise ranking losses (csrc/pair_rank.hip)
 * RankNet and LambdaRank on the scores of a rerank head: a pairwise logistic loss over the documents of each list, its gradient,
 * and - as a by-product of the same O(S^2) pass - the counting rank of every document.  score, labels: (B,S) fp32.
 * Definitions for list b:
 *   grade g_i: the rule of rlt_reward_spec - the label rounded to the nearest integer and clamped to 0..n_grades-1; NaN gives 0.
 *     n_grades in 2..8.  G_i = gain[g_i]; gain is a HOST array of n_grades floats, NULL = 2^g - 1.
 *   counting rank pi_i = #{ j : s_j > s_i, or s_j == s_i and j < i }, 0-based (+0 == -0 is a tie).  On NaN-free scores this is
 *     the inverse permutation rlt_rerank_lists writes as `rank`.  (A NaN compares false with everything: with NaNs present the
 *     counting rank is not a permutation, see below.)
 *   D(r) = 1 / log2(r + 2) from dcg_table, the float64 table of rlt_dcg_table_init (8-byte aligned; read by RLT_PAIR_LAMBDARANK
 *     only).  ideal: the list's ideal value as rlt_reward_spec defines it for a GAIN spec with the table's discount.
 *   pairs: all (i, j) with g_i > g_j; n_pairs[b] is their count.
 *   weight: RLT_PAIR_RANKNET w_ij = 1; RLT_PAIR_LAMBDARANK w_ij = |G_i - G_j| * |D(pi_i) - D(pi_j)|, divided by ideal when
 *     `normalize` is set and ideal > 0.
 *   x = sigma (s_i - s_j); l_ij = w_ij softplus(-x), softplus(-x) = max(-x, 0) + log1p(exp(-|x|)); lam_ij = -sigma w_ij sigmoid(-x).
 *   loss_per_list[b]: RANKNET sum l_ij / n_pairs, LAMBDARANK sum l_ij; 0, with a zero gradient, when n_pairs == 0.
 *   loss_out = (sum over lists) / B from a float64 sum in a fixed order.
 *   dscore[b,i] = gscale / B * (1 / n_pairs for RANKNET) * (sum_{j: g_i > g_j} lam_ij - sum_{j: g_j > g_i} lam_ji): the LambdaRank
 *     gradient (the weights are constants); for RANKNET the true gradient of loss_out.  gscale: device scalar, NULL = 1; it
 *     scales dscore and nothing else.
 *   A list with a NaN score has NaN loss_per_list and a NaN row of dscore, and makes loss_out NaN; its n_pairs is still exact
 *     and its rank_out follows the definition above.  Every other list's outputs are the bits they would be without it.
 * Outputs, each may be NULL but not all of them: loss_per_list (B) fp32, loss_out (1) fp32, dscore (B,S) fp32, rank_out (B,S)
 * int32, n_pairs (B) int32.
 * Arithmetic: s_i - s_j, x, the weight and every sum over j are float64 (the discount differences cancel); exp, log1p and the
 * sigmoid's division are fp32 on the fp32 head of |x|, its float64 tail applied as a first-order factor, so exp(-|x|) keeps its
 * relative accuracy on the saturated branch.  Pairs with g_i == g_j cost no transcendental.
 * Layout: S in 1..1024 (RLT_E_SHAPE beyond), any B >= 1 (64-bit element offsets).  A group of lanes inside one wavefront owns a
 * list: 16 lanes for S <= 64 (four lists per wavefront), 32 for S <= 128 (two), the whole wavefront beyond; a lane owns the
 * documents hl, hl + L, ... (4 of them up to S = 256, 8 up to 512, 16 up to 1024).  A workgroup has 4 wavefronts (2 for S > 512):
 * 16, 8, 4, 4 or 2 lists per workgroup.  The list's scores, grades and D(pi) live in the wavefront's LDS and are read as
 * broadcasts; a lane walks all j for its own documents and forms its own dscore from both sides of each of its pairs: no sum
 * crosses lanes for dscore, no atomics.  The grid is sized to the chip and strides over the lists.  One launch for the pass (every
 * workgroup leaves one float64 record in ws), then - only when loss_out is given - a one-workgroup fixed-order reduction.  No
 * allocation, no host synchronisation, capturable into a graph: two calls give the same bits.
 * ws: rlt_pair_rank_workspace(B, S) bytes, 8-byte aligned (0 for B <= 0 or S outside 1..1024; never smaller for a larger B).
 * Errors before any launch, in this order: RLT_E_ARG (score, labels or ws NULL; non-positive B or S; kind outside its codes;
 * sigma not finite or <= 0; n_grades outside 2..8; a non-finite gain; RLT_PAIR_LAMBDARANK with dcg_table NULL; every output NULL),
 * RLT_E_SHAPE (S > 1024), RLT_E_ALIGN (ws or dcg_table off 8 bytes; any other device pointer off 4: rows are read and written 4
 * bytes at a time, no 16-byte requirement), RLT_E_WORKSPACE.
 * Algorithmic bytes per list: read 8 S, write up to 8 S + 8; S^2 pair visits, of which the pairs of unequal grade (twice
 * n_pairs: each is seen from both sides) pay one exp and a division, half of them also one log1p. */
#define RLT_PAIR_RANKNET    0
#define RLT_PAIR_LAMBDARANK 1
size_t rlt_pair_rank_workspace(int B, int S);
int rlt_pair_rank_loss(const float* score, const float* labels, int B, int S, int kind, float sigma,
                       const float* gain, int n_grades, int normalize,
                       const void* dcg_table, const float* gscale,
                       float* loss_per_list, float* loss_out, float* dscore,
                       int32_t* rank_out, int32_t* n_pairs, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ truncation baselines
 * The reference's Baseline/ notebooks (Oracle, Fixed-k, Greedy-k, Truncation_analysis) from one pass over labels (B,S),
 * 0/1 in rank order, S in 1..1024.  With c_k = the sum of the first k labels and N = the sum of the list, for k = 1..S:
 *   F1@k  = 2 p r / (p + r), p = c_k / k, r = c_k / N (0 if N = 0), 0 if p + r = 0: float64 in cal_F1's operation order with
 *           correctly rounded division, so exactly tied values are bit-identical as in Python;
 *   DCG@k = sum_{i<k} (label == 1 ? 1 : penalty) / log2(i + 2) in float64 (cal_DCG; the notebooks' penalty is -1);
 *   k = 0 is an entry of every curve with value 0.
 *   curves (3 x (S+1) float64, required): row 0 = sum over lists of F1@k, row 1 = of DCG@k, row 2 = of c_k, k = 0..S;
 *   best_f1 / best_dcg (B) float64: each list's maximum over k = 0..S, best_f1_k / best_dcg_k (B) int32 its first maximum
 *           (np.argmax); each may be NULL;
 *   sums (3 doubles, may be NULL): sum of best F1, sum of best DCG, number of lists.
 * accumulate = 1 ADDS this batch into curves and sums (a split streams through batch by batch with no host synchronisation),
 * 0 overwrites them.  dcg_table: as for rlt_loss_metrics (8-byte aligned).  ws: rlt_truncation_curves_workspace(B, S) bytes,
 * 8-byte aligned (0 for B <= 0: B must be positive, as for the other metric entry points).  Two launches: the pass (a
 * wavefront owns whole lists - four per wavefront at S <= 64 - and keeps its per-k sums in registers; one float64 record per
 * workgroup in ws) and a fixed-order column reduction of the records; no atomics, bitwise reproducible.
 * Algorithmic bytes per list: read labels 4S (+ 24 B of per-list results). */
size_t rlt_truncation_curves_workspace(int B, int S);
int rlt_truncation_curves(const float* labels, int B, int S, double penalty, const void* dcg_table, int accumulate,
                          double* curves, double* best_f1, int32_t* best_f1_k, double* best_dcg, int32_t* best_dcg_k,
                          double* sums, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ cut report
 * What a trained model does with every list of a split, and the arithmetic of the reference's `--draw` figure (run.py:188,
 * 242-298), from one pass over the model's output p and - when there are any - the labels (B,S); S in 1..1024.
 *   rule   RLT_CUT_ARGMAX: p is (B,S), k = first maximum + 1 (run.py:141-142);
 *          RLT_CUT_PAIR:   p is (B,S,2), BiCut's rule (run.py:131-136): k = S when no position prefers class 0, otherwise the
 *                          first such position + 1; a tie goes to class 0; p 8-byte aligned.
 *   labels NULL = label-free mode: only k, p_k, margin, hist, pred_curve and sums[4] are produced (every labelled output must
 *          then be NULL; metric, penalty, metric_penalty, tau, dcg_coef and dcg_table are not read).
 * Per-list outputs (B each, each may be NULL):
 *   k int32; p_k fp32 = the winning value (PAIR: the class-0 value at position k - 1); margin fp32 = the maximum minus the
 *   runner-up, 0 for S = 1 (PAIR: class 0 minus class 1 at position k - 1, negative when no position prefers class 0);
 *   f1, dcg float64 = F1@k and DCG@k (DCG with metric_penalty), bit-identical to rlt_cut_metrics_ex;
 *   best_f1, best_f1_k, best_dcg, best_dcg_k = the list's best over k = 0..S and its first maximum, bit-identical to
 *   rlt_truncation_curves with penalty = metric_penalty;
 *   better int32 = the number of cut positions 1..S whose reward is strictly greater than the reward at k, the reward r
 *   being bit for bit the fp32 one of rlt_reward_matrix_ex(labels, dcg_coef, metric, penalty) (dcg_coef: fp32 log2(j + 2),
 *   S entries, required for RLT_METRIC_DCG).
 * Split outputs (float64, 8-byte aligned, each may be NULL; accumulate = 1 ADDS this batch, 0 overwrites):
 *   hist (S+1) = counts of k;  pred_curve (S) = sum over lists of softmax_j(p_j / sharpen) (PAIR: of the class-0 column);
 *   reward_curve (S) = sum over lists of softmax_j(r_j / tau);  sums (5) = sum f1, sum dcg (both in rlt_cut_metrics_ex's own
 *   order: bit-identical to its sums), sum best_f1, sum best_dcg, number of lists.
 * Both softmaxes subtract the row maximum and are formed in float64 (tau, sharpen > 0; the reference draws tau = 0.9 and
 * sharpen = tau * 1e-3).  The reference computes exp(p / 9e-4) in fp32 with no subtraction: it overflows once a p exceeds about
 * 0.08 and the figure is NaN from there; where the reference is finite this pass agrees with it to the reference's own fp32
 * rounding, and it stays finite everywhere else.  The `norm_s[-3:] = norm_s[-4]` overwrite of run.py:283 is presentation and
 * not applied here.
 * dcg_table: as for rlt_loss_metrics.  ws: rlt_cut_report_workspace(B, S) bytes, 8-byte aligned (0 for B <= 0 or S outside
 * 1..1024): one float64 record per workgroup, and F1@k / DCG@k per list for the ordered sums.  Three launches (two without
 * labels or sums): the pass (a wavefront owns whole lists - four per wavefront at S <= 64 - with its per-position sums in
 * registers), a fixed-order column reduction of the records, and the ordered sums; no atomics, no allocation, no host
 * synchronisation, bitwise reproducible.  Algorithmic bytes per list: 8 S read (4 S without labels). */
#define RLT_CUT_ARGMAX 0
#define RLT_CUT_PAIR   1
size_t rlt_cut_report_workspace(int B, int S);
int rlt_cut_report(const float* p, int rule, const float* labels, const float* dcg_coef, int B, int S, int metric, float penalty,
                   double metric_penalty, double tau, double sharpen, const void* dcg_table, int accumulate,
                   int32_t* k, float* p_k, float* margin, double* f1, double* dcg, double* best_f1, int32_t* best_f1_k,
                   double* best_dcg, int32_t* best_dcg_k, int32_t* better, double* hist, double* pred_curve, double* reward_curve,
                   double* sums, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ cut sweep
 * T threshold cut rules at once from one read of a per-position value array v and of the labels: where on the
 * effectiveness / cost trade-off a cut operates.  (The reference has no counterpart: it only ever takes the argmax.)
 *   v          (B,S) fp32 read at element stride v_stride = 1 or 2 (2: the class-0 column of BiCut's (B,S,2) output); S in
 *              1..1024, B >= 1.
 *   thresholds T float64 in device memory, 1 <= T <= 64, in any order; 8-byte aligned.
 *   rule, positions j = 1..S, v widened to float64 before every comparison, a NaN compares false:
 *     RLT_SWEEP_QUANTILE    v is a cut distribution.  C_j = the float64 inclusive prefix sum of v;
 *                           k = 1 + #{ j in 1..S-1 : C_j < tau * C_S }, in 1..S: the smallest k whose mass reaches the share tau
 *                           (tau * C_S is one float64 multiply).  A list whose total is 0 or NaN gets k = 1, because every
 *                           comparison is false; so does every tau <= 0 on non-negative v.
 *     RLT_SWEEP_FIRST_BELOW v holds retrieval scores.  k = the number of leading positions with v_j >= tau, in 0..S.  k = 0
 *                           keeps nothing and every metric of that list is 0: the k = 0 entry of rlt_truncation_curves.
 *     RLT_SWEEP_FIRST_ABOVE v is a per-position stop probability.  k = the first j with v_j >= tau, S if there is none.
 * Outputs (either may be NULL, not both):
 *   k     (B,T) int32: the cut of every list at every threshold;
 *   curve (RLT_SWEEP_COLS,T) float64, 8-byte aligned: sums over the lists - accumulate = 1 ADDS this batch, 0 overwrites - of
 *         row 0: k;  1: F1@k;  2: DCG@k with metric_penalty;  3: precision c_k / k (0 at k = 0);  4: recall c_k / N (0 if N = 0);
 *         5: F_beta = ((1 + beta^2) P) R / (beta^2 P + R), 0 if the denominator is 0;  6: [k == S] (nothing cut);  7: 1 (lists),
 *         c_k = the number of labels equal to 1 in the first k positions, N = their number in the list.
 * F1@k is formed from the integers (c_k, N, k) in rlt_cut_metrics_ex's operation order: bit-identical to that entry point for
 * k >= 1 on 0/1 labels.  DCG@k = sum_{j <= k} (label == 1 ? 1 : metric_penalty) * (the table's 1 / log2(j + 1)) from a prefix scan in position order
 * (64-lane scans carried across rounds of 64), not rlt_cut_metrics' lane-strided sum: equal to it to float64 rounding, not to
 * bits.  Rows 0, 6 and 7 are sums of integers and exact below 2^53.  The sums over lists go lane by lane, wavefront by
 * wavefront, then through one float64 record per workgroup and a fixed-order column reduction.
 * labels NULL = label-free mode (inference): curve must be NULL and k non-NULL; only the cuts are produced, and dcg_table, ws,
 * metric_penalty and beta are not read.  (labels with curve NULL does the same.)
 * dcg_table: as for rlt_loss_metrics.  ws: rlt_cut_sweep_workspace(B, S, T) bytes, 8-byte aligned (0 for B <= 0, S outside
 * 1..1024 or T outside 1..64; never smaller for a larger B).  Errors before any launch: RLT_E_ARG (v or thresholds NULL,
 * non-positive B, S or T, rule outside 0..2, v_stride outside {1,2}, both outputs NULL, curve without labels, dcg_table or ws),
 * RLT_E_SHAPE (S > 1024, T > 64), RLT_E_ALIGN, RLT_E_WORKSPACE.  Two launches (one without curve): the pass - a wavefront owns
 * whole lists, the count that defines k is taken per threshold over the wavefront, then the T thresholds are finished one lane
 * each from the count and DCG prefixes in LDS - and the reduction of the records; no atomics, no allocation, no host
 * synchronisation, bitwise reproducible.  Algorithmic bytes per list: 8 S read (4 S without labels) + 4 T of cuts. */
#define RLT_SWEEP_QUANTILE    0
#define RLT_SWEEP_FIRST_BELOW 1
#define RLT_SWEEP_FIRST_ABOVE 2
#define RLT_SWEEP_COLS        8
size_t rlt_cut_sweep_workspace(int B, int S, int T);
int rlt_cut_sweep(const float* v, int v_stride, int rule, const double* thresholds, int T,
                  const float* labels, int B, int S, double metric_penalty, double beta,
                  const void* dcg_table, int accumulate,
                  int32_t* k /* (B,T) or NULL */, double* curve /* (RLT_SWEEP_COLS,T) or NULL */,
                  void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ dense contraction (M2-M7)
 * C[M,N] (+)= op(A) * op(B) (+ bias[N] + bias2[N]), optional ReLU.  fp32 in, fp32 accumulate on
 * the f32 MFMA (exact fp32 products, v_mfma_f32_32x32x2_f32).
 *   ta = 0: A stored [M,K] (lda >= K);  ta = 1: A stored [K,M] (lda >= M)
 *   tb = 0: B stored [K,N] (ldb >= N);  tb = 1: B stored [N,K] (ldb >= K)   (nn.Linear: tb = 1)
 *   flags: RLT_GEMM_RELU, RLT_GEMM_ACCUMULATE (C += ...).
 * Replaces the nn.Linear / in_proj / out_proj / LSTM input-projection matmuls of
 * models/AttnCut.py:8-14 and their backward.  ws: rlt_gemm_workspace(...) bytes (split-K partials).
 */
#define RLT_GEMM_RELU       1
#define RLT_GEMM_ACCUMULATE 2
size_t rlt_gemm_workspace(int ta, int tb, int M, int N, int K);
int rlt_gemm(int ta, int tb, int M, int N, int K,
             const float* A, int lda, const float* B, int ldb, float* C, int ldc,
             const float* bias, const float* bias2, int flags,
             void* ws, size_t ws_bytes, int precision, void* stream);
/* rlt_gemm plus two fused side products of the backward pass:
 *   relu_mask (M x N, ldmask) : C = relu_mask > 0 ? C * mask_scale : 0 after the epilogue
 *                               (dH = (dY W2) * (H > 0) [/ (1-p) when the forward dropped H])
 *   drop_p, seed              : dropout on the output after bias/ReLU: keep(seed,row,col) ? C/(1-p) : 0
 *                               (the FFN hidden dropout of nn.TransformerEncoderLayer), 0 = off
 *   colsum_a  (M)             : = sum_k op(A)[m][k]; requires ta = 1.  With A = dY stored [T,N_out] this is
 *                               the bias gradient, produced by the dW = dY^T X product at no extra HBM pass. */
int rlt_gemm_ex(int ta, int tb, int M, int N, int K,
                const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                const float* bias, const float* bias2, int flags,
                const float* relu_mask, int ldmask, float mask_scale, float* colsum_a,
                float drop_p, uint32_t seed,
                void* ws, size_t ws_bytes, int precision, void* stream);

/* What the last rlt_gemm / rlt_gemm_ex / rlt_gemm_bits call of the CALLING THREAD decided (tests: tests/test_gemm_dispatch_gpu.py
 * asserts that a case reaches the kernel its id names).  Written on the host in the branch that launches; no device work, no
 * influence on the choice.  family RLT_GEMM_NONE: no product has been launched by this thread yet, or the last call returned
 * before its launch (argument / workspace error).
 *   fast       the branch-free loaders (gemm_kernel, gemm3_kernel; 1 for the families that have no other loader)
 *   persistent the workgroups walk the output tiles (gemm3b / gemm6c / gemm6e)
 *   ns, kchunk, slab_xcd   the final split-K plan: slabs, K per slab, slabs pinned to XCDs (1-D grid)
 *   epilogue, narrow       gemm6s only: its epilogue code (0 plain, 1 ReLU, 2 ReLU + bits out, 3 bits in), 128-column panels */
#define RLT_GEMM_NONE   0
#define RLT_GEMM_F32    1   /* gemm_kernel: exact fp32, 128 x 128 */
#define RLT_GEMM_3      2   /* gemm3_kernel: bf16x3, 128 x 128 */
#define RLT_GEMM_3B     3   /* gemm3b_kernel: bf16x3, 256 x 256 */
#define RLT_GEMM_6      4   /* gemm6_kernel: bf16x6, 256 x 128 */
#define RLT_GEMM_6B     5   /* gemm6b_kernel: bf16x6, 256 x 256, one K tile per slab */
#define RLT_GEMM_6C     6   /* gemm6c_kernel: bf16x6, 256 x 256, two wavefronts per SIMD */
#define RLT_GEMM_6E     7   /* gemm6e_kernel: bf16x6, 256 x 256, one wavefront per SIMD */
#define RLT_GEMM_6S     8   /* gemm6s_kernel: bf16x6, weights-stationary K = 256 / 128 */
typedef struct rlt_gemm_dispatch {
    int family, ta, tb, fast, persistent, ns, kchunk, slab_xcd, epilogue, narrow;
} rlt_gemm_dispatch;
int rlt_gemm_last_dispatch(rlt_gemm_dispatch* out);
/* What rlt_gemm / rlt_gemm_ex / rlt_gemm_bits decide for one call (csrc/gemm_plan.h: the decision is taken once per call, there;
 * tests: tests/test_gemm_plan.py, tests/test_gemm_dispatch_gpu.py).  Host only: no device work, no pointers - a call is described by
 * what the decision may depend on.  `out` is the record rlt_gemm_last_dispatch returns after the real call (family RLT_GEMM_NONE
 * where that call returns before its launch); the return value is the real call's before its launch: 0, RLT_E_WORKSPACE, or the
 * -1 of a mask output without RLT_GEMM_RELU on the weights-stationary kernel.  RLT_E_ARG: a null argument, M / N / K <= 0, a leading
 * dimension below its row, a column sum without ta, an unknown precision code.
 *   aligned16  bits RLT_GEMM_PTR_A .. _BITS_IN: the pointer is 16-byte aligned (read only for pointers that are present)
 *   present    bits RLT_GEMM_PTR_BIAS .. _COLSUM: the optional pointer is not NULL
 *   drop       drop_p > 0
 *   ws_null, ws_bytes     `ws` is NULL; the bytes the call is given */
#define RLT_GEMM_PTR_A         1
#define RLT_GEMM_PTR_B         2
#define RLT_GEMM_PTR_C         4
#define RLT_GEMM_PTR_BIAS      8
#define RLT_GEMM_PTR_BIAS2     16
#define RLT_GEMM_PTR_BITS_OUT  32
#define RLT_GEMM_PTR_BITS_IN   64
#define RLT_GEMM_PTR_RELU_MASK 128
#define RLT_GEMM_PTR_COLSUM    256
typedef struct rlt_gemm_call {
    int ta, tb, M, N, K, lda, ldb, ldc, flags;
    int aligned16, present, drop, ws_null;
    size_t ws_bytes;
} rlt_gemm_call;
int rlt_gemm_plan(const rlt_gemm_call* call, int precision, rlt_gemm_dispatch* out);

/* The FFN pair of rlt_gemm_ex epilogues with a 1-bit-per-element mask instead of the fp32 activation
 * (nn.TransformerEncoderLayer's linear1 -> ReLU -> dropout forward and the dH = (dY W2) * mask backward):
 *   relu_bits_out != NULL (flags must hold RLT_GEMM_RELU): C = dropout(relu(op(A) op(B) + bias)) with the keep mask of
 *     (drop_p, seed) as in rlt_gemm_ex (drop_p = 0: no dropout), and the mask bit of element (row, col) = (C > 0), i.e.
 *     the element passed the ReLU and was kept;
 *   mask_bits_in  != NULL: C = bit ? (op(A) op(B) + bias) * mask_scale : 0   (mask_scale = 1/(1-p); drop_p must be 0).
 * Mask layout (private to this pair of calls): packed along ROWS - bit (row & 31) of word [(row >> 5) * N + col];
 * rlt_gemm_bits_words(M, N) = ceil(M/32) * N words.  Exactly one of the two pointers; N % 32 == 0; no split-K, no
 * workspace.  The backward product then reads M*N/8 bytes of mask instead of 4*M*N (10 GB at 1,228,800 x 2048). */
size_t rlt_gemm_bits_words(int M, int N);
int rlt_gemm_bits(int ta, int tb, int M, int N, int K,
                  const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                  const float* bias, int flags, float drop_p, uint32_t seed,
                  uint32_t* relu_bits_out, const uint32_t* mask_bits_in, float mask_scale,
                  int precision, void* stream);
/* out[N] (+)= sum over the T rows of X[T,N] (ldx) - bias gradients.  ws: rlt_colsum_workspace bytes. */
size_t rlt_colsum_workspace(int T, int N);
int rlt_colsum(const float* X, int ldx, int T, int N, float* out, int accumulate,
               void* ws, size_t ws_bytes, void* stream);
/* out[g][n] (+)= sum_{r<R} X[(g*R + r)*ldx + n] for g < G: per-position sums (Choopy dPE) */
int rlt_segment_colsum(const float* X, int ldx, int G, int R, int N, float* out, int ldo,
                       int accumulate, void* stream);

/* Narrow weight gradient of an input projection: dW[M][I] = A^T X and db[M] = column sums of A, for 1 <= I <= 3
 * (the LSTM layer-0 input weights, input_size = 3, models/AttnCut.py:8; replaces the N = 3 case of the dW GEMM and
 * its bias-gradient side sum with ONE streaming pass over A for both directions).  A (T, lda >= M, M % 4 == 0),
 * X (T, ldx >= I); db may be NULL. */
size_t rlt_narrow_dw_workspace(int T, int M);
int rlt_narrow_dw(const float* A, int lda, const float* X, int ldx, int I, int T, int M,
                  float* dW, float* db, void* ws, size_t ws_bytes, void* stream);
/* y = max(x,0) backward etc. are fused in the kernels; dX *= (Y > 0) in place (FFN backward) */
int rlt_relu_bwd(float* dX, const float* Y, size_t n, void* stream);
/* x[i] *= *scale (device scalar) */
int rlt_scale(float* x, const float* scale, size_t n, void* stream);

/* ------------------------------------------------------------------ residual + LayerNorm (M3)
 * y = LayerNorm(x + r) * gamma + beta, eps inside the sqrt, biased variance
 * (nn.TransformerEncoderLayer post-norm, models/AttnCut.py:9).  stats: (T,2) mean, rstd.
 * bwd: dz (T,E) = gradient w.r.t. (x + r) (identical for x and r); dgamma/dbeta (E) (+)=.
 * E multiple of 64, E <= 1024.
 * Dropout (train mode, dropout1/dropout2 of the encoder layer): y = LN(x + drop(r)) with
 * drop(r) = keep(seed,t,c) ? r/(1-p) : 0; bwd then also writes dr = dz * keep/(1-p) (dr may be NULL
 * when drop_p == 0: the gradient of r is dz itself).
 */
int rlt_add_layernorm_fwd(const float* x, const float* r, const float* gamma, const float* beta,
                          int T, int E, float eps, float drop_p, uint32_t seed,
                          float* y, float* stats, void* stream);
size_t rlt_add_layernorm_bwd_workspace(int T, int E);
int rlt_add_layernorm_bwd(const float* x, const float* r, const float* gamma, const float* stats,
                          const float* dy, int T, int E, float drop_p, uint32_t seed,
                          float* dz, float* dr, float* dgamma, float* dbeta,
                          int accumulate, void* ws, size_t ws_bytes, void* stream);
/* the dropout keep-mask of the kernels above as data (tests): out[r][c] = keep(seed,r,c) ? 1/(1-p) : 0 */
int rlt_dropout_mask(uint32_t seed, size_t rows, int cols, float p, float* out, void* stream);

/* ------------------------------------------------------------------ list-axis attention (M3)
 * Multi-head self-attention where, at every position s and head h, the B lists of the
 * mini-batch attend to each other (F.multi_head_attention_forward on a (L=B, N=S, E) input,
 * models/AttnCut.py:9,18).  Flash-style: the B x B score matrix is never
 * materialised.
 *   qkv: (S*B, 3E) position-major, columns [q | k | v], head h = columns h*HD..h*HD+HD of each.
 *   out: (S*B, E) concatenated heads (input of out_proj).  lse: (S,H,B) log-sum-exp of the
 *   scaled scores (saved for backward).  scale = 1/sqrt(HD).
 *   drop_p, seed: dropout on the attention probabilities (train mode, the `dropout` of
 *   nn.MultiheadAttention); the mask is a pure function of (seed, s, h, query, key), recomputed in backward.
 * bwd: dqkv (S*B,3E) from dout; ws: rlt_list_attention_bwd_workspace bytes.
 * HD in {16, 32, 64}; E = H*HD.
 */
/* In the split-bf16 mode the forward first writes Q (pre-scaled), K and V as pre-split bf16 hi/lo tile
 * records (64-row tiles in the kernels' LDS layout) into `images` (rlt_list_attention_fwd_workspace bytes; 0 in
 * fp32 mode, then `images` may be NULL); the caller keeps `images` for the backward pass.  The records are written
 * for the dropout rate of THIS call (without dropout the head-dim-64 backward kernels read the transposed operands
 * straight from the row images and the transposed images of Q and K are not written): the backward entry points must
 * be given the same drop_p and seed as the forward call whose `images` they use. */
/* BF16X6, 512 lists and more in whole tiles (head dim 64, with or without dropout: csrc/attention6h.hip; head dim 16 without dropout:
 * csrc/attention6n.hip):
 * the pipelined forward kernels stage pre-split K / V tile images that the call itself writes into `images` (+ a flag word per
 * workgroup for its fix-up launch); the backward pass does not read them - rlt_list_attention_images_retained() tells whether the
 * caller has to keep `images` for the backward (1) or may treat it as scratch of the forward call (0).  `drop_p` of the workspace
 * query = the drop_p of the forward call (at head dim 16 a train-mode call has no pipelined form and needs no such buffer). */
size_t rlt_list_attention_fwd_workspace(int S, int B, int H, int HD, float drop_p, int precision);
int rlt_list_attention_images_retained(int S, int B, int H, int HD, int precision);
int rlt_list_attention_fwd(const float* qkv, int S, int B, int H, int HD, float drop_p, uint32_t seed,
                           float* out, float* lse, void* images, size_t images_bytes, int precision, void* stream);
/* backward: ws = [delta (S,H,B) | tile records], rlt_list_attention_bwd_workspace bytes.
 *   _bwd_prepare: delta = rowsum(dout*out) and (split-bf16 mode) the dO records;
 *   _bwd_dkv:     dK, dV columns of dqkv;   _bwd_dq: dQ columns of dqkv;
 *   _bwd:         the three in sequence.  `images` = the forward's buffer (NULL => exact-fp32 kernels).
 * BF16X6 at head dim 16 with 512 lists and more (Choopy / MtChoopy at scale; csrc/attention6n.hip): the backward kernels stage
 * pre-split 128-row tile images of Q, K, V, dO and the rows' seeds (-lse, -delta) from ws - _bwd_prepare writes the dO images and
 * the seeds, _bwd_dkv the Q images, _bwd_dq the K and V images, each before its kernel (so the three entry points stay callable
 * on their own; ws is scratch of ONE backward pass: the parts of a pass run on one stream, in any order after _bwd_prepare). */
/* `drop_p` of the workspace query and of _bwd_prepare = the drop_p of the forward call (train-mode kernels stage their tiles
 * themselves: ws is delta only).  The parts check ws_bytes against the same rule in their OWN precision scope and ws for 16-byte
 * alignment: RLT_E_WORKSPACE / RLT_E_ALIGN instead of a device write beyond a buffer sized under another mode. */
size_t rlt_list_attention_bwd_workspace(int S, int B, int H, int HD, float drop_p, int precision);
int rlt_list_attention_bwd(const float* qkv, const float* out, const float* dout, const float* lse,
                           int S, int B, int H, int HD, float drop_p, uint32_t seed, const void* images, float* dqkv,
                           void* ws, size_t ws_bytes, int precision, void* stream);
int rlt_list_attention_bwd_prepare(const float* out, const float* dout, const float* lse, int S, int B, int H, int HD, float drop_p,
                                   const void* images, void* ws, size_t ws_bytes, int precision, void* stream);
int rlt_list_attention_bwd_dkv(const float* qkv, const float* dout, const float* lse, const void* images, void* ws, size_t ws_bytes,
                               int S, int B, int H, int HD, float drop_p, uint32_t seed, float* dqkv, int precision, void* stream);
int rlt_list_attention_bwd_dq(const float* qkv, const float* dout, const float* lse, const void* images, void* ws, size_t ws_bytes,
                              int S, int B, int H, int HD, float drop_p, uint32_t seed, float* dqkv, int precision, void* stream);
/* What the entry points above decide for one call (csrc/attention_plan.h: the decision is taken once per call, there; tests:
 * tests/test_attention_plan.py, tests/test_attention_dispatch_gpu.py; every eval-mode kernel at its tile edges with lse, delta, the
 * fix-up flag words and the order of the backward parts: tests/test_attention_edges_gpu.py; the train-mode kernels:
 * tests/test_dropout_gpu.py).  Host only: no device work, no influence on the choice.
 * have_images: the call is given a usable `images` buffer (non-NULL; for the pipelined forwards also 16-byte aligned and
 * images_bytes long).  Errors: RLT_E_ARG (out NULL, non-positive S / B / H, drop_p outside [0, 1), precision), RLT_E_SHAPE (HD).
 *   fwd, dkv, dq     the kernel of rlt_list_attention_fwd / _bwd_dkv / _bwd_dq, an RLT_ATTN_* code
 *   fwd_fixup        the kernel of the forward's second launch over the workgroups the pipelined forward flagged, or RLT_ATTN_NONE
 *   *_prepare        what the entry point writes before its kernel, a mask of RLT_ATTN_PREP_*: the forward into `images` (the
 *                    blocks in the order of the set bits: Q | K | V, or K | V), _bwd_prepare / _bwd_dkv / _bwd_dq into ws
 *   images_kind, images_bytes, images_retained   the forward's `images` (= rlt_list_attention_fwd_workspace and
 *                    _images_retained); flags_offset / flags_bytes: the flag words of the fix-up launch at its end
 *   ws_kind, delta_bytes, ws_extra_bytes, ws_bytes   the backward workspace: delta, then ws_extra_bytes of ws_kind
 *                    (ws_bytes = the sum = rlt_list_attention_bwd_workspace)
 *   ws_prepare_bytes, ws_part_bytes   what _bwd_prepare and _bwd_dkv / _bwd_dq require of ws_bytes in THIS call (with
 *                    have_images = 0 they do not use - and _bwd_prepare does not ask for - tile records behind delta) */
#define RLT_ATTN_NONE           0
#define RLT_ATTN_F32            1   /* attn_*_kernel: exact fp32, 32x32x2 MFMA (dK+dV: two workgroups per CU) */
#define RLT_ATTN_F32_SB         2   /* ... forward / dQ at head dim 64: single-buffered, three workgroups per CU */
#define RLT_ATTN_F32_OCC1       3   /* ... dK+dV in the 512-register form (head dim 128; RLT_DKV_OCC=1) */
#define RLT_ATTN_F32_HD16       4   /* attn16_*_kernel: exact fp32 at head dim 16, 16x16x4 MFMA */
#define RLT_ATTN_X3             5   /* attn3_*_kernel: bf16x3 from tile records */
#define RLT_ATTN_X6             6   /* attn6_{fwd,bwd_dkv,bwd_dq}_kernel: bf16x6, two wavefronts per SIMD */
#define RLT_ATTN_X6_IMG         7   /* ... staging pre-split tile images (RLT_ATTN6_IMG=1) */
#define RLT_ATTN_X6_PP          8   /* attn6_fwd_pp_kernel: head dim 64 ping-pong forward */
#define RLT_ATTN_X6_PP_IMG      9   /* ... staging pre-split tile images */
#define RLT_ATTN_X6_DKV1        10  /* attn6_bwd_dkv1_kernel: head dim 64 dK+dV, one wavefront per SIMD */
#define RLT_ATTN_X6_DQ1         11  /* attn6_bwd_dq1_kernel: head dim 64 dQ, one wavefront per SIMD */
#define RLT_ATTN_X6N_2W         12  /* attn6n_*_kernel<.., false>: head dim 16, two wavefronts per SIMD, fewer than 512 lists */
#define RLT_ATTN_X6N_2W_SEEDED  13  /* attn6n_*_kernel<.., true>: ... 512 lists and more (score accumulators seeded with -lse, -delta) */
#define RLT_ATTN_X6N_PIPE       14  /* attn6n_fwd1_kernel / attn6n_bwd1_kernel: head dim 16 pipelined, from tile images */
#define RLT_ATTN_X6H_PIPE       15  /* attn6h_fwd1_kernel: head dim 64 pipelined forward, from tile images */
#define RLT_ATTN_PREP_Q      1
#define RLT_ATTN_PREP_K      2
#define RLT_ATTN_PREP_V      4
#define RLT_ATTN_PREP_DO     8
#define RLT_ATTN_PREP_SEEDS  16     /* the rows' -lse, -delta (head dim 16 pipelined backward) */
#define RLT_ATTN_PREP_DELTA  32     /* delta = rowsum(dout * out) */
#define RLT_ATTN_IMAGES_NONE    0
#define RLT_ATTN_IMAGES_X3_QKV  1   /* bf16x3 tile records of Q, K, V (retained) */
#define RLT_ATTN_IMAGES_X6_QKV  2   /* bf16x6 tile images of Q, K, V (RLT_ATTN6_IMG=1, retained) */
#define RLT_ATTN_IMAGES_X6N_KV  3   /* head dim 16 pipelined forward: K images | V images | flag words (scratch) */
#define RLT_ATTN_IMAGES_X6H_KV  4   /* head dim 64 pipelined forward: the same */
#define RLT_ATTN_WS_DELTA       0   /* nothing behind delta */
#define RLT_ATTN_WS_X3_DO       1   /* bf16x3 dO tile records */
#define RLT_ATTN_WS_X6_DO       2   /* bf16x6 dO tile images (RLT_ATTN6_IMG=1) */
#define RLT_ATTN_WS_X6N_BLOCKS  3   /* head dim 16 pipelined backward: image blocks Q | K | V | dO, then the seeds */
typedef struct rlt_attention_plan {
    int fwd, fwd_fixup, dkv, dq;
    int fwd_prepare, bwd_prepare, dkv_prepare, dq_prepare;
    int images_kind, images_retained, ws_kind;
    size_t images_bytes, flags_offset, flags_bytes;
    size_t delta_bytes, ws_extra_bytes, ws_bytes, ws_prepare_bytes, ws_part_bytes;
} rlt_attention_plan;
int rlt_list_attention_plan(int S, int B, int H, int HD, float drop_p, int have_images, int precision, rlt_attention_plan* out);
/* keep-mask of the attention-probability dropout as data (tests, small B): out (S,H,B,B) =
 * keep ? 1/(1-p) : 0 for (position, head, query, key) */
int rlt_attention_dropout_mask(uint32_t seed, int S, int B, int H, float p, float* out, void* stream);
/* the same for the (position, head) pairs pair0 .. pair0 + npair - 1 only, pair = position * H + head: out (npair,B,B)
 * (tests at benchmark sizes, where the whole (S,H,B,B) mask would not fit) */
int rlt_attention_dropout_mask_range(uint32_t seed, int pair0, int npair, int B, float p, float* out, void* stream);

/* ------------------------------------------------------------------ within-list ("position-axis") attention
 * Multi-head self-attention where every list of the mini-batch attends over its OWN S positions (nn.MultiheadAttention with
 * batch_first=True on a (B, S, E) input: the model of the AttnCut / Choopy papers; a list's output does not depend on the
 * other lists of the batch).  csrc/attention_seq.hip; tests: tests/test_seq_attention_abi.py, tests/test_seq_attention_gpu.py
 * against the float64 restatement tests/seq_attention_restate.py.
 *   qkv: (S*B, 3E) position-major as above (row s*B + b, columns [q | k | v], head h = columns h*HD..h*HD+HD of each): the
 *   problem of (list b, head h) is rows b, b+B, .., b+(S-1)B.  scores q k^T / sqrt(HD), softmax over the keys with the row
 *   maximum subtracted, optional dropout on the normalised probabilities, P V.
 *   out: (S*B, E) in the same row order.  lse: (B,H,S), log of the normaliser + the row maximum, of the UNdropped scores.
 *   drop_p, seed: the keep stream of csrc/common.h - the stream of pair b*H + h is pair_seed of (seed, b*H + h), an element is
 *   kept iff rlt_keep of (stream, query position, key position, the rlt_drop_threshold of drop_p), kept weights are scaled by
 *   1.f / (1.f - drop_p); the backward recomputes the same mask from (drop_p, seed).
 *   bwd: ONE launch writes the dQ, dK and dV columns of dqkv (S*B, 3E) and nothing else: a whole S x S problem lives in one
 *   workgroup, so no sum crosses workgroups - delta = rowsum(dout * out) is formed in the kernel, no atomics, no allocation,
 *   no host synchronisation, two calls give the same bits.  rlt_seq_attention_bwd_workspace is 0 today (ws may be NULL).
 * HD in {16, 64}; 1 <= S <= 1024; any B, H >= 1 with S*B*3E < 2^40 elements (the kernels index in 64 bits) and
 * B * ceil(H * HD / 64) < 2^24 workgroups.  The three precision codes run the SAME exact-fp32 kernels (32x32x2 f32 MFMA, fp32
 * accumulation, fp32 exp): at 4*B*H*S*S*HD flops per product pass that is at least what BF16X6 and BF16X3 promise; `precision`
 * is validated like everywhere else.
 * Errors before any launch, in this order: RLT_E_ARG (a precision code outside the three + DEFAULT - workspace query: 0 bytes;
 * a NULL qkv / out / dout / lse / dqkv; non-positive S / B / H; drop_p outside [0, 1)), RLT_E_SHAPE (HD not 16 or 64, S > 1024,
 * the index limits above), RLT_E_ALIGN (a pointer off 16 bytes), RLT_E_WORKSPACE (ws_bytes below the query's answer).
 * Algorithmic bytes: fwd reads 12*S*B*E (qkv) and writes 4*S*B*E + 4*B*H*S; bwd reads 12*S*B*E + 8*S*B*E + 4*B*H*S and writes
 * 12*S*B*E (K / V - in the backward also Q / dO - tiles are re-read once per 128 owned rows at head dim 64, per 32 at head
 * dim 16, from L2).
 * The mask (rlt_seq_attention_fwd_ex / _bwd_ex; the calls without _ex are the _ex calls with RLT_SEQ_MASK_NONE, same launches,
 * same bits): RLT_SEQ_MASK_NONE admits every key of the list for every query; RLT_SEQ_MASK_CAUSAL admits key j for query i
 * iff j <= i, so out, lse and - for a dout that is zero from position i on - dqkv of the positions < i do not depend on
 * the rows of positions >= i: bit for bit for finite inputs (tests/test_seq_causal_gpu.py against tests/seq_causal_restate.py).
 *   lse is the log-normaliser over the ADMITTED keys; delta = rowsum(dout * out) as before.  Row 0 admits key 0 alone: its
 *   weight is exactly 1, and without dropout out at position 0 IS V at position 0, bit for bit.
 *   dropout: the keep stream stays keyed by (pair, query, key) - a masked element's draw is simply never used, and the kept
 *   elements of a causal call are those of the unmasked call at the same (drop_p, seed).
 *   NOT isolated: non-finite values below a row.  A masked weight is an exact 0 multiplied into the K, V, Q or dO row of the
 *   same 32-row sub-tile, and 0 * NaN = 0 * inf = NaN: a NaN or inf planted BELOW position i can reach row i when both lie
 *   in one 32-position block (or, in the backward, one 32-query block that a key's wavefront visits).  Finite values never do.
 *   the kernels skip the 32 x 32 tiles above the diagonal (forward and both backward phases: t + 1 of the products of
 *   32-row block t) and do not stage the 64-row tiles no wavefront of the pass needs.  The algorithmic bytes are those above,
 *   unchanged: every row is still read and written once; only the L2 tile re-reads fall.
 *   a mask code outside {0, 1} is RLT_E_ARG, with the other argument errors and ahead of RLT_E_SHAPE / _ALIGN / _WORKSPACE. */
#define RLT_SEQ_MASK_NONE   0
#define RLT_SEQ_MASK_CAUSAL 1
size_t rlt_seq_attention_bwd_workspace(int S, int B, int H, int HD, float drop_p, int precision);   /* may be 0 */
int rlt_seq_attention_fwd(const float* qkv, int S, int B, int H, int HD, float drop_p, uint32_t seed,
                          float* out, float* lse, int precision, void* stream);
int rlt_seq_attention_bwd(const float* qkv, const float* out, const float* dout, const float* lse,
                          int S, int B, int H, int HD, float drop_p, uint32_t seed, float* dqkv,
                          void* ws, size_t ws_bytes, int precision, void* stream);
int rlt_seq_attention_fwd_ex(const float* qkv, int S, int B, int H, int HD, float drop_p, uint32_t seed, int mask,
                             float* out, float* lse, int precision, void* stream);
int rlt_seq_attention_bwd_ex(const float* qkv, const float* out, const float* dout, const float* lse,
                             int S, int B, int H, int HD, float drop_p, uint32_t seed, int mask, float* dqkv,
                             void* ws, size_t ws_bytes, int precision, void* stream);

/* ------------------------------------------------------------------ streaming: K/V-cached append attention
 * The causal within-list forward, one CHUNK of ranks at a time (csrc/attention_seq_append.hip; inference only: no dropout, no
 * backward).  tests: tests/test_stream_abi.py, tests/test_seq_append_gpu.py.
 *   qkv_chunk: (C*B, 3E) position-major, row i*B + b = [q | k | v] of rank t0 + i of list b - the in_proj of the chunk's rows.
 *   kv_cache:  (Smax*B, 2E) position-major, row s*B + b = [K | V] of rank s of list b.  The CALLER owns it: 8*Smax*B*E bytes,
 *              one per encoder layer, alive from the list's first chunk to its last.  It need not be initialised: the call reads
 *              rows < t0 only (what earlier calls appended) and writes rows t0 .. t0+C-1; rows >= t0+C are neither read nor
 *              written.
 *   active:    (B) int32 or NULL; active[b] == 0 retires list b: its workgroups leave at once, and its rows of out, of lse and of
 *              the cache are UNTOUCHED (not zeroed).  NULL: every list is active.
 *   out: (C*B, E), row i*B + b.  lse: (B,H,C) or NULL.
 * For an active list the call appends the chunk's K | V columns to cache rows t0 .. t0+C-1 and writes the attention of the C new
 * queries over ranks 0 .. t0+i.  PREFIX STATEMENT: out and lse of rank t0+i are, as fp32 values, those that
 * rlt_seq_attention_fwd_ex with RLT_SEQ_MASK_CAUSAL and drop_p = 0 gives for that rank on the whole list - whatever the chunking,
 * zero tolerance.  The kernel has the one-shot kernel's geometry and device functions (csrc/attention_seq_tile.h): passes aligned to
 * absolute multiples of 32 ranks, row q over the 32-key sub-tiles 0 .. floor(q/32) in order, keys > q at weight 0.  The tile
 * rows >= t0+C are staged as zeros where the one-shot call stages ranks behind the query (weight 0 either way): the sign of an
 * exactly-zero sum is the one thing that may differ (+0 against -0).  After the last chunk the cache holds the K | V columns of
 * the list's qkv bit for bit.  A tile is staged from the cache (ranks < t0) and from the chunk itself (ranks >= t0): the kernel
 * never reads a cache row it writes in the same launch.
 * Limits and errors are those of rlt_seq_attention_fwd_ex with Smax for S, before any launch and in this order: RLT_E_ARG (a bad
 * precision code; qkv_chunk, kv_cache or out NULL; C, Smax, B or H not positive; t0 < 0; t0 + C > Smax), RLT_E_SHAPE (HD not 16
 * or 64, Smax > 1024, the index limits), RLT_E_ALIGN (qkv_chunk, kv_cache, out or lse off 16 bytes).  The three precision codes
 * run the same exact-fp32 kernel.  No allocation, no host synchronisation, no atomics; two calls give the same bits.  Calls on one
 * cache must be ordered (one stream, or events): chunk t0 reads what the chunks before it wrote.
 * Algorithmic bytes per active list: reads 12*C*E (the chunk) + 8*t0*E (the cache), writes 8*C*E (cache) + 4*C*E + 4*H*C.  At
 * C = 1 one of a wavefront's 32 query lanes works and the call is bound by the 8*t0*B*E cache read; the key range is NOT split
 * across wavefronts, which would change the order of the sums and give up the prefix statement. */
int rlt_seq_attention_append(const float* qkv_chunk, float* kv_cache, int t0, int C, int Smax, int B, int H, int HD,
                             const int32_t* active, float* out, float* lse, int precision, void* stream);

/* ------------------------------------------------------------------ BiLSTM recurrence (M2)
 * One bidirectional LSTM layer with hidden size 128 (nn.LSTM(..., hidden_size=128,
 * bidirectional=True, batch_first=True), models/AttnCut.py:8): gate order i,f,g,o, h0=c0=0.
 * The input projections x_t W_ih^T + b_ih + b_hh of both directions are computed beforehand by
 * rlt_gemm into `gates` (S*B, 2, 512) position-major (dir 0 = forward in s, dir 1 = reverse).
 * fwd: adds h_{t-1} W_hh^T, applies the nonlinearities, overwrites `gates` in place with the
 *      ACTIVATED gates (i,f,g,o), writes the cell states c (S*B,2,128) and h_out (S*B,256) =
 *      [forward | reverse] hidden states.
 * bwd: from d_hout (S*B,256) and the stashes, writes d(pre-activation gates) in place over
 *      `gates` (then dW_ih, dW_hh, db, dx are plain rlt_gemm / rlt_colsum calls on it).
 * w_hh_fwd, w_hh_rev: (512,128) each = weight_hh_l{k}, weight_hh_l{k}_reverse.
 */
int rlt_bilstm_rec_fwd(float* gates, const float* w_hh_fwd, const float* w_hh_rev, int S, int B,
                       float* h_out, float* c_out, int precision, void* stream);

/* The same recurrence with the input projection fused in, for narrow inputs (1 <= I <= 3: layer 0 of the
 * reference's encoders, input_size = 3, models/AttnCut.py:6,8): pre-activations x W_ih^T + b_ih + b_hh are formed
 * inside the kernel from x (S*B, I) and never touch HBM; `gates` (S*B, 1024) is output only (activated gates for
 * rlt_bilstm_rec_bwd).  RLT_E_SHAPE for I > 3: use rlt_gemm + rlt_bilstm_rec_fwd. */
int rlt_bilstm_rec_fwd_x(const float* x, int I, const float* w_ih_fwd, const float* b_ih_fwd, const float* b_hh_fwd,
                         const float* w_ih_rev, const float* b_ih_rev, const float* b_hh_rev,
                         const float* w_hh_fwd, const float* w_hh_rev, int S, int B,
                         float* gates, float* h_out, float* c_out, int precision, void* stream);
int rlt_bilstm_rec_bwd(float* gates, const float* c, const float* w_hh_fwd, const float* w_hh_rev,
                       const float* d_hout, int S, int B, int precision, void* stream);
/* What the three entry points above decide for one call (csrc/lstm_common.h: the decision is taken once per call, there; tests:
 * tests/test_lstm_plan.py, tests/test_lstm_dispatch_gpu.py).  Host only: no device work, no influence on the choice.
 * xin: 1 for rlt_bilstm_rec_fwd_x (the forward kernel's instantiation with the fused input projection), 0 for
 * rlt_bilstm_rec_fwd; the codes do not depend on it.  Errors: RLT_E_ARG (out NULL, B <= 0, xin not 0 / 1, precision).
 *   fwd, bwd               the kernel of the forward / of rlt_bilstm_rec_bwd, an RLT_LSTM_* code
 *   fwd_lists, bwd_lists   lists per workgroup of that kernel (the grid is ceil(B / lists) x 2 directions)
 * The struct is named by its tag (C and C++ both allow a function of the same name next to a struct tag, not next to a typedef). */
#define RLT_LSTM_F32          1   /* bilstm_fwd_kernel / bilstm_bwd_kernel: exact fp32 on the f32 MFMA */
#define RLT_LSTM_X3           2   /* bilstm3_fwd_kernel / bilstm3_bwd8_kernel: bf16x3 */
#define RLT_LSTM_X6           3   /* bilstm6_fwd_kernel: bf16x6 in two phases per step (forward only: its backward is RLT_LSTM_F32) */
#define RLT_LSTM_X6W_SINGLE   4   /* bilstm6w_*_kernel<.., SINGLE>: bf16x6, one wavefront per SIMD, one 16-list half per workgroup */
#define RLT_LSTM_X6W_HALVES   5   /* bilstm6w_*_kernel: ... two independent 16-list halves per workgroup */
struct rlt_bilstm_rec_plan { int fwd, bwd, fwd_lists, bwd_lists; };
int rlt_bilstm_rec_plan(int B, int xin, int precision, struct rlt_bilstm_rec_plan* out);

/* ------------------------------------------------------------------ PATH-LEVEL ENTRY POINTS
 * One call = the forward or the backward of one module of the reference's models, composed inside the library from
 * the kernel-level entry points of this header (same launches, same order, same in-place accumulation): a host in any
 * language drives the hot path with these, the kernel-level entry points stay for tests and for hosts that fuse
 * differently.  Activations are position-major (S*B, E).  The caller owns two buffers per module:
 *   stash  written by the forward, read (the BiLSTM's: also overwritten) by the backward; layout documented at
 *          enc_stash() / lstm_stash() in csrc/path.hip;
 *   ws     scratch, dead after the call.
 * rlt_workspace_bytes(op, S, B, E, H, FF, train_dropout) reports their sizes; all regions are 256-byte aligned, pass
 * 256-byte aligned buffers.  For the RLT_OP_BILSTM_* queries E = the input feature count of layer 0, H and FF unused.
 */
#define RLT_OP_ENCODER_STASH   1   /* stash of rlt_encoder_layer_fwd/bwd (attention tile records only where the backward reads
                                    * them: rlt_list_attention_images_retained; independent of train_dropout)  */
#define RLT_OP_ENCODER_FWD_WS  2   /* ws of rlt_encoder_layer_fwd: split-K scratch + the attention images that are scratch of the
                                    * forward call (the pipelined bf16x6 forward kernels; train_dropout = the call's drop_p > 0) */
#define RLT_OP_ENCODER_BWD_WS  3   /* ws of rlt_encoder_layer_bwd (train_dropout != 0: + two (T,E) dropout grads) */
#define RLT_OP_BILSTM_STASH    4   /* stash of rlt_bilstm_fwd/bwd                                               */
#define RLT_OP_BILSTM_WS       5   /* ws of rlt_bilstm_fwd and rlt_bilstm_bwd                                   */
size_t rlt_workspace_bytes(int op, int S, int B, int E, int H, int FF, int train_dropout, int precision);

/* nn.TransformerEncoderLayer(d_model=E, nhead=H, dim_feedforward=FF, dropout) parameters, by state_dict name
 * (models/AttnCut.py:9: `attention_layer.layers.<i>.` + self_attn.in_proj_weight (3E,E), self_attn.in_proj_bias (3E),
 * self_attn.out_proj.weight (E,E), .bias (E), norm1.weight/.bias (E), linear1.weight (FF,E), .bias (FF),
 * linear2.weight (E,FF), .bias (E), norm2.weight/.bias (E)) */
typedef struct rlt_encoder_weights {
    const float *in_proj_weight, *in_proj_bias, *out_proj_weight, *out_proj_bias, *norm1_weight, *norm1_bias,
                *linear1_weight, *linear1_bias, *linear2_weight, *linear2_bias, *norm2_weight, *norm2_bias;
} rlt_encoder_weights;
typedef struct rlt_encoder_grads {     /* same shapes; every member is WRITTEN (=), not accumulated */
    float *in_proj_weight, *in_proj_bias, *out_proj_weight, *out_proj_bias, *norm1_weight, *norm1_bias,
          *linear1_weight, *linear1_bias, *linear2_weight, *linear2_bias, *norm2_weight, *norm2_bias;
} rlt_encoder_grads;
/* y = norm2(h1 + drop2(linear2(drop(relu(linear1(h1)))))),  h1 = norm1(x + drop1(out_proj(list_attention(in_proj(x)))))
 * (post-norm, ReLU, attention over the B lists at each of the S positions: F.multi_head_attention_forward on a
 * (L=B, N=S, E) input - models/AttnCut.py:9-10,18).  x, y: (S*B, E).  drop_p = 0 in eval();
 * seeds[4] = {attention probabilities, dropout1, FFN hidden, dropout2} (may be NULL when drop_p == 0).
 * bwd: dx (S*B, E) = d/dx, every member of g written; needs the same x, w, seeds and the forward's stash. */
int rlt_encoder_layer_fwd(const float* x, const rlt_encoder_weights* w, int S, int B, int E, int H, int FF, float eps,
                          float drop_p, const uint32_t* seeds, float* y, void* stash, size_t stash_bytes,
                          void* ws, size_t ws_bytes, int precision, void* stream);
int rlt_encoder_layer_bwd(const float* x, const rlt_encoder_weights* w, int S, int B, int E, int H, int FF, float eps,
                          float drop_p, const uint32_t* seeds, const float* dy, const void* stash, size_t stash_bytes,
                          float* dx, const rlt_encoder_grads* g, void* ws, size_t ws_bytes, int precision, void* stream);

/* One bidirectional layer of nn.LSTM(input, 128, num_layers=2, batch_first=True, bidirectional=True)
 * (models/AttnCut.py:8), index 0 = forward direction, 1 = reverse: weight_ih_l{k}[_reverse] (512, in),
 * weight_hh_l{k}[_reverse] (512,128), bias_ih_l{k}[_reverse] (512), bias_hh_l{k}[_reverse] (512). */
typedef struct rlt_lstm_layer_weights { const float *w_ih[2], *w_hh[2], *b_ih[2], *b_hh[2]; } rlt_lstm_layer_weights;
typedef struct rlt_lstm_layer_grads { float *w_ih[2], *w_hh[2], *b_ih[2], *b_hh[2]; } rlt_lstm_layer_grads;   /* written (=) */
/* The whole 2-layer stack: x (S*B, I) -> h_out (S*B, 256) = [forward | reverse] hidden states of layer 1; w[2], g[2] =
 * layers 0 and 1 (layer 1 has 256 inputs).  bwd: dh_out (S*B,256) -> g and, when dx != NULL, dx (S*B, I); it needs the
 * forward's h_out and stash, and overwrites the gate stashes (call it once per forward). */
int rlt_bilstm_fwd(const float* x, int I, const rlt_lstm_layer_weights* w, int S, int B, float* h_out,
                   void* stash, size_t stash_bytes, void* ws, size_t ws_bytes, int precision, void* stream);
int rlt_bilstm_bwd(const float* x, int I, const rlt_lstm_layer_weights* w, const float* h_out, const float* dh_out, int S, int B,
                   void* stash, size_t stash_bytes, float* dx, const rlt_lstm_layer_grads* g,
                   void* ws, size_t ws_bytes, int precision, void* stream);

/* The same 2-layer stack for ANY hidden size (`encoding_size` of models/MMOECut.py:57,63; every other model and every
 * BASELINE config uses 128, which runs on the persistent kernels above).  General form, built for coverage: one GEMM
 * per layer for the input projection, one small GEMM per direction and one cell kernel per time step, the backward
 * the same in reverse.  w[l].w_ih (4*hidden, in), w[l].w_hh (4*hidden, hidden), biases (4*hidden); layer 1 has
 * 2*hidden inputs; h_out (S*B, 2*hidden).  rlt_bilstm_generic_bytes(stash != 0, ...) / (0, ...) size the two buffers. */
size_t rlt_bilstm_generic_bytes(int stash, int S, int B, int I, int hidden);
int rlt_bilstm_generic_fwd(const float* x, int I, int hidden, const rlt_lstm_layer_weights* w, int S, int B, float* h_out,
                           void* stash, size_t stash_bytes, void* ws, size_t ws_bytes, int precision, void* stream);
int rlt_bilstm_generic_bwd(const float* x, int I, int hidden, const rlt_lstm_layer_weights* w, const float* h_out,
                           const float* dh_out, int S, int B, void* stash, size_t stash_bytes, float* dx,
                           const rlt_lstm_layer_grads* g, void* ws, size_t ws_bytes, int precision, void* stream);

/* ------------------------------------------------------------------ sparse layer-0 input (BiCut on its bag-of-words input)
 * models/Bicut.py:6,10 (BiCut(input_size=231449): nn.LSTM over the document vectors), data_prep/document_statics.ipynb
 * sections "bicut统计数据获取" / "Bicut输入数据" (per ranked document [token count, distinct-token count, bag-of-words vector]),
 * dataloader/split_bicut_data.py:21-24 (the retrieval score put in front) and dataloader/bicut_dataloader.py:15-40 (one
 * densified 300 x 231,451 pickle per query, `.float()`): the input projection x W_ih^T + b_ih + b_hh of BiLSTM layer 0 and
 * its weight gradient, with x never densified.  A token row t = s*B + b is `Dn` leading dense columns plus ONE row of a
 * device-resident CSR table; the layer-0 input width is I = Dn + V.
 *   dense (B,S,Dn) float32 and ids (B,S) int32 (row of each ranked document in the table) in the reference's (B,S) layout;
 *   table: indptr (n_docs+1) int64, indices int32 (term ids in [0,V), strictly ascending within a row), values float32; a row
 *   may be empty; total nonzeros are bounded by int64 only.  1 <= Dn <= 16, B*S < 2^31, Dn + V < 2^31.
 * The two layer-0 input weights are COLUMN-MAJOR: wt (I, 512) per direction, wt[c*512 + g] = weight_ih_l0[g, c] - the memory
 * of a (512, I) tensor with strides (1, 512) - so that one nonzero reads and one gradient column writes 2 KB contiguous per
 * direction (row-major it would be 1024 reads 4*I bytes apart per nonzero).
 *   fwd: gates[t, dir, :] = b_ih[dir] + b_hh[dir] + sum_{c<Dn} dense[t,c] wt[dir][c,:] + sum_{j in row ids[t]} values[j]
 *        wt[dir][Dn + indices[j], :], one fp32 fma chain per gate in exactly that order, into the (S*B, 2, 512) buffer that
 *        rlt_bilstm_rec_fwd consumes.  One launch, a workgroup per token row.
 *   bwd: from dgates (S*B, 2, 512) = the pre-activation gate gradients rlt_bilstm_rec_bwd leaves: dwt (I, 512) per direction
 *        with EVERY column written (=) - columns of terms absent from the batch are exact zeros -, db_ih = db_hh =
 *        colsum(dgates).  There is no dx: the input is data.  Needs two things beyond the forward's:
 *        - perm (S*B) int32: the token rows t ordered by (ids[t], t) ascending - a stable sort of the position-major ids;
 *        - the table's static term -> rows index, built once by the host: col_ptr (V+1) int64 / col_rows int32 / col_vals
 *          float32 = the table transposed (per term its rows ascending), cut into chunks of RLT_SPARSE_CHUNK entries:
 *          chunk_ptr (V+1) int32 = first chunk of each term, every term owning max(1, ceil(entries / RLT_SPARSE_CHUNK))
 *          consecutive chunks; chunk_col (n_chunks) int32 = the term of each chunk; multi_cols (n_multi) int32 = the terms
 *          that own more than one chunk, ascending.
 *        One workgroup per chunk adds its entries in index order (a row occurring at several token rows: in `perm` order);
 *        chunk 0 of a term writes the column, later chunks write partial sums into ws that one more launch adds in chunk
 *        order; the dense columns and biases are partial sums over blocks of 32 token rows reduced in block order.  No float
 *        atomics: bitwise reproducible.  ws: rlt_sparse_inproj_workspace(S, B, Dn, n_docs, V, n_chunks) bytes (0 for
 *        arguments out of range), 16-byte aligned.
 * A table row outside [0, n_docs), a term id outside [0, V) and a perm entry outside [0, S*B) are never dereferenced: they
 * contribute nothing (the Python binding tests the ids and raises, as for rlt_neighbor_features).  The static index is trusted
 * as far as its own arrays go (col_ptr within col_rows / col_vals); a chunk table that does not fit V and n_chunks writes nothing.
 * Errors before any launch: RLT_E_ARG (a NULL member or pointer, non-positive S, B, Dn, V, n_docs, n_chunks < V, n_multi
 * inconsistent with n_chunks), RLT_E_SHAPE (Dn > 16, B*S or Dn + V >= 2^31), RLT_E_ALIGN (weights, gradients, gates, ws off
 * 16 bytes; indptr / col_ptr off 8; any other array off 4), RLT_E_WORKSPACE.
 * Plain fp32 (no `precision` argument): a bandwidth kernel.  Algorithmic bytes per pass: 4 KB per nonzero of the batch, plus
 * the 4 KB x I gradient written once by the backward. */
#define RLT_SPARSE_CHUNK 256
typedef struct rlt_sparse_batch {
    const float* dense; const int32_t* ids; const int32_t* perm;                         /* perm: backward only */
    const int64_t* indptr; const int32_t* indices; const float* values;                  /* the table, CSR */
    const int64_t* col_ptr; const int32_t* col_rows; const float* col_vals;              /* backward only: the table by term */
    const int32_t *chunk_col, *chunk_ptr, *multi_cols;                                   /* backward only */
    int Dn, n_docs, V, n_chunks, n_multi;
} rlt_sparse_batch;
size_t rlt_sparse_inproj_workspace(int S, int B, int Dn, int n_docs, int V, int n_chunks);
int rlt_sparse_inproj_fwd(const rlt_sparse_batch* sb, int S, int B, const float* wt_fwd, const float* wt_rev,
                          const float* b_ih_fwd, const float* b_hh_fwd, const float* b_ih_rev, const float* b_hh_rev,
                          float* gates, void* stream);
int rlt_sparse_inproj_bwd(const rlt_sparse_batch* sb, int S, int B, const float* dgates, float* dwt_fwd, float* dwt_rev,
                          float* db_ih_fwd, float* db_hh_fwd, float* db_ih_rev, float* db_hh_rev,
                          void* ws, size_t ws_bytes, void* stream);
/* rlt_bilstm_fwd / rlt_bilstm_bwd with layer 0 fed by a sparse batch (models/Bicut.py:10,18 on the input above): layer 0's
 * gates, dW_ih and biases come from the two entry points above, the recurrences, the stash layout (RLT_OP_BILSTM_STASH) and
 * layer 1 are those of the dense stack.  w[0].w_ih / g[0].w_ih are the COLUMN-MAJOR (I, 512) buffers.  ws:
 * rlt_bilstm_sparse_workspace bytes (the dense stack's scratch at 256 inputs + the sparse backward's), 256-byte aligned. */
size_t rlt_bilstm_sparse_workspace(int S, int B, int Dn, int n_docs, int V, int n_chunks);
int rlt_bilstm_sparse_fwd(const rlt_sparse_batch* sb, const rlt_lstm_layer_weights* w, int S, int B, float* h_out,
                          void* stash, size_t stash_bytes, void* ws, size_t ws_bytes, int precision, void* stream);
int rlt_bilstm_sparse_bwd(const rlt_sparse_batch* sb, const rlt_lstm_layer_weights* w, const float* h_out, const float* dh_out,
                          int S, int B, void* stash, size_t stash_bytes, const rlt_lstm_layer_grads* g,
                          void* ws, size_t ws_bytes, int precision, void* stream);

/* ------------------------------------------------------------------ layout helpers
 * (B,S,F) user layout <-> (S*B,F) position-major */
int rlt_to_position_major(const float* x_bsf, int B, int S, int F, float* x_sbf, void* stream);
int rlt_from_position_major(const float* x_sbf, int B, int S, int F, float* x_bsf, void* stream);
/* Choopy input: out[(s*B+b), 0] = score[b,s]; out[.., 1+c] = pe[s,c] (models/Choopy.py:19-20).
 * E = 1 + pe columns (128). */
int rlt_choopy_embed(const float* score_bs, const float* pe, int B, int S, int E, float* out, void* stream);

/* ------------------------------------------------------------------ decision heads (M4, M6)
 * Up to 3 heads Linear(E,1) over the same position-major activations x (S*B,E), each followed
 * by softmax over the S positions of a list (kind 0), a sigmoid (1) or nothing (2):
 * models/AttnCut.py:11-14,19; models/MtAttnCut.py:11-19,24-26.
 *   w: (n_heads,E), b: (n_heads).  out: (n_heads,B,S) in the reference's (B,S) layout.
 * bwd: dout (n_heads,B,S) -> dx (S*B,E) (overwritten, or += with accumulate), dw (n_heads,E), db (n_heads).
 */
#define RLT_HEAD_SOFTMAX  0
#define RLT_HEAD_SIGMOID  1
#define RLT_HEAD_IDENTITY 2
int rlt_heads_fwd(const float* x, const float* w, const float* b, const int* kinds, int n_heads,
                  int S, int B, int E, float* out, void* stream);
size_t rlt_heads_bwd_workspace(int n_heads, int S, int B, int E);
int rlt_heads_bwd(const float* x, const float* w, const int* kinds, int n_heads,
                  const float* out, const float* dout, int S, int B, int E,
                  float* dx, int accumulate_dx, float* dw, float* db,
                  void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ hazard cut head (csrc/hazard.hip)
 * One Linear(E,1) head whose logit is a STOP logit: a discrete-time hazard parametrisation of the cut distribution, which the
 * reference does not have (its heads are Linear -> Softmax over all S positions).  0-based positions s = 0..S-1;
 * x (S*B,E) position-major, w (E), b (1), offset (S) fp32 or NULL - all device memory.
 *   z_s    = fp32 dot(x_s, w) + b (+ offset_s), accumulated in the order of the softmax heads above
 *   s < S-1:  stop_s = h_s = sigmoid(z_s),  L_s = - sum_{j<s} softplus(z_j),  p_s = exp(log sigmoid(z_s) + L_s)
 *   s = S-1:  stop = 1,  p = exp(L_{S-1})  (the remaining mass: "cut at S" cuts nothing); z_{S-1} is written, not used
 * i.e. p_s = h_s prod_{j<s} (1 - h_j), a distribution over the S cuts; S = 1 gives p = [1], stop = [1].  Everything after the
 * dot is float64 on the device (softplus, log-sigmoid and exp in their overflow-safe forms) and rounded to fp32 once.
 * PREFIX GUARANTEE: the sum over j < s runs in position order and is never formed as "total minus suffix", so p[b,s],
 * stop[b,s] and z[b,s] depend, to the bit, only on rows <= s of list b.  The one exception is p[b,S-1], the remainder.
 * Deep in a list p underflows to 0, as a softmax head's does; stop does not.
 *   fwd: p, z (B,S) required, stop (B,S) or NULL; in the reference's (B,S) layout.
 *   bwd: reads z and nothing else of the forward (a saturated h loses nothing); dp (B,S), dstop (B,S) or NULL.  It recomputes
 *        h, p, L from z in float64, takes T_j = sum_{k>j} p_k dp_k by a reverse scan in fixed order, and
 *          j < S-1:  dz_j = (1-h_j) p_j dp_j - h_j T_j + dstop_j h_j (1-h_j);      dz_{S-1} = 0 exactly
 *        then dx (S*B,E) = dz w (overwritten, or += with accumulate_dx), dw (E) = sum dz x, db (1) = sum dz: per-list partial
 *        rows in ws, then a fixed-order column reduction.  ws: rlt_hazard_head_bwd_workspace(S,B,E) bytes, 0 for arguments
 *        out of range.
 * Limits, those of the heads above: 1 <= S <= 1024, B >= 1, E % 64 == 0, E <= 1024 and at most 4 loads per lane and row (a
 * lane loads 4 floats where E % 256 == 0, 2 where E % 128 == 0, else 1: E = 64, 128, 192, 256, 384, 512, 768, 1024).  Errors, in this order, before any launch: RLT_E_ARG (a required
 * pointer NULL, a size not positive), RLT_E_SHAPE (the limits), RLT_E_ALIGN (x, w, dx off 16 bytes), RLT_E_WORKSPACE.
 * No atomics, no allocation, no host synchronisation; two calls give the same bits.  Algorithmic bytes: fwd reads x once,
 * 4 S B E, and writes 12 S B; bwd reads x and writes dx once, 8 S B E (12 S B E with accumulate_dx), reads 12 S B and moves
 * 8 B (E+4) of partial rows: those of a one-head softmax pass over the same shape. */
int rlt_hazard_head_fwd(const float* x, const float* w, const float* b, const float* offset, int S, int B, int E,
                        float* p, float* stop, float* z, void* stream);
size_t rlt_hazard_head_bwd_workspace(int S, int B, int E);
int rlt_hazard_head_bwd(const float* x, const float* w, const float* z, const float* dp, const float* dstop,
                        int S, int B, int E, float* dx, int accumulate_dx, float* dw, float* db,
                        void* ws, size_t ws_bytes, void* stream);
/* streaming: the hazard head one CHUNK of positions t0 .. t0+C-1 at a time, with the stop decision taken on the device
 * (csrc/hazard.hip; tests/test_stream_abi.py, tests/test_hazard_append_gpu.py).  Inference only.
 *   x (C*B,E) position-major: the encoder output of the chunk, row i*B + b = position t0+i of list b.  offset (C) or NULL: the
 *   chunk's slice offset[t0 .. t0+C-1] of the list's prior offset.  carry (B) float64, in and out: L = - sum_{j<t0} softplus(z_j)
 *   of each list - the caller ZEROES it before the chunk at t0 = 0 and hands it on unchanged from call to call.
 *   stop (B,C) required; p, z (B,C) or NULL.  final != 0: the chunk ends the list; only then does its last row take stop = 1 and
 *   p = the remaining mass.  Without it every row is an inner row (stop = sigmoid(z), p = exp(log sigmoid(z) + L)).
 *   The dot, the float64 terms and the rounding are those of rlt_hazard_head_fwd (one device text), the prefix sum starts from
 *   carry and continues in position order.  PREFIX STATEMENT: stop and z of position t0+i are, to the bit, those of the one-shot
 *   call on the whole list, whatever the chunking (the last position under final included).  p is the fp32 rounding of a float64
 *   whose prefix sum is associated per chunk: it differs from the one-shot float64 by rounding errors of that sum (about 1e-16
 *   relative to L), so its fp32 rounding is the one-shot p except where such a difference straddles an fp32 rounding boundary; one
 *   chunk of the whole list is the one-shot computation itself.  carry after the last chunk is - sum_j softplus(z_j).
 *   DECISION: active (B) int32 in and out, or NULL (then no decision is taken and k is not read).  For a list with
 *   active[b] != 0, the first row i of the chunk with (double)stop[b,i] >= tau - the comparison of rlt_cut_sweep's
 *   RLT_SWEEP_FIRST_ABOVE (a NaN compares false) - sets k[b] = t0 + i + 1 and active[b] = 0; under final a list that no row stopped
 *   stops at the last row, k[b] = t0 + C.  The chunk's rows behind the stop are still written (the list retires for the NEXT call).
 *   A list with active[b] == 0 on entry is skipped: its carry, k, stop, p and z are UNTOUCHED.
 * Limits and errors, those of the hazard head with C for S, before any launch and in this order: RLT_E_ARG (x, w, b, carry or stop
 * NULL, active without k, C / B / E not positive, t0 < 0), RLT_E_SHAPE, RLT_E_ALIGN (x, w off 16 bytes).  No atomics, no
 * allocation, no host synchronisation; two calls from the same carry / active / k give the same bits.  One stream: a chunk reads
 * what the chunk before it left in carry and active.  Algorithmic bytes per active list: reads 4*C*E, writes up to 12*C + 16. */
int rlt_hazard_head_append(const float* x, const float* w, const float* b, const float* offset, int t0, int C, int B, int E,
                           int final, double* carry, double tau, int32_t* active, int32_t* k, float* stop, float* p, float* z,
                           void* stream);

/* ------------------------------------------------------------------ streaming: compacting the live lists
 * A retired list still occupies a slot of the batch: the two append calls above skip it, the chunk's GEMMs and LayerNorms do not,
 * and what the attention skips is one cache row in every B.  These two calls take the retired slots OUT of a running stream
 * (csrc/stream_compact.hip; inference only).  tests: tests/test_stream_compact_abi.py, tests/test_stream_compact_gpu.py against the
 * numpy restatement tests/stream_compact_restate.py; utils/stream.py drives them (tests/test_stream_compact_model_gpu.py).
 * rlt_stream_compact_plan: the slot map and the per-list state.  B: the slots of the stream as it stands; B_full: the lists the
 * stream started with.  All arrays are device memory.
 *   active (B) int32, required: a slot is LIVE iff active[b] != 0 (any non-zero value).  origin (B) int32: the original list number
 *   of each slot, or NULL for the identity.  carry (B) float64 with carry_out (B), or both NULL.  k (B) int32 with k_full (B_full),
 *   or both NULL.
 *   slot_src (B): entries 0 .. n_live-1 are the live slots in ASCENDING order (a stable partition); the entries behind are -1.
 *   origin_out (B): origin[slot_src[j]] for j < n_live, -1 behind.  carry_out[j] = carry[slot_src[j]] for j < n_live, copied
 *   bitwise (NaN payloads, -0.0); its entries >= n_live are UNTOUCHED.  k_full[origin[b]] = k[b] for every slot with
 *   active[b] == 0: a retired list hands its cut over before its slot disappears; an origin value outside [0, B_full) is skipped,
 *   not written, and the entries of k_full that belong to live or absent lists are UNTOUCHED.  n_live (1): an int32 in device
 *   memory - the host is not synchronised; the caller reads it back when it wants to size the next launches.
 *   One workgroup walks B in chunks of 1024 with ballot / popcount prefixes and a carried count: no atomics, one fixed order, two
 *   calls give the same bits; no allocation.  Made for a B of a few thousand (time at B = 8192 and 1,048,576: DESIGN.md); not tuned.
 *   Errors before any launch, in this order: RLT_E_ARG (active, slot_src, origin_out or n_live NULL; one half of a pair without
 *   the other; B or B_full not positive; B > B_full; an output pointer equal to an input pointer or to another output pointer),
 *   RLT_E_SHAPE (the index limit: B_full > 2^30), RLT_E_ALIGN (carry / carry_out off 8 bytes, an int array off 4).
 *   Algorithmic bytes: reads 4 B (+ 4 B origin, 8 B carry, 4 B k), writes 8 B (+ 8 n_live, 4 (B - n_live)) + 4.
 * rlt_kv_cache_compact: the K/V cache of one layer, gathered through the map.
 *   src (t0*B_src, W) position-major: the first t0 ranks of a cache of B_src slots, W = 2E floats a row.  dst (t0*B_dst, W).
 *   dst[(s*B_dst + j)*W ..] = src[(s*B_src + slot_src[j])*W ..] for s < t0, j < B_dst, copied bitwise (NaN payloads and signed
 *   zeros survive).  Rows of dst at or behind t0*B_dst are neither read nor written; src is not written.  A slot_src[j] outside
 *   [0, B_src) leaves row j of every rank UNTOUCHED: the kernel bounds what it reads by construction - it cannot validate device
 *   data without a synchronising copy.  The ranges [src, src + t0*B_src*W) and [dst, dst + t0*B_dst*W) must not overlap (checked
 *   on the host from the pointer values): there is no in-place form, it would race between workgroups.  t0 == 0 or B_dst == 0
 *   returns 0 without a launch (after the checks).  After the call dst is a cache of B_dst slots for rlt_seq_attention_append at
 *   the same t0: the append's arithmetic for a list does not depend on B or on the list's slot, so the stream continues bit for bit.
 *   An HBM-bound gather copy: 16-byte loads and stores, four rows in flight per lane group before the first store, the grid strided
 *   over (rank, destination slot), the map entry read once per row.  No atomics, no allocation, no host synchronisation.
 *   Errors before any launch, in this order: RLT_E_ARG (src, dst or slot_src NULL; t0 < 0; B_src < 1; B_dst < 0; B_dst > B_src;
 *   W < 1; overlap), RLT_E_SHAPE (W % 4 != 0; W > 2048; the index limits: t0*B_src*W >= 2^40 elements, B_src > 2^30),
 *   RLT_E_ALIGN (src or dst off 16 bytes).
 *   Algorithmic bytes: reads 4*t0*B_dst*W (+ 4*B_dst of the map), writes 4*t0*B_dst*W. */
int rlt_stream_compact_plan(const int32_t* active, const int32_t* origin, const double* carry, const int32_t* k, int B, int B_full,
                            int32_t* slot_src, int32_t* origin_out, double* carry_out, int32_t* k_full, int32_t* n_live,
                            void* stream);
int rlt_kv_cache_compact(const float* src, float* dst, const int32_t* slot_src, int t0, int B_src, int B_dst, int W, void* stream);

/* ------------------------------------------------------------------ probe heads (the probing study)
 * models/Classification.py:4-12 (TaskC), models/Rerank.py:4-12 (TaskR), models/Probe.py:30-53,102-122 (TowerClass /
 * TowerRerank as the six probes of Probe), with their training losses of verify_BMT.py:37-44,71-80 and
 * verify_probe.py:120-135,162-177: up to 8 heads Linear(E,1) on FROZEN position-major features x (S*B,E), each ending in
 *   RLT_PROBE_BCE     Sigmoid -> nn.BCELoss() (mean over B*S; log clamped at -100; gradient = torch's BCE backward with its
 *                     1e-12 clamp on s(1-s), then the sigmoid backward: a saturated sigmoid gets 0), or
 *   RLT_PROBE_RERANK  Softmax over the S positions of a list -> RerankLoss (utils/losses.py:99-141): max(0, mean_{y=0} s -
 *                     mean_{y=1} s + margin) over the whole batch, 0 with a zero gradient when a class is missing or the
 *                     argument is <= 0 (the hinge of rlt_mt_terms, from the same arithmetic).
 *   w (n_heads,E), b (n_heads), kinds (n_heads, host array); labels (B,S) exactly 0/1.  1 <= n_heads <= 8, 1 <= E <= 1024,
 *   1 <= S <= 1024, B >= 1.
 *   loss (n_heads): each head's own loss.  dw (n_heads,E), db (n_heads): each head's gradient of its own loss, overwritten;
 *   both NULL for an evaluation call (loss and out are the same).  out (n_heads,B,S): the activations, or NULL.  No dx.
 * ws: rlt_probe_heads_workspace(n_heads,S,B,E) bytes (0 for arguments out of range).  Three launches: one pass (a workgroup
 * per list, online-softmax sums for the rerank heads) writing one record per list, a fixed-order column reduction of the
 * records, and a one-workgroup finish (losses, hinge flag and 1/n_pos, 1/n_neg applied to dw); no atomics, bitwise
 * reproducible.  Algorithmic bytes: read x 4*S*B*E once (+ labels 4*B*S, out 4*n*B*S, the records 4*B*(n*E + 3n + 2)). */
#define RLT_PROBE_BCE    0
#define RLT_PROBE_RERANK 1
size_t rlt_probe_heads_workspace(int n_heads, int S, int B, int E);
int rlt_probe_heads(const float* x, const float* w, const float* b, const int* kinds, int n_heads,
                    int S, int B, int E, const float* labels, float margin,
                    float* loss, float* dw, float* db, float* out,
                    void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ neighbour-similarity input features (AttnCut's statistics)
 * data_prep/data_review.ipynb (cos_simi, simi_docs, simi_list) and data_prep/document_statics.ipynb (cos_similarity,
 * neighbor_sim): for every position of a ranked list the cosine similarity of its document to the documents ranked next to it,
 * once over the tf-idf vectors and once over the doc2vec vectors.
 *   sim(a, b) = (a . b) / (|a| |b|), 0 when the denominator is 0 or the quotient is NaN;
 *   position 0: sim(0, 1);  position S-1: sim(S-2, S-1);  position i in between: (sim(i-1, i) + sim(i, i+1)) / 2.
 * doc_ids (B,S) int32: the row of each ranked document in the tables, rank order; every id in [0, n_docs) - the caller's duty,
 * the kernel does not test it.  B >= 1, S >= 2, B * S < 2^31.
 * Dense table d2v (n_docs, D) float32, row stride ld_d2v >= D floats, D in 1..1024.  Sparse table in CSR: indptr (n_docs + 1)
 * int64, indices int32 strictly ascending within a row, values float64 (8-byte aligned); a row may be empty or of any length.
 * Either table may be NULL (the sparse one: all three pointers NULL), not both.
 * out: float32, position (b, i) at out + (b * S + i) * ld_out + col; the tf-idf similarity first, then the doc2vec one (one
 * column only when a table is NULL): col = 1, ld_out = 3 writes columns 1..2 of the packed model input X (B,S,3) in place.
 * Every sum, the square roots and the division are float64 (the doc2vec column too: products of two float32 are exact there);
 * the half-sum is rounded to float32 once.  One launch, no workspace: a wavefront owns 64 positions of a list, walks their
 * documents in rank order (one document of overlap on either side), keeps the previous dense row and both squared norms in
 * registers and the previous sparse row in LDS (rows over 128 entries are searched in place), and intersects two sparse rows
 * by a binary search per entry.  Fixed reduction order, no atomics: bitwise reproducible.
 * Algorithmic bytes per position: 4 (id) + 4 D (dense row) + 12 nnz (sparse row) + 8 (two outputs). */
int rlt_neighbor_features(const int32_t* doc_ids, int B, int S, int n_docs, const float* d2v, int D, int ld_d2v,
                          const int64_t* indptr, const int32_t* indices, const double* values,
                          float* out, int ld_out, int col, void* stream);

/* ------------------------------------------------------------------ MMOE gates / mixture (M7)
 * models/MMOECut.py:93-94: gate[t][b][:] = softmax_e( flatten_s(h[b]) @ w_gate[t] ), h the BiLSTM
 * output (position-major (S*B,C), C = 256), w_gate[t]: (S*C, n_e) row index s*C + c.
 * models/MMOECut.py:101-102: mixed[t][tok][:] = sum_e gate[t][b][e] * expert[e][tok][:].
 *   gates out: (n_tasks,B,n_e).  n_e <= 8, n_tasks <= 3.
 * bwd of the gate: from dgate (n_tasks,B,n_e): dh (S*B,C) = or += (accumulate_dh), dw_gate[t] (S*C,n_e) =.
 * mix fwd: experts[e] (S*B,E), e < n_e (host array of device pointers) -> mixed (n_tasks,S*B,E).
 * mix bwd: dmixed (n_tasks,S*B,E) -> dexperts[e] (S*B,E) = ; dgate (n_tasks,B,n_e) = .
 * w_gate / dw_gate / experts / dexperts are HOST arrays of device pointers.
 */
int rlt_mmoe_gate_fwd(const float* h, const float* const* w_gate, int n_tasks, int n_e,
                      int S, int B, int C, float* gates, void* stream);
size_t rlt_mmoe_gate_bwd_workspace(int n_tasks, int n_e, int S, int B, int C);
int rlt_mmoe_gate_bwd(const float* h, const float* const* w_gate, const float* gates, const float* dgates,
                      int n_tasks, int n_e, int S, int B, int C,
                      float* dh, int accumulate_dh, float* const* dw_gate,
                      void* ws, size_t ws_bytes, void* stream);
int rlt_mmoe_mix_fwd(const float* const* experts, const float* gates, int n_tasks, int n_e,
                     int S, int B, int E, float* mixed, void* stream);
int rlt_mmoe_mix_bwd(const float* const* experts, const float* gates, const float* dmixed,
                     int n_tasks, int n_e, int S, int B, int E,
                     float* const* dexperts, float* dgates, void* stream);

/* ------------------------------------------------------------------ BiCut (section 8f row N4)
 * Two-class head of models/Bicut.py:11-16: position-major logits z (S*B, 2) -> Dropout on the logits -> softmax over
 * the two classes {0: truncate, 1: continue}; out is (B, S, 2) in the reference's layout.  bwd: dz (S*B, 2). */
int rlt_pair_softmax_fwd(const float* z, int B, int S, float drop_p, uint32_t seed, float* out, void* stream);
int rlt_pair_softmax_bwd(const float* out, const float* dout, int B, int S, float drop_p, uint32_t seed, float* dz, void* stream);
/* BiCutLoss (utils/losses.py:11-45) and its gradient in one pass.  out (B,S,2), labels (B,S) in {0,1}.
 * mask = positions up to and including the last one whose argmax is class 0 (all positions when none is);
 * metric_nci != 0: reward (0, -1/log2(j+2)) for label 1, (0, (j+1)/alpha) for label 0; otherwise ((1-alpha)/r, 0) and
 * (0, alpha/(1-r)).  loss = sum(out * mask * reward) / B; dout = mask * reward / B; per_list (B) unnormalised. */
int rlt_bicut_loss(const float* out, const float* labels, int B, int S, int metric_nci, float alpha, float r,
                   float* per_list, float* loss, float* dout, void* stream);

/* ------------------------------------------------------------------ WassDistLoss (section 8f row N4)
 * utils/losses.py:236-311: entropic optimal transport between the B predicted distributions p (B,S) and the B label
 * vectors (B,S) of a batch: squared-distance cost, uniform marginals, at most max_iter log-domain Sinkhorn iterations
 * with regularisation eps, stopped after the iteration whose sum |u - u_prev| < thresh (reference: 0.1; decided on the
 * device, no host synchronisation), loss = sum(pi * C).  fwd records the iterations in ws; bwd replays them in reverse
 * and writes dp = gscale[0] * d(loss)/dp (gscale NULL = 1).  ws: rlt_wass_loss_workspace(B, max_iter) bytes, the
 * same buffer for fwd and bwd. */
size_t rlt_wass_loss_workspace(int B, int max_iter);
int rlt_wass_loss_fwd(const float* p, const float* labels, int B, int S, float eps, int max_iter, float thresh,
                      float* loss, void* ws, size_t ws_bytes, void* stream);
int rlt_wass_loss_bwd(const float* p, const float* labels, const float* gscale, int B, int S, float eps, int max_iter,
                      void* ws, size_t ws_bytes, float* dp, void* stream);

/* ------------------------------------------------------------------ optimizer (N2, run.py:104,129)
 * torch.optim.Adam with coupled L2 (grad += wd * p), bias correction, eps outside the sqrt,
 * on a flat fp32 bucket.  step: 1-based step count. */
int rlt_adam_step(float* p, const float* g, float* m, float* v, size_t n, int step,
                  float lr, float beta1, float beta2, float eps, float weight_decay, void* stream);

/* ------------------------------------------------------------------ guarded optimizer step (csrc/optim.hip)
 * torch.nn.utils.clip_grad_norm_ followed by torch.optim.Adam, with the gradient norm per step and per parameter tensor and a
 * skip of steps whose gradient is not finite - decided on the device: no host read, no allocation, every launch ordered on
 * `stream`, and no scalar argument that changes from step to step (the step count lives in the state).
 *
 * struct rlt_opt_state: 104 bytes of DEVICE memory owned by the caller, 8-byte aligned, zero-initialised by the caller before
 * the first step and written only by the two entry points below (every member is 8 bytes wide up to `coef`: an int64 view of
 * 13 words reads it).
 *   step, skipped, clipped    steps applied / skipped as non-finite / applied with a coefficient below 1
 *   nonfinite, nan_count      the last norm call: NaN and +-Inf elements of the bucket, and the NaN among them
 *   sumsq, norm, max_abs      the last norm call: float64 sum of squares and max |g| over the FINITE elements; norm = sqrt of
 *                             sumsq, or what torch's norm of such a gradient is when nonfinite > 0: NaN if nan_count > 0, else Inf
 *   norm_sum, norm_max, norm_steps   running sum and maximum of `norm` over the norm calls whose gradient was finite, and their
 *                             number (a trainer reads them once per epoch and zeroes them)
 *   coef                      the last norm call's clip coefficient
 *   apply, bc1, bc2_sqrt      scratch of the guarded step: its decision and the bias corrections of the step it applies
 * struct rlt_grad_seg: one segment's figures - sumsq and max_abs over its finite elements, nonfinite its NaN / Inf count.
 *
 * The norm: one read of the flat fp32 gradient bucket g (n elements, n % 4 == 0, n <= 2^46, 16-byte aligned).  A segment is
 * one slot of the bucket: seg_offsets (n_seg + 1) int64 in DEVICE memory, ascending multiples of 4 with seg_offsets[0] == 0 and
 * seg_offsets[n_seg] == n; seg_out (n_seg) receives the segments' figures.  n_seg == 0 with seg_offsets NULL is one segment
 * over the whole bucket (seg_out may then be NULL).  The bucket's figures are the fixed-order sum of the segments' and go to
 * `state` with the norm and coef = min(1, max_norm / (norm + 1e-6)) - torch's rule, formed in float64 and rounded to float
 * once; a NaN norm gives a NaN coefficient as in torch.  max_norm <= 0 or +Inf: no clipping, coef is exactly 1.0f.
 * Every sum is float64 in an order fixed by n and the segment table alone (the bucket is cut into chunks of
 * RLT_GRAD_NORM_CHUNK elements at absolute positions; csrc/optim.hip states the order): no float atomics, the same bits
 * from every grid and every call.  The grid is min(chunks, RLT_GRAD_NORM_GRID) workgroups, one chunk per workgroup and trip;
 * the two query functions return those two constants.  Three launches: the pass, the segments, the bucket.
 * ws: the workspace query's bytes, 16-byte aligned (0 for n == 0, n % 4 != 0 or n_seg < 0).
 * Errors before any launch: RLT_E_ARG (g, ws or state NULL, n == 0, n_seg < 0, max_norm NaN, n_seg > 0 without seg_offsets
 * and seg_out, n_seg == 0 with seg_offsets; a segment table that is not as described above when the HOST can read it - pinned
 * or managed memory, or a process without a device; a table in device memory cannot be read without a synchronising copy: it is
 * the caller's duty, and the kernels stay inside g, ws and seg_out whatever it holds), RLT_E_SHAPE (n % 4, n > 2^46),
 * RLT_E_ALIGN, RLT_E_WORKSPACE (ws off 16 bytes or too small).
 * Algorithmic bytes: 4n read (+ 32 bytes written per chunk of 16 KB).
 *
 * The guarded step reads coef and nonfinite from `state` (so it follows a norm call on the same stream):
 *   skip_nonfinite != 0 and nonfinite != 0: p, m, v stay byte for byte as they were, `step` too, skipped += 1;
 *   otherwise t = ++step, clipped += 1 when coef < 1, and per element the arithmetic of rlt_adam_step at step t on
 *   gr = g * coef + weight_decay * p - clipping acts on the raw gradient, the coupled L2 term is added after it, as
 *   clip_grad_norm_ followed by torch.optim.Adam(weight_decay) does - with the bias corrections 1 - pow(beta, t) formed
 *   in float64 on the device and rounded to float.  g is not modified.  Without skip_nonfinite a non-finite gradient or
 *   coefficient propagates into p, m and v as it does in torch.
 * p, g, m, v: n elements each, n % 4 == 0, 16-byte aligned (RLT_E_SHAPE / RLT_E_ALIGN).  Two launches: the decision (one lane)
 * and the update.  Algorithmic bytes: 16n read, 12n written, as rlt_adam_step. */
#define RLT_GRAD_NORM_CHUNK 4096
#define RLT_GRAD_NORM_GRID  2048
typedef struct rlt_opt_state {
    int64_t step, skipped, clipped;
    int64_t nonfinite, nan_count;
    double sumsq, norm, max_abs;
    double norm_sum, norm_max;
    int64_t norm_steps;
    float coef;
    int32_t apply;
    float bc1, bc2_sqrt;
} rlt_opt_state;
typedef struct rlt_grad_seg { double sumsq; int64_t nonfinite; double max_abs; } rlt_grad_seg;
size_t rlt_grad_norm_chunk(void);
int rlt_grad_norm_grid(void);
size_t rlt_grad_norm_workspace(size_t n, int n_seg);
int rlt_grad_norm(const float* g, size_t n, const int64_t* seg_offsets, int n_seg, float max_norm,
                  void* ws, size_t ws_bytes, rlt_grad_seg* seg_out, rlt_opt_state* state, void* stream);
int rlt_adam_step_guarded(float* p, const float* g, float* m, float* v, size_t n, rlt_opt_state* state,
                          float lr, float beta1, float beta2, float eps, float weight_decay, int skip_nonfinite, void* stream);

/* ------------------------------------------------------------------ training recipe in one Adam pass (csrc/recipe.hip)
 * A learning-rate schedule, per-tensor parameter groups (learning-rate factor, weight decay, freezing), coupled or decoupled
 * (AdamW) weight decay and an exponential moving average of the parameters, in the one streaming pass of the guarded step: no host
 * read, no allocation, and no scalar the host advances - the schedule is evaluated on the device from the applied-step count of
 * struct rlt_opt_state, so a skipped step does not advance it.
 *
 * struct rlt_recipe: a HOST struct read at call time.  sched_kind: RLT_SCHED_*; weight_decay: the one group's, used when
 * n_seg == 0; ema_decay 0: no average (ema must then be NULL); skip_nonfinite, use_norm, decoupled, ema_warmup: 0 / 1.
 * struct rlt_recipe_group: one segment's {lr_scale, weight_decay}; groups = n_seg of them in DEVICE memory, 8-byte aligned, in the
 * order of seg_offsets - the table of rlt_grad_norm, checked on the host when the host can read it exactly as there.  n_seg == 0
 * with seg_offsets and groups NULL is one group: lr_scale 1, the recipe's weight_decay.
 * struct rlt_recipe_state: 32 bytes of DEVICE memory owned by the caller, 8-byte aligned, zero-initialised before the first step
 * (an int64 view of 4 words reads it; lr, ema_decay, coef are words 4, 5, 6 of its float view):
 *   lr64, lr       the schedule's float64 value at the last applied step, and that value rounded to float - what the step used
 *   ema_updates    EMA updates so far;  ema_decay: the decay d of the last one
 *   coef           scratch of the decision: the clip coefficient the update applies
 * The decision's other scratch is apply, bc1, bc2_sqrt of struct rlt_opt_state, as in the guarded step.
 *
 * The decision (one lane).  use_norm != 0: coef and nonfinite come from `state`, so a rlt_grad_norm call precedes on the same
 * stream; otherwise coef = 1 and nothing is skipped.  use_norm, skip_nonfinite and nonfinite != 0: the step is skipped - no byte of
 * p, m, v, ema or the recipe state changes, `step` stays, skipped += 1.  Otherwise t = ++step, clipped += 1 when coef < 1, the bias
 * corrections as in the guarded step (float64 pow, once), and the schedule in float64, each expression evaluated left to right as
 * written with every integer converted to float64 first, B = (double)base_lr, F = B * (double)min_lr_ratio, W = warmup_steps,
 * T = total_steps:
 *   t <= W                 B * t / W
 *   W < t <= T  CONSTANT   B
 *               LINEAR     F + (B - F) * (T - t) / (T - W)
 *               COSINE     F + (B - F) * 0.5 * (1.0 + cos(pi * (t - W) / (T - W)))          pi = 3.14159265358979323846
 *   t > T                  F (B for CONSTANT, which never reads T)
 * rounded to float once.  With ema: d = ema_decay, or with ema_warmup min((double)ema_decay, (1.0 + k) / (10.0 + k)) rounded to
 * float, k = the EMA updates before this one.  rlt_lr_at evaluates the same expression on the host (no device needed; t >= 1; NaN
 * for a recipe the step would refuse): equal bit for bit to the device's for CONSTANT and LINEAR, up to the two cos for COSINE.
 *
 * The update, per element of segment s, lr_s = lr * lr_scale[s] and wd_s = weight_decay[s] in float, gr and the moments as in the
 * guarded step (m = b1 m + (1 - b1) gr, v = b2 v + (1 - b2) gr gr, denom = sqrt(v) / bc2_sqrt + eps, u = (lr_s / bc1) * (m / denom)):
 *   coupled     gr = g * coef + wd_s * p (the term is left out when wd_s == 0),   p = p - u
 *   decoupled   gr = g * coef,   p = p - (lr_s * wd_s * p + u): torch.optim.AdamW's p * (1 - lr_s wd_s) - u with the decay taken
 *               from the parameter before the update, written so that p is rounded once at its own magnitude
 *   ema         ema = d * ema + (1 - d) * p with the new p; the caller initialises ema to a copy of p
 *   lr_scale[s] == 0 freezes the segment: none of its bytes in p, m, v, ema is read or written.
 * g is not modified.  The bucket is cut into chunks of RLT_RECIPE_CHUNK elements at absolute positions, one per workgroup and trip
 * of a grid of min(chunks, RLT_RECIPE_GRID) workgroups (the two query functions return the constants); a chunk's first segment is
 * found by one search of the table, the boundaries inside it by walking forward: no per-element side array.  Two launches.
 * Algorithmic bytes: 20n read, 16n written with ema; 16n read, 12n written without (+ the table: 16 n_seg bytes).
 * Errors before any launch: RLT_E_ARG (p, g, m, v, state, rstate or recipe NULL; n == 0; n_seg < 0; n_seg > 0 without both tables
 * or n_seg == 0 with one; a NaN in the recipe; sched_kind outside its codes; warmup_steps < 0; LINEAR or COSINE with
 * total_steps <= warmup_steps; min_lr_ratio outside [0, 1]; ema_decay outside [0, 1); ema without ema_decay or ema_decay without
 * ema; a host-readable segment table that is not as rlt_grad_norm wants it), RLT_E_SHAPE (n % 4, n > 2^46), RLT_E_ALIGN (p, g, m, v,
 * ema off 16 bytes; state, rstate, seg_offsets, groups off 8).
 *
 * rlt_swap_f32 exchanges two fp32 buffers in place (n % 4 == 0, 16-byte aligned, not overlapping: RLT_E_SHAPE / RLT_E_ALIGN /
 * RLT_E_ARG): evaluating with the averaged weights costs no second bucket.  Algorithmic bytes: 8n read, 8n written. */
#define RLT_SCHED_CONSTANT 0
#define RLT_SCHED_LINEAR   1
#define RLT_SCHED_COSINE   2
#define RLT_RECIPE_CHUNK 4096
#define RLT_RECIPE_GRID  2048
typedef struct rlt_recipe {
    float base_lr, beta1, beta2, eps, weight_decay;
    int32_t decoupled;
    int32_t sched_kind;
    int32_t ema_warmup;
    int64_t warmup_steps, total_steps;
    float min_lr_ratio, ema_decay;
    int32_t skip_nonfinite, use_norm;
} rlt_recipe;
typedef struct rlt_recipe_group { float lr_scale, weight_decay; } rlt_recipe_group;
typedef struct rlt_recipe_state {
    double lr64;
    int64_t ema_updates;
    float lr, ema_decay, coef, reserved;
} rlt_recipe_state;
size_t rlt_recipe_chunk(void);
int rlt_recipe_grid(void);
double rlt_lr_at(const rlt_recipe* recipe, int64_t t);
int rlt_adam_step_recipe(float* p, const float* g, float* m, float* v, float* ema, size_t n, const int64_t* seg_offsets,
                         const rlt_recipe_group* groups, int n_seg, rlt_opt_state* state, rlt_recipe_state* rstate,
                         const rlt_recipe* recipe, void* stream);
int rlt_swap_f32(float* a, float* b, size_t n, void* stream);

/* ------------------------------------------------------------------ paired significance tests (csrc/compare.hip)
 * Is system m better than the baseline on the same queries?  base (Q) and sys (M rows of Q, leading dimension ld >= Q) are float32
 * per-query values in one query order (columns of run.py --report-out).  One call leaves, per system, a record of
 * RLT_CMP_WORDS 8-byte words (int64 unless marked f64) and, optionally, the R replicate statistics of two resampling tests.
 * d[m][q] = (double)sys[m][q] - (double)base[q], exact in float64.  A pair with a NaN or Inf member is counted in NONFINITE, enters
 * the resampling with d = 0 and stays out of N, the sums and the win / tie / loss counts.
 *   RLT_CMP_N          finite pairs                       RLT_CMP_WINS / _TIES / _LOSSES   d > 0, d == 0, d < 0
 *   RLT_CMP_SUM_BASE   f64, sum of base                   RLT_CMP_NONFINITE                pairs with a NaN / Inf member
 *   RLT_CMP_SUM_SYS    f64, sum of sys                    RLT_CMP_T_OBS                    f64, the observed statistic: sum of d
 *   RLT_CMP_SUM_D      f64, sum of d                      RLT_CMP_RAND_GE                  replicates with |T_r| >= |T_obs|
 *   RLT_CMP_SSD        f64, sum of (d - mean)^2, a        RLT_CMP_BOOT_LE0 / _BOOT_GE0     bootstrap sums <= 0 / >= 0
 *                      second pass about SUM_D / N        RLT_CMP_RESAMPLES, RLT_CMP_FORM  R and the plan's form; RESERVED: 0
 * Randomization (Fisher sign flip): T_r = sum_q s(r,q) d[m][q], s = -1 where bit (q & 31) of word(r, q >> 5) is set, else +1.
 * Paired bootstrap: B_r = sum_{j<Q} d[m][idx(r,j)], idx(r,j) = (u(r,j) * Q) >> 32 on the 64-bit product.  All M systems see the
 * same signs and the same indices.  With mix32 and row_hash the two 32-bit functions of csrc/common.h (arithmetic mod 2^32):
 *   draw(seed, r, c) = mix32(row_hash(seed, r) ^ mix32(c + 0x7F4A7C15))
 *   word(r, k) = draw(seed, r, k)         u(r, j) = draw(mix32(seed ^ 0xA511E9B3), r, j)
 * a pure function of (seed, r, c).  idx is floor(u Q / 2^32): each index has probability within 2^-32 of 1/Q, a relative bias of
 * at most Q / 2^32.  T_obs is formed by the replicate code with every sign plus, in the same order: a replicate that draws all
 * plus or all minus ties with it bit for bit.  Every sum is float64 in an order fixed by Q, M and R (csrc/compare.hip states
 * it); no float atomics; two calls give the same bits.
 * rand_stat, boot_stat: (M, R) float64, row m = T_r / B_r of system m; either may be NULL.
 * Limits: 1 <= Q <= 2^26, 1 <= M <= RLT_COMPARE_MAX_SYSTEMS, 0 <= R <= 2^20.
 * The plan: RLT_COMPARE_RESIDENT while Q <= resident_max_q = 160 KB / (8 M) - d sits in LDS (lds_bytes), a workgroup of 16
 * wavefronts walks 16 * replicates_per_wave replicates, a wavefront per replicate; RLT_COMPARE_CHUNKED beyond - the grid runs over
 * replicates x `chunks` chunks of `chunk` = RLT_COMPARE_CHUNK queries, partial sums [chunk][m][r] go to the workspace and are added
 * in ascending chunk order; the bootstrap gathers then go through L2 / global memory.  `chunk` and resident_max_q are filled in
 * both forms.  The workspace holds d (8 Q M bytes), the partials (16 chunks M (R + 1) bytes), the sums and the moment records.
 * The plan and the workspace query answer without a GPU (0 bytes for dimensions outside the limits).  Seven launches, no
 * allocation, no host synchronisation.
 * Errors before any launch: RLT_E_ARG (base, sys, ws, record or the plan's out NULL; Q < 1, M < 1, R < 0; ld < Q), RLT_E_SHAPE (Q,
 * M or R above its limit), RLT_E_ALIGN (base / sys off 4 bytes, record / rand_stat / boot_stat off 8), RLT_E_WORKSPACE (ws off 16
 * bytes or too small). */
#define RLT_COMPARE_RESIDENT 1
#define RLT_COMPARE_CHUNKED  2
#define RLT_COMPARE_CHUNK    32768
#define RLT_COMPARE_MAX_SYSTEMS 8
#define RLT_CMP_N 0
#define RLT_CMP_SUM_BASE 1
#define RLT_CMP_SUM_SYS 2
#define RLT_CMP_SUM_D 3
#define RLT_CMP_SSD 4
#define RLT_CMP_WINS 5
#define RLT_CMP_TIES 6
#define RLT_CMP_LOSSES 7
#define RLT_CMP_NONFINITE 8
#define RLT_CMP_T_OBS 9
#define RLT_CMP_RAND_GE 10
#define RLT_CMP_BOOT_LE0 11
#define RLT_CMP_BOOT_GE0 12
#define RLT_CMP_RESAMPLES 13
#define RLT_CMP_FORM 14
#define RLT_CMP_RESERVED 15
#define RLT_CMP_WORDS 16
struct rlt_paired_compare_plan { int form, chunk, resident_max_q, chunks, replicates_per_wave, lds_bytes; };
int rlt_paired_compare_plan(int Q, int M, int R, struct rlt_paired_compare_plan* out);
size_t rlt_paired_compare_workspace(int Q, int M, int R);
int rlt_paired_compare(const float* base, const float* sys, int ld, int Q, int M, int R, uint32_t seed, void* ws, size_t ws_bytes,
                       int64_t* record, double* rand_stat, double* boot_stat, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RLT_HIP_H */
