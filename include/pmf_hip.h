/*
 * pmf_hip.h -- C-ABI of libpmf_hip.so: the MI355X (gfx950) engine for the
 * latent-factor update loop of rogeliolopezcamara/prob-matrix-factorization.
 *
 * The reference has no FFI of its own: its hot path is the body of
 * `fit()` / `predict()` / `evaluate_rmse()` of the classes in src/models/ (pure NumPy).
 * This header is the boundary a replacement binds instead: every entry point
 * names the reference code it stands in for (paths relative to the reference
 * repository root).  The binding a maintainer adds on the reference side is a
 * ctypes stub -- see INTEGRATION.md.
 *
 * Conventions
 *   - plain C types, caller-owned host buffers, 64-bit sizes, no torch types;
 *   - every function returns 0 on success and a negative PMF_E* code on
 *     failure; pmf_last_error() returns a thread-local message.  Nothing
 *     aborts or throws across the ABI;
 *   - a context is bound to one GPU and one HIP stream and is not thread-safe;
 *     distinct contexts are independent;
 *   - host <-> device exchange of model state is always float64 (the
 *     reference's dtype); device storage is the
 *     context's dtype (PMF_F32 for throughput, PMF_F64 for parity runs).
 */
#ifndef PMF_HIP_H
#define PMF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PMF_ABI_VERSION 3

/* error codes */
#define PMF_OK 0
#define PMF_EINVAL (-1)   /* bad argument / state not set */
#define PMF_EHIP (-2)     /* a HIP runtime call failed (message has the hipError string) */
#define PMF_ENOMEM (-3)
#define PMF_ERANGE (-4)   /* id outside [0, n_rows) or unsupported n_factors */
#define PMF_ECOMM (-5)    /* a collective / communicator call failed (RCCL error string in the message) */

/* device storage / arithmetic type of a context */
#define PMF_F32 0
#define PMF_F64 1

/* which block of the bipartite model a call addresses */
#define PMF_SIDE_USER 0
#define PMF_SIDE_ITEM 1

/* Model-state arrays (second argument of pmf_set_array / pmf_get_array).
 * Reference attribute each one mirrors:
 *   FACTOR   E_theta / E_beta        (poisson_mf_cavi.py:41-42, hpf_cavi.py:54-55)
 *            m_theta / m_beta        (gaussian_mf_cavi_bias.py:33,35)        [rows x K]
 *   SHAPE    a_theta / a_beta, gamma_a_theta / gamma_a_beta                  [rows x K]
 *   RATE     b_theta / b_beta, gamma_b_theta / gamma_b_beta                  [rows x K]
 *   PRIOR_RATE  E_xi / E_eta         (hpf_cavi.py:56-57)                     [rows]
 *   HYPER_RATE  gamma_b_xi / gamma_b_eta (hpf_cavi.py:46,50)                 [rows]
 *   COV      V_theta / V_beta        (gaussian_mf_cavi_bias.py:34,36)        [rows x K x K] on the
 *            host side; packed lower-triangular K(K+1)/2 per row on the device
 *   BIAS     m_user_bias / m_item_bias (gaussian_mf_cavi_bias.py:39-40)      [rows]
 *   SCALE / SCALE_SHAPE / SCALE_RATE   E_phi, a_phi, b_phi / E_psi, a_psi, b_psi of the extended
 *            Poisson model (poisson_mf_extended_cavi.py:34-45)                [rows]
 */
#define PMF_ARR_FACTOR 0
#define PMF_ARR_SHAPE 1
#define PMF_ARR_RATE 2
#define PMF_ARR_PRIOR_RATE 3
#define PMF_ARR_HYPER_RATE 4
#define PMF_ARR_COV 5
#define PMF_ARR_BIAS 6
#define PMF_ARR_SCALE 7
#define PMF_ARR_SCALE_SHAPE 8
#define PMF_ARR_SCALE_RATE 9
#define PMF_ARR_COUNT 10

/* kernel classes for pmf_prof_get (live hipEvent timing on the context's stream) */
#define PMF_KERNEL_GAMMA_SWEEP 0   /* Poisson/HPF half-sweep accumulate(+finalise) */
#define PMF_KERNEL_GAMMA_FINAL 1   /* split-row / distributed finalise */
#define PMF_KERNEL_GAUSS_ACCUM 2   /* Gaussian normal-equation accumulate */
#define PMF_KERNEL_GAUSS_SOLVE 3   /* K x K SPD inverse + mean */
#define PMF_KERNEL_GAUSS_BIAS 4    /* Gaussian bias half-sweep */
#define PMF_KERNEL_EVAL 5          /* fused predict + error reduction */
#define PMF_KERNEL_PREDICT 6
#define PMF_KERNEL_TOPK 7
#define PMF_KERNEL_GAUSS_COMBINE 8 /* split-row partial sums -> row sums */
#define PMF_KERNEL_GAUSS_SGD 9     /* MAP gradient half-sweep (no reference counterpart) */
#define PMF_KERNEL_COMM_ALLREDUCE 10 /* item-statistics all-reduce, timed on the collective stream */
#define PMF_KERNEL_COMM_WAIT 11    /* compute stream idle until a chunk's all-reduce has landed = exposed communication */
#define PMF_KERNEL_PREDICT_VAR 12   /* posterior predictive variance: per pair and the fused validation form */
#define PMF_KERNEL_COUNT 13

typedef struct pmf_ctx pmf_ctx;

/* ---- library ----------------------------------------------------------- */
int pmf_abi_version(void);
const char *pmf_last_error(void);
/* number of visible HIP devices (0 and PMF_EHIP when there is no usable GPU) */
int pmf_device_count(int *count);

/* ---- context ------------------------------------------------------------
 * One context = one model instance's device state on one GPU.
 * n_users / n_items follow `_infer_dimensions` (hpf_cavi.py:60-64): max id + 1
 * of the TRAINING ratings.  In a multi-GPU run n_users is the size of this
 * rank's user range (ids are local to it) and n_items is global. */
int pmf_ctx_create(int device, int64_t n_users, int64_t n_items, int n_factors, int dtype,
                   pmf_ctx **out);
int pmf_ctx_destroy(pmf_ctx *ctx);
/* run on an existing HIP stream (e.g. torch's current stream) instead of the
 * context's own; `hip_stream` is a hipStream_t.  NULL restores the own stream -- so the
 * null handle of the legacy default stream cannot be selected: order with torch / RCCL
 * through a non-default stream (pmf_hip/dist.py:StreamScope). */
int pmf_ctx_set_stream(pmf_ctx *ctx, void *hip_stream);
int pmf_ctx_sync(pmf_ctx *ctx);

/* Row chunks (no reference counterpart; multi-GPU pipelining).  `n_chunks` equal row ranges of
 * one side; the *_accumulate / *_finalize calls of that side then act on the chunk chosen with
 * pmf_ctx_select_chunk (-1 = all rows, the default) -- they read and write only rows
 * [row_begin, row_end) of the statistics buffer, at the same offsets as in an unchunked call,
 * so a caller can all-reduce the slice of chunk c while chunk c+1 is being accumulated.
 * The fused *_sweep calls always cover all rows.  Results do not depend on the chunking. */
int pmf_ctx_set_row_chunks(pmf_ctx *ctx, int side, int n_chunks);
int pmf_ctx_chunk_rows(pmf_ctx *ctx, int side, int chunk, int64_t *row_begin, int64_t *row_end);
int pmf_ctx_select_chunk(pmf_ctx *ctx, int side, int chunk);
/* bytes of device memory currently held by the context */
int pmf_ctx_device_bytes(pmf_ctx *ctx, int64_t *bytes);
/* Hot rows of `side` under the Gaussian gather cache policy (fp32, n_factors <= 64): the most-rated rows of the
 * side, most-rated first (ties: lower id first), as many as fit the PMF_GAUSS_HOT_MB budget (read when the context
 * is created; 0 turns the policy off) at cov_stride + kpad floats per row.  The opposite side's sweep gathers them
 * with the default cache policy and every other row non-temporally; results do not depend on it.  Writes the count
 * to *n_hot and the first min(count, capacity) ids to `rows` (may be NULL when capacity is 0).  Set by
 * pmf_ctx_set_ratings. */
int pmf_ctx_hot_rows(pmf_ctx *ctx, int side, int32_t *rows, int64_t capacity, int64_t *n_hot);
/* Length in ratings of the longest task of one of `side`'s work lists (a task is a contiguous run of one row's
 * ratings that one wavefront / lane group walks; rows longer than the list's task length are split evenly).  The
 * task length of the GAMMA, GAUSS and BIAS lists grows with the rating count (32 up to 2^21 ratings, doubling to
 * at most 512) or is fixed by PMF_TASK_CHUNK (a power of two in [32, 512], read when the context is created); the
 * SGD list's is always 256.  Results depend on it through the summation order of split rows only.  Set by
 * pmf_ctx_set_ratings. */
#define PMF_TASKS_GAMMA 0
#define PMF_TASKS_GAUSS 1
#define PMF_TASKS_BIAS 2
#define PMF_TASKS_SGD 3
int pmf_ctx_task_max_len(pmf_ctx *ctx, int side, int list, int *max_len);

/* Training ratings in their original order (COO).  Replaces
 * `_build_index_lists` (hpf_cavi.py:97-107, gaussian_mf_cavi_bias.py:69-86):
 * builds the by-user (CSR) and by-item (CSC) orderings with a stable counting
 * sort, so every row lists its ratings in ascending original position and
 * duplicate (u,i) pairs are kept.  Also builds the per-side work lists
 * (row chunks) the sweep kernels consume. */
int pmf_ctx_set_ratings(pmf_ctx *ctx, int64_t nnz, const int32_t *user_ids,
                        const int32_t *item_ids, const double *ratings);
/* The same with a confidence weight c_j per rating (Gaussian CAVI models): rating j has precision c_j / sigma2,
 *     x_j ~ N(b_r + b_o + theta_r . beta_o, sigma2 / c_j),   c_j > 0,
 * so every sum the Gaussian calls form over a row's ratings takes c_j inside: S_r = sum_j c_j (COV[o_j] + m_j m_j^T),
 * w_r = sum_j c_j m_j (x_j - b_r - b_o), C_r = sum_j c_j in the place of the row's rating count in the bias update, and
 * c_r = sum_j c_j (x_j - b_r - b_o)^2 in pmf_gauss_elbo_terms.  The weights go through the same stable permutation as
 * the ratings into a per-side [nnz] array of the context dtype, and C_r of both sides is formed once (in double, in
 * the row's rating order, rounded once to the context dtype).  `weights` = NULL is pmf_ctx_set_ratings, which is this
 * call with NULL: it clears the weights.  While the context holds weights, pmf_gauss_factor_sweep / _accumulate /
 * _finalize, pmf_gauss_bias_sweep / _accumulate / _finalize (second statistic: C_r) and pmf_gauss_elbo_terms follow
 * them, also under pmf_ctx_set_gauss_zeros' PMF_ZEROS_OBSERVED (a listed cell then has precision c_j / sigma2, an
 * unlisted one weight / sigma2: S'_r = sum_j (c_j - weight) A_j + weight G).  With all weights 1.0 the default mode
 * gives the bytes of the unweighted context.  pmf_predict*, pmf_eval_* and the top-k / rank calls do not read them.
 * PMF_EINVAL: a weight that is not finite or not > 0 (its position is named; checked on the host before anything is
 * touched: the context keeps its previous ratings); a context with a communicator.  While the context holds weights
 * pmf_comm_init / _attach, pmf_gauss_sgd_* and every pmf_gamma_* call that reads the ratings are PMF_EINVAL. */
int pmf_ctx_set_ratings_weighted(pmf_ctx *ctx, int64_t nnz, const int32_t *user_ids, const int32_t *item_ids,
                                 const double *ratings, const double *weights /* [nnz], may be NULL */);
/* *has = 1 while the context's ratings came with weights */
int pmf_ctx_has_rating_weights(pmf_ctx *ctx, int *has);
/* C_r of every row of `side` as the kernels read it (the row's weights summed in double, rounded once to the context
 * dtype); the rating counts when the context holds no weights.  After pmf_gauss_logit_refresh(side) they are the sums
 * that call re-formed, read back from the device.  PMF_EINVAL: ratings have not been set. */
int pmf_ctx_rating_weight_sums(pmf_ctx *ctx, int side, double *out /* rows */);
/* The ratings as `side` holds them (CSR when side = user, CSC when side = item), read back from the device after the
 * work queued on the context's stream: row_ptr [rows + 1], other_ids [nnz] (ids on the opposite side, every row in
 * ascending original position), ratings [nnz] and weights [nnz] as float64 of the stored context-dtype values.  Every
 * output may be NULL.  After pmf_gauss_logit_refresh(side) the ratings and weights are the refreshed ones.  PMF_EINVAL:
 * ratings have not been set; `weights` asked of a context that holds none. */
int pmf_ctx_side_ratings(pmf_ctx *ctx, int side, int64_t *row_ptr, int32_t *other_ids, double *ratings, double *weights);

/* Host float64 -> device (and back).  `host` holds rows x K (FACTOR, SHAPE,
 * RATE), rows (PRIOR_RATE, HYPER_RATE, BIAS) or rows x K x K (COV) doubles,
 * C-contiguous.  Setting an array allocates it. */
int pmf_set_array(pmf_ctx *ctx, int side, int array, const double *host);
int pmf_get_array(pmf_ctx *ctx, int side, int array, double *host);
/* Row subsets of the same arrays: `rows[n]` are row ids of `side` (any order, repeats allowed when
 * reading; when writing, a repeated row ends with one of its values); `host` holds n rows in the
 * layout above (n x K, n, or n x K x K doubles).  What the reference's row indexing does
 * (`V_beta[j_idx]`, `m_beta[j_idx]`, `V_theta[i] = ...`: gaussian_mf_cavi_bias.py:146-162) without
 * moving the whole stack: V_theta at 1M x 64 x 64 is 32.8 GB as host float64, 164 GB at the K = 128
 * shard of config C4.  A row id outside [0, rows) is PMF_ERANGE and nothing is copied. */
int pmf_get_array_rows(pmf_ctx *ctx, int side, int array, int64_t n, const int64_t *rows, double *host);
int pmf_set_array_rows(pmf_ctx *ctx, int side, int array, int64_t n, const int64_t *rows, const double *host);
/* COV shortcut for `_initialize_variational_params`
 * (gaussian_mf_cavi_bias.py:64-67): every row's covariance = scale * I. */
int pmf_set_cov_identity(pmf_ctx *ctx, int side, double scale);

/* ---- Poisson MF / HPF half-sweep ---------------------------------------
 * One block-Jacobi half-sweep over all rows of `side`
 * (poisson_mf_cavi.py:135-167 users, :173-197 items;
 *  hpf_cavi.py:126-153 users, :162-187 items):
 *     rate_j    = max(FACTOR_other[o_j] . FACTOR_side[r], 1e-10)
 *     SHAPE[r]  = shape_prior + sum_j x_j * FACTOR_other[o_j] * FACTOR_side[r] / rate_j
 *     RATE[r]   = rate_prior_r + sum_j FACTOR_other[o_j]
 *     FACTOR[r] = SHAPE[r] / RATE[r]
 * rate_prior_r is `rate_prior` when hierarchical == 0 (Poisson MF, b0) and
 * PRIOR_RATE[r] (E_xi / E_eta) when hierarchical != 0 (HPF).  In the
 * hierarchical case the epilogue also performs the xi / eta update of
 * hpf_cavi.py:155-159 / :189-193:
 *     HYPER_RATE[r] = hyper_rate_prior + sum_k FACTOR[r,k]
 *     PRIOR_RATE[r] = hyper_shape / HYPER_RATE[r]
 * Rows without ratings fall back to the priors (hpf_cavi.py:128-132). */
int pmf_gamma_sweep(pmf_ctx *ctx, int side, double shape_prior, double rate_prior,
                    int hierarchical, double hyper_shape, double hyper_rate_prior);

/* Extended Poisson MF half-sweep, x ~ Poisson(phi_u psi_i theta_u.beta_i)
 * (poisson_mf_extended_cavi.py:108-160 users, :163-215 items).  With s = SCALE of
 * the other side:
 *     SHAPE[r]  = a0 + sum_j x_j FACTOR_other[o_j] FACTOR_side[r] / (FACTOR_other[o_j].FACTOR_side[r])
 *     RATE[r]   = b0 + sum_j s[o_j] FACTOR_other[o_j];        FACTOR[r] = SHAPE[r] / RATE[r]
 *     SCALE_SHAPE[r] = a0 + sum_j x_j;
 *     SCALE_RATE[r]  = b0 + sum_j s[o_j] (FACTOR_other[o_j] . FACTOR[r])   -- with the NEW FACTOR[r]
 *     SCALE[r]       = SCALE_SHAPE[r] / SCALE_RATE[r]
 * The rate is not clamped (the reference divides by the raw dot product).  Rows
 * without ratings get the priors in SHAPE / RATE / SCALE_SHAPE / SCALE_RATE and keep
 * FACTOR and SCALE (the reference `continue`s before recomputing them). */
int pmf_gamma_ext_sweep(pmf_ctx *ctx, int side, double shape_prior, double rate_prior);

/* Fold-in: the variational parameters of NEW rows of `side` against the fitted opposite side, whose FACTOR stays
 * frozen.  No reference counterpart as an operation (the reference serves an unseen id by refitting); per row it
 * restates the reference's own row update -- poisson_mf_cavi.py:135-167 / hpf_cavi.py:126-159 (items: :173-197 /
 * :162-193) -- `n_iter` times with the other side fixed.  The batch is CSR as for pmf_gauss_fold_in: `row_ptr[n_rows + 1]`
 * (row_ptr[0] = 0, non-decreasing), `other_ids` / `ratings` [row_ptr[n_rows]] = ids on the opposite side and ratings.
 * The prior arguments mean what they mean in pmf_gamma_sweep; `rate_prior` is ignored when hierarchical != 0.  For a
 * row with ratings (o_j, x_j), j = 1 .. n (n may be 0), b_j = FACTOR_other[o_j]:
 *     rho^0   = init_prior_rate[r], else hyper_shape / hyper_rate_prior          (hierarchical)
 *     rho^t   = rate_prior for every t                                           (not hierarchical)
 *     theta^0 = init_factor[r], else shape_prior / rho^0 in every element
 *     B       = sum_j b_j                                                        (formed once per call)
 *     for t = 1 .. n_iter:
 *         rate_j = max(b_j . theta^(t-1), 1e-10)
 *         s^t = shape_prior + sum_j (x_j / rate_j) b_j * theta^(t-1),    r^t = rho^(t-1) + B,    theta^t = s^t / r^t
 *         hierarchical:  h^t = hyper_rate_prior + sum_k theta^t_k,   rho^t = hyper_shape / h^t
 *     out_factor[r] = theta^n_iter, out_shape[r] = s^n_iter, out_rate[r] = r^n_iter,
 *     out_prior_rate[r] = rho^n_iter, out_hyper_rate[r] = h^n_iter     (the last two: hierarchical only, else not written)
 * A row without ratings runs the same recursion with empty sums (the reference's empty-row rule).  With `init_factor`
 * and `init_prior_rate` given the call is a warm start: the known state of an existing row refreshed from new ratings.
 * One kernel launch covers all n_iter passes of a row block: a row's theta, B, rho and h stay in registers, B is summed
 * in the first pass only and nothing is written before the end.  A lane group owns a row; a row with more than
 * PMF_GAMMA_FOLD_LONG ratings (read when the context is created; default in DESIGN.md section 4.9) gets a whole block,
 * whose groups' partial sums are added in a fixed order: two calls give the same bits, whatever the row blocks are.
 * Reads the context's model state only: state, ratings, work lists and the stored validation set stay as they are;
 * FACTOR of `side` itself is not needed; never a collective, with or without a communicator.  The extended Poisson
 * model (SCALE arrays) is not covered.
 * PMF_EINVAL: null context (whatever n_rows is), bad side, n_rows < 0, a null array that is needed, row_ptr[0] != 0 or a
 * decreasing row_ptr, shape_prior <= 0, rate_prior <= 0 when not hierarchical, hyper_shape <= 0 or hyper_rate_prior <= 0
 * when hierarchical, n_iter < 1, FACTOR of the opposite side not set (named).  PMF_ERANGE: an other_ids entry outside
 * the opposite side (id and position named).  An argument error writes no output buffer; n_rows = 0 touches nothing.
 * Rows are processed in blocks of bounded staging (PMF_FOLD_IN_ROWS=n, read when the context is created, caps the rows
 * of a block of this call and of pmf_gauss_fold_in alike). */
int pmf_gamma_fold_in(pmf_ctx *ctx, int side, int64_t n_rows, const int64_t *row_ptr, const int32_t *other_ids,
                      const double *ratings, double shape_prior, double rate_prior, int hierarchical,
                      double hyper_shape, double hyper_rate_prior, int n_iter,
                      const double *init_factor /* n_rows x K, may be NULL */,
                      const double *init_prior_rate /* n_rows, may be NULL; hierarchical only */,
                      double *out_factor /* n_rows x K */, double *out_shape /* n_rows x K, may be NULL */,
                      double *out_rate /* n_rows x K, may be NULL */, double *out_prior_rate /* n_rows, may be NULL */,
                      double *out_hyper_rate /* n_rows, may be NULL */);

/* Evidence lower bound of the Poisson MF and HPF models: the per-row sums that do not depend on the hyperparameters.
 * No reference counterpart (the reference never evaluates its objective).  q is defined by SHAPE and RATE alone:
 * q(theta_rk) = Gamma(a_rk, b_rk) with a = SHAPE, b = RATE of `side`; FACTOR is not read -- E_rk = a/b and
 * Elog_rk = psi(a) - log b are formed from the same two arrays -- and neither is PRIOR_RATE.  With hierarchical != 0,
 * q(xi_r) = Gamma(kappa, h_r) with h_r = HYPER_RATE[r]; the shape kappa is the caller's (the host adds it).  The call
 * returns for `side`, per row r and summed over all its rows (with or without ratings), over the ratings (o_j, x_j) of
 * the row:
 *     PMF_GAMMA_ELBO_SUM_FACTOR         sum_k a/b
 *     PMF_GAMMA_ELBO_SUM_ELOG           sum_k psi(a) - log b
 *     PMF_GAMMA_ELBO_ENTROPY            sum_k a - log b + lgamma(a) + (1 - a) psi(a)
 *     PMF_GAMMA_ELBO_LOG_HYPER          log h_r
 *     PMF_GAMMA_ELBO_INV_HYPER          1 / h_r
 *     PMF_GAMMA_ELBO_FACTOR_OVER_HYPER  (sum_k a/b) / h_r                           (these three: 0 unless hierarchical)
 *     PMF_GAMMA_ELBO_DATA               sum_j [ x_j lse_j - sum_k E_rk E_{o_j k} ],  lse_j = log sum_k exp(Elog_rk + Elog_{o_j k})
 *     PMF_GAMMA_ELBO_LOGFACT            sum_j lgamma(x_j + 1)                       (these two: with_data != 0 only, else 0)
 * lse_j is the data term at its optimal auxiliary multinomial, phi_jk proportional to exp(Elog_rk + Elog_{o_j k}).  The
 * caller assembles, with DATA - LOGFACT taken from ONE side (either gives the same sum), R rows of a side and K factors:
 *   Poisson MF, priors (a0, b0), per side:
 *     R K (a0 log b0 - lgamma a0) + (a0 - 1) SUM_ELOG - b0 SUM_FACTOR + ENTROPY
 *   HPF, per side, (s, s', r') = (a, a', b') for users and (c, c', d') for items, kappa = s' + K s:
 *     K s (R psi(kappa) - LOG_HYPER) - R K lgamma(s) + (s - 1) SUM_ELOG - kappa FACTOR_OVER_HYPER + ENTROPY
 *       + R (s' log r' - lgamma s') + (s' - 1)(R psi(kappa) - LOG_HYPER) - r' kappa INV_HYPER
 *       + R (kappa + lgamma kappa + (1 - kappa) psi(kappa)) - LOG_HYPER
 *   L = DATA - LOGFACT + the two sides' sums      (src/models/_gamma_elbo.py:elbo_from_gamma_terms is this formula).
 * The reference's row update weights the factors with the arithmetic means E E / (E . E), not with exp(Elog); it is not
 * exact coordinate ascent on L, so L need not rise from one of its iterations to the next.  pmf_gamma_exact_sweep is the
 * update that is.
 * `totals[t]` is the sum of the per-row values in row order, in double: two calls give the same bits, whatever the task
 * length.  `per_row` (rows x PMF_GAMMA_ELBO_TERMS, row-major) may be NULL.  psi and lgamma of the row terms are
 * evaluated in double whatever the context's dtype (lgamma(a) + (1 - a) psi(a) cancels in fp32 once a shape reaches
 * the thousands); the per-rating arithmetic and the per-task and per-row sums of DATA are in the context's dtype,
 * LOGFACT is in double.  The data term runs over the side's GAMMA work list, the sweep's own cuts (read only); the
 * partial sums of a split row are added in slot order.  LOGFACT comes from a Stirling series that equals
 * lgamma(x + 1) for x >= 0; for a negative rating DATA and LOGFACT are undefined (finite-time, the values mean nothing; the
 * model classes refuse one).  Reads the context only: model state, ratings, work lists and the stored
 * validation set stay as they are; never a collective, with or without a communicator.  The row terms, the gathered
 * tables ([rows][2][kpad] of each side in the context's dtype) and the partial sums live in the context's scratch
 * buffer: pmf_ctx_device_bytes may grow on the first call and does not grow on the ones after it.  Launches are
 * timed as PMF_KERNEL_GAMMA_FINAL (row pass) and PMF_KERNEL_GAMMA_SWEEP (data pass).
 * Cost, measured at K = 64 fp32, 1M users, 50M ratings: the two kernels of a user call with data
 * take 3.00 times a user half-sweep of pmf_gamma_sweep, the data pass alone 2.06 times it and 2.34 times
 * pmf_prof_gather_ceiling; the whole call takes 5.1 times a full iteration by wall clock (1.27 times in kernel time: the
 * rest is the download of the per-row terms and the host's sum).  The extended Poisson model (SCALE arrays) is not covered.
 * PMF_EINVAL, with the missing thing named: null context, bad side, null totals, SHAPE or RATE of `side` not set;
 * with_data: SHAPE or RATE of the other side not set, no ratings; hierarchical: HYPER_RATE of `side` not set.  An
 * argument error writes nothing. */
#define PMF_GAMMA_ELBO_SUM_FACTOR 0
#define PMF_GAMMA_ELBO_SUM_ELOG 1
#define PMF_GAMMA_ELBO_ENTROPY 2
#define PMF_GAMMA_ELBO_LOG_HYPER 3
#define PMF_GAMMA_ELBO_INV_HYPER 4
#define PMF_GAMMA_ELBO_FACTOR_OVER_HYPER 5
#define PMF_GAMMA_ELBO_DATA 6
#define PMF_GAMMA_ELBO_LOGFACT 7
#define PMF_GAMMA_ELBO_TERMS 8
int pmf_gamma_elbo_terms(pmf_ctx *ctx, int side, int with_data, int hierarchical,
                         double *totals /* [PMF_GAMMA_ELBO_TERMS] */,
                         double *per_row /* rows x PMF_GAMMA_ELBO_TERMS, may be NULL */);

/* Multi-GPU form of the same half-sweep (ratings sharded by user range,
 * SURVEY.md section 8e).  `accumulate` writes this rank's raw sums
 * [rows x 2 x Kpad] (shape sums, then rate sums; Kpad from pmf_ctx_kpad) into
 * `stats_dev`, a DEVICE buffer the caller owns and all-reduces (RCCL) between
 * the two calls; `finalize` applies the priors and the epilogue above (it reads the
 * statistics only: FACTOR of `side` is allocated if it is not there). */
int pmf_ctx_kpad(pmf_ctx *ctx, int *kpad);
int pmf_gamma_accumulate(pmf_ctx *ctx, int side, void *stats_dev);
int pmf_gamma_finalize(pmf_ctx *ctx, int side, const void *stats_dev, double shape_prior,
                       double rate_prior, int hierarchical, double hyper_shape,
                       double hyper_rate_prior);

/* Exact coordinate-ascent half-sweep of the Poisson MF and HPF models: the statistics of pmf_gamma_sweep with the
 * weights of coordinate ascent on the bound of pmf_gamma_elbo_terms.  No reference counterpart (the reference's row
 * update weights a rating's factors with E E / (E . E), see above).  q is defined by SHAPE and RATE alone, as for
 * pmf_gamma_elbo_terms: Elog = psi(SHAPE) - log RATE and E = SHAPE / RATE, for both sides; FACTOR is not read.  For
 * row r of `side` with ratings (o_j, x_j):
 *     s_jk   = Elog_side[r,k] + Elog_other[o_j,k]
 *     phi_jk = exp(s_jk - lse_j),   lse_j = log sum_k exp(s_jk)                       (max-subtracted)
 *     SHAPE[r,k] = shape_prior + sum_j x_j phi_jk
 *     RATE[r,k]  = rate_prior_r + sum_j E_other[o_j,k]
 *     FACTOR[r]  = SHAPE[r] / RATE[r]
 * rate_prior_r, the hierarchical epilogue (HYPER_RATE, PRIOR_RATE) and the empty-row rule are those of pmf_gamma_sweep:
 * the same finalize code runs.  Under this update the bound cannot fall from one half-sweep to the next, except by
 * rounding.  A rating of 0 adds nothing to the shape sums and its E row to the rate sums; for a negative rating the
 * result is undefined (the model classes refuse one).  The extended Poisson model is not covered.
 * Both sides' (E log, E) tables ([rows][2][Kpad] in the context's dtype, psi evaluated in double) are rebuilt by every
 * call from SHAPE and RATE as they are at that time, into context-owned storage of their own -- an interleaved
 * pmf_gamma_elbo_terms call does not touch it: pmf_ctx_device_bytes may grow on the first call and does not grow after
 * it.  Per rating the weights come from a log-sum-exp (one max, one exp per element, one sum), never from a product of
 * exp(Elog) tables, which underflows in fp32 for small shapes.  No atomics; the rows cut into several tasks go through
 * pmf_gamma_sweep's split-row kernel: two calls from the same state give the same bits.  Launches are timed as
 * PMF_KERNEL_GAMMA_SWEEP (data pass) and PMF_KERNEL_GAMMA_FINAL (row pass, split rows, finalize).
 * With a communicator the ITEM call runs accumulate -> exchange -> finalize exactly as pmf_gamma_sweep does (tables
 * built once, before the first chunk); USER calls stay local.
 * pmf_gamma_exact_accumulate writes the raw sums [rows x 2 x Kpad] (shape sums, then rate sums: the layout of
 * pmf_gamma_accumulate) of the selected chunk into `stats_dev`; pmf_gamma_finalize finalises either kind.
 * PMF_EINVAL, with the missing thing named: null context, bad side, SHAPE or RATE of either side not set, no ratings,
 * hierarchical and PRIOR_RATE of `side` not set, null stats buffer.  An argument error writes nothing.
 * Cost, measured at K = 64 fp32, 1M users, 50M ratings: DESIGN.md section 4.12. */
int pmf_gamma_exact_sweep(pmf_ctx *ctx, int side, double shape_prior, double rate_prior,
                          int hierarchical, double hyper_shape, double hyper_rate_prior);
int pmf_gamma_exact_accumulate(pmf_ctx *ctx, int side, void *stats_dev);

/* Implicit feedback: unlisted cells counted as zeros.  No reference counterpart (the reference
 * treats the rating list as the whole data set; that stays the default).  pmf_ctx_set_gamma_zeros selects, for the
 * Poisson MF / HPF calls of this context, what a (user, item) cell without a rating is:
 *     PMF_ZEROS_MISSING   (default) not an observation: every sum runs over the listed ratings, bit for bit as before
 *     PMF_ZEROS_OBSERVED  a count of 0, the model of the HPF paper: every one of the U x I cells is an observation
 * A zero adds nothing to a shape sum (its weight is x / rate = 0, or x phi = 0) and its row of the other side's expected
 * factors to the rate sum -- for every row alike.  With C_k = sum over ALL rows o of the other side of E_other[o,k]:
 *   pmf_gamma_sweep        SHAPE as before;  RATE[r,k] = rate_prior_r + C_k, C from FACTOR of the other side as it is when
 *                          the call starts;  FACTOR, the hierarchical epilogue and the split-row path as before
 *   pmf_gamma_exact_sweep  the same, C from the E half of the other side's freshly built table
 *   pmf_gamma_fold_in      B = C of the opposite side's FACTOR for every row (a new row's unlisted cells are zeros), formed
 *                          once per call; the recursion, the long-row kernel and the warm start as before
 *   pmf_gamma_fold_in_exact  the same, C from the E half of the opposite side's freshly built table
 *   pmf_gamma_elbo_terms   PMF_GAMMA_ELBO_DATA of row r = sum_j x_j lse_j - sum_k E_rk C_k, C from the other side's E table:
 *                          sum over all cells of E_u . E_i = (sum_u E_u) . (sum_i E_i).  LOGFACT as before (lgamma(0 + 1) = 0).
 *                          DATA - LOGFACT from either side still gives the same total.
 * A row without ratings is no special case: SHAPE = shape_prior, RATE = rate_prior_r + C, DATA = -E_r . C, which is what
 * listing its zeros would give.  The result equals what PMF_ZEROS_MISSING computes on the same matrix with every missing
 * cell listed as an explicit rating of 0, up to rounding (C is summed in double, the listed rate sums in the context's
 * dtype), at the cost of two small launches per call instead of U x I ratings.  C is rounded once to the context's dtype
 * before it is added to the prior rate; the E . C products of the bound are formed in double.
 * Duplicate (u, i) pairs (pmf_ctx_set_ratings keeps them): the shape sums add their counts, the cell enters the rate
 * sums once, LOGFACT treats them as separate ratings -- a cell with one count is the caller's to ensure (the model
 * classes refuse duplicates).
 * A property of the context, like the row chunks: no state array changes, and a mode may be set before or after the
 * ratings.  pmf_gamma_predictive, pmf_predict, the top-k / ranking calls and the Gaussian calls do not read it.
 * Not covered, PMF_EINVAL naming the mode: pmf_gamma_accumulate, pmf_gamma_exact_accumulate, pmf_gamma_finalize (the
 * caller-driven multi-GPU form) and pmf_gamma_ext_sweep (the extended model) while the mode is PMF_ZEROS_OBSERVED; and
 * several ranks -- the user-side column sums would have to be added over the ranks: PMF_ZEROS_OBSERVED on a context
 * with a communicator is PMF_EINVAL, as are pmf_comm_init / pmf_comm_attach (and the test build's
 * pmf_comm_init_hostshm) on a context in that mode.  PMF_EINVAL also for a null context, a mode that is neither value and
 * a null `mode` of the getter.  An error changes nothing. */
#define PMF_ZEROS_MISSING 0
#define PMF_ZEROS_OBSERVED 1
int pmf_ctx_set_gamma_zeros(pmf_ctx *ctx, int mode);
int pmf_ctx_get_gamma_zeros(pmf_ctx *ctx, int *mode);
/* C_k, k < K, of `side` in either mode: the sum over ALL its rows of FACTOR[r,k] (from_q == 0) or of E[r,k] =
 * SHAPE[r,k] / RATE[r,k] (from_q != 0), formed as pmf_gamma_elbo_terms and pmf_gamma_exact_sweep form the E half of their
 * (E log, E) table: the quotient in double, rounded once to the context's dtype.  The sum itself is in DOUBLE whatever
 * the dtype.  A fixed number of blocks each add a contiguous row range in a fixed order (16-byte loads per lane, lane
 * groups over the rows of the range, group sums added in group order); a second launch adds the block sums in a fixed
 * order as well (contiguous runs of blocks in block order, the runs' sums in run order).  No atomics and no work list: two calls give the same bits, whatever the task length.  Reads the model state
 * only (from_q: the table is rebuilt into the context-owned storage of pmf_gamma_exact_sweep); the block sums live in the
 * context's scratch buffer: pmf_ctx_device_bytes may grow on the first call and does not grow after it.  Timed as
 * PMF_KERNEL_GAMMA_FINAL.  This is the building block of PMF_ZEROS_OBSERVED, visible for tests and callers.
 * PMF_EINVAL, with the missing thing named: null context, bad side, null out, FACTOR (from_q == 0) or SHAPE / RATE
 * (from_q != 0) of `side` not set.  Cost: DESIGN.md section 4.16. */
int pmf_gamma_column_sums(pmf_ctx *ctx, int side, int from_q, double *out /* [K] */);

/* Exact fold-in: pmf_gamma_fold_in with the update of pmf_gamma_exact_sweep -- coordinate ascent on the bound of
 * pmf_gamma_elbo_terms for NEW rows of `side`, the opposite side frozen as q = Gamma(SHAPE_o, RATE_o).  No reference
 * counterpart.  A model fitted with pmf_gamma_exact_sweep serves new and refreshed rows from the objective it was
 * fitted under: a folded row's bound cannot fall from one pass to the next, except by rounding, and a warm-started
 * refresh of a fitted row starts at the fit's own fixed point.  The batch, the prior arguments and the outputs are
 * pmf_gamma_fold_in's.  With L_o = psi(SHAPE_o) - log RATE_o and E_o = SHAPE_o / RATE_o of the opposite side (its
 * (E log, E) table, as pmf_gamma_exact_sweep builds it: psi in double, rounded once to the context's dtype; FACTOR is
 * not read), for a row with ratings (o_j, x_j), j = 1 .. n (n may be 0):
 *     rho^0 = init_prior_rate[r], else hyper_shape / hyper_rate_prior          (hierarchical)
 *     rho^t = rate_prior for every t                                           (not hierarchical)
 *     s^0   = init_shape[r], else shape_prior in every element
 *     r^0   = init_rate[r], else rho^0 in every element
 *     B     = sum_j E_{o_j}                                                    (formed once per call)
 *     for t = 1 .. n_iter:
 *         l_k    = psi(s_k^(t-1)) - log r_k^(t-1)
 *         phi_jk = exp(l_k + L_{o_j k} - lse_j),   lse_j = log sum_k exp(l_k + L_{o_j k})       (max-subtracted)
 *         s_k^t  = shape_prior + sum_j x_j phi_jk,    r_k^t = rho^(t-1) + B_k,    theta^t = s^t / r^t
 *         hierarchical:  h^t = hyper_rate_prior + sum_k theta_k^t,   rho^t = hyper_shape / h^t
 *     out_factor[r] = theta^n_iter, out_shape[r] = s^n_iter, out_rate[r] = r^n_iter,
 *     out_prior_rate[r] = rho^n_iter, out_hyper_rate[r] = h^n_iter     (the last two: hierarchical only, else not written)
 * Under PMF_ZEROS_OBSERVED B of every row is C of the opposite side as pmf_gamma_column_sums(other, from_q = 1) defines
 * it (a zero adds nothing to a shape sum).  A row without ratings runs the same statements on empty sums.  `init_shape`
 * and `init_rate` are given together or not at all; with them and `init_prior_rate` the call is a warm start.  One pass
 * from a context's own SHAPE / RATE / PRIOR_RATE on its own ratings is pmf_gamma_exact_sweep(side).
 * One kernel launch covers all n_iter passes of a row block: s, r, B, rho and h stay in registers from the first pass to
 * the last; between passes psi and log of the row's own s and r are evaluated in double and l is rounded once to the
 * context's dtype; B is summed in the first pass only and nothing is written before the end.  The weights come from a
 * log-sum-exp, never from a product of exp(E log) tables.  A lane group owns a row; a row with more than
 * PMF_GAMMA_FOLD_LONG ratings gets a whole block whose groups' partial sums are added in group order.  No atomics: two
 * calls give the same bits, whatever the row blocks are (PMF_FOLD_IN_ROWS).  Launches are timed as for
 * pmf_gamma_fold_in, the table and the column sums as PMF_KERNEL_GAMMA_FINAL.
 * Reads the context's model state only (the table is rebuilt, once per call, into the context-owned storage of
 * pmf_gamma_exact_sweep: pmf_ctx_device_bytes may grow on the first call and does not grow after it); never a
 * collective, with or without a communicator.  Not covered: the extended Poisson model -- a context with SCALE arrays is
 * PMF_EINVAL.
 * PMF_EINVAL and PMF_ERANGE exactly as for pmf_gamma_fold_in, with SHAPE and RATE of the opposite side (named) in the
 * place of its FACTOR, which is not needed; one more PMF_EINVAL: one of `init_shape` / `init_rate` without the other.
 * An argument error writes no output buffer; n_rows = 0 touches nothing.  Cost: DESIGN.md section 4.20. */
int pmf_gamma_fold_in_exact(pmf_ctx *ctx, int side, int64_t n_rows, const int64_t *row_ptr, const int32_t *other_ids,
                            const double *ratings, double shape_prior, double rate_prior, int hierarchical,
                            double hyper_shape, double hyper_rate_prior, int n_iter,
                            const double *init_shape /* n_rows x K, may be NULL */,
                            const double *init_rate /* n_rows x K, with init_shape or not at all */,
                            const double *init_prior_rate /* n_rows, may be NULL; hierarchical only */,
                            double *out_factor /* n_rows x K */, double *out_shape /* n_rows x K, may be NULL */,
                            double *out_rate /* n_rows x K, may be NULL */, double *out_prior_rate /* n_rows, may be NULL */,
                            double *out_hyper_rate /* n_rows, may be NULL */);

/* Posterior predictive of the Poisson MF and HPF models for n (user, item) pairs: mean and variance of the rate under
 * q and, with ratings, three log densities of the count.  No reference counterpart beyond PLUGIN (the reference's
 * PoissonLogPredictiveLikelihood, metrics.py:53-66, on the host).  q is defined by SHAPE and RATE alone, as for
 * pmf_gamma_elbo_terms: FACTOR, PRIOR_RATE and HYPER_RATE are not read, so one call serves both models.  For pair
 * (u, i) write a, b = SHAPE, RATE of user u and c, d = SHAPE, RATE of item i, k < K, x the pair's rating:
 *     E_k      = (a_k / b_k)(c_k / d_k)
 *     out_mean = mu = sum_k E_k                                       = E_q[theta_u . beta_i]
 *     out_var  = v  = sum_k E_k^2 (1/a_k + 1/c_k + 1/(a_k c_k))       = Var_q[theta_u . beta_i]
 *                                                  (E[theta^2] = (a/b)^2 (1 + 1/a); the factors are independent under q)
 *     PLUGIN   x log lambda - lambda - lgamma(x + 1),   lambda = max(mu, 1e-10)
 *                                                  (PoissonLogPredictiveLikelihood at E theta, E beta, clamp included)
 *     BOUND    x lse_k(psi(a_k) - log b_k + psi(c_k) - log d_k) - mu - lgamma(x + 1)
 *                                                  (the data term of pmf_gamma_elbo_terms on a held-out pair; <= PLUGIN
 *                                                   for x >= 0 by Jensen's inequality)
 *     NEGBIN   log NB(x; r, mu),  r = mu^2 / v:
 *              lgamma(x + r) - lgamma(r) - lgamma(x + 1) + r log(r / (r + mu)) + x log(mu / (r + mu))
 *                                                  (the rate moment-matched to a Gamma of mean mu and variance v; the
 *                                                   count's predictive variance is mu + v)
 * out_logp is n x PMF_GAMMA_PRED_KINDS, row-major.  totals[0] = sum of out_var, totals[1 + kind] = sum of that column.
 * NEGBIN is evaluated as  x log mu - lgamma(x + 1) - (r + x) log1p(mu / r) + D,  D = lgamma(x + r) - lgamma(r) - x log r:
 * the literal form loses every digit once r passes about 1e8 (terms of size r log r leave one of size x), and shapes in
 * the thousands make such r ordinary.  For r >= 10, D = (x + r - 1/2) log1p(x / r) - x + S(x + r) - S(r) with S the tail
 * of Stirling's series; below that both lgammas are shifted up.  It tends to the unclamped Poisson term
 * x log mu - mu - lgamma(x + 1) as v -> 0, and IS that term when v == 0 or r is not finite (x log mu = 0 at x = 0).
 * Precision: mu and v are summed in the context's dtype by a lane group per pair (the 16-byte row gathers of
 * pmf_predict); everything after them -- logs, lgamma terms -- is formed in double from the (mu, v) the call returns, so
 * out_mean and out_var are the very bits out_logp was formed from.  BOUND's lse is a max-subtracted log-sum-exp in the
 * context's dtype over (E log, E) tables whose psi is evaluated in double; it is never a product of exp tables.
 * With with_bound != 0 both sides' tables ([rows][2][Kpad], context dtype) are rebuilt by every call from SHAPE and RATE
 * as they are then, in the storage pmf_gamma_exact_sweep rebuilds its own tables in: every call of either kind writes
 * them before it reads them, pmf_gamma_elbo_terms never touches them, so interleaved calls do not disturb each other;
 * pmf_ctx_device_bytes may grow on the first call and does not grow after it.  With with_bound == 0 no table is built
 * and no psi is evaluated; the BOUND column and total are then quiet NaN.
 * Ratings need not be integers; for a negative rating the three densities are undefined (finite-time, the values mean
 * nothing; the model classes refuse one).  With ratings == NULL only out_mean / out_var / totals[0] are produced:
 * out_logp must be NULL, totals[1..3] are NaN and with_bound is ignored.
 * totals are per-block partial sums in double, added in block order, staging round after staging round: no atomics, two
 * calls give the same bits.  Pairs are staged in rounds of bounded scratch (2^20 pairs; PMF_GAMMA_PRED_PAIRS=n, read
 * when the context is created, caps them), so n is unbounded.  The pair pass is timed as PMF_KERNEL_EVAL when ratings
 * are given and PMF_KERNEL_PREDICT otherwise, the table pass as PMF_KERNEL_GAMMA_FINAL.  Reads the context only: model
 * state, ratings, work lists and the stored validation set stay as they are; never a collective, with or without a
 * communicator.  The extended Poisson model (SCALE arrays) is not covered.
 * PMF_EINVAL, naming what is missing: null context (whatever n is), n < 0, a null id array, all four outputs null,
 * out_logp without ratings, SHAPE or RATE of either side not set.  PMF_ERANGE: an id outside the trained dimensions (id
 * and position named; unlike pmf_predict, which scores such a pair as 0).  An argument error writes nothing; n = 0
 * touches nothing and returns 0.
 * Cost: DESIGN.md section 4.13. */
#define PMF_GAMMA_PRED_PLUGIN 0
#define PMF_GAMMA_PRED_BOUND  1
#define PMF_GAMMA_PRED_NEGBIN 2
#define PMF_GAMMA_PRED_KINDS  3
/* totals: [0] = sum of out_var, [1 + kind] = sum of out_logp[:, kind] */
#define PMF_GAMMA_PRED_TOTALS 4
int pmf_gamma_predictive(pmf_ctx *ctx, int64_t n, const int32_t *user_ids, const int32_t *item_ids,
                         const double *ratings /* n, may be NULL */, int with_bound,
                         double *out_mean /* n, may be NULL */, double *out_var /* n, may be NULL */,
                         double *out_logp /* n x PMF_GAMMA_PRED_KINDS, may be NULL */,
                         double *totals /* [PMF_GAMMA_PRED_TOTALS], may be NULL */);

/* ---- Gaussian MF half-sweeps -------------------------------------------
 * Factor half-sweep (gaussian_mf_cavi_bias.py:132-165 users, :170-201 items;
 * bias-free twin gaussian_mf_cavi.py:121-147 / :152-178 when no BIAS array is
 * set): for every row with at least one rating
 *     S      = sum_j ( COV_other[o_j] + FACTOR_other[o_j] FACTOR_other[o_j]^T )
 *     COV[r] = inv( I/eta2 + S/sigma2 )
 *     FACTOR[r] = (1/sigma2) COV[r] . sum_j FACTOR_other[o_j] (x_j - BIAS_side[r] - BIAS_other[o_j])
 * Rows without ratings keep their mean and covariance.  n_factors <= 256 (pmf_ctx_create refuses more; the reference
 * has no limit, its grids stop at 70); the MFMA kernels cover K <= 128 in fp32, K > 128 and fp64 run generic ones. */
int pmf_gauss_factor_sweep(pmf_ctx *ctx, int side, double sigma2, double eta2);
/* Bias half-sweep (gaussian_mf_cavi_bias.py:206-232 users, :237-263 items):
 *     BIAS[r] = var/sigma2 * sum_j (x_j - BIAS_other[o_j] - FACTOR_other[o_j].FACTOR_side[r]),
 *     var = 1 / (1/eta_bias2 + n_r/sigma2);   rows without ratings keep their value. */
int pmf_gauss_bias_sweep(pmf_ctx *ctx, int side, double sigma2, double eta_bias2);

/* Fold-in: the posterior of NEW rows of `side` against the fitted opposite side, whose FACTOR, COV and (bias model)
 * BIAS stay frozen.  No reference counterpart as an operation (the reference serves an unseen id by refitting); per
 * row it restates the reference's own row updates -- the factor update of gaussian_mf_cavi_bias.py:132-165 followed
 * by the bias update of :206-232 (items: :170-201, :237-263), `n_iter` times from b = 0.  The batch is CSR:
 * `row_ptr[n_rows + 1]` (row_ptr[0] = 0, non-decreasing), `other_ids` / `ratings` [row_ptr[n_rows]] = ids on the
 * opposite side and ratings in pmf_ctx_set_ratings' convention.  For a row with n > 0 ratings (o_j, x_j), m_j =
 * FACTOR_other[o_j]:
 *     S = sum_j ( COV_other[o_j] + m_j m_j^T ),      V = inv( I/eta2 + S/sigma2 ),      b^0 = 0
 *     m^t = V . sum_j m_j (x_j - b^(t-1) - BIAS_other[o_j]) / sigma2
 *     b^t = kappa . sum_j (x_j - BIAS_other[o_j] - m_j . m^t),     kappa = 1 / (sigma2 (1/eta_bias2 + n/sigma2))
 * out_factor[r] = m^n_iter, out_cov[r] = V (full K x K), out_bias[r] = b^n_iter.  V does not depend on b and m is
 * affine in it, so the covariance rows are gathered once per call whatever n_iter is.  Unless both sides have a
 * BIAS array, b = 0 throughout, n_iter has no effect and out_bias is zeros.  A row without ratings gets the prior:
 * m = 0, V = eta2 I, b = 0 (under pmf_ctx_set_gauss_zeros' PMF_ZEROS_OBSERVED, below, every row is blended with the
 * opposite side's Gram matrix and solved instead).  out_cov / out_bias may be NULL (nothing K x K is then expanded or copied).
 * Reads the context's model state only: state, ratings, work lists and the stored validation set stay as they
 * are; FACTOR / COV of `side` itself are not needed; never a collective, with or without a communicator.
 * PMF_EINVAL: null context (whatever n_rows is), bad side, n_rows < 0, a null array that is needed, row_ptr[0] != 0
 * or a decreasing row_ptr, a variance <= 0, n_iter < 1, FACTOR or COV of the opposite side not set (named).
 * PMF_ERANGE: an other_ids entry outside the opposite side.  An argument error writes no output
 * buffer; n_rows = 0 touches nothing.  Rows are processed in blocks of bounded scratch (PMF_FOLD_IN_ROWS=n, read
 * when the context is created, caps the rows of a block -- of this call and of pmf_gamma_fold_in alike). */
int pmf_gauss_fold_in(pmf_ctx *ctx, int side, int64_t n_rows, const int64_t *row_ptr, const int32_t *other_ids,
                      const double *ratings, double sigma2, double eta2, double eta_bias2, int n_iter,
                      double *out_factor /* n_rows x K */, double *out_cov /* n_rows x K x K, may be NULL */,
                      double *out_bias /* n_rows, may be NULL */);
/* The same with a weight per rating of the batch (pmf_ctx_set_ratings_weighted's model): S, the right-hand side, g =
 * sum_j c_j m_j, c0 = sum_j c_j (x_j - BIAS_other[o_j]) and kappa = 1 / (sigma2 (1/eta_bias2 + C/sigma2)), C = sum_j c_j.
 * `weights` = NULL is pmf_gauss_fold_in, which is this call with NULL.  Independent of whether the context's own
 * ratings have weights.  PMF_EINVAL also for a weight that is not finite or not > 0 (its position is named). */
int pmf_gauss_fold_in_weighted(pmf_ctx *ctx, int side, int64_t n_rows, const int64_t *row_ptr, const int32_t *other_ids,
                               const double *ratings, const double *weights /* [row_ptr[n_rows]], may be NULL */,
                               double sigma2, double eta2, double eta_bias2, int n_iter, double *out_factor, double *out_cov,
                               double *out_bias);

/* Evidence lower bound of the Gaussian models: the per-row sums that do not depend on the hyperparameters.  No
 * reference counterpart (the reference never evaluates its objective).  q is what the reference's updates imply:
 * q(theta_u) = N(m_u, V_u), q(beta_i) = N(m_i, V_i) and, in the bias model, q(b_r) = N(BIAS[r], v_r) with
 * v_r = 1 / (1/eta_bias2 + n_r/sigma2) -- the `var` of gaussian_mf_cavi_bias.py:206-263, which the reference computes
 * and drops; a row with n_r = 0 ratings has v_r = eta_bias2.  With N ratings, R rows of a side, K factors and, over the
 * ratings (o_j, x_j) of row r,
 *     S_r = sum_j ( COV_other[o_j] + m_j m_j^T ),   w_r = sum_j m_j (x_j - BIAS[r] - BIAS_other[o_j]),
 *     c_r = sum_j (x_j - BIAS[r] - BIAS_other[o_j])^2          (m_j = FACTOR_other[o_j]; biases 0 without BIAS arrays)
 * the call returns for `side`, per row and summed over all its rows (with or without ratings),
 *     PMF_ELBO_SQNORM   |m_r|^2 + tr V_r
 *     PMF_ELBO_LOGDET   log det V_r
 *     PMF_ELBO_BIAS_SQ  BIAS[r]^2
 *     PMF_ELBO_ESS      c_r - 2 m_r . w_r + < V_r + m_r m_r^T, S_r >   = the expected squared residual of the row's ratings
 *                       under q, the bias variances aside (with_data != 0 only)
 * and the caller assembles, with ESS taken from ONE side (either gives the same sum) and eta2 = eta_theta2 for users,
 * eta_beta2 for items:
 *     ESS' = ESS + sum_u n_u v_u + sum_i n_i v_i                                                   (bias model only)
 *     L = -N/2 log(2 pi sigma2) - ESS' / (2 sigma2)
 *         + sum_side [ -R K/2 log(2 pi eta2) - SQNORM / (2 eta2) + R K/2 (1 + log 2 pi) + LOGDET / 2 ]
 *         + sum_side [ -R/2 log(2 pi eta_bias2) - (BIAS_SQ + sum_r v_r) / (2 eta_bias2) + 1/2 sum_r (1 + log(2 pi v_r)) ]
 *                                                                                                  (bias model only)
 * (src/models/_gaussian_host.py:elbo_from_terms is this formula).  `totals[t]` is the sum of the per-row values in row
 * order, in double: two calls give the same bits, whatever the row windows are.  `per_row` (rows x PMF_ELBO_TERMS,
 * row-major) may be NULL.  Sums inside a row are in the context's dtype.  With a data term the rows go in windows whose
 * statistics fit a fixed scratch budget (PMF_ELBO_ROWS=n, read when the context is created, caps the rows of a window).
 * The same variable also sizes the windows of pmf_gauss_factor_sweep under PMF_ZEROS_OBSERVED, which are these windows.
 * Per window the sweep's own accumulate kernels run on the sweep's own task cuts; measured at K = 64 fp32 on 1M users
 * and 50M ratings, one call with a data term takes 1.3 times an accumulate of `side`.  Reads the context only: model state, ratings, work lists and the stored validation set stay
 * as they are; never a collective, with or without a communicator.  Needs FACTOR and COV of `side`; with_data != 0
 * also FACTOR and COV of the other side and the ratings.  PMF_EINVAL: null context, bad side, null totals, a missing
 * array (named), with_data without ratings.  An argument error writes nothing.  A row
 * whose COV is not positive definite gives NaN in its LOGDET and in that total; the call still returns 0 and the
 * other rows are unaffected. */
#define PMF_ELBO_SQNORM 0    /* |m_r|^2 + tr V_r */
#define PMF_ELBO_LOGDET 1    /* log det V_r; NaN for a row whose COV is not positive definite */
#define PMF_ELBO_BIAS_SQ 2   /* BIAS[r]^2; 0 unless both sides have a BIAS array */
#define PMF_ELBO_ESS 3       /* c_r - 2 m_r.w_r + <V_r + m_r m_r', S_r>; 0 for a row without ratings (PMF_ZEROS_MISSING) or when with_data == 0 */
#define PMF_ELBO_TERMS 4
int pmf_gauss_elbo_terms(pmf_ctx *ctx, int side, int with_data, double *totals /* [PMF_ELBO_TERMS] */,
                         double *per_row /* rows x PMF_ELBO_TERMS, may be NULL */);

/* Logistic matrix factorisation on the Gaussian path.  No reference counterpart.  Ratings
 * x_j in {0, 1}, p(x_j = 1) = sigmoid(theta_u . beta_i), bias-free, q Gaussian per row as the Gaussian CAVI model holds
 * it.  Under the Jaakkola-Jordan bound with one parameter xi_j per rating the likelihood is Gaussian: rating j adds
 * c_j = 2 lambda(xi_j) times the outer product and x_j - 1/2 times the mean to its row's statistics, lambda(xi) =
 * tanh(xi / 2) / (4 xi), which is pmf_ctx_set_ratings_weighted's model with sigma2 = 1, weight c_j and stored rating
 * y_j = (x_j - 1/2) / c_j.  The label stays readable as x_j = [y_j > 0].
 * The call sets every xi_j of `side`'s stream to its optimum under the current q,
 *     xi_j^2 = E[(theta_r . beta_o)^2] = < COV[r] + m_r m_r^T, COV_other[o_j] + m_o m_o^T >     (summed in the context dtype),
 * and overwrites that stream's weights with c_j and its ratings with y_j (everything from xi on in double, rounded once),
 * re-forms the side's weight sums C_r (in double in the row's rating order, rounded once), and returns in *data_term
 * (may be NULL: nothing is read back and the call does not wait) the data term of the bound at these xi,
 *     D = sum_j [ log sigmoid(xi_j) - xi_j / 2 + (x_j - 1/2) m_r . m_o ],
 * summed in double in a fixed order: two calls on the same state give the same bits.  The other side's stream is not
 * touched: refresh a side before its pmf_gauss_factor_sweep(side, 1.0, eta2).  The index, work lists and hot-row flags
 * stay valid; the work is timed under PMF_KERNEL_PREDICT_VAR.
 * PMF_EINVAL (nothing is written): null context, bad side, no ratings, a context whose ratings were not loaded through
 * pmf_ctx_set_ratings_weighted, BIAS arrays, a missing FACTOR / COV of either side (named), a communicator,
 * PMF_ZEROS_OBSERVED. */
int pmf_gauss_logit_refresh(pmf_ctx *ctx, int side, double *data_term /* may be NULL */);

/* Posterior draws of factor rows.  No reference counterpart.  A draw of row r of `side` is
 *     x = m_r + C_r z,     C_r the lower Cholesky factor of V_r = COV[r] (C_r C_r' = V_r),  m_r = FACTOR[r],
 * with z K standard normals from a counter-based stream that is a pure function of (seed, side, row id, draw index, k):
 * it does not depend on the launch shape, the batch, the order of the rows or the context's dtype.
 *   generator  Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85), key = (seed low
 *              32 bits, seed high 32 bits), counter = (row id, draw index, block b = k / 4, side); the four output words
 *              give the normals of k = 4b .. 4b + 3.
 *   normals    Box-Muller in double, for both dtypes: u = (word + 0.5) 2^-32, (z0, z1) = sqrt(-2 ln u0) (cos 2 pi u1,
 *              sin 2 pi u1) from words 0 and 1, (z2, z3) the same from words 2 and 3 -- 2 pi the double 6.283185307179586,
 *              the product 2 pi u1 rounded before the cosine; the result is rounded once to the context's dtype.
 * C_r is never stored: the kernels eliminate the Jacobi-scaled matrix as pmf_gauss_elbo_terms does for LOGDET and add
 * column k of the factor times z_k at step k.  Biases are NOT sampled: a draw keeps BIAS at its mean (the bias variance
 * depends on sigma2 and eta_bias2, which the context does not hold).  A row whose COV is not positive definite (a pivot
 * <= 0, or a NaN scale) gives NaN in every element of that row's draws, the rule of PMF_ELBO_LOGDET; no other row is touched.
 *
 * pmf_gauss_sample_rows: draw d (0 <= d < n_draws) of request q is the draw of row row_ids[q] with draw index draw0 + d, at
 * out[(q * n_draws + d) * K ..].  Rows may repeat and come in any order.  `z` (NULL, or n_rows x n_draws x K) replaces the
 * stream: it is converted to the context's dtype as pmf_set_array_rows converts, and `seed` and `draw0` are then ignored.
 * Large requests go in rounds of bounded device scratch (PMF_STAGE_BYTES).  No atomics: two calls give the same bits.
 * Timed under PMF_KERNEL_GAUSS_SOLVE.  The call only reads the context.  PMF_EINVAL: null context, bad side, negative
 * n_rows, null row_ids or out, n_draws < 1, draw0 < 0, FACTOR or COV of the side missing (named; every count-model context).
 * PMF_ERANGE: an id outside [0, rows), naming the id and its position.  n_rows = 0 touches nothing; an argument error
 * writes nothing. */
int pmf_gauss_sample_rows(pmf_ctx *ctx, int side, int64_t n_rows, const int32_t *row_ids, int n_draws, int draw0,
                          uint64_t seed, const double *z /* NULL, or [n_rows x n_draws x K] */,
                          double *out /* [n_rows x n_draws x K] */);

/* Implicit feedback for the bias-free Gaussian model: unlisted cells as weighted zeros.  No
 * reference counterpart (the reference treats the rating list as the whole data set; that stays the default).
 * pmf_ctx_set_gauss_zeros selects, for pmf_gauss_factor_sweep, pmf_gauss_fold_in and pmf_gauss_elbo_terms of this
 * context, what a (user, item) cell without a rating is:
 *     PMF_ZEROS_MISSING   (default) not an observation: every sum runs over the listed ratings, bit for bit as before
 *     PMF_ZEROS_OBSERVED  an observation of 0 (in pmf_ctx_set_ratings' convention) with variance sigma2 / weight,
 *                         weight in (0, 1]: 1 = every missing cell listed as an explicit 0, 1 / (1 + alpha) = the
 *                         confidence ratio of implicit ALS (Hu, Koren & Volinsky 2008)
 * With A_o = COV[o] + FACTOR[o] FACTOR[o]^T of a row of the other side, S_r and w_r the listed sums above and
 * G = sum over ALL rows o of the other side of A_o (K x K, the Gram matrix):
 *     S'_r   = (1 - weight) S_r + weight G
 *     COV[r] = inv(I/eta2 + S'_r/sigma2),  FACTOR[r] = COV[r] w_r / sigma2     for EVERY row, with or without ratings
 *     ESS_r  = c_r - 2 m_r . w_r + < V_r + m_r m_r^T, S'_r >                    (c_r = 0 for a row without ratings)
 *     L      = -1/2 [ N log(2 pi sigma2) + (U I - N) log(2 pi sigma2 / weight) ] - sum_r ESS_r / (2 sigma2)
 *              + the prior and entropy blocks as above
 * A row without ratings is no special case: m = 0 exactly and V = inv(I/eta2 + weight G/sigma2).  ESS summed over the
 * rows of either side gives the same total.
 *   pmf_gauss_factor_sweep  G of the other side from its state as it is when the call starts (pmf_gauss_gram's two
 *                           launches), then per row window (the windows of pmf_gauss_elbo_terms, PMF_ELBO_ROWS):
 *                           accumulate into a context-owned window, blend (S = fma(T(1 - weight), S, T(weight G)), one
 *                           element-wise pass), and the row solver over all rows of the window.
 *   pmf_gauss_fold_in       G of the opposite side once per call; every row of the batch is blended and solved, so a row
 *                           without ratings gets inv(I/eta2 + weight G/sigma2), not the prior.
 *   pmf_gauss_elbo_terms    with_data != 0: ESS from S'; every row has an ESS.  with_data == 0: unchanged.
 * A property of the context, independent of pmf_ctx_set_gamma_zeros: no state array changes, and it may be set before or
 * after the ratings.  `weight` is ignored (and the stored weight kept) under PMF_ZEROS_MISSING; the getter returns the
 * stored weight, 1.0 for a new context.  pmf_predict*, the top-k / rank calls and the Poisson / HPF calls do not read
 * the mode.  Duplicate (u, i) pairs are each a listed rating; a cell with one rating is the caller's to ensure (the
 * model classes refuse duplicates).
 * Not covered, PMF_EINVAL naming the mode, while the mode is PMF_ZEROS_OBSERVED: the three calls above when both sides
 * have a BIAS array; pmf_gauss_bias_sweep / _accumulate / _finalize; pmf_gauss_factor_accumulate / _finalize;
 * pmf_gauss_sgd_sweep / _accumulate / _finalize; and several ranks -- PMF_ZEROS_OBSERVED on a context with a
 * communicator, and pmf_comm_init / pmf_comm_attach (and the test build's pmf_comm_init_hostshm) on a context in the
 * mode.  PMF_EINVAL also for a null context, a mode that is neither value, a weight that is not finite or outside
 * (0, 1] under PMF_ZEROS_OBSERVED, and two null outputs of the getter.  An error changes nothing. */
int pmf_ctx_set_gauss_zeros(pmf_ctx *ctx, int mode, double weight);
int pmf_ctx_get_gauss_zeros(pmf_ctx *ctx, int *mode /* may be NULL */, double *weight /* may be NULL */);
/* G of `side` in either mode, as a full symmetric K x K matrix (row-major, double): G[i][j] = sum over ALL rows r of
 * COV[r][i][j] + FACTOR[r][i] FACTOR[r][j].  Every addend is formed in double from the stored values and the sum is in
 * double.  Two stages, no atomics and no work list: a fixed grid of blocks, each owning a tile of 256 packed positions
 * and a contiguous row range (16-byte loads per lane; a lane owns the same packed positions for every row, so its mean
 * indices are loop constants; the mean rows are staged in LDS as doubles), the four wavefronts' sums added in wavefront
 * order; a second launch adds the block sums of a position in block order and writes G packed in double and
 * weight x G, formed in double and rounded once to the context dtype.  Two calls give the same bits, whatever the task
 * length.  Reads the model state only; its work area is context-owned: pmf_ctx_device_bytes may grow on the first
 * call and does not grow after it.  Timed as PMF_KERNEL_GAUSS_COMBINE.  PMF_EINVAL, with the missing thing named: null
 * context, bad side, null out, FACTOR or COV of `side` not set.  Cost: DESIGN.md section 4.17. */
int pmf_gauss_gram(pmf_ctx *ctx, int side, double *out /* K x K */);

/* Multi-GPU forms: raw per-row sums into / from a caller-owned DEVICE buffer.
 * Factor: [rows x (Kp + Kpad)] = packed lower triangle of S, then the
 * right-hand side (Kp = K(K+1)/2 rounded up to a multiple of 4, see
 * pmf_ctx_cov_stride).  Bias: [rows x 2] = residual sum, rating count. */
int pmf_ctx_cov_stride(pmf_ctx *ctx, int *stride);
int pmf_gauss_factor_accumulate(pmf_ctx *ctx, int side, void *stats_dev);
int pmf_gauss_factor_finalize(pmf_ctx *ctx, int side, const void *stats_dev, double sigma2,
                              double eta2);
int pmf_gauss_bias_accumulate(pmf_ctx *ctx, int side, void *stats_dev);
int pmf_gauss_bias_finalize(pmf_ctx *ctx, int side, const void *stats_dev, double sigma2,
                            double eta_bias2);

/* ---- multi-GPU: RCCL inside the library (SURVEY.md section 8(b) `pmf_comm_init`, section 8(e)) ------
 * No reference counterpart (the reference is a single process).  One process per GPU; ratings are
 * sharded by USER RANGE (the context's n_users is this rank's range, ids local to it), the item block
 * is replicated.  Once a context has a communicator (of any size), every ITEM-side half-sweep
 * (pmf_gamma_sweep, pmf_gauss_factor_sweep, pmf_gauss_bias_sweep, pmf_gauss_sgd_sweep with
 * side = PMF_SIDE_ITEM) runs inside the library as
 *     accumulate raw per-item sums over this rank's ratings  ->  exchange (sum over ranks)  ->  finalize
 * on a library-owned statistics buffer, pipelined over the item row chunks of pmf_ctx_set_row_chunks:
 * the all-reduce of chunk c runs on a second, high-priority HIP stream and its finalisation on a third
 * (ordered against the compute stream by events, never by the host) while chunk c+1 is accumulated.  Per-row arithmetic is that of
 * the accumulate / finalize pair, so results do not depend on the chunking, and every rank ends the
 * half-sweep with bit-identical item state.  USER-side half-sweeps stay local.  The iteration order a
 * caller issues is unchanged (gaussian_mf_cavi_bias.py:129-263, hpf_cavi.py:121-193).
 * pmf_gamma_ext_sweep is not available with a communicator.
 *
 * pmf_comm_unique_id: 128 bytes from ncclGetUniqueId; rank 0 creates them and hands them to the other
 * ranks out of band (pmf_hip/dist.py: a file next to the launcher's rendezvous).  pmf_comm_init: RCCL
 * communicator over xGMI, collective (every rank must call it).  pmf_comm_attach lets a
 * second context of the same process and device share `owner`'s communicator; pmf_comm_destroy
 * detaches (the communicator goes with its last user; pmf_ctx_destroy detaches too).
 *
 * Exchange of a chunk's statistics (pmf_comm_set_exchange; the same mode on every rank):
 *   PMF_EXCHANGE_ALLREDUCE       ncclAllReduce, then every rank finalises every row;
 *   PMF_EXCHANGE_SCATTER_GATHER  ncclReduceScatter -> each rank finalises its 1/nranks of the chunk's rows ->
 *                                ncclAllGather of the finalised state (the reference solves each row once,
 *                                gaussian_mf_cavi_bias.py:170-201: so does the job as a whole, instead of
 *                                nranks times).  Same wire bytes for the Gaussian factor sweep, whose state
 *                                is as wide as its statistics; replicas stay bit-identical either way;
 *   PMF_EXCHANGE_AUTO (default)  SCATTER_GATHER for pmf_gauss_factor_sweep on more than one rank (finalize =
 *                                a K x K solve per row), ALLREDUCE for the sweeps whose finalize is
 *                                element-wise.  Environment PMF_COMM_EXCHANGE=allreduce|scatter_gather
 *                                sets the default of new contexts. */
#define PMF_UNIQUE_ID_BYTES 128
#define PMF_TRANSPORT_RCCL 0
#define PMF_OP_SUM 0
#define PMF_OP_MAX 1
#define PMF_EXCHANGE_AUTO 0
#define PMF_EXCHANGE_ALLREDUCE 1
#define PMF_EXCHANGE_SCATTER_GATHER 2
int pmf_comm_unique_id(void *id_out);
int pmf_comm_init(pmf_ctx *ctx, int nranks, int rank, const void *unique_id);
int pmf_comm_set_exchange(pmf_ctx *ctx, int mode);
#ifdef PMF_TEST_TRANSPORT
/* TEST BUILDS ONLY (libpmf_hip_test.so, -DPMF_TEST_TRANSPORT; the product library does not export it): the same
 * interface over POSIX shared memory for ranks that share ONE GPU -- a rehearsal transport for one-GPU
 * boxes (RCCL refuses two ranks per device). */
#define PMF_TRANSPORT_HOSTSHM 1
int pmf_comm_init_hostshm(pmf_ctx *ctx, int nranks, int rank, const void *unique_id);
#endif
int pmf_comm_attach(pmf_ctx *ctx, pmf_ctx *owner);
int pmf_comm_destroy(pmf_ctx *ctx);
int pmf_comm_info(pmf_ctx *ctx, int *nranks, int *rank, int *transport);
/* Waiting under a communicator: pmf_ctx_sync (of a context with a communicator), pmf_comm_barrier,
 * pmf_comm_allreduce_host and pmf_comm_gather_user_rows poll the stream, the communicator's asynchronous error
 * state and a deadline (environment PMF_COMM_TIMEOUT_S, seconds, default 1800, 0 = none).  When a peer died or
 * never reached its collective they abort the communicator and return PMF_ECOMM; every later collective call on
 * it returns PMF_ECOMM at once. */
/* all queued work of every rank (kernels and collectives) has finished when this returns */
int pmf_comm_barrier(pmf_ctx *ctx);
/* element-wise sum / max of n host doubles over the ranks, result on every rank (validation sums of
 * the sharded monitor -- hpf_cavi.py:196-211 --, timings) */
int pmf_comm_allreduce_host(pmf_ctx *ctx, double *values, int64_t n, int op);
/* the USER-side rows of `array` of every rank, concatenated in rank order, as host float64 on every
 * rank; bounds[nranks + 1] = the global user ranges (what `fit` needs to hand back full
 * E_theta / m_theta, train_poisson_full.py:68-76).  Collective. */
int pmf_comm_gather_user_rows(pmf_ctx *ctx, int array, const int64_t *bounds, double *host_full);

/* ---- Gaussian MF, MAP by stochastic gradient steps -------------
 * NO reference counterpart (the reference's Gaussian model is CAVI only): parity unpinned, the
 * oracle is this build's own restatement (oracle/cavi_oracle.py:gauss_sgd_half_sweep).  One call
 * walks every row of `side` through its ratings in input order with the other side fixed:
 *   e = x - b_r - b_o - f_r . f_o;  f_r += lr (e f_o / sigma2 - f_r / (eta2 n_r));
 *   b_r += lr (e / sigma2 - b_r / (eta_bias2 n_r))        (biases only if both BIAS arrays are set)
 * Rows longer than 256 ratings are cut into pieces that start from the row's old value; the row
 * moves by the rating-count-weighted mean of the pieces' displacements.  The accumulate / finalize
 * pair exposes that sum -- [rows x width] = sum len * d_f | sum len * d_b | sum len | 0 0, width from
 * pmf_ctx_sgd_stats_width -- so that ranks holding different ratings of an item can all-reduce it
 * (honours pmf_ctx_select_chunk like the other accumulate / finalize calls). */
int pmf_gauss_sgd_sweep(pmf_ctx *ctx, int side, double lr, double sigma2, double eta2, double eta_bias2);
int pmf_ctx_sgd_stats_width(pmf_ctx *ctx, int *width);
int pmf_gauss_sgd_accumulate(pmf_ctx *ctx, int side, void *stats_dev, double lr, double sigma2, double eta2,
                             double eta_bias2);
int pmf_gauss_sgd_finalize(pmf_ctx *ctx, int side, const void *stats_dev);

/* ---- predict / evaluate -------------------------------------------------
 * `predict` (hpf_cavi.py:215-231, poisson_mf_cavi.py:221-241,
 * gaussian_mf_cavi_bias.py:291-316): out[n] = FACTOR_user[u].FACTOR_item[i]
 * (+ BIAS_user[u] + BIAS_item[i] when bit 0 of `use_bias` is set; multiplied by
 * SCALE_user[u] SCALE_item[i] when bit 1 is set -- the extended Poisson model's
 * predict, poisson_mf_extended_cavi.py:239-259) for ids inside the trained
 * dimensions, 0 otherwise; `offset` (global_mean) is added to every row. */
#define PMF_PREDICT_BIAS 1
#define PMF_PREDICT_SCALE 2
int pmf_predict(pmf_ctx *ctx, int64_t n, const int32_t *user_ids, const int32_t *item_ids,
                int use_bias, double offset, double *out);

/* Validation set kept on the device for the per-iteration monitor of `fit`
 * (hpf_cavi.py:196-211, gaussian_mf_cavi_bias.py:268-284).  `label_index[n]`
 * maps each true rating to its position in np.unique(y_true) (n_labels <= 32)
 * for the per-label error sums of metrics.macro_mae (metrics.py:37-51). */
int pmf_eval_set(pmf_ctx *ctx, int64_t n, const int32_t *user_ids, const int32_t *item_ids,
                 const double *y_true, const int32_t *label_index, int n_labels);
/* Fused predict + reduction over the stored validation set: sum of squared
 * errors, per-label sum of |error| and per-label counts.  The host finishes
 * rmse = sqrt(sse / n) (metrics.py:6-10) and macro_mae = mean_l(abs_l / cnt_l). */
int pmf_eval_run(pmf_ctx *ctx, int use_bias, double offset, double *sum_sq_err,
                 double *abs_err_per_label, int64_t *count_per_label);

/* Posterior predictive variance of the Gaussian models (no reference counterpart: the reference's predict returns
 * the mean and its GaussianLogPredictiveLikelihood plugs the factor means in).  With q(theta_u) = N(m_u, V_u) and
 * q(beta_i) = N(m_i, V_i) independent (FACTOR / COV of the two sides; the biases are point values) and
 * f = theta_u . beta_i:
 *     E[f]   = m_u . m_i                                          (pmf_predict)
 *     Var[f] = m_u' V_i m_u + m_i' V_u m_i + tr(V_u V_i)
 * evaluated in one pass over the two packed rows, w_p = 1 on the diagonal and 2 off it, p = (r, c):
 *     out_var[n] = sum_p w_p ( V_i[p] m_u[r] m_u[c] + V_u[p] m_i[r] m_i[c] + V_u[p] V_i[p] )
 * for ids inside the trained dimensions, 0 otherwise (pmf_predict treats such a pair as the point 0).  The rating's
 * predictive variance is sigma2 + out_var.  Needs FACTOR and COV of both sides (PMF_EINVAL names a missing one);
 * n = 0 touches nothing. */
int pmf_predict_var(pmf_ctx *ctx, int64_t n, const int32_t *user_ids, const int32_t *item_ids, double *out_var);
/* The same over the stored validation set (pmf_eval_set), fused with pmf_predict: with v = Var[f] of a pair and
 * e = y_true - predict (`use_bias`, `offset` as for pmf_eval_run),
 *     *sum_var         = sum v
 *     *sum_log_density = sum ( -1/2 log(2 pi (sigma2 + v)) - e^2 / (2 (sigma2 + v)) ),      sigma2 > 0,
 * the total log density of the ratings under N(predict, sigma2 + v).  Per-block partial sums combined in block
 * order on the host: two calls give the same bits. */
int pmf_eval_run_var(pmf_ctx *ctx, int use_bias, double offset, double sigma2, double *sum_var,
                     double *sum_log_density);

/* Top-k items per user from the dense reconstruction FACTOR_user . FACTOR_item^T
 * (the "identical top-k item rankings" check of the north star; the reference
 * has no ranking API -- scores follow `predict`: `use_bias` is predict's flag, 0, PMF_PREDICT_BIAS
 * (+ BIAS_user[u] + BIAS_item[i]) or PMF_PREDICT_SCALE (x SCALE_user[u] SCALE_item[i], the extended
 * Poisson model); ties are broken by the lower item id, NaN scores never rank).
 * out_items / out_scores hold n_query x k entries (-1 / 0 when fewer than k items rank).
 * fp32 contexts with Kpad <= 128 and k <= 64 run one fused kernel: score tiles on the matrix cores
 * (v_mfma_f32_32x32x2_f32), the running k best per user in LDS, no score matrix in HBM. */
int pmf_topk_items(pmf_ctx *ctx, int64_t n_query, const int32_t *user_ids, int k, int use_bias,
                   int32_t *out_items, double *out_scores);
/* pmf_topk_items over the items a user has not rated: what a recommender serves, and the list whose recall@k
 * pmf_rank_items(.., exclude_train = 1) measures.  With `exclude_train` == 0 the call IS pmf_topk_items (same code
 * path, same bits).  With `exclude_train` != 0 the candidates of query user u are the items j that are not among the
 * DISTINCT items of u's training ratings (pmf_ctx_set_ratings keeps duplicate pairs; each item counts once; a user
 * without ratings excludes nothing).  Order, ties (lower item id), -0.0 == +0.0 and "a NaN score never ranks" are
 * those of pmf_topk_items, and the item at position p of u's row is the candidate whose
 * pmf_rank_items(.., exclude_train = 1) rank is p -- to the bit, tie groups included: both calls take the score of a
 * pair from the same three functions.  A user with fewer than k rankable candidates gets -1 / 0.0 in the rest of the
 * row: min(k, out_candidates of pmf_rank_items) entries are valid, none for a user who rated every item.  Repeated
 * query users are allowed; k in [1, min(1024, n_items)].
 * Reads the context only: model state, ratings, work lists and the stored validation set stay as they are (the first
 * excluding call after pmf_ctx_set_ratings builds the distinct-item lists unless pmf_rank_items already has, and
 * pmf_ctx_device_bytes then counts them; later calls of either kind add nothing; new ratings rebuild them).  Never a
 * collective; two calls give the same bits.
 * Errors (naming what is missing): those of pmf_topk_items, and PMF_EINVAL for `exclude_train` without ratings.  An
 * argument error writes nothing; n_query = 0 touches nothing.
 * The fused kernel drops an excluded item where a score has already passed its user's threshold, so the scan's steady
 * state is that of pmf_topk_items; the two-phase path overwrites the excluded pairs' scores with NaN before the
 * select (DESIGN.md 4.14 has the mechanism and what it costs).  Timed under PMF_KERNEL_TOPK. */
int pmf_topk_items_excluding(pmf_ctx *ctx, int64_t n_query, const int32_t *user_ids, int k, int use_bias,
                             int exclude_train, int32_t *out_items, double *out_scores);

/* Ranks of held-out items (no reference counterpart: the reference evaluates point errors only).  Query row r is user
 * user_ids[r] (repeats allowed) with the target items item_ids[row_ptr[r] .. row_ptr[r + 1]) (row_ptr[0] = 0,
 * non-decreasing; a row without targets is legal).  With s_uj the score pmf_topk_items / pmf_predict define under
 * `use_bias` (0, PMF_PREDICT_BIAS or PMF_PREDICT_SCALE; no offset, which does not change the order), the 0-based rank of
 * target i of user u is
 *     out_rank = #{ j in [0, n_items), j != i, j not excluded for u :  s_uj > s_ui  or  (s_uj == s_ui and j < i) }
 * -- the order of pmf_topk_items: score descending, ties to the lower item id, -0.0 == +0.0, a NaN score never
 * outranks anything; a target whose own score is NaN gets -1.  With `exclude_train` != 0 the excluded items of u are
 * the DISTINCT items of u's training ratings (pmf_ctx_set_ratings keeps duplicate pairs; each item counts once).
 * Exclusion applies to competitors only: a target that is itself a training item is ranked against the rest.
 *     out_candidates[r] = #{ j : s_uj is not NaN, j not excluded for u }          (may be NULL)
 * so that a percentile rank needs no second call.  s_ui is the very number the scan computes for item i of user u
 * (exact score ties are common: every item without ratings keeps its prior row).
 * Reads FACTOR of both sides (BIAS / SCALE under the flag) and, for `exclude_train`, the training ratings; model
 * state, ratings, work lists and the stored validation set stay as they are (the first `exclude_train` call after
 * pmf_ctx_set_ratings builds the distinct-item lists, which pmf_ctx_device_bytes then counts).  Never a collective.
 * PMF_EINVAL (naming what is missing): null context or array, n_rows < 0, bad row_ptr, bad use_bias, a missing array,
 * `exclude_train` without ratings; PMF_ERANGE: a user or item id outside the trained dimensions (or a context of more
 * than 2^31 - 65 items: the kernels count items in 32-bit integers).  An argument error
 * writes nothing; n_rows = 0 touches nothing.
 * fp32 contexts with Kpad <= 128 scan Theta . Beta^T in score tiles on the matrix cores as pmf_topk_items does and
 * count instead of keeping lists; no score matrix in HBM.  Timed under PMF_KERNEL_TOPK. */
int pmf_rank_items(pmf_ctx *ctx, int64_t n_rows, const int32_t *user_ids, const int64_t *row_ptr,
                   const int32_t *item_ids, int use_bias, int exclude_train, int64_t *out_rank,
                   int64_t *out_candidates);

/* Top-k and ranks for ANY query rows against all rows of one side: recommendations for rows the fit has not seen (the
 * factors pmf_gauss_fold_in / pmf_gamma_fold_in return), similar items and similar users (one side against itself), the
 * audience of an item (users as candidates).  The scans are those of pmf_topk_items / pmf_rank_items; what differs is
 * where their operands come from.
 * Candidates are all rows of `cand_side` (either side); k in [1, min(1024, rows(cand_side))].  Exactly one of `query_ids`
 * and `query_factor` is non-null:
 *   ids mode     query row q is row query_ids[q] of `query_side`'s FACTOR (repeats allowed); under PMF_PREDICT_BIAS its
 *                coefficient is BIAS[query_ids[q]], under PMF_PREDICT_SCALE SCALE[query_ids[q]].  query_side == cand_side
 *                is allowed with `score` 0 or PMF_SCORE_COSINE only: a bias or scale of two rows of one side is no model
 *                score (PMF_EINVAL).
 *   vector mode  query row q is the caller's K doubles query_factor[q K .. q K + K), converted to the context's dtype as
 *                pmf_set_array_rows converts; `query_side` is ignored; query_coef[q] is the row's bias or scale, required
 *                under PMF_PREDICT_BIAS / PMF_PREDICT_SCALE and ignored otherwise.
 * Score: that of pmf_topk_items under `score` = 0, PMF_PREDICT_BIAS or PMF_PREDICT_SCALE, from the same arithmetic.
 * PMF_SCORE_COSINE is dot * (inv_q * inv_c) with inv = 1 / sqrt(sum_k f_k^2) in the context's dtype (correctly rounded
 * square root and division), formed per call from the staged query rows and from cand_side's FACTOR as it is then; it runs
 * as PMF_PREDICT_SCALE on those inverse norms.  A zero row needs no special case: 0 * inf is NaN and a NaN never ranks, so
 * a zero candidate never appears and a zero query row gets a row of -1 / 0.0.
 * Order, ties (lower candidate id first), -0.0 == +0.0 and the NaN rule are those of pmf_topk_items.
 * Exclusion (ex_ptr may be NULL: none): ex_ids[ex_ptr[q] .. ex_ptr[q + 1]) are candidate ids that are no candidates of
 * query ROW q -- the list belongs to the row, not to the id: two rows with the same id may carry different lists.  The
 * lists may be in any order and hold repeats (the library sorts each and drops repeats before the upload).  In
 * pmf_rank_query exclusion applies to competitors only, as in pmf_rank_items.  Leaving the query itself out (similar
 * items) is the caller's one-entry list; there is no flag for it.
 * pmf_rank_query: the targets of row q are tgt_ids[tgt_ptr[q] .. tgt_ptr[q + 1]); out_rank (one per target) and
 * out_candidates (one per row, may be NULL) are defined as in pmf_rank_items with "item" read as "row of cand_side".
 * Position equals rank: the id at position p of row q in pmf_topk_query is the candidate whose pmf_rank_query rank is p,
 * to the bit, tie groups included (both calls stage the rows, the coefficients and the inverse norms with the same code);
 * min(k, out_candidates) entries of a row are valid.
 * pmf_topk_query(PMF_SIDE_ITEM, n, PMF_SIDE_USER, ids, NULL, NULL, score, NULL, NULL, k, ..) gives the bytes of
 * pmf_topk_items(n, ids, k, score), and with every row's list set to that user's training items those of
 * pmf_topk_items_excluding(.., 1, ..); the same holds for pmf_rank_query and pmf_rank_items.
 * Reads the context only: model state, ratings, work lists and the stored validation set stay as they are (the staging
 * buffers grow on the first call, pmf_ctx_device_bytes counts them, and a later call of the same size adds nothing).
 * Never a collective; two calls give the same bits.
 * PMF_EINVAL (naming what is wrong): null context, bad side, both or neither query source, a missing query_coef, a bad
 * score, a bad ex_ptr / tgt_ptr ([0] != 0 or decreasing), a null argument, a missing array (FACTOR of cand_side always,
 * FACTOR of query_side in ids mode, BIAS / SCALE as the score needs them).  PMF_ERANGE: k, a query id, a target id or an
 * excluded id out of range (naming the id and its position); for pmf_rank_query also more than 2^31 - 65 candidates
 * (pmf_topk_query sends that case to the two-phase path).  An argument error writes nothing; n_query = 0 touches nothing.
 * fp32 contexts with Kpad <= 128 (and k <= 64) run the fused scans, everything else the two-phase path / the generic
 * ranking kernel, as the item calls do; the diagnostic switches of those calls act here too.  Timed under
 * PMF_KERNEL_TOPK. */
#define PMF_SCORE_COSINE 4     /* `score` of the two query calls only; 0, PMF_PREDICT_BIAS, PMF_PREDICT_SCALE as elsewhere */
int pmf_topk_query(pmf_ctx *ctx, int cand_side, int64_t n_query, int query_side, const int32_t *query_ids,
                   const double *query_factor, const double *query_coef, int score, const int64_t *ex_ptr,
                   const int32_t *ex_ids, int k, int32_t *out_ids, double *out_scores);
int pmf_rank_query(pmf_ctx *ctx, int cand_side, int64_t n_query, int query_side, const int32_t *query_ids,
                   const double *query_factor, const double *query_coef, int score, const int64_t *ex_ptr,
                   const int32_t *ex_ids, const int64_t *tgt_ptr, const int32_t *tgt_ids, int64_t *out_rank,
                   int64_t *out_candidates);

/* Thompson-sampled top-k: pmf_topk_query in ids mode, scored on ONE joint posterior draw (pmf_gauss_sample_rows defines a
 * draw).  Every row of cand_side is sampled into a context-owned table of rows x Kpad elements (allocated on first use,
 * counted by pmf_ctx_device_bytes, kept: a later call of the same size adds nothing) that takes the place of cand_side's
 * FACTOR in the scan, and the query rows of every round are sampled into the staged query table; both sides use draw index
 * `draw` under `seed`.  Contract, to the bit: the row of (side, id) the scan reads equals pmf_gauss_sample_rows(side, id,
 * n_draws = 1, draw0 = draw, seed) converted to the context's dtype.  Biases (score = PMF_PREDICT_BIAS) are the stored
 * means.  Exclusion lists, order, ties, the NaN rule (a row that is not positive definite scores NaN), the limits of k,
 * the rounds and the fused / two-phase choice are pmf_topk_query's.  PMF_EINVAL besides pmf_topk_query's cases: null
 * query_ids, a score other than 0 or PMF_PREDICT_BIAS (PMF_SCORE_COSINE and PMF_PREDICT_SCALE are refused), draw < 0, COV
 * of either side missing.  The sampling is timed under PMF_KERNEL_GAUSS_SOLVE, the scan under PMF_KERNEL_TOPK. */
int pmf_topk_sampled(pmf_ctx *ctx, int cand_side, int64_t n_query, int query_side, const int32_t *query_ids,
                     int score /* 0 or PMF_PREDICT_BIAS */, const int64_t *ex_ptr, const int32_t *ex_ids, int k, uint64_t seed,
                     int draw, int32_t *out_ids, double *out_scores);

/* ---- profiling ----------------------------------------------------------
 * When enabled every kernel launch is bracketed by hipEvents on the context's
 * stream; pmf_prof_get synchronises and returns the accumulated device time
 * and launch count of one kernel class. */
int pmf_prof_enable(pmf_ctx *ctx, int enable);
int pmf_prof_reset(pmf_ctx *ctx);
int pmf_prof_get(pmf_ctx *ctx, int kernel, double *total_ms, int64_t *launches);
/* Gather ceiling of the Poisson/HPF half-sweep of `side` on THIS context's ratings and tables: the
 * average device time of `repeats` launches of the sweep kernel's memory side alone (same tasks, same
 * index / rating streams, same 16-byte-per-lane row gathers; one add per loaded value, no row output).
 * The gathered table of C3 (25.6 MB of item rows, 256 MB of user rows) lives in L2 / Infinity Cache,
 * so the sweep is bound by what the caches deliver for this pattern, not by HBM: algorithmic bytes /
 * this time is the kernel's roofline (bench.py, `roofline.bound = "cache_gather"`). */
int pmf_prof_gather_ceiling(pmf_ctx *ctx, int side, int repeats, double *ms_per_launch);

#ifdef __cplusplus
}
#endif
#endif /* PMF_HIP_H */
