// Internal declarations shared by the translation units of libpmf_hip.so.
// gfx950 only: wave64, 16-byte vector accesses, DPP row reductions.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <functional>
#include <initializer_list>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "pmf_hip.h"
#include "pmf_batch.h"   // pmf_set_error, pmf_check_offsets, PmfLayout, pmf_block_cut

#ifndef PMF_TRANSPORT_HOSTSHM
#define PMF_TRANSPORT_HOSTSHM 1   // declared by the header in test builds only (-DPMF_TEST_TRANSPORT)
#endif

#define PMF_WAVE 64
#define PMF_VEC 4               // elements per lane access (16 B fp32 / 32 B fp64)
#define PMF_RATE_FLOOR 1e-10    // hpf_cavi.py:141
#define PMF_MAX_LABELS 32

#define PMF_HIP_CHECK(expr)                                                         \
    do {                                                                            \
        hipError_t _e = (expr);                                                     \
        if (_e != hipSuccess) {                                                     \
            pmf_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),    \
                          __FILE__, __LINE__);                                      \
            return PMF_EHIP;                                                        \
        }                                                                           \
    } while (0)

#define PMF_REQUIRE(cond, code, ...)      \
    do {                                  \
        if (!(cond)) {                    \
            pmf_set_error(__VA_ARGS__);   \
            return (code);                \
        }                                 \
    } while (0)

// every ids[k] lies in [0, rows), or PMF_ERANGE naming the first that does not ("user id", "item id", "id")
static inline int pmf_check_ids(const int32_t *ids, int64_t n, int64_t rows, const char *fn, const char *noun) {
    for (int64_t k = 0; k < n; ++k)
        PMF_REQUIRE(ids[k] >= 0 && ids[k] < rows, PMF_ERANGE, "%s: %s %d at position %lld outside [0, %lld)", fn, noun, ids[k],
                    (long long)k, (long long)rows);
    return PMF_OK;
}

// f(), with std::bad_alloc turned into PMF_ENOMEM: host containers may throw, and nothing propagates across the C boundary
template <typename F>
static inline int pmf_no_throw(const char *fn, F &&f) {
    try {
        return f();
    } catch (const std::bad_alloc &) {
        pmf_set_error("%s: out of host memory", fn);
        return PMF_ENOMEM;
    }
}

// prologue of the per-side entry points (`ctx` and `side` are their arguments)
#define PMF_SIDE_ENTRY(fn)                                                                             \
    PMF_REQUIRE(ctx != nullptr, PMF_EINVAL, fn ": null context");                                      \
    PMF_REQUIRE(side == PMF_SIDE_USER || side == PMF_SIDE_ITEM, PMF_EINVAL, fn ": bad side %d", side); \
    PMF_HIP_CHECK(hipSetDevice(ctx->device))

// which part of a half-sweep a call runs: all of it, the raw statistics only, or the rows from summed statistics
enum PmfPass { PMF_PASS_FUSED, PMF_PASS_ACCUMULATE, PMF_PASS_FINALIZE };

// Owner of one allocation (hipMalloc, or hipHostMalloc for a PINNED one): the pointer, its byte count and the context
// whose device_bytes counts it (null: counted nowhere -- pinned memory, the communicator's and the index build's
// buffers).  Move-only; the destructor releases.  Everything that is handed to a kernel is a raw view from as<T>().
class PmfBuf {
public:
    enum Kind { DEVICE, PINNED };
    explicit PmfBuf(Kind kind = DEVICE) : pinned_(kind == PINNED) {}
    PmfBuf(PmfBuf &&o) noexcept : pinned_(o.pinned_) { *this = std::move(o); }
    PmfBuf &operator=(PmfBuf &&o) noexcept;
    ~PmfBuf() { reset(); }
    // a fresh allocation of `bytes` (0 -> 16) in place of what the buffer held
    int alloc(pmf_ctx *owner, size_t bytes);
    // grow-only: nothing happens while `bytes` fit; else the streams in `sync` (work queued on them may still use
    // the buffer) are waited for and the buffer is replaced by a larger one -- its content is not kept
    int reserve(pmf_ctx *owner, size_t bytes, std::initializer_list<hipStream_t> sync);
    void reset();
    template <typename T = void>
    T *as() const { return static_cast<T *>(p_); }
    explicit operator bool() const { return p_ != nullptr; }

private:
    void *p_ = nullptr;
    size_t bytes_ = 0;
    pmf_ctx *owner_ = nullptr;
    bool pinned_;
};

// One unit of sweep work: a contiguous run of one row's ratings.
// slot < 0  : the run is the whole row  -> the kernel finalises the row itself
// slot >= 0 : the row is split          -> raw sums go to partial slot `slot`
struct PmfTask {
    int64_t start;   // offset into the side's col/val arrays
    int32_t row;
    int32_t len;
    int32_t slot;
    int32_t pad;
};

// A row whose ratings were split over several tasks (heavy rows).
struct PmfSplitRow {
    int32_t row;
    int32_t first_slot;
    int32_t n_slots;
    int32_t pad;
};

struct PmfTaskList {
    int64_t n_tasks = 0;
    int64_t n_slots = 0;
    int64_t n_split = 0;
    int32_t max_len = 0;
    PmfBuf d_tasks;       // PmfTask [n_tasks]
    PmfBuf d_split;       // PmfSplitRow [n_split]
    PmfBuf d_split_rows;  // int32_t [n_split]: row id of every split row (solve list)
    // row chunks (pmf_ctx_set_row_chunks): tasks are grouped by the chunk of their row,
    // longest-first inside each group; [n_chunks + 1] offsets into d_tasks / d_split
    std::vector<int64_t> task_off, split_off;
};

// The part of a task list (and of the row range) one accumulate / finalize call covers.
struct PmfTaskView {
    const PmfTask *d_tasks = nullptr;
    const PmfSplitRow *d_split = nullptr;
    const int32_t *d_split_rows = nullptr;
    int64_t n_tasks = 0, n_split = 0, n_slots = 0;
    int64_t row0 = 0, row1 = 0;            // row range [row0, row1)
    const int32_t *d_nonempty = nullptr;   // rows of the range with at least one rating
    int64_t n_nonempty = 0;
};

// The rows of a side in windows whose Gaussian statistics fit a fixed budget (pmf_gauss.hip), for the factor sweep under
// PMF_ZEROS_OBSERVED and for pmf_gauss_elbo_terms.  The tasks are the Gaussian list again (same length, same cuts) by window.
struct PmfRowWindows {
    PmfTaskList tasks;
    std::vector<int64_t> bounds;      // [n_windows + 1] first row of every window; empty = not built
    std::vector<uint8_t> has_empty;   // [n_windows] 1 if the window has a row without ratings, which no task writes
};

// Ratings ordered by one side (CSR when side = user, CSC when side = item).  A default-constructed value is
// "no ratings": d_ptr is what the sweeps test.
struct PmfSideIndex {
    PmfBuf d_ptr;                // int64_t [rows + 1]
    PmfBuf d_other;              // int32_t [nnz] id on the opposite side
    PmfBuf d_val;                // [nnz] rating, context dtype
    // pmf_ctx_set_ratings_weighted: the per-rating confidence weights c_j in this side's order and the per-row sums C_r
    // (summed in double in the row's rating order, rounded once).  Both null while the context holds no weights.
    PmfBuf d_wgt;                // [nnz] context dtype
    PmfBuf d_wsum;               // [rows] context dtype
    std::vector<double> h_wsum;  // [rows] C_r in double (pmf_ctx_rating_weight_sums); empty without weights
    // pmf_gauss_logit_refresh has rewritten d_wgt / d_wsum of this side: h_wsum is stale, pmf_ctx_rating_weight_sums
    // reads d_wsum back instead.  Goes with the ratings.
    bool wsum_refreshed = false;
    std::vector<int64_t> h_ptr;  // host copy of ptr (task building)
    PmfBuf d_nonempty;           // int32_t [n_nonempty]: rows with at least one rating (Gaussian solve list)
    int64_t n_nonempty = 0;
    std::vector<int32_t> h_nonempty;    // host copy of d_nonempty
    std::vector<int64_t> nonempty_off;  // [n_chunks + 1] offsets into d_nonempty
    PmfTaskList gamma_tasks;     // chunk = PMF_GAMMA_CHUNK, empty rows included
    PmfTaskList gauss_tasks;     // chunk = PMF_GAUSS_CHUNK, empty rows excluded
    PmfTaskList bias_tasks;      // chunk <= PMF_GAMMA_CHUNK, empty rows excluded
    PmfTaskList sgd_tasks;       // chunk = PMF_SGD_CHUNK exactly (the gradient mode is defined by it), empty rows excluded
    PmfRowWindows windows;       // built by the first call that needs them; goes with the ratings
    // pmf_rank_items with exclude_train (USER side only): every row's DISTINCT ids on the opposite side, ascending --
    // pmf_ctx_set_ratings keeps duplicate pairs.  Built on the first such call (pmf_index_distinct); goes with the ratings.
    PmfBuf d_distinct_ptr;       // int64_t [rows + 1]; null = not built
    PmfBuf d_distinct;           // int32_t [d_distinct_ptr[rows]]
    // Gaussian gather cache policy (PMF_GAUSS_HOT_MB; fp32, K <= 64): this side's most-rated rows, as many as fit
    // the budget, most-rated first (ties: lower id first) ...
    std::vector<int32_t> h_hot;
    // ... and per entry of d_other: 1 if that row of the OPPOSITE side is hot.  Null when the policy is off.
    PmfBuf d_other_hot;          // uint8_t [nnz]
};

struct PmfEvalSet {
    int64_t n = 0;
    int n_labels = 0;
    PmfBuf d_u, d_i;   // int32_t [n]
    PmfBuf d_y;        // double [n]
    PmfBuf d_label;    // int32_t [n]
};

struct pmf_ctx {
    int device = 0;
    int dtype = PMF_F32;
    int64_t rows[2] = {0, 0};
    int K = 0;
    int kpad = 0;        // K rounded up to PMF_VEC
    int kp = 0;          // K(K+1)/2
    int cov_stride = 0;  // kp rounded up to PMF_VEC
    int64_t nnz = 0;
    bool weighted = false;   // the ratings came with weights (pmf_ctx_set_ratings_weighted): index[side].d_wgt / d_wsum are set
    // Members are destroyed in reverse order: every buffer below goes (and is taken off device_bytes) before the
    // context's own stream does.
    struct OwnStream {
        hipStream_t s = nullptr;
        ~OwnStream() {
            if (s) (void)hipStreamDestroy(s);
        }
    } own_stream;
    hipStream_t stream = nullptr;
    size_t elem = 4;
    int64_t device_bytes = 0;   // what the context's device buffers hold (pmf_ctx_device_bytes); kept by PmfBuf

    int n_chunks[2] = {1, 1};    // row chunks per side (multi-GPU pipelining of a half-sweep)
    int cur_chunk[2] = {-1, -1};  // chunk the accumulate / finalize calls act on; -1 = all rows
    // row window of a finalize-from-statistics call inside pmf_comm_half_sweep (the sub-range of a chunk this rank
    // owns under the SCATTER_GATHER exchange); -1 = the whole selected chunk
    int64_t fin_row0 = -1, fin_row1 = -1;
    int exchange = PMF_EXCHANGE_AUTO;   // pmf_comm_set_exchange
    // pmf_ctx_set_gamma_zeros: PMF_ZEROS_OBSERVED makes the Poisson / HPF calls count every unlisted cell as a rating of 0
    // (the rate sums come from the other side's column sums, pmf_gamma.hip).  Never set together with a communicator.
    int gamma_zeros = PMF_ZEROS_MISSING;
    // pmf_ctx_set_gauss_zeros: PMF_ZEROS_OBSERVED makes pmf_gauss_factor_sweep / _fold_in / _elbo_terms count every unlisted
    // cell as an observation of 0 with variance sigma2 / gauss_zero_weight (the row statistics are blended with the other
    // side's Gram matrix, pmf_gauss.hip).  Independent of gamma_zeros; never set together with a communicator.
    int gauss_zeros = PMF_ZEROS_MISSING;
    double gauss_zero_weight = 1.0;

    PmfBuf arr[2][PMF_ARR_COUNT];   // model state, pmf_array_elems(side, array) elements of the context dtype
    PmfSideIndex index[2];
    PmfEvalSet eval;

    // scratch, grown on demand (pmf_ensure_*)
    PmfBuf d_partial, d_scratch;
    // Gaussian bias sweep from the factor sweep's mean sums (pmf_gauss.hip): d_mdot[side][r] = m_r . H_r, with m_r the
    // mean the fused factor sweep of `side` has just written and H_r the sum of the mean rows of the other side it
    // gathered for row r (a pair rated twice counts twice).  gauss_mdot_valid[side] holds while the FACTOR arrays of
    // BOTH sides and the ratings are what that sweep saw: everything that may write either calls pmf_factor_written.
    PmfBuf d_mdot[2];
    bool gauss_mdot_valid[2] = {false, false};
    // pmf_gamma_exact_sweep / _accumulate: the (E log, E) tables [rows][2][kpad] of the users, then of the items; rebuilt
    // by every call, in storage of their own so that a pmf_gamma_elbo_terms call (d_scratch) cannot write over them
    PmfBuf d_gamma_tables;
    // pmf_gauss_gram and the Gaussian calls under PMF_ZEROS_OBSERVED (pmf_gauss.hip): the Gram pass's block sums, the packed
    // G in double and w0 G in the context dtype; and the statistics window of the zero-mode sweep.  In storage of their own:
    // the row solvers and the ELBO row kernel lay out d_scratch while G is still needed.
    PmfBuf d_gauss_gram, d_gauss_window;
    // pmf_topk_query / pmf_rank_query (pmf_topk.hip): what a call keeps for all its rounds -- the sorted exclusion CSR and
    // the candidates' inverse norms -- and the staged query rows of one round (table, coefficients, gather ids).  Grown on
    // demand, in storage of their own: the scans' outputs and score matrix live in d_scratch.
    PmfBuf d_query_call, d_query_rows;
    // pmf_topk_sampled (pmf_topk.hip): the draw of every row of the candidate side, [rows x kpad] in the context dtype, and
    // behind it the sample kernel's packed triangles where they do not fit LDS.  Grown on first use, kept for the next call.
    PmfBuf d_sample_table;
    PmfBuf h_pinned{PmfBuf::PINNED};

    // diagnostic switches, read from the environment once when the context is created
    bool gauss_generic = false;    // PMF_GAUSS_GENERIC: the generic accumulate kernel instead of the MFMA ones
    bool gauss_unfused = false;    // PMF_GAUSS_UNFUSED: accumulate and solve as separate launches
    bool gauss_lds_solve = false;  // PMF_GAUSS_LDS_SOLVE: the block-per-row LDS solve for 64 < K <= 128
    bool gauss_bias_gather = false;  // PMF_GAUSS_BIAS_GATHER: the bias sweep always gathers the mean rows (never the factor sweep's mean sums)
    int64_t gauss_hot_bytes = 0;   // PMF_GAUSS_HOT_MB: budget of the hot gathered rows per side (0: policy off)
    int topk_max_blocks = 0;       // PMF_TOPK_MAX_BLOCKS=n caps the fused kernel's persistent grid (tests: many tiles per block)
    int topk_stage_buffers = 0;    // PMF_TOPK_STAGE_BUFFERS=1|2 pins the fused kernel's stage buffering (0: by residency)
    bool topk_two_phase = false;   // PMF_TOPK_TWO_PHASE: score matrix in HBM + select instead of the fused kernel
    int rank_targets = 0;          // PMF_RANK_TARGETS=n caps the target slots of a query row of pmf_rank_items (tests: the splitting path with few targets; 0: all RANK_SLOTS)
    int64_t fold_in_rows = 0;      // PMF_FOLD_IN_ROWS=n caps the rows of one block of pmf_gauss_fold_in and pmf_gamma_fold_in (tests: many blocks on a small batch; 0: by scratch size)
    int64_t gamma_fold_long = 0;   // PMF_GAMMA_FOLD_LONG=n: rows of pmf_gamma_fold_in with more than n ratings take the block-per-row kernel (tests: both kernels on small rows; 0: kGammaFoldLongRow)
    int64_t gamma_pred_pairs = 0;  // PMF_GAMMA_PRED_PAIRS=n caps the pairs of one staging round of pmf_gamma_predictive (tests: many rounds on a small batch; 0: kGammaPredPairs)
    int64_t topk_query_rows = 0;   // PMF_TOPK_QUERY_ROWS=n caps the query rows of one round of pmf_topk_items*, pmf_rank_items and the two query calls, rounded down to a multiple of 32 and at least 32 (tests: many rounds on a small batch; 0: 1 << 20 rows, or 512 MB of scores on the two-phase path)
    int64_t stage_bytes = 64ll << 20;   // PMF_STAGE_BYTES=n: bytes of one staging round of pmf_set_array / pmf_get_array, the row exchanges, the fold-ins' downloads and pmf_comm_gather_user_rows, at least one row (tests: many rounds on a few rows; 0 / unset: 64 MiB)
    int64_t window_rows = 0;       // PMF_ELBO_ROWS=n caps the rows of one statistics window (PmfRowWindows) of pmf_gauss_elbo_terms and of the zero-mode factor sweep (tests: many windows on a small problem; 0: by scratch size)
    int task_chunk = 0;            // PMF_TASK_CHUNK=n (power of two in [32, 512]) fixes the task length of the gamma / Gaussian / bias lists (tests: long tasks on small problems; 0: by nnz)

    // multi-GPU (pmf_comm.hip): the communicator (shared between contexts of one process, refcounted)
    // and the library-owned statistics buffers of the item half-sweeps
    // (0: factor / gamma / gradient statistics, 1: Gaussian bias statistics)
    struct PmfComm *comm = nullptr;
    PmfBuf d_stats[2];

    bool prof = false;
    struct ProfRec {
        hipEvent_t a, b;
        int kernel;
    };
    std::vector<ProfRec> prof_pending;
    std::vector<hipEvent_t> prof_pool;
    double prof_ms[PMF_KERNEL_COUNT] = {};
    int64_t prof_n[PMF_KERNEL_COUNT] = {};

    ~pmf_ctx();   // with the context's device current: waits for the stream, releases the communicator, then the members
};

#define PMF_GAMMA_CHUNK 512   // (256 until round 2: 512 halves the split-row slots; HPF K=64 at C3: gamma_final 0.16 -> 0.08 ms)
#define PMF_SGD_CHUNK 256     // the gradient mode's piece length is part of its definition (include/pmf_hip.h)
#define PMF_GAUSS_CHUNK 512
#define PMF_FOLD_IN_BLOCK_NNZ (32ll << 20)   // staged ratings of one row block of the fold-ins (a longer single row still goes)
#define PMF_GAUSS_HOT_MB_DEFAULT 224   // hot-row budget when PMF_GAUSS_HOT_MB is unset

// The row blocks of a fold-in's CSR batch (row_ptr, other_ids, ratings), staged one at a time in buffers of the call.
// stage() takes the block that begins at row r0: it ends at r1 (pmf_block_cut: at most max_rows rows and
// PMF_FOLD_IN_BLOCK_NNZ ratings, and `fits` if given), holds the nnz ratings from offset `at` of the batch, and has its
// offsets (`ptr`, rebased to 0) and ratings (`val`, in the context dtype T) on the host and room for them and the ids on
// the device; upload(), after the caller's own reserves, puts them there.  The previous block must have ended with a
// stream synchronise: nothing queued may still read the buffers.
template <typename T>
struct PmfFoldStage {
    PmfBuf d_ptr, d_other, d_val;   // int64_t [r1 - r0 + 1], int32_t [nnz], T [nnz]
    PmfBuf d_wgt, d_wsum;           // T [nnz], T [r1 - r0]: the ratings' weights and their row sums (stage() with weights only)
    std::vector<int64_t> ptr;
    std::vector<T> val, wgt, wsum;
    int64_t r1 = 0, nnz = 0, at = 0;

    // `weights` (may be null): one per rating of the batch; staged with the ratings, with every row's sum (formed in
    // double in rating order, rounded once)
    int stage(pmf_ctx *ctx, int64_t n_rows, const int64_t *row_ptr, const double *ratings, int64_t r0, int64_t max_rows,
              const std::function<bool(int64_t)> &fits = nullptr, const double *weights = nullptr) {
        r1 = pmf_block_cut(row_ptr, n_rows, r0, max_rows, PMF_FOLD_IN_BLOCK_NNZ, [&](int64_t n) { return !fits || fits(n); });
        at = row_ptr[r0];
        nnz = row_ptr[r1] - at;
        ptr.resize((size_t)(r1 - r0) + 1);
        for (int64_t r = r0; r <= r1; ++r) ptr[(size_t)(r - r0)] = row_ptr[r] - at;
        val.resize((size_t)nnz);
        for (int64_t k = 0; k < nnz; ++k) val[(size_t)k] = (T)ratings[at + k];
        int rc;
        wgt.clear();
        wsum.clear();
        if (weights) {
            wgt.resize((size_t)nnz);
            for (int64_t k = 0; k < nnz; ++k) wgt[(size_t)k] = (T)weights[at + k];
            wsum.resize((size_t)(r1 - r0));
            for (int64_t r = r0; r < r1; ++r) {
                double c = 0.0;
                for (int64_t k = row_ptr[r]; k < row_ptr[r + 1]; ++k) c += weights[k];
                wsum[(size_t)(r - r0)] = (T)c;
            }
            if ((rc = d_wgt.reserve(ctx, (size_t)nnz * sizeof(T), {ctx->stream}))) return rc;
            if ((rc = d_wsum.reserve(ctx, wsum.size() * sizeof(T), {ctx->stream}))) return rc;
        }
        if ((rc = d_ptr.reserve(ctx, ptr.size() * sizeof(int64_t), {ctx->stream}))) return rc;
        if ((rc = d_other.reserve(ctx, (size_t)nnz * sizeof(int32_t), {ctx->stream}))) return rc;
        return d_val.reserve(ctx, (size_t)nnz * sizeof(T), {ctx->stream});
    }
    int upload(const int32_t *other_ids) {
        PMF_HIP_CHECK(hipMemcpy(d_ptr.as(), ptr.data(), ptr.size() * sizeof(int64_t), hipMemcpyHostToDevice));
        if (nnz) {
            PMF_HIP_CHECK(hipMemcpy(d_other.as(), other_ids + at, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice));
            PMF_HIP_CHECK(hipMemcpy(d_val.as(), val.data(), (size_t)nnz * sizeof(T), hipMemcpyHostToDevice));
            if (!wgt.empty()) PMF_HIP_CHECK(hipMemcpy(d_wgt.as(), wgt.data(), (size_t)nnz * sizeof(T), hipMemcpyHostToDevice));
        }
        if (!wsum.empty()) PMF_HIP_CHECK(hipMemcpy(d_wsum.as(), wsum.data(), wsum.size() * sizeof(T), hipMemcpyHostToDevice));
        return PMF_OK;
    }
};

// first row of chunk c of a side (c = n_chunks gives the row count)
static inline int64_t pmf_chunk_row0(const pmf_ctx *ctx, int side, int c) {
    return ctx->rows[side] * (int64_t)c / ctx->n_chunks[side];
}
// Work list of `rows` rows given by their offsets `ptr` (pmf_ctx.hip): runs of at most `chunk` ratings, longest first
// inside each row group of `row_bounds`; rows longer than `chunk` are split evenly and listed in `split`.
void pmf_build_tasks(const std::vector<int64_t> &ptr, int64_t rows, int chunk, bool keep_empty,
                     const std::vector<int64_t> &row_bounds, std::vector<PmfTask> &tasks, std::vector<PmfSplitRow> &split,
                     int64_t &n_slots, std::vector<int64_t> &task_off, std::vector<int64_t> &split_off);
// pmf_build_tasks into `out` and onto the device.  `solve_list`: also d_split_rows, the ids of the split rows.
int pmf_upload_tasks(pmf_ctx *ctx, const std::vector<int64_t> &ptr, int64_t rows, int chunk, bool keep_empty,
                     const std::vector<int64_t> &row_bounds, bool solve_list, PmfTaskList &out);
// task length of the context's gamma / Gaussian / bias lists: PMF_TASK_CHUNK, or by the rating count, at most `max_chunk`
int pmf_task_chunk(const pmf_ctx *ctx, int max_chunk);
// `select` = honour pmf_ctx_select_chunk (accumulate / finalize); fused sweeps pass false
PmfTaskView pmf_task_view(const pmf_ctx *ctx, int side, const PmfTaskList &tl, bool select);

int pmf_ensure_partial(pmf_ctx *ctx, size_t bytes);
int pmf_ensure_scratch(pmf_ctx *ctx, size_t bytes);
int pmf_ensure_pinned(pmf_ctx *ctx, size_t bytes);
// allow `kernel` `bytes` of dynamic LDS on the current device: asks the runtime only for more than the default 48 KB and
// more than the function has been granted before (grants never shrink); PMF_EHIP with the runtime's message if it refuses
int pmf_allow_dynamic_lds(const void *kernel, size_t bytes);
size_t pmf_array_elems(const pmf_ctx *ctx, int side, int array);  // device elements
int pmf_require_array(pmf_ctx *ctx, int side, int array, const char *what);
int pmf_alloc_array(pmf_ctx *ctx, int side, int array);  // no-op if present (zero-filled)

// device-side index build (pmf_index.hip)
struct PmfIndexBuild;
int pmf_index_device_begin(pmf_ctx *ctx, int64_t nnz, const int32_t *user_ids, const int32_t *item_ids,
                           const double *ratings, const double *weights /* may be null */, PmfIndexBuild **out,
                           int64_t *bad_position);
void pmf_index_device_abort(PmfIndexBuild *b);
int pmf_index_device_finish(pmf_ctx *ctx, PmfIndexBuild *b, int64_t nnz);
// index[side].d_distinct_ptr / d_distinct from the side's d_ptr / d_other (no-op once built)
int pmf_index_distinct(pmf_ctx *ctx, int side);

// host <-> device layout helpers (pmf_ctx.hip)
void pmf_array_shape(const pmf_ctx *ctx, int array, int *host_width, int *dev_stride);
void pmf_unpack_rows(const pmf_ctx *ctx, int array, const void *src, double *dst, int64_t rows);
// `rows` rows of a device array laid out like `array` of the model state -> host float64, in pinned steps (ends with a
// stream synchronise)
int pmf_fold_in_download(pmf_ctx *ctx, int array, const void *dev, double *host, int64_t rows);

// Posterior draws of rows of `side` (pmf_gauss.hip; pmf_gauss_sample_rows documents them), queued on the context's stream
// and timed under PMF_KERNEL_GAUSS_SOLVE: request q is row d_ids[q] (device; null: row q), its draws d = 0 .. n_draws - 1
// have draw index draw0 + d and go to d_out[(q * n_draws + d) * kpad ..] in the context dtype, pad columns zero.  d_z
// (device, laid out like d_out; may be null) replaces the stream.  d_tri: pmf_gauss_sample_tri_bytes(ctx, n) bytes of the
// caller's for the packed triangles that do not fit LDS (0 bytes: null).  FACTOR and COV of `side` are checked by the caller.
size_t pmf_gauss_sample_tri_bytes(const pmf_ctx *ctx, int64_t n);
int pmf_gauss_sample_launch(pmf_ctx *ctx, int side, const int32_t *d_ids, int64_t n, int n_draws, int draw0, uint64_t seed,
                            const void *d_z, void *d_out, void *d_tri);

// multi-GPU (pmf_comm.hip).  With an attached communicator of more than one rank the ITEM half-sweeps
// run  accumulate -> all-reduce -> finalize  through pmf_comm_half_sweep.
bool pmf_comm_active(const pmf_ctx *ctx);
void pmf_comm_release(pmf_ctx *ctx);   // detach + free the statistics buffers (~pmf_ctx)
// hipStreamSynchronize for a context with a communicator: polls the stream, RCCL's asynchronous error state and
// a deadline (PMF_COMM_TIMEOUT_S, default 1800; 0 = wait for ever), so that a peer that died or never arrived
// ends in PMF_ECOMM on the surviving ranks instead of a hang.
int pmf_comm_wait_stream(pmf_ctx *ctx, hipStream_t stream, const char *what);
// what a half-sweep's finalize writes (the arrays of `side` the SCATTER_GATHER exchange all-gathers) and whether
// PMF_EXCHANGE_AUTO should pick that exchange for it (true where finalize is expensive: the Gaussian row solves)
struct PmfExchange {
    bool prefer_scatter = false;
    int n_arrays = 0;
    int arrays[6] = {0, 0, 0, 0, 0, 0};
};
// `which` = the statistics buffer (pmf_ctx::d_stats), `width` = its elements per row; accumulate / finalize get it
int pmf_comm_half_sweep(pmf_ctx *ctx, int side, int which, size_t width, bool chunked, const PmfExchange &ex,
                        const std::function<int(void *)> &accumulate, const std::function<int(void *)> &finalize);

// profiling brackets (the *_on forms time work on another stream than the context's)
void pmf_prof_begin(pmf_ctx *ctx, int kernel);
void pmf_prof_end(pmf_ctx *ctx);
void pmf_prof_begin_on(pmf_ctx *ctx, int kernel, hipStream_t stream);
void pmf_prof_end_on(pmf_ctx *ctx, hipStream_t stream);

struct PmfProfScope {
    pmf_ctx *ctx;
    PmfProfScope(pmf_ctx *c, int kernel) : ctx(c) { pmf_prof_begin(c, kernel); }
    ~PmfProfScope() { pmf_prof_end(ctx); }
};

static inline int pmf_lanes_per_row(int kpad) {
    int kv = kpad / PMF_VEC;
    int l = 1;
    while (l < kv) l <<= 1;
    return l;
}

// f(float()) or f(double()), by the context's dtype
template <typename F>
static inline auto pmf_with_dtype(const pmf_ctx *ctx, F &&f) {
    if (ctx->dtype == PMF_F64) return f(double());
    return f(float());
}

// f(std::integral_constant<int, L>()) for the power of two L in [MIN, 64] that n rounds up to (64 for n > 64):
// lanes per row, register tiles of K <= 64.  The instantiations are L = MIN, 2 MIN, ..., 64.
template <int MIN, typename F>
static inline auto pmf_with_pow2(int n, F &&f) {
    if (MIN == 64 || n <= MIN) return f(std::integral_constant<int, MIN>());
    return pmf_with_pow2<MIN < 64 ? 2 * MIN : 64>(n, f);
}

// f(std::integral_constant<int, MODE>()) for predict's mode: 0, PMF_PREDICT_BIAS or PMF_PREDICT_SCALE (checked by the caller)
template <typename F>
static inline auto pmf_with_predict_mode(int mode, F &&f) {
    if (mode == PMF_PREDICT_BIAS) return f(std::integral_constant<int, PMF_PREDICT_BIAS>());
    if (mode == PMF_PREDICT_SCALE) return f(std::integral_constant<int, PMF_PREDICT_SCALE>());
    return f(std::integral_constant<int, 0>());
}

// a FACTOR array or the ratings are about to change: the mean sums of the last factor sweeps no longer describe them
static inline void pmf_factor_written(pmf_ctx *ctx) { ctx->gauss_mdot_valid[0] = ctx->gauss_mdot_valid[1] = false; }

// Calls that read the ratings but have no weighted form refuse a context that holds weights: a silently unweighted fit
// is the worse failure.
#define PMF_REQUIRE_UNWEIGHTED(fn)                      \
    PMF_REQUIRE(!ctx->weighted, PMF_EINVAL,             \
                fn ": not available while the context holds rating weights (pmf_ctx_set_ratings_weighted)")

// every weights[k] is finite and > 0, or PMF_EINVAL naming the first that is not
static inline int pmf_check_weights(const double *weights, int64_t n, const char *fn) {
    for (int64_t k = 0; k < n; ++k)
        PMF_REQUIRE(weights[k] > 0.0 && weights[k] <= 1.7976931348623157e308, PMF_EINVAL,   // (false for a NaN as well)
                    "%s: weight %g at position %lld is not finite and > 0", fn, weights[k], (long long)k);
    return PMF_OK;
}

static inline bool pmf_has_bias(const pmf_ctx *ctx) { return ctx->arr[0][PMF_ARR_BIAS] && ctx->arr[1][PMF_ARR_BIAS]; }

static inline bool pmf_gauss_zeros_observed(const pmf_ctx *ctx) { return ctx->gauss_zeros == PMF_ZEROS_OBSERVED; }
// PMF_ZEROS_OBSERVED (pmf_ctx_set_gauss_zeros) at the Gaussian entry points.  _GAUSS_ZEROS_MISSING: the calls the mode does
// not cover refuse it (pmf_gauss_factor_accumulate / _finalize, pmf_gauss_bias_sweep / _accumulate / _finalize).  _ZERO_MODE_
// BIAS_FREE: the calls it covers refuse the bias model under it (pmf_gauss_factor_sweep, _fold_in, _elbo_terms with data).
#define PMF_REQUIRE_GAUSS_ZEROS_MISSING(fn)                         \
    PMF_REQUIRE(!pmf_gauss_zeros_observed(ctx), PMF_EINVAL,         \
                fn ": not available while the context counts unobserved cells as weighted zeros (pmf_ctx_set_gauss_zeros, PMF_ZEROS_OBSERVED)")
#define PMF_REQUIRE_ZERO_MODE_BIAS_FREE(fn)                                         \
    PMF_REQUIRE(!(pmf_gauss_zeros_observed(ctx) && pmf_has_bias(ctx)), PMF_EINVAL,  \
                fn ": the bias model is not available while the context counts unobserved cells as weighted zeros (pmf_ctx_set_gauss_zeros, PMF_ZEROS_OBSERVED)")
