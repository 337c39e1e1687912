// Logistic matrix factorisation on the Gaussian path: the refresh of the Jaakkola-Jordan
// parameter xi_j of every rating of one side's stream, which turns the Bernoulli-logit likelihood into the weighted
// Gaussian one pmf_gauss_factor_sweep already fits (pmf_ctx_set_ratings_weighted), and the read-back of a side's stream.
#include <algorithm>
#include <vector>

#include "pmf_device.h"

// lambda(xi) = tanh(xi / 2) / (4 xi), in double.  Below kLogitSeries the quotient is replaced by its series
// 1/8 - xi^2/96 + xi^4/960 (next term 17 xi^6 / 161280: below 1e-22 relative at the switch), which also covers xi = 0.
#define PMF_LOGIT_SERIES_BELOW 1e-3
__host__ __device__ static inline double pmf_logit_lambda(double xi) {
    if (xi < PMF_LOGIT_SERIES_BELOW) {
        const double x2 = xi * xi;
        return 0.125 - x2 * (1.0 / 96.0) + x2 * x2 * (1.0 / 960.0);
    }
    return tanh(0.5 * xi) / (4.0 * xi);
}

template <typename T>
struct LogitParams {
    const PmfTask *tasks;
    int64_t n_tasks;
    const int32_t *other;   // the side's stream: ids on the opposite side, ratings and weights (both rewritten)
    T *val;
    T *wgt;
    const T *fr, *fo;       // FACTOR of the side / of the opposite side
    const T *cr, *co;       // COV likewise, cov_stride elements per row
    int kpad;
    int kp;                 // K (K + 1) / 2: the entries [kp, cov_stride) of a packed row are don't-care
    int cov_stride;
    double *block_out;      // [gridDim.x] partial sums of the data term
};

// row of packed index p (predict_var's rule, pmf_eval.hip): 8 p + 1 < 2^24 for every K <= 256
__device__ __forceinline__ int logit_packed_row(int p) {
    int r = (int)((sqrtf((float)(8 * p + 1)) - 1.0f) * 0.5f);
    if (r * (r + 1) / 2 > p) --r;
    if ((r + 1) * (r + 2) / 2 <= p) ++r;
    return r;
}

__device__ __forceinline__ void logit_lds_fence() {
    // a lane group never spans wavefronts and the LDS operations of one wavefront execute in order: this only stops the
    // compiler from moving LDS accesses across the point
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// The four entries p0 .. p0 + 3 of the row's own second moment, weighted for the packed sum:
//     s[j] = w_p (V_r[p] + m_r[r] m_r[c]),   w_p = 1 on the diagonal, 2 off it;   0 past kp, whatever the row holds there.
template <typename T>
__device__ __forceinline__ Vec4<T> logit_own_chunk(const Vec4<T> &x, int p0, int kp, const T *mr) {
    int r = logit_packed_row(p0);
    int col = p0 - r * (r + 1) / 2;
    Vec4<T> s;
#pragma unroll
    for (int j = 0; j < PMF_VEC; ++j) {
        const bool in = p0 + j < kp;
        const T e = fma(mr[in ? r : 0], mr[in ? col : 0], x.v[j]);
        s.v[j] = in ? (r == col ? e : (T)2 * e) : (T)0;
        if (++col > r) {
            ++r;
            col = 0;
        }
    }
    return s;
}

// acc[j] += s[j] (V_o[p] + m_o[r] m_o[c]) for the same four entries: one fma for the other side's second moment, one
// for the product and the sum.
template <typename T>
__device__ __forceinline__ void logit_chunk(const Vec4<T> &s, const Vec4<T> &y, int p0, int kp, const T *mo, T *acc) {
    int r = logit_packed_row(p0);
    int col = p0 - r * (r + 1) / 2;
#pragma unroll
    for (int j = 0; j < PMF_VEC; ++j) {
        const bool in = p0 + j < kp;
        T e = fma(mo[in ? r : 0], mo[in ? col : 0], y.v[j]);
        if (!in) e = (T)0;
        acc[j] = fma(s.v[j], e, acc[j]);
        if (++col > r) {
            ++r;
            col = 0;
        }
    }
}

// One lane group of L lanes per task of the side's Gaussian work list (a whole row, or one cut of a split row: only
// values change, so the cuts need no combine).  Per task the group puts the row's mean and -- OWN_LDS -- its weighted
// second moment S_r into its LDS area once; otherwise every rating re-forms S_r from the row's global COV, which the
// caches hold after the first.  Per rating the other side's mean goes to LDS and every lane streams each L-th 16-byte
// chunk of the other side's packed covariance, non-temporally, UNR chunks in flight, into one partial sum per chunk
// position:   E[s^2] = < S_r, S_o > = sum_p s_r[p] (V_o[p] + m_o[r] m_o[c]),   in the context dtype.
// Lane n % L keeps rating n's E[s^2] and m_r . m_o; after L ratings (or at the task's end) every lane finishes ITS rating
// in double -- xi, lambda, c, y, the data term -- so the transcendental work is spread over the group and the stores are
// coalesced.  The label is the sign of the stored rating.  Data term: per thread, then per block in thread order.
// BLOCK threads per block: 256, or 128 at L = 64 where four groups' areas do not fit but two do (fp64 at K = 64).
template <typename T, int L, bool OWN_LDS, int BLOCK>
__global__ __launch_bounds__(BLOCK) void logit_refresh_kernel(LogitParams<T> q) {
    static_assert(OWN_LDS ? (BLOCK == 256 || L == 64) : (L == 64 && BLOCK == 256), "the forms the host launches");
    extern __shared__ __align__(16) double logit_lds[];
    __shared__ double s_part[BLOCK];
    constexpr int G = BLOCK / L;
    constexpr int UNR = sizeof(T) == 4 ? 4 : 2;
    const int c = threadIdx.x % L;
    const int g = threadIdx.x / L;
    const int chunks = q.cov_stride / PMF_VEC;
    T *mo = reinterpret_cast<T *>(logit_lds) + (size_t)g * (2 * q.kpad + (OWN_LDS ? q.cov_stride : 0));
    T *mr = mo + q.kpad;
    T *own = mr + q.kpad;
    double d_sum = 0.0;
    for (int64_t t = (int64_t)blockIdx.x * G + g; t < q.n_tasks; t += (int64_t)gridDim.x * G) {
        const PmfTask task = q.tasks[t];
        const T *vr = q.cr + (int64_t)task.row * q.cov_stride;   // 64-bit: row * cov_stride passes 2^31 at 1M x K = 64
        logit_lds_fence();   // the previous task's reads of the area are done
        for (int k = c * PMF_VEC; k < q.kpad; k += L * PMF_VEC) {
            const Vec4<T> a = load4(q.fr + (int64_t)task.row * q.kpad + k);
#pragma unroll
            for (int j = 0; j < PMF_VEC; ++j) mr[k + j] = a.v[j];
        }
        logit_lds_fence();
        if (OWN_LDS) {
            for (int ch = c; ch < chunks; ch += L) {
                const Vec4<T> s = logit_own_chunk(load4(vr + ch * PMF_VEC), ch * PMF_VEC, q.kp, mr);
#pragma unroll
                for (int j = 0; j < PMF_VEC; ++j) own[ch * PMF_VEC + j] = s.v[j];
            }
            logit_lds_fence();
        }
        T my_e = (T)0, my_dot = (T)0;
        for (int n0 = 0; n0 < task.len; n0 += L) {
            const int cnt = min(L, task.len - n0);
            for (int n = 0; n < cnt; ++n) {
                const int32_t o = q.other[task.start + n0 + n];
                const T *vo = q.co + (int64_t)o * q.cov_stride;
                T dot = (T)0;
                for (int k = c * PMF_VEC; k < q.kpad; k += L * PMF_VEC) {
                    const Vec4<T> a = load4(q.fo + (int64_t)o * q.kpad + k);
#pragma unroll
                    for (int j = 0; j < PMF_VEC; ++j) {
                        mo[k + j] = a.v[j];
                        dot = fma(a.v[j], mr[k + j], dot);
                    }
                }
                logit_lds_fence();
                T acc[PMF_VEC] = {(T)0, (T)0, (T)0, (T)0};
                for (int ch0 = c; ch0 < chunks; ch0 += UNR * L) {
                    Vec4<T> y[UNR];
#pragma unroll
                    for (int u = 0; u < UNR; ++u) {
                        const int ch = ch0 + u * L;
                        y[u] = ch < chunks ? load4_nt(vo + ch * PMF_VEC) : zero4<T>();
                    }
#pragma unroll
                    for (int u = 0; u < UNR; ++u) {
                        const int ch = ch0 + u * L;
                        if (ch < chunks) {
                            const Vec4<T> s = OWN_LDS ? load4(own + ch * PMF_VEC)
                                                      : logit_own_chunk(load4(vr + ch * PMF_VEC), ch * PMF_VEC, q.kp, mr);
                            logit_chunk(s, y[u], ch * PMF_VEC, q.kp, mo, acc);
                        }
                    }
                }
                const T e = group_sum<L>((acc[0] + acc[1]) + (acc[2] + acc[3]));
                dot = group_sum<L>(dot);
                if (c == n) {
                    my_e = e;
                    my_dot = dot;
                }
                logit_lds_fence();   // the next rating overwrites `mo`
            }
            if (c < cnt) {
                const int64_t j = task.start + n0 + c;
                const double half = q.val[j] > (T)0 ? 0.5 : -0.5;   // x_j - 1/2
                const double xi = sqrt(fmax((double)my_e, 0.0));
                const double cj = 2.0 * pmf_logit_lambda(xi);
                q.wgt[j] = (T)cj;
                q.val[j] = (T)(half / cj);
                d_sum += -log1p(exp(-xi)) - 0.5 * xi + half * (double)my_dot;
            }
        }
    }
    s_part[threadIdx.x] = d_sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int k = 0; k < BLOCK; ++k) s += s_part[k];
        q.block_out[blockIdx.x] = s;
    }
}

// the block sums in block order: thread k adds every 256th from k, thread 0 the 256 results in thread order
__global__ __launch_bounds__(256) void logit_total_kernel(const double *block_out, int n, double *out) {
    __shared__ double s_part[256];
    double s = 0.0;
    for (int k = threadIdx.x; k < n; k += 256) s += block_out[k];
    s_part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = 0.0;
        for (int k = 0; k < 256; ++k) total += s_part[k];
        *out = total;
    }
}

// C_r again from the refreshed weights: in double in the row's rating order, rounded once (pmf_ctx_set_ratings_weighted's
// rule); 0 for a row without ratings
template <typename T>
__global__ __launch_bounds__(256) void logit_wsum_kernel(const int64_t *ptr, const T *wgt, int64_t rows, T *wsum) {
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    double s = 0.0;
    for (int64_t k = ptr[r]; k < ptr[r + 1]; ++k) s += (double)wgt[k];
    wsum[r] = (T)s;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static inline int logit_lanes(int cov_stride) { return (cov_stride / PMF_VEC + 3) / 4; }   // pmf_var_lanes' rule

// dynamic LDS of a block of `groups` lane groups: two mean rows per group and, `own`, the row's weighted second moment
static size_t logit_lds_bytes(const pmf_ctx *ctx, int groups, bool own) {
    return (size_t)groups * (size_t)(2 * ctx->kpad + (own ? ctx->cov_stride : 0)) * ctx->elem;
}
// the row's own second moment stays in LDS while a block's areas fit this (with the kernel's 2 KB of static LDS: 62 KB
// of the 64 KB a workgroup may address; two blocks per CU at the limit)
static const size_t kLogitOwnLdsMax = 60 * 1024;

template <typename T, int L, bool OWN, int BLOCK>
static int logit_launch(pmf_ctx *ctx, const LogitParams<T> &q, int max_grid, int *grid) {
    const int G = BLOCK / L;
    *grid = (int)std::min<int64_t>((q.n_tasks + G - 1) / G, max_grid);
    const size_t smem = logit_lds_bytes(ctx, G, OWN);
    if (int rc = pmf_allow_dynamic_lds((const void *)logit_refresh_kernel<T, L, OWN, BLOCK>, smem)) return rc;
    hipLaunchKernelGGL((logit_refresh_kernel<T, L, OWN, BLOCK>), dim3(*grid), dim3(BLOCK), smem, ctx->stream, q);
    return PMF_OK;
}

// The form that serves the context: the row's own second moment in LDS with 256 threads per block where four groups'
// areas fit (every L < 64 does: at most 128 chunks per row), with 128 threads at L = 64 where two fit, else the generic
// form (L = 64 only).
template <typename T>
static int logit_launch_refresh(pmf_ctx *ctx, const LogitParams<T> &q, int max_grid, int *grid) {
    int rc = PMF_OK;
    pmf_with_pow2<4>(logit_lanes(ctx->cov_stride), [&](auto L) {
        if (logit_lds_bytes(ctx, 256 / L, true) <= kLogitOwnLdsMax) {
            rc = logit_launch<T, L, true, 256>(ctx, q, max_grid, grid);
        } else if constexpr (L == 64) {
            if (logit_lds_bytes(ctx, 2, true) <= kLogitOwnLdsMax) rc = logit_launch<T, 64, true, 128>(ctx, q, max_grid, grid);
            else rc = logit_launch<T, 64, false, 256>(ctx, q, max_grid, grid);
        } else {
            pmf_set_error("pmf_gauss_logit_refresh: %d lanes per task and no room in LDS (internal error)", (int)L);
            rc = PMF_EINVAL;
        }
    });
    return rc;
}

template <typename T>
static int run_logit_refresh(pmf_ctx *ctx, int side, double *data_term) {
    const int other = 1 - side;
    PmfSideIndex &ix = ctx->index[side];
    const PmfTaskView tv = pmf_task_view(ctx, side, ix.gauss_tasks, false);
    LogitParams<T> q;
    q.tasks = tv.d_tasks;
    q.n_tasks = tv.n_tasks;
    q.other = ix.d_other.as<const int32_t>();
    q.val = ix.d_val.as<T>();
    q.wgt = ix.d_wgt.as<T>();
    q.fr = ctx->arr[side][PMF_ARR_FACTOR].as<const T>();
    q.fo = ctx->arr[other][PMF_ARR_FACTOR].as<const T>();
    q.cr = ctx->arr[side][PMF_ARR_COV].as<const T>();
    q.co = ctx->arr[other][PMF_ARR_COV].as<const T>();
    q.kpad = ctx->kpad;
    q.kp = ctx->kp;
    q.cov_stride = ctx->cov_stride;
    int rc = PMF_OK, grid = 0;
    const int max_grid = 4096;
    if ((rc = pmf_ensure_scratch(ctx, (size_t)(max_grid + 1) * sizeof(double)))) return rc;
    if (data_term && (rc = pmf_ensure_pinned(ctx, sizeof(double)))) return rc;
    q.block_out = ctx->d_scratch.as<double>();
    double *d_total = q.block_out + max_grid;
    {
        PmfProfScope prof(ctx, PMF_KERNEL_PREDICT_VAR);
        if ((rc = logit_launch_refresh<T>(ctx, q, max_grid, &grid))) return rc;   // (nothing has been queued)
        // from here on the stream's values change: the factor sweeps' mean sums no longer describe the ratings, and the
        // host copy of the weight sums is stale
        pmf_factor_written(ctx);
        ix.wsum_refreshed = true;
        const int64_t rows = ctx->rows[side];
        hipLaunchKernelGGL((logit_wsum_kernel<T>), dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, ctx->stream,
                           ix.d_ptr.as<const int64_t>(), ix.d_wgt.as<const T>(), rows, ix.d_wsum.as<T>());
        if (data_term) hipLaunchKernelGGL(logit_total_kernel, dim3(1), dim3(256), 0, ctx->stream, q.block_out, grid, d_total);
    }
    PMF_HIP_CHECK(hipGetLastError());
    if (data_term) {
        PMF_HIP_CHECK(hipMemcpyAsync(ctx->h_pinned.as(), d_total, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        PMF_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        *data_term = *ctx->h_pinned.as<const double>();
    }
    return PMF_OK;
}

extern "C" int pmf_gauss_logit_refresh(pmf_ctx *ctx, int side, double *data_term) {
    const char *fn = "pmf_gauss_logit_refresh";
    PMF_SIDE_ENTRY("pmf_gauss_logit_refresh");
    PMF_REQUIRE(ctx->comm == nullptr, PMF_EINVAL, "%s: not available on a context with a communicator", fn);
    PMF_REQUIRE_GAUSS_ZEROS_MISSING("pmf_gauss_logit_refresh");
    PMF_REQUIRE(ctx->index[side].d_ptr && ctx->nnz > 0, PMF_EINVAL, "%s: ratings have not been set", fn);
    PMF_REQUIRE(ctx->weighted, PMF_EINVAL,
                "%s: the context holds no rating weights (load the ratings with pmf_ctx_set_ratings_weighted)", fn);
    PMF_REQUIRE(!pmf_has_bias(ctx), PMF_EINVAL, "%s: the logistic model is bias-free, the context holds BIAS arrays", fn);
    for (int s = 0; s < 2; ++s) {
        if (int rc = pmf_require_array(ctx, s, PMF_ARR_FACTOR, fn)) return rc;
        if (int rc = pmf_require_array(ctx, s, PMF_ARR_COV, fn)) return rc;
    }
    return pmf_with_dtype(ctx, [&](auto t) { return run_logit_refresh<decltype(t)>(ctx, side, data_term); });
}

template <typename T>
static int download_as_double(pmf_ctx *ctx, const PmfBuf &src, int64_t n, double *out) {
    if (!out || n == 0) return PMF_OK;
    std::vector<T> host((size_t)n);
    PMF_HIP_CHECK(hipMemcpy(host.data(), src.as(), (size_t)n * sizeof(T), hipMemcpyDeviceToHost));
    for (int64_t k = 0; k < n; ++k) out[k] = (double)host[(size_t)k];
    return PMF_OK;
}

static int side_ratings_impl(pmf_ctx *ctx, int side, int64_t *row_ptr, int32_t *other_ids, double *ratings, double *weights) {
    const char *fn = "pmf_ctx_side_ratings";
    PMF_SIDE_ENTRY("pmf_ctx_side_ratings");
    const PmfSideIndex &ix = ctx->index[side];
    PMF_REQUIRE(ix.d_ptr, PMF_EINVAL, "%s: ratings have not been set", fn);
    PMF_REQUIRE(!weights || ctx->weighted, PMF_EINVAL, "%s: the context holds no rating weights", fn);
    PMF_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (row_ptr) std::copy(ix.h_ptr.begin(), ix.h_ptr.end(), row_ptr);
    if (other_ids && ctx->nnz)
        PMF_HIP_CHECK(hipMemcpy(other_ids, ix.d_other.as(), (size_t)ctx->nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
    return pmf_with_dtype(ctx, [&](auto t) {
        if (int rc = download_as_double<decltype(t)>(ctx, ix.d_val, ctx->nnz, ratings)) return rc;
        return download_as_double<decltype(t)>(ctx, ix.d_wgt, ctx->nnz, weights);
    });
}

extern "C" int pmf_ctx_side_ratings(pmf_ctx *ctx, int side, int64_t *row_ptr, int32_t *other_ids, double *ratings,
                                    double *weights) {
    return pmf_no_throw("pmf_ctx_side_ratings", [&] { return side_ratings_impl(ctx, side, row_ptr, other_ids, ratings, weights); });
}
