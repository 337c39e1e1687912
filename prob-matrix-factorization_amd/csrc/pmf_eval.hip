// predict / evaluate / top-k kernels (rows a10, a11 of SURVEY.md section 8 and
// the "identical top-k" check of the north star).
#include <algorithm>
#include <vector>

#include "pmf_device.h"

template <typename T>
struct PredictParams {
    const int32_t *u;
    const int32_t *i;
    int64_t n;
    const T *fu;
    const T *fi;
    const T *bu;  // null when biases are not used
    const T *bi;
    const T *su;  // null unless the scalar factors of the extended Poisson model apply
    const T *si;
    int64_t n_users, n_items;
    int kpad;
    double offset;
};

// dot(FACTOR_user[u], FACTOR_item[i]) (+ biases) for one pair, computed by a
// lane group; ids outside the trained dimensions give 0 (hpf_cavi.py:220-229).
template <typename T, int LPR>
__device__ __forceinline__ double predict_pair(const PredictParams<T> &p, int64_t idx, int c) {
    const int u = p.u[idx], i = p.i[idx];
    const bool valid = u >= 0 && i >= 0 && u < p.n_users && i < p.n_items;
    const int koff = c * PMF_VEC;
    T d = (T)0;
    if (valid && koff < p.kpad) {
        Vec4<T> a = load4(p.fu + (int64_t)u * p.kpad + koff);
        Vec4<T> b = load4(p.fi + (int64_t)i * p.kpad + koff);
        d = a.v[0] * b.v[0];
        d = fma(a.v[1], b.v[1], d);
        d = fma(a.v[2], b.v[2], d);
        d = fma(a.v[3], b.v[3], d);
    }
    d = group_sum<LPR>(d);
    if (valid && p.su) d = p.su[u] * p.si[i] * d;
    if (valid && p.bu) d = p.bu[u] + p.bi[i] + d;
    return (valid ? (double)d : 0.0) + p.offset;
}

template <typename T, int LPR>
__global__ __launch_bounds__(256) void predict_kernel(PredictParams<T> p, double *out) {
    constexpr int G = 256 / LPR;
    const int c = threadIdx.x % LPR;
    const int64_t stride = (int64_t)gridDim.x * G;
    // all groups of a wavefront iterate the same number of times (DPP inside)
    const int64_t rounds = (p.n + stride - 1) / stride;
    int64_t idx = (int64_t)blockIdx.x * G + threadIdx.x / LPR;
    for (int64_t r = 0; r < rounds; ++r, idx += stride) {
        if (idx < p.n) {
            double v = predict_pair<T, LPR>(p, idx, c);
            if (c == 0) out[idx] = v;
        }
    }
}

// Fused validation monitor: per-block partial sums of squared error and of the
// per-label absolute error / count, combined in block order on the host
// (deterministic; metrics.py:6-10, :37-51).
template <typename T, int LPR>
__global__ __launch_bounds__(256) void eval_kernel(PredictParams<T> p, const double *y, const int32_t *label,
                                                   int n_labels, double *block_out) {
    constexpr int G = 256 / LPR;
    __shared__ double s_sse[G];
    __shared__ double s_abs[G][PMF_MAX_LABELS];
    __shared__ int s_cnt[G][PMF_MAX_LABELS];
    const int c = threadIdx.x % LPR;
    const int g = threadIdx.x / LPR;
    for (int t = threadIdx.x; t < G * PMF_MAX_LABELS; t += 256) {
        (&s_abs[0][0])[t] = 0.0;
        (&s_cnt[0][0])[t] = 0;
    }
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * G;
    const int64_t rounds = (p.n + stride - 1) / stride;
    int64_t idx = (int64_t)blockIdx.x * G + g;
    double sse = 0.0;
    for (int64_t r = 0; r < rounds; ++r, idx += stride) {
        if (idx < p.n) {
            double err = y[idx] - predict_pair<T, LPR>(p, idx, c);
            if (c == 0) {
                sse += err * err;
                int l = label[idx];
                s_abs[g][l] += fabs(err);
                s_cnt[g][l] += 1;
            }
        }
    }
    if (c == 0) s_sse[g] = sse;
    __syncthreads();
    double *dst = block_out + (int64_t)blockIdx.x * (1 + 2 * PMF_MAX_LABELS);
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int k = 0; k < G; ++k) s += s_sse[k];
        dst[0] = s;
    }
    if (threadIdx.x < n_labels) {
        double a = 0.0;
        long long n = 0;
        for (int k = 0; k < G; ++k) {
            a += s_abs[k][threadIdx.x];
            n += s_cnt[k][threadIdx.x];
        }
        dst[1 + threadIdx.x] = a;
        dst[1 + PMF_MAX_LABELS + threadIdx.x] = (double)n;
    }
}

// ---------------------------------------------------------------------------
// Posterior predictive variance of f = theta_u . beta_i under independent q(theta_u) = N(mu, Vu), q(beta_i) = N(mi, Vi)
// (no reference counterpart):   Var[f] = mu' Vi mu + mi' Vu mi + tr(Vu Vi).
// Both covariances are packed lower triangles (entry (r, c), c <= r, at r (r + 1) / 2 + c), so with w_p = 1 on the
// diagonal and 2 off it the three terms are ONE pass over p:
//     Var[f] = sum_p w_p ( Vi[p] mu[r] mu[c] + Vu[p] mi[r] mi[c] + Vu[p] Vi[p] ).
// ---------------------------------------------------------------------------
template <typename T>
struct VarParams {
    PredictParams<T> p;
    const T *cu;      // COV_user / COV_item, cov_stride elements per row
    const T *ci;
    int K;
    int kp;           // K (K + 1) / 2: the entries [kp, cov_stride) of a packed row are don't-care
    int cov_stride;
};

// row of packed index p: the r with r (r + 1) / 2 <= p < (r + 1) (r + 2) / 2.  8 p + 1 < 2^24 for every K <= 256, so
// the float argument is exact; the two corrections cover the rounding of the square root and of the halving.
__device__ __forceinline__ int packed_row(int p) {
    int r = (int)((sqrtf((float)(8 * p + 1)) - 1.0f) * 0.5f);
    if (r * (r + 1) / 2 > p) --r;
    if ((r + 1) * (r + 2) / 2 <= p) ++r;
    return r;
}

// lanes of a pair's group, from the 16-byte chunks of a packed row: four chunks per lane and trip at K <= 10 (4 lanes),
// a whole wavefront from K = 32
static inline int pmf_var_lanes(int cov_stride) { return (cov_stride / PMF_VEC + 3) / 4; }

// the two means of one factor index side by side: one LDS read per index of an entry
template <typename T>
struct alignas(2 * sizeof(T)) MeanPair {
    T u, i;
};

// the four entries p0 .. p0 + 3 of both packed rows (x of Vu, y of Vi) into the four partial sums.  MASK: the chunk
// reaches past kp -- those entries are dropped by index, whatever they hold (and never index the means).
template <typename T, bool MASK>
__device__ __forceinline__ void var_chunk(const Vec4<T> &x, const Vec4<T> &y, int p0, int kp, const MeanPair<T> *m, T *acc) {
    int r = packed_row(p0);
    int col = p0 - r * (r + 1) / 2;
#pragma unroll
    for (int j = 0; j < PMF_VEC; ++j) {
        const bool in = !MASK || p0 + j < kp;
        const MeanPair<T> a = m[in ? r : 0], b = m[in ? col : 0];
        T e = x.v[j] * y.v[j];
        e = fma(x.v[j], a.i * b.i, e);
        e = fma(y.v[j], a.u * b.u, e);
        if (MASK && !in) e = (T)0;
        acc[j] = fma(r == col ? (T)1 : (T)2, e, acc[j]);
        if (++col > r) {
            ++r;
            col = 0;
        }
    }
}

// Var[f] of pair `idx` by its group of L lanes (lane c of the group); every thread of the block calls it together
// (`live`: the group has a pair in this round).  The group's two mean rows go to its LDS area `means` (K rounded up to
// PMF_VEC pairs) once, where the pass reads the four means of every entry; each lane then streams every L-th
// 16-byte chunk of both packed rows, non-temporally (a row is touched once per pair), UNR chunks in flight, into one
// partial sum per chunk position.  Pairs outside the trained dimensions give 0: predict treats them as the point 0.
template <typename T, int L>
__device__ __forceinline__ double predict_var_pair(const VarParams<T> &q, int64_t idx, bool live, int c, MeanPair<T> *means) {
    constexpr int UNR = sizeof(T) == 4 ? 4 : 2;
    const int k4 = (q.K + PMF_VEC - 1) / PMF_VEC * PMF_VEC;
    int u = 0, i = 0;
    if (live) {
        u = q.p.u[idx];
        i = q.p.i[idx];
    }
    const bool valid = live && u >= 0 && i >= 0 && u < q.p.n_users && i < q.p.n_items;
    if (valid) {
        for (int k = c * PMF_VEC; k < k4; k += L * PMF_VEC) {
            const Vec4<T> a = load4(q.p.fu + (int64_t)u * q.p.kpad + k);
            const Vec4<T> b = load4(q.p.fi + (int64_t)i * q.p.kpad + k);
#pragma unroll
            for (int j = 0; j < PMF_VEC; ++j) means[k + j] = MeanPair<T>{a.v[j], b.v[j]};
        }
    }
    __syncthreads();
    T acc[PMF_VEC] = {(T)0, (T)0, (T)0, (T)0};
    if (valid) {
        const T *vu = q.cu + (int64_t)u * q.cov_stride;   // 64-bit: row * cov_stride passes 2^31 at 1M x K = 64
        const T *vi = q.ci + (int64_t)i * q.cov_stride;
        const int chunks = q.cov_stride / PMF_VEC;
        for (int ch0 = c; ch0 < chunks; ch0 += UNR * L) {
            Vec4<T> x[UNR], y[UNR];
#pragma unroll
            for (int t = 0; t < UNR; ++t) {
                const int ch = ch0 + t * L;
                x[t] = ch < chunks ? load4_nt(vu + ch * PMF_VEC) : zero4<T>();
                y[t] = ch < chunks ? load4_nt(vi + ch * PMF_VEC) : zero4<T>();
            }
#pragma unroll
            for (int t = 0; t < UNR; ++t) {
                const int p0 = (ch0 + t * L) * PMF_VEC;
                if (p0 + PMF_VEC <= q.kp) var_chunk<T, false>(x[t], y[t], p0, q.kp, means, acc);
                else var_chunk<T, true>(x[t], y[t], p0, q.kp, means, acc);
            }
        }
    }
    const T s = group_sum<L>((acc[0] + acc[1]) + (acc[2] + acc[3]));
    __syncthreads();   // the next round overwrites `means`
    return valid ? (double)s : 0.0;
}

template <typename T, int L>
__global__ __launch_bounds__(256) void predict_var_kernel(VarParams<T> q, double *out) {
    extern __shared__ __align__(16) double var_lds[];
    constexpr int G = 256 / L;
    const int c = threadIdx.x % L;
    const int g = threadIdx.x / L;
    MeanPair<T> *means = reinterpret_cast<MeanPair<T> *>(var_lds) + (size_t)g * ((q.K + PMF_VEC - 1) / PMF_VEC * PMF_VEC);
    const int64_t stride = (int64_t)gridDim.x * G;
    // every thread of the block iterates the same number of times (barriers and DPP inside)
    const int64_t rounds = (q.p.n + stride - 1) / stride;
    int64_t idx = (int64_t)blockIdx.x * G + g;
    for (int64_t r = 0; r < rounds; ++r, idx += stride) {
        const double v = predict_var_pair<T, L>(q, idx, idx < q.p.n, c, means);
        if (c == 0 && idx < q.p.n) out[idx] = v;
    }
}

// Fused form over the stored validation set: per-block partial sums of Var[f] and of the log predictive density term
//     -1/2 log(2 pi (sigma2 + v)) - e^2 / (2 (sigma2 + v)),    e = y - predict  (predict_pair with the lane-group width LP
// of predict_kernel / eval_kernel: the same bits), combined in block order on the host.  No atomics.
template <typename T, int L, int LP>
__global__ __launch_bounds__(256) void eval_var_kernel(VarParams<T> q, const double *y, double sigma2, double *block_out) {
    static_assert(LP <= L, "the predict groups tile the variance group");
    extern __shared__ __align__(16) double var_lds[];
    constexpr int G = 256 / L;
    __shared__ double s_part[G][2];
    const int c = threadIdx.x % L;
    const int g = threadIdx.x / L;
    MeanPair<T> *means = reinterpret_cast<MeanPair<T> *>(var_lds) + (size_t)g * ((q.K + PMF_VEC - 1) / PMF_VEC * PMF_VEC);
    const int64_t stride = (int64_t)gridDim.x * G;
    const int64_t rounds = (q.p.n + stride - 1) / stride;
    int64_t idx = (int64_t)blockIdx.x * G + g;
    double sum_v = 0.0, sum_ld = 0.0;
    for (int64_t r = 0; r < rounds; ++r, idx += stride) {
        const bool live = idx < q.p.n;
        const double v = predict_var_pair<T, L>(q, idx, live, c, means);
        if (live) {
            // every aligned LP lanes of the group form the same dot product
            const double err = y[idx] - predict_pair<T, LP>(q.p, idx, threadIdx.x % LP);
            if (c == 0) {
                const double d = sigma2 + v;
                sum_v += v;
                sum_ld += -0.5 * log(6.283185307179586 * d) - err * err / (2.0 * d);
            }
        }
    }
    if (c == 0) {
        s_part[g][0] = sum_v;
        s_part[g][1] = sum_ld;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        double s = 0.0;
        for (int k = 0; k < G; ++k) s += s_part[k][threadIdx.x];
        block_out[(int64_t)blockIdx.x * 2 + threadIdx.x] = s;
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
template <typename T>
static int fill_params(pmf_ctx *ctx, int use_bias, double offset, PredictParams<T> &p, const char *fn) {
    int rc;
    if ((rc = pmf_require_array(ctx, PMF_SIDE_USER, PMF_ARR_FACTOR, fn))) return rc;
    if ((rc = pmf_require_array(ctx, PMF_SIDE_ITEM, PMF_ARR_FACTOR, fn))) return rc;
    const bool scale = (use_bias & PMF_PREDICT_SCALE) != 0;
    use_bias &= PMF_PREDICT_BIAS;
    if (use_bias) {
        if ((rc = pmf_require_array(ctx, PMF_SIDE_USER, PMF_ARR_BIAS, fn))) return rc;
        if ((rc = pmf_require_array(ctx, PMF_SIDE_ITEM, PMF_ARR_BIAS, fn))) return rc;
    }
    if (scale) {
        if ((rc = pmf_require_array(ctx, PMF_SIDE_USER, PMF_ARR_SCALE, fn))) return rc;
        if ((rc = pmf_require_array(ctx, PMF_SIDE_ITEM, PMF_ARR_SCALE, fn))) return rc;
    }
    p.su = scale ? ctx->arr[PMF_SIDE_USER][PMF_ARR_SCALE].as<const T>() : nullptr;
    p.si = scale ? ctx->arr[PMF_SIDE_ITEM][PMF_ARR_SCALE].as<const T>() : nullptr;
    p.fu = ctx->arr[PMF_SIDE_USER][PMF_ARR_FACTOR].as<const T>();
    p.fi = ctx->arr[PMF_SIDE_ITEM][PMF_ARR_FACTOR].as<const T>();
    p.bu = use_bias ? ctx->arr[PMF_SIDE_USER][PMF_ARR_BIAS].as<const T>() : nullptr;
    p.bi = use_bias ? ctx->arr[PMF_SIDE_ITEM][PMF_ARR_BIAS].as<const T>() : nullptr;
    p.n_users = ctx->rows[0];
    p.n_items = ctx->rows[1];
    p.kpad = ctx->kpad;
    p.offset = offset;
    return PMF_OK;
}

// The pairs (u, i) in staging rounds: ids up, launch(d_u, d_i, cnt, d_out) timed as `kernel`, cnt values down.
template <typename Launch>
static int pair_rounds(pmf_ctx *ctx, int kernel, int64_t n, const int32_t *u, const int32_t *i, double *out, Launch &&launch) {
    const int64_t step = 4 << 20;  // pairs per staging round
    const size_t m = (size_t)std::min(n, step);
    PmfLayout lay;
    const auto u_at = lay.add<int32_t>(m), i_at = lay.add<int32_t>(m);
    const auto out_at = lay.add<double>(m);
    if (int rc = pmf_ensure_scratch(ctx, lay.bytes())) return rc;
    void *base = ctx->d_scratch.as();
    int32_t *d_u = u_at.at(base), *d_i = i_at.at(base);
    double *d_out = out_at.at(base);
    for (int64_t at = 0; at < n; at += step) {
        const int64_t cnt = std::min(step, n - at);
        PMF_HIP_CHECK(hipMemcpyAsync(d_u, u + at, (size_t)cnt * 4, hipMemcpyHostToDevice, ctx->stream));
        PMF_HIP_CHECK(hipMemcpyAsync(d_i, i + at, (size_t)cnt * 4, hipMemcpyHostToDevice, ctx->stream));
        {
            PmfProfScope prof(ctx, kernel);
            launch(d_u, d_i, cnt, d_out);
        }
        PMF_HIP_CHECK(hipGetLastError());
        PMF_HIP_CHECK(hipMemcpyAsync(out + at, d_out, (size_t)cnt * 8, hipMemcpyDeviceToHost, ctx->stream));
        PMF_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    return PMF_OK;
}

template <typename T>
static int run_predict(pmf_ctx *ctx, int64_t n, const int32_t *u, const int32_t *i, int use_bias,
                       double offset, double *out) {
    PredictParams<T> p;
    if (int rc = fill_params(ctx, use_bias, offset, p, "pmf_predict")) return rc;
    return pair_rounds(ctx, PMF_KERNEL_PREDICT, n, u, i, out, [&](const int32_t *d_u, const int32_t *d_i, int64_t cnt, double *d_out) {
        p.u = d_u;
        p.i = d_i;
        p.n = cnt;
        pmf_with_pow2<4>(pmf_lanes_per_row(ctx->kpad), [&](auto L) {
            const int grid = (int)std::min<int64_t>((p.n + 256 / L - 1) / (256 / L), 8192);
            hipLaunchKernelGGL((predict_kernel<T, L>), dim3(grid), dim3(256), 0, ctx->stream, p, d_out);
        });
    });
}

extern "C" int pmf_predict(pmf_ctx *ctx, int64_t n, const int32_t *user_ids, const int32_t *item_ids,
                           int use_bias, double offset, double *out) {
    PMF_REQUIRE(ctx != nullptr, PMF_EINVAL, "pmf_predict: null context");
    PMF_REQUIRE(n >= 0, PMF_EINVAL, "pmf_predict: negative n");
    if (n == 0) return PMF_OK;
    PMF_REQUIRE(user_ids && item_ids && out, PMF_EINVAL, "pmf_predict: null argument");
    PMF_HIP_CHECK(hipSetDevice(ctx->device));
    return pmf_with_dtype(ctx, [&](auto t) { return run_predict<decltype(t)>(ctx, n, user_ids, item_ids, use_bias, offset, out); });
}

extern "C" int pmf_eval_set(pmf_ctx *ctx, int64_t n, const int32_t *user_ids, const int32_t *item_ids,
                            const double *y_true, const int32_t *label_index, int n_labels) {
    PMF_REQUIRE(ctx != nullptr, PMF_EINVAL, "pmf_eval_set: null context");
    PMF_REQUIRE(n > 0 && user_ids && item_ids && y_true && label_index, PMF_EINVAL,
                "pmf_eval_set: empty or null input");
    PMF_REQUIRE(n_labels >= 1 && n_labels <= PMF_MAX_LABELS, PMF_ERANGE,
                "pmf_eval_set: n_labels=%d outside [1, %d]", n_labels, PMF_MAX_LABELS);
    for (int64_t k = 0; k < n; ++k)
        PMF_REQUIRE(label_index[k] >= 0 && label_index[k] < n_labels, PMF_ERANGE,
                    "pmf_eval_set: label index %d at position %lld outside [0, %d)", label_index[k],
                    (long long)k, n_labels);
    PMF_HIP_CHECK(hipSetDevice(ctx->device));
    PMF_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    ctx->eval = PmfEvalSet();   // the old set goes first; a failure below leaves the context without one
    PmfEvalSet ev;
    int rc;
    if ((rc = ev.d_u.alloc(ctx, (size_t)n * 4))) return rc;
    if ((rc = ev.d_i.alloc(ctx, (size_t)n * 4))) return rc;
    if ((rc = ev.d_y.alloc(ctx, (size_t)n * 8))) return rc;
    if ((rc = ev.d_label.alloc(ctx, (size_t)n * 4))) return rc;
    ev.n = n;
    ev.n_labels = n_labels;
    PMF_HIP_CHECK(hipMemcpy(ev.d_u.as(), user_ids, (size_t)n * 4, hipMemcpyHostToDevice));
    PMF_HIP_CHECK(hipMemcpy(ev.d_i.as(), item_ids, (size_t)n * 4, hipMemcpyHostToDevice));
    PMF_HIP_CHECK(hipMemcpy(ev.d_y.as(), y_true, (size_t)n * 8, hipMemcpyHostToDevice));
    PMF_HIP_CHECK(hipMemcpy(ev.d_label.as(), label_index, (size_t)n * 4, hipMemcpyHostToDevice));
    ctx->eval = std::move(ev);
    return PMF_OK;
}

template <typename T>
static int run_eval(pmf_ctx *ctx, int use_bias, double offset, double *sse, double *abs_l, int64_t *cnt_l) {
    PredictParams<T> p;
    int rc = fill_params(ctx, use_bias, offset, p, "pmf_eval_run");
    if (rc) return rc;
    const PmfEvalSet &ev = ctx->eval;
    p.u = ev.d_u.as<int32_t>();
    p.i = ev.d_i.as<int32_t>();
    p.n = ev.n;
    const int lpr = std::max(4, pmf_lanes_per_row(ctx->kpad));
    const int G = 256 / lpr;
    const int grid = (int)std::min<int64_t>((ev.n + G - 1) / G, 1024);
    const size_t rec = 1 + 2 * PMF_MAX_LABELS;
    const size_t bytes = (size_t)grid * rec * sizeof(double);
    if ((rc = pmf_ensure_scratch(ctx, bytes))) return rc;
    if ((rc = pmf_ensure_pinned(ctx, bytes))) return rc;
    double *block_out = ctx->d_scratch.as<double>();
    {
        PmfProfScope prof(ctx, PMF_KERNEL_EVAL);
        pmf_with_pow2<4>(lpr, [&](auto L) {
            hipLaunchKernelGGL((eval_kernel<T, L>), dim3(grid), dim3(256), 0, ctx->stream, p, ev.d_y.as<double>(), ev.d_label.as<int32_t>(), ev.n_labels,
                               block_out);
        });
    }
    PMF_HIP_CHECK(hipGetLastError());
    PMF_HIP_CHECK(hipMemcpyAsync(ctx->h_pinned.as(), block_out, bytes, hipMemcpyDeviceToHost, ctx->stream));
    PMF_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    const double *h = ctx->h_pinned.as<const double>();
    double s = 0.0;
    for (int l = 0; l < ev.n_labels; ++l) {
        abs_l[l] = 0.0;
        cnt_l[l] = 0;
    }
    for (int b = 0; b < grid; ++b) {
        const double *r = h + (size_t)b * rec;
        s += r[0];
        for (int l = 0; l < ev.n_labels; ++l) {
            abs_l[l] += r[1 + l];
            cnt_l[l] += (int64_t)r[1 + PMF_MAX_LABELS + l];
        }
    }
    *sse = s;
    return PMF_OK;
}

extern "C" int pmf_eval_run(pmf_ctx *ctx, int use_bias, double offset, double *sum_sq_err,
                            double *abs_err_per_label, int64_t *count_per_label) {
    PMF_REQUIRE(ctx != nullptr, PMF_EINVAL, "pmf_eval_run: null context");
    PMF_REQUIRE(sum_sq_err && abs_err_per_label && count_per_label, PMF_EINVAL, "pmf_eval_run: null argument");
    PMF_REQUIRE(ctx->eval.n > 0, PMF_EINVAL, "pmf_eval_run: no validation set (call pmf_eval_set)");
    PMF_HIP_CHECK(hipSetDevice(ctx->device));
    return pmf_with_dtype(ctx, [&](auto t) {
        return run_eval<decltype(t)>(ctx, use_bias, offset, sum_sq_err, abs_err_per_label, count_per_label);
    });
}

// ---- predictive variance ----------------------------------------------------------------------------------------
template <typename T>
static int fill_var_params(pmf_ctx *ctx, int use_bias, double offset, VarParams<T> &q, const char *fn) {
    int rc = fill_params(ctx, use_bias, offset, q.p, fn);
    if (rc) return rc;
    if ((rc = pmf_require_array(ctx, PMF_SIDE_USER, PMF_ARR_COV, fn))) return rc;
    if ((rc = pmf_require_array(ctx, PMF_SIDE_ITEM, PMF_ARR_COV, fn))) return rc;
    q.cu = ctx->arr[PMF_SIDE_USER][PMF_ARR_COV].as<const T>();
    q.ci = ctx->arr[PMF_SIDE_ITEM][PMF_ARR_COV].as<const T>();
    q.K = ctx->K;
    q.kp = ctx->kp;
    q.cov_stride = ctx->cov_stride;
    return PMF_OK;
}

// dynamic LDS of a block of 256 / lanes groups: two mean rows per group
template <typename T>
static size_t var_lds_bytes(const pmf_ctx *ctx, int lanes) {
    return (size_t)(256 / lanes) * 2 * ((ctx->K + PMF_VEC - 1) / PMF_VEC * PMF_VEC) * sizeof(T);
}

template <typename T>
static int run_predict_var(pmf_ctx *ctx, int64_t n, const int32_t *u, const int32_t *i, double *out) {
    VarParams<T> q;
    if (int rc = fill_var_params(ctx, 0, 0.0, q, "pmf_predict_var")) return rc;
    return pair_rounds(ctx, PMF_KERNEL_PREDICT_VAR, n, u, i, out, [&](const int32_t *d_u, const int32_t *d_i, int64_t cnt, double *d_out) {
        q.p.u = d_u;
        q.p.i = d_i;
        q.p.n = cnt;
        pmf_with_pow2<4>(pmf_var_lanes(ctx->cov_stride), [&](auto L) {
            const int grid = (int)std::min<int64_t>((cnt + 256 / L - 1) / (256 / L), 8192);
            hipLaunchKernelGGL((predict_var_kernel<T, L>), dim3(grid), dim3(256), var_lds_bytes<T>(ctx, L), ctx->stream, q, d_out);
        });
    });
}

extern "C" int pmf_predict_var(pmf_ctx *ctx, int64_t n, const int32_t *user_ids, const int32_t *item_ids, double *out_var) {
    PMF_REQUIRE(ctx != nullptr, PMF_EINVAL, "pmf_predict_var: null context");
    PMF_REQUIRE(n >= 0, PMF_EINVAL, "pmf_predict_var: negative n");
    if (n == 0) return PMF_OK;
    PMF_REQUIRE(user_ids && item_ids && out_var, PMF_EINVAL, "pmf_predict_var: null argument");
    PMF_HIP_CHECK(hipSetDevice(ctx->device));
    return pmf_with_dtype(ctx, [&](auto t) { return run_predict_var<decltype(t)>(ctx, n, user_ids, item_ids, out_var); });
}

template <typename T>
static int run_eval_var(pmf_ctx *ctx, int use_bias, double offset, double sigma2, double *sum_var, double *sum_ld) {
    VarParams<T> q;
    int rc = fill_var_params(ctx, use_bias, offset, q, "pmf_eval_run_var");
    if (rc) return rc;
    const PmfEvalSet &ev = ctx->eval;
    q.p.u = ev.d_u.as<int32_t>();
    q.p.i = ev.d_i.as<int32_t>();
    q.p.n = ev.n;
    const int lp = std::max(4, pmf_lanes_per_row(ctx->kpad));       // eval_kernel's lane groups
    const int lanes = std::max(lp, pmf_var_lanes(ctx->cov_stride));
    const int max_grid = 1024;
    if ((rc = pmf_ensure_scratch(ctx, (size_t)max_grid * 2 * sizeof(double)))) return rc;
    if ((rc = pmf_ensure_pinned(ctx, (size_t)max_grid * 2 * sizeof(double)))) return rc;
    double *block_out = ctx->d_scratch.as<double>();
    int grid = 0;
    {
        PmfProfScope prof(ctx, PMF_KERNEL_PREDICT_VAR);
        pmf_with_pow2<4>(lanes, [&](auto L) {
            grid = (int)std::min<int64_t>((ev.n + 256 / L - 1) / (256 / L), max_grid);
            pmf_with_pow2<4>(lp, [&](auto LP) {
                if constexpr (LP <= L)
                    hipLaunchKernelGGL((eval_var_kernel<T, L, LP>), dim3(grid), dim3(256), var_lds_bytes<T>(ctx, L), ctx->stream, q,
                                       ev.d_y.as<double>(), sigma2, block_out);
            });
        });
    }
    const size_t bytes = (size_t)grid * 2 * sizeof(double);
    PMF_HIP_CHECK(hipGetLastError());
    PMF_HIP_CHECK(hipMemcpyAsync(ctx->h_pinned.as(), block_out, bytes, hipMemcpyDeviceToHost, ctx->stream));
    PMF_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    const double *h = ctx->h_pinned.as<const double>();
    double sv = 0.0, sl = 0.0;
    for (int b = 0; b < grid; ++b) {
        sv += h[2 * b];
        sl += h[2 * b + 1];
    }
    *sum_var = sv;
    *sum_ld = sl;
    return PMF_OK;
}

extern "C" int pmf_eval_run_var(pmf_ctx *ctx, int use_bias, double offset, double sigma2, double *sum_var,
                                double *sum_log_density) {
    PMF_REQUIRE(ctx != nullptr, PMF_EINVAL, "pmf_eval_run_var: null context");
    PMF_REQUIRE(sum_var && sum_log_density, PMF_EINVAL, "pmf_eval_run_var: null argument");
    PMF_REQUIRE(sigma2 > 0.0, PMF_EINVAL, "pmf_eval_run_var: sigma2=%g must be positive", sigma2);
    PMF_REQUIRE(ctx->eval.n > 0, PMF_EINVAL, "pmf_eval_run_var: no validation set (call pmf_eval_set)");
    PMF_HIP_CHECK(hipSetDevice(ctx->device));
    return pmf_with_dtype(ctx, [&](auto t) {
        return run_eval_var<decltype(t)>(ctx, use_bias, offset, sigma2, sum_var, sum_log_density);
    });
}
