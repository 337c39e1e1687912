// Poisson MF / HPF half-sweep kernels (rows a5, a6, a7 of SURVEY.md section 8).
//
// Work decomposition: a *lane group* of LPR = pow2(Kpad/4) lanes owns one task
// (a run of at most PMF_GAMMA_CHUNK ratings of one row); lane c of the group
// owns factor elements [4c, 4c+4) of every K-vector it touches, so one gathered
// factor row is one 16-byte access per lane and a wavefront gathers 64/LPR rows
// per instruction (K = 64 fp32: 4 rows x 256 B = one full 1-KiB wave access).
// The K-length dot product is a 4-FMA partial per lane + a DPP reduction inside
// the group; shape/rate sums live in registers for the whole task, so every
// rating costs exactly one index, one value and one gathered row of HBM traffic.
// No atomics: rows that exceed one chunk write per-chunk partial sums that a
// second kernel adds in chunk order, so results are bitwise reproducible.
#include <algorithm>
#include <new>

#include "pmf_device.h"

template <typename T>
struct GammaParams {
    const PmfTask *tasks;
    int64_t n_tasks;
    const PmfSplitRow *split;
    const int32_t *other;
    const T *val;
    T *factor_self;
    const T *factor_other;
    T *shape;
    T *rate;
    T *prior_rate_vec;  // E_xi / E_eta (HPF) or null
    T *hyper_rate;      // gamma_b_xi / gamma_b_eta (HPF) or null
    // extended model (EXT): per-row scalar factors phi / psi
    const T *scale_other;
    T *scale_self;
    T *scale_shape;
    T *scale_rate;
    int pw;             // partial slot width: 2*kpad (+ PMF_VEC carrying sum x when EXT)
    T *partial;         // [n_slots][pw]
    T *stats;           // [rows][2][kpad], STATS mode only
    const T *colsum;    // [kpad] column sums of the other side's expected factors (PMF_ZEROS_OBSERVED: every row's rate sum), or null
    T shape_prior, rate_prior, hyper_shape, hyper_rate_prior;
    int hierarchical;
    int K, kpad;
    int64_t row0;       // first row of a finalize-from-stats launch
    int64_t rows;       // one past its last row
};

// shape = prior + sum, rate = prior_rate + sum, E = shape / rate, plus the
// xi / eta update (hpf_cavi.py:155-159) when hierarchical.
template <typename T, int LPR, bool EXT>
__device__ __forceinline__ void gamma_finalize_row(const GammaParams<T> &p, int row, int c, bool active,
                                                   const Vec4<T> &sum_a, const Vec4<T> &sum_b, T xsum, bool empty) {
    const int koff = c * PMF_VEC;
    const T rp = p.hierarchical ? p.prior_rate_vec[row] : p.rate_prior;
    Vec4<T> sh, rt, ex;
    // unlisted cells counted as zeros: every row's rate sum is the other side's column sum (the same for all lanes of the launch)
    Vec4<T> rsum = sum_b;
    if (!EXT && p.colsum && active) rsum = load4(p.colsum + koff);
    T esum = (T)0;
#pragma unroll
    for (int e = 0; e < PMF_VEC; ++e) {
        const bool ok = active && (koff + e) < p.K;
        T s = p.shape_prior + sum_a.v[e];
        T r = rp + rsum.v[e];
        T x = s / r;
        sh.v[e] = ok ? s : (T)0;
        rt.v[e] = ok ? r : (T)0;
        ex.v[e] = ok ? x : (T)0;
        esum += EXT ? ex.v[e] * sum_b.v[e] : ex.v[e];
    }
    if (active) {
        const int64_t at = (int64_t)row * p.kpad + koff;
        store4(p.shape + at, sh);
        store4(p.rate + at, rt);
        if (!(EXT && empty)) store4(p.factor_self + at, ex);
    }
    if (EXT) {
        // phi / psi: shape a0 + sum x, rate b0 + sum_j s_j (other_j . FACTOR_new[row]) = b0 + FACTOR_new . sum_b
        esum = group_sum<LPR>(esum);
        if (c == 0) {
            const T ss = p.shape_prior + xsum;
            const T sr = p.rate_prior + (empty ? (T)0 : esum);
            p.scale_shape[row] = ss;
            p.scale_rate[row] = sr;
            if (!empty) p.scale_self[row] = ss / sr;
        }
    } else if (p.hierarchical) {
        esum = group_sum<LPR>(esum);
        if (c == 0) {
            T hr = p.hyper_rate_prior + esum;
            p.hyper_rate[row] = hr;
            p.prior_rate_vec[row] = p.hyper_shape / hr;
        }
    }
}

template <typename T, int LPR, bool STATS, bool EXT>
__global__ __launch_bounds__(256) void gamma_sweep_kernel(GammaParams<T> p) {
    constexpr int G = 256 / LPR;
    constexpr int UN = LPR < 4 ? LPR : 4;
    const int c = threadIdx.x % LPR;
    const int64_t task_id = (int64_t)blockIdx.x * G + threadIdx.x / LPR;
    if (task_id >= p.n_tasks) return;
    const PmfTask t = p.tasks[task_id];
    const int koff = c * PMF_VEC;
    const bool active = koff < p.kpad;
    const int kpad = p.kpad;

    Vec4<T> self = active ? load4(p.factor_self + (int64_t)t.row * kpad + koff) : zero4<T>();
    Vec4<T> acc_a = zero4<T>(), acc_b = zero4<T>();
    T xsum = (T)0;
    const int32_t *col = p.other + t.start;
    const T *val = p.val + t.start;

    for (int base = 0; base < t.len; base += LPR) {
        const int n = min(LPR, t.len - base);
        int my_o = 0;
        T my_x = (T)0;
        if (c < n) {
            my_o = col[base + c];
            my_x = val[base + c];
        }
        for (int tt = 0; tt < n; tt += UN) {
            int o[UN];
            T xv[UN], sv[UN];
            Vec4<T> b[UN];
#pragma unroll
            for (int q = 0; q < UN; ++q) {
                o[q] = __shfl(my_o, tt + q, LPR);
                xv[q] = __shfl(my_x, tt + q, LPR);
            }
#pragma unroll
            for (int q = 0; q < UN; ++q) {
                b[q] = active ? load4(p.factor_other + (int64_t)o[q] * kpad + koff) : zero4<T>();
                sv[q] = EXT ? p.scale_other[o[q]] : (T)1;
            }
#pragma unroll
            for (int q = 0; q < UN; ++q) {
                if (tt + q < n) {
                    T d = b[q].v[0] * self.v[0];
                    d = fma(b[q].v[1], self.v[1], d);
                    d = fma(b[q].v[2], self.v[2], d);
                    d = fma(b[q].v[3], self.v[3], d);
                    d = group_sum<LPR>(d);
                    if (!EXT) d = vmax(d, (T)PMF_RATE_FLOOR);
                    const T w = xv[q] / d;
                    if (EXT) xsum += xv[q];
#pragma unroll
                    for (int e = 0; e < PMF_VEC; ++e) {
                        acc_a.v[e] += (w * b[q].v[e]) * self.v[e];
                        acc_b.v[e] += EXT ? b[q].v[e] * sv[q] : b[q].v[e];
                    }
                }
            }
        }
    }

    if (t.slot >= 0) {
        T *slot = p.partial + (int64_t)t.slot * p.pw;
        if (active) {
            store4(slot + koff, acc_a);
            store4(slot + kpad + koff, acc_b);
        }
        if (EXT && c == 0) slot[2 * kpad] = xsum;
    } else if (STATS) {
        if (active) {
            T *dst = p.stats + (int64_t)t.row * 2 * kpad + koff;
            store4(dst, acc_a);
            store4(dst + kpad, acc_b);
        }
    } else {
        gamma_finalize_row<T, LPR, EXT>(p, t.row, c, active, acc_a, acc_b, xsum, t.len == 0);
    }
}

// Gather ceiling of this access shape (profiling aid, pmf_prof_gather_ceiling): the sweep kernel's
// memory side only -- the same tasks, the same coalesced index / rating loads, the same 16-byte-per-lane
// row gathers with UN in flight -- with the arithmetic reduced to one add per loaded value and no row
// output.  Its time is what the L2 / Infinity Cache / HBM deliver for this gather pattern; the real
// kernel cannot be faster.
template <typename T, int LPR>
__global__ __launch_bounds__(256) void gamma_gather_probe_kernel(GammaParams<T> p, T *sink) {
    constexpr int G = 256 / LPR;
    constexpr int UN = LPR < 4 ? LPR : 4;
    const int c = threadIdx.x % LPR;
    const int64_t task_id = (int64_t)blockIdx.x * G + threadIdx.x / LPR;
    if (task_id >= p.n_tasks) return;
    const PmfTask t = p.tasks[task_id];
    const int koff = c * PMF_VEC;
    const bool active = koff < p.kpad;
    const int kpad = p.kpad;
    Vec4<T> acc = active ? load4(p.factor_self + (int64_t)t.row * kpad + koff) : zero4<T>();
    const int32_t *col = p.other + t.start;
    const T *val = p.val + t.start;
    for (int base = 0; base < t.len; base += LPR) {
        const int n = min(LPR, t.len - base);
        int my_o = 0;
        T my_x = (T)0;
        if (c < n) {
            my_o = col[base + c];
            my_x = val[base + c];
        }
        acc.v[0] += my_x;
        for (int tt = 0; tt < n; tt += UN) {
            int o[UN];
            Vec4<T> b[UN];
#pragma unroll
            for (int q = 0; q < UN; ++q) o[q] = __shfl(my_o, tt + q, LPR);
#pragma unroll
            for (int q = 0; q < UN; ++q) b[q] = active ? load4(p.factor_other + (int64_t)o[q] * kpad + koff) : zero4<T>();
#pragma unroll
            for (int q = 0; q < UN; ++q)
                if (tt + q < n) {
#pragma unroll
                    for (int e = 0; e < PMF_VEC; ++e) acc.v[e] += b[q].v[e];
                }
        }
    }
    // never true for finite data; keeps every load alive without an output stream
    if (acc.v[0] + acc.v[1] + acc.v[2] + acc.v[3] == (T)-1.2345678e30) sink[0] = acc.v[0];
}

// One block per split row: group g adds slots g, g+G, ... in order, the G
// group sums are then added in group order by group 0 (fixed order => bitwise
// reproducible), which finalises the row (or writes its raw sums in STATS mode).
template <typename T, int LPR, bool STATS, bool EXT>
__global__ __launch_bounds__(256) void gamma_split_kernel(GammaParams<T> p) {
    constexpr int G = 256 / LPR;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    T *smem = reinterpret_cast<T *>(smem_raw);  // [G][2][kpad]
    const PmfSplitRow sr = p.split[blockIdx.x];
    const int c = threadIdx.x % LPR;
    const int g = threadIdx.x / LPR;
    const int koff = c * PMF_VEC;
    const int kpad = p.kpad;
    const bool active = koff < kpad;
    Vec4<T> sa = zero4<T>(), sb = zero4<T>();
    T xsum = (T)0;
    if (EXT && threadIdx.x == 0)  // G*2*kpad sums are staged in LDS; sum x is tiny: one lane adds it in order
        for (int s = 0; s < sr.n_slots; ++s) xsum += p.partial[(int64_t)(sr.first_slot + s) * p.pw + 2 * kpad];
    if (active) {
        for (int s = g; s < sr.n_slots; s += G) {
            const T *src = p.partial + (int64_t)(sr.first_slot + s) * p.pw + koff;
            Vec4<T> a = load4(src), b = load4(src + kpad);
#pragma unroll
            for (int e = 0; e < PMF_VEC; ++e) {
                sa.v[e] += a.v[e];
                sb.v[e] += b.v[e];
            }
        }
        store4(smem + (int64_t)g * 2 * kpad + koff, sa);
        store4(smem + (int64_t)g * 2 * kpad + kpad + koff, sb);
    }
    __syncthreads();
    if (g != 0) return;
    sa = zero4<T>();
    sb = zero4<T>();
    if (active) {
        const int ng = min(G, sr.n_slots);
        for (int s = 0; s < ng; ++s) {
            Vec4<T> a = load4(smem + (int64_t)s * 2 * kpad + koff);
            Vec4<T> b = load4(smem + (int64_t)s * 2 * kpad + kpad + koff);
#pragma unroll
            for (int e = 0; e < PMF_VEC; ++e) {
                sa.v[e] += a.v[e];
                sb.v[e] += b.v[e];
            }
        }
    }
    if (STATS) {
        if (active) {
            T *dst = p.stats + (int64_t)sr.row * 2 * kpad + koff;
            store4(dst, sa);
            store4(dst + kpad, sb);
        }
    } else {
        if (EXT) xsum = __shfl(xsum, 0, LPR);  // group 0 = lanes [0, LPR): lane 0 holds the total
        gamma_finalize_row<T, LPR, EXT>(p, sr.row, c, active, sa, sb, xsum, false);
    }
}

// STATS mode, after the all-reduce: every row from its summed statistics.
template <typename T, int LPR>
__global__ __launch_bounds__(256) void gamma_finalize_all_kernel(GammaParams<T> p) {
    constexpr int G = 256 / LPR;
    const int c = threadIdx.x % LPR;
    const int64_t row = p.row0 + (int64_t)blockIdx.x * G + threadIdx.x / LPR;
    if (row >= p.rows) return;
    const int koff = c * PMF_VEC;
    const bool active = koff < p.kpad;
    Vec4<T> sa = zero4<T>(), sb = zero4<T>();
    if (active) {
        const T *src = p.stats + row * 2 * p.kpad + koff;
        sa = load4(src);
        sb = load4(src + p.kpad);
    }
    gamma_finalize_row<T, LPR, false>(p, (int)row, c, active, sa, sb, (T)0, false);
}

// ---------------------------------------------------------------------------
// column sums (pmf_gamma_column_sums; the rate sums of PMF_ZEROS_OBSERVED): C_k = sum over all rows of src[row * stride + k]
// ---------------------------------------------------------------------------
// `src` is a FACTOR array (stride kpad) or the E half of an (E log, E) table (stride 2 kpad, src offset by kpad), in the
// context dtype; the sums are formed in DOUBLE whatever the dtype.  Two stages, no atomics, the same order every time
// and for every task length (the work lists are not read):
//   stage 1  kGammaColsumBlocks blocks; block b owns the contiguous rows [rows b / NB, rows (b + 1) / NB).  Lane c of a lane
//            group owns elements [4c, 4c + 4) (one 16-byte load per lane per row, UN rows in flight); group g adds rows
//            g, g + G, ... of the range in ascending order, the G group sums are added in group order through LDS.
//   stage 2  one block of 1024 threads = 1024 / kpad thread groups; thread k of group g adds the block sums of element k
//            of the contiguous blocks [NB g / groups, NB (g + 1) / groups) in block order, the group sums are added in group
//            order through LDS, and C_k is written as double and, rounded once, in the context dtype (what the sweeps add
//            to the prior rate).
// Pad elements are 0 in both kinds of source, so C is 0 there.
static const int kGammaColsumBlocks = 1024;

template <typename T>
__global__ __launch_bounds__(256) void gamma_colsum_kernel(const T *src, int64_t rows, int64_t stride, int kpad, int lpr_shift,
                                                           double *partial /* [gridDim.x][kpad] */) {
    constexpr int UN = 4;
    __shared__ double s_sum[256 * PMF_VEC];   // [G][4 LPR]
    const int lpr = 1 << lpr_shift, G = 256 >> lpr_shift;
    const int c = threadIdx.x & (lpr - 1), g = threadIdx.x >> lpr_shift;
    const int koff = c * PMF_VEC;
    const bool active = koff < kpad;
    const int64_t r0 = rows * (int64_t)blockIdx.x / gridDim.x, r1 = rows * ((int64_t)blockIdx.x + 1) / gridDim.x;
    double acc[PMF_VEC] = {0.0, 0.0, 0.0, 0.0};
    if (active) {
        const T *at = src + koff;
        int64_t r = r0 + g;
        for (; r + (int64_t)(UN - 1) * G < r1; r += (int64_t)UN * G) {
            Vec4<T> v[UN];
#pragma unroll
            for (int q = 0; q < UN; ++q) v[q] = load4(at + (r + (int64_t)q * G) * stride);
#pragma unroll
            for (int q = 0; q < UN; ++q)
#pragma unroll
                for (int e = 0; e < PMF_VEC; ++e) acc[e] += (double)v[q].v[e];
        }
        for (; r < r1; r += G) {
            const Vec4<T> v = load4(at + r * stride);
#pragma unroll
            for (int e = 0; e < PMF_VEC; ++e) acc[e] += (double)v.v[e];
        }
    }
#pragma unroll
    for (int e = 0; e < PMF_VEC; ++e) s_sum[threadIdx.x * PMF_VEC + e] = acc[e];   // = s_sum[g][koff + e], rows of 4 LPR
    __syncthreads();
    if ((int)threadIdx.x < kpad) {
        double t = 0.0;
        for (int k = 0; k < G; ++k) t += s_sum[k * lpr * PMF_VEC + threadIdx.x];
        partial[(int64_t)blockIdx.x * kpad + threadIdx.x] = t;
    }
}

template <typename T>
__global__ __launch_bounds__(1024) void gamma_colsum_final_kernel(const double *partial, int n_blocks, int kpad, double *out, T *out_t) {
    __shared__ double s_group[1024];   // [groups][kpad]
    const int groups = 1024 / kpad;    // >= 4: kpad <= 256
    const int k = threadIdx.x % kpad, g = threadIdx.x / kpad;
    if (g < groups) {   // (the threads past groups * kpad have no element)
        const int b0 = (int)((int64_t)n_blocks * g / groups), b1 = (int)((int64_t)n_blocks * (g + 1) / groups);
        double t = 0.0;
#pragma unroll 8
        for (int b = b0; b < b1; ++b) t += partial[(int64_t)b * kpad + k];
        s_group[g * kpad + k] = t;
    }
    __syncthreads();
    if ((int)threadIdx.x >= kpad) return;
    double t = 0.0;
    for (int j = 0; j < groups; ++j) t += s_group[j * kpad + threadIdx.x];
    out[threadIdx.x] = t;
    out_t[threadIdx.x] = (T)t;
}

// ---------------------------------------------------------------------------
// fold-in (pmf_gamma_fold_in): the whole n_iter recursion of NEW rows against the frozen other side
// ---------------------------------------------------------------------------
// A fold-in row depends on no other row, so its recursion
//     s = shape_prior + sum_j (x_j / max(b_j . theta, floor)) b_j * theta,   r = rho + sum_j b_j,   theta = s / r,
//     h = hyper_rate_prior + sum_k theta_k,   rho = hyper_shape / h                                   (hierarchical)
// stays with the lanes that own the row: theta, sum_j b_j, the running shape sums, rho and h live in registers from the
// first pass to the last, sum_j b_j is formed in the first pass only, and nothing is written before the end.  The
// access shape is gamma_sweep_kernel's (lane c owns elements 4c .. 4c+3, one 16-byte load per lane per gathered row,
// ids and ratings handed out by __shfl, UN gathers in flight).  Only K values are gathered per rating and every pass
// after the first finds them in the caches, so a row is not cut into tasks: LONG = false gives each lane group one
// row whatever its length (256 / LPR rows per block); LONG = true gives one row to a whole block, group g walking the
// LPR-rating batches g, g + G, ..., for the rows whose serial walk by one group would outlast the rest of the batch.
template <typename T>
struct GammaFoldParams {
    const int32_t *rows;       // [n] rows of the block this launch covers (the short or the long list)
    int64_t n;
    const int64_t *ptr;        // [rows of the block + 1] offsets into other / val
    const int32_t *other;
    const T *val;
    const T *factor_other;
    const T *init_factor;      // [rows][kpad] or null: shape_prior / rho in every element
    const T *init_prior_rate;  // [rows] or null: hyper_shape / hyper_rate_prior
    const T *colsum;           // [kpad] or null.  PMF_ZEROS_OBSERVED: B of every row is the column sum of factor_other
    T *factor, *shape, *rate;  // [rows][kpad]
    T *prior_rate, *hyper_rate;   // [rows], hierarchical only
    T shape_prior, rate_prior, hyper_shape, hyper_rate_prior;
    int hierarchical, n_iter, K, kpad;
};

// pmf_gamma_fold_in_exact (gamma_fold_exact_kernel, with the exact update's code below): the same batch against the
// opposite side's (E log, E) table; factor_other, init_factor and the floor are not used
template <typename T>
struct GammaFoldExactParams : GammaFoldParams<T> {
    const T *table_other;            // [rows of the other side][2][kpad]: E log (pad elements -inf), then E (pad elements 0)
    const T *init_shape, *init_rate; // [rows][kpad] (zero pad elements), both or neither: shape_prior / rho in every element
};

// what a lane keeps of its row between the passes
template <typename T>
struct GammaFoldRow {
    Vec4<T> theta, shape, rate;
    T rho, hyper;
};

template <typename T>
__device__ __forceinline__ GammaFoldRow<T> gamma_fold_start(const GammaFoldParams<T> &p, int64_t row, int c, bool active) {
    const int koff = c * PMF_VEC;
    GammaFoldRow<T> st;
    st.hyper = (T)0;
    st.rho = !p.hierarchical ? p.rate_prior : p.init_prior_rate ? p.init_prior_rate[row] : p.hyper_shape / p.hyper_rate_prior;
    st.shape = st.rate = zero4<T>();
    if (p.init_factor) {   // (staged with zero pad elements)
        st.theta = active ? load4(p.init_factor + row * p.kpad + koff) : zero4<T>();
    } else {
        const T t0 = p.shape_prior / st.rho;
#pragma unroll
        for (int e = 0; e < PMF_VEC; ++e) st.theta.v[e] = (active && koff + e < p.K) ? t0 : (T)0;
    }
    return st;
}

// The ratings [0, n) of one row in batches of LPR, batch `first`, first + step, ...: acc += (x_j / rate_j) b_j * theta and,
// in the call's first pass (`with_b`), bsum += b_j.  All lanes of the group call it together.
template <typename T, int LPR>
__device__ __forceinline__ void gamma_fold_pass(const GammaFoldParams<T> &p, const int32_t *col, const T *val, int64_t n, int first,
                                                int step, int c, bool active, bool with_b, const Vec4<T> &theta, Vec4<T> &acc,
                                                Vec4<T> &bsum) {
    constexpr int UN = LPR < 4 ? LPR : 4;
    const int koff = c * PMF_VEC;
    for (int64_t base = (int64_t)first * LPR; base < n; base += (int64_t)step * LPR) {
        const int cnt = (int)min((int64_t)LPR, n - base);
        int my_o = 0;
        T my_x = (T)0;
        if (c < cnt) {
            my_o = col[base + c];
            my_x = val[base + c];
        }
        for (int tt = 0; tt < cnt; tt += UN) {
            int o[UN];
            T xv[UN];
            Vec4<T> b[UN];
#pragma unroll
            for (int q = 0; q < UN; ++q) {
                o[q] = __shfl(my_o, tt + q, LPR);   // (lanes past the batch hold id 0: a valid row, loaded and not used)
                xv[q] = __shfl(my_x, tt + q, LPR);
            }
#pragma unroll
            for (int q = 0; q < UN; ++q) b[q] = active ? load4(p.factor_other + (int64_t)o[q] * p.kpad + koff) : zero4<T>();
#pragma unroll
            for (int q = 0; q < UN; ++q) {
                if (tt + q < cnt) {
                    T d = b[q].v[0] * theta.v[0];
                    d = fma(b[q].v[1], theta.v[1], d);
                    d = fma(b[q].v[2], theta.v[2], d);
                    d = fma(b[q].v[3], theta.v[3], d);
                    d = vmax(group_sum<LPR>(d), (T)PMF_RATE_FLOOR);
                    const T w = xv[q] / d;
#pragma unroll
                    for (int e = 0; e < PMF_VEC; ++e) {
                        acc.v[e] += (w * b[q].v[e]) * theta.v[e];
                        if (with_b) bsum.v[e] += b[q].v[e];
                    }
                }
            }
        }
    }
}

// theta, rho of the next pass from the row's sums (the arithmetic of gamma_finalize_row)
template <typename T, int LPR>
__device__ __forceinline__ void gamma_fold_update(const GammaFoldParams<T> &p, int c, bool active, const Vec4<T> &acc,
                                                  const Vec4<T> &bsum, GammaFoldRow<T> &st) {
    const int koff = c * PMF_VEC;
    T esum = (T)0;
#pragma unroll
    for (int e = 0; e < PMF_VEC; ++e) {
        const bool ok = active && (koff + e) < p.K;
        const T s = p.shape_prior + acc.v[e];
        const T r = st.rho + bsum.v[e];
        st.shape.v[e] = ok ? s : (T)0;
        st.rate.v[e] = ok ? r : (T)0;
        st.theta.v[e] = ok ? s / r : (T)0;
        esum += st.theta.v[e];
    }
    if (p.hierarchical) {
        st.hyper = p.hyper_rate_prior + group_sum<LPR>(esum);
        st.rho = p.hyper_shape / st.hyper;
    }
}

template <typename T>
__device__ __forceinline__ void gamma_fold_store(const GammaFoldParams<T> &p, int64_t row, int c, bool active, const GammaFoldRow<T> &st) {
    if (active) {
        const int64_t at = row * p.kpad + c * PMF_VEC;
        store4(p.factor + at, st.theta);
        store4(p.shape + at, st.shape);
        store4(p.rate + at, st.rate);
    }
    if (p.hierarchical && c == 0) {
        p.prior_rate[row] = st.rho;
        p.hyper_rate[row] = st.hyper;
    }
}

template <typename T, int LPR, bool LONG>
__global__ __launch_bounds__(256) void gamma_fold_kernel(GammaFoldParams<T> p) {
    constexpr int G = 256 / LPR;
    const int c = threadIdx.x % LPR;
    const int g = threadIdx.x / LPR;
    const int koff = c * PMF_VEC;
    const int kpad = p.kpad;
    const bool active = koff < kpad;
    if constexpr (!LONG) {
        const int64_t at = (int64_t)blockIdx.x * G + g;
        if (at >= p.n) return;
        const int64_t row = p.rows[at];
        const int64_t start = p.ptr[row], n = p.ptr[row + 1] - start;
        const int32_t *col = p.other + start;
        const T *val = p.val + start;
        GammaFoldRow<T> st = gamma_fold_start(p, row, c, active);
        Vec4<T> bsum = (p.colsum && active) ? load4(p.colsum + koff) : zero4<T>();
        for (int t = 0; t < p.n_iter; ++t) {
            Vec4<T> acc = zero4<T>();
            gamma_fold_pass<T, LPR>(p, col, val, n, 0, 1, c, active, t == 0 && !p.colsum, st.theta, acc, bsum);
            gamma_fold_update<T, LPR>(p, c, active, acc, bsum, st);
        }
        gamma_fold_store(p, row, c, active, st);
    } else {
        // One block per row (the grid is the long list exactly: every thread reaches every barrier).  Per pass each
        // group leaves its partial sums in LDS; after the barrier EVERY group adds the G partials in group order, so
        // all groups hold the same theta / rho bit for bit without a broadcast; the second barrier keeps the next
        // pass's partials off the ones still being read.
        extern __shared__ __align__(16) unsigned char smem_raw[];
        T *part = reinterpret_cast<T *>(smem_raw);   // [G][kpad] shape partials, then [G][kpad] sum_j b_j partials (first pass)
        const int64_t row = p.rows[blockIdx.x];
        const int64_t start = p.ptr[row], n = p.ptr[row + 1] - start;
        const int32_t *col = p.other + start;
        const T *val = p.val + start;
        GammaFoldRow<T> st = gamma_fold_start(p, row, c, active);
        Vec4<T> bsum = (p.colsum && active) ? load4(p.colsum + koff) : zero4<T>();
        for (int t = 0; t < p.n_iter; ++t) {
            const bool with_b = t == 0 && !p.colsum;   // (the same in every thread)
            Vec4<T> acc = zero4<T>(), bpart = zero4<T>();
            gamma_fold_pass<T, LPR>(p, col, val, n, g, G, c, active, with_b, st.theta, acc, bpart);
            if (active) {
                store4(part + g * kpad + koff, acc);
                if (with_b) store4(part + (G + g) * kpad + koff, bpart);
            }
            __syncthreads();
            acc = zero4<T>();
            if (active) {
#pragma unroll 4   // (unrolled whole, G = 32 partials in flight cost 150 registers)
                for (int s = 0; s < G; ++s) {
                    const Vec4<T> a = load4(part + s * kpad + koff);
#pragma unroll
                    for (int e = 0; e < PMF_VEC; ++e) acc.v[e] += a.v[e];
                    if (with_b) {
                        const Vec4<T> b = load4(part + (G + s) * kpad + koff);
#pragma unroll
                        for (int e = 0; e < PMF_VEC; ++e) bsum.v[e] += b.v[e];
                    }
                }
            }
            gamma_fold_update<T, LPR>(p, c, active, acc, bsum, st);
            __syncthreads();
        }
        if (g == 0) gamma_fold_store(p, row, c, active, st);
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
struct GammaPriors { double shape = 0, rate = 0; int hierarchical = 0; double hyper_shape = 0, hyper_rate = 0; };

// SWEEP (gamma_sweep_kernel, or gamma_exact_kernel with its two tables in `more`) over the tasks, then the split
// kernel over the rows cut into several tasks
template <typename T, int LPR, bool STATS, bool EXT, auto SWEEP, typename... A>
static void launch_gamma(pmf_ctx *ctx, const GammaParams<T> &p, const PmfTaskView &tl, A... more) {
    constexpr int G = 256 / LPR;
    if (tl.n_tasks > 0) {
        PmfProfScope prof(ctx, PMF_KERNEL_GAMMA_SWEEP);
        hipLaunchKernelGGL(SWEEP, dim3((unsigned)((tl.n_tasks + G - 1) / G)), dim3(256), 0, ctx->stream, p, more...);
    }
    if (tl.n_split > 0) {
        PmfProfScope prof(ctx, PMF_KERNEL_GAMMA_FINAL);
        size_t smem = (size_t)G * 2 * ctx->kpad * sizeof(T);
        hipLaunchKernelGGL((gamma_split_kernel<T, LPR, STATS, EXT>), dim3((unsigned)tl.n_split), dim3(256), smem, ctx->stream, p);
    }
}

// f(std::integral_constant<int, LPR>()) for the context's lanes per row (at most 64: pmf_ctx_create caps n_factors),
// then the launch error check
template <typename F>
static int gamma_launch(pmf_ctx *ctx, F &&f) {
    pmf_with_pow2<1>(pmf_lanes_per_row(ctx->kpad), f);
    PMF_HIP_CHECK(hipGetLastError());
    return PMF_OK;
}

static bool gamma_zeros_observed(const pmf_ctx *ctx) { return ctx->gamma_zeros == PMF_ZEROS_OBSERVED; }

// the caller-driven and extended forms, which PMF_ZEROS_OBSERVED does not cover
#define PMF_REQUIRE_ZEROS_MISSING(fn)                                                                                      \
    PMF_REQUIRE(!gamma_zeros_observed(ctx), PMF_EINVAL,                                                                    \
                fn ": not available while the context counts unobserved cells as zeros (pmf_ctx_set_gamma_zeros, PMF_ZEROS_OBSERVED)")

// The work area of one column sum inside a scratch layout -- the block sums, C in double, C in the context dtype -- and
// its two launches (the caller holds the profile bracket -- brackets do not nest -- and checks the launch).  `on` false:
// the layout gets nothing and launch() must not be called.
template <typename T>
struct GammaColsum {
    PmfLayout::Piece<double> part_at, sum_at;
    PmfLayout::Piece<T> sum_t_at;
    GammaColsum(PmfLayout &lay, int kpad, bool on = true)
        : part_at(lay.add<double>(on ? (size_t)kGammaColsumBlocks * kpad : 0)), sum_at(lay.add<double>(on ? (size_t)kpad : 0)),
          sum_t_at(lay.add<T>(on ? (size_t)kpad : 0)) {}
    void launch(pmf_ctx *ctx, void *base, const T *src, int64_t rows, int64_t stride) const {
        int shift = 0;
        while ((1 << shift) < pmf_lanes_per_row(ctx->kpad)) ++shift;
        hipLaunchKernelGGL((gamma_colsum_kernel<T>), dim3(kGammaColsumBlocks), dim3(256), 0, ctx->stream, src, rows, stride, ctx->kpad, shift,
                           part_at.at(base));
        hipLaunchKernelGGL((gamma_colsum_final_kernel<T>), dim3(1), dim3(1024), 0, ctx->stream, part_at.at(base), kGammaColsumBlocks, ctx->kpad,
                           sum_at.at(base), sum_t_at.at(base));
    }
};

// The column sums of `src` ([rows][stride]) into the context's scratch buffer, which holds nothing else for the caller:
// *sum (double) and *sum_t (context dtype) stay valid until the next call that lays out the scratch buffer.  Timed as
// PMF_KERNEL_GAMMA_FINAL, in a bracket of its own: call it outside any other.
template <typename T>
static int gamma_colsum_scratch(pmf_ctx *ctx, const T *src, int64_t rows, int64_t stride, const double **sum, const T **sum_t) {
    PmfLayout lay(256);
    const GammaColsum<T> cs(lay, ctx->kpad);
    int rc;
    if ((rc = pmf_ensure_scratch(ctx, lay.bytes()))) return rc;
    void *base = ctx->d_scratch.as();
    {
        PmfProfScope prof(ctx, PMF_KERNEL_GAMMA_FINAL);
        cs.launch(ctx, base, src, rows, stride);
    }
    PMF_HIP_CHECK(hipGetLastError());
    if (sum) *sum = cs.sum_at.at(base);
    if (sum_t) *sum_t = cs.sum_t_at.at(base);
    return PMF_OK;
}

// the arrays and ratings every gamma launch reads
static int check_gamma_inputs(pmf_ctx *ctx, int side) {
    int rc;
    if ((rc = pmf_require_array(ctx, side, PMF_ARR_FACTOR, "pmf_gamma_sweep"))) return rc;
    if ((rc = pmf_require_array(ctx, 1 - side, PMF_ARR_FACTOR, "pmf_gamma_sweep"))) return rc;
    PMF_REQUIRE(ctx->index[side].d_ptr, PMF_EINVAL, "pmf_gamma_sweep: ratings have not been set");
    return PMF_OK;
}

// SHAPE and RATE of the sides listed are set: q itself, which the ELBO, the exact update and the predictive read
static int require_gamma_q(pmf_ctx *ctx, std::initializer_list<int> sides, const char *what) {
    int rc;
    for (int s : sides) {
        if ((rc = pmf_require_array(ctx, s, PMF_ARR_SHAPE, what))) return rc;
        if ((rc = pmf_require_array(ctx, s, PMF_ARR_RATE, what))) return rc;
    }
    return PMF_OK;
}

template <typename T>
static GammaParams<T> gamma_params(const pmf_ctx *ctx, int side, const PmfTaskView &tl, void *stats, const GammaPriors &pr, int pw) {
    const int other = 1 - side;
    const PmfSideIndex &ix = ctx->index[side];
    GammaParams<T> p;
    p.tasks = tl.d_tasks;
    p.n_tasks = tl.n_tasks;
    p.split = tl.d_split;
    p.other = ix.d_other.as<int32_t>();
    p.val = ix.d_val.as<const T>();
    p.factor_self = ctx->arr[side][PMF_ARR_FACTOR].as<T>();
    p.factor_other = ctx->arr[other][PMF_ARR_FACTOR].as<const T>();
    p.shape = ctx->arr[side][PMF_ARR_SHAPE].as<T>();
    p.rate = ctx->arr[side][PMF_ARR_RATE].as<T>();
    p.prior_rate_vec = ctx->arr[side][PMF_ARR_PRIOR_RATE].as<T>();
    p.hyper_rate = ctx->arr[side][PMF_ARR_HYPER_RATE].as<T>();
    p.scale_other = ctx->arr[other][PMF_ARR_SCALE].as<const T>();
    p.scale_self = ctx->arr[side][PMF_ARR_SCALE].as<T>();
    p.scale_shape = ctx->arr[side][PMF_ARR_SCALE_SHAPE].as<T>();
    p.scale_rate = ctx->arr[side][PMF_ARR_SCALE_RATE].as<T>();
    p.pw = pw;
    p.partial = ctx->d_partial.as<T>();
    p.stats = (T *)stats;
    p.colsum = nullptr;
    p.shape_prior = (T)pr.shape;
    p.rate_prior = (T)pr.rate;
    p.hyper_shape = (T)pr.hyper_shape;
    p.hyper_rate_prior = (T)pr.hyper_rate;
    p.hierarchical = pr.hierarchical;
    p.K = ctx->K;
    p.kpad = ctx->kpad;
    p.row0 = tl.row0;   // finalize-from-stats covers rows [row0, rows)
    p.rows = tl.row1;
    return p;
}

// `ext`: the extended model (per-row scalar factors phi / psi), fused pass only
template <typename T>
static int run_gamma(pmf_ctx *ctx, int side, PmfPass pass, bool ext, void *stats, const GammaPriors &pr) {
    const PmfTaskView tl = pmf_task_view(ctx, side, ctx->index[side].gamma_tasks, pass != PMF_PASS_FUSED);
    int rc;
    pmf_factor_written(ctx);
    if (pass == PMF_PASS_FINALIZE) {
        // reads the statistics only, whichever accumulate wrote them: after pmf_gamma_exact_accumulate no FACTOR need exist
        if ((rc = pmf_alloc_array(ctx, side, PMF_ARR_FACTOR))) return rc;
    } else if ((rc = check_gamma_inputs(ctx, side))) {
        return rc;
    }
    if (pass != PMF_PASS_ACCUMULATE) {
        if ((rc = pmf_alloc_array(ctx, side, PMF_ARR_SHAPE))) return rc;
        if ((rc = pmf_alloc_array(ctx, side, PMF_ARR_RATE))) return rc;
        if (pr.hierarchical) {
            if ((rc = pmf_require_array(ctx, side, PMF_ARR_PRIOR_RATE, "pmf_gamma_sweep (hierarchical)"))) return rc;
            if ((rc = pmf_alloc_array(ctx, side, PMF_ARR_HYPER_RATE))) return rc;
        }
    }
    const int pw = 2 * ctx->kpad + (ext ? PMF_VEC : 0);
    if (pass != PMF_PASS_FINALIZE && tl.n_slots > 0 && (rc = pmf_ensure_partial(ctx, (size_t)tl.n_slots * pw * sizeof(T)))) return rc;
    if (ext) {
        if ((rc = pmf_require_array(ctx, side, PMF_ARR_SCALE, "pmf_gamma_ext_sweep"))) return rc;
        if ((rc = pmf_require_array(ctx, 1 - side, PMF_ARR_SCALE, "pmf_gamma_ext_sweep"))) return rc;
        if ((rc = pmf_alloc_array(ctx, side, PMF_ARR_SCALE_SHAPE))) return rc;
        if ((rc = pmf_alloc_array(ctx, side, PMF_ARR_SCALE_RATE))) return rc;
    }
    GammaParams<T> p = gamma_params<T>(ctx, side, tl, stats, pr, pw);
    // unlisted cells as zeros (fused pass of the plain model only: the entry points refuse the rest): every row's rate sum
    // is the column sum of the other side's FACTOR as it is now
    if (gamma_zeros_observed(ctx) && pass == PMF_PASS_FUSED && !ext &&
        (rc = gamma_colsum_scratch<T>(ctx, p.factor_other, ctx->rows[1 - side], ctx->kpad, nullptr, &p.colsum)))
        return rc;
    return gamma_launch(ctx, [&](auto L) {
        constexpr int G = 256 / L;
        if (pass == PMF_PASS_FINALIZE) {
            PmfProfScope prof(ctx, PMF_KERNEL_GAMMA_FINAL);
            if (p.rows > p.row0)
                hipLaunchKernelGGL((gamma_finalize_all_kernel<T, L>), dim3((unsigned)((p.rows - p.row0 + G - 1) / G)), dim3(256), 0,
                                   ctx->stream, p);
        } else if (pass == PMF_PASS_ACCUMULATE) {
            launch_gamma<T, L, true, false, gamma_sweep_kernel<T, L, true, false>>(ctx, p, tl);
        } else if (ext) {
            launch_gamma<T, L, false, true, gamma_sweep_kernel<T, L, false, true>>(ctx, p, tl);
        } else {
            launch_gamma<T, L, false, false, gamma_sweep_kernel<T, L, false, false>>(ctx, p, tl);
        }
    });
}

// one launch of the gather-only twin of the fused sweep (pmf_prof_gather_ceiling)
template <typename T>
static int run_gather_probe(pmf_ctx *ctx, int side) {
    const PmfTaskView tl = pmf_task_view(ctx, side, ctx->index[side].gamma_tasks, false);
    int rc;
    if ((rc = check_gamma_inputs(ctx, side)) || (rc = pmf_ensure_scratch(ctx, 64))) return rc;
    const GammaParams<T> p = gamma_params<T>(ctx, side, tl, nullptr, GammaPriors(), 2 * ctx->kpad);
    return gamma_launch(ctx, [&](auto L) {
        constexpr int G = 256 / L;
        if (tl.n_tasks > 0)
            hipLaunchKernelGGL((gamma_gather_probe_kernel<T, L>), dim3((unsigned)((tl.n_tasks + G - 1) / G)), dim3(256), 0,
                               ctx->stream, p, ctx->d_scratch.as<T>());
    });
}

// The item half-sweep on several ranks (pmf_comm.hip): `accumulate` per chunk, the exchange, run_gamma's finalize.
// Finalize is element-wise (cheap) and writes 3 Kpad + 2 values per row for 2 Kpad of statistics, so the plain
// all-reduce is the default exchange here.  `alloc`: the arrays of the side the call creates first, in this order
// (HYPER_RATE only when hierarchical).
template <typename T>
static int gamma_comm_half_sweep(pmf_ctx *ctx, int side, const GammaPriors &pr, std::initializer_list<int> alloc,
                                 const std::function<int(void *)> &accumulate) {
    const PmfExchange ex = {false, pr.hierarchical ? 5 : 3,
                            {PMF_ARR_FACTOR, PMF_ARR_SHAPE, PMF_ARR_RATE, PMF_ARR_PRIOR_RATE, PMF_ARR_HYPER_RATE}};
    int rc;
    for (int array : alloc)
        if ((array != PMF_ARR_HYPER_RATE || pr.hierarchical) && (rc = pmf_alloc_array(ctx, side, array))) return rc;
    return pmf_comm_half_sweep(ctx, side, 0, (size_t)2 * ctx->kpad, true, ex, accumulate,
                               [&](void *s) { return run_gamma<T>(ctx, side, PMF_PASS_FINALIZE, false, s, pr); });
}

extern "C" int pmf_gamma_sweep(pmf_ctx *ctx, int side, double shape_prior, double rate_prior,
                               int hierarchical, double hyper_shape, double hyper_rate_prior) {
    PMF_SIDE_ENTRY("pmf_gamma_sweep");
    PMF_REQUIRE_UNWEIGHTED("pmf_gamma_sweep");
    const GammaPriors pr = {shape_prior, rate_prior, hierarchical, hyper_shape, hyper_rate_prior};
    return pmf_with_dtype(ctx, [&](auto t) {
        using T = decltype(t);
        if (side != PMF_SIDE_ITEM || !pmf_comm_active(ctx)) return run_gamma<T>(ctx, side, PMF_PASS_FUSED, false, nullptr, pr);
        // (SHAPE and RATE: the gathers address them before finalize runs)
        return gamma_comm_half_sweep<T>(ctx, side, pr, {PMF_ARR_SHAPE, PMF_ARR_RATE, PMF_ARR_HYPER_RATE}, [&](void *s) {
            return run_gamma<T>(ctx, side, PMF_PASS_ACCUMULATE, false, s, GammaPriors());
        });
    });
}

extern "C" int pmf_gamma_ext_sweep(pmf_ctx *ctx, int side, double shape_prior, double rate_prior) {
    PMF_SIDE_ENTRY("pmf_gamma_ext_sweep");
    PMF_REQUIRE_UNWEIGHTED("pmf_gamma_ext_sweep");
    PMF_REQUIRE_ZEROS_MISSING("pmf_gamma_ext_sweep");
    PMF_REQUIRE(!pmf_comm_active(ctx), PMF_EINVAL, "pmf_gamma_ext_sweep: the extended model is not available on several ranks");
    const GammaPriors pr = {shape_prior, rate_prior};
    return pmf_with_dtype(ctx, [&](auto t) { return run_gamma<decltype(t)>(ctx, side, PMF_PASS_FUSED, true, nullptr, pr); });
}

extern "C" int pmf_gamma_accumulate(pmf_ctx *ctx, int side, void *stats_dev) {
    PMF_SIDE_ENTRY("pmf_gamma_accumulate");
    PMF_REQUIRE_UNWEIGHTED("pmf_gamma_accumulate");
    PMF_REQUIRE_ZEROS_MISSING("pmf_gamma_accumulate");
    PMF_REQUIRE(stats_dev, PMF_EINVAL, "pmf_gamma_accumulate: null stats buffer");
    return pmf_with_dtype(ctx, [&](auto t) { return run_gamma<decltype(t)>(ctx, side, PMF_PASS_ACCUMULATE, false, stats_dev, {}); });
}

extern "C" int pmf_gamma_finalize(pmf_ctx *ctx, int side, const void *stats_dev, double shape_prior,
                                  double rate_prior, int hierarchical, double hyper_shape,
                                  double hyper_rate_prior) {
    PMF_SIDE_ENTRY("pmf_gamma_finalize");
    PMF_REQUIRE_ZEROS_MISSING("pmf_gamma_finalize");
    PMF_REQUIRE(stats_dev, PMF_EINVAL, "pmf_gamma_finalize: null stats buffer");
    const GammaPriors pr = {shape_prior, rate_prior, hierarchical, hyper_shape, hyper_rate_prior};
    return pmf_with_dtype(ctx, [&](auto t) { return run_gamma<decltype(t)>(ctx, side, PMF_PASS_FINALIZE, false, (void *)stats_dev, pr); });
}

// ---- fold-in -----------------------------------------------------------------
// Rows with more than this many ratings take the block-per-row kernel (PMF_GAMMA_FOLD_LONG=n overrides it).
// Measured on one MI355X (tools/probe_gamma_fold_in.py, K = 64 fp32, n_iter = 10; tables in DESIGN.md section 4.9):
//  - 256 rows of 2^6 .. 2^16 ratings, nothing else on the chip: the block kernel wins at every length (64 ratings: 0.045
//    against 0.138 ms; 1024: 0.22 against 2.64 ms; 65536: 11.1 against 167.3 ms).  That sweep has no crossover, because
//    256 lane groups fill 16 of the 256 CUs: it shows one group's serial walk, 0.26 us per rating and update.
//  - the batch a threshold is for, 100 000 rows x 50 ratings (1.27 ms) plus ONE long row: with 256 ratings the row
//    variant alone is faster (1.271 against 1.332 ms), with 512 the long row is the tail (1.85 against 1.35 ms), with
//    1024 it takes 2.98 against 1.44 ms.  The crossover lies between 256 and 512 ratings for this batch and moves in
//    proportion to the batch's own kernel time.
// The tests pin rows of up to 700 ratings to the row variant under the default, so the default is the smallest
// multiple of 256 above that, not the 512 the second measurement would suggest: a 768-rating row costs a batch of this
// size about 1 ms more than it would in a block of its own.
static const int64_t kGammaFoldLongRow = 768;
static const int64_t kGammaFoldRowBytes = 256ll << 20;   // one [rows][kpad] buffer of a row block

struct GammaFoldBatch {
    int64_t n_rows;
    const int64_t *row_ptr;
    const int32_t *other_ids;
    const double *ratings;
    GammaPriors pr;
    int n_iter;
    const double *init_factor, *init_prior_rate;
    double *out_factor, *out_shape, *out_rate, *out_prior_rate, *out_hyper_rate;
    bool exact = false;                  // pmf_gamma_fold_in_exact: `init_factor` holds init_shape
    const double *init_rate = nullptr;   // [n_rows][K] with init_shape, exact only
};

// the exact recursion's two steps of the shared host path (defined with its kernel, below the exact half-sweep):
// the opposite side's freshly built (E log, E) table and, in zero mode, the column sums of its E half
template <typename T>
static int gamma_fold_exact_other(pmf_ctx *ctx, int side, const T **table, const T **colsum);
// one launch of each variant at most, timed as the reference fold-in's
template <typename T>
static void launch_gamma_fold_exact(pmf_ctx *ctx, GammaFoldExactParams<T> &p, const int32_t *list, int64_t n_short, int64_t n_long);

// The batch in row blocks of at most PMF_FOLD_IN_BLOCK_NNZ staged ratings (a longer single row still goes), ctx->fold_in_rows
// rows and kGammaFoldRowBytes per row buffer.  Per block: stage offsets, ids, ratings and start values in the context
// dtype, list the short and the long rows, one launch of each kernel at most, download.  Everything lives in buffers
// of this call: the context's model state, index and work lists are only read.
template <typename T>
static int run_gamma_fold_in(pmf_ctx *ctx, int side, const GammaFoldBatch &a) {
    const int K = ctx->K, kpad = ctx->kpad;
    const int lpr = pmf_lanes_per_row(kpad);
    const int64_t long_row = ctx->gamma_fold_long > 0 ? ctx->gamma_fold_long : kGammaFoldLongRow;
    const int64_t by_bytes = std::max<int64_t>(1, kGammaFoldRowBytes / ((int64_t)kpad * (int64_t)sizeof(T)));
    const int64_t max_rows = std::min(by_bytes, ctx->fold_in_rows > 0 ? ctx->fold_in_rows : (int64_t)INT32_MAX);
    const bool hier = a.pr.hierarchical != 0;
    PmfFoldStage<T> st;
    PmfBuf d_list, d_init, d_init_b, d_init_rate, d_factor, d_shape, d_rate, d_prior_rate, d_hyper_rate;
    std::vector<int32_t> list;   // the short rows, then the long rows
    std::vector<T> init, init_b, init_rate;
    int rc;
    // unlisted cells as zeros: B of every row is the column sum of the other side's FACTOR (exact: of the E half of its
    // table, which is built here, once per call), formed once per call
    const T *colsum = nullptr, *table_other = nullptr;
    if (a.exact) {
        if ((rc = gamma_fold_exact_other<T>(ctx, side, &table_other, &colsum))) return rc;
    } else if (gamma_zeros_observed(ctx) &&
               (rc = gamma_colsum_scratch<T>(ctx, ctx->arr[1 - side][PMF_ARR_FACTOR].as<const T>(), ctx->rows[1 - side], kpad, nullptr, &colsum))) {
        return rc;
    }
    // start values of a row block in the context dtype, pad elements 0
    const auto stage_rows = [&](const double *src, int64_t r0, int64_t B, std::vector<T> &dst) {
        dst.assign((size_t)B * kpad, (T)0);
        for (int64_t r = 0; r < B; ++r)
            for (int k = 0; k < K; ++k) dst[(size_t)(r * kpad + k)] = (T)src[(r0 + r) * K + k];
    };
    for (int64_t r0 = 0; r0 < a.n_rows; r0 = st.r1) {
        // (the previous block ended with a stream synchronise: nothing queued still reads the block's buffers)
        if ((rc = st.stage(ctx, a.n_rows, a.row_ptr, a.ratings, r0, max_rows))) return rc;
        const std::vector<int64_t> &ptr = st.ptr;
        const int64_t B = st.r1 - r0;
        list.clear();
        for (int64_t r = 0; r < B; ++r)
            if (ptr[(size_t)r + 1] - ptr[(size_t)r] <= long_row) list.push_back((int32_t)r);
        const int64_t n_short = (int64_t)list.size(), n_long = B - n_short;
        // longest first (as the sweeps' task lists): the lane group with the longest walk starts with the launch
        const auto longer = [&](int32_t x, int32_t y) { return ptr[(size_t)x + 1] - ptr[(size_t)x] > ptr[(size_t)y + 1] - ptr[(size_t)y]; };
        if (!std::is_sorted(list.begin(), list.end(), longer)) std::stable_sort(list.begin(), list.end(), longer);
        for (int64_t r = 0; r < B; ++r)
            if (ptr[(size_t)r + 1] - ptr[(size_t)r] > long_row) list.push_back((int32_t)r);
        if (a.init_factor) stage_rows(a.init_factor, r0, B, init);
        if (a.init_rate) stage_rows(a.init_rate, r0, B, init_b);
        if (hier && a.init_prior_rate) {
            init_rate.resize((size_t)B);
            for (int64_t r = 0; r < B; ++r) init_rate[(size_t)r] = (T)a.init_prior_rate[r0 + r];
        }
        const size_t row_bytes = (size_t)B * kpad * sizeof(T);
        if ((rc = d_list.reserve(ctx, (size_t)B * sizeof(int32_t), {ctx->stream}))) return rc;
        if ((rc = d_factor.reserve(ctx, row_bytes, {ctx->stream}))) return rc;
        if ((rc = d_shape.reserve(ctx, row_bytes, {ctx->stream}))) return rc;
        if ((rc = d_rate.reserve(ctx, row_bytes, {ctx->stream}))) return rc;
        if (a.init_factor && (rc = d_init.reserve(ctx, row_bytes, {ctx->stream}))) return rc;
        if (a.init_rate && (rc = d_init_b.reserve(ctx, row_bytes, {ctx->stream}))) return rc;
        if (hier) {
            if ((rc = d_prior_rate.reserve(ctx, (size_t)B * sizeof(T), {ctx->stream}))) return rc;
            if ((rc = d_hyper_rate.reserve(ctx, (size_t)B * sizeof(T), {ctx->stream}))) return rc;
            if (a.init_prior_rate && (rc = d_init_rate.reserve(ctx, (size_t)B * sizeof(T), {ctx->stream}))) return rc;
        }
        if ((rc = st.upload(a.other_ids))) return rc;
        PMF_HIP_CHECK(hipMemcpy(d_list.as(), list.data(), (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice));
        if (a.init_factor) PMF_HIP_CHECK(hipMemcpy(d_init.as(), init.data(), row_bytes, hipMemcpyHostToDevice));
        if (a.init_rate) PMF_HIP_CHECK(hipMemcpy(d_init_b.as(), init_b.data(), row_bytes, hipMemcpyHostToDevice));
        if (hier && a.init_prior_rate)
            PMF_HIP_CHECK(hipMemcpy(d_init_rate.as(), init_rate.data(), (size_t)B * sizeof(T), hipMemcpyHostToDevice));
        GammaFoldExactParams<T> p;   // (the reference recursion's launches take its GammaFoldParams part)
        p.ptr = st.d_ptr.template as<const int64_t>();
        p.other = st.d_other.template as<const int32_t>();
        p.val = st.d_val.template as<const T>();
        p.factor_other = a.exact ? nullptr : ctx->arr[1 - side][PMF_ARR_FACTOR].as<const T>();
        p.init_factor = a.init_factor && !a.exact ? d_init.as<const T>() : nullptr;
        p.table_other = table_other;
        p.init_shape = a.init_factor && a.exact ? d_init.as<const T>() : nullptr;
        p.init_rate = a.init_rate ? d_init_b.as<const T>() : nullptr;
        p.init_prior_rate = hier && a.init_prior_rate ? d_init_rate.as<const T>() : nullptr;
        p.colsum = colsum;
        p.factor = d_factor.as<T>();
        p.shape = d_shape.as<T>();
        p.rate = d_rate.as<T>();
        p.prior_rate = hier ? d_prior_rate.as<T>() : nullptr;
        p.hyper_rate = hier ? d_hyper_rate.as<T>() : nullptr;
        p.shape_prior = (T)a.pr.shape;
        p.rate_prior = (T)a.pr.rate;
        p.hyper_shape = (T)a.pr.hyper_shape;
        p.hyper_rate_prior = (T)a.pr.hyper_rate;
        p.hierarchical = a.pr.hierarchical;
        p.n_iter = a.n_iter;
        p.K = K;
        p.kpad = kpad;
        if (a.exact) launch_gamma_fold_exact<T>(ctx, p, d_list.as<const int32_t>(), n_short, n_long);
        else pmf_with_pow2<1>(lpr, [&](auto L) {
            constexpr int G = 256 / L;
            GammaFoldParams<T> &q = p;
            if (n_short > 0) {
                PmfProfScope prof(ctx, PMF_KERNEL_GAMMA_SWEEP);
                q.rows = d_list.as<const int32_t>();
                q.n = n_short;
                hipLaunchKernelGGL((gamma_fold_kernel<T, L, false>), dim3((unsigned)((n_short + G - 1) / G)), dim3(256), 0, ctx->stream, q);
            }
            if (n_long > 0) {
                PmfProfScope prof(ctx, PMF_KERNEL_GAMMA_FINAL);
                q.rows = d_list.as<const int32_t>() + n_short;
                q.n = n_long;
                hipLaunchKernelGGL((gamma_fold_kernel<T, L, true>), dim3((unsigned)n_long), dim3(256), (size_t)G * 2 * kpad * sizeof(T),
                                   ctx->stream, q);
            }
        });
        PMF_HIP_CHECK(hipGetLastError());
        // (every download ends with a stream synchronise: the block's kernels are done with the staging buffers)
        if ((rc = pmf_fold_in_download(ctx, PMF_ARR_FACTOR, d_factor.as(), a.out_factor + r0 * K, B))) return rc;
        if (a.out_shape && (rc = pmf_fold_in_download(ctx, PMF_ARR_SHAPE, d_shape.as(), a.out_shape + r0 * K, B))) return rc;
        if (a.out_rate && (rc = pmf_fold_in_download(ctx, PMF_ARR_RATE, d_rate.as(), a.out_rate + r0 * K, B))) return rc;
        if (hier && a.out_prior_rate && (rc = pmf_fold_in_download(ctx, PMF_ARR_PRIOR_RATE, d_prior_rate.as(), a.out_prior_rate + r0, B))) return rc;
        if (hier && a.out_hyper_rate && (rc = pmf_fold_in_download(ctx, PMF_ARR_HYPER_RATE, d_hyper_rate.as(), a.out_hyper_rate + r0, B))) return rc;
    }
    return PMF_OK;
}

// What the two fold-in entry points share after PMF_SIDE_ENTRY: the argument checks (`fn` names the caller in every
// message; `exact`: SHAPE and RATE of the opposite side in place of its FACTOR, init_shape / init_rate together, no
// SCALE arrays) and the run.
static int gamma_fold_in_call(const char *fn, pmf_ctx *ctx, int side, const GammaFoldBatch &a) {
    PMF_REQUIRE(a.n_rows >= 0, PMF_EINVAL, "%s: negative row count", fn);
    if (a.n_rows == 0) return PMF_OK;
    PMF_REQUIRE(a.row_ptr && a.out_factor, PMF_EINVAL, "%s: null argument", fn);
    int rc;
    if ((rc = pmf_check_offsets(fn, "row_ptr", a.row_ptr, a.n_rows))) return rc;
    const int64_t nnz = a.row_ptr[a.n_rows];
    PMF_REQUIRE(nnz == 0 || (a.other_ids && a.ratings), PMF_EINVAL, "%s: null argument", fn);
    PMF_REQUIRE(a.pr.shape > 0, PMF_EINVAL, "%s: shape_prior must be positive", fn);
    if (a.pr.hierarchical)
        PMF_REQUIRE(a.pr.hyper_shape > 0 && a.pr.hyper_rate > 0, PMF_EINVAL, "%s: hyper_shape and hyper_rate_prior must be positive", fn);
    else
        PMF_REQUIRE(a.pr.rate > 0, PMF_EINVAL, "%s: rate_prior must be positive", fn);
    PMF_REQUIRE(a.n_iter >= 1, PMF_EINVAL, "%s: n_iter = %d, must be at least 1", fn, a.n_iter);
    const int other = 1 - side;
    if (a.exact) {
        PMF_REQUIRE((a.init_factor != nullptr) == (a.init_rate != nullptr), PMF_EINVAL,
                    "%s: init_shape and init_rate are given together or not at all", fn);
        PMF_REQUIRE(!ctx->arr[0][PMF_ARR_SCALE] && !ctx->arr[1][PMF_ARR_SCALE], PMF_EINVAL,
                    "%s: the extended Poisson model (a context with SCALE arrays) is not covered", fn);
        if ((rc = require_gamma_q(ctx, {other}, fn))) return rc;
    } else if ((rc = pmf_require_array(ctx, other, PMF_ARR_FACTOR, fn))) {
        return rc;
    }
    if ((rc = pmf_check_ids(a.other_ids, nnz, ctx->rows[other], fn, "id"))) return rc;
    return pmf_no_throw(fn, [&] {
        return pmf_with_dtype(ctx, [&](auto t) { return run_gamma_fold_in<decltype(t)>(ctx, side, a); });
    });
}

extern "C" int pmf_gamma_fold_in(pmf_ctx *ctx, int side, int64_t n_rows, const int64_t *row_ptr, const int32_t *other_ids,
                                 const double *ratings, double shape_prior, double rate_prior, int hierarchical,
                                 double hyper_shape, double hyper_rate_prior, int n_iter, const double *init_factor,
                                 const double *init_prior_rate, double *out_factor, double *out_shape, double *out_rate,
                                 double *out_prior_rate, double *out_hyper_rate) {
    PMF_SIDE_ENTRY("pmf_gamma_fold_in");
    return gamma_fold_in_call("pmf_gamma_fold_in", ctx, side,
                              {n_rows, row_ptr, other_ids, ratings, {shape_prior, rate_prior, hierarchical, hyper_shape, hyper_rate_prior},
                               n_iter, init_factor, init_prior_rate, out_factor, out_shape, out_rate, out_prior_rate, out_hyper_rate});
}

extern "C" int pmf_gamma_fold_in_exact(pmf_ctx *ctx, int side, int64_t n_rows, const int64_t *row_ptr, const int32_t *other_ids,
                                       const double *ratings, double shape_prior, double rate_prior, int hierarchical,
                                       double hyper_shape, double hyper_rate_prior, int n_iter, const double *init_shape,
                                       const double *init_rate, const double *init_prior_rate, double *out_factor,
                                       double *out_shape, double *out_rate, double *out_prior_rate, double *out_hyper_rate) {
    PMF_SIDE_ENTRY("pmf_gamma_fold_in_exact");
    return gamma_fold_in_call("pmf_gamma_fold_in_exact", ctx, side,
                              {n_rows, row_ptr, other_ids, ratings, {shape_prior, rate_prior, hierarchical, hyper_shape, hyper_rate_prior},
                               n_iter, init_shape, init_prior_rate, out_factor, out_shape, out_rate, out_prior_rate, out_hyper_rate,
                               true, init_rate});
}

// ---------------------------------------------------------------------------
// evidence lower bound (pmf_gamma_elbo_terms): the per-row sums that do not depend on the hyperparameters
// ---------------------------------------------------------------------------
// q(theta_rk) = Gamma(SHAPE, RATE) only (FACTOR is not read).  Two passes:
//   row pass   a lane group per row in the sweep's layout; digamma and lgamma in DOUBLE whatever the context dtype -- it
//              is rows x K evaluations, and lgamma(a) + (1 - a) psi(a) cancels in fp32 once a shape reaches the thousands
//              (a = 1e4: two terms of 8e4 leave 6, fp32 keeps 7e-3 of it) -- and writes, in the context dtype, the table
//              the data pass gathers from: [rows][2][kpad] = E log (pad elements -inf), then E (pad elements 0), so the
//              two 16-byte pieces a lane needs of one rating lie in one 2 kpad block and exp of a pad adds 0.
//   data pass  a lane group per task of the side's GAMMA list (read only); the row's own pair stays in registers; per
//              rating the other row's pair is gathered and  x (m + log sum_k exp(s_k - m)) - sum_k E E  is formed with a
//              DPP max and two DPP sums.  Log-sum-exp, not a dot product of exp(E log) tables: with a small prior shape
//              psi(a) ~ -1/a and the product of two such entries underflows in fp32.  lgamma(x + 1) by the lane that
//              loaded x, in double (gamma_log_factorial).  No atomics: the tasks of a split row leave partial sums that one thread adds in slot
//              order.

// psi(x), x > 0: psi(x) = psi(x + n) - sum_{j<n} 1/(x + j) up to x + n >= 10, then the asymptotic series
//     ln x - 1/(2x) - sum_{n=1..6} B_2n / (2n x^2n).
// The series' error is below its first omitted term, 1/(12 x^14) <= 8.4e-16 at x >= 10 -- under one ulp of
// psi(10) = 2.25, so far below the 1e-11 relative bound of the tests that the shift needs no tuning; at most ten
// recurrence steps (the loop is counted: a shape that is not positive gives a meaningless value, never a hang).
__device__ __forceinline__ double gamma_digamma(double x) {
    double shift = 0.0;
    for (int n = 0; n < 10 && x < 10.0; ++n) {
        shift += 1.0 / x;
        x += 1.0;
    }
    const double r = 1.0 / x, r2 = r * r;
    const double s = r2 * (1.0 / 12 - r2 * (1.0 / 120 - r2 * (1.0 / 252 - r2 * (1.0 / 240 - r2 * (1.0 / 132 - r2 * (691.0 / 32760))))));
    return log(x) - 0.5 * r - s - shift;
}

// lgamma(x + 1) of a rating x >= 0, for the data pass: x + 1 is shifted up to y >= 10 (at most nine factors, their
// product stays below 1e10), then Stirling's series (y - 1/2) ln y - y + ln(2 pi)/2 + sum_{n=1..6} B_2n / (2n (2n - 1) y^(2n-1)),
// whose first omitted term is 1/(156 y^13) <= 6.4e-16.  Ratings 0 and 1 give exactly 0, as lgamma does.  The library's
// lgamma stays out of this kernel: its coefficient tables are loop-invariant, the compiler keeps them in registers across
// the rating loop and the fp32 kernel needs 204 VGPRs (2 waves per SIMD) instead of 68 (7 waves).
__device__ __forceinline__ double gamma_log_factorial(double x) {
    double y = x + 1.0;
    if (y == 1.0 || y == 2.0) return 0.0;
    double prod = 1.0;
    for (int n = 0; n < 9 && y < 10.0; ++n) {
        prod *= y;
        y += 1.0;
    }
    const double r = 1.0 / y, r2 = r * r;
    const double s = r * (1.0 / 12 - r2 * (1.0 / 360 - r2 * (1.0 / 1260 - r2 * (1.0 / 1680 - r2 * (1.0 / 1188 - r2 * (691.0 / 360360))))));
    return (y - 0.5) * log(y) - y + 0.91893853320467274178 + s - log(prod);
}

// max over the lane group (group_sum's moves)
template <int LANES, typename T>
__device__ __forceinline__ T group_max(T x) {
    if constexpr (LANES >= 2) x = vmax(x, dpp_move<0xB1>(x));
    if constexpr (LANES >= 4) x = vmax(x, dpp_move<0x4E>(x));
    if constexpr (LANES >= 8) x = vmax(x, dpp_move<0x141>(x));
    if constexpr (LANES >= 16) x = vmax(x, dpp_move<0x140>(x));
    if constexpr (LANES >= 32) x = vmax(x, __shfl_xor(x, 16, 64));
    if constexpr (LANES >= 64) x = vmax(x, __shfl_xor(x, 32, 64));
    return x;
}

template <typename T>
struct GammaElboRowParams {
    const T *shape, *rate;   // [rows][kpad]
    const T *hyper_rate;     // [rows], or null: not hierarchical
    T *table;                // [rows][2][kpad]
    double *out;             // [rows][PMF_GAMMA_ELBO_TERMS], or null: the table only (the other side of a data call)
    const double *colsum;    // [kpad] column sums of the other side's E, or null.  PMF_ZEROS_OBSERVED: DATA starts at -E_r . C
    int64_t rows;
    int K, kpad;
};

template <typename T, int LPR>
__global__ __launch_bounds__(256) void gamma_elbo_row_kernel(GammaElboRowParams<T> p) {
    constexpr int G = 256 / LPR;
    const int c = threadIdx.x % LPR;
    const int64_t row = (int64_t)blockIdx.x * G + threadIdx.x / LPR;
    if (row >= p.rows) return;
    const int koff = c * PMF_VEC;
    const bool active = koff < p.kpad;
    Vec4<T> a4 = zero4<T>(), b4 = zero4<T>();
    if (active) {
        a4 = load4(p.shape + row * p.kpad + koff);
        b4 = load4(p.rate + row * p.kpad + koff);
    }
    Vec4<T> elog, ex;
    double sum_e = 0.0, sum_elog = 0.0, entropy = 0.0, zeros = 0.0;
#pragma unroll
    for (int e = 0; e < PMF_VEC; ++e) {
        elog.v[e] = (T)(-INFINITY);
        ex.v[e] = (T)0;
        if (active && koff + e < p.K) {
            const double a = (double)a4.v[e], b = (double)b4.v[e];
            const double lb = log(b), psi = gamma_digamma(a), x = a / b, el = psi - lb;
            sum_e += x;
            sum_elog += el;
            if (p.out) entropy += a - lb + lgamma(a) + (1.0 - a) * psi;
            elog.v[e] = (T)el;
            ex.v[e] = (T)x;
            if (p.out && p.colsum) zeros += (double)ex.v[e] * p.colsum[koff + e];   // (the table's E: what C of this side sums)
        }
    }
    if (active) {
        T *dst = p.table + row * 2 * p.kpad + koff;
        store4(dst, elog);
        store4(dst + p.kpad, ex);
    }
    if (!p.out) return;   // (the same in every lane)
    sum_e = group_sum<LPR>(sum_e);
    sum_elog = group_sum<LPR>(sum_elog);
    entropy = group_sum<LPR>(entropy);
    if (p.colsum) zeros = group_sum<LPR>(zeros);   // (the same in every lane)
    if (c == 0) {
        double *o = p.out + row * PMF_GAMMA_ELBO_TERMS;
        o[PMF_GAMMA_ELBO_SUM_FACTOR] = sum_e;
        o[PMF_GAMMA_ELBO_SUM_ELOG] = sum_elog;
        o[PMF_GAMMA_ELBO_ENTROPY] = entropy;
        const bool hier = p.hyper_rate != nullptr;
        const double h = hier ? (double)p.hyper_rate[row] : 1.0;
        o[PMF_GAMMA_ELBO_LOG_HYPER] = hier ? log(h) : 0.0;
        o[PMF_GAMMA_ELBO_INV_HYPER] = hier ? 1.0 / h : 0.0;
        o[PMF_GAMMA_ELBO_FACTOR_OVER_HYPER] = hier ? sum_e / h : 0.0;
        o[PMF_GAMMA_ELBO_DATA] = p.colsum ? -zeros : 0.0;   // (the data pass writes over these two; with `colsum` it adds to DATA)
        o[PMF_GAMMA_ELBO_LOGFACT] = 0.0;
    }
}

template <typename T>
struct GammaElboDataParams {
    const PmfTask *tasks;
    int64_t n_tasks;
    const int32_t *other;
    const T *val;
    const T *table_self, *table_other;   // [rows][2][kpad]
    T *part_data;                        // [n_slots]
    double *part_logfact;                // [n_slots]
    double *out;                         // [rows][PMF_GAMMA_ELBO_TERMS]
    int kpad;
    int zeros;                           // PMF_ZEROS_OBSERVED: no E . E per rating; DATA is added to what the row pass left (-E_r . C)
};

template <typename T, int LPR>
__global__ __launch_bounds__(256) void gamma_elbo_data_kernel(GammaElboDataParams<T> p) {
    constexpr int G = 256 / LPR;
    constexpr int UN = LPR < 4 ? LPR : 4;
    const int c = threadIdx.x % LPR;
    const int64_t task_id = (int64_t)blockIdx.x * G + threadIdx.x / LPR;
    if (task_id >= p.n_tasks) return;
    const PmfTask t = p.tasks[task_id];
    const int koff = c * PMF_VEC;
    const int kpad = p.kpad;
    const bool active = koff < kpad;
    const T ninf = (T)(-INFINITY);

    Vec4<T> sl, se = zero4<T>();   // the row's own E log and E; a lane past kpad holds pads
    sl.v[0] = sl.v[1] = sl.v[2] = sl.v[3] = ninf;
    if (active) {
        const T *src = p.table_self + (int64_t)t.row * 2 * kpad + koff;
        sl = load4(src);
        se = load4(src + kpad);
    }
    T acc = (T)0;
    double logfact = 0.0;
    const int32_t *col = p.other + t.start;
    const T *val = p.val + t.start;

    for (int base = 0; base < t.len; base += LPR) {
        const int n = min(LPR, t.len - base);
        int my_o = 0;
        T my_x = (T)0;
        if (c < n) {
            my_o = col[base + c];
            my_x = val[base + c];
            logfact += gamma_log_factorial((double)my_x);
        }
        for (int tt = 0; tt < n; tt += UN) {
            int o[UN];
            T xv[UN];
            Vec4<T> bl[UN], be[UN];
#pragma unroll
            for (int q = 0; q < UN; ++q) {
                o[q] = __shfl(my_o, tt + q, LPR);   // (lanes past the batch hold id 0: a valid row, loaded and not used)
                xv[q] = __shfl(my_x, tt + q, LPR);
            }
#pragma unroll
            for (int q = 0; q < UN; ++q) {
                bl[q] = sl;   // (-inf in every element: what an inactive lane contributes)
                be[q] = zero4<T>();
                if (active) {
                    const T *src = p.table_other + (int64_t)o[q] * 2 * kpad + koff;
                    bl[q] = load4(src);
                    if (!p.zeros) be[q] = load4(src + kpad);   // (else d below is 0: the row pass has the product over ALL cells)
                }
            }
#pragma unroll
            for (int q = 0; q < UN; ++q) {
                if (tt + q < n) {
                    T s[PMF_VEC];
#pragma unroll
                    for (int e = 0; e < PMF_VEC; ++e) s[e] = sl.v[e] + bl[q].v[e];
                    const T m = group_max<LPR>(vmax(vmax(s[0], s[1]), vmax(s[2], s[3])));
                    T z = exp(s[0] - m);   // (a pad is -inf: exp gives 0)
                    z += exp(s[1] - m);
                    z += exp(s[2] - m);
                    z += exp(s[3] - m);
                    T d = be[q].v[0] * se.v[0];
                    d = fma(be[q].v[1], se.v[1], d);
                    d = fma(be[q].v[2], se.v[2], d);
                    d = fma(be[q].v[3], se.v[3], d);
                    z = group_sum<LPR>(z);
                    d = group_sum<LPR>(d);
                    acc += xv[q] * (m + log(z)) - d;
                }
            }
        }
    }
    logfact = group_sum<LPR>(logfact);
    if (c != 0) return;
    if (t.slot >= 0) {
        p.part_data[t.slot] = acc;
        p.part_logfact[t.slot] = logfact;
    } else {
        double *o = p.out + (int64_t)t.row * PMF_GAMMA_ELBO_TERMS;
        o[PMF_GAMMA_ELBO_DATA] = p.zeros ? o[PMF_GAMMA_ELBO_DATA] + (double)acc : (double)acc;
        o[PMF_GAMMA_ELBO_LOGFACT] = logfact;
    }
}

// one thread per split row: its partial sums in slot order
template <typename T>
__global__ void gamma_elbo_split_kernel(const PmfSplitRow *split, int64_t n_split, const T *part_data, const double *part_logfact,
                                        double *out, int zeros) {
    const int64_t at = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (at >= n_split) return;
    const PmfSplitRow sr = split[at];
    T d = (T)0;
    double lf = 0.0;
    for (int s = 0; s < sr.n_slots; ++s) {
        d += part_data[sr.first_slot + s];
        lf += part_logfact[sr.first_slot + s];
    }
    double *o = out + (int64_t)sr.row * PMF_GAMMA_ELBO_TERMS;
    o[PMF_GAMMA_ELBO_DATA] = zeros ? o[PMF_GAMMA_ELBO_DATA] + (double)d : (double)d;
    o[PMF_GAMMA_ELBO_LOGFACT] = lf;
}

// gamma_elbo_row_kernel over the rows of side `s`: their (E log, E) table into `table` and, with `out`, the per-row
// terms (`hierarchical`: those of HYPER_RATE among them).  The caller holds the profile bracket and checks the launch.
template <typename T, int LPR>
static void launch_gamma_row_table(pmf_ctx *ctx, int s, T *table, double *out, bool hierarchical, const double *colsum = nullptr) {
    constexpr int G = 256 / LPR;
    GammaElboRowParams<T> r;
    r.shape = ctx->arr[s][PMF_ARR_SHAPE].as<const T>();
    r.rate = ctx->arr[s][PMF_ARR_RATE].as<const T>();
    r.hyper_rate = hierarchical ? ctx->arr[s][PMF_ARR_HYPER_RATE].as<const T>() : nullptr;
    r.table = table;
    r.out = out;
    r.colsum = colsum;
    r.rows = ctx->rows[s];
    r.K = ctx->K;
    r.kpad = ctx->kpad;
    if (r.rows > 0)
        hipLaunchKernelGGL((gamma_elbo_row_kernel<T, LPR>), dim3((unsigned)((r.rows + G - 1) / G)), dim3(256), 0, ctx->stream, r);
}

// Everything the call writes lives in the context's scratch buffer (grown once, kept): the per-row terms, both tables
// and the split rows' partial sums.  The row pass is timed as PMF_KERNEL_GAMMA_FINAL (with the split rows' sums), the
// data pass as PMF_KERNEL_GAMMA_SWEEP.
template <typename T>
static int run_gamma_elbo_terms(pmf_ctx *ctx, int side, bool with_data, bool hierarchical, double *totals, double *per_row) {
    const int other = 1 - side, kpad = ctx->kpad;
    const int64_t rows = ctx->rows[side], rows_o = ctx->rows[other];
    const int lpr = pmf_lanes_per_row(kpad);
    PmfTaskView tl;
    if (with_data) tl = pmf_task_view(ctx, side, ctx->index[side].gamma_tasks, false);
    PmfLayout lay(256);
    const auto out_at = lay.add<double>((size_t)rows * PMF_GAMMA_ELBO_TERMS);
    const auto lf_at = lay.add<double>((size_t)tl.n_slots);
    const auto pd_at = lay.add<T>((size_t)tl.n_slots);
    const auto self_at = lay.add<T>((size_t)rows * 2 * kpad);
    const auto other_at = lay.add<T>(with_data ? (size_t)rows_o * 2 * kpad : 0);
    // unlisted cells as zeros: sum over ALL cells of E_r . E_o = E_r . C, C the column sums of the other side's E half
    const bool zeros = with_data && gamma_zeros_observed(ctx);
    const GammaColsum<T> cs(lay, kpad, zeros);   // (the default mode's scratch layout stays what it was)
    int rc;
    if ((rc = pmf_ensure_scratch(ctx, lay.bytes()))) return rc;
    void *base = ctx->d_scratch.as();
    double *d_out = out_at.at(base), *d_lf = lf_at.at(base);
    T *d_pd = pd_at.at(base), *d_self = self_at.at(base), *d_other = other_at.at(base);

    GammaElboDataParams<T> d;
    d.tasks = tl.d_tasks;
    d.n_tasks = tl.n_tasks;
    d.other = ctx->index[side].d_other.as<int32_t>();
    d.val = ctx->index[side].d_val.as<const T>();
    d.table_self = d_self;
    d.table_other = d_other;
    d.part_data = d_pd;
    d.part_logfact = d_lf;
    d.out = d_out;
    d.kpad = kpad;
    d.zeros = zeros;
    pmf_with_pow2<1>(lpr, [&](auto L) {
        constexpr int G = 256 / L;
        if (rows > 0) {
            PmfProfScope prof(ctx, PMF_KERNEL_GAMMA_FINAL);
            if (with_data) launch_gamma_row_table<T, L>(ctx, other, d_other, nullptr, false);   // the other side: its table only
            if (zeros) cs.launch(ctx, base, d_other + kpad, rows_o, 2 * (int64_t)kpad);   // (inside this bracket: the row pass)
            launch_gamma_row_table<T, L>(ctx, side, d_self, d_out, hierarchical, zeros ? cs.sum_at.at(base) : nullptr);
        }
        if (with_data && tl.n_tasks > 0) {
            PmfProfScope prof(ctx, PMF_KERNEL_GAMMA_SWEEP);
            hipLaunchKernelGGL((gamma_elbo_data_kernel<T, L>), dim3((unsigned)((tl.n_tasks + G - 1) / G)), dim3(256), 0, ctx->stream, d);
        }
        if (with_data && tl.n_split > 0) {
            PmfProfScope prof(ctx, PMF_KERNEL_GAMMA_FINAL);
            hipLaunchKernelGGL((gamma_elbo_split_kernel<T>), dim3((unsigned)((tl.n_split + 255) / 256)), dim3(256), 0, ctx->stream,
                               tl.d_split, tl.n_split, d_pd, d_lf, d_out, (int)zeros);
        }
    });
    PMF_HIP_CHECK(hipGetLastError());
    // per-row terms to the host; the totals are their sums in row order
    std::vector<double> host;
    double *dst = per_row;
    if (!dst) {
        host.resize((size_t)rows * PMF_GAMMA_ELBO_TERMS);
        dst = host.data();
    }
    if (rows > 0)
        PMF_HIP_CHECK(hipMemcpyAsync(dst, d_out, (size_t)rows * PMF_GAMMA_ELBO_TERMS * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    PMF_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    double sum[PMF_GAMMA_ELBO_TERMS] = {};
    for (int64_t row = 0; row < rows; ++row)
        for (int t = 0; t < PMF_GAMMA_ELBO_TERMS; ++t) sum[t] += dst[row * PMF_GAMMA_ELBO_TERMS + t];
    std::copy_n(sum, PMF_GAMMA_ELBO_TERMS, totals);
    return PMF_OK;
}

extern "C" int pmf_gamma_elbo_terms(pmf_ctx *ctx, int side, int with_data, int hierarchical, double *totals, double *per_row) {
    PMF_SIDE_ENTRY("pmf_gamma_elbo_terms");
    PMF_REQUIRE(totals, PMF_EINVAL, "pmf_gamma_elbo_terms: null totals");
    if (with_data) PMF_REQUIRE_UNWEIGHTED("pmf_gamma_elbo_terms");
    int rc;
    if ((rc = require_gamma_q(ctx, {side}, "pmf_gamma_elbo_terms"))) return rc;
    if (with_data) {
        if ((rc = require_gamma_q(ctx, {1 - side}, "pmf_gamma_elbo_terms"))) return rc;
        PMF_REQUIRE(ctx->index[side].d_ptr, PMF_EINVAL, "pmf_gamma_elbo_terms: ratings have not been set");
    }
    if (hierarchical && (rc = pmf_require_array(ctx, side, PMF_ARR_HYPER_RATE, "pmf_gamma_elbo_terms (hierarchical)"))) return rc;
    return pmf_no_throw("pmf_gamma_elbo_terms", [&] {
        return pmf_with_dtype(ctx, [&](auto t) {
            return run_gamma_elbo_terms<decltype(t)>(ctx, side, with_data != 0, hierarchical != 0, totals, per_row);
        });
    });
}

// ---------------------------------------------------------------------------
// exact coordinate-ascent half-sweep (pmf_gamma_exact_sweep / pmf_gamma_exact_accumulate)
// ---------------------------------------------------------------------------
// The statistics of pmf_gamma_sweep with the weights of coordinate ascent on the bound: phi_jk = exp(s_jk - lse_j),
// s_jk = Elog_side[r,k] + Elog_other[o_j,k], instead of E E / (E . E).  Both tables come from gamma_elbo_row_kernel
// (psi in double) and are rebuilt by every call from SHAPE and RATE as they are, into a buffer of their own
// (pmf_ctx::d_gamma_tables: pmf_gamma_elbo_terms writes the scratch buffer and cannot touch them).  The access shape is
// gamma_elbo_data_kernel's: a lane group per task, the row's own E log in registers, the other row's (E log, E) pair
// gathered from one 2 kpad block, UN gathers in flight.  Per rating one DPP max, one exp per element -- the same
// e_k = exp(s_k - m) is the normaliser's addend and the weight's numerator -- one DPP sum and one division.
// Log-sum-exp, not a dot product of exp(E log) tables, for the reason given at the ELBO data pass.  A pad is -inf in
// the E log half and 0 in the E half: it adds 0 to both sums.  The epilogue is gamma_sweep_kernel's.
template <typename T, int LPR, bool STATS>
__global__ __launch_bounds__(256) void gamma_exact_kernel(GammaParams<T> p, const T *table_self, const T *table_other) {
    constexpr int G = 256 / LPR;
    constexpr int UN = LPR < 4 ? LPR : 4;
    const int c = threadIdx.x % LPR;
    const int64_t task_id = (int64_t)blockIdx.x * G + threadIdx.x / LPR;
    if (task_id >= p.n_tasks) return;
    const PmfTask t = p.tasks[task_id];
    const int koff = c * PMF_VEC;
    const int kpad = p.kpad;
    const bool active = koff < kpad;
    const T ninf = (T)(-INFINITY);

    Vec4<T> sl;   // the row's own E log; a lane past kpad holds pads
    sl.v[0] = sl.v[1] = sl.v[2] = sl.v[3] = ninf;
    if (active) sl = load4(table_self + (int64_t)t.row * 2 * kpad + koff);
    Vec4<T> acc_a = zero4<T>(), acc_b = zero4<T>();
    const int32_t *col = p.other + t.start;
    const T *val = p.val + t.start;

    for (int base = 0; base < t.len; base += LPR) {
        const int n = min(LPR, t.len - base);
        int my_o = 0;
        T my_x = (T)0;
        if (c < n) {
            my_o = col[base + c];
            my_x = val[base + c];
        }
        for (int tt = 0; tt < n; tt += UN) {
            int o[UN];
            T xv[UN];
            Vec4<T> bl[UN], be[UN];
#pragma unroll
            for (int q = 0; q < UN; ++q) {
                o[q] = __shfl(my_o, tt + q, LPR);   // (lanes past the batch hold id 0: a valid row, loaded and not used)
                xv[q] = __shfl(my_x, tt + q, LPR);
            }
#pragma unroll
            for (int q = 0; q < UN; ++q) {
                bl[q] = sl;   // (-inf in every element: what an inactive lane contributes)
                be[q] = zero4<T>();
                if (active) {
                    const T *src = table_other + (int64_t)o[q] * 2 * kpad + koff;
                    bl[q] = load4(src);
                    be[q] = load4(src + kpad);
                }
            }
#pragma unroll
            for (int q = 0; q < UN; ++q) {
                if (tt + q < n) {
                    T s[PMF_VEC], ex[PMF_VEC];
#pragma unroll
                    for (int e = 0; e < PMF_VEC; ++e) s[e] = sl.v[e] + bl[q].v[e];
                    const T m = group_max<LPR>(vmax(vmax(s[0], s[1]), vmax(s[2], s[3])));
#pragma unroll
                    for (int e = 0; e < PMF_VEC; ++e) ex[e] = exp(s[e] - m);   // (a pad is -inf: exp gives 0)
                    T z = ex[0];
                    z += ex[1];
                    z += ex[2];
                    z += ex[3];
                    z = group_sum<LPR>(z);   // >= 1: the largest element adds exp(0)
                    const T w = xv[q] / z;
#pragma unroll
                    for (int e = 0; e < PMF_VEC; ++e) {
                        acc_a.v[e] += w * ex[e];
                        acc_b.v[e] += be[q].v[e];
                    }
                }
            }
        }
    }

    if (t.slot >= 0) {
        if (active) {
            T *slot = p.partial + (int64_t)t.slot * p.pw;
            store4(slot + koff, acc_a);
            store4(slot + kpad + koff, acc_b);
        }
    } else if (STATS) {
        if (active) {
            T *dst = p.stats + (int64_t)t.row * 2 * kpad + koff;
            store4(dst, acc_a);
            store4(dst + kpad, acc_b);
        }
    } else {
        gamma_finalize_row<T, LPR, false>(p, t.row, c, active, acc_a, acc_b, (T)0, t.len == 0);
    }
}

static int check_gamma_exact_inputs(pmf_ctx *ctx, int side, const char *what) {
    int rc;
    if ((rc = require_gamma_q(ctx, {side, 1 - side}, what))) return rc;
    PMF_REQUIRE(ctx->index[side].d_ptr, PMF_EINVAL, "%s: ratings have not been set", what);
    return PMF_OK;
}

// the user table, then the item table: the same bytes whichever side a call sweeps, so the buffer grows once
template <typename T>
static T *gamma_exact_table(const pmf_ctx *ctx, int side) {
    return ctx->d_gamma_tables.as<T>() + (side == PMF_SIDE_USER ? 0 : (size_t)ctx->rows[PMF_SIDE_USER] * 2 * ctx->kpad);
}

// Both sides' (E log, E) tables from SHAPE and RATE as they are now, on the context's stream (timed as the row pass).
template <typename T>
static int gamma_exact_build_tables(pmf_ctx *ctx, std::initializer_list<int> sides = {PMF_SIDE_USER, PMF_SIDE_ITEM}) {
    int rc;
    if ((rc = ctx->d_gamma_tables.reserve(ctx, (size_t)(ctx->rows[0] + ctx->rows[1]) * 2 * ctx->kpad * sizeof(T), {ctx->stream}))) return rc;
    PmfProfScope prof(ctx, PMF_KERNEL_GAMMA_FINAL);
    pmf_with_pow2<1>(pmf_lanes_per_row(ctx->kpad), [&](auto L) {
        for (int s : sides) launch_gamma_row_table<T, L>(ctx, s, gamma_exact_table<T>(ctx, s), nullptr, false);
    });
    PMF_HIP_CHECK(hipGetLastError());
    return PMF_OK;
}

// PMF_PASS_FUSED or PMF_PASS_ACCUMULATE (finalize is run_gamma's).  The caller has checked the inputs and, with
// `tables` false, built the tables itself.
template <typename T>
static int run_gamma_exact(pmf_ctx *ctx, int side, PmfPass pass, bool tables, void *stats, const GammaPriors &pr) {
    const PmfTaskView tl = pmf_task_view(ctx, side, ctx->index[side].gamma_tasks, pass != PMF_PASS_FUSED);
    int rc;
    pmf_factor_written(ctx);
    if (pass == PMF_PASS_FUSED) {
        if ((rc = pmf_alloc_array(ctx, side, PMF_ARR_FACTOR))) return rc;   // (written, never read)
        if (pr.hierarchical && (rc = pmf_alloc_array(ctx, side, PMF_ARR_HYPER_RATE))) return rc;
    }
    const int pw = 2 * ctx->kpad;
    if (tl.n_slots > 0 && (rc = pmf_ensure_partial(ctx, (size_t)tl.n_slots * pw * sizeof(T)))) return rc;
    if (tables && (rc = gamma_exact_build_tables<T>(ctx))) return rc;
    GammaParams<T> p = gamma_params<T>(ctx, side, tl, stats, pr, pw);
    const T *table_self = gamma_exact_table<T>(ctx, side), *table_other = gamma_exact_table<T>(ctx, 1 - side);
    // unlisted cells as zeros (fused pass only): every row's rate sum is the column sum of the other table's E half
    if (gamma_zeros_observed(ctx) && pass == PMF_PASS_FUSED &&
        (rc = gamma_colsum_scratch<T>(ctx, table_other + ctx->kpad, ctx->rows[1 - side], 2 * (int64_t)ctx->kpad, nullptr, &p.colsum)))
        return rc;
    return gamma_launch(ctx, [&](auto L) {
        if (pass == PMF_PASS_ACCUMULATE)   // (the split kernel is the reference sweep's)
            launch_gamma<T, L, true, false, gamma_exact_kernel<T, L, true>>(ctx, p, tl, table_self, table_other);
        else
            launch_gamma<T, L, false, false, gamma_exact_kernel<T, L, false>>(ctx, p, tl, table_self, table_other);
    });
}

extern "C" int pmf_gamma_exact_sweep(pmf_ctx *ctx, int side, double shape_prior, double rate_prior,
                                     int hierarchical, double hyper_shape, double hyper_rate_prior) {
    PMF_SIDE_ENTRY("pmf_gamma_exact_sweep");
    PMF_REQUIRE_UNWEIGHTED("pmf_gamma_exact_sweep");
    const GammaPriors pr = {shape_prior, rate_prior, hierarchical, hyper_shape, hyper_rate_prior};
    int rc;
    if ((rc = check_gamma_exact_inputs(ctx, side, "pmf_gamma_exact_sweep"))) return rc;
    if (hierarchical && (rc = pmf_require_array(ctx, side, PMF_ARR_PRIOR_RATE, "pmf_gamma_exact_sweep (hierarchical)"))) return rc;
    return pmf_with_dtype(ctx, [&](auto t) {
        using T = decltype(t);
        if (side != PMF_SIDE_ITEM || !pmf_comm_active(ctx)) return run_gamma_exact<T>(ctx, side, PMF_PASS_FUSED, true, nullptr, pr);
        // several ranks: pmf_gamma_sweep's exchange with the exact accumulate; the tables are built once, on the compute
        // stream, before the first chunk (finalize writes SHAPE and RATE of chunk c while later chunks still read the tables)
        int rc;
        if ((rc = gamma_exact_build_tables<T>(ctx))) return rc;
        return gamma_comm_half_sweep<T>(ctx, side, pr, {PMF_ARR_FACTOR, PMF_ARR_HYPER_RATE}, [&](void *s) {
            return run_gamma_exact<T>(ctx, side, PMF_PASS_ACCUMULATE, false, s, GammaPriors());
        });
    });
}

extern "C" int pmf_gamma_exact_accumulate(pmf_ctx *ctx, int side, void *stats_dev) {
    PMF_SIDE_ENTRY("pmf_gamma_exact_accumulate");
    PMF_REQUIRE_UNWEIGHTED("pmf_gamma_exact_accumulate");
    PMF_REQUIRE_ZEROS_MISSING("pmf_gamma_exact_accumulate");
    PMF_REQUIRE(stats_dev, PMF_EINVAL, "pmf_gamma_exact_accumulate: null stats buffer");
    int rc;
    if ((rc = check_gamma_exact_inputs(ctx, side, "pmf_gamma_exact_accumulate"))) return rc;
    return pmf_with_dtype(ctx, [&](auto t) { return run_gamma_exact<decltype(t)>(ctx, side, PMF_PASS_ACCUMULATE, true, stats_dev, {}); });
}

// C_k of `side`: the column sums of FACTOR, or (from_q) of the E half of the side's freshly built (E log, E) table
extern "C" int pmf_gamma_column_sums(pmf_ctx *ctx, int side, int from_q, double *out) {
    PMF_SIDE_ENTRY("pmf_gamma_column_sums");
    PMF_REQUIRE(out != nullptr, PMF_EINVAL, "pmf_gamma_column_sums: null out");
    int rc;
    if (from_q) {
        if ((rc = require_gamma_q(ctx, {side}, "pmf_gamma_column_sums"))) return rc;
    } else if ((rc = pmf_require_array(ctx, side, PMF_ARR_FACTOR, "pmf_gamma_column_sums"))) {
        return rc;
    }
    return pmf_with_dtype(ctx, [&](auto t) {
        using T = decltype(t);
        int rc;
        const T *src = ctx->arr[side][PMF_ARR_FACTOR].as<const T>();
        int64_t stride = ctx->kpad;
        if (from_q) {
            if ((rc = gamma_exact_build_tables<T>(ctx, {side}))) return rc;
            src = gamma_exact_table<T>(ctx, side) + ctx->kpad;
            stride = 2 * (int64_t)ctx->kpad;
        }
        const double *sum = nullptr;
        if ((rc = gamma_colsum_scratch<T>(ctx, src, ctx->rows[side], stride, &sum, nullptr))) return rc;
        PMF_HIP_CHECK(hipMemcpyAsync(out, sum, (size_t)ctx->K * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        PMF_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        return PMF_OK;
    });
}

// ---------------------------------------------------------------------------
// exact fold-in (pmf_gamma_fold_in_exact): the n_iter passes of coordinate ascent on the bound for NEW rows
// ---------------------------------------------------------------------------
// gamma_fold_kernel's access shape (a lane group owns a row for the whole call, lane c owns elements 4c .. 4c+3, ids and
// ratings handed out by __shfl, UN gathers in flight, LONG = true: a block per row, group partials added through LDS in
// group order) around gamma_exact_kernel's inner loop (the other row's (E log, E) pair gathered from one 2 kpad block;
// per rating a DPP max, one exp per element, a DPP sum, w = x / z; pads are -inf / 0).  What is new lies between the
// passes: the row's own E log = psi(s) - log r is re-formed in registers from the s and r the pass before left there --
// psi and log in double (gamma_digamma, the statement of gamma_elbo_row_kernel), rounded once to T -- so s, r, B, rho and
// h never leave the lanes, the E half is gathered in the first pass only (B is summed there), and nothing is written
// before the end.  No atomics.

// psi(a) - log(b) in double: the statement of gamma_elbo_row_kernel.  Not inlined: four copies of the shift loop and the
// two logarithms per pass keep enough masks and constants alive across the rating loop to spill SGPRs.
__device__ __noinline__ double gamma_fold_exact_elog1(double a, double b) {
    const double lb = log(b), psi = gamma_digamma(a);
    return psi - lb;
}

// e_k = exp(s_k - m) of the lane's four elements.  The double form is not inlined, as gamma_pred_exp_sum's is not: four
// inlined double exponentials per gathered row in flight cost the fp64 kernels SGPR spills.
__device__ __forceinline__ Vec4<float> gamma_fold_exact_exp(float s0, float s1, float s2, float s3, float m) {
    Vec4<float> ex;
    ex.v[0] = exp(s0 - m); ex.v[1] = exp(s1 - m); ex.v[2] = exp(s2 - m); ex.v[3] = exp(s3 - m);
    return ex;
}
__device__ __noinline__ Vec4<double> gamma_fold_exact_exp(double s0, double s1, double s2, double s3, double m) {
    Vec4<double> ex;
    ex.v[0] = exp(s0 - m); ex.v[1] = exp(s1 - m); ex.v[2] = exp(s2 - m); ex.v[3] = exp(s3 - m);
    return ex;
}

// l = psi(shape) - log(rate) of the lane's four elements; a pad (and every element of a lane past kpad) is -inf
template <typename T>
__device__ __forceinline__ Vec4<T> gamma_fold_exact_elog(const GammaFoldParams<T> &p, int c, bool active, const Vec4<T> &shape,
                                                         const Vec4<T> &rate) {
    const int koff = c * PMF_VEC;
    Vec4<T> l;
#pragma unroll
    for (int e = 0; e < PMF_VEC; ++e) {
        l.v[e] = (T)(-INFINITY);
        if (active && koff + e < p.K) l.v[e] = (T)gamma_fold_exact_elog1((double)shape.v[e], (double)rate.v[e]);
    }
    return l;
}

// s^0, r^0 and rho^0 of a row (theta and h are set by the first update)
template <typename T>
__device__ __forceinline__ GammaFoldRow<T> gamma_fold_exact_start(const GammaFoldExactParams<T> &p, int64_t row, int c, bool active) {
    const int koff = c * PMF_VEC;
    GammaFoldRow<T> st;
    st.hyper = (T)0;
    st.rho = !p.hierarchical ? p.rate_prior : p.init_prior_rate ? p.init_prior_rate[row] : p.hyper_shape / p.hyper_rate_prior;
    st.theta = zero4<T>();
    if (p.init_shape) {   // (staged with zero pad elements)
        st.shape = active ? load4(p.init_shape + row * p.kpad + koff) : zero4<T>();
        st.rate = active ? load4(p.init_rate + row * p.kpad + koff) : zero4<T>();
    } else {
#pragma unroll
        for (int e = 0; e < PMF_VEC; ++e) {
            const bool ok = active && koff + e < p.K;
            st.shape.v[e] = ok ? p.shape_prior : (T)0;
            st.rate.v[e] = ok ? st.rho : (T)0;
        }
    }
    return st;
}

// The ratings [0, n) of one row in batches of LPR, batch `first`, first + step, ...: acc += x_j phi_j with
// phi_jk = exp(sl_k + L_{o_j k} - lse_j) and, in the call's first pass (`with_b`), bsum += E_{o_j}.  The statements per
// rating are gamma_exact_kernel's, in its order.  All lanes of the group call it together.
template <typename T, int LPR>
__device__ __forceinline__ void gamma_fold_exact_pass(const GammaFoldExactParams<T> &p, const int32_t *col, const T *val, int64_t n,
                                                      int first, int step, int c, bool active, bool with_b, const Vec4<T> &sl,
                                                      Vec4<T> &acc, Vec4<T> &bsum) {
    constexpr int UN = LPR < 4 ? LPR : 4;
    const int koff = c * PMF_VEC;
    const int kpad = p.kpad;
    for (int64_t base = (int64_t)first * LPR; base < n; base += (int64_t)step * LPR) {
        const int cnt = (int)min((int64_t)LPR, n - base);
        int my_o = 0;
        T my_x = (T)0;
        if (c < cnt) {
            my_o = col[base + c];
            my_x = val[base + c];
        }
        for (int tt = 0; tt < cnt; tt += UN) {
            int o[UN];
            T xv[UN];
            Vec4<T> bl[UN], be[UN];
#pragma unroll
            for (int q = 0; q < UN; ++q) {
                o[q] = __shfl(my_o, tt + q, LPR);   // (lanes past the batch hold id 0: a valid row, loaded and not used)
                xv[q] = __shfl(my_x, tt + q, LPR);
            }
#pragma unroll
            for (int q = 0; q < UN; ++q) {
                bl[q] = sl;   // (-inf in every element: what an inactive lane contributes)
                be[q] = zero4<T>();
                if (active) {
                    const T *src = p.table_other + (int64_t)o[q] * 2 * kpad + koff;
                    bl[q] = load4(src);
                    if (with_b) be[q] = load4(src + kpad);   // (the same in every lane)
                }
            }
#pragma unroll
            for (int q = 0; q < UN; ++q) {
                if (tt + q < cnt) {
                    T s[PMF_VEC];
#pragma unroll
                    for (int e = 0; e < PMF_VEC; ++e) s[e] = sl.v[e] + bl[q].v[e];
                    const T m = group_max<LPR>(vmax(vmax(s[0], s[1]), vmax(s[2], s[3])));
                    const Vec4<T> ex = gamma_fold_exact_exp(s[0], s[1], s[2], s[3], m);   // (a pad is -inf: exp gives 0)
                    T z = ex.v[0];
                    z += ex.v[1];
                    z += ex.v[2];
                    z += ex.v[3];
                    z = group_sum<LPR>(z);   // >= 1: the largest element adds exp(0)
                    const T w = xv[q] / z;
#pragma unroll
                    for (int e = 0; e < PMF_VEC; ++e) {
                        acc.v[e] += w * ex.v[e];
                        if (with_b) bsum.v[e] += be[q].v[e];
                    }
                }
            }
        }
    }
}

// `ptr` lives in vector registers from here on (an empty statement the compiler cannot see through)
template <typename T>
__device__ __forceinline__ void gamma_fold_hold(T *&ptr) {
    asm volatile("" : "+v"(ptr));
}

template <typename T, int LPR, bool LONG>
__global__ __launch_bounds__(256) void gamma_fold_exact_kernel(GammaFoldExactParams<T> p) {
    constexpr int G = 256 / LPR;
    const int c = threadIdx.x % LPR;
    const int g = threadIdx.x / LPR;
    const int koff = c * PMF_VEC;
    const int kpad = p.kpad;
    const bool active = koff < kpad;
    if constexpr (!LONG) {
        const int64_t at = (int64_t)blockIdx.x * G + g;
        if (at >= p.n) return;
        const int64_t row = p.rows[at];
        const int64_t start = p.ptr[row], n = p.ptr[row + 1] - start;
        const int32_t *col = p.other + start;
        const T *val = p.val + start;
        GammaFoldRow<T> st = gamma_fold_exact_start(p, row, c, active);
        Vec4<T> bsum = (p.colsum && active) ? load4(p.colsum + koff) : zero4<T>();
        for (int t = 0; t < p.n_iter; ++t) {
            const Vec4<T> sl = gamma_fold_exact_elog<T>(p, c, active, st.shape, st.rate);
            Vec4<T> acc = zero4<T>();
            gamma_fold_exact_pass<T, LPR>(p, col, val, n, 0, 1, c, active, t == 0 && !p.colsum, sl, acc, bsum);
            gamma_fold_update<T, LPR>(p, c, active, acc, bsum, st);
        }
        gamma_fold_store(p, row, c, active, st);
    } else {
        // gamma_fold_kernel's block variant: one block per row (the grid is the long list exactly: every thread reaches
        // every barrier); every group adds the G partials in group order and so holds the same s, r, rho -- and forms
        // the same E log from them -- bit for bit, without a broadcast.
        extern __shared__ __align__(16) unsigned char smem_raw[];
        T *part = reinterpret_cast<T *>(smem_raw);   // [G][kpad] shape partials, then [G][kpad] sum_j E_{o_j} partials (first pass)
        const int64_t row = p.rows[blockIdx.x];
        const int64_t start = p.ptr[row], n = p.ptr[row + 1] - start;
        const int32_t *col = p.other + start;
        const T *val = p.val + start;
        GammaFoldRow<T> st = gamma_fold_exact_start(p, row, c, active);
        Vec4<T> bsum = (p.colsum && active) ? load4(p.colsum + koff) : zero4<T>();
        // The output pointers are read after the last pass only.  They are the same in every lane, so they would hold
        // scalar registers through the rating loop, and with the calls of the double kernels inside it some spill:
        // they wait in vector registers instead.
        GammaFoldParams<T> out = p;
        gamma_fold_hold(out.factor), gamma_fold_hold(out.shape), gamma_fold_hold(out.rate);
        gamma_fold_hold(out.prior_rate), gamma_fold_hold(out.hyper_rate);
        for (int t = 0; t < p.n_iter; ++t) {
            const bool with_b = t == 0 && !p.colsum;   // (the same in every thread)
            const Vec4<T> sl = gamma_fold_exact_elog<T>(p, c, active, st.shape, st.rate);
            Vec4<T> acc = zero4<T>(), bpart = zero4<T>();
            gamma_fold_exact_pass<T, LPR>(p, col, val, n, g, G, c, active, with_b, sl, acc, bpart);
            if (active) {
                store4(part + g * kpad + koff, acc);
                if (with_b) store4(part + (G + g) * kpad + koff, bpart);
            }
            __syncthreads();
            acc = zero4<T>();
            if (active) {
#pragma unroll 4
                for (int s = 0; s < G; ++s) {
                    const Vec4<T> a = load4(part + s * kpad + koff);
#pragma unroll
                    for (int e = 0; e < PMF_VEC; ++e) acc.v[e] += a.v[e];
                    if (with_b) {
                        const Vec4<T> b = load4(part + (G + s) * kpad + koff);
#pragma unroll
                        for (int e = 0; e < PMF_VEC; ++e) bsum.v[e] += b.v[e];
                    }
                }
            }
            gamma_fold_update<T, LPR>(p, c, active, acc, bsum, st);
            __syncthreads();
        }
        if (g == 0) gamma_fold_store(out, row, c, active, st);
    }
}

// the opposite side's table, built once per call into pmf_ctx::d_gamma_tables (at the place gamma_exact_table gives it,
// so the buffer has the size every exact call reserves), and the zero mode's C from its E half
template <typename T>
static int gamma_fold_exact_other(pmf_ctx *ctx, int side, const T **table, const T **colsum) {
    const int other = 1 - side;
    int rc;
    if ((rc = gamma_exact_build_tables<T>(ctx, {other}))) return rc;
    *table = gamma_exact_table<T>(ctx, other);
    if (!gamma_zeros_observed(ctx)) return PMF_OK;
    return gamma_colsum_scratch<T>(ctx, *table + ctx->kpad, ctx->rows[other], 2 * (int64_t)ctx->kpad, nullptr, colsum);
}

template <typename T>
static void launch_gamma_fold_exact(pmf_ctx *ctx, GammaFoldExactParams<T> &p, const int32_t *list, int64_t n_short, int64_t n_long) {
    pmf_with_pow2<1>(pmf_lanes_per_row(p.kpad), [&](auto L) {
        constexpr int G = 256 / L;
        if (n_short > 0) {
            PmfProfScope prof(ctx, PMF_KERNEL_GAMMA_SWEEP);
            p.rows = list;
            p.n = n_short;
            hipLaunchKernelGGL((gamma_fold_exact_kernel<T, L, false>), dim3((unsigned)((n_short + G - 1) / G)), dim3(256), 0, ctx->stream, p);
        }
        if (n_long > 0) {
            PmfProfScope prof(ctx, PMF_KERNEL_GAMMA_FINAL);
            p.rows = list + n_short;
            p.n = n_long;
            hipLaunchKernelGGL((gamma_fold_exact_kernel<T, L, true>), dim3((unsigned)n_long), dim3(256), (size_t)G * 2 * p.kpad * sizeof(T),
                                ctx->stream, p);
        }
    });
}

// ---------------------------------------------------------------------------
// posterior predictive of a pair (pmf_gamma_predictive): mean, variance and three log densities of a count
// ---------------------------------------------------------------------------
// q is SHAPE and RATE of both sides (FACTOR is not read).  A lane group owns a batch of LPR consecutive pairs: lane j
// loads pair j's ids (one coalesced read) and hands them out by __shfl, as the sweeps hand out a task's ratings.  Per
// pair the whole group works in predict_pair's layout: lane c owns elements [4c, 4c + 4) of the four gathered rows (a, b
// of the user, c, d of the item; UN pairs' gathers in flight), forms E_k = (a/b)(c/d) and E_k^2 (1/a + 1/c + 1/(a c)) for
// its elements in the context dtype, and two DPP sums give the pair's mean and variance.  Under BOUND the E log halves
// of the two table rows (gamma_elbo_row_kernel's, psi in double) are gathered as well and lse_k(E log + E log) is a DPP
// max, one exp per element and a DPP sum, as in the ELBO's data pass.  Lane j keeps pair j's three numbers; after the
// batch every lane converts ITS pair's (mean, var) to double and forms every log and lgamma term from those two numbers
// -- what the call returns as mean and var are the bits the densities were formed from -- so the double arithmetic (seven
// logarithms a pair) runs on all lanes of the wavefront instead of on one lane in LPR, and the ratings are read and the
// outputs written one pair per lane, coalesced.  A lane's sums over its pairs, a DPP sum over the group, the groups of a
// block in group order through LDS, the blocks in block order on the host: no atomics, the same bits every time.

// S(y) = sum_{n=1..6} B_2n / (2n (2n - 1) y^(2n-1)), the tail of Stirling's series (gamma_log_factorial's); y >= 10
__device__ __forceinline__ double gamma_stirling_tail(double y) {
    const double r = 1.0 / y, r2 = r * r;
    return r * (1.0 / 12 - r2 * (1.0 / 360 - r2 * (1.0 / 1260 - r2 * (1.0 / 1680 - r2 * (1.0 / 1188 - r2 * (691.0 / 360360))))));
}

// log(1 + t), t > -1, from log alone: with u = fl(1 + t), log(u) t / (u - 1) -- the quotient puts back what the rounding
// of 1 + t lost (t itself where u == 1).  A few ulp.  The library's log1p stays out of the kernel for the reason its
// lgamma does: a second table of coefficients that the compiler keeps in registers across the pair loop.
__device__ __forceinline__ double gamma_log1p(double t) {
    const double u = 1.0 + t;
    return u == 1.0 ? t : log(u) * (t / (u - 1.0));
}

// D(x, r) = lgamma(x + r) - lgamma(r) - x log r, the part of the negative binomial's log density that vanishes as
// r -> inf.  Its three terms are of size r log r and leave x^2 / (2 r): past r ~ 1e8 nothing of D survives in double.
// Stirling's series of both lgammas with the x log r and the r log r parts cancelled by hand gives, for r >= 10,
//     D(x, r) = (x + r - 1/2) log1p(x / r) - x + S(x + r) - S(r),
// whose terms are of size x.  Below 10 both arguments are shifted up by the same n <= 10 steps to s = r + n:
//     D(x, r) = D(x, s) + x log(s / r) - log prod_{j<n} (x + r + j) / (r + j).
__device__ __forceinline__ double gamma_negbin_excess(double x, double r) {
    double s = r, num = 1.0, den = 1.0;
    for (int n = 0; n < 10 && s < 10.0; ++n) {
        num *= x + s;
        den *= s;
        s += 1.0;
    }
    const double d = (x + s - 0.5) * gamma_log1p(x / s) - x + gamma_stirling_tail(x + s) - gamma_stirling_tail(s);
    return s == r ? d : d + x * log(s / r) - log(num / den);
}

template <typename T>
struct GammaPredParams {
    const int32_t *u, *i;   // [n] ids inside the trained dimensions (the host has checked them)
    int64_t n;
    const T *shape_u, *rate_u, *shape_i, *rate_i;   // [rows][kpad]
    const T *table_u, *table_i;                     // [rows][2][kpad], BOUND only
    const double *x;        // [n] ratings, or null: the moments only
    double *mean, *var;     // [n], or null
    double *logp;           // [n][PMF_GAMMA_PRED_KINDS], or null
    double *block_out;      // [grid][PMF_GAMMA_PRED_TOTALS]
    int K, kpad;
};

// this lane's share of the mean and the variance of theta_u . beta_i from its elements of the four rows, in the context
// dtype.  Every operation is rounded on its own (no contraction): the two instantiations of the kernel give the same
// bits, and the tests count the roundings.
template <typename T>
__device__ __forceinline__ void gamma_pred_moments(const Vec4<T> &a, const Vec4<T> &b, const Vec4<T> &s, const Vec4<T> &d, int koff, int K,
                                                   T &m, T &v) {
#pragma clang fp contract(off)
    m = (T)0;
    v = (T)0;
#pragma unroll
    for (int e = 0; e < PMF_VEC; ++e) {
        if (koff + e < K) {   // (a pad element holds 0 / 0)
            const T ex = (a.v[e] / b.v[e]) * (s.v[e] / d.v[e]);
            const T w = ((T)1 / a.v[e] + (T)1 / s.v[e]) + (T)1 / (a.v[e] * s.v[e]);
            m += ex;
            v += (ex * ex) * w;
        }
    }
}

// PLUGIN and NEGBIN of one pair from its rating and the (mean, variance) the call returns, all in double; `rest` is
// -mu - lgamma(x + 1), what BOUND adds to x lse.  A function of its own, not inlined: its seven logarithms' coefficients
// (64-bit constants sit in scalar register pairs on this target) then live for the length of one call instead of across
// the kernel's pair loop, where the scalar registers are taken by the call's twelve base pointers.
struct GammaPredDensities {
    double plugin, negbin, rest;
};
__device__ __noinline__ GammaPredDensities gamma_pred_densities(double x, double mu, double vv) {
    double plugin, negbin;
    const double lf = gamma_log_factorial(x);
    const double lmu = log(mu);
    const bool floored = mu < PMF_RATE_FLOOR;
    plugin = floored ? x * -23.025850929940457 - PMF_RATE_FLOOR - lf : x * lmu - mu - lf;   // (log 1e-10)
    const double xlm = x == 0.0 ? 0.0 : x * lmu;   // 0 log 0 = 0: a count of 0 has density exp(-mu)
    // the rate moment-matched to Gamma(r, r / mu): the count is negative binomial; the unclamped Poisson term where the
    // variance is 0 or r leaves double's range
    const double rr = mu * mu / vv;
    negbin = xlm - mu - lf;
    if (vv != 0.0 && isfinite(rr)) negbin = xlm - lf - (rr + x) * gamma_log1p(mu / rr) + gamma_negbin_excess(x, rr);
    return {plugin, negbin, -mu - lf};
}

// sum_k exp(e_k - mx) of a lane's four elements and the logarithm of the group's sum: inline in fp32, calls in fp64 (for
// the reason above: exp and log in double bring some forty scalar registers of coefficients)
__device__ __forceinline__ float gamma_pred_exp_sum(float e0, float e1, float e2, float e3, float mx) {
    float z = exp(e0 - mx);   // (a pad is -inf: exp gives 0)
    z += exp(e1 - mx);
    z += exp(e2 - mx);
    z += exp(e3 - mx);
    return z;
}
__device__ __noinline__ double gamma_pred_exp_sum(double e0, double e1, double e2, double e3, double mx) {
    double z = exp(e0 - mx);
    z += exp(e1 - mx);
    z += exp(e2 - mx);
    z += exp(e3 - mx);
    return z;
}
__device__ __forceinline__ float gamma_pred_log(float z) { return log(z); }
__device__ __noinline__ double gamma_pred_log(double z) { return log(z); }

template <typename T, int LPR, bool BOUND>
__global__ __launch_bounds__(256) void gamma_pred_kernel(GammaPredParams<T> p) {
    constexpr int G = 256 / LPR;
    constexpr int UN = sizeof(T) == 4 ? 4 : 2;   // pairs whose gathers are in flight (LPR >= 4)
    __shared__ double s_part[G][PMF_GAMMA_PRED_TOTALS];
    const int c = threadIdx.x % LPR;
    const int g = threadIdx.x / LPR;
    const int koff = c * PMF_VEC;
    const int kpad = p.kpad;
    const bool active = koff < kpad;
    const T ninf = (T)(-INFINITY);
    const int64_t batches = (p.n + LPR - 1) / LPR;
    const int64_t stride = (int64_t)gridDim.x * G;
    // all groups of a wavefront iterate the same number of times (DPP inside)
    const int64_t rounds = (batches + stride - 1) / stride;
    int64_t batch = (int64_t)blockIdx.x * G + g;
    double sum_v = 0.0, sum_plugin = 0.0, sum_bound = 0.0, sum_negbin = 0.0;
    for (int64_t r = 0; r < rounds; ++r, batch += stride) {
        if (batch < batches) {
            const int64_t base = batch * LPR;
            const int cnt = (int)min((int64_t)LPR, p.n - base);
            int my_u = 0, my_i = 0;   // (lanes past the batch hold id 0: a valid row, loaded and not used)
            if (c < cnt) {
                my_u = p.u[base + c];
                my_i = p.i[base + c];
            }
            T my_m = (T)0, my_v = (T)0, my_lse = (T)0;
            for (int tt = 0; tt < cnt; tt += UN) {
                int64_t au[UN], ai[UN];
                Vec4<T> a[UN], b[UN], s[UN], d[UN], lu[UN], li[UN];
#pragma unroll
                for (int q = 0; q < UN; ++q) {
                    au[q] = (int64_t)__shfl(my_u, tt + q, LPR) * kpad + koff;
                    ai[q] = (int64_t)__shfl(my_i, tt + q, LPR) * kpad + koff;
                }
#pragma unroll
                for (int q = 0; q < UN; ++q) {
                    a[q] = b[q] = s[q] = d[q] = zero4<T>();
                    if (active) {
                        a[q] = load4(p.shape_u + au[q]);
                        b[q] = load4(p.rate_u + au[q]);
                        s[q] = load4(p.shape_i + ai[q]);
                        d[q] = load4(p.rate_i + ai[q]);
                    }
                    if constexpr (BOUND) {
                        // (-inf in every element: what a lane past kpad contributes; a pad of the tables is -inf too)
                        lu[q].v[0] = lu[q].v[1] = lu[q].v[2] = lu[q].v[3] = ninf;
                        li[q] = lu[q];
                        if (active) {
                            lu[q] = load4(p.table_u + 2 * au[q] - koff);   // row * 2 kpad + koff
                            li[q] = load4(p.table_i + 2 * ai[q] - koff);
                        }
                    }
                }
#pragma unroll
                for (int q = 0; q < UN; ++q) {
                    if (tt + q < cnt) {
                        T m, v, lse = (T)0;
                        gamma_pred_moments<T>(a[q], b[q], s[q], d[q], koff, active ? p.K : 0, m, v);
                        m = group_sum<LPR>(m);
                        v = group_sum<LPR>(v);
                        if constexpr (BOUND) {
                            T e[PMF_VEC];
#pragma unroll
                            for (int k = 0; k < PMF_VEC; ++k) e[k] = lu[q].v[k] + li[q].v[k];
                            const T mx = group_max<LPR>(vmax(vmax(e[0], e[1]), vmax(e[2], e[3])));
                            const T z = group_sum<LPR>(gamma_pred_exp_sum(e[0], e[1], e[2], e[3], mx));   // >= 1: the largest element adds exp(0)
                            lse = mx + gamma_pred_log(z);
                        }
                        if (c == tt + q) {
                            my_m = m;
                            my_v = v;
                            my_lse = lse;
                        }
                    }
                }
            }
            if (c < cnt) {   // this lane's pair of the batch
                const int64_t idx = base + c;
                const double mu = (double)my_m, vv = (double)my_v;
                if (p.mean) p.mean[idx] = mu;
                if (p.var) p.var[idx] = vv;
                sum_v += vv;
                if (p.x) {
                    const double x = p.x[idx];
                    const GammaPredDensities t = gamma_pred_densities(x, mu, vv);
                    const double plugin = t.plugin, negbin = t.negbin;
                    double bound = __builtin_nan("");
                    if constexpr (BOUND) {
                        bound = x * (double)my_lse + t.rest;
                        sum_bound += bound;
                    }
                    sum_plugin += plugin;
                    sum_negbin += negbin;
                    if (p.logp) {
                        double *o = p.logp + idx * PMF_GAMMA_PRED_KINDS;
                        o[PMF_GAMMA_PRED_PLUGIN] = plugin;
                        o[PMF_GAMMA_PRED_BOUND] = bound;
                        o[PMF_GAMMA_PRED_NEGBIN] = negbin;
                    }
                }
            }
        }
    }
    // (every lane of the block arrives: the rounds are the same for all)
    sum_v = group_sum<LPR>(sum_v);
    sum_plugin = group_sum<LPR>(sum_plugin);
    sum_bound = group_sum<LPR>(sum_bound);
    sum_negbin = group_sum<LPR>(sum_negbin);
    if (c == 0) {
        s_part[g][0] = sum_v;
        s_part[g][1 + PMF_GAMMA_PRED_PLUGIN] = sum_plugin;
        s_part[g][1 + PMF_GAMMA_PRED_BOUND] = sum_bound;
        s_part[g][1 + PMF_GAMMA_PRED_NEGBIN] = sum_negbin;
    }
    __syncthreads();
    if (threadIdx.x < PMF_GAMMA_PRED_TOTALS) {
        double s = 0.0;
        for (int k = 0; k < G; ++k) s += s_part[k][threadIdx.x];
        p.block_out[(int64_t)blockIdx.x * PMF_GAMMA_PRED_TOTALS + threadIdx.x] = s;
    }
}

static const int64_t kGammaPredPairs = 1 << 20;   // pairs per staging round (PMF_GAMMA_PRED_PAIRS=n overrides it): 56 MB of scratch
static const int kGammaPredMaxGrid = 1024;

// Pairs in staging rounds: ids (and ratings) up, one launch, the per-pair outputs and the block partial sums down; the
// totals are the partial sums in block order, round after round.  The scratch layout does not depend on what was
// asked for, so a call never grows what an earlier call of the same n left.
template <typename T>
static int run_gamma_predictive(pmf_ctx *ctx, int64_t n, const int32_t *u, const int32_t *i, const double *x, bool bound,
                                double *out_mean, double *out_var, double *out_logp, double *totals) {
    const int kpad = ctx->kpad;
    const int64_t step = ctx->gamma_pred_pairs > 0 ? ctx->gamma_pred_pairs : kGammaPredPairs;
    const int64_t m = std::min(n, step);
    const size_t n_part = (size_t)kGammaPredMaxGrid * PMF_GAMMA_PRED_TOTALS;
    PmfLayout lay;
    const auto part_at = lay.add<double>(n_part), x_at = lay.add<double>((size_t)m), mean_at = lay.add<double>((size_t)m);
    const auto var_at = lay.add<double>((size_t)m), logp_at = lay.add<double>((size_t)m * PMF_GAMMA_PRED_KINDS);
    const auto u_at = lay.add<int32_t>((size_t)m), i_at = lay.add<int32_t>((size_t)m);
    int rc;
    if ((rc = pmf_ensure_scratch(ctx, lay.bytes()))) return rc;
    if ((rc = pmf_ensure_pinned(ctx, n_part * sizeof(double)))) return rc;
    void *base = ctx->d_scratch.as();
    double *d_part = part_at.at(base), *d_x = x_at.at(base), *d_mean = mean_at.at(base), *d_var = var_at.at(base);
    double *d_logp = logp_at.at(base);
    int32_t *d_u = u_at.at(base), *d_i = i_at.at(base);
    if (bound && (rc = gamma_exact_build_tables<T>(ctx))) return rc;

    GammaPredParams<T> p;
    p.u = d_u;
    p.i = d_i;
    p.shape_u = ctx->arr[PMF_SIDE_USER][PMF_ARR_SHAPE].as<const T>();
    p.rate_u = ctx->arr[PMF_SIDE_USER][PMF_ARR_RATE].as<const T>();
    p.shape_i = ctx->arr[PMF_SIDE_ITEM][PMF_ARR_SHAPE].as<const T>();
    p.rate_i = ctx->arr[PMF_SIDE_ITEM][PMF_ARR_RATE].as<const T>();
    p.table_u = bound ? gamma_exact_table<T>(ctx, PMF_SIDE_USER) : nullptr;
    p.table_i = bound ? gamma_exact_table<T>(ctx, PMF_SIDE_ITEM) : nullptr;
    p.x = x ? d_x : nullptr;
    p.mean = out_mean ? d_mean : nullptr;
    p.var = out_var ? d_var : nullptr;
    p.logp = out_logp ? d_logp : nullptr;
    p.block_out = d_part;
    p.K = ctx->K;
    p.kpad = kpad;
    double sum[PMF_GAMMA_PRED_TOTALS] = {};
    for (int64_t at = 0; at < n; at += step) {
        const int64_t cnt = std::min(step, n - at);
        PMF_HIP_CHECK(hipMemcpyAsync(d_u, u + at, (size_t)cnt * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        PMF_HIP_CHECK(hipMemcpyAsync(d_i, i + at, (size_t)cnt * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        if (x) PMF_HIP_CHECK(hipMemcpyAsync(d_x, x + at, (size_t)cnt * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        p.n = cnt;
        int grid = 0;
        {
            PmfProfScope prof(ctx, x ? PMF_KERNEL_EVAL : PMF_KERNEL_PREDICT);
            pmf_with_pow2<4>(pmf_lanes_per_row(kpad), [&](auto L) {
                grid = (int)std::min<int64_t>((cnt + 255) / 256, kGammaPredMaxGrid);   // a block's 256 / L groups take L pairs each
                if (bound)
                    hipLaunchKernelGGL((gamma_pred_kernel<T, L, true>), dim3(grid), dim3(256), 0, ctx->stream, p);
                else
                    hipLaunchKernelGGL((gamma_pred_kernel<T, L, false>), dim3(grid), dim3(256), 0, ctx->stream, p);
            });
        }
        PMF_HIP_CHECK(hipGetLastError());
        if (out_mean) PMF_HIP_CHECK(hipMemcpyAsync(out_mean + at, d_mean, (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (out_var) PMF_HIP_CHECK(hipMemcpyAsync(out_var + at, d_var, (size_t)cnt * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        if (out_logp)
            PMF_HIP_CHECK(hipMemcpyAsync(out_logp + at * PMF_GAMMA_PRED_KINDS, d_logp, (size_t)cnt * PMF_GAMMA_PRED_KINDS * sizeof(double),
                                         hipMemcpyDeviceToHost, ctx->stream));
        PMF_HIP_CHECK(hipMemcpyAsync(ctx->h_pinned.as(), d_part, (size_t)grid * PMF_GAMMA_PRED_TOTALS * sizeof(double), hipMemcpyDeviceToHost,
                                     ctx->stream));
        PMF_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        const double *h = ctx->h_pinned.as<const double>();
        for (int b = 0; b < grid; ++b)
            for (int t = 0; t < PMF_GAMMA_PRED_TOTALS; ++t) sum[t] += h[(size_t)b * PMF_GAMMA_PRED_TOTALS + t];
    }
    if (totals) {
        const double nan = __builtin_nan("");
        totals[0] = sum[0];
        totals[1 + PMF_GAMMA_PRED_PLUGIN] = x ? sum[1 + PMF_GAMMA_PRED_PLUGIN] : nan;
        totals[1 + PMF_GAMMA_PRED_BOUND] = x && bound ? sum[1 + PMF_GAMMA_PRED_BOUND] : nan;
        totals[1 + PMF_GAMMA_PRED_NEGBIN] = x ? sum[1 + PMF_GAMMA_PRED_NEGBIN] : nan;
    }
    return PMF_OK;
}

extern "C" int pmf_gamma_predictive(pmf_ctx *ctx, int64_t n, const int32_t *user_ids, const int32_t *item_ids, const double *ratings,
                                    int with_bound, double *out_mean, double *out_var, double *out_logp, double *totals) {
    PMF_REQUIRE(ctx != nullptr, PMF_EINVAL, "pmf_gamma_predictive: null context");
    PMF_REQUIRE(n >= 0, PMF_EINVAL, "pmf_gamma_predictive: negative n");
    if (n == 0) return PMF_OK;
    PMF_REQUIRE(user_ids != nullptr, PMF_EINVAL, "pmf_gamma_predictive: null user_ids");
    PMF_REQUIRE(item_ids != nullptr, PMF_EINVAL, "pmf_gamma_predictive: null item_ids");
    PMF_REQUIRE(out_mean || out_var || out_logp || totals, PMF_EINVAL, "pmf_gamma_predictive: no output (out_mean, out_var, out_logp and totals are all null)");
    PMF_REQUIRE(ratings || !out_logp, PMF_EINVAL, "pmf_gamma_predictive: out_logp without ratings");
    int rc;
    if ((rc = require_gamma_q(ctx, {PMF_SIDE_USER, PMF_SIDE_ITEM}, "pmf_gamma_predictive"))) return rc;
    for (int64_t k = 0; k < n; ++k) {
        PMF_REQUIRE(user_ids[k] >= 0 && user_ids[k] < ctx->rows[PMF_SIDE_USER], PMF_ERANGE,
                    "pmf_gamma_predictive: user id %d at position %lld outside [0, %lld)", user_ids[k], (long long)k,
                    (long long)ctx->rows[PMF_SIDE_USER]);
        PMF_REQUIRE(item_ids[k] >= 0 && item_ids[k] < ctx->rows[PMF_SIDE_ITEM], PMF_ERANGE,
                    "pmf_gamma_predictive: item id %d at position %lld outside [0, %lld)", item_ids[k], (long long)k,
                    (long long)ctx->rows[PMF_SIDE_ITEM]);
    }
    PMF_HIP_CHECK(hipSetDevice(ctx->device));
    return pmf_with_dtype(ctx, [&](auto t) {
        // (without ratings there is no BOUND to form: no table is built)
        return run_gamma_predictive<decltype(t)>(ctx, n, user_ids, item_ids, ratings, with_bound != 0 && ratings, out_mean, out_var, out_logp,
                                                 totals);
    });
}

// Profiling aid (no reference counterpart): average device time of `repeats` launches of the
// gather-only twin of the Poisson/HPF half-sweep of `side` -- the ceiling the cache hierarchy sets
// for this context's gather pattern (bench.py reports the sweep kernel against it).
extern "C" int pmf_prof_gather_ceiling(pmf_ctx *ctx, int side, int repeats, double *ms_per_launch) {
    PMF_SIDE_ENTRY("pmf_prof_gather_ceiling");
    PMF_REQUIRE(ms_per_launch != nullptr && repeats >= 1, PMF_EINVAL, "pmf_prof_gather_ceiling: bad arguments");
    hipEvent_t a = nullptr, b = nullptr;
    PMF_HIP_CHECK(hipEventCreate(&a));
    hipError_t e = hipEventCreate(&b);
    if (e != hipSuccess) {
        (void)hipEventDestroy(a);
        pmf_set_error("hipEventCreate failed: %s", hipGetErrorString(e));
        return PMF_EHIP;
    }
    int rc = PMF_OK;
    for (int k = 0; k <= repeats && !rc; ++k) {   // launch 0 warms the caches and is not timed
        if (k == 1) (void)hipEventRecord(a, ctx->stream);
        rc = pmf_with_dtype(ctx, [&](auto t) { return run_gather_probe<decltype(t)>(ctx, side); });
    }
    float ms = 0.f;
    if (!rc) {
        e = hipEventRecord(b, ctx->stream);
        if (e == hipSuccess) e = hipEventSynchronize(b);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, a, b);
        if (e != hipSuccess) {
            pmf_set_error("pmf_prof_gather_ceiling: %s", hipGetErrorString(e));
            rc = PMF_EHIP;
        }
    }
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    *ms_per_launch = (double)ms / repeats;
    return rc;
}
