// Gaussian MF half-sweep kernels (rows a8, a9 of SURVEY.md section 8).
//
// A factor half-sweep is two phases:
//   accumulate : per row r, S = sum_j (COV_other[o_j] + m_j m_j^T) (packed lower
//                triangle) and w = sum_j m_j * resid_j.  Pure streaming: every
//                rating gathers one packed covariance row (K(K+1)/2 values) and
//                one mean row.  One wavefront per task (run of <= PMF_GAUSS_CHUNK
//                ratings of one row), sums in registers, written once.  The
//                sums go IN PLACE into COV_side[r] / FACTOR_side[r] (nobody
//                gathers this side during its own sweep), so no row-sized
//                scratch is needed at 1M+ rows.
//   solve      : per non-empty row, COV[r] = inv(I/eta2 + S/sigma2) and
//                FACTOR[r] = COV[r] w / sigma2, one wavefront per row with the
//                whole K x K matrix in registers (lane = column).
// K = 64 / fp32 (the benchmark configuration) has a dedicated accumulate kernel
// that forms sum_j m_j m_j^T on the matrix cores (v_mfma_f32_32x32x2_f32: exact
// fp32 FMA chains) while the VALU only adds the gathered covariance rows.
#include <stdlib.h>

#include <algorithm>
#include <new>
#include <type_traits>
#include <vector>

#include "pmf_device.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

template <typename T>
struct GaussParams {
    const PmfTask *tasks;
    int64_t n_tasks;
    const PmfSplitRow *split;
    const int32_t *other;
    const T *val;
    const T *factor_other;
    const T *cov_other;
    const T *bias_self;   // null when the model has no biases
    const T *bias_other;
    T *partial;           // [n_slots][cov_stride + kpad]
    // destination of a complete row's raw sums
    T *dst_s;
    int64_t dst_s_stride;
    T *dst_w;
    int64_t dst_w_stride;
    int K, kpad, kp, cov_stride;
    // [nnz] per rating of `other`: 1 if that row of the opposite side is hot (PMF_GAUSS_HOT_MB), null = all hot.
    // Read by the fp32 K <= 64 accumulate only: cold rows are gathered with non-temporal loads.
    const uint8_t *hot = nullptr;
    // Mean sums for the bias sweep, H_r = sum_j m_j over the ratings of row r (fused fp32 K <= 64 factor sweep only;
    // all null everywhere else): a whole-row task stores m_r . H_r, with m_r the mean it has just solved, to mdot[r];
    // a split task stores its part of H to partial_h[slot], the combine sums the parts in slot order into
    // hsplit[position in `split`], and the split rows' solve forms the dot.
    T *mdot = nullptr;        // [rows]
    T *partial_h = nullptr;   // [n_slots][kpad]
    T *hsplit = nullptr;      // [n_split][kpad]
};

// What the host code carries, and the argument of the weighted instantiations (WT) of the accumulate kernels: wgt[j] =
// the confidence weight c_j of rating j ([nnz], beside val; null: no weights).  S takes c_j - zero_w, w takes c_j;
// zero_w = the zero weight w0 under PMF_ZEROS_OBSERVED (the blend then adds w0 G), else 0.  The unweighted
// instantiations keep GaussParams as their argument, so their code does not depend on this struct.
template <typename T>
struct GaussParamsW : GaussParams<T> {
    const T *wgt = nullptr;
    T zero_w = (T)0;
    const GaussParams<T> &plain() const { return *this; }
};
template <typename T, bool WT>
using GaussArgs = std::conditional_t<WT, GaussParamsW<T>, GaussParams<T>>;

__device__ __forceinline__ void wave_lds_fence() {
    // LDS operations of one wavefront execute in order; this only stops the
    // compiler from moving LDS accesses across the point.
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int rfl(int x) { return __builtin_amdgcn_readfirstlane(x); }

__device__ __forceinline__ PmfTask load_task_uniform(const PmfTask *tasks, int64_t id) {
    PmfTask t = tasks[id];
    PmfTask r;
    r.row = rfl(t.row);
    r.len = rfl(t.len);
    r.slot = rfl(t.slot);
    r.pad = 0;
    unsigned lo = (unsigned)rfl((int)(t.start & 0xFFFFFFFFll)), hi = (unsigned)rfl((int)(t.start >> 32));
    r.start = (int64_t)(((unsigned long long)hi << 32) | lo);
    return r;
}

// packed index p -> (row, col) of the lower triangle
__device__ __forceinline__ void tri_rc(int p, int &r, int &c) {
    r = (int)((sqrtf(8.0f * (float)p + 1.0f) - 1.0f) * 0.5f);
    while ((r + 1) * (r + 2) / 2 <= p) ++r;
    while (r * (r + 1) / 2 > p) --r;
    c = p - r * (r + 1) / 2;
}

// ---------------------------------------------------------------------------
// accumulate, generic (any K <= 256, fp32 / fp64): VALU outer products
// ---------------------------------------------------------------------------
// One wavefront per task.  The packed range is covered in passes of 64 x CH
// 4-element chunks (lane owns chunks q = lane + 64 s of the pass); per pass the
// task's ratings are streamed two at a time: their mean rows are staged in LDS
// (the outer product needs m[r] m[c] for every packed entry), their covariance
// chunks are loaded as 16/32-byte accesses (2 x CH in flight per lane) and
// acc += V + m[r] m[c].  The (r, c) of a lane's entries are pass constants.
template <typename T, int KR>
__device__ __forceinline__ T solve_from_image(const T *img, T wj, int K, int kpad, T inv_sigma2, T inv_eta2,
                                              T *vout, T *mout, int lane);

// KS > 0 (K <= 64): a task that is a whole row keeps its sums in an LDS image and is solved on the spot by the
// same wavefront (the KS-row register sweep), as in the MFMA kernels -- this is how fp64 contexts (parity mode)
// stop paying a separate solve launch.
template <typename T, int KS = 0, bool WT = false>
__global__ __launch_bounds__(256) void gauss_accum_generic_kernel(GaussArgs<T, WT> p, T inv_sigma2 = (T)0, T inv_eta2 = (T)0,
                                                                  T *cov_self = nullptr, T *factor_self = nullptr) {
    constexpr int CH = sizeof(T) == 8 ? 5 : 4;  // chunks per lane per pass -> 64 * CH * 4 packed entries per pass (fp64, K = 64: 2 passes instead of 3)
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t task_id = (int64_t)blockIdx.x * 4 + wave;
    if (task_id >= p.n_tasks) return;
    const PmfTask t = load_task_uniform(p.tasks, task_id);
    const int lds_per_wave = 2 * p.kpad + (KS > 0 ? p.cov_stride : 0);
    T *m0 = reinterpret_cast<T *>(smem_raw) + (int64_t)wave * lds_per_wave;
    T *m1 = m0 + p.kpad;
    T *img = m1 + p.kpad;                       // [cov_stride], KS > 0 only
    const bool solve_here = KS > 0 && t.slot < 0;
    const int32_t *col = p.other + t.start;
    const T *val = p.val + t.start;
    const T *wgt = nullptr;
    if constexpr (WT) wgt = p.wgt + t.start;
    const T b_self = p.bias_self ? p.bias_self[t.row] : (T)0;
    const int chunks = p.cov_stride / PMF_VEC;
    T *out_s, *out_w;
    if (t.slot >= 0) {
        out_s = p.partial + (int64_t)t.slot * (p.cov_stride + p.kpad);
        out_w = out_s + p.cov_stride;
    } else {
        out_s = p.dst_s + (int64_t)t.row * p.dst_s_stride;
        out_w = p.dst_w + (int64_t)t.row * p.dst_w_stride;
    }
    T wacc[4] = {(T)0, (T)0, (T)0, (T)0};  // K <= 256: k = lane + 64 e
    for (int q0 = 0; q0 < chunks; q0 += 64 * CH) {
        Vec4<T> acc[CH];
        int rc[CH][PMF_VEC];  // r | c << 8 of every entry this lane owns in this pass
#pragma unroll
        for (int s = 0; s < CH; ++s) {
            acc[s] = zero4<T>();
            const int q = q0 + lane + 64 * s;
#pragma unroll
            for (int e = 0; e < PMF_VEC; ++e) {
                int r = 0, c = 0;
                const int pi = q * PMF_VEC + e;
                if (q < chunks && pi < p.kp) tri_rc(pi, r, c);
                rc[s][e] = r | (c << 8);
            }
        }
        for (int j = 0; j < t.len; j += 2) {
            const bool two = j + 1 < t.len;
            const int o0 = col[j], o1 = two ? col[j + 1] : o0;
            for (int k = lane; k < p.kpad; k += 64) {
                m0[k] = p.factor_other[(int64_t)o0 * p.kpad + k];
                m1[k] = two ? p.factor_other[(int64_t)o1 * p.kpad + k] : (T)0;
            }
            const T *v0 = p.cov_other + (int64_t)o0 * p.cov_stride;
            const T *v1 = p.cov_other + (int64_t)o1 * p.cov_stride;
            Vec4<T> a[CH], b[CH];
#pragma unroll
            for (int s = 0; s < CH; ++s) {
                const int q = min(q0 + lane + 64 * s, chunks - 1);  // clamped lanes are never stored
                a[s] = load4(v0 + (int64_t)q * PMF_VEC);
                b[s] = two ? load4(v1 + (int64_t)q * PMF_VEC) : zero4<T>();
            }
            T c0 = (T)1, c1 = (T)1;   // WT: the pair's weights (the absent second rating: 0, its addends are zeros)
            if constexpr (WT) {
                c0 = wgt[j];
                c1 = two ? wgt[j + 1] : (T)0;
            }
            wave_lds_fence();
            if (q0 == 0) {
                T r0 = val[j] - b_self - (p.bias_other ? p.bias_other[o0] : (T)0);
                T r1 = two ? val[j + 1] - b_self - (p.bias_other ? p.bias_other[o1] : (T)0) : (T)0;
                if constexpr (WT) {
                    r0 *= c0;
                    r1 *= c1;
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = lane + 64 * e;
                    if (k < p.K) wacc[e] += m0[k] * r0 + m1[k] * r1;
                }
            }
#pragma unroll
            for (int s = 0; s < CH; ++s)
#pragma unroll
                for (int e = 0; e < PMF_VEC; ++e) {
                    const int r = rc[s][e] & 255, c = rc[s][e] >> 8;
                    // reference order: (V_j + m_j m_j^T) added rating by rating
                    if constexpr (WT) {
                        acc[s].v[e] += (c0 - p.zero_w) * fma(m0[r], m0[c], a[s].v[e]);
                        if (two) acc[s].v[e] += (c1 - p.zero_w) * fma(m1[r], m1[c], b[s].v[e]);
                    } else {
                        acc[s].v[e] += fma(m0[r], m0[c], a[s].v[e]);
                        acc[s].v[e] += fma(m1[r], m1[c], b[s].v[e]);
                    }
                }
            wave_lds_fence();
        }
#pragma unroll
        for (int s = 0; s < CH; ++s) {
            const int q = q0 + lane + 64 * s;
            if (q < chunks) {
#pragma unroll
                for (int e = 0; e < PMF_VEC; ++e)
                    if (q * PMF_VEC + e >= p.kp) acc[s].v[e] = (T)0;
                store4((solve_here ? img : out_s) + (int64_t)q * PMF_VEC, acc[s]);
            }
        }
    }
    if constexpr (KS > 0) {
        if (solve_here) {
            wave_lds_fence();
            solve_from_image<T, KS>(img, wacc[0], p.K, p.kpad, inv_sigma2, inv_eta2,
                                    cov_self + (int64_t)t.row * p.cov_stride, factor_self + (int64_t)t.row * p.kpad, lane);
            return;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int k = lane + 64 * e;
        if (k < p.kpad) out_w[k] = k < p.K ? wacc[e] : (T)0;
    }
}

template <typename T>
struct SolveParams {
    const int32_t *rows;  // list of rows to solve, or null = rows row0 .. row0 + n (skip rows with S == 0)
    int64_t row0;
    int64_t n;
    const T *src_s;
    int64_t src_s_stride;
    const T *src_w;
    int64_t src_w_stride;
    T *cov;
    T *factor;
    T inv_sigma2, inv_eta2;
    int K, kpad, kp, cov_stride;
    // K <= 64, both or neither: hsum[k] = the mean sums of rows[k] ([n][kpad], GaussParams::hsplit), mdot[row] receives
    // the new mean's dot product with them
    const T *hsum = nullptr;
    T *mdot = nullptr;
};

__device__ __forceinline__ float readlane_dyn(float x, int lane) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), lane));
}
__device__ __forceinline__ double readlane_dyn(double x, int lane) {
    long long q = __builtin_bit_cast(long long, x);
    int lo = __builtin_amdgcn_readlane((int)(q & 0xFFFFFFFFll), lane);
    int hi = __builtin_amdgcn_readlane((int)(q >> 32), lane);
    q = ((long long)hi << 32) | (unsigned int)lo;
    return __builtin_bit_cast(double, q);
}

// A row's matrix in registers, one wavefront per row: B[i] = row i, lane j = column j.  The row solver, the ELBO row pass
// and the posterior draws all start from it Jacobi-scaled to a unit diagonal: g_j = 1 / sqrt(B_jj), B_ij *= g_i g_j.
// Returns lane j's g_j.
template <typename T, int KR>
__device__ __forceinline__ T reg_jacobi_scale(T *B, int j) {
    T diag = (T)1;
#pragma unroll
    for (int i = 0; i < KR; ++i) {
        const T dii = readlane_dyn(B[i], i);
        if (j == i) diag = dii;
    }
    const T g = (T)1 / sqrt(diag);
#pragma unroll
    for (int i = 0; i < KR; ++i) B[i] = B[i] * g * readlane_dyn(g, i);
    return g;
}

// B from the packed lower triangle `img` in LDS, rows and columns >= K the identity, then scaled; returns g_j
template <typename T, int KR>
__device__ __forceinline__ T reg_load_scaled(const T *img, int K, int lane, T *B) {
    const int j = lane, jc = j < K ? j : 0;
#pragma unroll
    for (int i = 0; i < KR; ++i) {
        const int ic = i < K ? i : 0;
        const int lo = ic < jc ? ic : jc, hi = ic < jc ? jc : ic;
        T s = img[hi * (hi + 1) / 2 + lo];
        if (!(i < K && j < K)) s = (i == j) ? (T)1 : (T)0;
        B[i] = s;
    }
    return reg_jacobi_scale<T, KR>(B, j);
}

// One wavefront per row, lane j = column j, B[i] = row (i + step) mod KR.
// Symmetric sweep on the Jacobi-scaled matrix (unit diagonal => pivots in
// (0, 1], which keeps the column update fma(-s, 1 - 1/d, s) = s/d free of
// cancellation).  The pivot row is always register 0 because every update
// writes row i into register i-1; after KR steps the rows are back in place
// and B = -inverse.  `img` is the packed lower triangle of S in LDS, `wj` lane
// j's right-hand side; writes the packed inverse and the mean, and returns lane j's element of the mean as stored.
template <typename T, int KR>
__device__ __forceinline__ T solve_from_image(const T *img, T wj, int K, int kpad, T inv_sigma2, T inv_eta2,
                                              T *vout, T *mout, int lane) {
    const int j = lane;
    T B[KR];
    const int jc = j < K ? j : 0;
#pragma unroll
    for (int i = 0; i < KR; ++i) {
        const int ic = i < K ? i : 0;
        const int lo = ic < jc ? ic : jc, hi = ic < jc ? jc : ic;
        T s = img[hi * (hi + 1) / 2 + lo] * inv_sigma2;
        if (!(i < K && j < K)) s = (T)0;
        if (i == j) s += (i < K) ? inv_eta2 : (T)1;
        B[i] = s;
    }
    const T g = reg_jacobi_scale<T, KR>(B, j);   // g_j = 1/sqrt(P_jj)

    for (int k = 0; k < KR; ++k) {
        const T v = B[0];
        const T pinv = (T)1 / readlane_dyn(v, k);
        const T u = v * pinv;
        const T uc = (j == k) ? ((T)1 - pinv) : u;
        // column k as scalars first (one batch of v_readlane into SGPRs), then the
        // rank-1 update: back-to-back readlane -> use pairs cost a wait state each
        constexpr int SB = sizeof(T) == 8 ? (KR < 16 ? KR : 16) : (KR < 32 ? KR : 32);   // fp64: 16 scalars = 32 SGPRs per batch (32 would spill)
#pragma unroll
        for (int i0 = 1; i0 < KR; i0 += SB) {
            T sc[SB];
#pragma unroll
            for (int q = 0; q < SB; ++q)
                if (i0 + q < KR) sc[q] = readlane_dyn(B[i0 + q], k);
#pragma unroll
            for (int q = 0; q < SB; ++q)
                if (i0 + q < KR) B[i0 + q - 1] = fma(-sc[q], uc, B[i0 + q]);
        }
        B[KR - 1] = (j == k) ? -pinv : u;
    }
    // V = -(g_i g_j) B ;  m_j = inv_sigma2 * sum_i V[i][j] w_i
    // (g2: an opaque copy, so the 64 per-row scale scalars are re-read here instead of
    //  being kept alive in SGPRs across the whole sweep loop and spilled)
    T g2 = g;
    asm volatile("" : "+v"(g2));
    T mj = (T)0;
#pragma unroll
    for (int i = 0; i < KR; ++i) {
        const T vij = -B[i] * g2 * readlane_dyn(g2, i);
        mj = fma(vij, readlane_dyn(wj, i), mj);
        if (i < K && j <= i) vout[i * (i + 1) / 2 + j] = vij;
    }
    const T mean = (j < K) ? mj * inv_sigma2 : (T)0;
    if (j < kpad) mout[j] = mean;
    return mean;
}

template <typename T, int KR>
__global__ __launch_bounds__(256) void gauss_solve_reg_kernel(SolveParams<T> p) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t idx = (int64_t)blockIdx.x * 4 + wave;
    if (idx >= p.n) return;
    const int row = p.rows ? rfl(p.rows[idx]) : (int)(p.row0 + idx);
    const T *S = p.src_s + (int64_t)row * p.src_s_stride;
    if (!p.rows && S[0] == (T)0) return;  // no rating anywhere for this row
    T *img = reinterpret_cast<T *>(smem_raw) + (int64_t)wave * p.cov_stride;
    for (int q = lane * PMF_VEC; q < p.cov_stride; q += 64 * PMF_VEC) store4(img + q, load4(S + q));
    wave_lds_fence();
    const T wj = (lane < p.K) ? p.src_w[(int64_t)row * p.src_w_stride + lane] : (T)0;
    const T mean = solve_from_image<T, KR>(img, wj, p.K, p.kpad, p.inv_sigma2, p.inv_eta2,
                                           p.cov + (int64_t)row * p.cov_stride, p.factor + (int64_t)row * p.kpad, lane);
    if (p.hsum) {   // (uniform; lanes >= K hold a zero mean.  The position is formed again, as a scalar: nothing of it stays live across the sweep)
        const int64_t k = (int64_t)blockIdx.x * 4 + rfl(threadIdx.x >> 6);
        const T dot = group_sum<64>(mean * p.hsum[k * p.kpad + min((int)(threadIdx.x & 63), p.kpad - 1)]);
        if ((threadIdx.x & 63) == 0) p.mdot[rfl(p.rows[k])] = dot;   // (hsum comes with a row list)
    }
}

// 64 < K <= 128, fp32: a row is handled by the TWO wavefronts of a 128-thread block.
// LDS layout shared by the accumulate kernel and the solve:
//   img [8256]  full 128-row packed lower triangle: S for rows < K; for the padding rows
//               >= K zeros with a diagonal chosen so that P_ii = S_ii/sigma2 + 1/eta2 = 1,
//               which removes every K-dependent mask from the register build
//   xbuf [1024] the MFMA sweep's two 128 x 4 pivot panels (double-buffered by step)
//   gbuf [128] (Jacobi scales), wbuf [128] (right-hand side)
// (Rounds 1-2 swept the matrix on the VALU, split between the two waves by rows (K <= 96) or by columns, one scalar
//  pivot at a time with the pivot row broadcast through LDS -- 85 VALU instructions and a 128-scalar LDS round trip per
//  pivot; the block sweep below replaced them in round 3: profiles/r03_solve_mfma_vs_valu.jsonl.)
#define PAIR_IMG 8256
#define PAIR_XBUF 1024   // two 128 x 4 pivot panels
#define PAIR_LDS_FLOATS (PAIR_IMG + PAIR_XBUF + 128 + 128)

__device__ __forceinline__ float pair_pad_diag(float inv_sigma2, float inv_eta2) { return (1.f - inv_eta2) / inv_sigma2; }

// the entries at or past kp (the padding rows) of chunk q .. q + 3 of the image: pad_diag on the diagonal, zero off it
__device__ __forceinline__ void pair_pad_chunk(Vec4<float> &v, int q, int kp, float pad_diag) {
    if (q + PMF_VEC > kp) {
#pragma unroll
        for (int e = 0; e < PMF_VEC; ++e)
            if (q + e >= kp) {
                int r, c;
                tri_rc(q + e, r, c);
                if (r == c) v.v[e] = pad_diag;
                else v.v[e] = 0.f;
            }
    }
}

// ---- 64 < K <= 128 on the matrix cores: block sweep, four pivots per step ------------------------------------------
// The symmetric sweep of the K x K matrix as RANK-4 updates on v_mfma_f32_16x16x4_f32 (exact fp32 FMA chains).  The
// Jacobi-scaled matrix B (padded to 16 TT rows with the identity) lives in the accumulator tiles of the block's two
// wavefronts: wave 0 owns tile rows [0, TH), wave 1 the rest, every tile column; lane l of a tile holds column l & 15 of
// rows 4 (l >> 4) + 0..3.  One step sweeps the pivot set Kb = {p .. p + 3}: with R = B[Kb, :] (4 x n, the pivot rows),
// D = B[Kb, Kb] and U = R^T D^-1 (n x 4),
//     B[i][j] -= U[i,:] R[:,j]  (i, j not in Kb),   B[i, Kb] = U[i,:],   B[Kb, j] = U[j,:]^T,   B[Kb, Kb] = -D^-1
// -- four scalar sweeps in one.  D^-1 is never formed: with D = L diag(d) L^T (L unit lower triangular), W = L^-1 and
// Y = W R (4 x n), U = Y^T diag(1/d) W and U R = Y^T diag(1/d) Y -- the four rank-1 updates of the scalar sweep, every
// term as well scaled as there.  (Multiplying R by an explicit D^-1 loses cond(D) digits more than the scalar sweep: a
// nearly singular pivot block whose rows couple to a row outside it -- three of four equicorrelated rows in one block,
// the fourth in the next -- then misses the error bound of DESIGN.md section 4.3 by a factor of 25 .. 100.)  All four
// cases come out of ONE MFMA per tile when
//   * the accumulator entries in the pivot rows and pivot columns are zeroed first,
//   * the B operand (lane: pivot index c, column j) is Y[c][j], with -e_(j - p) in the place of R[:, j] for the pivot
//     columns themselves, i.e. -W[c][j - p],
//   * the A operand (lane: row i, pivot index c) is -(1 / d[c]) times the B operand of column i:
// a pivot row k' then receives  sum_c (W[c][k'] / d[c]) Y[c][j] = U[j][k'],  a pivot column c'  sum_c (-Y[c][i] / d[c])
// (-W[c][c']) = U[i][c'],
// and the pivot block  sum_c (W[c][k'] / d[c]) (-W[c][c']) = -D^-1.  The only data exchanged per step is the pivot panel R
// (128 x 4 floats, double-buffered in LDS): its owner -- the 16 lanes that hold those four rows in their four
// accumulator registers -- writes it as one float4 per column as soon as that tile row has been updated (the tile row
// of the NEXT pivots is updated first), so the panel's write -> barrier -> read trip runs under the remaining MFMAs.
// Every wave factors the 4 x 4 pivot block itself (in registers, identical on all lanes).  Per step a
// wave issues TH x TT MFMAs (32 at K = 128: 1024 matrix-pipe cycles) and about 150 VALU instructions, against the
// 128 LDS-broadcast-bound scalar pivots x 85 VALU instructions of the VALU splits it replaced.
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float rcp_nr(float x) {
    float r = __builtin_amdgcn_rcpf(x);
    return fmaf(fmaf(-x, r, 1.f), r, r);   // one Newton step: within an ulp of 1 / x
}

// Precondition: img / wbuf are complete and the block has synchronised.  rt = PAIR_XBUF floats.
// W = the wavefront (0 / 1) as a compile-time constant: its tile rows are then known statically, the image build and the
// packed write-back know for every tile whether it lies below, on or above the diagonal (no per-element compare; the
// tiles above the diagonal are not written at all), and the two waves run their own copy of the code with the same
// sequence of barriers.
template <int TT, int W>
__device__ __forceinline__ void pair_solve_mfma_wave(float *img, float *rt, float *gbuf, const float *wbuf, int K, int kpad,
                                                     int cov_stride, float inv_sigma2, float inv_eta2, float *vout, float *mout,
                                                     int lane) {
    constexpr int TH = (TT + 1) / 2;
    constexpr int wave = W;
    const int tid = 64 * wave + lane;
    gbuf[tid] = 1.f / sqrtf(img[tid * (tid + 3) / 2] * inv_sigma2 + inv_eta2);   // (rows >= K: the padding diagonal gives 1)
    __syncthreads();
    const int lc = lane & 15, lg = lane >> 4;
    constexpr int base = W ? TH : 0, nrows = W ? TT - TH : TH;
    f32x4 D[TH][TT];
    float gj[TT];
    int tj[TT];                               // packed offset of this lane's column j as a ROW
#pragma unroll
    for (int J = 0; J < TT; ++J) {
        gj[J] = gbuf[16 * J + lc];
        tj[J] = (16 * J + lc) * (16 * J + lc + 1) / 2;
    }
#pragma unroll
    for (int ii = 0; ii < TH; ++ii) {
        if (ii < nrows) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 16 * (base + ii) + 4 * lg + r;
                const float gi = gbuf[i] * inv_sigma2;
                const int ti = i * (i + 1) / 2;
#pragma unroll
                for (int J = 0; J < TT; ++J) {
                    const int j = 16 * J + lc;
                    float v;
                    if (base + ii > J) v = img[ti + j];                                  // a tile below the diagonal
                    else if (base + ii < J) v = img[tj[J] + i];                          // above: the transposed entry
                    else v = img[i >= j ? ti + j : tj[J] + i];
                    v *= gi;
                    if (base + ii == J && i == j) v = fmaf(inv_eta2, gbuf[i], v);
                    D[ii][J][r] = v * gj[J];
                }
            }
        } else {
#pragma unroll
            for (int J = 0; J < TT; ++J) D[ii][J] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    // the 16 lanes holding pivot rows 4 qg .. 4 qg + 3 of local tile row `ii` write them as the panel of a step
    auto publish = [&](float *dst, int ii_local, int qg) {
#pragma unroll
        for (int ii = 0; ii < TH; ++ii)
            if (ii == ii_local && lg == qg) {
#pragma unroll
                for (int J = 0; J < TT; ++J)
                    *reinterpret_cast<float4 *>(dst + (16 * J + lc) * 4) = make_float4(D[ii][J][0], D[ii][J][1], D[ii][J][2], D[ii][J][3]);
            }
    };
    const int steps = (K + 3) >> 2;
    if (wave == 0) publish(rt, 0, 0);
#pragma unroll 1
    for (int s = 0; s < steps; ++s) {
        const int p = 4 * s, Ip = p >> 4, q = p & 15, qg = q >> 2;
        const float *rb = rt + (s & 1) * 512;
        __syncthreads();   // the panel of step s is visible; everybody has finished reading the other buffer
        // D = B[Kb, Kb] (4 x 4, symmetric) = L diag(d) L^T, identical on every lane; W = L^-1 (unit lower triangular)
        float m[4][4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float4 col = *reinterpret_cast<const float4 *>(rb + (p + c) * 4);
            m[0][c] = col.x; m[1][c] = col.y; m[2][c] = col.z; m[3][c] = col.w;
        }
        float dinv[4], l[4][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            dinv[k] = rcp_nr(m[k][k]);
#pragma unroll
            for (int i = k + 1; i < 4; ++i) l[i][k] = m[i][k] * dinv[k];
#pragma unroll
            for (int i = k + 1; i < 4; ++i)
#pragma unroll
                for (int j = k + 1; j <= i; ++j) m[i][j] = fmaf(-l[i][k], m[j][k], m[i][j]);   // (the lower triangle)
        }
        const float w10 = -l[1][0];
        const float w21 = -l[2][1], w20 = fmaf(-l[2][1], w10, -l[2][0]);
        const float w32 = -l[3][2], w31 = fmaf(-l[3][2], w21, -l[3][1]);
        const float w30 = fmaf(-l[3][2], w20, fmaf(-l[3][1], w10, -l[3][0]));
        // this lane's pivot index is lg: row lg of W, and -1 / d[lg]
        const float wr0 = lg == 0 ? 1.f : lg == 1 ? w10 : lg == 2 ? w20 : w30;
        const float wr1 = lg == 0 ? 0.f : lg == 1 ? 1.f : lg == 2 ? w21 : w31;
        const float wr2 = lg <= 1 ? 0.f : lg == 2 ? 1.f : w32;
        const float wr3 = lg == 3 ? 1.f : 0.f;
        const float ndinv = -(lg == 0 ? dinv[0] : lg == 1 ? dinv[1] : lg == 2 ? dinv[2] : dinv[3]);
        const int cq = lc - q;                      // 0..3 when this lane's row / column index is a pivot
        const bool piv = cq >= 0 && cq < 4;
        // y[c][j] = (W R)[c][j] for this lane's column j and c = lg, with -e_(j - p) in the place of R[:, j] for the pivot
        // columns themselves: the B operand.  The A operand of row i is -y[c][i] / d[c] (update_row).
        float bop[TT];
#pragma unroll
        for (int J = 0; J < TT; ++J) {
            float4 x = *reinterpret_cast<const float4 *>(rb + (16 * J + lc) * 4);
            if (J == Ip && piv) x = make_float4(cq == 0 ? -1.f : 0.f, cq == 1 ? -1.f : 0.f, cq == 2 ? -1.f : 0.f, cq == 3 ? -1.f : 0.f);
            bop[J] = fmaf(wr3, x.w, fmaf(wr2, x.z, fmaf(wr1, x.y, wr0 * x.x)));
        }
        auto update_row = [&](auto ii_tag) {
            constexpr int ii = decltype(ii_tag)::value;
            constexpr int I = base + ii;
            const float a = ndinv * bop[I < TT ? I : 0];   // (I >= TT: a tile row this wave does not have, never run)
            const bool prow = I == Ip;              // wave-uniform
            // the accumulator entries of the pivot rows (tile row Ip) and pivot columns (tile column Ip) start from zero.
            // Wave-uniform BRANCHES around the selects (the empty asm keeps the compiler from turning them back into
            // selects on every tile): vector instructions take their issue cycles from the fp32 matrix pipe
            if (prow) {
                asm volatile("" ::: "memory");
#pragma unroll
                for (int J = 0; J < TT; ++J)
                    if (lg == qg) D[ii][J] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int J = 0; J < TT; ++J) {
                if (J == Ip) {
                    asm volatile("" ::: "memory");
                    if (piv) D[ii][J] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
                D[ii][J] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bop[J], D[ii][J], 0, 0, 0);
            }
        };
        // the tile row that holds the next pivots first, then its panel, then the rest
        const int pn = p + 4, inext = (s + 1 < steps) ? (pn >> 4) - base : -1;
        auto for_rows = [&](auto &&body) {
            if constexpr (TH > 0) body(std::integral_constant<int, 0>{});
            if constexpr (TH > 1) body(std::integral_constant<int, 1>{});
            if constexpr (TH > 2) body(std::integral_constant<int, 2>{});
            if constexpr (TH > 3) body(std::integral_constant<int, 3>{});
        };
        for_rows([&](auto tag) {
            if (decltype(tag)::value == inext) update_row(tag);
        });
        if (inext >= 0 && inext < nrows) publish(rt + ((s + 1) & 1) * 512, inext, (pn & 15) >> 2);
        for_rows([&](auto tag) {
            if (decltype(tag)::value != inext && decltype(tag)::value < nrows) update_row(tag);
        });
    }
    // V = -(g_i g_j) B (packed lower triangle, staged in the LDS image and written out coalesced);
    // m_i = inv_sigma2 * sum_j V[i][j] w_j: each wave has its rows complete
    __syncthreads();   // (the image is free since the build; the last panel reads are done)
    float xj[TT];
#pragma unroll
    for (int J = 0; J < TT; ++J) xj[J] = gj[J] * wbuf[16 * J + lc];
#pragma unroll
    for (int ii = 0; ii < TH; ++ii) {
        if (ii < nrows) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 16 * (base + ii) + 4 * lg + r;
                const float gi = -gbuf[i];
                float acc = 0.f;
#pragma unroll
                for (int J = 0; J < TT; ++J) {
                    const int j = 16 * J + lc;
                    const float b = D[ii][J][r] * gi;
                    acc = fmaf(b, xj[J], acc);
                    if (base + ii > J) {                       // below the diagonal: every entry is stored
                        if (i < K) img[i * (i + 1) / 2 + j] = b * gj[J];
                    } else if (base + ii == J) {
                        if (j <= i && i < K) img[i * (i + 1) / 2 + j] = b * gj[J];
                    }
                }
                acc = group_sum<16>(acc);
                if (lc == 0 && i < kpad) mout[i] = i < K ? acc * inv_sigma2 : 0.f;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
    for (int qv = threadIdx.x * PMF_VEC; qv < cov_stride; qv += 128 * PMF_VEC) store4(vout + qv, load4(img + qv));
}

template <int TT>
__device__ __forceinline__ void pair_solve_mfma(float *img, float *rt, float *gbuf, const float *wbuf, int K, int kpad,
                                                int cov_stride, float inv_sigma2, float inv_eta2, float *vout, float *mout,
                                                int wave, int lane) {
    if (wave == 0) pair_solve_mfma_wave<TT, 0>(img, rt, gbuf, wbuf, K, kpad, cov_stride, inv_sigma2, inv_eta2, vout, mout, lane);
    else pair_solve_mfma_wave<TT, 1>(img, rt, gbuf, wbuf, K, kpad, cov_stride, inv_sigma2, inv_eta2, vout, mout, lane);
}

template <int MT>
__global__ __launch_bounds__(128, 2) void gauss_solve_pair_kernel(SolveParams<float> p) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    float *img = reinterpret_cast<float *>(smem_raw);
    float *xbuf = img + PAIR_IMG, *gbuf = xbuf + PAIR_XBUF, *wbuf = gbuf + 128;
    const int wave = rfl(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int64_t idx = blockIdx.x;
    const int row = p.rows ? p.rows[idx] : (int)(p.row0 + idx);
    const float *S = p.src_s + (int64_t)row * p.src_s_stride;
    if (!p.rows && S[0] == 0.f) return;  // uniform for the whole block
    const int K = p.K, j = 64 * wave + lane;
    const float pad_diag = pair_pad_diag(p.inv_sigma2, p.inv_eta2);
    for (int q = threadIdx.x * PMF_VEC; q < PAIR_IMG; q += 128 * PMF_VEC) {
        Vec4<float> v = q < p.cov_stride ? load4(S + q) : zero4<float>();
        pair_pad_chunk(v, q, p.kp, pad_diag);
        store4(img + q, v);
    }
    wbuf[j] = j < K ? p.src_w[(int64_t)row * p.src_w_stride + j] : 0.f;
    __syncthreads();
    pair_solve_mfma<MT>(img, xbuf, gbuf, wbuf, K, p.kpad, p.cov_stride, p.inv_sigma2, p.inv_eta2,
                        p.cov + (int64_t)row * p.cov_stride, p.factor + (int64_t)row * p.kpad, wave, lane);
}

// ---------------------------------------------------------------------------
// accumulate (+ fused solve), fp32, 64 < K <= 128: two wavefronts per task
// ---------------------------------------------------------------------------
// Wave w streams half of the packed covariance chunks ([w * H, (w+1) * H), up to 17
// 16-byte chunks per lane) and owns five of the ten lower 32x32 blocks of sum m m^T
// (wave 0: (0,0) (1,0) (1,1) (2,0) (2,1); wave 1: (2,2) (3,0) (3,1) (3,2) (3,3)).
// Both waves fold their blocks into the shared LDS image; a complete row is then
// solved in place by the same two waves (pair_solve_mfma).
// NT = chunk columns per wave (host picks the smallest that covers ceil(chunks / 2) / 64):
// 17 for K = 128 (1032 chunks per wave), 13 for K <= 114, 9 for K <= 95.
template <int NT, bool FUSE, int MT = 0, bool WT = false>
__global__ __launch_bounds__(128, 2) void gauss_accum_mfma128_kernel(GaussArgs<float, WT> p, float inv_sigma2, float inv_eta2,
                                                                     float *cov_self, float *factor_self) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    float *img = reinterpret_cast<float *>(smem_raw);
    float *xbuf = img + PAIR_IMG, *gbuf = xbuf + PAIR_XBUF, *wbuf = gbuf + 128;
    const int wave = rfl(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const PmfTask t = load_task_uniform(p.tasks, blockIdx.x);
    const int h = lane >> 5, c = lane & 31;
    const int K = p.K, kpad = p.kpad, stride = p.cov_stride, chunks = p.cov_stride / PMF_VEC;
    const int half = (chunks + 1) / 2;
    const int q_begin = wave ? half : 0, q_end = wave ? chunks : half;
    const int32_t *col = p.other + t.start;
    const float *val = p.val + t.start;
    const float b_self = p.bias_self ? p.bias_self[t.row] : 0.f;

    f32x16 d[5];
#pragma unroll
    for (int b = 0; b < 5; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) d[b][r] = 0.f;
    float4 acc[NT];
#pragma unroll
    for (int s = 0; s < NT; ++s) acc[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    float wA = 0.f, wB = 0.f;  // rhs segments 2*wave and 2*wave + 1

    // The task's row ids and ratings are fetched 64 at a time (one coalesced load each) and handed
    // out with v_readlane: the ids are SGPRs (scalar address arithmetic, SGPR-base loads) and no
    // trip waits for an index.  Every load of a trip is unconditional (clamped index, value
    // selected afterwards), so the m / rating / bias loads and the 17 covariance chunks leave
    // back to back and the trip pays ONE memory latency per rating.  (The first version loaded
    // the ids per trip and predicated the small loads with branches: index -> second index ->
    // m/rating/bias -> chunks of rating 0 -> chunks of rating 1 were five dependent latencies
    // per pair.)
    const bool has_bias = p.bias_other != nullptr;
    const float *bias_ptr = has_bias ? p.bias_other : p.factor_other;   // always readable
    const int bias_mul = has_bias ? 1 : 0;
    int idx_b = 0;
    float val_b = 0.f;
    float wgt_b = 1.f;   // WT: the batch's weights, handed out like val_b
    for (int j = 0; j < t.len; j += 2) {
        if ((j & 63) == 0) {
            const int jj = min(j + lane, t.len - 1);
            idx_b = col[jj];
            val_b = val[jj];
            if constexpr (WT) wgt_b = p.wgt[t.start + jj];
        }
        const bool two = j + 1 < t.len;
        const int l0 = j & 63;   // even: l0 + 1 is in the same batch
        const int o0 = __builtin_amdgcn_readlane(idx_b, l0);
        const int o1 = two ? __builtin_amdgcn_readlane(idx_b, l0 + 1) : o0;
        const float x0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, val_b), l0));
        const float x1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, val_b), two ? l0 + 1 : l0));
        const int oh = h ? o1 : o0;
        const bool live = (h == 0) || two;
        const float *mrow = p.factor_other + (int64_t)oh * kpad;
        float m[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) m[b] = mrow[min(32 * b + c, kpad - 1)];
        const float bo = bias_ptr[(int64_t)oh * bias_mul];
#pragma unroll
        for (int b = 0; b < 4; ++b) m[b] = (live && 32 * b + c < K) ? m[b] : 0.f;
        float res = live ? (h ? x1 : x0) - b_self - (has_bias ? bo : 0.f) : 0.f;
        // WT: c0 / c1 = the S-side weights of the pair (uniform), cm = this lane half's scale of the MFMA A operand
        float c0 = 1.f, c1 = 1.f, cm = 1.f;
        if constexpr (WT) {
            const float g0 = readlane_dyn(wgt_b, l0), g1 = readlane_dyn(wgt_b, two ? l0 + 1 : l0);
            res *= h ? g1 : g0;
            c0 = g0 - p.zero_w;
            c1 = g1 - p.zero_w;
            cm = h ? c1 : c0;
        }
        const float4 *v0 = reinterpret_cast<const float4 *>(p.cov_other + (int64_t)o0 * stride);
        // one rating's chunks in flight at a time (68 VGPRs): with the MFMA blocks the kernel then
        // fits 256 registers, i.e. two blocks' worth of waves per SIMD, so one block can solve
        // while the other streams
        // every column is loaded, clamped to the wave's last chunk: no uniform branches around the
        // loads, and the clamped lanes (same cache line again) are never stored.  The lane base is
        // made opaque each trip so that the 17 clamped offsets are recomputed (two VALU ops per
        // load) instead of being kept live -- and spilled -- across the loop
        int qb = q_begin + lane;
        asm volatile("" : "+v"(qb));
        // NT <= 9 (K <= 95) leaves registers for BOTH ratings of the pair in flight (2 x 36 load registers):
        // more bytes outstanding per streaming wave, which matters while the CU's other blocks are solving
        constexpr bool BOTH = NT <= 9;
        float4 a[NT], a2[BOTH ? NT : 1];
#pragma unroll
        for (int s = 0; s < NT; ++s)   // uniform base + 32-bit unsigned byte offset: the SGPR-base load form
            a[s] = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(v0) +
                                                     (unsigned)min(qb + 64 * s, q_end - 1) * 16u);
        if constexpr (BOTH) {
            // (o1 == o0 when the pair has one rating: the same lines again, never added)
            const float *v1 = p.cov_other + (int64_t)o1 * stride;
#pragma unroll
            for (int s = 0; s < NT; ++s)
                a2[s] = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(v1) +
                                                          (unsigned)min(qb + 64 * s, q_end - 1) * 16u);
        }
        wA = fmaf(wave ? m[2] : m[0], res, wA);
        wB = fmaf(wave ? m[3] : m[1], res, wB);
        // operand pairs of this wave's five blocks (wave is uniform: scalar selects)
        // (WT: the scaled mean c m is the A operand only, B stays m)
        const float A0 = (wave ? m[2] : m[0]) * cm, B0 = wave ? m[2] : m[0];
        const float A1 = (wave ? m[3] : m[1]) * cm, B1 = m[0];
        const float A2 = A1, B2 = m[1];
        const float A3 = (wave ? m[3] : m[2]) * cm, B3 = wave ? m[2] : m[0];
        const float A4 = A3, B4 = wave ? m[3] : m[1];
        d[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(A0, B0, d[0], 0, 0, 0);
        d[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(A1, B1, d[1], 0, 0, 0);
        d[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(A2, B2, d[2], 0, 0, 0);
        d[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(A3, B3, d[3], 0, 0, 0);
        d[4] = __builtin_amdgcn_mfma_f32_32x32x2f32(A4, B4, d[4], 0, 0, 0);
        // (WT: fmaf(1, a, acc) = acc + a, the unweighted bits when every weight is 1)
#pragma unroll
        for (int s = 0; s < NT; ++s) {
            if constexpr (WT) {
                acc[s].x = fmaf(c0, a[s].x, acc[s].x);
                acc[s].y = fmaf(c0, a[s].y, acc[s].y);
                acc[s].z = fmaf(c0, a[s].z, acc[s].z);
                acc[s].w = fmaf(c0, a[s].w, acc[s].w);
            } else {
                acc[s].x += a[s].x;
                acc[s].y += a[s].y;
                acc[s].z += a[s].z;
                acc[s].w += a[s].w;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (BOTH) {
            if (two) {
#pragma unroll
                for (int s = 0; s < NT; ++s) {
                    if constexpr (WT) {
                        acc[s].x = fmaf(c1, a2[s].x, acc[s].x);
                        acc[s].y = fmaf(c1, a2[s].y, acc[s].y);
                        acc[s].z = fmaf(c1, a2[s].z, acc[s].z);
                        acc[s].w = fmaf(c1, a2[s].w, acc[s].w);
                    } else {
                        acc[s].x += a2[s].x;
                        acc[s].y += a2[s].y;
                        acc[s].z += a2[s].z;
                        acc[s].w += a2[s].w;
                    }
                }
            }
        } else if (two) {
            // (the id is read again here so that the base stays a scalar inside this block)
            const float *v1 = p.cov_other + (int64_t)__builtin_amdgcn_readlane(idx_b, l0 + 1) * stride;
#pragma unroll
            for (int s = 0; s < NT; ++s)
                a[s] = *reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(v1) +
                                                         (unsigned)min(qb + 64 * s, q_end - 1) * 16u);
#pragma unroll
            for (int s = 0; s < NT; ++s) {
                if constexpr (WT) {
                    acc[s].x = fmaf(c1, a[s].x, acc[s].x);
                    acc[s].y = fmaf(c1, a[s].y, acc[s].y);
                    acc[s].z = fmaf(c1, a[s].z, acc[s].z);
                    acc[s].w = fmaf(c1, a[s].w, acc[s].w);
                } else {
                    acc[s].x += a[s].x;
                    acc[s].y += a[s].y;
                    acc[s].z += a[s].z;
                    acc[s].w += a[s].w;
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }

    // ---- fold: image = zeros (+ padding diagonal), then the ten MFMA blocks ----
    const float pad_diag = pair_pad_diag(inv_sigma2, inv_eta2);
    for (int q = threadIdx.x * PMF_VEC; q < PAIR_IMG; q += 128 * PMF_VEC) {
        Vec4<float> v = zero4<float>();
        if (FUSE) pair_pad_chunk(v, q, p.kp, pad_diag);
        store4(img + q, v);
    }
    __syncthreads();
    // block (bi, bj) of d[b]: wave 0: (0,0) (1,0) (1,1) (2,0) (2,1); wave 1: (2,2) (3,0) (3,1) (3,2) (3,3)
#pragma unroll
    for (int b = 0; b < 5; ++b) {
        const int bi = wave ? (b == 0 ? 2 : 3) : (b == 0 ? 0 : (b <= 2 ? 1 : 2));
        const int bj = wave ? (b == 0 ? 2 : b - 1) : (b == 0 ? 0 : (b == 2 ? 1 : (b == 4 ? 1 : 0)));
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int R = 32 * bi + (r & 3) + 8 * (r >> 2) + 4 * h;
            const int C = 32 * bj + c;
            if (R < K && C <= R) img[R * (R + 1) / 2 + C] = d[b][r];
        }
    }
    wA += __shfl_xor(wA, 32, 64);
    wB += __shfl_xor(wB, 32, 64);
    if (h == 0) {
        wbuf[64 * wave + c] = wA;
        wbuf[64 * wave + 32 + c] = wB;
    }
    __syncthreads();
    if constexpr (FUSE && MT > 0) if (t.slot < 0) {
#pragma unroll
        for (int s = 0; s < NT; ++s) {
            const int q = q_begin + lane + 64 * s;
            if (q < q_end) {
                float4 mm = reinterpret_cast<float4 *>(img)[q];
                mm.x += acc[s].x;
                mm.y += acc[s].y;
                mm.z += acc[s].z;
                mm.w += acc[s].w;
                reinterpret_cast<float4 *>(img)[q] = mm;
            }
        }
        __syncthreads();
        pair_solve_mfma<MT>(img, xbuf, gbuf, wbuf, K, kpad, stride, inv_sigma2, inv_eta2,
                            cov_self + (int64_t)t.row * stride, factor_self + (int64_t)t.row * kpad, wave, lane);
        return;
    }
    float *out_s, *out_w;
    if (t.slot >= 0) {
        out_s = p.partial + (int64_t)t.slot * (stride + kpad);
        out_w = out_s + stride;
    } else {
        out_s = p.dst_s + (int64_t)t.row * p.dst_s_stride;
        out_w = p.dst_w + (int64_t)t.row * p.dst_w_stride;
    }
#pragma unroll
    for (int s = 0; s < NT; ++s) {
        const int q = q_begin + lane + 64 * s;
        if (q < q_end) {
            const float4 mm = reinterpret_cast<const float4 *>(img)[q];
            float4 o = acc[s];
            o.x += mm.x;
            o.y += mm.y;
            o.z += mm.z;
            o.w += mm.w;
            reinterpret_cast<float4 *>(out_s)[q] = o;
        }
    }
    const int jj = threadIdx.x;
    if (jj < kpad) out_w[jj] = jj < K ? wbuf[jj] : 0.f;
}

// ---------------------------------------------------------------------------
// accumulate (+ fused solve), fp32, K <= 64: covariance rows on the VALU, m m^T on
// the MFMA pipe
// ---------------------------------------------------------------------------
// KB = 32 (K <= 32: one 32x32 block) or 64 (the three lower 32x32 blocks).  The
// packed row is cov_stride/4 16-byte chunks: chunk q = lane + 64 s, s < NT.  Two
// ratings feed one v_mfma_f32_32x32x2_f32 (k = 2): lanes 0-31 carry rating j,
// lanes 32-63 rating j+1 (operand lanes >= K hold zeros, so K need not be a
// multiple of 32; storage stays the exact K(K+1)/2 packing).  PU pairs are in
// flight per loop trip so that short rows (small K) still keep ~18 16-byte loads
// per lane outstanding.  The MFMA blocks are folded into the packed image through
// LDS once per task; a task that is a whole row is solved on the spot (FUSE).
// KS = register rows of the fused solve (8 / 16 for K <= 8 / 16: a quarter / half of the 32-row sweep).
//
// Cache policy of the gathers (p.hot): the most-rated rows of the gathered table, as many as fit the
// PMF_GAUSS_HOT_MB budget, are loaded with the default policy and all others non-temporally, so that
// once-touched cold rows do not evict the hot set from the Infinity Cache under its recency-based
// replacement.  The per-rating flags come 64 at a time with the ids and are ballot-ed into one
// uniform mask; each trip runs the variant of its pair's (hot, hot) case.  Only the load
// instructions differ: the sums and their order are those of the uniform default policy.

template <bool HOT>
__device__ __forceinline__ float4 gather_ld(const float4 *ptr) {
    if constexpr (HOT) {
        return *ptr;
    } else {
        const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(ptr));
        return make_float4(v.x, v.y, v.z, v.w);
    }
}

template <bool HOT>
__device__ __forceinline__ float gather_ld(const float *ptr) {
    if constexpr (HOT) return *ptr;
    else return __builtin_nontemporal_load(ptr);
}

// WT (weighted ratings, GaussParams::wgt): a third batch register carries the weights.  Per pair the two S-side weights
// c0 / c1 (c_j - zero_w) are uniform: the covariance adds become acc += fmaf(c0, a, c1 * b) (the pair sum first, then the
// accumulator, as in the unweighted form: the same bits when every weight is 1), the MFMA takes c_h m as its A operand
// only (B stays m), the residual is multiplied by the lane half's c_j, and the mean sums (mdot) become H_r = sum_j c_j m_j.
template <int KB, int NT, bool FUSE, int KS = KB, bool WT = false>
__global__ __launch_bounds__(256, KB == 64 ? 2 : 3) void gauss_accum_mfma_kernel(GaussArgs<float, WT> p, float inv_sigma2,
                                                                                float inv_eta2, float *cov_self,
                                                                                float *factor_self) {
    constexpr int NB = KB == 64 ? 3 : 1;
    // (the scheduler interleaves the trip's waits and adds with its loads -- about ten of the 18 are in
    //  flight at a time; forcing all 18 out before the first use: item sweep 68.4 -> 66.8 ms, user sweep
    //  56.6 -> 60.4 ms, worse overall -- and selecting that form for the item sweep only changed the
    //  epoch by less than the box-to-box noise (128.2 / 128.9 against 128.1 / 128.3 ms);
    //  issuing pair t+1 before consuming pair t needs 2 x 75 load registers and spills at NT >= 8)
    // (measured at K = 64 / NT = 9: two pairs in flight 1-2 % slower; one rating at a time at 3 waves
    //  per SIMD 2.5 % slower than one pair at 2 waves per SIMD.  Non-temporal loads of ALL the item
    //  side's covariance rows made no difference: they only traded the ~6 % of gathers that LRU kept
    //  in the Infinity Cache for none.  Non-temporal loads of the COLD rows only (p.hot) keep the
    //  most-rated rows resident instead: item side 67.7 -> 60.1 ms, user side 57.3 -> 56.0 ms at the
    //  224 MB default budget)
    constexpr int PU = NT >= 5 ? 1 : (NT >= 3 ? 2 : (NT == 2 ? 4 : 8));
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t task_id = (int64_t)blockIdx.x * 4 + wave;
    if (task_id >= p.n_tasks) return;
    const PmfTask t = load_task_uniform(p.tasks, task_id);
    const int h = lane >> 5, c = lane & 31;
    const int K = p.K, kpad = p.kpad, stride = p.cov_stride, chunks = p.cov_stride / PMF_VEC;
    const int32_t *col = p.other + t.start;
    const float *val = p.val + t.start;
    const float b_self = p.bias_self ? p.bias_self[t.row] : 0.f;
    const bool lo_ok = c < K, hi_ok = (KB == 64) && (32 + c < K);

    f32x16 d[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) d[b][r] = 0.f;
    float4 acc[NT];
#pragma unroll
    for (int s = 0; s < NT; ++s) acc[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    float wlo = 0.f, whi = 0.f;
    float hlo = 0.f, hhi = 0.f;   // FUSE: the sum of the gathered mean rows themselves (GaussParams::mdot), two adds per pair

    // one loop trip = PU pairs of ratings; FULL trips carry no validity tests
    // The task's row ids and ratings come 64 at a time (one coalesced load each per 64 ratings) and
    // are handed out with v_readlane: ids in SGPRs without a dependent scalar load per pair (the
    // PU = 8 trip of K <= 16 used to wait for eight of them in turn).
    int idx_b = 0;
    float val_b = 0.f;
    float wgt_b = 1.f;        // WT: the batch's weights
    uint64_t hot_b = ~0ull;   // bit l: rating l of the batch gathers a hot row
    const uint8_t *hot = p.hot ? p.hot + t.start : nullptr;
    auto fetch = [&](int j) {
        if ((j & 63) == 0) {   // a trip never straddles a batch: 2 PU divides 64
            const int jj = min(j + lane, t.len - 1);
            idx_b = col[jj];
            val_b = val[jj];
            if constexpr (WT) wgt_b = p.wgt[t.start + jj];
            if (hot) hot_b = __builtin_amdgcn_ballot_w64(__builtin_nontemporal_load(hot + jj) != 0);
        }
    };
    // POL: the (hot0, hot1) case of the trip's pair as bits 0 / 1 (PU = 1); -1 = per pair (PU > 1)
    auto trip = [&](int j, auto full_tag, auto pol_tag) {
        constexpr bool FULL = decltype(full_tag)::value;
        constexpr int POL = decltype(pol_tag)::value;
        float4 a[PU][NT], b[PU][NT];
        float mlo[PU], mhi[PU], res[PU];
        float cs0[PU], cs1[PU], ch[PU];   // WT: the pair's S-side weights (uniform) and the lane half's own c_j
#pragma unroll
        for (int u = 0; u < PU; ++u) {
            const int j0 = j + 2 * u, l0 = j0 & 63;
            const bool has0 = FULL || j0 < t.len, has1 = FULL || j0 + 1 < t.len;
            const int o0 = __builtin_amdgcn_readlane(idx_b, l0);                 // lanes past the task hold
            const int o1 = __builtin_amdgcn_readlane(idx_b, l0 + 1);             // its last (valid) id
            const float x0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, val_b), l0));
            const float x1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, val_b), l0 + 1));
            const int oh = h ? o1 : o0;
            const bool live = h ? has1 : has0;
            const float *mrow = p.factor_other + (int64_t)oh * kpad;
            const float xh = h ? x1 : x0;
            res[u] = live ? xh - b_self - (p.bias_other ? p.bias_other[oh] : 0.f) : 0.f;
            if constexpr (WT) {   // (a rating past the task: the weight of the task's last one, times zeros)
                const float g0 = readlane_dyn(wgt_b, l0), g1 = readlane_dyn(wgt_b, l0 + 1);
                ch[u] = h ? g1 : g0;
                res[u] *= ch[u];
                cs0[u] = g0 - p.zero_w;
                cs1[u] = g1 - p.zero_w;
            }
            const float4 *v0 = reinterpret_cast<const float4 *>(p.cov_other + (int64_t)o0 * stride);
            const float4 *v1 = reinterpret_cast<const float4 *>(p.cov_other + (int64_t)o1 * stride);
            auto loads = [&](auto h0_tag, auto h1_tag) {
                constexpr bool H0 = decltype(h0_tag)::value, H1 = decltype(h1_tag)::value;
                // one mean-row load serves both ratings: non-temporal only when both rows are cold
                mlo[u] = (live && lo_ok) ? gather_ld<H0 || H1>(mrow + c) : 0.f;
                mhi[u] = (live && hi_ok) ? gather_ld<H0 || H1>(mrow + 32 + c) : 0.f;
#pragma unroll
                for (int s = 0; s < NT; ++s) {
                    // only the last chunk column can run past the row: those lanes re-read the row's
                    // last chunk (same cache line, no extra traffic) and their sums are never stored,
                    // which keeps the whole trip free of divergent branches
                    const int q = (s + 1 < NT) ? lane + 64 * s : min(lane + 64 * s, chunks - 1);
                    a[u][s] = make_float4(0.f, 0.f, 0.f, 0.f);
                    b[u][s] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (has0) a[u][s] = gather_ld<H0>(v0 + q);
                    if (has1) b[u][s] = gather_ld<H1>(v1 + q);
                }
            };
            using T_ = std::true_type;
            using F_ = std::false_type;
            const int pol = POL >= 0 ? POL : (int)((hot_b >> l0) & 3);   // uniform
            if (pol == 3) loads(T_{}, T_{});
            else if (pol == 2) loads(F_{}, T_{});
            else if (pol == 1) loads(T_{}, F_{});
            else loads(F_{}, F_{});
        }
#pragma unroll
        for (int u = 0; u < PU; ++u) {
            wlo = fmaf(mlo[u], res[u], wlo);
            whi = fmaf(mhi[u], res[u], whi);
            if constexpr (FUSE && !WT) {
                hlo += mlo[u];
                if constexpr (KB == 64) hhi += mhi[u];
            }
            if constexpr (FUSE && WT) {   // H_r = sum_j c_j m_j
                hlo = fmaf(ch[u], mlo[u], hlo);
                if constexpr (KB == 64) hhi = fmaf(ch[u], mhi[u], hhi);
            }
            float alo = mlo[u], ahi = mhi[u];   // the A operands
            if constexpr (WT) {
                const float cm = h ? cs1[u] : cs0[u];
                alo *= cm;
                ahi *= cm;
            }
            d[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(alo, mlo[u], d[0], 0, 0, 0);
            if constexpr (KB == 64) {
                d[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(ahi, mlo[u], d[1], 0, 0, 0);
                d[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(ahi, mhi[u], d[2], 0, 0, 0);
            }
#pragma unroll
            for (int s = 0; s < NT; ++s) {
                if constexpr (WT) {
                    acc[s].x += fmaf(cs0[u], a[u][s].x, cs1[u] * b[u][s].x);
                    acc[s].y += fmaf(cs0[u], a[u][s].y, cs1[u] * b[u][s].y);
                    acc[s].z += fmaf(cs0[u], a[u][s].z, cs1[u] * b[u][s].z);
                    acc[s].w += fmaf(cs0[u], a[u][s].w, cs1[u] * b[u][s].w);
                } else {
                    acc[s].x += a[u][s].x + b[u][s].x;
                    acc[s].y += a[u][s].y + b[u][s].y;
                    acc[s].z += a[u][s].z + b[u][s].z;
                    acc[s].w += a[u][s].w + b[u][s].w;
                }
            }
        }
    };
    // PU = 1 (K > 48): the whole trip, adds included, is specialised on its pair's case, so that the
    // scheduler interleaves the 18 loads with the adds exactly as in the single-policy trip.  PU > 1
    // issues all of a trip's loads before its adds anyway: there each pair picks its loads' variant.
    auto run = [&](int j, auto full_tag) {
        fetch(j);
        if constexpr (PU > 1) {
            trip(j, full_tag, std::integral_constant<int, -1>{});
        } else {
            const int pol = (int)((hot_b >> (j & 63)) & 3);
            if (pol == 3) trip(j, full_tag, std::integral_constant<int, 3>{});
            else if (pol == 2) trip(j, full_tag, std::integral_constant<int, 2>{});
            else if (pol == 1) trip(j, full_tag, std::integral_constant<int, 1>{});
            else trip(j, full_tag, std::integral_constant<int, 0>{});
        }
    };
    int j = 0;
    for (; j + 2 * PU <= t.len; j += 2 * PU) run(j, std::true_type{});
    if (j < t.len) run(j, std::false_type{});

    // fold the outer-product blocks into the packed image via LDS
    float *img = reinterpret_cast<float *>(smem_raw) + (int64_t)wave * stride;
    // (the fold below writes every packed entry but not the row padding: clear first)
    for (int q = lane; q < chunks; q += 64) reinterpret_cast<float4 *>(img)[q] = make_float4(0.f, 0.f, 0.f, 0.f);
    wave_lds_fence();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;  // C/D layout of the 32x32 MFMA
        if (row < K && c <= row) img[row * (row + 1) / 2 + c] = d[0][r];
        if constexpr (KB == 64) {
            const int R1 = 32 + row;
            if (R1 < K) {
                if (c < K) img[R1 * (R1 + 1) / 2 + c] = d[1][r];
                if (c <= row) img[R1 * (R1 + 1) / 2 + 32 + c] = d[2][r];
            }
        }
    }
    wave_lds_fence();
    wlo += __shfl_xor(wlo, 32, 64);
    whi += __shfl_xor(whi, 32, 64);
    if constexpr (FUSE) {
        hlo += __shfl_xor(hlo, 32, 64);
        if constexpr (KB == 64) hhi += __shfl_xor(hhi, 32, 64);
    }
    if (FUSE && t.slot < 0) {
        // the row is complete: finish it here (S = image + covariance sums stays in
        // LDS) while the other wavefronts of the CU keep streaming
#pragma unroll
        for (int s = 0; s < NT; ++s) {
            const int q = lane + 64 * s;
            if (q < chunks) {
                float4 m = reinterpret_cast<float4 *>(img)[q];
                m.x += acc[s].x;
                m.y += acc[s].y;
                m.z += acc[s].z;
                m.w += acc[s].w;
                reinterpret_cast<float4 *>(img)[q] = m;
            }
        }
        wave_lds_fence();
        const float mean = solve_from_image<float, KS>(img, h ? whi : wlo, K, kpad, inv_sigma2, inv_eta2,
                                                       cov_self + (int64_t)t.row * stride, factor_self + (int64_t)t.row * kpad, lane);
        if (p.mdot) {   // (uniform; lanes >= K hold a zero mean)
            const float dot = group_sum<64>(mean * (h ? hhi : hlo));
            if (lane == 0) p.mdot[t.row] = dot;
        }
        return;
    }
    float *out_s, *out_w;
    if (t.slot >= 0) {
        out_s = p.partial + (int64_t)t.slot * (stride + kpad);
        out_w = out_s + stride;
        if constexpr (FUSE) {
            if (p.partial_h && h == 0) {   // (lanes >= K summed zeros: the row padding is written as such)
                float *out_h = p.partial_h + (int64_t)t.slot * kpad;
                if (c < kpad) out_h[c] = hlo;
                if (KB == 64 && 32 + c < kpad) out_h[32 + c] = hhi;
            }
        }
    } else {
        out_s = p.dst_s + (int64_t)t.row * p.dst_s_stride;
        out_w = p.dst_w + (int64_t)t.row * p.dst_w_stride;
    }
#pragma unroll
    for (int s = 0; s < NT; ++s) {
        const int q = lane + 64 * s;
        if (q < chunks) {
            const float4 m = reinterpret_cast<const float4 *>(img)[q];
            float4 o = acc[s];
            o.x += m.x;
            o.y += m.y;
            o.z += m.z;
            o.w += m.w;
            reinterpret_cast<float4 *>(out_s)[q] = o;
        }
    }
    if (h == 0) {
        if (c < kpad) out_w[c] = wlo;
        if (KB == 64 && 32 + c < kpad) out_w[32 + c] = whi;
    }
}

// ---------------------------------------------------------------------------
// combine the partial slots of split rows (slot order => deterministic)
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void gauss_combine_kernel(GaussParams<T> p) {
    constexpr int UN = 8;
    const PmfSplitRow sr = p.split[blockIdx.x];
    const int width = p.cov_stride + p.kpad;  // multiple of PMF_VEC
    T *out_s = p.dst_s + (int64_t)sr.row * p.dst_s_stride;
    T *out_w = p.dst_w + (int64_t)sr.row * p.dst_w_stride;
    // with p.partial_h the row's mean sums are kpad more elements behind the slot's width, in a slot array of their own
    const int total = width + (p.partial_h ? p.kpad : 0);
    for (int e = threadIdx.x * PMF_VEC; e < total; e += 256 * PMF_VEC) {
        const bool hpart = e >= width;
        const T *base = hpart ? p.partial_h + (int64_t)sr.first_slot * p.kpad + (e - width)
                              : p.partial + (int64_t)sr.first_slot * width + e;
        const int64_t step = hpart ? p.kpad : width;
        Vec4<T> acc = zero4<T>();
        int k = 0;
        for (; k + UN <= sr.n_slots; k += UN) {
            Vec4<T> v[UN];
#pragma unroll
            for (int q = 0; q < UN; ++q) v[q] = load4(base + (int64_t)(k + q) * step);
#pragma unroll
            for (int q = 0; q < UN; ++q)
#pragma unroll
                for (int c = 0; c < PMF_VEC; ++c) acc.v[c] += v[q].v[c];
        }
        for (; k < sr.n_slots; ++k) {
            Vec4<T> v = load4(base + (int64_t)k * step);
#pragma unroll
            for (int c = 0; c < PMF_VEC; ++c) acc.v[c] += v.v[c];
        }
        if (e < p.cov_stride) store4(out_s + e, acc);
        else if (!hpart) store4(out_w + (e - p.cov_stride), acc);
        else store4(p.hsplit + (int64_t)blockIdx.x * p.kpad + (e - width), acc);
    }
}

// ---------------------------------------------------------------------------
// solve: V = inv(I/eta2 + S/sigma2), m = V w / sigma2
// ---------------------------------------------------------------------------

// Generic solve for K > 64 (fp64) / K > 128: one block per row, Gauss-Jordan sweep on the full matrix.  The matrix
// lives in LDS while K (K + 1) + 3 K elements fit the CU's 160 KB (fp32: K <= 200, fp64: K <= 141); beyond that
// (`scratch` != null) every block keeps it in its own slice of a global scratch buffer -- L2-resident, slow, and
// only there so that the Gaussian model has no K limit below the context's 256 (the reference has none at all).
template <typename T>
__global__ __launch_bounds__(256) void gauss_solve_lds_kernel(SolveParams<T> p, T *scratch) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int K = p.K, ld = K + 1;
    T *lds = reinterpret_cast<T *>(smem_raw);
    T *A = scratch ? scratch + (int64_t)blockIdx.x * K * ld : lds;   // [K][ld]
    T *g = scratch ? lds : lds + K * ld;                             // [K] scaling
    T *prow = g + K;                                                 // [K] scaled pivot row
    T *pcol = prow + K;                                              // [K] pivot column
    const int tid = threadIdx.x;
    for (int64_t idx = blockIdx.x; idx < p.n; idx += gridDim.x) {
    const int row = p.rows ? p.rows[idx] : (int)(p.row0 + idx);
    const T *S = p.src_s + (int64_t)row * p.src_s_stride;
    if (!p.rows && S[0] == (T)0) continue;   // uniform for the block
    __syncthreads();
    for (int e = tid; e < K * K; e += 256) {
        const int i = e / K, j = e % K;
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        T s = S[hi * (hi + 1) / 2 + lo] * p.inv_sigma2;
        if (i == j) s += p.inv_eta2;
        A[i * ld + j] = s;
    }
    __syncthreads();
    for (int i = tid; i < K; i += 256) g[i] = (T)1 / sqrt(A[i * ld + i]);
    __syncthreads();
    for (int e = tid; e < K * K; e += 256) {
        const int i = e / K, j = e % K;
        A[i * ld + j] *= g[i] * g[j];
    }
    __syncthreads();
    for (int k = 0; k < K; ++k) {
        const T pinv = (T)1 / A[k * ld + k];
        __syncthreads();
        for (int i = tid; i < K; i += 256) {
            prow[i] = A[k * ld + i] * pinv;
            pcol[i] = A[i * ld + k];
        }
        __syncthreads();
        for (int e = tid; e < K * K; e += 256) {
            const int i = e / K, j = e % K;
            T x;
            if (i == k) x = (j == k) ? -pinv : prow[j];
            else if (j == k) x = pcol[i] * pinv;
            else x = fma(-pcol[i], prow[j], A[i * ld + j]);
            A[i * ld + j] = x;
        }
        __syncthreads();
    }
    // V = -g g A ; m = inv_sigma2 V w
    T *vout = p.cov + (int64_t)row * p.cov_stride;
    for (int e = tid; e < K * K; e += 256) {
        const int i = e / K, j = e % K;
        const T v = -A[i * ld + j] * g[i] * g[j];
        A[i * ld + j] = v;
        if (j <= i) vout[i * (i + 1) / 2 + j] = v;
    }
    for (int i = tid; i < K; i += 256) prow[i] = p.src_w[(int64_t)row * p.src_w_stride + i];
    __syncthreads();
    for (int i = tid; i < p.kpad; i += 256) {
        T m = (T)0;
        if (i < K)
            for (int jj = 0; jj < K; ++jj) m = fma(A[i * ld + jj], prow[jj], m);
        p.factor[(int64_t)row * p.kpad + i] = m * p.inv_sigma2;
    }
    }
}

// ---------------------------------------------------------------------------
// bias half-sweep (lane group per task, same decomposition as the gamma sweep)
// ---------------------------------------------------------------------------
template <typename T>
struct BiasParams {
    const PmfTask *tasks;
    int64_t n_tasks;
    const PmfSplitRow *split;
    const int32_t *other;
    const T *val;
    const T *factor_self;
    const T *factor_other;
    T *bias_self;
    const T *bias_other;
    T *partial;  // [n_slots]
    T *stats;    // [rows][2] (residual sum, count), STATS mode
    T inv_sigma2, inv_eta_bias2;
    int kpad;
    int64_t row0, rows;  // finalize-from-stats covers rows [row0, rows)
    // weighted ratings (both or neither): wgt[j] = c_j beside val, wsum[r] = C_r = the sum of row r's weights, which takes
    // the place of the row's rating count
    const T *wgt = nullptr;
    const T *wsum = nullptr;
};

template <typename T>
__device__ __forceinline__ T bias_from_sum(const BiasParams<T> &p, T sum, T count) {
    // gaussian_mf_cavi_bias.py:222-230: var = 1/(1/eta_b2 + n/sigma2); b = var/sigma2 * sum
    const T var = (T)1 / (p.inv_eta_bias2 + count * p.inv_sigma2);
    return (var * p.inv_sigma2) * sum;
}

template <typename T, int LPR, bool STATS, bool WT = false>
__global__ __launch_bounds__(256) void gauss_bias_kernel(BiasParams<T> p) {
    constexpr int G = 256 / LPR;
    constexpr int UN = LPR < 4 ? LPR : 4;
    const int c = threadIdx.x % LPR;
    const int64_t task_id = (int64_t)blockIdx.x * G + threadIdx.x / LPR;
    if (task_id >= p.n_tasks) return;
    const PmfTask t = p.tasks[task_id];
    const int koff = c * PMF_VEC;
    const bool active = koff < p.kpad;
    const Vec4<T> self = active ? load4(p.factor_self + (int64_t)t.row * p.kpad + koff) : zero4<T>();
    const int32_t *col = p.other + t.start;
    const T *val = p.val + t.start;
    T sum = (T)0;
    for (int base = 0; base < t.len; base += LPR) {
        const int n = min(LPR, t.len - base);
        int my_o = 0;
        T my_r = (T)0, my_w = (T)1;
        if (c < n) {
            my_o = col[base + c];
            my_r = val[base + c] - p.bias_other[my_o];
            if constexpr (WT) my_w = p.wgt[t.start + base + c];
        }
        for (int tt = 0; tt < n; tt += UN) {
            int o[UN];
            T rv[UN], cw[UN];
            Vec4<T> b[UN];
#pragma unroll
            for (int q = 0; q < UN; ++q) {
                o[q] = __shfl(my_o, tt + q, LPR);
                rv[q] = __shfl(my_r, tt + q, LPR);
                if constexpr (WT) cw[q] = __shfl(my_w, tt + q, LPR);
            }
#pragma unroll
            for (int q = 0; q < UN; ++q)
                b[q] = active ? load4(p.factor_other + (int64_t)o[q] * p.kpad + koff) : zero4<T>();
#pragma unroll
            for (int q = 0; q < UN; ++q) {
                if (tt + q < n) {
                    T d = b[q].v[0] * self.v[0];
                    d = fma(b[q].v[1], self.v[1], d);
                    d = fma(b[q].v[2], self.v[2], d);
                    d = fma(b[q].v[3], self.v[3], d);
                    d = group_sum<LPR>(d);
                    if constexpr (WT) sum += cw[q] * (rv[q] - d);
                    else sum += rv[q] - d;
                }
            }
        }
    }
    if (c != 0) return;
    if (t.slot >= 0) {
        p.partial[t.slot] = sum;
        return;
    }
    T cnt = (T)t.len;
    if constexpr (WT) cnt = p.wsum[t.row];
    if (STATS) {
        p.stats[(int64_t)t.row * 2] = sum;
        p.stats[(int64_t)t.row * 2 + 1] = cnt;
    } else {
        p.bias_self[t.row] = bias_from_sum(p, sum, cnt);
    }
}

// The same sums without the gather, for a side whose fused factor sweep has left mdot[r] = m_r . H_r, H_r = the sum
// of the mean rows of r's ratings (GaussParams::mdot; valid while neither side's means nor the ratings have changed):
//     sum_j (x_j - b_o(j) - m_r . m_o(j)) = sum_j (x_j - b_o(j)) - m_r . H_r
// What is left is a stream of 8 bytes per rating (id and rating, coalesced over the LPR lanes of the task's group)
// and one 4-byte gather from the other side's bias table; LPR follows the task length, not K.  A split task leaves
// its part of the first sum in its slot and gauss_bias_split_kernel subtracts the dot product once per row.
template <typename T, int LPR, bool WT = false>
__global__ __launch_bounds__(256) void gauss_bias_sums_kernel(BiasParams<T> p, const T *mdot) {
    constexpr int G = 256 / LPR;
    constexpr int UN = 4;
    const int c = threadIdx.x % LPR;
    const int64_t task_id = (int64_t)blockIdx.x * G + threadIdx.x / LPR;
    if (task_id >= p.n_tasks) return;
    const PmfTask t = p.tasks[task_id];
    const int32_t *col = p.other + t.start;
    const T *val = p.val + t.start;
    T sum = (T)0;
    for (int base = c; base < t.len; base += UN * LPR) {
        int o[UN];
        T x[UN], b[UN], cw[UN];
#pragma unroll
        for (int q = 0; q < UN; ++q) {   // (past the task: its last rating again, not added)
            const int j = min(base + q * LPR, t.len - 1);
            o[q] = col[j];
            x[q] = val[j];
            if constexpr (WT) cw[q] = p.wgt[t.start + j];
        }
#pragma unroll
        for (int q = 0; q < UN; ++q) b[q] = p.bias_other[o[q]];
#pragma unroll
        for (int q = 0; q < UN; ++q)
            if (base + q * LPR < t.len) {
                if constexpr (WT) sum += cw[q] * (x[q] - b[q]);
                else sum += x[q] - b[q];
            }
    }
    sum = group_sum<LPR>(sum);
    if (c != 0) return;
    T cnt = (T)t.len;
    if constexpr (WT) cnt = p.wsum[t.row];
    if (t.slot >= 0) p.partial[t.slot] = sum;
    else p.bias_self[t.row] = bias_from_sum(p, sum - mdot[t.row], cnt);
}

// `mdot` (may be null): subtracted from a split row's sum, see gauss_bias_sums_kernel
template <typename T, bool STATS>
__global__ void gauss_bias_split_kernel(BiasParams<T> p, int64_t n_split, const int64_t *ptr, const T *mdot) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_split) return;
    const PmfSplitRow sr = p.split[s];
    T sum = (T)0;
    for (int k = 0; k < sr.n_slots; ++k) sum += p.partial[sr.first_slot + k];
    if (mdot) sum -= mdot[sr.row];
    const T cnt = p.wsum ? p.wsum[sr.row] : (T)(ptr[sr.row + 1] - ptr[sr.row]);
    if (STATS) {
        p.stats[(int64_t)sr.row * 2] = sum;
        p.stats[(int64_t)sr.row * 2 + 1] = cnt;
    } else {
        p.bias_self[sr.row] = bias_from_sum(p, sum, cnt);
    }
}

template <typename T>
__global__ void gauss_bias_finalize_all_kernel(BiasParams<T> p) {
    const int64_t r = p.row0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= p.rows) return;
    const T cnt = p.stats[r * 2 + 1];
    if (cnt > (T)0) p.bias_self[r] = bias_from_sum(p, p.stats[r * 2], cnt);
}

// ---------------------------------------------------------------------------
// fold-in (pmf_gauss_fold_in): the factor / bias alternation of NEW rows, bias model
// ---------------------------------------------------------------------------
// The accumulate and solve kernels above have left V and m0 = V w0 / sigma2, w0 = sum_j m_j (x_j - b_o), of every
// row of the block.  V does not depend on the row's bias b, and m is affine in it, so the alternation
// (gaussian_mf_cavi_bias.py:132-165 then :206-232, n_iter times from b = 0) is a scalar recursion:
//     g = sum_j m_j,  c0 = sum_j (x_j - b_o),  h = V g / sigma2,  alpha = g . m0,  beta = g . h
//     m^t = m0 - b^(t-1) h,   b^t = kappa (c0 - alpha + beta b^(t-1)),   kappa = 1 / (sigma2 (1/eta_bias2 + n/sigma2))
// One lane group per row, lane c owning elements 4c .. 4c+3 of the K-vectors as in gauss_bias_kernel.  The row's
// ratings are walked by that one group whatever their number: only the mean row (K values) and one bias are
// gathered per rating here, the covariance rows were gathered once by the accumulate.  h is a symmetric mat-vec
// over the packed lower triangle, four rows at a time: the lanes left of the diagonal block read their four columns
// of those rows; an entry V[i][j] adds V g_j to the row sum of i (reduced over the group, kept by the lane that owns
// i) and, for j < i, V g_i to the owner's own element j.
template <typename T>
struct FoldBiasParams {
    const int64_t *ptr;   // [n + 1] offsets of the block's rows into other / val
    int64_t n;
    const int32_t *other;
    const T *val;
    const T *factor_other;
    const T *bias_other;
    const T *cov;         // [n][cov_stride] packed V of the rows
    T *factor;            // [n][kpad] in: m0, out: m
    T *bias;              // [n] out
    T inv_sigma2, inv_eta_bias2;
    int n_iter, K, kpad, cov_stride;
    // weighted batch (both or neither): wgt[j] = c_j beside val, wsum[row] = C = the sum of the row's weights
    const T *wgt = nullptr;
    const T *wsum = nullptr;
};

template <typename T, int LPR>
__global__ __launch_bounds__(256) void gauss_fold_bias_kernel(FoldBiasParams<T> p) {
    constexpr int G = 256 / LPR;
    constexpr int UN = LPR < 4 ? LPR : 4;
    const int c = threadIdx.x % LPR;
    const int64_t row = (int64_t)blockIdx.x * G + threadIdx.x / LPR;
    if (row >= p.n) return;
    const int64_t start = p.ptr[row], n = p.ptr[row + 1] - start;
    if (n == 0) {   // (the host writes the prior)
        if (c == 0) p.bias[row] = (T)0;
        return;
    }
    const int koff = c * PMF_VEC;
    const bool active = koff < p.kpad;
    const int32_t *col = p.other + start;
    const T *val = p.val + start;
    Vec4<T> g = zero4<T>();
    T c0 = (T)0;
    for (int64_t base = 0; base < n; base += LPR) {
        const int cnt = (int)min((int64_t)LPR, n - base);
        int my_o = 0;
        T my_w = (T)1;
        if (c < cnt) {
            my_o = col[base + c];
            if (p.wgt) {
                my_w = p.wgt[start + base + c];
                c0 += my_w * (val[base + c] - p.bias_other[my_o]);
            } else {
                c0 += val[base + c] - p.bias_other[my_o];
            }
        }
        for (int tt = 0; tt < cnt; tt += UN) {
            Vec4<T> b[UN];
            T cw[UN];
#pragma unroll
            for (int q = 0; q < UN; ++q) {
                const int o = __shfl(my_o, tt + q, LPR);   // (lanes past the batch hold id 0: never loaded)
                cw[q] = __shfl(my_w, tt + q, LPR);
                b[q] = (active && tt + q < cnt) ? load4(p.factor_other + (int64_t)o * p.kpad + koff) : zero4<T>();
            }
            if (p.wgt) {   // (uniform)
#pragma unroll
                for (int q = 0; q < UN; ++q)
#pragma unroll
                    for (int e = 0; e < PMF_VEC; ++e) g.v[e] += cw[q] * b[q].v[e];
            } else {
#pragma unroll
                for (int q = 0; q < UN; ++q)
#pragma unroll
                    for (int e = 0; e < PMF_VEC; ++e) g.v[e] += b[q].v[e];
            }
        }
    }
    c0 = group_sum<LPR>(c0);
    const T *V = p.cov + row * p.cov_stride;
    Vec4<T> h = zero4<T>();
    for (int b = 0; b * PMF_VEC < p.K; ++b) {   // (b < LPR: the group has a lane for every four elements of a row)
        T gi[PMF_VEC], d[PMF_VEC];
#pragma unroll
        for (int r = 0; r < PMF_VEC; ++r) gi[r] = __shfl(g.v[r], b, LPR);
#pragma unroll
        for (int r = 0; r < PMF_VEC; ++r) {
            const int i = b * PMF_VEC + r;
            T dot = (T)0;
            if (i < p.K && c <= b) {
                const T *vr = V + i * (i + 1) / 2 + koff;
#pragma unroll
                for (int e = 0; e < PMF_VEC; ++e) {
                    if (koff + e <= i) {
                        const T v = vr[e];
                        dot = fma(v, g.v[e], dot);
                        if (koff + e < i) h.v[e] = fma(v, gi[r], h.v[e]);
                    }
                }
            }
            d[r] = dot;
        }
#pragma unroll
        for (int r = 0; r < PMF_VEC; ++r) d[r] = group_sum<LPR>(d[r]);
        if (c == b) {
#pragma unroll
            for (int r = 0; r < PMF_VEC; ++r) h.v[r] += d[r];
        }
    }
    T *mrow = p.factor + row * p.kpad + koff;
    const Vec4<T> m0 = active ? load4(mrow) : zero4<T>();
    T alpha = (T)0, beta = (T)0;
#pragma unroll
    for (int e = 0; e < PMF_VEC; ++e) {
        h.v[e] *= p.inv_sigma2;
        alpha = fma(g.v[e], m0.v[e], alpha);
        beta = fma(g.v[e], h.v[e], beta);
    }
    alpha = group_sum<LPR>(alpha);
    beta = group_sum<LPR>(beta);
    // gaussian_mf_cavi_bias.py:222-230: var = 1/(1/eta_b2 + n/sigma2); b = var/sigma2 * sum
    const T kappa = p.inv_sigma2 / (p.inv_eta_bias2 + (p.wsum ? p.wsum[row] : (T)n) * p.inv_sigma2);
    T b_prev = (T)0, b_cur = (T)0;
    for (int t = 0; t < p.n_iter; ++t) {
        b_prev = b_cur;
        b_cur = kappa * (c0 - alpha + beta * b_prev);
    }
    if (active) {
        Vec4<T> m;
#pragma unroll
        for (int e = 0; e < PMF_VEC; ++e) m.v[e] = fma(-b_prev, h.v[e], m0.v[e]);
        store4(mrow, m);
    }
    if (c == 0) p.bias[row] = b_cur;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// Where the statistics of the rows row0, row0 + 1, ... of a side live: S of row row0 + i at s + i * s_stride, its w at w + i *
// w_stride.  One constructor per layout in use; launch_accumulate alone calls set_dst and solve_params alone set_src.
template <typename T>
struct GaussStats {
    T *s, *w;
    int64_t s_stride, w_stride, row0;
    bool one_buffer;   // a row's w follows its S: the rows are one run of memory
    // in place: COV / FACTOR of `side` (the fused pass: nobody gathers a side during its own sweep)
    static GaussStats in_place(const pmf_ctx *ctx, int side) {
        return {ctx->arr[side][PMF_ARR_COV].as<T>(), ctx->arr[side][PMF_ARR_FACTOR].as<T>(), ctx->cov_stride, ctx->kpad, 0, false};
    }
    // interleaved: rows of [cov_stride + kpad] in `buf` from row `row0` on (accumulate / finalize and communicator: 0; a window)
    static GaussStats interleaved(const pmf_ctx *ctx, T *buf, int64_t row0) {
        return {buf, buf + ctx->cov_stride, ctx->cov_stride + ctx->kpad, ctx->cov_stride + ctx->kpad, row0, true};
    }
    // separate: an S buffer [rows][cov_stride] and a w buffer [rows][kpad] (a fold-in block, solved in place)
    static GaussStats separate(const pmf_ctx *ctx, T *s, T *w) { return {s, w, ctx->cov_stride, ctx->kpad, 0, false}; }
    // What a kernel gets for `at` = s or w.  Tasks and solves name a row by its id in the side, so the base is biased to
    // at - row0 * stride; only rows from row0 on are ever addressed.  In integers: it may lie outside the allocation.
    T *base(T *at, int64_t stride) const {
        return reinterpret_cast<T *>(reinterpret_cast<uintptr_t>(at) - (uintptr_t)row0 * stride * sizeof(T));
    }
    void set_dst(GaussParamsW<T> &p) const {
        p.dst_s = base(s, s_stride);
        p.dst_s_stride = s_stride;
        p.dst_w = base(w, w_stride);
        p.dst_w_stride = w_stride;
    }
    void set_src(SolveParams<T> &sp) const {
        sp.src_s = base(s, s_stride);
        sp.src_s_stride = s_stride;
        sp.src_w = base(w, w_stride);
        sp.src_w_stride = w_stride;
    }
};

// fuse: sums in place, then solve   !fuse: sums only (into the statistics or in place)
template <int KB, int NT, int KS = KB>
static void launch_accum_mfma_nt(pmf_ctx *ctx, const GaussParamsW<float> &p, dim3 grid, bool fuse, float is2, float ie2,
                                 float *cov, float *fac) {
    const size_t smem = (size_t)4 * ctx->cov_stride * sizeof(float);
    if (p.wgt) {   // weighted ratings
        if (fuse)
            hipLaunchKernelGGL((gauss_accum_mfma_kernel<KB, NT, true, KS, true>), grid, dim3(256), smem, ctx->stream, p, is2, ie2, cov, fac);
        else
            hipLaunchKernelGGL((gauss_accum_mfma_kernel<KB, NT, false, KB, true>), grid, dim3(256), smem, ctx->stream, p, 0.f, 0.f,
                               (float *)nullptr, (float *)nullptr);
        return;
    }
    if (fuse)
        hipLaunchKernelGGL((gauss_accum_mfma_kernel<KB, NT, true, KS>), grid, dim3(256), smem, ctx->stream, p.plain(), is2, ie2, cov, fac);
    else
        hipLaunchKernelGGL((gauss_accum_mfma_kernel<KB, NT, false>), grid, dim3(256), smem, ctx->stream, p.plain(), 0.f, 0.f,
                           (float *)nullptr, (float *)nullptr);
}

// K <= 64, fp32: pick the instantiation by MFMA block count and packed-row chunk count
static void launch_accum_mfma(pmf_ctx *ctx, const GaussParamsW<float> &p, dim3 grid, bool fuse, float is2, float ie2,
                              float *cov, float *fac) {
    const int nt = (ctx->cov_stride / PMF_VEC + 63) / 64;  // 1..9
    if (ctx->K <= 8) {
        launch_accum_mfma_nt<32, 1, 8>(ctx, p, grid, fuse, is2, ie2, cov, fac);
    } else if (ctx->K <= 16) {
        launch_accum_mfma_nt<32, 1, 16>(ctx, p, grid, fuse, is2, ie2, cov, fac);
    } else if (ctx->K <= 32) {
        switch (nt) {
            case 1: launch_accum_mfma_nt<32, 1>(ctx, p, grid, fuse, is2, ie2, cov, fac); break;
            case 2: launch_accum_mfma_nt<32, 2>(ctx, p, grid, fuse, is2, ie2, cov, fac); break;
            default: launch_accum_mfma_nt<32, 3>(ctx, p, grid, fuse, is2, ie2, cov, fac); break;
        }
    } else if (ctx->K <= 48) {   // Kp <= 1176: 3..5 chunk columns; a 48-row sweep instead of the 64-row one
        switch (nt) {
            case 3: launch_accum_mfma_nt<64, 3, 48>(ctx, p, grid, fuse, is2, ie2, cov, fac); break;
            case 4: launch_accum_mfma_nt<64, 4, 48>(ctx, p, grid, fuse, is2, ie2, cov, fac); break;
            default: launch_accum_mfma_nt<64, 5, 48>(ctx, p, grid, fuse, is2, ie2, cov, fac); break;
        }
    } else if (ctx->K <= 56) {   // Kp <= 1596: 5..7 chunk columns; a 56-row sweep (K = 50 is in the reference's grid)
        switch (nt) {
            case 5: launch_accum_mfma_nt<64, 5, 56>(ctx, p, grid, fuse, is2, ie2, cov, fac); break;
            case 6: launch_accum_mfma_nt<64, 6, 56>(ctx, p, grid, fuse, is2, ie2, cov, fac); break;
            default: launch_accum_mfma_nt<64, 7, 56>(ctx, p, grid, fuse, is2, ie2, cov, fac); break;
        }
    } else {
        switch (nt) {
            case 3: launch_accum_mfma_nt<64, 3>(ctx, p, grid, fuse, is2, ie2, cov, fac); break;
            case 4: launch_accum_mfma_nt<64, 4>(ctx, p, grid, fuse, is2, ie2, cov, fac); break;
            case 5: launch_accum_mfma_nt<64, 5>(ctx, p, grid, fuse, is2, ie2, cov, fac); break;
            case 6: launch_accum_mfma_nt<64, 6>(ctx, p, grid, fuse, is2, ie2, cov, fac); break;
            case 7: launch_accum_mfma_nt<64, 7>(ctx, p, grid, fuse, is2, ie2, cov, fac); break;
            case 8: launch_accum_mfma_nt<64, 8>(ctx, p, grid, fuse, is2, ie2, cov, fac); break;
            default: launch_accum_mfma_nt<64, 9>(ctx, p, grid, fuse, is2, ie2, cov, fac); break;
        }
    }
}

// MT = 16-row tiles per dimension of the fused MFMA block sweep: ceil(K / 16), from K alone.  NT follows the chunk
// count and its classes end elsewhere (NT = 9 reaches K = 95, NT = 13 K = 114), so NT = 13 meets MT = 8 at K = 113, 114.
template <int NT, int MT>
static void launch_accum_mfma128_fused(pmf_ctx *ctx, const GaussParamsW<float> &p, dim3 grid, size_t smem, float is2, float ie2,
                                       float *cov, float *fac) {
    if (p.wgt)
        hipLaunchKernelGGL((gauss_accum_mfma128_kernel<NT, true, MT, true>), grid, dim3(128), smem, ctx->stream, p, is2, ie2, cov, fac);
    else
        hipLaunchKernelGGL((gauss_accum_mfma128_kernel<NT, true, MT>), grid, dim3(128), smem, ctx->stream, p.plain(), is2, ie2, cov, fac);
}

template <int NT>
static void launch_accum_mfma128(pmf_ctx *ctx, const GaussParamsW<float> &p, dim3 grid, size_t smem, bool fuse, float is2,
                                 float ie2, float *cov, float *fac) {
    if (!fuse) {
        if (p.wgt)
            hipLaunchKernelGGL((gauss_accum_mfma128_kernel<NT, false, 0, true>), grid, dim3(128), smem, ctx->stream, p, 0.f, 0.f,
                               (float *)nullptr, (float *)nullptr);
        else
            hipLaunchKernelGGL((gauss_accum_mfma128_kernel<NT, false>), grid, dim3(128), smem, ctx->stream, p.plain(), 0.f, 0.f,
                               (float *)nullptr, (float *)nullptr);
        return;
    }
    const int mt = (ctx->K + 15) / 16;   // 5..8
    if constexpr (NT == 9) {          // 64 < K <= 95: 5 or 6 tiles
        if (mt <= 5) launch_accum_mfma128_fused<NT, 5>(ctx, p, grid, smem, is2, ie2, cov, fac);
        else launch_accum_mfma128_fused<NT, 6>(ctx, p, grid, smem, is2, ie2, cov, fac);
    } else if constexpr (NT == 13) {  // 96 <= K <= 114: 6, 7 or 8 tiles
        if (mt <= 6) launch_accum_mfma128_fused<NT, 6>(ctx, p, grid, smem, is2, ie2, cov, fac);
        else if (mt == 7) launch_accum_mfma128_fused<NT, 7>(ctx, p, grid, smem, is2, ie2, cov, fac);
        else launch_accum_mfma128_fused<NT, 8>(ctx, p, grid, smem, is2, ie2, cov, fac);
    } else {                          // 115 <= K <= 128: 8 tiles
        launch_accum_mfma128_fused<NT, 8>(ctx, p, grid, smem, is2, ie2, cov, fac);
    }
}

// fp32, K <= 128: the MFMA accumulate kernels.  Returns whether they also solved the rows that are one task (`fuse`:
// the fused pass sums in place, so the solved rows go where the sums went, `cov` / `fac` = COV / FACTOR).
static bool launch_accum_mfma_fp32(pmf_ctx *ctx, const GaussParamsW<float> &p, bool fuse, float is2, float ie2, float *cov, float *fac) {
    if (ctx->K <= 64) {
        launch_accum_mfma(ctx, p, dim3((unsigned)((p.n_tasks + 3) / 4)), fuse, is2, ie2, cov, fac);
    } else {  // 64 < K <= 128: one 128-thread block (two wavefronts) per task
        const size_t smem = (size_t)PAIR_LDS_FLOATS * sizeof(float);
        dim3 g2((unsigned)p.n_tasks);
        const int chunks = ctx->cov_stride / PMF_VEC, nt = ((chunks + 1) / 2 + 63) / 64;
        if (nt <= 9) launch_accum_mfma128<9>(ctx, p, g2, smem, fuse, is2, ie2, cov, fac);
        else if (nt <= 13) launch_accum_mfma128<13>(ctx, p, g2, smem, fuse, is2, ie2, cov, fac);
        else launch_accum_mfma128<17>(ctx, p, g2, smem, fuse, is2, ie2, cov, fac);
    }
    return fuse;
}

// fp64, fp32 with PMF_GAUSS_GENERIC, and 128 < K <= 256 (no reference configuration is this large): the generic
// accumulate kernel.  Returns whether it also solved the rows that are one task (`fuse`, K <= 64: fp64 only -- the
// fp32 build has no fused generic kernel, so fuse / is2 / ie2 do not apply to it).
template <typename T>
static bool launch_accum_generic(pmf_ctx *ctx, const GaussParamsW<T> &p, bool fuse, T is2, T ie2, T *cov, T *fac) {
    dim3 grid((unsigned)((p.n_tasks + 3) / 4));
    const size_t plain = (size_t)4 * 2 * ctx->kpad * sizeof(T), lds = plain + (size_t)4 * ctx->cov_stride * sizeof(T);
    if constexpr (std::is_same<T, double>::value) {
        if (fuse) {
            pmf_with_pow2<8>(ctx->K, [&](auto KR) {
                if (p.wgt)
                    hipLaunchKernelGGL((gauss_accum_generic_kernel<T, KR, true>), grid, dim3(256), lds, ctx->stream, p, is2, ie2, cov, fac);
                else
                    hipLaunchKernelGGL((gauss_accum_generic_kernel<T, KR>), grid, dim3(256), lds, ctx->stream, p.plain(), is2, ie2, cov, fac);
            });
            return true;
        }
    }
    if (p.wgt)
        hipLaunchKernelGGL((gauss_accum_generic_kernel<T, 0, true>), grid, dim3(256), plain, ctx->stream, p, (T)0, (T)0,
                           (T *)nullptr, (T *)nullptr);
    else
        hipLaunchKernelGGL((gauss_accum_generic_kernel<T, 0>), grid, dim3(256), plain, ctx->stream, p.plain(), (T)0, (T)0,
                           (T *)nullptr, (T *)nullptr);
    return false;
}

// FACTOR and COV of `side`, then (with `both`) of the other side, have been set: PMF_EINVAL in the name of `fn` if not
static int gauss_require_state(pmf_ctx *ctx, int side, bool both, const char *fn) {
    int rc = pmf_require_array(ctx, side, PMF_ARR_FACTOR, fn);
    if (!rc) rc = pmf_require_array(ctx, side, PMF_ARR_COV, fn);
    return rc || !both ? rc : gauss_require_state(ctx, 1 - side, false, fn);
}

// What the accumulate kernels take from the context: the gathered tables of the other side, `side`'s ratings, hot
// flags and bias, the partial slots and the geometry.  The caller sets the tasks and the split rows.
template <typename T>
static GaussParamsW<T> gauss_params(const pmf_ctx *ctx, int side) {
    const int other = 1 - side;
    const PmfSideIndex &ix = ctx->index[side];
    const bool bias = pmf_has_bias(ctx);
    GaussParamsW<T> p;
    p.other = ix.d_other.as<int32_t>();
    p.val = ix.d_val.as<const T>();
    p.factor_other = ctx->arr[other][PMF_ARR_FACTOR].as<const T>();
    p.cov_other = ctx->arr[other][PMF_ARR_COV].as<const T>();
    p.hot = ix.d_other_hot.as<uint8_t>();
    p.bias_self = bias ? ctx->arr[side][PMF_ARR_BIAS].as<const T>() : nullptr;
    p.bias_other = bias ? ctx->arr[other][PMF_ARR_BIAS].as<const T>() : nullptr;
    p.partial = ctx->d_partial.as<T>();
    p.K = ctx->K;
    p.kpad = ctx->kpad;
    p.kp = ctx->kp;
    p.cov_stride = ctx->cov_stride;
    p.wgt = ctx->weighted ? ix.d_wgt.as<const T>() : nullptr;
    p.zero_w = pmf_gauss_zeros_observed(ctx) ? (T)ctx->gauss_zero_weight : (T)0;
    return p;
}

// S and w of p's tasks into `st` by the accumulate kernel for the context's K and dtype, then the combine of the `n_split`
// split rows p.split lists.  `fuse`: the sums go in place (`st` is COV / FACTOR) and the kernel, where it has a fused
// form, also solves every row that is one task; *solved tells whether it did, so that the caller solves the rest.
template <typename T>
static int launch_accumulate(pmf_ctx *ctx, GaussParamsW<T> &p, int64_t n_split, const GaussStats<T> &st, bool fuse = false,
                             double sigma2 = 1, double eta2 = 1, bool *solved = nullptr) {
    bool did = false;
    st.set_dst(p);
    if (p.n_tasks > 0) {
        PmfProfScope prof(ctx, PMF_KERNEL_GAUSS_ACCUM);
        const T is2 = (T)(1.0 / sigma2), ie2 = (T)(1.0 / eta2);
        if (std::is_same<T, float>::value && !ctx->gauss_generic && ctx->K <= 128) {
            if constexpr (std::is_same<T, float>::value) did = launch_accum_mfma_fp32(ctx, p, fuse, is2, ie2, st.s, st.w);
        } else {
            did = launch_accum_generic(ctx, p, fuse && ctx->K <= 64, is2, ie2, st.s, st.w);
        }
    }
    if (solved) *solved = did;
    if (n_split > 0) {
        PmfProfScope prof(ctx, PMF_KERNEL_GAUSS_COMBINE);
        hipLaunchKernelGGL((gauss_combine_kernel<T>), dim3((unsigned)n_split), dim3(256), 0, ctx->stream, p.plain());
    }
    PMF_HIP_CHECK(hipGetLastError());
    return PMF_OK;
}

// GaussParams::partial_h of the fused factor sweep: behind the partial slots, and behind it GaussParams::hsplit
template <typename T>
static T *gauss_partial_h(const pmf_ctx *ctx, const PmfTaskView &tl) {
    return ctx->d_partial.as<T>() + tl.n_slots * (ctx->cov_stride + ctx->kpad);
}

// The fused pass sums in place into COV / FACTOR, the accumulate pass into `stats`.  *fused (fused pass): the kernel
// also solved every single-task row, so the caller only solves the split rows.  *sums (fused pass): the kernel also
// emits the mean sums of the bias sweep (GaussParams::mdot) -- only the fused fp32 K <= 64 kernel of a context with
// biases and without a communicator does.
template <typename T>
static int run_factor_accumulate(pmf_ctx *ctx, int side, PmfPass pass, void *stats, double sigma2, double eta2,
                                 bool *fused = nullptr, bool *sums = nullptr) {
    const PmfSideIndex &ix = ctx->index[side];
    const bool acc = pass == PMF_PASS_ACCUMULATE;
    const PmfTaskView tl = pmf_task_view(ctx, side, ix.gauss_tasks, acc);
    int rc;
    PMF_REQUIRE(ix.d_ptr, PMF_EINVAL, "pmf_gauss_factor_sweep: ratings have not been set");
    if ((rc = gauss_require_state(ctx, side, true, "pmf_gauss_factor_sweep"))) return rc;
    const int width = ctx->cov_stride + ctx->kpad;
    const bool fuse = !acc && !ctx->gauss_unfused;
    const bool emit = sums && fuse && std::is_same<T, float>::value && !ctx->gauss_generic && ctx->K <= 64 &&
                      !ctx->gauss_bias_gather && pmf_has_bias(ctx) && !pmf_comm_active(ctx);
    const size_t h_elems = emit ? (size_t)(tl.n_slots + tl.n_split) * ctx->kpad : 0;
    if (tl.n_slots > 0 && (rc = pmf_ensure_partial(ctx, ((size_t)tl.n_slots * width + h_elems) * sizeof(T)))) return rc;
    if (emit && (rc = ctx->d_mdot[side].reserve(ctx, (size_t)ctx->rows[side] * sizeof(T), {ctx->stream}))) return rc;
    if (acc && tl.row1 > tl.row0)  // rows without ratings on this rank contribute zeros
        PMF_HIP_CHECK(hipMemsetAsync((T *)stats + tl.row0 * width, 0, (size_t)(tl.row1 - tl.row0) * width * sizeof(T), ctx->stream));
    GaussParamsW<T> p = gauss_params<T>(ctx, side);
    p.tasks = tl.d_tasks;
    p.n_tasks = tl.n_tasks;
    p.split = tl.d_split;
    if (emit) {
        p.mdot = ctx->d_mdot[side].as<T>();
        p.partial_h = gauss_partial_h<T>(ctx, tl);
        p.hsplit = p.partial_h + tl.n_slots * ctx->kpad;
    }
    if (sums) *sums = emit;
    const GaussStats<T> st = acc ? GaussStats<T>::interleaved(ctx, (T *)stats, 0) : GaussStats<T>::in_place(ctx, side);
    return launch_accumulate<T>(ctx, p, tl.n_split, st, fuse, sigma2, eta2, fused);
}

// Where a block-per-row kernel (row solver, ELBO row pass, posterior draws at K > 64) keeps a row's matrix of `mat` bytes:
// in LDS while it fits the CU's 160 KB beside the kernel's `vecs` bytes of vectors and its static LDS; else every resident
// block has a slice of global scratch, and at most `cap` blocks walk the rows.
struct RowMatrixPlan {
    size_t mat, vecs;
    int64_t cap;
    bool in_lds;
    RowMatrixPlan(size_t mat, size_t vecs, size_t static_lds, int64_t cap)
        : mat(mat), vecs(vecs), cap(cap), in_lds(mat + vecs + static_lds <= (size_t)160 * 1024) {}
    unsigned blocks(int64_t n) const { return (unsigned)std::min<int64_t>(n, in_lds ? n : cap); }
    size_t smem() const { return in_lds ? mat + vecs : vecs; }   // dynamic LDS
    size_t scratch_bytes(int64_t n) const { return in_lds ? 0 : (size_t)blocks(n) * mat; }
};

// the row solver for the context's K and dtype over the rows `sp` names
template <typename T>
static int launch_solve(pmf_ctx *ctx, const SolveParams<T> &sp) {
    int rc;
    if (sp.n == 0) return PMF_OK;
    PmfProfScope prof(ctx, PMF_KERNEL_GAUSS_SOLVE);
    if (ctx->K <= 64)
        pmf_with_pow2<8>(ctx->K, [&](auto KR) {
            hipLaunchKernelGGL((gauss_solve_reg_kernel<T, KR>), dim3((unsigned)((sp.n + 3) / 4)), dim3(256),
                               (size_t)4 * ctx->cov_stride * sizeof(T), ctx->stream, sp);
        });
    else if (std::is_same<T, float>::value && !ctx->gauss_lds_solve && ctx->K <= 128) {
        if constexpr (std::is_same<T, float>::value) {
            const size_t smem = (size_t)PAIR_LDS_FLOATS * sizeof(float);
            switch ((ctx->K + 15) / 16) {
                case 5: hipLaunchKernelGGL((gauss_solve_pair_kernel<5>), dim3((unsigned)sp.n), dim3(128), smem, ctx->stream, sp); break;
                case 6: hipLaunchKernelGGL((gauss_solve_pair_kernel<6>), dim3((unsigned)sp.n), dim3(128), smem, ctx->stream, sp); break;
                case 7: hipLaunchKernelGGL((gauss_solve_pair_kernel<7>), dim3((unsigned)sp.n), dim3(128), smem, ctx->stream, sp); break;
                default: hipLaunchKernelGGL((gauss_solve_pair_kernel<8>), dim3((unsigned)sp.n), dim3(128), smem, ctx->stream, sp); break;
            }
        }
    } else {
        const int K = ctx->K;
        const RowMatrixPlan plan((size_t)K * (K + 1) * sizeof(T), (size_t)3 * K * sizeof(T), 0, 2048);
        T *scratch = nullptr;
        if (!plan.in_lds) {   // one matrix per resident block (<= 2048 x 264 KB)
            if ((rc = pmf_ensure_scratch(ctx, plan.scratch_bytes(sp.n)))) return rc;
            scratch = ctx->d_scratch.as<T>();
        }
        if ((rc = pmf_allow_dynamic_lds((const void *)gauss_solve_lds_kernel<T>, plan.smem()))) return rc;
        hipLaunchKernelGGL((gauss_solve_lds_kernel<T>), dim3(plan.blocks(sp.n)), dim3(256), plan.smem(), ctx->stream, sp, scratch);
    }
    PMF_HIP_CHECK(hipGetLastError());
    return PMF_OK;
}

// A row solve from the statistics `src` into `dst`.s / .w (COV / FACTOR of a side, or a fold-in block in place), with the
// geometry and the two inverse variances; every row from 0 on unless the caller sets rows / row0, and the caller sets n.
template <typename T>
static SolveParams<T> solve_params(const pmf_ctx *ctx, double sigma2, double eta2, const GaussStats<T> &src, const GaussStats<T> &dst) {
    SolveParams<T> sp;
    src.set_src(sp);
    sp.cov = dst.s;
    sp.factor = dst.w;
    sp.rows = nullptr;
    sp.row0 = 0;
    sp.inv_sigma2 = (T)(1.0 / sigma2);
    sp.inv_eta2 = (T)(1.0 / eta2);
    sp.K = ctx->K;
    sp.kpad = ctx->kpad;
    sp.kp = ctx->kp;
    sp.cov_stride = ctx->cov_stride;
    return sp;
}

// ---------------------------------------------------------------------------
// unlisted cells as weighted zeros (pmf_ctx_set_gauss_zeros, PMF_ZEROS_OBSERVED): Gram matrix and blend
// ---------------------------------------------------------------------------
// G[p] = sum over ALL rows r of a side of V_r[p] + m_r[row p] m_r[col p], p over the packed lower triangle: the S every
// row of the other side would accumulate if all cells were listed.  One streaming pass over COV, two stages, no atomics
// and no work list:
//   stage 1  grid (column tiles, row blocks).  A tile is kGramTile 16-byte chunks (256 packed positions): lane l of every
//            wavefront owns chunk tile * 64 + l for every row, so the (row, col) of its four entries -- its mean indices --
//            are loop constants.  Block (t, b) owns the contiguous rows [rows b / NB, rows (b + 1) / NB); wavefront w adds
//            rows w, w + 4, ... of the range in ascending order, UN rows in flight (one 16-byte load per lane per row; the
//            UN mean rows are staged in the wavefront's LDS slice as doubles).  Every addend is (double)V + (double)m_r
//            (double)m_c, one fma, added in double; the four wavefronts' sums are added in wavefront order through LDS.
//   stage 2  one thread per packed position adds the NB block sums in block order; G goes out packed in double and, as
//            w0 G formed in double and rounded once, in the context dtype.
// Entries at or past kp (the padding of the packed row) come out as 0.
static const int kGramTile = 64;          // chunks per column tile = lanes of a wavefront
static const int kGramBlocks = 4096;      // blocks aimed at (column tiles x row blocks)
static const int kGramRowBlocks = 1024;   // row blocks at most

template <typename T>
__global__ __launch_bounds__(256) void gauss_gram_kernel(const T *cov, const T *factor, int64_t rows, int kpad, int kp,
                                                         int cov_stride, double *partial /* [gridDim.y][cov_stride] */) {
    constexpr int UN = 4;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    __shared__ double s_sum[4][kGramTile * PMF_VEC];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double *mw = reinterpret_cast<double *>(smem_raw) + (int64_t)wave * UN * kpad;   // [UN][kpad]
    const int chunks = cov_stride / PMF_VEC;
    const int q = min((int)blockIdx.x * kGramTile + lane, chunks - 1);   // clamped lanes are never stored
    int ri[PMF_VEC], ci[PMF_VEC];
#pragma unroll
    for (int e = 0; e < PMF_VEC; ++e) {
        ri[e] = ci[e] = 0;
        if (q * PMF_VEC + e < kp) tri_rc(q * PMF_VEC + e, ri[e], ci[e]);
    }
    const int64_t r0 = rows * (int64_t)blockIdx.y / gridDim.y, r1 = rows * ((int64_t)blockIdx.y + 1) / gridDim.y;
    double acc[PMF_VEC] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t r = r0 + wave; r < r1; r += 4 * UN) {
        Vec4<T> v[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const bool live = r + 4 * u < r1;                 // wave-uniform
            const int64_t rr = live ? r + 4 * u : r;          // (a row past the range: row r again, never added)
            v[u] = load4(cov + rr * cov_stride + (int64_t)q * PMF_VEC);
            for (int k = lane; k < kpad; k += 64) mw[u * kpad + k] = (double)factor[rr * kpad + k];
        }
        wave_lds_fence();
#pragma unroll
        for (int u = 0; u < UN; ++u)
            if (r + 4 * u < r1) {
#pragma unroll
                for (int e = 0; e < PMF_VEC; ++e) acc[e] += fma(mw[u * kpad + ri[e]], mw[u * kpad + ci[e]], (double)v[u].v[e]);
            }
        wave_lds_fence();
    }
#pragma unroll
    for (int e = 0; e < PMF_VEC; ++e) s_sum[wave][lane * PMF_VEC + e] = acc[e];
    __syncthreads();
    const int pos = (int)blockIdx.x * kGramTile * PMF_VEC + (int)threadIdx.x;
    if (pos < cov_stride) {
        const double t = ((s_sum[0][threadIdx.x] + s_sum[1][threadIdx.x]) + s_sum[2][threadIdx.x]) + s_sum[3][threadIdx.x];
        partial[(int64_t)blockIdx.y * cov_stride + pos] = pos < kp ? t : 0.0;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void gauss_gram_final_kernel(const double *partial, int n_blocks, int cov_stride, double w0,
                                                               double *g, T *gw) {
    const int pos = (int)(blockIdx.x * 256 + threadIdx.x);
    if (pos >= cov_stride) return;
    double t = 0.0;
#pragma unroll 8
    for (int b = 0; b < n_blocks; ++b) t += partial[(int64_t)b * cov_stride + pos];
    g[pos] = t;
    gw[pos] = (T)(w0 * t);
}

// S[p] = fma(T(1 - w0), S[p], gw[p]) over the packed S of `n` statistics rows `stride` elements apart; what follows S
// in a row (the right-hand side) is not touched.  One 16-byte chunk per thread.
template <typename T>
__global__ __launch_bounds__(256) void gauss_zero_blend_kernel(T *stats, int64_t n, int64_t stride, int chunks, T one_minus_w0,
                                                               const T *gw) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n * chunks) return;
    const int64_t row = idx / chunks;
    const int q = (int)(idx - row * chunks) * PMF_VEC;
    T *s = stats + row * stride + q;
    Vec4<T> v = load4(s);
    const Vec4<T> g = load4(gw + q);
#pragma unroll
    for (int e = 0; e < PMF_VEC; ++e) v.v[e] = fma(one_minus_w0, v.v[e], g.v[e]);
    store4(s, v);
}

// the work area of the Gram pass in pmf_ctx::d_gauss_gram: block sums, packed G (double), w0 G (context dtype)
template <typename T>
struct GaussGram {
    int tiles, row_blocks;
    PmfLayout lay{256};
    PmfLayout::Piece<double> part_at, g_at;
    PmfLayout::Piece<T> gw_at;
    explicit GaussGram(const pmf_ctx *ctx)
        : tiles((ctx->cov_stride / PMF_VEC + kGramTile - 1) / kGramTile),
          row_blocks(std::max(1, std::min(kGramRowBlocks, kGramBlocks / tiles))),
          part_at(lay.add<double>((size_t)row_blocks * ctx->cov_stride)), g_at(lay.add<double>((size_t)ctx->cov_stride)),
          gw_at(lay.add<T>((size_t)ctx->cov_stride)) {}
};

// G of `side` and w0 G into the context's Gram work area (the two launches, in a profile bracket of their own: call it
// outside any other); *g / *gw stay valid until the next Gram pass of the context.
template <typename T>
static int gauss_gram_run(pmf_ctx *ctx, int side, const double **g, const T **gw) {
    const GaussGram<T> gg(ctx);
    int rc;
    if ((rc = ctx->d_gauss_gram.reserve(ctx, gg.lay.bytes(), {ctx->stream}))) return rc;
    void *base = ctx->d_gauss_gram.as();
    {
        PmfProfScope prof(ctx, PMF_KERNEL_GAUSS_COMBINE);
        hipLaunchKernelGGL((gauss_gram_kernel<T>), dim3((unsigned)gg.tiles, (unsigned)gg.row_blocks), dim3(256),
                           (size_t)4 * 4 * ctx->kpad * sizeof(double), ctx->stream, ctx->arr[side][PMF_ARR_COV].as<const T>(),
                           ctx->arr[side][PMF_ARR_FACTOR].as<const T>(), ctx->rows[side], ctx->kpad, ctx->kp, ctx->cov_stride,
                           gg.part_at.at(base));
        hipLaunchKernelGGL((gauss_gram_final_kernel<T>), dim3((unsigned)((ctx->cov_stride + 255) / 256)), dim3(256), 0, ctx->stream,
                           gg.part_at.at(base), gg.row_blocks, ctx->cov_stride, ctx->gauss_zero_weight, gg.g_at.at(base),
                           gg.gw_at.at(base));
    }
    PMF_HIP_CHECK(hipGetLastError());
    if (g) *g = gg.g_at.at(base);
    if (gw) *gw = gg.gw_at.at(base);
    return PMF_OK;
}

// *gw = w0 G of the side opposite `side`, for the blend of `side`'s statistics; null when unlisted cells are missing
template <typename T>
static int gauss_zero_gram(pmf_ctx *ctx, int side, const T **gw) {
    *gw = nullptr;
    return pmf_gauss_zeros_observed(ctx) ? gauss_gram_run<T>(ctx, 1 - side, nullptr, gw) : PMF_OK;
}

// The statistics of the first `n_rows` rows of `st`, the one way for the window and block loops: accumulate p's tasks,
// combine the split rows and, with gw (gauss_zero_gram), blend every row's S with w0 G (timed with the combine; weighted
// tasks have summed (c_j - w0) A_j, so their blend is S + w0 G).
// `zero_first` clears the rows before that.  The rule: zero when a row that no task writes -- a row without ratings --
// will be read.  Fold-in solves every row of a block, and under PMF_ZEROS_OBSERVED every row of a window is blended and
// read; the default-mode ELBO never zeroes: its row kernel reads neither the statistics nor c_r of a row without ratings.
template <typename T>
static int gauss_block_stats(pmf_ctx *ctx, GaussParamsW<T> &p, int64_t n_split, const GaussStats<T> &st, int64_t n_rows,
                             bool zero_first, const T *gw) {
    int rc;
    if (zero_first) PMF_HIP_CHECK(hipMemsetAsync(st.s, 0, (size_t)n_rows * st.s_stride * sizeof(T), ctx->stream));
    if (zero_first && !st.one_buffer) PMF_HIP_CHECK(hipMemsetAsync(st.w, 0, (size_t)n_rows * st.w_stride * sizeof(T), ctx->stream));
    if ((rc = launch_accumulate<T>(ctx, p, n_split, st))) return rc;
    if (!gw || n_rows == 0) return PMF_OK;
    const int chunks = ctx->cov_stride / PMF_VEC;
    PmfProfScope prof(ctx, PMF_KERNEL_GAUSS_COMBINE);
    hipLaunchKernelGGL((gauss_zero_blend_kernel<T>), dim3((unsigned)((n_rows * chunks + 255) / 256)), dim3(256), 0, ctx->stream, st.s,
                       n_rows, st.s_stride, chunks, p.wgt ? (T)1 : (T)(1.0 - ctx->gauss_zero_weight), gw);
    PMF_HIP_CHECK(hipGetLastError());
    return PMF_OK;
}

static const int64_t kWindowStatsBytes = 256ll << 20;   // statistics of one row window (PmfRowWindows)
// The side's windows (built once per set of ratings) and the partial slots of their split rows.  *win_rows = the rows of
// a full window: what fits kWindowStatsBytes, at most PMF_ELBO_ROWS.
template <typename T>
static int gauss_ensure_windows(pmf_ctx *ctx, int side, int64_t *win_rows) {
    const int64_t rows = ctx->rows[side], width = ctx->cov_stride + ctx->kpad;
    const int64_t by_bytes = std::max<int64_t>(1, kWindowStatsBytes / (width * (int64_t)sizeof(T)));
    *win_rows = std::min(ctx->window_rows > 0 ? std::min(ctx->window_rows, by_bytes) : by_bytes, rows);
    const std::vector<int64_t> &ptr = ctx->index[side].h_ptr;
    PmfRowWindows &rw = ctx->index[side].windows;
    int rc;
    if (rw.bounds.empty()) {
        std::vector<int64_t> bounds;
        for (int64_t r = 0; r < rows; r += *win_rows) bounds.push_back(r);
        bounds.push_back(rows);
        PmfTaskList tl;   // (no solve list: a window's rows are all solved, or none is)
        if ((rc = pmf_upload_tasks(ctx, ptr, rows, pmf_task_chunk(ctx, PMF_GAUSS_CHUNK), false, bounds, false, tl))) return rc;
        rw.has_empty.assign(bounds.size() - 1, 0);
        for (size_t w = 0; w + 1 < bounds.size(); ++w)
            rw.has_empty[w] = std::adjacent_find(ptr.begin() + bounds[w], ptr.begin() + bounds[w + 1] + 1) != ptr.begin() + bounds[w + 1] + 1;
        rw.tasks = std::move(tl);
        rw.bounds.swap(bounds);
    }
    return rw.tasks.n_slots > 0 ? pmf_ensure_partial(ctx, (size_t)rw.tasks.n_slots * width * sizeof(T)) : PMF_OK;
}

// the tasks and split rows of window `w` (rows bounds[w] .. bounds[w + 1]) into `p`; returns the window's split-row count
template <typename T>
static int64_t gauss_window_tasks(const PmfRowWindows &rw, size_t w, GaussParamsW<T> &p) {
    const PmfTaskList &tl = rw.tasks;
    p.tasks = tl.d_tasks.as<PmfTask>() + tl.task_off[w];
    p.n_tasks = tl.task_off[w + 1] - tl.task_off[w];
    p.split = tl.d_split.as<PmfSplitRow>() + tl.split_off[w];
    return tl.split_off[w + 1] - tl.split_off[w];
}

extern "C" int pmf_gauss_gram(pmf_ctx *ctx, int side, double *out) {
    PMF_SIDE_ENTRY("pmf_gauss_gram");
    PMF_REQUIRE(out != nullptr, PMF_EINVAL, "pmf_gauss_gram: null out");
    int rc;
    if ((rc = gauss_require_state(ctx, side, false, "pmf_gauss_gram"))) return rc;
    return pmf_no_throw("pmf_gauss_gram", [&] {
        return pmf_with_dtype(ctx, [&](auto t) {
            using T = decltype(t);
            const double *g = nullptr;
            int rc2;
            if ((rc2 = gauss_gram_run<T>(ctx, side, &g, nullptr))) return rc2;
            std::vector<double> packed((size_t)ctx->cov_stride);
            PMF_HIP_CHECK(hipMemcpyAsync(packed.data(), g, packed.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
            PMF_HIP_CHECK(hipStreamSynchronize(ctx->stream));
            const int K = ctx->K;
            for (int i = 0; i < K; ++i)
                for (int j = 0; j <= i; ++j) out[(size_t)i * K + j] = out[(size_t)j * K + i] = packed[(size_t)i * (i + 1) / 2 + j];
            return (int)PMF_OK;
        });
    });
}

// finalize pass: every row of the selected range from `stats`; fused pass: the rows with ratings (the split rows only
// when the accumulate kernel solved the others) from the sums in COV / FACTOR.  `sums` (with split_rows_only): the
// accumulate emitted the mean sums, so the split rows' solve completes ctx->d_mdot[side].
template <typename T>
static int run_factor_solve(pmf_ctx *ctx, int side, PmfPass pass, const void *stats, double sigma2, double eta2,
                            bool split_rows_only = false, bool sums = false) {
    PMF_REQUIRE(sigma2 > 0 && eta2 > 0, PMF_EINVAL, "pmf_gauss_factor_sweep: variances must be positive");
    int rc;
    if ((rc = gauss_require_state(ctx, side, false, "pmf_gauss_factor_finalize"))) return rc;
    const bool fin = pass == PMF_PASS_FINALIZE;
    const PmfTaskView tl = pmf_task_view(ctx, side, ctx->index[side].gauss_tasks, fin);
    const GaussStats<T> self = GaussStats<T>::in_place(ctx, side);
    SolveParams<T> sp = solve_params<T>(ctx, sigma2, eta2, fin ? GaussStats<T>::interleaved(ctx, (T *)stats, 0) : self, self);
    sp.rows = fin ? nullptr : split_rows_only ? tl.d_split_rows : tl.d_nonempty;
    sp.row0 = fin ? tl.row0 : 0;
    sp.n = fin ? tl.row1 - tl.row0 : split_rows_only ? tl.n_split : tl.n_nonempty;
    if (sums && split_rows_only && sp.n > 0) {
        sp.hsum = gauss_partial_h<T>(ctx, tl) + tl.n_slots * ctx->kpad;
        sp.mdot = ctx->d_mdot[side].as<T>();
    }
    return launch_solve<T>(ctx, sp);
}

// pmf_gauss_factor_sweep under PMF_ZEROS_OBSERVED: G of the other side, then per row window of the side the listed sums
// into the context's window (zeroed first where the window has rows no task writes), blended with w0 G, and a solve of
// every row of the window into COV / FACTOR.
template <typename T>
static int run_zero_sweep(pmf_ctx *ctx, int side, double sigma2, double eta2) {
    const PmfRowWindows &rw = ctx->index[side].windows;
    int64_t win_rows;
    int rc;
    PMF_REQUIRE(ctx->index[side].d_ptr, PMF_EINVAL, "pmf_gauss_factor_sweep: ratings have not been set");
    if ((rc = gauss_require_state(ctx, side, true, "pmf_gauss_factor_sweep"))) return rc;
    if ((rc = gauss_ensure_windows<T>(ctx, side, &win_rows))) return rc;
    if ((rc = ctx->d_gauss_window.reserve(ctx, (size_t)win_rows * (ctx->cov_stride + ctx->kpad) * sizeof(T), {ctx->stream}))) return rc;
    const T *gw;
    if ((rc = gauss_zero_gram<T>(ctx, side, &gw))) return rc;
    GaussParamsW<T> p = gauss_params<T>(ctx, side);
    for (size_t w = 0; w + 1 < rw.bounds.size(); ++w) {
        const int64_t r0 = rw.bounds[w], n = rw.bounds[w + 1] - r0, ns = gauss_window_tasks<T>(rw, w, p);
        const GaussStats<T> st = GaussStats<T>::interleaved(ctx, ctx->d_gauss_window.as<T>(), r0);   // (tasks carry the row's id in the side)
        if ((rc = gauss_block_stats<T>(ctx, p, ns, st, n, rw.has_empty[w], gw))) return rc;
        // (no row list: every row is solved, S'[0] = (1 - w0) S[0] + w0 G[0] > 0)
        SolveParams<T> sp = solve_params<T>(ctx, sigma2, eta2, st, GaussStats<T>::in_place(ctx, side));
        sp.row0 = r0;
        sp.n = n;
        if ((rc = launch_solve<T>(ctx, sp))) return rc;
    }
    return PMF_OK;
}

extern "C" int pmf_gauss_factor_sweep(pmf_ctx *ctx, int side, double sigma2, double eta2) {
    PMF_SIDE_ENTRY("pmf_gauss_factor_sweep");
    PMF_REQUIRE(sigma2 > 0 && eta2 > 0, PMF_EINVAL, "pmf_gauss_factor_sweep: variances must be positive");
    PMF_REQUIRE_ZERO_MODE_BIAS_FREE("pmf_gauss_factor_sweep");
    pmf_factor_written(ctx);   // the other side's mean sums were taken against this side's old means
    if (pmf_gauss_zeros_observed(ctx))   // (never with a communicator)
        return pmf_no_throw("pmf_gauss_factor_sweep", [&] {
            return pmf_with_dtype(ctx, [&](auto t) { return run_zero_sweep<decltype(t)>(ctx, side, sigma2, eta2); });
        });
    return pmf_with_dtype(ctx, [&](auto t) {
        using T = decltype(t);
        if (side == PMF_SIDE_ITEM && pmf_comm_active(ctx)) {
            // several ranks (pmf_comm.hip): finalize = one K x K solve per row, and the finalised state ([Kp + Kpad] per row) is
            // as wide as the statistics: reduce-scatter -> solve 1/N of the rows -> all-gather moves the same bytes, 1/N the solves
            const PmfExchange ex = {true, 2, {PMF_ARR_FACTOR, PMF_ARR_COV}};
            return pmf_comm_half_sweep(ctx, side, 0, (size_t)ctx->cov_stride + ctx->kpad, true, ex,
                                       [&](void *s) { return run_factor_accumulate<T>(ctx, side, PMF_PASS_ACCUMULATE, s, 1.0, 1.0); },
                                       [&](void *s) { return run_factor_solve<T>(ctx, side, PMF_PASS_FINALIZE, s, sigma2, eta2); });
        }
        bool fused = false, sums = false;
        int rc = run_factor_accumulate<T>(ctx, side, PMF_PASS_FUSED, nullptr, sigma2, eta2, &fused, &sums);
        if (!rc) rc = run_factor_solve<T>(ctx, side, PMF_PASS_FUSED, nullptr, sigma2, eta2, fused, fused && sums);
        // every row with ratings was solved with its mean sums at hand: by the accumulate kernel or as a split row
        if (!rc && fused && sums) ctx->gauss_mdot_valid[side] = true;
        return rc;
    });
}

extern "C" int pmf_gauss_factor_accumulate(pmf_ctx *ctx, int side, void *stats_dev) {
    PMF_SIDE_ENTRY("pmf_gauss_factor_accumulate");
    PMF_REQUIRE_GAUSS_ZEROS_MISSING("pmf_gauss_factor_accumulate");
    PMF_REQUIRE(stats_dev, PMF_EINVAL, "pmf_gauss_factor_accumulate: null stats buffer");
    return pmf_with_dtype(ctx, [&](auto t) { return run_factor_accumulate<decltype(t)>(ctx, side, PMF_PASS_ACCUMULATE, stats_dev, 1, 1); });
}

extern "C" int pmf_gauss_factor_finalize(pmf_ctx *ctx, int side, const void *stats_dev, double sigma2,
                                         double eta2) {
    PMF_SIDE_ENTRY("pmf_gauss_factor_finalize");
    PMF_REQUIRE_GAUSS_ZEROS_MISSING("pmf_gauss_factor_finalize");
    PMF_REQUIRE(stats_dev, PMF_EINVAL, "pmf_gauss_factor_finalize: null stats buffer");
    pmf_factor_written(ctx);
    return pmf_with_dtype(ctx, [&](auto t) { return run_factor_solve<decltype(t)>(ctx, side, PMF_PASS_FINALIZE, stats_dev, sigma2, eta2); });
}

// ---- bias ------------------------------------------------------------------
template <typename T>
static int run_bias(pmf_ctx *ctx, int side, PmfPass pass, void *stats, double sigma2, double eta_bias2) {
    const int other = 1 - side;
    const PmfSideIndex &ix = ctx->index[side];
    const PmfTaskView tl = pmf_task_view(ctx, side, ix.bias_tasks, pass != PMF_PASS_FUSED);
    const bool acc = pass == PMF_PASS_ACCUMULATE;
    int rc;
    PMF_REQUIRE(ix.d_ptr, PMF_EINVAL, "pmf_gauss_bias_sweep: ratings have not been set");
    if ((rc = pmf_require_array(ctx, side, PMF_ARR_FACTOR, "pmf_gauss_bias_sweep"))) return rc;
    if ((rc = pmf_require_array(ctx, other, PMF_ARR_FACTOR, "pmf_gauss_bias_sweep"))) return rc;
    if ((rc = pmf_require_array(ctx, side, PMF_ARR_BIAS, "pmf_gauss_bias_sweep"))) return rc;
    if ((rc = pmf_require_array(ctx, other, PMF_ARR_BIAS, "pmf_gauss_bias_sweep"))) return rc;
    if (!acc) PMF_REQUIRE(sigma2 > 0 && eta_bias2 > 0, PMF_EINVAL, "pmf_gauss_bias_sweep: variances must be positive");
    if (pass != PMF_PASS_FINALIZE && tl.n_slots > 0 && (rc = pmf_ensure_partial(ctx, (size_t)tl.n_slots * sizeof(T)))) return rc;
    BiasParams<T> p;
    p.tasks = tl.d_tasks;
    p.n_tasks = tl.n_tasks;
    p.split = tl.d_split;
    p.other = ix.d_other.as<int32_t>();
    p.val = ix.d_val.as<const T>();
    p.factor_self = ctx->arr[side][PMF_ARR_FACTOR].as<const T>();
    p.factor_other = ctx->arr[other][PMF_ARR_FACTOR].as<const T>();
    p.bias_self = ctx->arr[side][PMF_ARR_BIAS].as<T>();
    p.bias_other = ctx->arr[other][PMF_ARR_BIAS].as<const T>();
    p.partial = ctx->d_partial.as<T>();
    p.stats = (T *)stats;
    p.inv_sigma2 = acc ? (T)1 : (T)(1.0 / sigma2);
    p.inv_eta_bias2 = acc ? (T)1 : (T)(1.0 / eta_bias2);
    p.kpad = ctx->kpad;
    p.row0 = tl.row0;
    p.rows = tl.row1;
    if (ctx->weighted) {
        p.wgt = ix.d_wgt.as<const T>();
        p.wsum = ix.d_wsum.as<const T>();
    }
    // fused single-rank fp32 pass after this side's fused factor sweep, nothing written since: the sums form
    const bool from_sums = pass == PMF_PASS_FUSED && std::is_same<T, float>::value && ctx->gauss_mdot_valid[side] &&
                           !ctx->gauss_bias_gather && !pmf_comm_active(ctx);
    const T *mdot = from_sums ? ctx->d_mdot[side].as<const T>() : nullptr;
    PmfProfScope prof(ctx, PMF_KERNEL_GAUSS_BIAS);   // (the statistics memset included)
    if (pass == PMF_PASS_FINALIZE) {
        if (p.rows > p.row0)
            hipLaunchKernelGGL((gauss_bias_finalize_all_kernel<T>), dim3((unsigned)((p.rows - p.row0 + 255) / 256)), dim3(256), 0,
                               ctx->stream, p);
    } else {
        if (acc && p.rows > p.row0)
            PMF_HIP_CHECK(hipMemsetAsync((T *)stats + p.row0 * 2, 0, (size_t)(p.rows - p.row0) * 2 * sizeof(T), ctx->stream));
        if (tl.n_tasks > 0 && from_sums) {
            // a wavefront per task where the tasks are long (the benchmark's item side: 512), 16 lanes otherwise
            const bool wide = ctx->nnz / tl.n_tasks >= 64;
            const dim3 grid((unsigned)(wide ? (p.n_tasks + 3) / 4 : (p.n_tasks + 15) / 16));
            if (p.wgt) {
                if (wide) hipLaunchKernelGGL((gauss_bias_sums_kernel<T, 64, true>), grid, dim3(256), 0, ctx->stream, p, mdot);
                else hipLaunchKernelGGL((gauss_bias_sums_kernel<T, 16, true>), grid, dim3(256), 0, ctx->stream, p, mdot);
            } else if (wide)
                hipLaunchKernelGGL((gauss_bias_sums_kernel<T, 64>), grid, dim3(256), 0, ctx->stream, p, mdot);
            else
                hipLaunchKernelGGL((gauss_bias_sums_kernel<T, 16>), grid, dim3(256), 0, ctx->stream, p, mdot);
        } else if (tl.n_tasks > 0)
            pmf_with_pow2<1>(pmf_lanes_per_row(ctx->kpad), [&](auto L) {
                dim3 grid((unsigned)((p.n_tasks + 256 / L - 1) / (256 / L)));
                if (p.wgt) {
                    if (acc) hipLaunchKernelGGL((gauss_bias_kernel<T, L, true, true>), grid, dim3(256), 0, ctx->stream, p);
                    else hipLaunchKernelGGL((gauss_bias_kernel<T, L, false, true>), grid, dim3(256), 0, ctx->stream, p);
                } else if (acc) hipLaunchKernelGGL((gauss_bias_kernel<T, L, true>), grid, dim3(256), 0, ctx->stream, p);
                else hipLaunchKernelGGL((gauss_bias_kernel<T, L, false>), grid, dim3(256), 0, ctx->stream, p);
            });
        if (tl.n_split > 0) {
            dim3 grid((unsigned)((tl.n_split + 255) / 256));
            if (acc) hipLaunchKernelGGL((gauss_bias_split_kernel<T, true>), grid, dim3(256), 0, ctx->stream, p, tl.n_split, ix.d_ptr.as<int64_t>(), mdot);
            else hipLaunchKernelGGL((gauss_bias_split_kernel<T, false>), grid, dim3(256), 0, ctx->stream, p, tl.n_split, ix.d_ptr.as<int64_t>(), mdot);
        }
    }
    PMF_HIP_CHECK(hipGetLastError());
    return PMF_OK;
}

extern "C" int pmf_gauss_bias_sweep(pmf_ctx *ctx, int side, double sigma2, double eta_bias2) {
    PMF_SIDE_ENTRY("pmf_gauss_bias_sweep");
    PMF_REQUIRE_GAUSS_ZEROS_MISSING("pmf_gauss_bias_sweep");
    return pmf_with_dtype(ctx, [&](auto t) {
        using T = decltype(t);
        if (side != PMF_SIDE_ITEM || !pmf_comm_active(ctx)) return run_bias<T>(ctx, side, PMF_PASS_FUSED, nullptr, sigma2, eta_bias2);
        const PmfExchange ex = {false, 1, {PMF_ARR_BIAS}};   // several ranks: statistics [rows x 2], latency-bound, one message
        return pmf_comm_half_sweep(ctx, side, 1, 2, false, ex,
                                   [&](void *s) { return run_bias<T>(ctx, side, PMF_PASS_ACCUMULATE, s, 1, 1); },
                                   [&](void *s) { return run_bias<T>(ctx, side, PMF_PASS_FINALIZE, s, sigma2, eta_bias2); });
    });
}

extern "C" int pmf_gauss_bias_accumulate(pmf_ctx *ctx, int side, void *stats_dev) {
    PMF_SIDE_ENTRY("pmf_gauss_bias_accumulate");
    PMF_REQUIRE_GAUSS_ZEROS_MISSING("pmf_gauss_bias_accumulate");
    PMF_REQUIRE(stats_dev, PMF_EINVAL, "pmf_gauss_bias_accumulate: null stats buffer");
    return pmf_with_dtype(ctx, [&](auto t) { return run_bias<decltype(t)>(ctx, side, PMF_PASS_ACCUMULATE, stats_dev, 1, 1); });
}

extern "C" int pmf_gauss_bias_finalize(pmf_ctx *ctx, int side, const void *stats_dev, double sigma2,
                                       double eta_bias2) {
    PMF_SIDE_ENTRY("pmf_gauss_bias_finalize");
    PMF_REQUIRE_GAUSS_ZEROS_MISSING("pmf_gauss_bias_finalize");
    PMF_REQUIRE(stats_dev, PMF_EINVAL, "pmf_gauss_bias_finalize: null stats buffer");
    return pmf_with_dtype(ctx, [&](auto t) { return run_bias<decltype(t)>(ctx, side, PMF_PASS_FINALIZE, (void *)stats_dev, sigma2, eta_bias2); });
}

// ---- fold-in ---------------------------------------------------------------
static const int64_t kFoldInStatsBytes = 256ll << 20;   // statistics + partial slots of one row block
struct FoldInBatch {
    int64_t n_rows;
    const int64_t *row_ptr;
    const int32_t *other_ids;
    const double *ratings;
    const double *weights;   // [row_ptr[n_rows]] or null
    double sigma2, eta2, eta_bias2;
    int n_iter;
    double *out_factor, *out_cov, *out_bias;
};

// The batch in row blocks whose statistics ([cov_stride + kpad + 1] per row) and partial slots ([cov_stride + kpad] per
// task of a split row) fit kFoldInStatsBytes.  Per block: stage ratings and a task list, accumulate S and w0 with the
// sweep's kernels (accumulate-only form), solve in place, run the bias alternation, download.  Everything lives in
// buffers of this call: the context's model state, index and work lists are only read.
template <typename T>
static int run_fold_in(pmf_ctx *ctx, int side, const FoldInBatch &a) {
    const int K = ctx->K, kpad = ctx->kpad, cs = ctx->cov_stride, width = cs + kpad;
    const bool bias = pmf_has_bias(ctx);
    const int chunk = pmf_task_chunk(ctx, PMF_GAUSS_CHUNK);
    const int64_t max_units = std::max<int64_t>(1, kFoldInStatsBytes / ((int64_t)(width + 1) * (int64_t)sizeof(T)));
    const int64_t max_rows = ctx->fold_in_rows > 0 ? ctx->fold_in_rows : (int64_t)INT32_MAX;
    PmfFoldStage<T> st;
    PmfBuf d_tasks, d_split, d_s, d_w, d_b, d_partial;
    std::vector<int64_t> task_off, split_off;
    std::vector<PmfTask> tasks;
    std::vector<PmfSplitRow> split;
    int rc;
    // unlisted cells as weighted zeros: every row's S is blended with w0 G of the opposite side (formed once), and a row
    // without ratings is solved like the rest
    const T *gw;
    if ((rc = gauss_zero_gram<T>(ctx, side, &gw))) return rc;
    for (int64_t r0 = 0; r0 < a.n_rows; r0 = st.r1) {
        int64_t units = 0;   // a row's statistics, and the partial slots of a row that is split
        const auto fits = [&](int64_t n) { return (units += 1 + (n > chunk ? (n + chunk - 1) / chunk : 0)) <= max_units; };
        // (the previous block ended with a stream synchronise: nothing queued still reads the block's buffers)
        if ((rc = st.stage(ctx, a.n_rows, a.row_ptr, a.ratings, r0, max_rows, fits, a.weights))) return rc;
        const int64_t B = st.r1 - r0, nnz = st.nnz;
        const bool has_empty = std::adjacent_find(st.ptr.begin(), st.ptr.end()) != st.ptr.end();
        tasks.clear();
        split.clear();
        int64_t n_slots = 0;
        pmf_build_tasks(st.ptr, B, chunk, false, {0, B}, tasks, split, n_slots, task_off, split_off);
        if ((rc = d_tasks.reserve(ctx, tasks.size() * sizeof(PmfTask), {ctx->stream}))) return rc;
        if ((rc = d_split.reserve(ctx, split.size() * sizeof(PmfSplitRow), {ctx->stream}))) return rc;
        if ((rc = d_s.reserve(ctx, (size_t)B * cs * sizeof(T), {ctx->stream}))) return rc;
        if ((rc = d_w.reserve(ctx, (size_t)B * kpad * sizeof(T), {ctx->stream}))) return rc;
        if ((rc = d_b.reserve(ctx, (size_t)B * sizeof(T), {ctx->stream}))) return rc;
        if ((rc = d_partial.reserve(ctx, (size_t)n_slots * width * sizeof(T), {ctx->stream}))) return rc;
        if ((rc = st.upload(a.other_ids))) return rc;
        if (nnz) PMF_HIP_CHECK(hipMemcpy(d_tasks.as(), tasks.data(), tasks.size() * sizeof(PmfTask), hipMemcpyHostToDevice));
        if (!split.empty())
            PMF_HIP_CHECK(hipMemcpy(d_split.as(), split.data(), split.size() * sizeof(PmfSplitRow), hipMemcpyHostToDevice));
        GaussParamsW<T> p = gauss_params<T>(ctx, side);   // over the block's own buffers; no hot flags, and b = 0
        p.tasks = d_tasks.as<PmfTask>();
        p.n_tasks = (int64_t)tasks.size();
        p.split = d_split.as<PmfSplitRow>();
        p.other = st.d_other.template as<int32_t>();
        p.val = st.d_val.template as<const T>();
        p.wgt = a.weights ? st.d_wgt.template as<const T>() : nullptr;   // (the batch's own weights, not the context's)
        p.hot = nullptr;
        p.bias_self = nullptr;
        p.partial = d_partial.as<T>();
        const GaussStats<T> stats = GaussStats<T>::separate(ctx, d_s.as<T>(), d_w.as<T>());
        if ((rc = gauss_block_stats<T>(ctx, p, (int64_t)split.size(), stats, B, has_empty, gw))) return rc;
        SolveParams<T> sp = solve_params<T>(ctx, a.sigma2, a.eta2, stats, stats);   // (in place)
        sp.n = B;
        if ((rc = launch_solve<T>(ctx, sp))) return rc;
        if (bias) {
            FoldBiasParams<T> q;
            q.ptr = st.d_ptr.template as<const int64_t>();
            q.n = B;
            q.other = p.other;
            q.val = p.val;
            q.factor_other = p.factor_other;
            q.bias_other = p.bias_other;
            q.cov = d_s.as<const T>();
            q.factor = d_w.as<T>();
            q.bias = d_b.as<T>();
            q.inv_sigma2 = (T)(1.0 / a.sigma2);
            q.inv_eta_bias2 = (T)(1.0 / a.eta_bias2);
            q.n_iter = a.n_iter;
            q.K = K;
            q.kpad = kpad;
            q.cov_stride = cs;
            if (a.weights) {
                q.wgt = p.wgt;
                q.wsum = st.d_wsum.template as<const T>();
            }
            PmfProfScope prof(ctx, PMF_KERNEL_GAUSS_BIAS);
            pmf_with_pow2<1>(pmf_lanes_per_row(kpad), [&](auto L) {
                dim3 grid((unsigned)((B + 256 / L - 1) / (256 / L)));
                hipLaunchKernelGGL((gauss_fold_bias_kernel<T, L>), grid, dim3(256), 0, ctx->stream, q);
            });
        }
        PMF_HIP_CHECK(hipGetLastError());
        double *of = a.out_factor + r0 * K;
        double *oc = a.out_cov ? a.out_cov + r0 * (int64_t)K * K : nullptr;
        double *ob = a.out_bias ? a.out_bias + r0 : nullptr;
        // (every download ends with a stream synchronise: the block's kernels are done with the staging buffers)
        if ((rc = pmf_fold_in_download(ctx, PMF_ARR_FACTOR, d_w.as(), of, B))) return rc;
        if (oc && (rc = pmf_fold_in_download(ctx, PMF_ARR_COV, d_s.as(), oc, B))) return rc;
        if (ob && bias && (rc = pmf_fold_in_download(ctx, PMF_ARR_BIAS, d_b.as(), ob, B))) return rc;
        if (ob && !bias) std::fill_n(ob, (size_t)B, 0.0);
        for (int64_t r = 0; has_empty && !gw && r < B; ++r) {
            if (st.ptr[(size_t)r + 1] > st.ptr[(size_t)r]) continue;
            // a row without ratings gets the prior: m = 0, V = eta2 I, b = 0
            std::fill_n(of + r * K, (size_t)K, 0.0);
            if (ob) ob[r] = 0.0;
            if (oc) {
                double *v = oc + r * (int64_t)K * K;
                std::fill_n(v, (size_t)K * K, 0.0);
                for (int k = 0; k < K; ++k) v[(size_t)k * K + k] = a.eta2;
            }
        }
    }
    return PMF_OK;
}

extern "C" int pmf_gauss_fold_in(pmf_ctx *ctx, int side, int64_t n_rows, const int64_t *row_ptr, const int32_t *other_ids,
                                 const double *ratings, double sigma2, double eta2, double eta_bias2, int n_iter,
                                 double *out_factor, double *out_cov, double *out_bias) {
    return pmf_gauss_fold_in_weighted(ctx, side, n_rows, row_ptr, other_ids, ratings, nullptr, sigma2, eta2, eta_bias2, n_iter,
                                      out_factor, out_cov, out_bias);
}

extern "C" int pmf_gauss_fold_in_weighted(pmf_ctx *ctx, int side, int64_t n_rows, const int64_t *row_ptr,
                                          const int32_t *other_ids, const double *ratings, const double *weights, double sigma2,
                                          double eta2, double eta_bias2, int n_iter, double *out_factor, double *out_cov,
                                          double *out_bias) {
    PMF_SIDE_ENTRY("pmf_gauss_fold_in");
    PMF_REQUIRE(n_rows >= 0, PMF_EINVAL, "pmf_gauss_fold_in: negative row count");
    PMF_REQUIRE_ZERO_MODE_BIAS_FREE("pmf_gauss_fold_in");
    if (n_rows == 0) return PMF_OK;
    PMF_REQUIRE(row_ptr && out_factor, PMF_EINVAL, "pmf_gauss_fold_in: null argument");
    int rc;
    if ((rc = pmf_check_offsets("pmf_gauss_fold_in", "row_ptr", row_ptr, n_rows))) return rc;
    const int64_t nnz = row_ptr[n_rows];
    PMF_REQUIRE(nnz == 0 || (other_ids && ratings), PMF_EINVAL, "pmf_gauss_fold_in: null argument");
    PMF_REQUIRE(sigma2 > 0 && eta2 > 0 && eta_bias2 > 0, PMF_EINVAL, "pmf_gauss_fold_in: variances must be positive");
    PMF_REQUIRE(n_iter >= 1, PMF_EINVAL, "pmf_gauss_fold_in: n_iter = %d, must be at least 1", n_iter);
    const int other = 1 - side;
    if ((rc = gauss_require_state(ctx, other, false, "pmf_gauss_fold_in"))) return rc;
    if ((rc = pmf_check_ids(other_ids, nnz, ctx->rows[other], "pmf_gauss_fold_in", "id"))) return rc;
    if (weights && (rc = pmf_check_weights(weights, nnz, "pmf_gauss_fold_in"))) return rc;
    const FoldInBatch a = {n_rows, row_ptr, other_ids, ratings, weights, sigma2, eta2, eta_bias2, n_iter, out_factor, out_cov, out_bias};
    return pmf_no_throw("pmf_gauss_fold_in", [&] {
        return pmf_with_dtype(ctx, [&](auto t) { return run_fold_in<decltype(t)>(ctx, side, a); });
    });
}

// ---------------------------------------------------------------------------
// evidence lower bound (pmf_gauss_elbo_terms): the per-row sums that do not depend on the hyperparameters
// ---------------------------------------------------------------------------
// No reference counterpart.  Per row r of a side, with q(row) = N(m_r, V_r) and the user-side statistics the sweep
// builds (S_r, w_r over the row's ratings, residuals x_j - b_r - b_o):
//     SQNORM = |m_r|^2 + tr V_r      LOGDET = log det V_r      BIAS_SQ = BIAS[r]^2
//     ESS    = c_r - 2 m_r . w_r + <V_r + m_r m_r^T, S_r>,     c_r = sum_j (x_j - b_r - b_o)^2
// ESS is the expected squared residual of all of the row's ratings (bias variances aside: the host adds them).
// The rows go in the side's row windows (gauss_ensure_windows: statistics [rows x (cov_stride + kpad)] within a fixed
// budget): per window run the sweep's accumulate kernels (accumulate-only form) and the split-row combine on the window's
// tasks, then c_r and the row reduction.  The windows' task list is the Gaussian one again (same task length, so every row
// is cut and summed as in the sweep).  Sums inside a row are in the context dtype; the logarithms and everything across
// rows are double.

template <typename T>
struct ElboParams {
    int64_t row0, n;       // rows [row0, row0 + n) of the side
    const T *stats;        // the window: row row0 + i at stats + i * (cov_stride + kpad), packed S then w; null = no data term
    const T *csum;         // [n] c_r of the window's rows (with stats)
    const int64_t *ptr;    // the side's row offsets (with stats): a row without ratings has no statistics; null = every row of the window has (PMF_ZEROS_OBSERVED)
    const T *cov, *factor;
    const T *bias;         // null unless both sides have a BIAS array
    double *out;           // [rows of the side][PMF_ELBO_TERMS]
    int K, kpad, kp, cov_stride;
};

template <typename T>
struct ElboSqParams {
    const PmfTask *tasks;
    int64_t n_tasks;
    const int32_t *other;
    const T *val;
    const T *bias_self, *bias_other;   // null when the model has no biases
    T *partial;                        // [n_slots] of split rows
    T *csum;                           // row r of the window at csum[r - row0]
    int64_t row0;
    const T *wgt = nullptr;            // weighted ratings: c_j beside val, c_r = sum_j c_j e_j^2
};

// c_r: 16 lanes per task (a task is at most the context's task length), lane c takes ratings c, c + 16, ...
template <typename T>
__global__ __launch_bounds__(256) void gauss_elbo_sq_kernel(ElboSqParams<T> p) {
    constexpr int LPR = 16, G = 256 / LPR;
    const int c = threadIdx.x % LPR;
    const int64_t task_id = (int64_t)blockIdx.x * G + threadIdx.x / LPR;
    if (task_id >= p.n_tasks) return;
    const PmfTask t = p.tasks[task_id];
    const T bs = p.bias_self ? p.bias_self[t.row] : (T)0;
    const int32_t *col = p.other + t.start;
    const T *val = p.val + t.start;
    const T *wgt = p.wgt ? p.wgt + t.start : nullptr;
    T sum = (T)0;
    for (int j = c; j < t.len; j += LPR) {
        const T e = val[j] - bs - (p.bias_other ? p.bias_other[col[j]] : (T)0);
        sum = fma(wgt ? wgt[j] * e : e, e, sum);
    }
    sum = group_sum<LPR>(sum);
    if (c != 0) return;
    if (t.slot >= 0) p.partial[t.slot] = sum;
    else p.csum[(int64_t)t.row - p.row0] = sum;
}

// split rows: the slots of a row in slot order
template <typename T>
__global__ void gauss_elbo_sq_split_kernel(const PmfSplitRow *split, int64_t n_split, const T *partial, T *csum, int64_t row0) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_split) return;
    const PmfSplitRow sr = split[s];
    T sum = (T)0;
    for (int k = 0; k < sr.n_slots; ++k) sum += partial[sr.first_slot + k];
    csum[(int64_t)sr.row - row0] = sum;
}

// One 16-byte chunk (packed entries q .. q + 3, (r, c) = position of entry q) of the walk over a row's packed V and S:
// tr += V_rr,  acc[e] += w (V + m_r m_c) S  with w = 1 on the diagonal and 2 off it.
template <typename T>
__device__ __forceinline__ void elbo_walk_chunk(const Vec4<T> &v, const Vec4<T> &s, const T *ms, int q, int kp, int r, int c,
                                                T *acc, T &tr) {
#pragma unroll
    for (int e = 0; e < PMF_VEC; ++e) {
        if (q + e < kp) {
            const T t = fma(ms[r], ms[c], v.v[e]);
            if (r == c) {
                tr += v.v[e];
                acc[e] = fma(t, s.v[e], acc[e]);
            } else {
                acc[e] = fma(t + t, s.v[e], acc[e]);
            }
        }
        if (++c > r) {
            ++r;
            c = 0;
        }
    }
}

__device__ __forceinline__ double elbo_log_term(double piv, double g) {
    // log of a pivot of the scaled matrix, and the scale added back; a pivot that is not positive: not positive definite
    return (piv > 0.0 ? log(piv) : __builtin_nan("")) - 2.0 * log(g);
}

// The symmetric elimination (LDL^T without L) of the matrix held as B[i] = row k0 + i, lane j = column j, shared by the
// ELBO row pass (which keeps the pivots) and the posterior draws (which take the factor's columns along): before the
// rank-1 update of step k, `step(k, v, d)` sees the pivot row v and the pivot d = v_k.  The pivot row is always register 0:
// every update writes row i into register i - 1, as the solver's sweep does; after 8 steps (N / 2 below 16 rows) the live
// rows are registers 0 .. N - 9 and the same code runs at that width: 2 240 update instructions at 64 rows where a
// full-width sweep has 4 032 and the triangle 2 016.
template <typename T, int N, typename Step>
__device__ __forceinline__ void reg_eliminate(T *B, int k0, const Step &step) {
    constexpr int STEPS = N > 8 ? 8 : (N > 1 ? N / 2 : 1);
#pragma unroll 1
    for (int s = 0; s < STEPS; ++s) {
        const int k = k0 + s;
        const T v = B[0];
        const T d = readlane_dyn(v, k);
        step(k, v, d);
        if constexpr (N > 1) {
            const T u = v * ((T)1 / d);
#pragma unroll
            for (int i = 1; i < N; ++i) B[i - 1] = fma(-readlane_dyn(B[i], k), u, B[i]);
            B[N - 1] = (T)0;
        }
    }
    if constexpr (N > 1) reg_eliminate<T, N - STEPS>(B, k0 + STEPS, step);
}

// The same for a block per row (K > 64) on the packed lower triangle A, in LDS or global scratch: g[i] = 1 / sqrt(A_ii),
// A_ij *= g_i g_j, then the right-looking elimination, wavefront w taking rows k + 1 + w, k + 5 + w, ... of step k.
// Thread 0 runs `pivot(k, d)` at each step.  Begins with a barrier (A complete) and ends with one (A[i, k] = d_k L_ik).
template <typename T, typename Pivot>
__device__ __forceinline__ void block_scale_eliminate(T *A, T *g, int K, int kp, const Pivot &pivot) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    __syncthreads();
    for (int i = tid; i < K; i += 256) g[i] = (T)1 / sqrt(A[i * (i + 3) / 2]);
    __syncthreads();
    for (int e = tid; e < kp; e += 256) {
        int r, c;
        tri_rc(e, r, c);
        A[e] *= g[r] * g[c];
    }
    for (int k = 0; k < K; ++k) {
        __syncthreads();
        const T d = A[k * (k + 3) / 2];
        if (tid == 0) pivot(k, d);
        const T pinv = (T)1 / d;
        for (int i = k + 1 + wave; i < K; i += 4) {
            const T f = A[i * (i + 1) / 2 + k] * pinv;
            for (int jj = k + 1 + lane; jj <= i; jj += 64)
                A[i * (i + 1) / 2 + jj] = fma(-f, A[jj * (jj + 1) / 2 + k], A[i * (i + 1) / 2 + jj]);
        }
    }
    __syncthreads();
}

template <typename T>
__device__ __forceinline__ void elbo_store_terms(const ElboParams<T> &p, int64_t row, T sq, double ld, T ess, bool data) {
    double *o = p.out + row * PMF_ELBO_TERMS;
    const T b = p.bias ? p.bias[row] : (T)0;
    o[PMF_ELBO_SQNORM] = (double)sq;
    o[PMF_ELBO_LOGDET] = ld;
    o[PMF_ELBO_BIAS_SQ] = (double)(b * b);
    o[PMF_ELBO_ESS] = data ? (double)ess : 0.0;
}

// K <= 64: one wavefront per row, the matrix in registers
template <typename T, int KR>
__global__ __launch_bounds__(256) void gauss_elbo_row_reg_kernel(ElboParams<T> p) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t idx = (int64_t)blockIdx.x * 4 + wave;
    if (idx >= p.n) return;
    const int64_t row = p.row0 + idx;
    const int K = p.K, width = p.cov_stride + p.kpad;
    T *img = reinterpret_cast<T *>(smem_raw) + (int64_t)wave * width;
    T *ms = img + p.cov_stride;
    const T *V = p.cov + row * p.cov_stride;
    const T *m = p.factor + row * p.kpad;
    for (int k = lane; k < p.kpad; k += 64) ms[k] = m[k];
    wave_lds_fence();
    const bool data = p.stats != nullptr && (p.ptr == nullptr || p.ptr[row + 1] > p.ptr[row]);
    const T *S = p.stats ? p.stats + idx * width : nullptr;
    T acc[PMF_VEC] = {(T)0, (T)0, (T)0, (T)0}, tr = (T)0;
    for (int q = lane * PMF_VEC; q < p.cov_stride; q += 64 * PMF_VEC) {
        const Vec4<T> v = load4(V + q);
        const Vec4<T> s = data ? load4(S + q) : zero4<T>();
        store4(img + q, v);
        int r, c;
        tri_rc(q, r, c);
        elbo_walk_chunk(v, s, ms, q, p.kp, r, c, acc, tr);
    }
    T ess = (acc[0] + acc[1]) + (acc[2] + acc[3]), sq = tr;
    if (lane < K) {
        const T mk = ms[lane];
        sq = fma(mk, mk, sq);
        if (data) ess = fma((T)-2 * mk, S[p.cov_stride + lane], ess);
    }
    ess = group_sum<64>(ess);
    sq = group_sum<64>(sq);
    if (data) ess += p.csum[idx];
    wave_lds_fence();
    T B[KR];
    const T g = reg_load_scaled<T, KR>(img, K, lane, B);
    T piv = (T)1;
    const auto keep = [&](int k, T, T d) {   // lane k keeps pivot k
        if (lane == k) piv = d;
    };
    reg_eliminate<T, KR>(B, 0, keep);
    double ld = lane < K ? elbo_log_term((double)piv, (double)g) : 0.0;
    ld = group_sum<64>(ld);
    if (lane == 0) elbo_store_terms(p, row, sq, ld, ess, data);
}

// sum over the 256 threads of a block, the four wavefronts' sums added in order; every thread gets it
template <typename T>
__device__ __forceinline__ T elbo_block_sum(T x, T *red) {
    x = group_sum<64>(x);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// K > 64: one block per row on the packed lower triangle, in LDS or -- `scratch` != null: it does not fit the CU's 160 KB,
// fp64 at large K -- in the block's own slice of a global scratch buffer (RowMatrixPlan decides)
// dynamic LDS: [cov_stride unless `scratch`] + ms [kpad] + g [K] + pv [K]
template <typename T>
__global__ __launch_bounds__(256) void gauss_elbo_row_lds_kernel(ElboParams<T> p, T *scratch) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    __shared__ double red_d[4];
    __shared__ T red_t[4];
    const int K = p.K, kp = p.kp, width = p.cov_stride + p.kpad;
    T *lds = reinterpret_cast<T *>(smem_raw);
    T *A = scratch ? scratch + (int64_t)blockIdx.x * p.cov_stride : lds;   // packed lower triangle
    T *ms = scratch ? lds : lds + p.cov_stride;                            // [kpad] the row's mean
    T *g = ms + p.kpad;                                                    // [K] Jacobi scales
    T *pv = g + K;                                                         // [K] pivots
    const int tid = threadIdx.x;
    for (int64_t idx = blockIdx.x; idx < p.n; idx += gridDim.x) {
        const int64_t row = p.row0 + idx;
        const T *V = p.cov + row * p.cov_stride;
        const T *m = p.factor + row * p.kpad;
        __syncthreads();
        for (int k = tid; k < p.kpad; k += 256) ms[k] = m[k];
        __syncthreads();
        const bool data = p.stats != nullptr && (p.ptr == nullptr || p.ptr[row + 1] > p.ptr[row]);
        const T *S = p.stats ? p.stats + idx * width : nullptr;
        T acc[PMF_VEC] = {(T)0, (T)0, (T)0, (T)0}, tr = (T)0;
        for (int q = tid * PMF_VEC; q < p.cov_stride; q += 256 * PMF_VEC) {
            const Vec4<T> v = load4(V + q);
            const Vec4<T> s = data ? load4(S + q) : zero4<T>();
            store4(A + q, v);
            int r, c;
            tri_rc(q, r, c);
            elbo_walk_chunk(v, s, ms, q, kp, r, c, acc, tr);
        }
        T ess = (acc[0] + acc[1]) + (acc[2] + acc[3]), sq = tr;
        for (int k = tid; k < K; k += 256) {
            const T mk = ms[k];
            sq = fma(mk, mk, sq);
            if (data) ess = fma((T)-2 * mk, S[p.cov_stride + k], ess);
        }
        ess = elbo_block_sum(ess, red_t);
        sq = elbo_block_sum(sq, red_t);
        if (data) ess += p.csum[idx];
        block_scale_eliminate(A, g, K, kp, [&](int k, T d) { pv[k] = d; });
        double ld = 0.0;
        for (int k = tid; k < K; k += 256) ld += elbo_log_term((double)pv[k], (double)g[k]);
        ld = elbo_block_sum(ld, red_d);
        if (tid == 0) elbo_store_terms(p, row, sq, ld, ess, data);
    }
}

template <typename T>
static int launch_elbo_rows(pmf_ctx *ctx, const ElboParams<T> &e) {
    int rc = PMF_OK;
    if (e.n == 0) return PMF_OK;
    const int K = ctx->K;
    if (K <= 64) {
        const size_t smem = (size_t)4 * (ctx->cov_stride + ctx->kpad) * sizeof(T);
        pmf_with_pow2<8>(K, [&](auto KR) {
            rc = pmf_allow_dynamic_lds((const void *)gauss_elbo_row_reg_kernel<T, KR>, smem);   // fp64 at K = 64: 67 KB
            if (rc == PMF_OK)
                hipLaunchKernelGGL((gauss_elbo_row_reg_kernel<T, KR>), dim3((unsigned)((e.n + 3) / 4)), dim3(256), smem,
                                   ctx->stream, e);
        });
        if (rc) return rc;
    } else {
        const RowMatrixPlan plan((size_t)ctx->cov_stride * sizeof(T), (size_t)(ctx->kpad + 2 * K) * sizeof(T), 64, 1024);
        T *scratch = nullptr;
        if (!plan.in_lds) {   // one packed triangle per resident block (<= 1024 x 263 KB)
            if ((rc = pmf_ensure_scratch(ctx, plan.scratch_bytes(e.n)))) return rc;
            scratch = ctx->d_scratch.as<T>();
        }
        if ((rc = pmf_allow_dynamic_lds((const void *)gauss_elbo_row_lds_kernel<T>, plan.smem()))) return rc;
        hipLaunchKernelGGL((gauss_elbo_row_lds_kernel<T>), dim3(plan.blocks(e.n)), dim3(256), plan.smem(), ctx->stream, e, scratch);
    }
    PMF_HIP_CHECK(hipGetLastError());
    return PMF_OK;
}

template <typename T>
static int run_elbo_terms(pmf_ctx *ctx, int side, bool with_data, double *totals, double *per_row) {
    const int64_t rows = ctx->rows[side];
    const int cs = ctx->cov_stride, kpad = ctx->kpad, width = cs + kpad;
    const bool bias = pmf_has_bias(ctx);
    PmfSideIndex &ix = ctx->index[side];
    PmfBuf d_out, d_win, d_c, d_cpart;
    int rc;
    if ((rc = d_out.alloc(ctx, (size_t)rows * PMF_ELBO_TERMS * sizeof(double)))) return rc;
    ElboParams<T> e;
    e.stats = nullptr;
    e.csum = nullptr;
    e.ptr = nullptr;
    e.cov = ctx->arr[side][PMF_ARR_COV].as<const T>();
    e.factor = ctx->arr[side][PMF_ARR_FACTOR].as<const T>();
    e.bias = bias ? ctx->arr[side][PMF_ARR_BIAS].as<const T>() : nullptr;
    e.out = d_out.as<double>();
    e.K = ctx->K;
    e.kpad = kpad;
    e.kp = ctx->kp;
    e.cov_stride = cs;
    if (!with_data) {
        e.row0 = 0;
        e.n = rows;
        PmfProfScope prof(ctx, PMF_KERNEL_GAUSS_SOLVE);
        if ((rc = launch_elbo_rows<T>(ctx, e))) return rc;
    } else {
        const PmfRowWindows &rw = ix.windows;
        int64_t win_rows;
        if ((rc = gauss_ensure_windows<T>(ctx, side, &win_rows))) return rc;
        if ((rc = d_cpart.alloc(ctx, (size_t)rw.tasks.n_slots * sizeof(T)))) return rc;
        if ((rc = d_win.alloc(ctx, (size_t)win_rows * width * sizeof(T)))) return rc;
        if ((rc = d_c.alloc(ctx, (size_t)win_rows * sizeof(T)))) return rc;
        // unlisted cells as weighted zeros (gw is set): S of EVERY row is blended with w0 G of the other side, so every
        // row has statistics (e.ptr stays null) and the rows no task writes start from zero sums and c_r = 0
        const T *gw;
        if ((rc = gauss_zero_gram<T>(ctx, side, &gw))) return rc;
        GaussParamsW<T> p = gauss_params<T>(ctx, side);
        e.stats = d_win.as<const T>();
        e.csum = d_c.as<const T>();
        e.ptr = gw ? nullptr : ix.d_ptr.as<const int64_t>();
        for (size_t w = 0; w + 1 < rw.bounds.size(); ++w) {
            const int64_t r0 = rw.bounds[w], n = rw.bounds[w + 1] - r0, ns = gauss_window_tasks<T>(rw, w, p), nt = p.n_tasks;
            const bool zero_first = gw && rw.has_empty[w];
            if (zero_first) PMF_HIP_CHECK(hipMemsetAsync(d_c.as(), 0, (size_t)n * sizeof(T), ctx->stream));
            if ((rc = gauss_block_stats<T>(ctx, p, ns, GaussStats<T>::interleaved(ctx, d_win.as<T>(), r0), n, zero_first, gw))) return rc;
            PmfProfScope prof(ctx, PMF_KERNEL_GAUSS_SOLVE);
            if (nt > 0) {
                ElboSqParams<T> q;
                q.tasks = p.tasks;
                q.n_tasks = nt;
                q.other = p.other;
                q.val = p.val;
                q.bias_self = p.bias_self;
                q.bias_other = p.bias_other;
                q.partial = d_cpart.as<T>();
                q.csum = d_c.as<T>();
                q.row0 = r0;
                q.wgt = p.wgt;
                hipLaunchKernelGGL((gauss_elbo_sq_kernel<T>), dim3((unsigned)((nt + 15) / 16)), dim3(256), 0, ctx->stream, q);
            }
            if (ns > 0)
                hipLaunchKernelGGL((gauss_elbo_sq_split_kernel<T>), dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, ctx->stream,
                                   p.split, ns, d_cpart.as<const T>(), d_c.as<T>(), r0);
            PMF_HIP_CHECK(hipGetLastError());
            e.row0 = r0;
            e.n = n;
            if ((rc = launch_elbo_rows<T>(ctx, e))) return rc;
        }
    }
    // per-row terms to the host; the totals are their sums in row order, whatever the windows were
    std::vector<double> host;
    double *dst = per_row;
    if (!dst) {
        host.resize((size_t)rows * PMF_ELBO_TERMS);
        dst = host.data();
    }
    PMF_HIP_CHECK(hipMemcpyAsync(dst, d_out.as(), (size_t)rows * PMF_ELBO_TERMS * sizeof(double), hipMemcpyDeviceToHost,
                                 ctx->stream));
    PMF_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    double sum[PMF_ELBO_TERMS] = {};
    for (int64_t r = 0; r < rows; ++r)
        for (int t = 0; t < PMF_ELBO_TERMS; ++t) sum[t] += dst[r * PMF_ELBO_TERMS + t];
    std::copy_n(sum, PMF_ELBO_TERMS, totals);
    return PMF_OK;
}

extern "C" int pmf_gauss_elbo_terms(pmf_ctx *ctx, int side, int with_data, double *totals, double *per_row) {
    PMF_SIDE_ENTRY("pmf_gauss_elbo_terms");
    PMF_REQUIRE(totals, PMF_EINVAL, "pmf_gauss_elbo_terms: null totals");
    int rc;
    if ((rc = gauss_require_state(ctx, side, false, "pmf_gauss_elbo_terms"))) return rc;
    if (with_data) {
        PMF_REQUIRE_ZERO_MODE_BIAS_FREE("pmf_gauss_elbo_terms");
        if ((rc = gauss_require_state(ctx, 1 - side, false, "pmf_gauss_elbo_terms"))) return rc;
        PMF_REQUIRE(ctx->index[side].d_ptr, PMF_EINVAL, "pmf_gauss_elbo_terms: ratings have not been set");
    }
    return pmf_no_throw("pmf_gauss_elbo_terms", [&] {
        return pmf_with_dtype(ctx, [&](auto t) { return run_elbo_terms<decltype(t)>(ctx, side, with_data != 0, totals, per_row); });
    });
}

// ---------------------------------------------------------------------------
// posterior draws (pmf_gauss_sample_rows, and the tables of pmf_topk_sampled)
// ---------------------------------------------------------------------------
// No reference counterpart.  A draw of row r is x = m_r + C_r z with C_r the lower Cholesky factor of V_r and z K standard
// normals.  C_r is never stored: the elimination the ELBO row kernels run on the Jacobi-scaled matrix A = G V G (G =
// diag(g), g_j = 1 / sqrt(V_jj)) has, at step k, d_k L[:, k] in the pivot row (A = L D L^T), so column k of chol(A) is that
// row times 1 / sqrt(d_k), and  x = m + G^-1 chol(A) z  is accumulated column by column.  The normals are a pure function
// of (seed, side, row id, draw index, k): Philox4x32-10 on the counter (row id, draw index, k / 4, side) under the key
// (seed low, seed high), then Box-Muller in double on the words (0, 1) and (2, 3), rounded once to the context dtype.
// A row with a pivot that is not positive (or a NaN scale) gives NaN in all its elements, as PMF_ELBO_LOGDET does.

static const int kSampleDraws = 8;   // draws per pass of the elimination (register kernel) / of the mat-vec (block kernel)

template <typename T>
struct SampleParams {
    const int32_t *ids;    // device [n]: the row of request q, or null: request q is row q
    int64_t n;
    const T *cov, *factor;
    const T *z;            // device [n x n_draws x kpad]: the normals in place of the stream, or null
    T *out;                // [n x n_draws x kpad]
    int K, kpad, kp, cov_stride;
    int side, n_draws;
    uint32_t draw0, key0, key1;
};

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t (&w)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0;
        c1 = (uint32_t)p1;
        c2 = n2;
        c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    w[0] = c0;
    w[1] = c1;
    w[2] = c2;
    w[3] = c3;
}

// z_k of (side, row, draw): words 2h, 2h + 1 of block k / 4 with h = (k / 2) % 2; even k takes the cosine, odd k the sine
template <typename T>
__device__ __forceinline__ T sample_normal(const SampleParams<T> &p, uint32_t row, uint32_t draw, int k) {
    uint32_t w[4];
    philox4x32_10(row, draw, (uint32_t)k >> 2, (uint32_t)p.side, p.key0, p.key1, w);
    const bool hi = (k & 2) != 0;
    const double u0 = ((double)(hi ? w[2] : w[0]) + 0.5) * 0x1p-32, u1 = ((double)(hi ? w[3] : w[1]) + 0.5) * 0x1p-32;
    const double r = sqrt(-2.0 * log(u0));
    double sn, cs;
    sincos(6.283185307179586 * u1, &sn, &cs);
    return (T)(r * ((k & 1) ? sn : cs));
}

// K <= 64: one wavefront per (request, pass of DR draws), the matrix in registers; DR draws ride on one elimination
// (reg_eliminate), and a request of more draws takes ceil(n_draws / DR)
// wavefronts, each with an elimination of its own (`passes` per request; wavefront w: request w / passes, pass w % passes).
// dynamic LDS: 4 waves x (cov_stride + DR x 64) elements
template <typename T, int KR, int DR>
__global__ __launch_bounds__(256) void gauss_sample_reg_kernel(SampleParams<T> p, int passes) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + wave;
    const int64_t idx = w / passes;
    if (idx >= p.n) return;
    const int d0 = (int)(w - idx * passes) * DR;
    const int64_t row = p.ids ? (int64_t)p.ids[idx] : idx;
    const int K = p.K;
    T *img = reinterpret_cast<T *>(smem_raw) + (int64_t)wave * (p.cov_stride + DR * 64);
    T *zs = img + p.cov_stride;   // [DR][64] the pass's normals, staged so that the generator is inlined once
    const T *V = p.cov + row * p.cov_stride;
    for (int q = lane * PMF_VEC; q < p.cov_stride; q += 64 * PMF_VEC) store4(img + q, load4(V + q));
    const int j = lane;
    const T mj = j < K ? p.factor[row * p.kpad + j] : (T)0;
    const int64_t at = idx * p.n_draws * p.kpad;
#pragma unroll 1
    for (int dd = 0; dd < DR; ++dd) {
        const int d = d0 + dd;
        T z = (T)0;   // (lanes >= K: their columns of the identity padding add nothing)
        if (j < K && d < p.n_draws)
            z = p.z ? p.z[at + (int64_t)d * p.kpad + j] : sample_normal<T>(p, (uint32_t)row, p.draw0 + (uint32_t)d, j);
        zs[dd * 64 + lane] = z;
    }
    wave_lds_fence();
    T zr[DR], acc[DR];
#pragma unroll
    for (int dd = 0; dd < DR; ++dd) {
        zr[dd] = zs[dd * 64 + lane];
        acc[dd] = (T)0;
    }
    T B[KR];
    const T g = reg_load_scaled<T, KR>(img, K, lane, B);
    bool ok = true;
    // at step k the pivot row times 1 / sqrt(d_k) is column k of the factor on lanes j >= k -- lanes j < k hold the rounding
    // residue of d (1 / d) - 1, not zeros, and are masked -- and draw d adds it times z_{d,k}, which lane k holds
    const auto column = [&](int k, T v, T d) {
        if (k < K && !(d > (T)0)) ok = false;
        const T c = lane >= k ? v * ((T)1 / sqrt(d)) : (T)0;
#pragma unroll
        for (int dd = 0; dd < DR; ++dd) acc[dd] = fma(c, readlane_dyn(zr[dd], k), acc[dd]);
    };
    reg_eliminate<T, KR>(B, 0, column);
    if (j < p.kpad) {
#pragma unroll
        for (int dd = 0; dd < DR; ++dd)
            if (d0 + dd < p.n_draws)
                p.out[at + (int64_t)(d0 + dd) * p.kpad + j] = j < K ? (ok ? mj + acc[dd] / g : (T)__builtin_nan("")) : (T)0;
    }
}

// K > 64: one block per request on the packed lower triangle, in LDS or (`scratch` != null) in the block's slice of a
// global buffer.  After block_scale_eliminate A[i, k] (i > k)
// holds d_k L_ik and the pivots d_k; column k times 1 / sqrt(d_k) makes the triangle chol(A) in place, and the draws are
// the packed mat-vec  x_i = m_i + (1 / g_i) sum_{k <= i} A[i, k] z_k:  wavefront w takes rows w, w + 4, ..., lane l the
// columns l, l + 64, ..., then the lanes' sums in group_sum's fixed order.
// dynamic LDS: [cov_stride unless `scratch`] + g [K] + rs [K] + z [kSampleDraws][K]
template <typename T>
__global__ __launch_bounds__(256) void gauss_sample_lds_kernel(SampleParams<T> p, T *scratch) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    __shared__ int bad;
    constexpr int DC = kSampleDraws;
    const int K = p.K, kp = p.kp;
    T *lds = reinterpret_cast<T *>(smem_raw);
    T *A = scratch ? scratch + (int64_t)blockIdx.x * p.cov_stride : lds;   // packed lower triangle
    T *g = scratch ? lds : lds + p.cov_stride;                             // [K] Jacobi scales
    T *rs = g + K;                                                         // [K] 1 / sqrt(pivot)
    T *zs = rs + K;                                                        // [DC][K] the pass's normals
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int64_t idx = blockIdx.x; idx < p.n; idx += gridDim.x) {
        const int64_t row = p.ids ? (int64_t)p.ids[idx] : idx;
        const T *V = p.cov + row * p.cov_stride;
        const T *m = p.factor + row * p.kpad;
        const int64_t at = idx * p.n_draws * p.kpad;
        __syncthreads();
        if (tid == 0) bad = 0;
        for (int q = tid * PMF_VEC; q < p.cov_stride; q += 256 * PMF_VEC) store4(A + q, load4(V + q));
        block_scale_eliminate(A, g, K, kp, [&](int k, T d) {
            if (!(d > (T)0)) bad = 1;
            rs[k] = (T)1 / sqrt(d);
        });
        for (int e = tid; e < kp; e += 256) {
            int r, c;
            tri_rc(e, r, c);
            A[e] *= rs[c];
        }
        const bool ok = bad == 0;
        for (int d0 = 0; d0 < p.n_draws; d0 += DC) {
            __syncthreads();
            for (int e = tid; e < DC * K; e += 256) {
                const int dd = e / K, k = e - dd * K, d = d0 + dd;
                T z = (T)0;
                if (d < p.n_draws)
                    z = p.z ? p.z[at + (int64_t)d * p.kpad + k] : sample_normal<T>(p, (uint32_t)row, p.draw0 + (uint32_t)d, k);
                zs[e] = z;
            }
            __syncthreads();
            for (int i = wave; i < p.kpad; i += 4) {
                T s[DC];
#pragma unroll
                for (int dd = 0; dd < DC; ++dd) s[dd] = (T)0;
                if (i < K)
                    for (int k = lane; k <= i; k += 64) {
                        const T a = A[i * (i + 1) / 2 + k];
#pragma unroll
                        for (int dd = 0; dd < DC; ++dd) s[dd] = fma(a, zs[dd * K + k], s[dd]);
                    }
#pragma unroll
                for (int dd = 0; dd < DC; ++dd) {
                    const T sum = group_sum<64>(s[dd]);
                    if (lane == 0 && d0 + dd < p.n_draws)
                        p.out[at + (int64_t)(d0 + dd) * p.kpad + i] = i < K ? (ok ? m[i] + sum / g[i] : (T)__builtin_nan("")) : (T)0;
                }
            }
        }
    }
}

// the block-per-row kernel's placement: the caller of the launch provides the scratch (pmf_gauss_sample_tri_bytes)
template <typename T>
static RowMatrixPlan sample_plan(const pmf_ctx *ctx) {
    return RowMatrixPlan((size_t)ctx->cov_stride * sizeof(T), (size_t)(2 + kSampleDraws) * ctx->K * sizeof(T), 64, 1024);
}

size_t pmf_gauss_sample_tri_bytes(const pmf_ctx *ctx, int64_t n) {
    if (ctx->K <= 64 || n <= 0) return 0;
    return pmf_with_dtype(ctx, [&](auto t) { return sample_plan<decltype(t)>(ctx).scratch_bytes(n); });
}

template <typename T>
static int launch_sample(pmf_ctx *ctx, const SampleParams<T> &s, T *tri) {
    int rc = PMF_OK;
    if (s.n == 0) return PMF_OK;
    const int K = ctx->K;
    PmfProfScope prof(ctx, PMF_KERNEL_GAUSS_SOLVE);
    if (K <= 64) {
        const int many = s.n_draws > 1, dr = many ? kSampleDraws : 1, passes = (s.n_draws + dr - 1) / dr;
        const size_t smem = (size_t)4 * (ctx->cov_stride + dr * 64) * sizeof(T);
        const int64_t blocks = (s.n * passes + 3) / 4;
        PMF_REQUIRE(blocks <= (int64_t)INT32_MAX, PMF_ERANGE, "gauss sample: %lld rows x %d draws in one launch", (long long)s.n, s.n_draws);
        const dim3 grid((unsigned)blocks);
        pmf_with_pow2<8>(K, [&](auto KR) {
            auto go = [&](auto kernel) {
                rc = pmf_allow_dynamic_lds((const void *)kernel, smem);   // fp64 at K = 64
                if (rc == PMF_OK) hipLaunchKernelGGL(kernel, grid, dim3(256), smem, ctx->stream, s, passes);
            };
            if (many) go(gauss_sample_reg_kernel<T, KR, kSampleDraws>);
            else go(gauss_sample_reg_kernel<T, KR, 1>);
        });
        if (rc) return rc;
    } else {
        const RowMatrixPlan plan = sample_plan<T>(ctx);
        PMF_REQUIRE(plan.in_lds || tri, PMF_EINVAL, "gauss sample: no buffer for the packed triangles");
        if ((rc = pmf_allow_dynamic_lds((const void *)gauss_sample_lds_kernel<T>, plan.smem()))) return rc;
        hipLaunchKernelGGL((gauss_sample_lds_kernel<T>), dim3(plan.blocks(s.n)), dim3(256), plan.smem(), ctx->stream, s,
                           plan.in_lds ? (T *)nullptr : tri);
    }
    PMF_HIP_CHECK(hipGetLastError());
    return PMF_OK;
}

int pmf_gauss_sample_launch(pmf_ctx *ctx, int side, const int32_t *d_ids, int64_t n, int n_draws, int draw0, uint64_t seed,
                            const void *d_z, void *d_out, void *d_tri) {
    return pmf_with_dtype(ctx, [&](auto t) {
        using T = decltype(t);
        SampleParams<T> s;
        s.ids = d_ids;
        s.n = n;
        s.cov = ctx->arr[side][PMF_ARR_COV].as<const T>();
        s.factor = ctx->arr[side][PMF_ARR_FACTOR].as<const T>();
        s.z = static_cast<const T *>(d_z);
        s.out = static_cast<T *>(d_out);
        s.K = ctx->K;
        s.kpad = ctx->kpad;
        s.kp = ctx->kp;
        s.cov_stride = ctx->cov_stride;
        s.side = side;
        s.n_draws = n_draws;
        s.draw0 = (uint32_t)draw0;
        s.key0 = (uint32_t)(seed & 0xFFFFFFFFull);
        s.key1 = (uint32_t)(seed >> 32);
        return launch_sample<T>(ctx, s, static_cast<T *>(d_tri));
    });
}

// The rounds of pmf_gauss_sample_rows: per round (pmf_sample_round_rows of the staging budget) the ids and, if given, the
// normals go up through pinned memory, the kernel fills the round's table and the table comes down as FACTOR-shaped rows.
template <typename T>
static int run_sample_rows(pmf_ctx *ctx, int side, int64_t n_rows, const int32_t *row_ids, int n_draws, int draw0, uint64_t seed,
                           const double *z, double *out) {
    const int K = ctx->K, kpad = ctx->kpad;
    const int64_t R = pmf_sample_round_rows(n_rows, n_draws, kpad, sizeof(T), z != nullptr, ctx->stage_bytes);
    const size_t tri_bytes = pmf_gauss_sample_tri_bytes(ctx, R);
    PmfLayout lay;
    const auto out_at = lay.add<T>((size_t)R * n_draws * kpad), z_at = lay.add<T>(z ? (size_t)R * n_draws * kpad : 0);
    const auto ids_at = lay.add<int32_t>((size_t)R);
    const auto tri_at = lay.add<unsigned char>(tri_bytes);
    int rc;
    if ((rc = pmf_ensure_scratch(ctx, lay.bytes()))) return rc;
    void *base = ctx->d_scratch.as();
    for (int64_t r0 = 0; r0 < n_rows; r0 += R) {
        const int64_t nr = std::min(R, n_rows - r0), vecs = nr * n_draws;
        PMF_HIP_CHECK(hipMemcpyAsync(ids_at.at(base), row_ids + r0, (size_t)nr * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        if (z) {   // the conversion of pmf_set_array_rows: rounded to T, zero-padded to Kpad
            if ((rc = pmf_ensure_pinned(ctx, (size_t)vecs * kpad * sizeof(T)))) return rc;
            T *pin = ctx->h_pinned.as<T>();
            for (int64_t v = 0; v < vecs; ++v) {
                const double *src = z + (r0 * n_draws + v) * K;
                T *dst = pin + v * kpad;
                for (int k = 0; k < K; ++k) dst[k] = (T)src[k];
                for (int k = K; k < kpad; ++k) dst[k] = (T)0;
            }
            PMF_HIP_CHECK(hipMemcpyAsync(z_at.at(base), pin, (size_t)vecs * kpad * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
        }
        if ((rc = pmf_gauss_sample_launch(ctx, side, ids_at.at(base), nr, n_draws, draw0, seed, z ? z_at.at(base) : nullptr,
                                          out_at.at(base), tri_bytes ? tri_at.at(base) : nullptr)))
            return rc;
        if ((rc = pmf_fold_in_download(ctx, PMF_ARR_FACTOR, out_at.at(base), out + r0 * n_draws * K, vecs))) return rc;
    }
    return PMF_OK;
}

extern "C" int pmf_gauss_sample_rows(pmf_ctx *ctx, int side, int64_t n_rows, const int32_t *row_ids, int n_draws, int draw0,
                                     uint64_t seed, const double *z, double *out) {
    const char *fn = "pmf_gauss_sample_rows";
    PMF_SIDE_ENTRY("pmf_gauss_sample_rows");
    int rc;
    if ((rc = pmf_sample_check(fn, n_rows, row_ids, n_draws, draw0, out, ctx->rows[side]))) return rc;
    if (n_rows == 0) return PMF_OK;
    if ((rc = gauss_require_state(ctx, side, false, fn))) return rc;
    return pmf_no_throw(fn, [&] {
        return pmf_with_dtype(ctx, [&](auto t) {
            return run_sample_rows<decltype(t)>(ctx, side, n_rows, row_ids, n_draws, draw0, seed, z, out);
        });
    });
}
