// Device-side build of the two rating orders (CSR by user, CSC by item).
//
// Replaces `_build_index_lists` (hpf_cavi.py:97-107, poisson_mf_cavi.py:73-84,
// gaussian_mf_cavi_bias.py:69-86): the reference appends every rating to the list
// of its user and of its item in input order.  Here the (user, item, rating)
// triples are uploaded once and, per side, a STABLE radix sort of the positions
// by row id (rocPRIM, least-significant-digit passes) gives the same within-row
// order; the opposite-side ids and the ratings are then gathered into row order
// and the row pointers are found by binary search in the sorted keys.
#include <cstring>

#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include <limits.h>

#include "pmf_internal.h"

namespace {

constexpr unsigned long long NO_BAD = ~0ull;

__global__ void check_ids_kernel(const int32_t *u, const int32_t *i, int64_t nnz, int64_t U, int64_t I,
                                 unsigned long long *first_bad) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= nnz) return;
    const int32_t a = u[n], b = i[n];
    if (a < 0 || a >= U || b < 0 || b >= I) atomicMin(first_bad, (unsigned long long)n);
}

__global__ void iota_kernel(uint32_t *p, int64_t n) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) p[k] = (uint32_t)k;
}

// w_in (with w_out) may be null: the ratings' weights go through the same permutation
template <typename T>
__global__ void gather_kernel(const uint32_t *perm, const int32_t *other_in, const double *x_in, const double *w_in,
                              int32_t *other_out, T *val_out, T *w_out, int64_t n) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t src = perm[k];
    other_out[k] = other_in[src];
    val_out[k] = (T)x_in[src];
    if (w_in) w_out[k] = (T)w_in[src];
}

// C_r of every row: its weights (in double, input order gathered by `perm`) added in the row's rating order
template <typename T>
__global__ void weight_sum_kernel(const uint32_t *perm, const double *w_in, const int64_t *ptr, int64_t rows, double *sum_out,
                                  T *sum_out_t) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    double c = 0.0;
    for (int64_t k = ptr[r]; k < ptr[r + 1]; ++k) c += w_in[perm[k]];
    sum_out[r] = c;
    sum_out_t[r] = (T)c;
}

// ptr[r] = number of ratings whose row id is < r (r = 0 .. rows)
__global__ void row_ptr_kernel(const uint32_t *sorted_keys, int64_t nnz, int64_t rows, int64_t *ptr) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > rows) return;
    int64_t lo = 0, hi = nnz;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)sorted_keys[mid] < r) lo = mid + 1;
        else hi = mid;
    }
    ptr[r] = lo;
}

inline unsigned grid_for(int64_t n) { return (unsigned)((n + 255) / 256); }

inline unsigned key_bits(int64_t rows) {  // row ids are < rows
    unsigned bits = 1;
    while (bits < 32 && ((int64_t)1 << bits) < rows) ++bits;
    return bits;
}

}  // namespace

// Two-phase interface used by pmf_ctx_set_ratings (pmf_ctx.hip):
//   pmf_index_device_begin  uploads and validates (context untouched on failure),
//   pmf_index_device_finish fills index[side].{d_ptr, d_other, d_val, h_ptr} (already allocated).
// The temporaries of one build belong to no context (not in device_bytes) and go with the struct on every exit path.
struct PmfIndexBuild {
    PmfBuf d_u, d_i;   // int32_t [nnz], input order
    PmfBuf d_x;        // double [nnz]
    PmfBuf d_w;        // double [nnz] the weights; null without
};

// Upload + validate.  On success the device copies live in `b` and *bad < 0; a bad id gives its
// position in *bad (no device state of the context has been touched yet).
static int upload_and_check(pmf_ctx *ctx, PmfIndexBuild &b, int64_t nnz, const int32_t *user_ids, const int32_t *item_ids,
                            const double *ratings, const double *weights, int64_t *bad) {
    *bad = -1;
    int rc;
    PmfBuf d_bad;
    if ((rc = b.d_u.alloc(nullptr, (size_t)nnz * sizeof(int32_t)))) return rc;
    if ((rc = b.d_i.alloc(nullptr, (size_t)nnz * sizeof(int32_t)))) return rc;
    if ((rc = b.d_x.alloc(nullptr, (size_t)nnz * sizeof(double)))) return rc;
    if (weights && (rc = b.d_w.alloc(nullptr, (size_t)nnz * sizeof(double)))) return rc;
    if ((rc = d_bad.alloc(nullptr, sizeof(unsigned long long)))) return rc;
    if (nnz == 0) return PMF_OK;
    PMF_HIP_CHECK(hipMemcpyAsync(b.d_u.as(), user_ids, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    PMF_HIP_CHECK(hipMemcpyAsync(b.d_i.as(), item_ids, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    PMF_HIP_CHECK(hipMemcpyAsync(b.d_x.as(), ratings, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (weights)
        PMF_HIP_CHECK(hipMemcpyAsync(b.d_w.as(), weights, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    PMF_HIP_CHECK(hipMemsetAsync(d_bad.as(), 0xff, sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(check_ids_kernel, dim3(grid_for(nnz)), dim3(256), 0, ctx->stream, b.d_u.as<int32_t>(),
                       b.d_i.as<int32_t>(), nnz, ctx->rows[0], ctx->rows[1], d_bad.as<unsigned long long>());
    PMF_HIP_CHECK(hipGetLastError());
    unsigned long long h_bad = NO_BAD;
    PMF_HIP_CHECK(hipMemcpyAsync(&h_bad, d_bad.as(), sizeof(h_bad), hipMemcpyDeviceToHost, ctx->stream));
    PMF_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (h_bad != NO_BAD) *bad = (int64_t)h_bad;
    return PMF_OK;
}

template <typename T>
static int order_side(pmf_ctx *ctx, int side, int64_t nnz, const int32_t *d_key, const int32_t *d_oth,
                      const double *d_x, const double *d_w, uint32_t *d_keys_out, uint32_t *d_pos_in, uint32_t *d_pos_out, void *d_tmp,
                      size_t tmp_bytes) {
    PmfSideIndex &ix = ctx->index[side];
    const int64_t rows = ctx->rows[side];
    if (nnz > 0) {
        const unsigned bits = key_bits(rows);
        hipLaunchKernelGGL(iota_kernel, dim3(grid_for(nnz)), dim3(256), 0, ctx->stream, d_pos_in, nnz);
        size_t bytes = tmp_bytes;
        PMF_HIP_CHECK(rocprim::radix_sort_pairs(d_tmp, bytes, (const uint32_t *)d_key, d_keys_out, (const uint32_t *)d_pos_in,
                                                d_pos_out, (size_t)nnz, 0u, bits, ctx->stream));
        hipLaunchKernelGGL((gather_kernel<T>), dim3(grid_for(nnz)), dim3(256), 0, ctx->stream, d_pos_out, d_oth, d_x,
                           d_w, ix.d_other.as<int32_t>(), ix.d_val.as<T>(), ix.d_wgt.as<T>(), nnz);
    }
    hipLaunchKernelGGL(row_ptr_kernel, dim3(grid_for(rows + 1)), dim3(256), 0, ctx->stream, d_keys_out, nnz, rows,
                       ix.d_ptr.as<int64_t>());
    PMF_HIP_CHECK(hipGetLastError());
    ix.h_ptr.resize((size_t)rows + 1);
    PMF_HIP_CHECK(hipMemcpyAsync(ix.h_ptr.data(), ix.d_ptr.as(), (size_t)(rows + 1) * sizeof(int64_t), hipMemcpyDeviceToHost,
                                 ctx->stream));
    if (d_w) {   // (the double sums share the keys' successor on the stream: a buffer of this call)
        PmfBuf d_sum;
        int rc;
        if ((rc = d_sum.alloc(nullptr, (size_t)rows * sizeof(double)))) return rc;
        ix.h_wsum.assign((size_t)rows, 0.0);
        if (rows > 0) {
            hipLaunchKernelGGL((weight_sum_kernel<T>), dim3(grid_for(rows)), dim3(256), 0, ctx->stream, d_pos_out, d_w,
                               ix.d_ptr.as<int64_t>(), rows, d_sum.as<double>(), ix.d_wsum.as<T>());
            PMF_HIP_CHECK(hipGetLastError());
            PMF_HIP_CHECK(hipMemcpyAsync(ix.h_wsum.data(), d_sum.as(), (size_t)rows * sizeof(double), hipMemcpyDeviceToHost,
                                         ctx->stream));
        }
        PMF_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        return PMF_OK;
    }
    PMF_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return PMF_OK;
}

int pmf_index_device_begin(pmf_ctx *ctx, int64_t nnz, const int32_t *user_ids, const int32_t *item_ids,
                           const double *ratings, const double *weights, PmfIndexBuild **out, int64_t *bad_position) {
    PmfIndexBuild *b = new PmfIndexBuild();
    int rc = upload_and_check(ctx, *b, nnz, user_ids, item_ids, ratings, weights, bad_position);
    if (rc != PMF_OK || *bad_position >= 0) {
        delete b;
        b = nullptr;
    }
    *out = b;
    return rc;
}

void pmf_index_device_abort(PmfIndexBuild *b) { delete b; }

int pmf_index_device_finish(pmf_ctx *ctx, PmfIndexBuild *b, int64_t nnz) {
    struct Guard {
        PmfIndexBuild *b;
        ~Guard() { delete b; }
    } guard{b};
    PmfBuf d_keys_out, d_pos_in, d_pos_out, d_tmp;
    size_t tmp_bytes = 0;
    int rc;
    if ((rc = d_keys_out.alloc(nullptr, (size_t)nnz * sizeof(uint32_t)))) return rc;
    if ((rc = d_pos_in.alloc(nullptr, (size_t)nnz * sizeof(uint32_t)))) return rc;
    if ((rc = d_pos_out.alloc(nullptr, (size_t)nnz * sizeof(uint32_t)))) return rc;
    const int32_t *d_u = b->d_u.as<int32_t>(), *d_i = b->d_i.as<int32_t>();
    uint32_t *keys_out = d_keys_out.as<uint32_t>(), *pos_in = d_pos_in.as<uint32_t>(), *pos_out = d_pos_out.as<uint32_t>();
    if (nnz > 0) {
        for (int side = 0; side < 2; ++side) {  // the larger of the two sorts' temporary storage
            size_t need = 0;
            PMF_HIP_CHECK(rocprim::radix_sort_pairs(nullptr, need, (const uint32_t *)d_u, keys_out,
                                                    (const uint32_t *)pos_in, pos_out, (size_t)nnz, 0u,
                                                    key_bits(ctx->rows[side]), ctx->stream));
            if (need > tmp_bytes) tmp_bytes = need;
        }
        if ((rc = d_tmp.alloc(nullptr, tmp_bytes))) return rc;
    }
    for (int side = 0; side < 2; ++side) {
        const int32_t *key = side == PMF_SIDE_USER ? d_u : d_i;
        const int32_t *oth = side == PMF_SIDE_USER ? d_i : d_u;
        const double *x = b->d_x.as<double>(), *w = b->d_w.as<double>();
        rc = ctx->dtype == PMF_F64
                 ? order_side<double>(ctx, side, nnz, key, oth, x, w, keys_out, pos_in, pos_out, d_tmp.as(), tmp_bytes)
                 : order_side<float>(ctx, side, nnz, key, oth, x, w, keys_out, pos_in, pos_out, d_tmp.as(), tmp_bytes);
        if (rc) return rc;
    }
    return PMF_OK;
}

// ---------------------------------------------------------------------------
// distinct opposite-side ids per row (pmf_rank_items: "items the user has rated", each once)
// ---------------------------------------------------------------------------
namespace {

// key[p] = row << 32 | other id, for entry p of the side's row order (the row by binary search in ptr)
__global__ void pair_key_kernel(const int64_t *ptr, const int32_t *other, int64_t rows, int64_t nnz, uint64_t *key) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz) return;
    int64_t lo = 0, hi = rows;   // last row with ptr[row] <= p
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (ptr[mid] <= p) lo = mid;
        else hi = mid;
    }
    key[p] = ((uint64_t)lo << 32) | (uint32_t)other[p];
}

__global__ void pair_split_kernel(const uint64_t *key, int64_t n, int32_t *other) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n) other[p] = (int32_t)(uint32_t)key[p];
}

// ptr[r] = number of keys whose row is < r (r = 0 .. rows)
__global__ void pair_ptr_kernel(const uint64_t *key, int64_t n, int64_t rows, int64_t *ptr) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r > rows) return;
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)(key[mid] >> 32) < r) lo = mid + 1;
        else hi = mid;
    }
    ptr[r] = lo;
}

}  // namespace

// Sort-unique of the (row, other id) pairs: one radix sort of 64-bit keys, rocPRIM's unique, and the row offsets by
// binary search.  The temporaries belong to no context; the two result arrays do.
int pmf_index_distinct(pmf_ctx *ctx, int side) {
    PmfSideIndex &ix = ctx->index[side];
    if (ix.d_distinct_ptr) return PMF_OK;
    const int64_t rows = ctx->rows[side], nnz = ctx->nnz;
    PmfBuf d_key, d_sorted, d_count, d_tmp, d_ptr, d_items;
    int rc;
    if ((rc = d_key.alloc(nullptr, (size_t)nnz * sizeof(uint64_t)))) return rc;
    if ((rc = d_sorted.alloc(nullptr, (size_t)nnz * sizeof(uint64_t)))) return rc;
    if ((rc = d_count.alloc(nullptr, sizeof(uint64_t)))) return rc;
    if ((rc = d_ptr.alloc(ctx, (size_t)(rows + 1) * sizeof(int64_t)))) return rc;
    uint64_t *key = d_key.as<uint64_t>(), *sorted = d_sorted.as<uint64_t>();
    uint64_t n_distinct = 0;
    if (nnz > 0) {
        const unsigned bits = 32 + key_bits(rows);
        size_t need_sort = 0, need_unique = 0;
        PMF_HIP_CHECK(rocprim::radix_sort_keys(nullptr, need_sort, key, sorted, (size_t)nnz, 0u, bits, ctx->stream));
        PMF_HIP_CHECK(rocprim::unique(nullptr, need_unique, sorted, key, d_count.as<uint64_t>(), (size_t)nnz,
                                      rocprim::equal_to<uint64_t>(), ctx->stream));
        if ((rc = d_tmp.alloc(nullptr, std::max(need_sort, need_unique)))) return rc;
        hipLaunchKernelGGL(pair_key_kernel, dim3(grid_for(nnz)), dim3(256), 0, ctx->stream, ix.d_ptr.as<int64_t>(),
                           ix.d_other.as<int32_t>(), rows, nnz, key);
        PMF_HIP_CHECK(rocprim::radix_sort_keys(d_tmp.as(), need_sort, key, sorted, (size_t)nnz, 0u, bits, ctx->stream));
        PMF_HIP_CHECK(rocprim::unique(d_tmp.as(), need_unique, sorted, key, d_count.as<uint64_t>(), (size_t)nnz,
                                      rocprim::equal_to<uint64_t>(), ctx->stream));
        PMF_HIP_CHECK(hipMemcpyAsync(&n_distinct, d_count.as(), sizeof(n_distinct), hipMemcpyDeviceToHost, ctx->stream));
        PMF_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    if ((rc = d_items.alloc(ctx, (size_t)n_distinct * sizeof(int32_t)))) return rc;
    if (n_distinct > 0)
        hipLaunchKernelGGL(pair_split_kernel, dim3(grid_for((int64_t)n_distinct)), dim3(256), 0, ctx->stream, key,
                           (int64_t)n_distinct, d_items.as<int32_t>());
    hipLaunchKernelGGL(pair_ptr_kernel, dim3(grid_for(rows + 1)), dim3(256), 0, ctx->stream, key, (int64_t)n_distinct, rows,
                       d_ptr.as<int64_t>());
    PMF_HIP_CHECK(hipGetLastError());
    PMF_HIP_CHECK(hipStreamSynchronize(ctx->stream));   // the keys go with this scope
    ix.d_distinct_ptr = std::move(d_ptr);
    ix.d_distinct = std::move(d_items);
    return PMF_OK;
}
