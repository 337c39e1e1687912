// Host-side chores of the batched entry points: the offset-array check, the layout of one scratch buffer, the cut of
// a CSR batch into row blocks and the argument check and round size of pmf_gauss_sample_rows.  Standard library only --
// no HIP, no context -- so that tests/batch_host_main.cpp and tests/sample_host_main.cpp can build it with a plain host
// compiler and run it under the sanitizers.
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifndef PMF_EINVAL   // (include/pmf_hip.h's values, for a unit that includes this header alone)
#define PMF_OK 0
#define PMF_EINVAL (-1)
#define PMF_ERANGE (-4)
#endif

void pmf_set_error(const char *fmt, ...);

// ptr[0 .. n] are the offsets of a CSR batch of n rows: ptr[0] = 0 and no decrease, or PMF_EINVAL naming the call `fn`,
// the array `name` and the first row that ends before it begins
static inline int pmf_check_offsets(const char *fn, const char *name, const int64_t *ptr, int64_t n) {
    if (ptr[0] != 0) {
        pmf_set_error("%s: %s[0] = %lld, not 0", fn, name, (long long)ptr[0]);
        return PMF_EINVAL;
    }
    for (int64_t r = 0; r < n; ++r)
        if (ptr[r + 1] < ptr[r]) {
            pmf_set_error("%s: %s decreases at row %lld", fn, name, (long long)r);
            return PMF_EINVAL;
        }
    return PMF_OK;
}

// The arguments of pmf_gauss_sample_rows that need no context state, in the order the header lists them (`rows` = rows of
// the side): PMF_EINVAL for a negative n_rows, null row_ids / out, n_draws < 1 or draw0 < 0, PMF_ERANGE naming the first
// id outside [0, rows) and its position.  n_rows = 0 is accepted whatever the pointers are: the call touches nothing.
static inline int pmf_sample_check(const char *fn, int64_t n_rows, const int32_t *row_ids, int n_draws, int draw0,
                                   const void *out, int64_t rows) {
    if (n_rows < 0) {
        pmf_set_error("%s: negative n_rows", fn);
        return PMF_EINVAL;
    }
    if (n_rows == 0) return PMF_OK;
    if (!row_ids || !out) {
        pmf_set_error("%s: null %s", fn, !row_ids ? "row_ids" : "out");
        return PMF_EINVAL;
    }
    if (n_draws < 1) {
        pmf_set_error("%s: n_draws=%d, at least 1 is needed", fn, n_draws);
        return PMF_EINVAL;
    }
    if (draw0 < 0) {
        pmf_set_error("%s: negative draw0 %d", fn, draw0);
        return PMF_EINVAL;
    }
    for (int64_t q = 0; q < n_rows; ++q)
        if (row_ids[q] < 0 || row_ids[q] >= rows) {
            pmf_set_error("%s: row id %d at position %lld outside [0, %lld)", fn, row_ids[q], (long long)q, (long long)rows);
            return PMF_ERANGE;
        }
    return PMF_OK;
}

// Rows of one round of pmf_gauss_sample_rows: as many as keep the round's device tables -- the draws [rows x n_draws x
// kpad] of `elem` bytes, the supplied normals of the same shape (`with_z`) and the row ids -- within `budget` bytes; at
// least one row (a single row over the budget still goes, in a round of its own) and at most n_rows, 0 for no rows.
static inline int64_t pmf_sample_round_rows(int64_t n_rows, int n_draws, int kpad, size_t elem, bool with_z, int64_t budget) {
    if (n_rows <= 0) return 0;
    const int64_t per_row = (int64_t)n_draws * kpad * (int64_t)elem * (with_z ? 2 : 1) + (int64_t)sizeof(int32_t);
    const int64_t fit = budget / per_row;
    return fit < 1 ? 1 : (fit < n_rows ? fit : n_rows);
}

// One buffer carved into typed pieces.  add<T>(n) for every piece, in order; bytes() is what to allocate; piece.at(base)
// is the piece inside an allocation that begins at `base`.  Every piece begins on a multiple of `align` bytes (as `base`
// must).  An empty piece takes no room, so its pointer may be the end of the buffer: pass `keep` for a piece whose
// pointer is handed to a kernel even when it is empty, and it takes one alignment unit.
class PmfLayout {
public:
    template <typename T>
    struct Piece {
        size_t offset;
        T *at(void *base) const { return reinterpret_cast<T *>(static_cast<char *>(base) + offset); }
    };
    explicit PmfLayout(size_t align = 16) : align_(align) {}
    template <typename T>
    Piece<T> add(size_t n, bool keep = false) {
        const Piece<T> piece = {bytes_};
        const size_t units = (n * sizeof(T) + align_ - 1) / align_;
        bytes_ += (units == 0 && keep ? 1 : units) * align_;
        return piece;
    }
    size_t bytes() const { return bytes_; }

private:
    size_t align_, bytes_ = 0;
};

// End row r1 of the block of a CSR batch that begins at row r0: greedily as many rows as stay within `max_rows` rows,
// `max_nnz` entries and the caller's own budget.  fits(n) is called once per row, in order, with the row's length; it
// counts the row and says whether the block still fits with it.  The first row is counted like every other but always
// admitted: a single row over a cap still goes, in a block of its own.
template <typename Fits>
static inline int64_t pmf_block_cut(const int64_t *row_ptr, int64_t n_rows, int64_t r0, int64_t max_rows, int64_t max_nnz,
                                    Fits &&fits) {
    int64_t r1 = r0, nnz = 0;
    for (; r1 < n_rows && r1 - r0 < max_rows; ++r1) {
        const int64_t n = row_ptr[r1 + 1] - row_ptr[r1];
        const bool fit = fits(n);
        if (r1 > r0 && !(fit && nnz + n <= max_nnz)) break;
        nnz += n;
    }
    return r1;
}
