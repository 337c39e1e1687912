// Stand-alone check of prob-matrix-factorization_amd/csrc/pmf_batch.h (tests/test_batch_host_cpu.py builds it with the
// host compiler under the address and undefined-behaviour sanitizers and runs it): the offset-array check, the scratch
// layout and the block cut of the fold-ins.  Exit status 0 when everything holds, else 1 with one line on stderr.
#include "pmf_batch.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

static char g_error[512];

void pmf_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            fprintf(stderr, "%s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                 \
            fprintf(stderr, "\n");                        \
            exit(1);                                      \
        }                                                 \
    } while (0)

static bool ends_with(const char *s, const char *tail) {
    const size_t n = strlen(s), m = strlen(tail);
    return n >= m && strcmp(s + n - m, tail) == 0;
}

// ---- offsets ---------------------------------------------------------------------------------------------------
static void offsets_refused(std::vector<int64_t> ptr, const char *tail) {
    g_error[0] = 0;
    const int rc = pmf_check_offsets("pmf_some_call", "row_ptr", ptr.data(), (int64_t)ptr.size() - 1);
    CHECK(rc == PMF_EINVAL, "offsets: status %d where PMF_EINVAL was due (%s)", rc, tail);
    CHECK(ends_with(g_error, tail), "offsets: message '%s' does not end with '%s'", g_error, tail);
    CHECK(strncmp(g_error, "pmf_some_call: ", 15) == 0, "offsets: message '%s' does not name the call", g_error);
}

static void test_offsets() {
    const std::vector<int64_t> one = {0}, flat = {0, 0, 0};
    g_error[0] = 0;
    CHECK(pmf_check_offsets("f", "row_ptr", one.data(), 0) == PMF_OK && !g_error[0], "offsets: [0] with n = 0 refused: %s", g_error);
    CHECK(pmf_check_offsets("f", "row_ptr", flat.data(), 2) == PMF_OK && !g_error[0], "offsets: [0,0,0] refused: %s", g_error);
    offsets_refused({1, 3}, "row_ptr[0] = 1, not 0");
    offsets_refused({0, 3, 2, 5}, "row_ptr decreases at row 1");
    offsets_refused({0, 3, 2, 1}, "row_ptr decreases at row 1");
}

// ---- layout ----------------------------------------------------------------------------------------------------
struct PieceSpec {
    size_t n;
    bool wide, keep;   // 8-byte elements; handed to a kernel even when empty
};

static void test_layout_case(const std::vector<PieceSpec> &pieces, size_t align) {
    PmfLayout lay(align);
    std::vector<size_t> off;
    for (const PieceSpec &p : pieces) off.push_back(p.wide ? lay.add<double>(p.n, p.keep).offset : lay.add<uint32_t>(p.n, p.keep).offset);
    size_t end = 0;
    for (size_t k = 0; k < pieces.size(); ++k) {
        const size_t bytes = pieces[k].n * (pieces[k].wide ? 8 : 4);
        CHECK(off[k] % align == 0, "layout: offset %zu of piece %zu is no multiple of %zu", off[k], k, align);
        CHECK(off[k] == end, "layout: piece %zu begins at %zu, the piece before it ends at %zu", k, off[k], end);
        // the next multiple of the alignment after its bytes; empty: one unit when kept, else nothing
        end = off[k] + (bytes ? (bytes + align - 1) / align * align : (pieces[k].keep ? align : 0));
    }
    CHECK(lay.bytes() == end, "layout: %zu bytes in all, the last piece ends at %zu", lay.bytes(), end);
    // the pointers, in an allocation of exactly bytes(): every element of every piece is written (the sanitizer watches)
    char *base = static_cast<char *>(aligned_alloc(align, std::max(lay.bytes(), align)));
    CHECK(base != nullptr, "layout: no memory");
    PmfLayout again(align);
    for (size_t k = 0; k < pieces.size(); ++k) {
        const PieceSpec &p = pieces[k];
        if (p.wide) {
            double *d = again.add<double>(p.n, p.keep).at(base);
            CHECK(reinterpret_cast<char *>(d) == base + off[k], "layout: pointer of piece %zu", k);
            for (size_t e = 0; e < p.n; ++e) d[e] = 1.0;
        } else {
            uint32_t *d = again.add<uint32_t>(p.n, p.keep).at(base);
            CHECK(reinterpret_cast<char *>(d) == base + off[k], "layout: pointer of piece %zu", k);
            for (size_t e = 0; e < p.n; ++e) d[e] = 1u;
        }
        if (p.n == 0 && p.keep) CHECK(off[k] + align <= lay.bytes(), "layout: the kept empty piece %zu lies outside the buffer", k);
    }
    free(base);
}

static void test_layout() {
    std::vector<size_t> counts = {0, 1, 3, 17};
    for (size_t align : {(size_t)16, (size_t)256}) {
        std::sort(counts.begin(), counts.end());
        do {   // every order of the four counts, every mix of 4- and 8-byte elements, every choice of kept pieces
            for (int wide = 0; wide < 16; ++wide)
                for (int keep = 0; keep < 16; ++keep) {
                    std::vector<PieceSpec> pieces;
                    for (int k = 0; k < 4; ++k) pieces.push_back({counts[(size_t)k], (wide >> k & 1) != 0, (keep >> k & 1) != 0});
                    test_layout_case(pieces, align);
                }
        } while (std::next_permutation(counts.begin(), counts.end()));
        // an empty piece: one alignment unit when kept, nothing otherwise
        PmfLayout kept(align), dropped(align);
        kept.add<uint32_t>(0, true);
        dropped.add<uint32_t>(0);
        CHECK(kept.bytes() == align && dropped.bytes() == 0, "layout: empty pieces take %zu (kept) and %zu bytes at alignment %zu",
              kept.bytes(), dropped.bytes(), align);
    }
}

// ---- block cut -------------------------------------------------------------------------------------------------
static const int64_t kNoCap = INT32_MAX;

// the Gaussian fold-in's statistics units of a row of n ratings, with task length 4
static int64_t row_units(int64_t n) { return 1 + (n > 4 ? (n + 3) / 4 : 0); }

static void test_cut_case(const std::vector<int64_t> &len, int64_t max_rows, int64_t max_nnz, int64_t max_units) {
    const int64_t n_rows = (int64_t)len.size();
    std::vector<int64_t> ptr(len.size() + 1, 0);
    for (size_t r = 0; r < len.size(); ++r) ptr[r + 1] = ptr[r] + len[r];
    int64_t r0 = 0;
    while (r0 < n_rows) {
        int64_t counted = 0;
        const int64_t r1 = pmf_block_cut(ptr.data(), n_rows, r0, max_rows, max_nnz, [&](int64_t n) { return (counted += row_units(n)) <= max_units; });
        CHECK(r1 > r0 && r1 <= n_rows, "cut: block [%lld, %lld) of %lld rows", (long long)r0, (long long)r1, (long long)n_rows);
        int64_t nnz = 0, units = 0;
        for (int64_t r = r0; r < r1; ++r) {
            nnz += len[(size_t)r];
            units += row_units(len[(size_t)r]);
        }
        const int64_t rows = r1 - r0;
        CHECK(rows == 1 || (rows <= max_rows && nnz <= max_nnz && units <= max_units),
              "cut: block [%lld, %lld) holds %lld rows, %lld entries, %lld units under the caps %lld, %lld, %lld", (long long)r0, (long long)r1,
              (long long)rows, (long long)nnz, (long long)units, (long long)max_rows, (long long)max_nnz, (long long)max_units);
        CHECK(rows <= max_rows, "cut: %lld rows under a row cap of %lld", (long long)rows, (long long)max_rows);
        if (r1 < n_rows) {
            const int64_t n = len[(size_t)r1];
            CHECK(rows + 1 > max_rows || nnz + n > max_nnz || units + row_units(n) > max_units,
                  "cut: block [%lld, %lld) under the caps %lld, %lld, %lld would have held row %lld as well", (long long)r0, (long long)r1,
                  (long long)max_rows, (long long)max_nnz, (long long)max_units, (long long)r1);
        }
        r0 = r1;
    }
    CHECK(r0 == n_rows, "cut: the blocks end at row %lld of %lld", (long long)r0, (long long)n_rows);
}

static void test_cut() {
    const int64_t lengths[] = {0, 1, 2, 5, 9};
    for (int n_rows = 0; n_rows <= 6; ++n_rows) {
        int64_t total = 1;
        for (int r = 0; r < n_rows; ++r) total *= 5;
        for (int64_t code = 0; code < total; ++code) {
            std::vector<int64_t> len;
            for (int64_t r = 0, c = code; r < n_rows; ++r, c /= 5) len.push_back(lengths[c % 5]);
            for (int64_t max_rows : {(int64_t)1, (int64_t)2, (int64_t)3, kNoCap})
                for (int64_t max_nnz : {(int64_t)4, (int64_t)8})
                    for (int64_t max_units : {(int64_t)2, (int64_t)3, kNoCap}) test_cut_case(len, max_rows, max_nnz, max_units);
        }
    }
}

int main() {
    test_offsets();
    test_layout();
    test_cut();
    printf("batch host helpers ok\n");
    return 0;
}
