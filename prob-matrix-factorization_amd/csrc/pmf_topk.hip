// Top-k items per user from the dense reconstruction FACTOR_user . FACTOR_item^T
// (+ biases): the one dense contraction of the product, so it runs on the matrix
// cores (v_mfma_f32_32x32x2_f32, exact fp32 FMA chains) for fp32 contexts.
// Scores follow `predict` (hpf_cavi.py:215-231); ties go to the lower item id.
//
// Two phases per batch of Q query users: (1) score tile kernel writes
// scores[Q x I]; (2) one wavefront per user selects the k best in k passes
// (each pass = strided scan + wave arg-max restricted to entries ranked after
// the previous pick), which is deterministic and needs no sorting network.
#include <algorithm>
#include <climits>
#include <type_traits>

#include "pmf_device.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct TopkParams {
    const int32_t *users;  // [nq] query user ids (device)
    int nq;
    int64_t n_items;
    int K, kpad;
};

// TopkParams of an excluding call (pmf_topk_items_excluding): item j is no candidate of user u when it is among
// ex_items[ex_ptr[u] .. ex_ptr[u + 1]), ascending item ids, each once -- the context's distinct training items
// (pmf_index_distinct), as in RankParams; pmf_topk_query hands a caller's own CSR, indexed by the staged row, to the same
// two pointers.
struct TopkExcludeParams : TopkParams {
    const int64_t *ex_ptr;
    const int32_t *ex_items;
};

// 32 users x 32 items per wavefront, 4 item tiles per block.
// (bu / bi: BIAS arrays when mode == PMF_PREDICT_BIAS, SCALE arrays when mode == PMF_PREDICT_SCALE, else null)
__global__ __launch_bounds__(256) void topk_scores_f32_kernel(TopkParams p, const float *fu, const float *fi,
                                                              const float *bu, const float *bi, int mode, float *scores) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int h = lane >> 5, c = lane & 31;
    const int q0 = blockIdx.x * 32;
    const int64_t i0 = ((int64_t)blockIdx.y * 4 + wave) * 32;
    if (i0 >= p.n_items) return;
    // k is split between the two half-waves: half h covers [h*H, (h+1)*H)
    const int H = ((p.kpad / 2) + 3) / 4 * 4;
    const int q = q0 + c;
    const int64_t it = i0 + c;
    const int user = (q < p.nq) ? p.users[q] : -1;
    const float *arow = (user >= 0) ? fu + (int64_t)user * p.kpad : nullptr;
    const float *brow = (it < p.n_items) ? fi + it * p.kpad : nullptr;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int t = 0; t < H; t += 4) {
        const int k = h * H + t;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if (k < p.kpad) {
            if (arow) a = *reinterpret_cast<const float4 *>(arow + k);
            if (brow) b = *reinterpret_cast<const float4 *>(brow + k);
        }
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
    }
    // C/D layout: col = lane & 31 (item), row = (r&3) + 8*(r>>2) + 4*(lane>>5) (user)
    const float bcol = (bi && it < p.n_items) ? bi[it] : 0.f;
    const bool scale = mode == PMF_PREDICT_SCALE;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
        const int qq = q0 + row;
        if (qq < p.nq && it < p.n_items) {
            float s = acc[r];
            if (bu) s = scale ? s * (bu[p.users[qq]] * bcol) : bu[p.users[qq]] + bcol + s;
            scores[(int64_t)qq * p.n_items + it] = s;
        }
    }
}

// fp64 contexts: plain dot products (parity mode, not a throughput path)
__global__ void topk_scores_f64_kernel(TopkParams p, const double *fu, const double *fi, const double *bu,
                                       const double *bi, int mode, double *scores) {
    const int64_t total = (int64_t)p.nq * p.n_items;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int q = (int)(e / p.n_items);
        const int64_t it = e % p.n_items;
        const int user = p.users[q];
        const double *a = fu + (int64_t)user * p.kpad, *b = fi + it * p.kpad;
        double s = 0.0;
        for (int k = 0; k < p.K; ++k) s = fma(a[k], b[k], s);
        if (bu) s = mode == PMF_PREDICT_SCALE ? s * (bu[user] * bi[it]) : bu[user] + bi[it] + s;
        scores[e] = s;
    }
}

// Exclusion on the two-phase path, between the score kernel and the select: the score of every excluded (query row, item)
// pair becomes NaN, which the select never ranks.  One block per query row at a time, one thread per list entry (a user
// repeated in the batch has a row of its own per repeat).
template <typename S>
__global__ __launch_bounds__(256) void topk_exclude_scores_kernel(TopkExcludeParams p, S *scores) {
    for (int q = blockIdx.x; q < p.nq; q += gridDim.x) {
        const int user = p.users[q];
        const int64_t end = p.ex_ptr[user + 1];
        for (int64_t e = p.ex_ptr[user] + threadIdx.x; e < end; e += blockDim.x)
            scores[(int64_t)q * p.n_items + p.ex_items[e]] = (S)__builtin_nanf("");
    }
}

// (value desc, index asc) order helpers
template <typename S>
__device__ __forceinline__ bool ranks_before(S v1, int i1, S v2, int i2) {
    return v1 > v2 || (v1 == v2 && i1 < i2);
}

// wave arg-best under (value desc, index asc); every lane returns the winner
template <typename S>
__device__ __forceinline__ void wave_best(S &bv, int &bidx, bool &found) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const S ov = __shfl_xor(bv, off, 64);
        const int oi = __shfl_xor(bidx, off, 64);
        const int of = __shfl_xor((int)found, off, 64);
        if (of && (!found || ranks_before(ov, oi, bv, bidx))) {
            bv = ov;
            bidx = oi;
            found = true;
        }
    }
}

// A wavefront writes one user's k best candidates, best first, to out_items / out_scores (the user's k entries): k passes,
// each the wave arg-best of the candidates that rank after the previous pick -- deterministic, no sorting network.
// scan(visit) calls visit(value, index) for every candidate of this lane (no NaN among them).  Fewer than k candidates:
// the rest is item -1, score 0.0.
template <typename S, typename Scan>
__device__ __forceinline__ void topk_select_passes(int lane, int k, int32_t *out_items, double *out_scores, Scan &&scan) {
    bool have_prev = false;
    S pv = (S)0;
    int pi = -1;
    for (int t = 0; t < k; ++t) {
        bool found = false;
        S bv = (S)0;
        int bidx = 0x7fffffff;
        scan([&](S v, int i) __attribute__((always_inline)) {
            if (have_prev && !ranks_before(pv, pi, v, i)) return;
            if (!found || ranks_before(v, i, bv, bidx)) {
                bv = v;
                bidx = i;
                found = true;
            }
        });
        wave_best(bv, bidx, found);
        if (lane == 0) {
            out_items[t] = found ? bidx : -1;
            out_scores[t] = found ? (double)bv : 0.0;
        }
        if (!found) {  // fewer than k rankable items: fill the rest
            for (int r = t + 1; r < k && lane == 0; ++r) {
                out_items[r] = -1;
                out_scores[r] = 0.0;
            }
            break;
        }
        have_prev = true;
        pv = bv;
        pi = bidx;
    }
}

// One wavefront per user, k <= 64.  Two passes over the user's score row instead of k:
//  (1) per-lane maxima; the k-th largest of the 64 lane maxima is a lower bound tau of the
//      k-th best score (the k best lane maxima are k distinct entries >= tau);
//  (2) every entry >= tau is compacted (ballot + prefix) into an LDS candidate list, from
//      which the k winners are drawn with the deterministic (value desc, index asc) rule.
// A list that would overflow (massive ties) falls back to the k-pass scan of the row.
#define TOPK_CAP 1024
template <typename S>
__global__ __launch_bounds__(256) void topk_select_kernel(const S *scores, int nq, int64_t n_items, int k,
                                                          int32_t *out_items, double *out_scores) {
    __shared__ S c_val[4][TOPK_CAP];
    __shared__ int c_idx[4][TOPK_CAP];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + wave;
    if (q >= nq) return;
    const S *row = scores + (int64_t)q * n_items;
    S *cv = c_val[wave];
    int *ci = c_idx[wave];
    int count = -1;  // -1: candidate list unusable -> scan the row itself
    if (k <= 64) {
        // pass 1: lane maxima
        bool have = false;
        S lm = (S)0;
        for (int64_t i = lane; i < n_items; i += 64) {
            const S v = row[i];
            if (v == v && (!have || v > lm)) {
                lm = v;
                have = true;
            }
        }
        // k-th largest lane maximum (values only; ties are harmless for a lower bound)
        S tau = (S)0;
        bool tau_ok = false;
        {
            bool alive = have;
            for (int t = 0; t < k; ++t) {
                S bv = lm;
                int bidx = lane;
                bool found = alive;
                wave_best(bv, bidx, found);
                tau_ok = found;
                if (!found) break;
                tau = bv;
                if (lane == bidx) alive = false;
            }
        }
        if (tau_ok) {
            // pass 2: compact entries >= tau
            count = 0;
            const int64_t rounds = (n_items + 63) / 64;
            for (int64_t r = 0; r < rounds && count >= 0; ++r) {
                const int64_t i = r * 64 + lane;
                S v = (S)0;
                bool pred = false;
                if (i < n_items) {
                    v = row[i];
                    pred = (v == v) && v >= tau;
                }
                const unsigned long long mask = __ballot(pred);
                const int n = __popcll(mask);
                if (n) {
                    if (count + n > TOPK_CAP) {
                        count = -1;
                    } else {
                        if (pred) {
                            const int at = count + __popcll(mask & ((1ull << lane) - 1ull));
                            cv[at] = v;
                            ci[at] = (int)i;
                        }
                        count += n;
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
    topk_select_passes<S>(lane, k, out_items + (int64_t)q * k, out_scores + (int64_t)q * k, [&](auto visit) __attribute__((always_inline)) {
        if (count >= 0) {
            for (int e = lane; e < count; e += 64) visit(cv[e], ci[e]);
        } else {
            for (int64_t i = lane; i < n_items; i += 64) {
                const S v = row[i];
                if (v == v) visit(v, (int)i);         // NaN never ranks
            }
        }
    });
}

// ---------------------------------------------------------------------------
// fused score + select, fp32, Kpad <= 128, k <= 64: scores never touch HBM
// ---------------------------------------------------------------------------
// One wavefront owns 32 query users for a whole segment of the item range; the four wavefronts of a block
// walk that range together.  A wave's A operand -- its 32 users' factor rows -- is loaded ONCE into KH
// registers per lane (lane (i = l & 31, h = l >> 5) holds the 16-byte pieces 2 q + h, q = 0 .. KH / 4 - 1, of
// user i: the k order of the MFMA steps is a permutation, the same one for both operands) and stays there.
// The B operand is staged by the block: ST item rows per stage are fetched with fully coalesced 16-byte
// loads (a thread's piece is contiguous with its neighbours': 2 lines per 256-byte row, where a lane-per-row
// load touches 64 lines per instruction and left the kernel bound by the texture addresser, 0.58 of the MFMA
// peak), parked in registers while the previous stage is multiplied, and written to one of two LDS buffers
// with an odd row pitch (KH / 2 + 1 pieces), from which every wave reads its MFMA layout with conflict-free
// ds_read_b128 -- each item row leaves the L2 once per 128 users instead of once per 32.  One barrier per
// stage.  Per 32-item tile a wave runs KH v_mfma_f32_32x32x2_f32 and compares its 16 scores with the users'
// current k-th best.  Almost every tile ends there (a user's list changes about k ln(N / k) times over N
// items); a score that does qualify is inserted into that user's sorted list in LDS by the lanes of the
// wave in parallel (lane e holds entry e: one compare, one ballot, one shift), in ascending item order, so
// ties keep the lower item id.  With few query users the item range is cut into segments (gridDim.y) so
// that the chip is filled; a merge kernel then picks the k best of the segments' lists.
// (The A pieces, the MFMA chain, the score and the priority slices are functions that rank_fused_kernel uses too.  Its
//  staging lambdas, publish and stage loop are still a COPY of this kernel's, less the one-buffer publish and the priority
//  rotation before the last full stage: as a shared function or struct, in nine spellings, they changed the register
//  allocation of rank_fused_kernel<32, 0, 1> into one with VGPR spills.  A change to the staging or the stage loop of
//  either kernel belongs in the other too.)
#define TOPK_NEG_INF (-__builtin_inff())
#ifndef PRIO_SLICE
#define PRIO_SLICE 16      // stages between priority rotations (tools/probe_topk_stamps.py sweeps it: 1 .. 64 are equivalent)
#endif

#ifdef PMF_TOPK_STAMPS
// DIAGNOSTIC BUILD ONLY (tools/probe_topk_stamps.py compiles this file with -DPMF_TOPK_STAMPS into a library of its
// own; the product library has no stamp): per (wavefront, user tile) the 100 MHz real-time stamps of the scan's begin
// and end, the block's grid size and its XCC id -- the residency timeline of a launch -- and the shader-clock cycles
// the wave spent ranking candidates and waiting at the stage barriers, with the number of candidates.
__device__ long long g_topk_stamps[16384 * 8];
extern "C" int pmf_debug_topk_stamps(long long *host, int n_waves) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_topk_stamps), (size_t)n_waves * 8 * sizeof(long long));
}
#endif

// v_writelane_b32: (value, lane, old) -> old with `value` in lane `lane` (both wave-uniform).  This clang has no
// __builtin for it; a declaration carrying the intrinsic's name binds to it.
extern "C" __device__ int pmf_writelane(int value, int lane, int old) __asm("llvm.amdgcn.writelane");

// list keys of the fused kernel: (score bits mapped so that unsigned order is the scores' order) << 32 | ~item.  An empty
// entry is -inf's key with a zero low word: below every candidate's key (no item id has ~item == 0), and its score
// reads back as -inf without a special case.
#define TOPK_EMPTY_KEY 0x007fffff00000000ull
__device__ __forceinline__ unsigned topk_key_score_bits(unsigned hi) {   // (integer throughout: stays on the scalar unit)
    return hi ^ ((int)hi < 0 ? 0x80000000u : 0xffffffffu);
}
__device__ __forceinline__ float topk_key_score(unsigned hi) { return __uint_as_float(topk_key_score_bits(hi)); }

template <int KH>
struct TopkStage {
    static constexpr int ST = KH == 8 ? 64 : 32;      // item rows per stage (one MFMA tile; two where a tile is too short a load)
    static constexpr int PR = KH / 2;                 // 16-byte pieces per (padded) factor row
    static constexpr int PQ = PR + 1;                 // LDS row pitch in pieces; odd -> the 16 lanes of a b128 group hit 16 bank quads
    static constexpr int LPT = ST * PR / 256;         // pieces fetched per thread per stage
    static constexpr size_t buffer_bytes = (size_t)ST * PQ * 16;   // the kernel takes one or two of these (nbuf)
};

// LDS of topk_fused_kernel behind its stage buffers: the block's 4 x 32 lists of k 8-byte keys, + 64 entries (insert()
// reads a full wave's width), then -- excluding scans only -- 20 bytes per wave and local user (the kernel says what)
__host__ __device__ constexpr size_t topk_list_bytes(int k) { return (size_t)4 * 32 * k * 8 + 512; }
#define TOPK_EXCLUDE_LDS_BYTES (4 * 32 * 20)

// The score arithmetic of the fused kernels -- topk_fused_kernel, rank_fused_kernel and rank_rows_kernel -- is the three
// functions below and nothing else: pmf_rank_items is right only if all three give a score with the same bits (an MFMA
// output element depends on its A row, its B column and the k sequence only).

// A operand: lane (c = l & 31, h = l >> 5) holds the 16-byte pieces 2 q + h, q = 0 .. KH / 4 - 1, of the row of `user`
// in a[4 q .. 4 q + 3]; this is the piece of t = 4 q (zero past Kpad, and for user < 0: no user).
// (The caller keeps the loop over t: the same loop inside a function of its own changes the register allocation of every
//  fused kernel -- topk_fused_kernel<16, 0, 2> goes from 87 to 99 VGPRs, five waves per SIMD to four;
//  tools/kernel_asm_table.py shows it.)
__device__ __forceinline__ float4 topk_a_piece(const float *fu, int user, int kpad, int h, int t) {
    const int kk = 2 * t + 4 * h;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (user >= 0 && kk < kpad) v = *reinterpret_cast<const float4 *>(fu + (int64_t)user * kpad + kk);
    return v;
}

// the KH MFMA steps of one 32-item tile; piece(t), t = 0, 4, .., KH - 4, is piece t / 2 + h of this lane's item (column c)
// -- past Kpad the last piece again, as the stage holds it (the A operand is zero there)
template <int KH, typename Piece>
__device__ __forceinline__ void topk_mfma_tile(const float (&a)[KH], f32x16 &acc, Piece &&piece) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int t = 0; t < KH; t += 4) {
        const f32x4 b = piece(t);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t + 1], b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t + 2], b.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t + 3], b.w, acc, 0, 0, 0);
    }
}

// dot product -> score: predict's arithmetic order (ucst / ccst: the user's and the item's bias or scale)
template <int MODE, typename S>
__device__ __forceinline__ S rank_score(S dot, S ucst, S ccst) {
    if (MODE == PMF_PREDICT_BIAS) return ucst + ccst + dot;
    if (MODE == PMF_PREDICT_SCALE) return dot * (ucst * ccst);
    return dot;
}

// Time-sliced priority.  Left alone, the SIMD's arbitration favours the same resident wave for a whole scan: the
// four blocks of a CU then finish one after the other (9.4 .. 16.5 ms for the same work) and the last quarter of
// the launch runs at 3, 2, 1 blocks per CU.  Rotating s_setprio over the SIMD's wave slots every PRIO_SLICE stages
// makes them finish together (12.3 .. 12.7 ms): profiles/r03_topk_wave_stamps.jsonl.
__device__ __forceinline__ int topk_wave_slot() {   // HW_ID.WAVE_ID: this wave's slot on its SIMD
    return __builtin_amdgcn_s_getreg(4 | (0 << 6) | (3 << 11)) & 3;
}
__device__ __forceinline__ void topk_slice_priority(int slot, int stage_no) {
    switch ((slot + stage_no / PRIO_SLICE) & 3) {
        case 0: __builtin_amdgcn_s_setprio(0); break;
        case 1: __builtin_amdgcn_s_setprio(1); break;
        case 2: __builtin_amdgcn_s_setprio(2); break;
        default: __builtin_amdgcn_s_setprio(3); break;
    }
}

// (waves per SIMD the register allocation must leave room for: four for the plain K <= 64 scan, whose lists leave room for
//  four blocks per CU; the bias / scale modes and K > 64 need more registers than that)
// EXCLUDE: the epilogue policy of pmf_topk_items_excluding -- a score that passed its user's threshold is dropped in
// drain() when its item is on the user's exclusion list, before it reaches insert(); the tile test and the stage loop are
// those of the plain scan.  (The exclusion pointers ride in the first argument, whose type depends on EXCLUDE: the plain
// instantiations keep their argument layout, and with it their code.)
template <int KH, int MODE, int NBUF, bool EXCLUDE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(KH <= 32 ? (MODE == 0 ? 4 : 3) : 2))) void topk_fused_kernel(std::conditional_t<EXCLUDE, TopkExcludeParams, TopkParams> p, const float *fu, const float *fi, const float *cu,
                                                         const float *ci, int k, int64_t seg_items, int nseg,
                                                         float *cand_val, int32_t *cand_idx, int32_t *out_items,
                                                         double *out_scores) {
    using S = TopkStage<KH>;
    constexpr int ST = S::ST, PR = S::PR, PQ = S::PQ, LPT = S::LPT;
    constexpr int nbuf = NBUF;                        // stage buffers: two, or one where that keeps another block on the CU
    extern __shared__ __align__(16) unsigned char smem_raw[];
    // (readfirstlane: the wave index is uniform, and the compiler only knows it once told -- what hangs off q0 then
    //  branches on SCC instead of masking exec)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int h = lane >> 5, c = lane & 31;
    f32x4 *stage = reinterpret_cast<f32x4 *>(smem_raw);                                          // [nbuf][ST][PQ]
    // [32][k] list entries of this wave's users, best first: 64-bit keys (insert() below)
    unsigned long long *le = reinterpret_cast<unsigned long long *>(smem_raw + nbuf * S::buffer_bytes) + (size_t)wave * 32 * k;
    // EXCLUDE: behind the lists and their padding (topk_list_bytes), per wave and local user, where the user's exclusion
    // list begins in ex_items, (position of the first entry not yet passed, length) relative to that -- 32-bit, so
    // that drain() compares them on the scalar unit -- and the item id AT that position (past the end: INT_MAX), which
    // clears most candidates without a look at the list
    unsigned char *ex_lds = smem_raw + nbuf * S::buffer_bytes + topk_list_bytes(k) + (size_t)wave * (TOPK_EXCLUDE_LDS_BYTES / 4);
    long long *ex_start = reinterpret_cast<long long *>(ex_lds);          // [32]
    int2 *ex_at = reinterpret_cast<int2 *>(ex_lds + 32 * sizeof(long long));   // [32] (x: position, y: length)
    int *ex_next = reinterpret_cast<int *>(ex_lds + 32 * (sizeof(long long) + sizeof(int2)));   // [32]
    const int seg = blockIdx.y;
    // (item indices are ints in here -- the host sends more than 2^31 - 64 items to the two-phase path: 64-bit compares
    //  have no scalar form, and every instruction of this loop is paid for)
    const int i_begin = (int)((int64_t)seg * seg_items);
    const int i_end = (int)((int64_t)i_begin + seg_items < p.n_items ? (int64_t)i_begin + seg_items : p.n_items);
    const int kpad = p.kpad;

    // PERSISTENT blocks: the grid is sized to what the chip holds at once (launch_topk_fused_mode) and a block walks
    // the 128-user tiles blockIdx.x, blockIdx.x + gridDim.x, ...
    const int n_user_tiles = (p.nq + 127) / 128;
    for (int ut = blockIdx.x; ut < n_user_tiles; ut += gridDim.x) {
    const int q0 = (ut * 4 + wave) * 32;
    const bool active = q0 < p.nq;                     // a wave without users still stages item rows
#ifdef PMF_TOPK_STAMPS
    const long long st_begin = __builtin_amdgcn_s_memrealtime();
    long long st_drain = 0, st_barrier = 0, st_cand = 0, st_tiles = 0;
#endif
    auto barrier = [&]() __attribute__((always_inline)) {   // the scan's block barrier (the stamped build times the wait)
#ifdef PMF_TOPK_STAMPS
        const long long t_ = __builtin_amdgcn_s_memtime();
#endif
        __syncthreads();
#ifdef PMF_TOPK_STAMPS
        st_barrier += __builtin_amdgcn_s_memtime() - t_;
#endif
    };

    // A operand: this lane's pieces of user (q0 + c)'s row, resident for the whole scan
    const int user = (q0 + c < p.nq) ? p.users[q0 + c] : -1;
    float a[KH];
#pragma unroll
    for (int t = 0; t < KH; t += 4) {
        const float4 v = topk_a_piece(fu, user, kpad, h, t);
        a[t] = v.x; a[t + 1] = v.y; a[t + 2] = v.z; a[t + 3] = v.w;
    }
    // per accumulator register r: the user of row (r & 3) + 8 (r >> 2) + 4 h, its bias / scale, its k-th best
    float tau[16], ucst[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int qq = q0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        tau[r] = qq < p.nq ? TOPK_NEG_INF : __builtin_inff();   // rows past the last query never qualify
        ucst[r] = MODE == PMF_PREDICT_SCALE ? 1.f : 0.f;
        if (MODE != 0 && qq < p.nq) ucst[r] = cu[p.users[qq]];
    }
    for (int e = lane; e < 32 * k; e += 64) le[e] = TOPK_EMPTY_KEY;
    if constexpr (EXCLUDE) {
        // lane c: user (q0 + c)'s list, and where this segment's part of it begins (the first entry >= i_begin) -- the
        // scan only ever moves on from there
        long long first = 0;
        int at = 0, n = 0;
        if (user >= 0) {
            first = p.ex_ptr[user];
            n = (int)(p.ex_ptr[user + 1] - first);     // (distinct items of one user: fewer than n_items)
            int hi = n;
            while (i_begin > 0 && at < hi) {
                const int mid = at + ((hi - at) >> 1);
                if (p.ex_items[first + mid] < i_begin) at = mid + 1; else hi = mid;
            }
        }
        if (h == 0) {
            ex_start[c] = first;
            ex_at[c] = make_int2(at, n);
            ex_next[c] = at < n ? p.ex_items[first + at] : INT_MAX;
        }
    }

    // Loads are unconditional (no branch, nothing for the loop's wait counters to merge): a row past the
    // segment's end re-reads the last row (its scores are never ranked), a piece past Kpad re-reads the
    // last piece (the A operand is zero there).
    // (The scan is bound by the fp32 matrix pipe, and on gfx950 the fp32 MFMA shares the SIMD's fp32 lanes with the VALU:
    //  every vector instruction of ANY resident wave costs the pipe its issue cycles -- profiles/r03_topk_wave_stamps.jsonl:
    //  9.5 k cycles per tile for four waves whose MFMAs need 8.2 k.  Hence the running pointers here instead of 64-bit
    //  row-address arithmetic per stage, and the scalar masks in the threshold test below.)
    f32x4 g[LPT];
    const int last_piece = kpad / 4 - 1;
    // full stages: one scalar base for the block, advanced per stage, plus this thread's constant 32-bit byte offsets
    // (global_load with an SGPR base: no per-thread pointer arithmetic in the loop)
    const char *next_stage = reinterpret_cast<const char *>(fi + (int64_t)i_begin * kpad);
    const unsigned stage_bytes = (unsigned)ST * kpad * 4;
    unsigned goff[LPT];
#pragma unroll
    for (int j = 0; j < LPT; ++j) {
        const int idx = j * 256 + (int)threadIdx.x;
        const int r = idx / PR, pc = idx % PR;
        goff[j] = ((unsigned)r * kpad + 4u * (pc < last_piece ? pc : last_piece)) * 4u;
    }
    auto fetch_full = [&]() __attribute__((always_inline)) {          // (out of line, g[] would live in scratch)
#pragma unroll
        for (int j = 0; j < LPT; ++j) {
            unsigned off = goff[j];
            asm volatile("" : "+v"(off));             // (keeps the zero-extension in the loop: SGPR base + 32-bit VGPR offset)
            g[j] = *reinterpret_cast<const f32x4 *>(next_stage + off);
        }
        next_stage += stage_bytes;
    };
    auto fetch_tail = [&](int i0) __attribute__((always_inline)) {    // the segment's last, partial stage
#pragma unroll
        for (int j = 0; j < LPT; ++j) {
            const int idx = j * 256 + (int)threadIdx.x;
            const int r = idx / PR, pc = idx % PR;
            const int it = i0 + r < i_end ? i0 + r : i_end - 1;
            g[j] = *reinterpret_cast<const f32x4 *>(fi + (int64_t)it * kpad + 4 * (pc < last_piece ? pc : last_piece));
        }
    };
    auto stash = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < LPT; ++j) {
            const int idx = j * 256 + (int)threadIdx.x;
            stage[(size_t)buf * ST * PQ + (idx / PR) * PQ + idx % PR] = g[j];
        }
    };
    // insert the candidate (score bits vb, ~item) into the list of local user `ul`; returns that list's new k-th best value
    // (its bits).  Lane e holds entry e.  An entry is one 64-bit key, (score bits made monotone) << 32 | ~item: a bigger key
    // ranks first, so the candidate's place is ONE 64-bit compare and a ballot, its key is built with scalar instructions
    // and dropped into its lane with v_writelane, and the entries behind it move down one lane by DPP under an EXEC mask
    // the scalar unit derives from the ballot.  EVERY instruction counts here, scalar ones as much as vector ones: beside
    // waves that stream MFMAs an instruction of a ranking wave costs the SIMD about five cycles whatever unit runs it
    // (profiles/r03_topk_instruction_cost.log) -- hence the one asm block (no EXEC save / restore pairs, no branch
    // around the masked store, lane select straight from an SGPR, both words stored by one ds_write2).
    const unsigned long long kmask = k >= 64 ? ~0ull : (1ull << k) - 1;   // the lanes that hold list entries
    typedef __attribute__((address_space(3))) unsigned long long lds_u64;
    const unsigned le_lane = (unsigned)(size_t)(lds_u64 *)(le + lane);    // LDS byte address of this lane's entry of list 0
    auto insert = [&](int ul, unsigned vb, unsigned nitem) __attribute__((always_inline)) -> unsigned {
        if (vb == 0x80000000u) vb = 0u;                              // -0.0 ranks as +0.0 does
        const unsigned ov = vb ^ ((unsigned)((int)vb >> 31) | 0x80000000u);
        const unsigned long long ck = ((unsigned long long)ov << 32) | nitem;
        // (every lane reads: past entry k - 1 it is the next lists' entries, or the padding behind the last one; they are
        //  masked out of the ballot and never written back -- no divergent region, the k-th entry is read as a scalar)
        const unsigned long long e = le[ul * k + lane];
        unsigned lo = (unsigned)e, hi = (unsigned)(e >> 32);
        const int pos = __popcll(__builtin_amdgcn_ballot_w64(e > ck) & kmask);   // entries that rank before the candidate
        if (pos < k) {                                               // (an earlier candidate of this tile may have filled the list)
            // lanes >= pos take the entry of the lane below (lane pos has no active source: it keeps its entry until the
            // writelane), the candidate goes into lane pos, lanes < k store.  EXEC is all ones here (no divergent region).
            asm volatile("s_mov_b32 m0, %[pos]\n\t"               // (one SGPR per vector instruction: the lane select rides in M0,
                         "s_mov_b64 exec, %[from]\n\t"             //  which nothing else in this kernel uses -- tests/test_abi_cpu.py)
                         "s_nop 4\n\t"
                         "v_mov_b32_dpp %[lo], %[lo] wave_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                         "v_mov_b32_dpp %[hi], %[hi] wave_shr:1 row_mask:0xf bank_mask:0xf\n\t"
                         "s_mov_b64 exec, %[kmask]\n\t"
                         "v_writelane_b32 %[lo], %[nitem], m0\n\t"
                         "v_writelane_b32 %[hi], %[ov], m0\n\t"
                         "ds_write2_b32 %[addr], %[lo], %[hi] offset1:1\n\t"
                         "s_mov_b64 exec, -1"
                         : [lo] "+v"(lo), [hi] "+v"(hi)
                         : [from] "s"(~0ull << pos), [kmask] "s"(kmask), [nitem] "s"(nitem), [ov] "s"(ov), [pos] "s"(pos),
                           [addr] "v"(le_lane + (unsigned)(ul * k) * 8u)
                         : "memory");
        }
        const unsigned kth = (unsigned)__builtin_amdgcn_readlane((int)hi, k - 1);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        return topk_key_score_bits(kth);
    };

    // dot products -> scores; TAIL: the stage holds rows past the segment's end
    auto scores = [&](auto TAIL, int i0, f32x16 &acc) __attribute__((always_inline)) {
        if (MODE == 0) return;
        const int it = i0 + c;
        float ccst = MODE == PMF_PREDICT_SCALE ? 1.f : 0.f;
        if (!decltype(TAIL)::value || it < i_end) ccst = ci[it];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = rank_score<MODE>(acc[r], ucst[r], ccst);
    };
    // Does any score of the tile reach its user's list?  Almost never (a list changes ~k ln(N / k) times in N items), so
    // the test itself is what a tile pays: 16 v_cmpx narrow EXEC to the lanes whose rows are ALL below their thresholds
    // -- no mask per row, no OR chain (16 scalar instructions the compare-and-collect form needs) -- and two scalar
    // instructions see whether that is every lane.  (Two asm blocks: an asm statement takes 30 operands.  Each leaves
    // EXEC as it found it.  The s_nop pair is the MFMA -> VALU read distance the compiler cannot see into an asm for.)
    auto all_below = [&](const f32x16 &acc, unsigned long long &m1, unsigned long long &m2) __attribute__((always_inline)) -> bool {
        asm volatile("s_nop 15\n\ts_nop 3\n\t"
                     "v_cmpx_lt_f32 vcc, %[a0], %[t0]\n\tv_cmpx_lt_f32 vcc, %[a1], %[t1]\n\t"
                     "v_cmpx_lt_f32 vcc, %[a2], %[t2]\n\tv_cmpx_lt_f32 vcc, %[a3], %[t3]\n\t"
                     "v_cmpx_lt_f32 vcc, %[a4], %[t4]\n\tv_cmpx_lt_f32 vcc, %[a5], %[t5]\n\t"
                     "v_cmpx_lt_f32 vcc, %[a6], %[t6]\n\tv_cmpx_lt_f32 vcc, %[a7], %[t7]\n\t"
                     "s_mov_b64 %[m], exec\n\ts_mov_b64 exec, -1"
                     : [m] "=s"(m1)
                     : [a0] "v"(acc[0]), [t0] "v"(tau[0]), [a1] "v"(acc[1]), [t1] "v"(tau[1]), [a2] "v"(acc[2]), [t2] "v"(tau[2]),
                       [a3] "v"(acc[3]), [t3] "v"(tau[3]), [a4] "v"(acc[4]), [t4] "v"(tau[4]), [a5] "v"(acc[5]), [t5] "v"(tau[5]),
                       [a6] "v"(acc[6]), [t6] "v"(tau[6]), [a7] "v"(acc[7]), [t7] "v"(tau[7])
                     : "vcc");
        asm volatile("v_cmpx_lt_f32 vcc, %[a0], %[t0]\n\tv_cmpx_lt_f32 vcc, %[a1], %[t1]\n\t"
                     "v_cmpx_lt_f32 vcc, %[a2], %[t2]\n\tv_cmpx_lt_f32 vcc, %[a3], %[t3]\n\t"
                     "v_cmpx_lt_f32 vcc, %[a4], %[t4]\n\tv_cmpx_lt_f32 vcc, %[a5], %[t5]\n\t"
                     "v_cmpx_lt_f32 vcc, %[a6], %[t6]\n\tv_cmpx_lt_f32 vcc, %[a7], %[t7]\n\t"
                     "s_mov_b64 %[m], exec\n\ts_mov_b64 exec, -1"
                     : [m] "=s"(m2)
                     : [a0] "v"(acc[8]), [t0] "v"(tau[8]), [a1] "v"(acc[9]), [t1] "v"(tau[9]), [a2] "v"(acc[10]), [t2] "v"(tau[10]),
                       [a3] "v"(acc[11]), [t3] "v"(tau[11]), [a4] "v"(acc[12]), [t4] "v"(tau[12]), [a5] "v"(acc[13]), [t5] "v"(tau[13]),
                       [a6] "v"(acc[14]), [t6] "v"(tau[14]), [a7] "v"(acc[15]), [t7] "v"(tau[15])
                     : "vcc");
        return (m1 & m2) == ~0ull;
    };
    // the 16 threshold compares with their lane masks left in SGPRs (v_cmp -> s[..]): the scan for candidates is scalar
    auto thresholds = [&](int r0, int r1, const f32x16 &acc, unsigned long long (&mk)[16]) __attribute__((always_inline)) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (r >= r0 && r < r1) mk[r] = __builtin_amdgcn_ballot_w64(acc[r] >= tau[r]);
    };
    // EXCLUDE: is `item` on the exclusion list of local user `ul`?  Everything here is wave-uniform.  A user's candidates
    // reach drain() in ascending item order (tiles ascend, the lanes of a row ascend) and the list is sorted the same
    // way, so one cursor per user only moves forward.  A candidate below the item id at the cursor is cleared by one LDS
    // read and a scalar compare -- a load from the list here would be waited for behind the stage prefetch by the whole
    // block, on every candidate.  Otherwise the cursor has to move (at most twice per list entry): the 64 lanes load the
    // 64 entries at the cursor (past the end: an id above every item's), one ballot of `< item` advances the cursor, one
    // of `== item` answers, and the entry now at the cursor is read from the loaded ones; the loop repeats only when all
    // 64 entries were below.  The load is unconditional (the index is clamped) and the branches are scalar: EXEC stays
    // all ones for insert().
    auto excluded = [&](int ul, int item) __attribute__((always_inline)) -> bool {
        if constexpr (EXCLUDE) {
            if (item < __builtin_amdgcn_readfirstlane(ex_next[ul])) return false;
            const int2 pn = ex_at[ul];
            const int n = __builtin_amdgcn_readfirstlane(pn.y);      // (the cursor is inside the list: its entry is <= item)
            const long long st = ex_start[ul];
            const int32_t *list = p.ex_items + (((long long)__builtin_amdgcn_readfirstlane((int)(st >> 32)) << 32) |
                                                (unsigned)__builtin_amdgcn_readfirstlane((int)st));
            int pos = __builtin_amdgcn_readfirstlane(pn.x), next = INT_MAX;
            bool hit = false;
            do {
                const int at = pos + lane;
                const int v = list[at < n ? at : n - 1];
                const int w = at < n ? v : INT_MAX;
                int below = __popcll(__builtin_amdgcn_ballot_w64(w < item));   // (sorted: a prefix of the lanes)
                hit = __builtin_amdgcn_ballot_w64(w == item) != 0ull;
                if (hit && below < 63) ++below;       // (step over the entry that excludes this item: no candidate meets it again)
                pos += below;
                if (below < 64) {
                    next = __builtin_amdgcn_readlane(w, below);
                    break;
                }
            } while (pos < n);
            ex_at[ul].x = pos;
            ex_next[ul] = next;
            return hit;
        }
        return false;
    };
    // the tile's candidates go into their lists in ascending item order (lane order within the tile), so equal scores
    // keep the lower item id in front
    auto drain = [&](int r0, int r1, int i0, const f32x16 &acc, const unsigned long long (&mk)[16], unsigned long long okm)
                     __attribute__((always_inline)) {
        const unsigned ni0 = ~(unsigned)i0;           // ~(i0 + j) == ~i0 - j
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (r < r0 || r >= r1) continue;
            unsigned long long m = mk[r] & okm;
            while (m) {
                const int L = __builtin_ctzll(m);
                asm("s_bitset0_b64 %0, %1" : "+s"(m) : "s"(L));
#ifdef PMF_TOPK_STAMPS
                ++st_cand;
#endif
                const int hh = L >> 5;
                // (a row past the last query user never gets here: its threshold is +inf -- and if an infinite score did
                //  bring it here, the list it lands in exists in LDS and is never handed over)
                const int ul = (r & 3) + 8 * (r >> 2) + 4 * hh;
                if (EXCLUDE && excluded(ul, i0 + (L & 31))) continue;   // dropped: never in the list, never moves tau
                const unsigned vb = (unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(acc[r]), L);
#ifdef PMF_TOPK_PAD_SCALAR   // (diagnostic: what an extra scalar / vector instruction per candidate costs the launch --
#pragma unroll                // profiles/r03_topk_instruction_cost.log: about five cycles of SIMD time each, either kind)
                for (int pad = 0; pad < PMF_TOPK_PAD_SCALAR; ++pad) { int d_; asm volatile("s_mov_b32 %0, 0" : "=s"(d_)); }
#endif
#ifdef PMF_TOPK_PAD_VECTOR
#pragma unroll
                for (int pad = 0; pad < PMF_TOPK_PAD_VECTOR; ++pad) { int d_; asm volatile("v_mov_b32 %0, 0" : "=v"(d_)); }
#endif
                // (an earlier candidate of this tile may have raised the list's threshold past v: insert() re-checks)
                const unsigned nt = insert(ul, vb, ni0 - (unsigned)(L & 31));
                // tau[r] = nt in the half-wave (h == hh) that holds this user's row: one v_mov under a scalar EXEC
                asm volatile("s_mov_b64 exec, %[half]\n\t"
                             "v_mov_b32 %[t], %[nt]\n\t"
                             "s_mov_b64 exec, -1"
                             : [t] "+v"(tau[r])
                             : [half] "s"(0xffffffffull << (32 * hh)), [nt] "s"(nt));
            }
        }
    };
    const int slot = topk_wave_slot();
    auto slice_priority = [&](int stage_no) __attribute__((always_inline)) { topk_slice_priority(slot, stage_no); };
    auto rotate_priority = [&](int stage_no) __attribute__((always_inline)) {
        if ((stage_no & (PRIO_SLICE - 1)) == 0) slice_priority(stage_no);
    };
    auto tile = [&](auto TAIL, int i0, const f32x4 *rows, int stage_no) __attribute__((always_inline)) {
        f32x16 acc;
        unsigned long long mk[16], okm;
        const f32x4 *mine = rows + c * PQ + h;
        topk_mfma_tile<KH>(a, acc, [&](int t) __attribute__((always_inline)) { return mine[t / 2]; });
        scores(TAIL, i0, acc);
        // which half of the rows holds a candidate (the v_cmpx blocks' lane masks); a partial tile takes both
        unsigned long long m1 = 0ull, m2 = 0ull;
        if (!decltype(TAIL)::value && all_below(acc, m1, m2)) return;
        okm = decltype(TAIL)::value ? __builtin_amdgcn_ballot_w64(i0 + c < i_end) : ~0ull;
#ifdef PMF_TOPK_STAMPS
        const long long t_ = __builtin_amdgcn_s_memtime();
        ++st_tiles;
#endif
#ifdef PMF_TOPK_RANK_PRIORITY   // (experiment: rank at the top priority, then step back to the time slice's -- no gain)
        __builtin_amdgcn_s_setprio(3);
#endif
        if (m1 != ~0ull) {
            thresholds(0, 8, acc, mk);
            drain(0, 8, i0, acc, mk, okm);
        }
        if (m2 != ~0ull) {
            thresholds(8, 16, acc, mk);
            drain(8, 16, i0, acc, mk, okm);
        }
#ifdef PMF_TOPK_RANK_PRIORITY
        slice_priority(stage_no);
#endif
#ifdef PMF_TOPK_STAMPS
        st_drain += __builtin_amdgcn_s_memtime() - t_;
#endif
    };
    auto tiles = [&](auto TAIL, int i0, const f32x4 *rows, int stage_no) __attribute__((always_inline)) {
        if (!active) return;                          // a wave without users only stages item rows
        tile(TAIL, i0, rows, stage_no);
        if (ST == 64 && (!decltype(TAIL)::value || i0 + 32 < i_end)) tile(TAIL, i0 + 32, rows + 32 * PQ, stage_no);
    };
    // the stage in g[] becomes the one the block multiplies next (every wave runs the same stages: the barriers)
    int buf = 0;
    auto publish = [&]() __attribute__((always_inline)) {
        if (nbuf == 2) {
            stash(buf ^ 1);                           // last read there: the stage before this one, behind the barrier
            barrier();
            buf ^= 1;
        } else {                                      // one buffer (long lists: the LDS saved keeps another block resident)
            barrier();                                // every wave has read this stage
            stash(0);
            barrier();
        }
    };
    // The loop proper has no case to tell apart: it runs while the stage after the current one is a full one; the
    // segment's last full stage and its partial one (rows past the end re-read the last row and are never ranked) follow.
    const int n_full = (i_end - i_begin) / ST;
    const bool has_tail = (i_end - i_begin) % ST != 0;
    const std::integral_constant<bool, false> FULL;
    const std::integral_constant<bool, true> PARTIAL;
    int stage_no = 0, i0 = i_begin;
    if (n_full > 0) fetch_full(); else fetch_tail(i_begin);            // (segments are never empty)
    stash(0);
    __syncthreads();
    const int n_steady = n_full > 0 ? n_full - 1 : 0;
    for (int s0 = 0; s0 < n_steady; s0 += PRIO_SLICE) {               // (one priority slice per trip: nothing to test per stage)
        slice_priority(s0);
        const int s1 = s0 + PRIO_SLICE < n_steady ? s0 + PRIO_SLICE : n_steady;
        for (int st = s0; st < s1; ++st, i0 += ST) {
            fetch_full();
            tiles(FULL, i0, stage + (size_t)buf * ST * PQ, st);
            publish();
        }
    }
    stage_no = n_steady;
    if (n_full > 0) {
        rotate_priority(stage_no);
        if (has_tail) fetch_tail(i0 + ST);
        tiles(FULL, i0, stage + (size_t)buf * ST * PQ, stage_no);
        if (has_tail) publish();
        ++stage_no;
        i0 += ST;
    }
    if (has_tail) tiles(PARTIAL, i0, stage + (size_t)buf * ST * PQ, stage_no);
    barrier();                                        // the next user tile's first stage goes where this one is read
    // hand the lists over: final result when the item range was not segmented, else this segment's candidates
    for (int e = lane; e < 32 * k; e += 64) {
        const int ul = e / k, t = e % k;
        const int qq = q0 + ul;
        if (qq >= p.nq) continue;
        const unsigned long long ent = le[e];
        const float v = topk_key_score((unsigned)(ent >> 32));
        const int idx = (unsigned)ent == 0u ? 0x7fffffff : (int)~(unsigned)ent;
        if (nseg == 1) {
            out_items[(int64_t)qq * k + t] = idx == 0x7fffffff ? -1 : idx;
            out_scores[(int64_t)qq * k + t] = idx == 0x7fffffff ? 0.0 : (double)v;
        } else {
            cand_val[((int64_t)qq * nseg + seg) * k + t] = v;
            cand_idx[((int64_t)qq * nseg + seg) * k + t] = idx;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // the lists are re-initialised for the next user tile
    __builtin_amdgcn_wave_barrier();
#ifdef PMF_TOPK_STAMPS
    if (lane == 0 && seg == 0) {
        long long *o = g_topk_stamps + (size_t)((ut * 4 + wave) & 16383) * 8;
        o[0] = st_begin;
        o[1] = __builtin_amdgcn_s_memrealtime();
        o[2] = gridDim.x;
        o[3] = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (31 << 11));   // XCC_ID
        o[4] = st_drain;
        o[5] = st_barrier;
        o[6] = st_cand;
        o[7] = st_tiles;
    }
#endif
    }   // user tiles
    __builtin_amdgcn_s_setprio(0);
}

// k best of a user's nseg * k segment candidates, (value desc, item id asc); one wavefront per user
__global__ __launch_bounds__(256) void topk_merge_kernel(const float *cand_val, const int32_t *cand_idx, int nq, int n_cand,
                                                         int k, int32_t *out_items, double *out_scores) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + wave;
    if (q >= nq) return;
    const float *cv = cand_val + (int64_t)q * n_cand;
    const int32_t *ci = cand_idx + (int64_t)q * n_cand;
    topk_select_passes<float>(lane, k, out_items + (int64_t)q * k, out_scores + (int64_t)q * k, [&](auto visit) __attribute__((always_inline)) {
        for (int e = lane; e < n_cand; e += 64) {
            const float v = cv[e];
            const int i = ci[e];
            if (i != 0x7fffffff) visit(v, i);         // (0x7fffffff: an unused list slot)
        }
    });
}

// query rows of one round of the fused top-k and of pmf_rank_items (ctx->topk_query_rows: PMF_TOPK_QUERY_ROWS, for the tests)
static int64_t topk_round_rows(const pmf_ctx *ctx) { return ctx->topk_query_rows > 0 ? ctx->topk_query_rows : (int64_t)1 << 20; }

// Segments of the item range of a fused scan (gridDim.y).  Few query rows: cut the range so that the grid still has a few
// thousand wavefronts.  Returns the number of segments; *seg_items = items per segment, a multiple of 32.
static int topk_segments(int64_t n_rows, int64_t I, int64_t *seg_items) {
    const int64_t waves = (n_rows + 31) / 32;
    int nseg = (int)std::min<int64_t>(64, std::max<int64_t>(1, 4096 / waves));
    nseg = (int)std::min<int64_t>(nseg, std::max<int64_t>(1, I / 2048));
    *seg_items = ((I + nseg - 1) / nseg + 31) / 32 * 32;
    return (int)((I + *seg_items - 1) / *seg_items);
}

// The fused scans are persistent in x: at most as many blocks as are resident at once (per_cu, the occupancy query, x CUs),
// each walking its share of the 128-user tiles; with a segmented item range (few users) every (tile, segment) keeps its own
// block.
static hipError_t topk_persistent_grid(const pmf_ctx *ctx, int per_cu, dim3 *grid) {
    int cus = 0;
    const hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
    if (e != hipSuccess || grid->y != 1) return e;
    unsigned resident = (unsigned)std::max(1, per_cu) * (unsigned)std::max(1, cus);
    if (ctx->topk_max_blocks > 0) resident = std::min(resident, (unsigned)ctx->topk_max_blocks);   // (tests: few blocks, many tiles each)
    if (grid->x > resident) grid->x = resident;
    return hipSuccess;
}

// (P: TopkParams, or TopkExcludeParams for the excluding kernels, whose lists are followed by the cursor words: the
//  occupancy queries below are asked about the kernel and the LDS size that are launched)
template <int KH, int MODE, typename P>
static hipError_t launch_topk_fused_mode(pmf_ctx *ctx, const P &p, dim3 grid, const float *fu,
                                         const float *fi, const float *cu, const float *ci, int k, int64_t seg_items,
                                         int nseg, float *cand_val, int32_t *cand_idx, int32_t *out_items,
                                         double *out_scores) {
    constexpr bool EXCLUDE = std::is_same<P, TopkExcludeParams>::value;
    const size_t list_bytes = topk_list_bytes(k) + (EXCLUDE ? TOPK_EXCLUDE_LDS_BYTES : 0);
    // One stage buffer or two.  Two (one barrier per stage) is the faster loop at equal residency, but the lists take
    // 1 KB of LDS per k and block: from k = 23 at K = 64 the second buffer costs the CU a resident block
    // (profiles/r03_topk_long_lists.jsonl: 34.3 -> 30.8 ms at k = 24, 72.9 -> 49.3 ms at k = 64).  Take one buffer where
    // it keeps more blocks on the CU.  (ctx->topk_stage_buffers pins it: PMF_TOPK_STAGE_BUFFERS, for the probes.)
    const void *fn2 = (const void *)topk_fused_kernel<KH, MODE, 2, EXCLUDE>, *fn1 = (const void *)topk_fused_kernel<KH, MODE, 1, EXCLUDE>;
    const size_t smem2 = 2 * TopkStage<KH>::buffer_bytes + list_bytes, smem1 = TopkStage<KH>::buffer_bytes + list_bytes;
    if (smem2 > (64u << 10)) {   // long lists at K > 64: past the default dynamic-LDS limit
        hipError_t e = hipFuncSetAttribute(fn2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem2);
        if (e == hipSuccess) e = hipFuncSetAttribute(fn1, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem2);
        if (e != hipSuccess) return e;
    }
    int per_cu2 = 0, per_cu1 = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu2, fn2, 256, smem2);
    if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu1, fn1, 256, smem1);
    if (e != hipSuccess) return e;
    int nbuf = per_cu1 > per_cu2 ? 1 : 2;
    if (ctx->topk_stage_buffers == 1 || ctx->topk_stage_buffers == 2) nbuf = ctx->topk_stage_buffers;
    const size_t smem = nbuf == 2 ? smem2 : smem1;
    if ((e = topk_persistent_grid(ctx, nbuf == 2 ? per_cu2 : per_cu1, &grid)) != hipSuccess) return e;
    if (nbuf == 2)
        hipLaunchKernelGGL((topk_fused_kernel<KH, MODE, 2, EXCLUDE>), grid, dim3(256), smem, ctx->stream, p, fu, fi, cu, ci, k, seg_items,
                           nseg, cand_val, cand_idx, out_items, out_scores);
    else
        hipLaunchKernelGGL((topk_fused_kernel<KH, MODE, 1, EXCLUDE>), grid, dim3(256), smem, ctx->stream, p, fu, fi, cu, ci, k, seg_items,
                           nseg, cand_val, cand_idx, out_items, out_scores);
    return hipSuccess;
}

// ---------------------------------------------------------------------------
// what a scan reads: the query source
// ---------------------------------------------------------------------------
// The A side (the query rows: a table addressed by the ids in p.users, and their bias / scale), the B side (the
// candidates: all n_cand rows of a table, and theirs) and the exclusion CSR, which is indexed by the A ids.  The item
// calls (pmf_topk_items*, pmf_rank_items) pass the context's USER arrays against its ITEM arrays with the callers' user
// ids; the query calls (pmf_topk_query, pmf_rank_query) stage the rows of every round into a dense table first.
struct QueryStage;
struct TopkSource {
    const void *fa = nullptr, *ca = nullptr;   // A: FACTOR-shaped table [.. x kpad] and coefficients (null under score 0); context dtype
    const void *fb = nullptr, *cb = nullptr;   // B: the same for the candidates
    int64_t n_cand = 0;                        // rows of the B table
    const int64_t *ex_ptr = nullptr;           // device: ex_ids[ex_ptr[a] .. ex_ptr[a + 1]) are no candidates of A id a (ascending, distinct), or null
    const int32_t *ex_ids = nullptr;
    const int32_t *ids = nullptr;              // host: the A id of the caller's row n -- or null with `staged`:
    const QueryStage *staged = nullptr;        // the rows are staged per round, and row n of a round that begins at row n0 has A id n - n0
};
// the source of one round, rows [row0, row0 + n): `src` itself, or with fa / ca / ex_ptr those of the rows staged here
static int topk_round_source(pmf_ctx *ctx, const TopkSource &src, int64_t row0, int64_t n, TopkSource *round);
// ... and the round's A ids on the device, one per row
static int topk_round_ids(pmf_ctx *ctx, const TopkSource &src, int64_t row0, int n, int32_t *d_ids);

// The rounds of both top-k paths: per round of at most Q query rows its source and A ids (d_users), launch(p, r, nq) --
// the path's kernels over the round's parameters `p` and source `r`, timed as PMF_KERNEL_TOPK -- and the nq x k results
// from d_out_items / d_out_scores to the caller's arrays.
template <typename Launch>
static int topk_rounds(pmf_ctx *ctx, const TopkSource &src, int64_t n_query, int64_t Q, int k, int32_t *d_users,
                       int32_t *d_out_items, double *d_out_scores, int32_t *out_items, double *out_scores, Launch &&launch) {
    int rc;
    for (int64_t at = 0; at < n_query; at += Q) {
        const int nq = (int)std::min<int64_t>(Q, n_query - at);
        TopkSource r;
        if ((rc = topk_round_source(ctx, src, at, nq, &r)) || (rc = topk_round_ids(ctx, src, at, nq, d_users))) return rc;
        TopkExcludeParams p;
        p.users = d_users;
        p.nq = nq;
        p.n_items = src.n_cand;
        p.K = ctx->K;
        p.kpad = ctx->kpad;
        p.ex_ptr = r.ex_ptr;
        p.ex_items = r.ex_ids;
        {
            PmfProfScope prof(ctx, PMF_KERNEL_TOPK);
            if ((rc = launch(p, r, nq))) return rc;
        }
        PMF_HIP_CHECK(hipGetLastError());
        PMF_HIP_CHECK(hipMemcpyAsync(out_items + at * k, d_out_items, (size_t)nq * k * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        PMF_HIP_CHECK(hipMemcpyAsync(out_scores + at * k, d_out_scores, (size_t)nq * k * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        PMF_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    return PMF_OK;
}

// fp32, Kpad <= 128, k <= 64
// (cu / ci / the exclusion lists: src's, per round)
static int run_topk_fused(pmf_ctx *ctx, const TopkSource &src, int64_t n_query, int k, int mode, int32_t *out_items,
                          double *out_scores) {
    const int64_t Q = std::min<int64_t>(n_query, topk_round_rows(ctx));   // query users per launch
    int64_t seg_items;
    const int nseg = topk_segments(Q, src.n_cand, &seg_items);
    const size_t n_cand = nseg > 1 ? (size_t)nseg * k : 0;
    PmfLayout lay;
    const auto scores_at = lay.add<double>((size_t)Q * k);
    const auto items_at = lay.add<int32_t>((size_t)Q * k), users_at = lay.add<int32_t>((size_t)Q);
    const auto cv_at = lay.add<float>((size_t)Q * n_cand);
    const auto ci_at = lay.add<int32_t>((size_t)Q * n_cand);
    if (int rc = pmf_ensure_scratch(ctx, lay.bytes())) return rc;
    void *base = ctx->d_scratch.as();
    double *d_out_scores = scores_at.at(base);
    int32_t *d_out_items = items_at.at(base), *d_ci = ci_at.at(base);
    float *d_cv = cv_at.at(base);
    return topk_rounds(ctx, src, n_query, Q, k, users_at.at(base), d_out_items, d_out_scores, out_items, out_scores,
                       [&](const TopkExcludeParams &p, const TopkSource &r, int nq) {
        const float *fu = static_cast<const float *>(r.fa), *fi = static_cast<const float *>(r.fb);
        const float *cu = static_cast<const float *>(r.ca), *ci = static_cast<const float *>(r.cb);
        dim3 grid((unsigned)((nq + 127) / 128), (unsigned)nseg);
        // the instantiation for the K class KH and the bias mode
        PMF_HIP_CHECK(pmf_with_pow2<8>(ctx->kpad / 2, [&](auto kh) {   // KH: kpad / 2 rounded up to 8, 16, 32 or 64
            return pmf_with_predict_mode(mode, [&](auto m) {
                if (p.ex_ptr)
                    return launch_topk_fused_mode<kh, m>(ctx, p, grid, fu, fi, cu, ci, k, seg_items, nseg, d_cv, d_ci,
                                                         d_out_items, d_out_scores);
                return launch_topk_fused_mode<kh, m>(ctx, static_cast<const TopkParams &>(p), grid, fu, fi, cu, ci, k, seg_items,
                                                     nseg, d_cv, d_ci, d_out_items, d_out_scores);
            });
        }));
        if (nseg > 1)
            hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, ctx->stream, d_cv, d_ci, nq,
                               (int)n_cand, k, d_out_items, d_out_scores);
        return PMF_OK;
    });
}

// (arguments, arrays and flag are checked: topk_items_impl)
template <typename T>
static int run_topk(pmf_ctx *ctx, const TopkSource &src, int64_t n_query, int k, int use_bias, int32_t *out_items,
                    double *out_scores) {
    const int64_t I = src.n_cand;
    if constexpr (std::is_same<T, float>::value) {
        if (ctx->kpad <= 128 && k <= 64 && I <= (int64_t)INT32_MAX - 64 && !ctx->topk_two_phase)   // (the fused scan counts items in ints)
            return run_topk_fused(ctx, src, n_query, k, use_bias, out_items, out_scores);
    }
    // batch size: scores buffer of at most ~512 MB
    int64_t Q = std::max<int64_t>(32, (512ll << 20) / (I * (int64_t)sizeof(T)));
    Q = std::min<int64_t>(Q / 32 * 32, (n_query + 31) / 32 * 32);
    if (ctx->topk_query_rows > 0) Q = std::min(Q, ctx->topk_query_rows);
    PmfLayout lay;
    const auto all_at = lay.add<T>((size_t)Q * I);
    const auto scores_at = lay.add<double>((size_t)Q * k);
    const auto items_at = lay.add<int32_t>((size_t)Q * k), users_at = lay.add<int32_t>((size_t)Q);
    if (int rc = pmf_ensure_scratch(ctx, lay.bytes())) return rc;
    void *base = ctx->d_scratch.as();
    T *d_scores = all_at.at(base);
    double *d_out_scores = scores_at.at(base);
    int32_t *d_out_items = items_at.at(base);
    return topk_rounds(ctx, src, n_query, Q, k, users_at.at(base), d_out_items, d_out_scores, out_items, out_scores,
                       [&](const TopkExcludeParams &p, const TopkSource &r, int nq) {
        const T *fu = static_cast<const T *>(r.fa), *fi = static_cast<const T *>(r.fb);
        const T *bu = static_cast<const T *>(r.ca), *bi = static_cast<const T *>(r.cb);
        if constexpr (std::is_same<T, float>::value) {
            dim3 grid((unsigned)((nq + 31) / 32), (unsigned)((I + 127) / 128));
            hipLaunchKernelGGL(topk_scores_f32_kernel, grid, dim3(256), 0, ctx->stream, p, fu, fi, bu, bi, use_bias, d_scores);
        } else {
            const int64_t total = (int64_t)nq * I;
            hipLaunchKernelGGL(topk_scores_f64_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 65535)),
                               dim3(256), 0, ctx->stream, p, fu, fi, bu, bi, use_bias, d_scores);
        }
        if (p.ex_ptr)   // excluded pairs score NaN from here on: the select never ranks them
            hipLaunchKernelGGL((topk_exclude_scores_kernel<T>), dim3((unsigned)std::min(nq, 65535)), dim3(256), 0, ctx->stream,
                               p, d_scores);
        hipLaunchKernelGGL((topk_select_kernel<T>), dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, ctx->stream,
                           d_scores, nq, I, k, d_out_items, d_out_scores);
        return PMF_OK;
    });
}

// the source of the item calls: the context's users (by the caller's ids) against its items under `mode`, with the users'
// distinct training items excluded (built: pmf_index_distinct) or nothing
static TopkSource topk_items_source(const pmf_ctx *ctx, const int32_t *user_ids, int mode, bool exclude_train) {
    const int carr = mode == PMF_PREDICT_SCALE ? PMF_ARR_SCALE : PMF_ARR_BIAS;
    TopkSource src;
    src.fa = ctx->arr[PMF_SIDE_USER][PMF_ARR_FACTOR].as();
    src.fb = ctx->arr[PMF_SIDE_ITEM][PMF_ARR_FACTOR].as();
    src.ca = mode ? ctx->arr[PMF_SIDE_USER][carr].as() : nullptr;
    src.cb = mode ? ctx->arr[PMF_SIDE_ITEM][carr].as() : nullptr;
    src.n_cand = ctx->rows[PMF_SIDE_ITEM];
    if (exclude_train) {
        src.ex_ptr = ctx->index[PMF_SIDE_USER].d_distinct_ptr.as<const int64_t>();
        src.ex_ids = ctx->index[PMF_SIDE_USER].d_distinct.as<const int32_t>();
    }
    src.ids = user_ids;
    return src;
}

// pmf_topk_items (`fn` names the entry point in a refusal), and with `exclude_train` pmf_topk_items_excluding
static int topk_items_impl(const char *fn, pmf_ctx *ctx, int64_t n_query, const int32_t *user_ids, int k, int use_bias,
                           int exclude_train, int32_t *out_items, double *out_scores) {
    PMF_REQUIRE(ctx != nullptr, PMF_EINVAL, "%s: null context", fn);
    PMF_REQUIRE(n_query >= 0, PMF_EINVAL, "%s: negative n_query", fn);
    if (n_query == 0) return PMF_OK;
    PMF_REQUIRE(user_ids && out_items && out_scores, PMF_EINVAL, "%s: null argument", fn);
    PMF_REQUIRE(k >= 1 && k <= 1024 && k <= ctx->rows[PMF_SIDE_ITEM], PMF_ERANGE, "%s: k=%d outside [1, min(1024, n_items)]", fn, k);
    if (int rc = pmf_check_ids(user_ids, n_query, ctx->rows[PMF_SIDE_USER], fn, "user id")) return rc;
    // (every refusal comes before the first write: an argument error leaves the outputs and the context as they were)
    int rc;
    if ((rc = pmf_require_array(ctx, PMF_SIDE_USER, PMF_ARR_FACTOR, fn))) return rc;
    if ((rc = pmf_require_array(ctx, PMF_SIDE_ITEM, PMF_ARR_FACTOR, fn))) return rc;
    PMF_REQUIRE(use_bias == 0 || use_bias == PMF_PREDICT_BIAS || use_bias == PMF_PREDICT_SCALE, PMF_EINVAL,
                "%s: use_bias must be 0, PMF_PREDICT_BIAS or PMF_PREDICT_SCALE (got %d)", fn, use_bias);
    if (use_bias) {
        const int carr = use_bias == PMF_PREDICT_SCALE ? PMF_ARR_SCALE : PMF_ARR_BIAS;
        if ((rc = pmf_require_array(ctx, PMF_SIDE_USER, carr, fn))) return rc;
        if ((rc = pmf_require_array(ctx, PMF_SIDE_ITEM, carr, fn))) return rc;
    }
    PMF_REQUIRE(!exclude_train || ctx->index[PMF_SIDE_USER].d_ptr, PMF_EINVAL,
                "%s: exclude_train needs the training ratings (pmf_ctx_set_ratings); the context holds none", fn);
    PMF_HIP_CHECK(hipSetDevice(ctx->device));
    if (exclude_train && (rc = pmf_index_distinct(ctx, PMF_SIDE_USER))) return rc;   // (built once per set of ratings)
    const TopkSource src = topk_items_source(ctx, user_ids, use_bias, exclude_train != 0);
    return pmf_with_dtype(ctx, [&](auto t) { return run_topk<decltype(t)>(ctx, src, n_query, k, use_bias, out_items, out_scores); });
}

extern "C" int pmf_topk_items(pmf_ctx *ctx, int64_t n_query, const int32_t *user_ids, int k, int use_bias,
                              int32_t *out_items, double *out_scores) {
    return topk_items_impl("pmf_topk_items", ctx, n_query, user_ids, k, use_bias, 0, out_items, out_scores);
}

extern "C" int pmf_topk_items_excluding(pmf_ctx *ctx, int64_t n_query, const int32_t *user_ids, int k, int use_bias,
                                        int exclude_train, int32_t *out_items, double *out_scores) {
    return pmf_no_throw("pmf_topk_items_excluding", [&] {
        return topk_items_impl("pmf_topk_items_excluding", ctx, n_query, user_ids, k, use_bias, exclude_train, out_items, out_scores);
    });
}

// ---------------------------------------------------------------------------
// pmf_rank_items: the rank of held-out items among a user's candidates
// ---------------------------------------------------------------------------
// A QUERY ROW is a user with up to RANK_SLOTS target items (the host cuts a user with more targets into several).  Per
// query row the device keeps RANK_STRIDE int32 counters: per slot the number of items that rank before the target, the
// number of NaN scores, the number of excluded (training) items with a non-NaN score, and a bit mask of the slots whose
// own score is NaN.  rank = counter, candidates = n_items - NaN scores - excluded.
//
// fp32, Kpad <= 128 -- three launches, all of which produce a score with the SAME arithmetic, that of topk_fused_kernel:
// topk_load_a(), topk_mfma_tile(), then rank_score().  Exact ties are the normal case here (every item without ratings
// keeps its prior row), so a threshold that differed from the scan's score of the same item in the last bit would move a
// rank by the size of the tie group.
//   rank_rows_kernel<.., false>  thresholds: one wavefront per query row, all 32 A rows the user's, B column t = the slot's
//                                target item -> the target's own score
//   rank_fused_kernel            the scan of topk_fused_kernel (same staging, same tiles); its epilogue counts, per slot,
//                                the scores above the threshold (v_cmp + v_addc) and notes equal ones; only a tile that
//                                holds a tie or a NaN takes the second pass that breaks ties by item id and counts NaNs
//   rank_rows_kernel<.., true>   exclusion: one wavefront per query row, B columns = 32 of the user's distinct training
//                                items at a time; what the scan counted for them is subtracted
// fp64 contexts and Kpad > 128: rank_generic_kernel, fma chains, one wavefront per query row.
#define RANK_SLOTS 4
#define RANK_NAN (RANK_SLOTS)          // counter: NaN scores
#define RANK_EXCL (RANK_SLOTS + 1)     // counter: excluded items with a non-NaN score
#define RANK_MASK (RANK_SLOTS + 2)     // bit t: the score of slot t's target is NaN
#define RANK_STRIDE (RANK_SLOTS + 3)

// does a competitor (score s, item j) rank before the target (score th, item tg)?
template <typename S>
__device__ __forceinline__ bool rank_beats(S s, int j, S th, int tg) {
    return (s > th || (s == th && j < tg)) && j != tg;
}

// sum over the 32 lanes of this lane's half-wave; every lane of the half receives it
__device__ __forceinline__ int rank_half_sum(int x) {
    x += __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x141, 0xF, 0xF, false);
    x += __builtin_amdgcn_update_dpp(0, x, 0x140, 0xF, 0xF, false);
    return x + __shfl_xor(x, 16, 64);
}

struct RankParams {
    const int32_t *tgt;   // [nq][RANK_SLOTS] target item of a slot, -1: unused
    void *th;             // [nq][RANK_SLOTS] the targets' own scores (NaN in an unused slot); context dtype
    int32_t *cnt;         // [nq][RANK_STRIDE]
    const int64_t *ex_ptr;    // the users' distinct training items (exclusion), or null
    const int32_t *ex_items;
};

// One wavefront per query row.  EXCLUDE = false: the targets' scores.  EXCLUDE = true: the training items' scores, and
// what the scan counted for them taken off the counters.  (1 / 32 of the MFMA's rows is used: n_targets + n_ratings / 32
// tiles per user against n_items / 32 per 32 users in the scan.)
template <int KH, int MODE, bool EXCLUDE>
__global__ __launch_bounds__(256) void rank_rows_kernel(TopkParams p, RankParams rp, const float *fu, const float *fi,
                                                        const float *cu, const float *ci) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int h = lane >> 5, c = lane & 31;
    const int q = blockIdx.x * 4 + wave;
    if (q >= p.nq) return;
    const int kpad = p.kpad, last_piece = kpad / 4 - 1;
    const int user = p.users[q];
    float a[KH];
#pragma unroll
    for (int t = 0; t < KH; t += 4) {
        const float4 v = topk_a_piece(fu, user, kpad, h, t);
        a[t] = v.x; a[t + 1] = v.y; a[t + 2] = v.z; a[t + 3] = v.w;
    }
    const float ucst = MODE != 0 ? cu[user] : 0.f;
    // the user's score of this lane's column: item `item` (< 0: none, the result is not used)
    auto column_score = [&](int item) __attribute__((always_inline)) -> float {
        const float *row = fi + (int64_t)(item < 0 ? 0 : item) * kpad;
        f32x16 acc;
        topk_mfma_tile<KH>(a, acc, [&](int t) __attribute__((always_inline)) {
            const int pc = t / 2 + h;
            return *reinterpret_cast<const f32x4 *>(row + 4 * (pc < last_piece ? pc : last_piece));
        });
        const float ccst = (MODE != 0 && item >= 0) ? ci[item] : 0.f;
        return rank_score<MODE>(acc[0], ucst, ccst);   // (every row of the tile is this user's)
    };
    if (!EXCLUDE) {
        const int item = c < RANK_SLOTS ? rp.tgt[(int64_t)q * RANK_SLOTS + c] : -1;
        const float s = column_score(item);
        const unsigned long long nan = __builtin_amdgcn_ballot_w64(item >= 0 && s != s);
        if (h == 0 && c < RANK_SLOTS) static_cast<float *>(rp.th)[(int64_t)q * RANK_SLOTS + c] = item >= 0 ? s : __builtin_nanf("");
        if (lane == 0) rp.cnt[(int64_t)q * RANK_STRIDE + RANK_MASK] = (int)(nan & ((1u << RANK_SLOTS) - 1u));
    } else {
        float th[RANK_SLOTS];
        int tg[RANK_SLOTS], sub[RANK_SLOTS], n_ok = 0;
#pragma unroll
        for (int t = 0; t < RANK_SLOTS; ++t) {
            th[t] = static_cast<const float *>(rp.th)[(int64_t)q * RANK_SLOTS + t];
            tg[t] = rp.tgt[(int64_t)q * RANK_SLOTS + t];
            sub[t] = 0;
        }
        const int64_t end = rp.ex_ptr[user + 1];
        for (int64_t base = rp.ex_ptr[user]; base < end; base += 32) {
            const int item = base + c < end ? rp.ex_items[base + c] : -1;   // (both half-waves: each holds half of the column's k)
            const float s = column_score(item);
            const bool mine = h == 0 && item >= 0;                          // ... and one of them counts it
            n_ok += __popcll(__builtin_amdgcn_ballot_w64(mine && s == s));
#pragma unroll
            for (int t = 0; t < RANK_SLOTS; ++t)
                sub[t] += __popcll(__builtin_amdgcn_ballot_w64(mine && rank_beats(s, item, th[t], tg[t])));
        }
        if (lane == 0) {
#pragma unroll
            for (int t = 0; t < RANK_SLOTS; ++t) rp.cnt[(int64_t)q * RANK_STRIDE + t] -= sub[t];
            rp.cnt[(int64_t)q * RANK_STRIDE + RANK_EXCL] = n_ok;
        }
    }
}

// The scan.  Two stage buffers, persistent blocks in x and item segments in y, as in topk_fused_kernel; the score comes
// from the functions that kernel uses, while the staging lambdas, publish and the stage loop are a COPY of its code (the
// comment above that kernel says why, and what the copy leaves out): a change to either copy belongs in the other too.
// TS = target slots held in registers (1 when no query row of the call has more than one target).
// Per accumulator register r and slot t: one threshold, one counter.  Segments add their counts with integer atomics.
// (waves per SIMD the register allocation leaves room for: the thresholds and counters take 32 TS registers, the A rows
//  KH, the bias / scale modes 16 more -- at K = 64 those fit one step lower than the plain score does)
template <int KH, int MODE, int TS>
__global__ __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(KH < 32 || (KH == 32 && MODE == 0) ? (TS == 1 ? (MODE == 0 ? 4 : 3) : 2) : (TS == 1 ? 2 : 1))))
void rank_fused_kernel(TopkParams p, RankParams rp, const float *fu, const float *fi,
                                                         const float *cu, const float *ci, int64_t seg_items) {
    using S = TopkStage<KH>;
    constexpr int ST = S::ST, PR = S::PR, PQ = S::PQ, LPT = S::LPT;
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int h = lane >> 5, c = lane & 31;
    f32x4 *stage = reinterpret_cast<f32x4 *>(smem_raw);                                          // [2][ST][PQ]
    const int i_begin = (int)((int64_t)blockIdx.y * seg_items);
    const int i_end = (int)((int64_t)i_begin + seg_items < p.n_items ? (int64_t)i_begin + seg_items : p.n_items);
    const int kpad = p.kpad;
    const float *th_in = static_cast<const float *>(rp.th);
    const int slot = topk_wave_slot();
    auto slice_priority = [&](int stage_no) __attribute__((always_inline)) { topk_slice_priority(slot, stage_no); };

    const int n_user_tiles = (p.nq + 127) / 128;
    for (int ut = blockIdx.x; ut < n_user_tiles; ut += gridDim.x) {
    const int q0 = (ut * 4 + wave) * 32;
    const bool active = q0 < p.nq;                     // a wave without query rows still stages item rows
    const int user = (q0 + c < p.nq) ? p.users[q0 + c] : -1;
    float a[KH];
#pragma unroll
    for (int t = 0; t < KH; t += 4) {
        const float4 v = topk_a_piece(fu, user, kpad, h, t);
        a[t] = v.x; a[t + 1] = v.y; a[t + 2] = v.z; a[t + 3] = v.w;
    }
    // per accumulator register r: the query row (r & 3) + 8 (r >> 2) + 4 h, its bias / scale, its thresholds and counters
    // (a NaN threshold -- an unused slot, a row past the last query, a NaN target -- compares false both ways)
    float ucst[16], th[TS][16];
    int cnt[TS][16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int qq = q0 + (r & 3) + 8 * (r >> 2) + 4 * h;
        ucst[r] = 0.f;
        if (MODE != 0 && qq < p.nq) ucst[r] = cu[p.users[qq]];
#pragma unroll
        for (int t = 0; t < TS; ++t) {
            th[t][r] = qq < p.nq ? th_in[(int64_t)qq * RANK_SLOTS + t] : __builtin_nanf("");
            cnt[t][r] = 0;
        }
    }

    // ---- staging: as in topk_fused_kernel -------------------------------------------------------------------------
    f32x4 g[LPT];
    const int last_piece = kpad / 4 - 1;
    const char *next_stage = reinterpret_cast<const char *>(fi + (int64_t)i_begin * kpad);
    const unsigned stage_bytes = (unsigned)ST * kpad * 4;
    unsigned goff[LPT];
#pragma unroll
    for (int j = 0; j < LPT; ++j) {
        const int idx = j * 256 + (int)threadIdx.x;
        const int r = idx / PR, pc = idx % PR;
        goff[j] = ((unsigned)r * kpad + 4u * (pc < last_piece ? pc : last_piece)) * 4u;
    }
    auto fetch_full = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < LPT; ++j) {
            unsigned off = goff[j];
            asm volatile("" : "+v"(off));             // (SGPR base + 32-bit VGPR offset)
            g[j] = *reinterpret_cast<const f32x4 *>(next_stage + off);
        }
        next_stage += stage_bytes;
    };
    auto fetch_tail = [&](int i0) __attribute__((always_inline)) {    // the segment's last, partial stage: rows past the end re-read the last row
        int tid = (int)threadIdx.x;
        asm volatile("" : "+v"(tid));                 // (once per segment: its addresses are formed here, not kept in registers)
#pragma unroll
        for (int j = 0; j < LPT; ++j) {
            const int idx = j * 256 + tid;
            const int r = idx / PR, pc = idx % PR;
            const int it = i0 + r < i_end ? i0 + r : i_end - 1;
            g[j] = *reinterpret_cast<const f32x4 *>(fi + (int64_t)it * kpad + 4 * (pc < last_piece ? pc : last_piece));
        }
    };
    auto stash = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < LPT; ++j) {
            const int idx = j * 256 + (int)threadIdx.x;
            stage[(size_t)buf * ST * PQ + (idx / PR) * PQ + idx % PR] = g[j];
        }
    };
    // ---- one 32-item tile ----------------------------------------------------------------------------------------
    auto tile = [&](auto TAIL, int i0, const f32x4 *rows) __attribute__((always_inline)) {
        f32x16 acc;
        const f32x4 *mine = rows + c * PQ + h;
        topk_mfma_tile<KH>(a, acc, [&](int t) __attribute__((always_inline)) { return mine[t / 2]; });
        const int it = i0 + c;
        const bool in_range = !decltype(TAIL)::value || it < i_end;
        if (MODE != 0) {
            const float ccst = in_range ? ci[it] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = rank_score<MODE>(acc[r], ucst[r], ccst);
        }
        if (decltype(TAIL)::value) {
            // a column past the segment's end scores -inf: above no threshold, no NaN, and equal to a -inf threshold only
            // with an item id above every target's
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = in_range ? acc[r] : TOPK_NEG_INF;
        }
        // first pass: what almost every tile needs -- scores above a threshold are counted, equal ones and NaNs noted
        unsigned long long special = 0ull;
#pragma unroll
        for (int t = 0; t < TS; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                cnt[t][r] += acc[r] > th[t][r] ? 1 : 0;
                special |= __builtin_amdgcn_ballot_w64(acc[r] == th[t][r]);
            }
#pragma unroll
        for (int r = 0; r < 16; r += 2) special |= __builtin_amdgcn_ballot_w64(__builtin_isunordered(acc[r], acc[r + 1]));
        if (special == 0ull) return;
        // second pass (rare): ties go to the lower item id -- the target itself is not its own competitor -- and NaN
        // scores are counted.  (The empty asm makes the compiler compare again here instead of keeping the first pass's
        // 16 TS lane masks alive across the branch, which it can only do by spilling scalars in the loop.)
        // (this lane's rows are q0 + 4 h + a constant per register: one pointer each, immediate offsets -- formed here, behind
        //  an empty asm, so that they hold no registers in the loop)
        int first_row = q0 + 4 * h;
        asm volatile("" : "+v"(first_row));
        const int32_t *tgt_lane = rp.tgt + (int64_t)first_row * RANK_SLOTS;
        int32_t *cnt_lane = rp.cnt + (int64_t)first_row * RANK_STRIDE;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = (r & 3) + 8 * (r >> 2);
            float s = acc[r];
            asm volatile("" : "+v"(s));
            const int nn = rank_half_sum(s != s ? 1 : 0);
            if (c == 0 && nn && first_row + row < p.nq)   // (a NaN item row scores NaN in the rows past the last query too)
                atomicAdd(cnt_lane + row * RANK_STRIDE + RANK_NAN, nn);
#pragma unroll
            for (int t = 0; t < TS; ++t)
                if (in_range && s == th[t][r])        // (an equal threshold: the row is a query row)
                    cnt[t][r] += it < tgt_lane[row * RANK_SLOTS + t] ? 1 : 0;
        }
    };
    auto tiles = [&](auto TAIL, int i0, const f32x4 *rows) __attribute__((always_inline)) {
        if (!active) return;
        tile(TAIL, i0, rows);
        if (ST == 64 && (!decltype(TAIL)::value || i0 + 32 < i_end)) tile(TAIL, i0 + 32, rows + 32 * PQ);
    };
    int buf = 0;
    auto publish = [&]() __attribute__((always_inline)) {
        stash(buf ^ 1);                               // last read there: the stage before this one, behind the barrier
        __syncthreads();
        buf ^= 1;
    };
    const int n_full = (i_end - i_begin) / ST;
    const bool has_tail = (i_end - i_begin) % ST != 0;
    const std::integral_constant<bool, false> FULL;
    const std::integral_constant<bool, true> PARTIAL;
    int i0 = i_begin;
    if (n_full > 0) fetch_full(); else fetch_tail(i_begin);            // (segments are never empty)
    stash(0);
    __syncthreads();
    const int n_steady = n_full > 0 ? n_full - 1 : 0;
    for (int s0 = 0; s0 < n_steady; s0 += PRIO_SLICE) {
        slice_priority(s0);
        const int s1 = s0 + PRIO_SLICE < n_steady ? s0 + PRIO_SLICE : n_steady;
        for (int st = s0; st < s1; ++st, i0 += ST) {
            fetch_full();
            tiles(FULL, i0, stage + (size_t)buf * ST * PQ);
            publish();
        }
    }
    if (n_full > 0) {
        if (has_tail) fetch_tail(i0 + ST);
        tiles(FULL, i0, stage + (size_t)buf * ST * PQ);
        if (has_tail) publish();
        i0 += ST;
    }
    if (has_tail) tiles(PARTIAL, i0, stage + (size_t)buf * ST * PQ);
    __syncthreads();                                  // the next user tile's first stage goes where this one is read
    // hand the counts over: sum over the 32 item columns of a half-wave, one atomic per (query row, counter) and segment
    if (active) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int qq = q0 + (r & 3) + 8 * (r >> 2) + 4 * h;
#pragma unroll
            for (int t = 0; t < TS; ++t) {
                const int n = rank_half_sum(cnt[t][r]);
                if (c == 0 && qq < p.nq && n) atomicAdd(rp.cnt + (int64_t)qq * RANK_STRIDE + t, n);
            }
        }
    }
    }   // user tiles
    __builtin_amdgcn_s_setprio(0);
}

// fp64 contexts and Kpad > 128: one wavefront per query row, lanes stride the items; thresholds, competitors and excluded
// items all come from the same fma chain.  Parity path.
template <typename S>
__global__ __launch_bounds__(256) void rank_generic_kernel(TopkParams p, RankParams rp, const S *fu, const S *fi, const S *bu,
                                                           const S *bi, int mode) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + wave;
    if (q >= p.nq) return;
    const int user = p.users[q];
    const S *arow = fu + (int64_t)user * p.kpad;
    auto score = [&](int it) -> S {
        const S *b = fi + (int64_t)it * p.kpad;
        S s = (S)0;
        for (int k = 0; k < p.K; ++k) s = fma(arow[k], b[k], s);
        if (mode == PMF_PREDICT_BIAS) return rank_score<PMF_PREDICT_BIAS>(s, bu[user], bi[it]);
        if (mode == PMF_PREDICT_SCALE) return rank_score<PMF_PREDICT_SCALE>(s, bu[user], bi[it]);
        return s;
    };
    S th[RANK_SLOTS];
    int tg[RANK_SLOTS], cnt[RANK_SLOTS], n_nan = 0, n_excl = 0, mask = 0;
    // lane t scores slot t's target (the chain the competitors go through); the wave reads the results from it
    const int my_tg = lane < RANK_SLOTS ? rp.tgt[(int64_t)q * RANK_SLOTS + lane] : -1;
    const S my_th = my_tg >= 0 ? score(my_tg) : (S)__builtin_nanf("");
#pragma unroll
    for (int t = 0; t < RANK_SLOTS; ++t) {
        tg[t] = __shfl(my_tg, t, 64);
        th[t] = __shfl(my_th, t, 64);
        if (tg[t] >= 0 && th[t] != th[t]) mask |= 1 << t;
        cnt[t] = 0;
    }
    for (int it = lane; it < (int)p.n_items; it += 64) {
        const S s = score(it);
        n_nan += s != s ? 1 : 0;
#pragma unroll
        for (int t = 0; t < RANK_SLOTS; ++t) cnt[t] += rank_beats(s, it, th[t], tg[t]) ? 1 : 0;
    }
    if (rp.ex_ptr) {
        const int64_t end = rp.ex_ptr[user + 1];
        for (int64_t e = rp.ex_ptr[user] + lane; e < end; e += 64) {
            const int it = rp.ex_items[e];
            const S s = score(it);
            n_excl += s == s ? 1 : 0;
#pragma unroll
            for (int t = 0; t < RANK_SLOTS; ++t) cnt[t] -= rank_beats(s, it, th[t], tg[t]) ? 1 : 0;
        }
    }
    int32_t *out = rp.cnt + (int64_t)q * RANK_STRIDE;
#pragma unroll
    for (int t = 0; t < RANK_SLOTS; ++t) {
        const int n = rank_half_sum(cnt[t]);
        const int total = n + __shfl_xor(n, 32, 64);
        if (lane == 0) out[t] = total;
    }
    n_nan = rank_half_sum(n_nan);
    n_nan += __shfl_xor(n_nan, 32, 64);
    n_excl = rank_half_sum(n_excl);
    n_excl += __shfl_xor(n_excl, 32, 64);
    if (lane == 0) {
        out[RANK_NAN] = n_nan;
        out[RANK_EXCL] = n_excl;
        out[RANK_MASK] = mask;
    }
}

template <int KH, int MODE, int TS>
static hipError_t launch_rank_fused(pmf_ctx *ctx, const TopkParams &p, const RankParams &rp, dim3 grid, const float *fu,
                                    const float *fi, const float *cu, const float *ci, int64_t seg_items) {
    const void *fn = (const void *)rank_fused_kernel<KH, MODE, TS>;
    const size_t smem = 2 * TopkStage<KH>::buffer_bytes;
    int per_cu = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 256, smem);
    if (e == hipSuccess) e = topk_persistent_grid(ctx, per_cu, &grid);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((rank_fused_kernel<KH, MODE, TS>), grid, dim3(256), smem, ctx->stream, p, rp, fu, fi, cu, ci, seg_items);
    return hipSuccess;
}

// the launches of one batch of query rows (ids, targets and zeroed counters are on the device)
template <typename T>
static int launch_rank(pmf_ctx *ctx, const TopkSource &src, const TopkParams &p, const RankParams &rp, int mode, bool one_slot) {
    const int64_t I = p.n_items;
    const T *fu = static_cast<const T *>(src.fa), *fi = static_cast<const T *>(src.fb);
    const T *cu = static_cast<const T *>(src.ca), *ci = static_cast<const T *>(src.cb);
    const dim3 row_grid((unsigned)((p.nq + 3) / 4));
    PmfProfScope prof(ctx, PMF_KERNEL_TOPK);
    if constexpr (std::is_same<T, float>::value) {
        if (ctx->kpad <= 128) {   // (the item count fits the scan's ints: rank_items_impl)
            int64_t seg_items;
            const int nseg = topk_segments(p.nq, I, &seg_items);
            const dim3 grid((unsigned)((p.nq + 127) / 128), (unsigned)nseg);
            PMF_HIP_CHECK(pmf_with_pow2<8>(ctx->kpad / 2, [&](auto kh) {
                return pmf_with_predict_mode(mode, [&](auto m) {
                    constexpr int KH = decltype(kh)::value, MODE = decltype(m)::value;
                    hipLaunchKernelGGL((rank_rows_kernel<KH, MODE, false>), row_grid, dim3(256), 0, ctx->stream, p, rp, fu, fi, cu, ci);
                    hipError_t e = one_slot ? launch_rank_fused<KH, MODE, 1>(ctx, p, rp, grid, fu, fi, cu, ci, seg_items)
                                            : launch_rank_fused<KH, MODE, RANK_SLOTS>(ctx, p, rp, grid, fu, fi, cu, ci, seg_items);
                    if (e == hipSuccess && rp.ex_ptr)
                        hipLaunchKernelGGL((rank_rows_kernel<KH, MODE, true>), row_grid, dim3(256), 0, ctx->stream, p, rp, fu, fi, cu, ci);
                    return e;
                });
            }));
            return PMF_OK;
        }
    }
    hipLaunchKernelGGL((rank_generic_kernel<T>), row_grid, dim3(256), 0, ctx->stream, p, rp, fu, fi, cu, ci, mode);
    return PMF_OK;
}

// The ranks of the targets item_ids[row_ptr[n] .. row_ptr[n + 1]) of every row n of `src` among its candidates (arguments
// and arrays are checked, the device is current: rank_items_impl, pmf_rank_query).
static int run_rank(pmf_ctx *ctx, const TopkSource &src, int64_t n_rows, const int64_t *row_ptr, const int32_t *item_ids,
                    int use_bias, int64_t *out_rank, int64_t *out_candidates) {
    const int64_t I = src.n_cand;
    int rc;
    // query rows: a user's targets in runs of at most `slots`; a user without targets keeps one row (its candidates)
    const int slots = ctx->rank_targets > 0 ? std::min(ctx->rank_targets, RANK_SLOTS) : RANK_SLOTS;
    struct QueryRow {
        int64_t row, first;   // the caller's row and the offset of the run's first target in item_ids
        int n;
    };
    std::vector<QueryRow> qrows;
    bool one_slot = true;
    for (int64_t n = 0; n < n_rows; ++n) {
        int64_t at = row_ptr[n];
        do {
            const int len = (int)std::min<int64_t>(slots, row_ptr[n + 1] - at);
            qrows.push_back({n, at, len});
            one_slot = one_slot && len <= 1;
            at += len;
        } while (at < row_ptr[n + 1]);
    }
    const int64_t n_query = (int64_t)qrows.size();
    const int64_t Q = std::min<int64_t>(n_query, topk_round_rows(ctx));   // query rows per launch
    PmfLayout lay;
    const auto users_at = lay.add<int32_t>((size_t)Q), tgt_at = lay.add<int32_t>((size_t)Q * RANK_SLOTS);
    const auto th_at = lay.add<double>((size_t)Q * RANK_SLOTS);     // thresholds, context dtype
    const auto cnt_at = lay.add<int32_t>((size_t)Q * RANK_STRIDE);
    if ((rc = pmf_ensure_scratch(ctx, lay.bytes()))) return rc;
    void *base = ctx->d_scratch.as();
    int32_t *d_users = users_at.at(base), *d_tgt = tgt_at.at(base), *d_cnt = cnt_at.at(base);
    void *d_th = th_at.at(base);
    std::vector<int32_t> h_users((size_t)Q), h_tgt((size_t)Q * RANK_SLOTS), h_cnt((size_t)Q * RANK_STRIDE);
    for (int64_t at = 0; at < n_query; at += Q) {
        const int nq = (int)std::min<int64_t>(Q, n_query - at);
        // (a staged source: the round's query rows belong to the caller's rows row0 .. row1, which are what is staged)
        const int64_t row0 = qrows[(size_t)at].row, row1 = qrows[(size_t)(at + nq - 1)].row;
        TopkSource r;
        if ((rc = topk_round_source(ctx, src, row0, row1 - row0 + 1, &r))) return rc;
        for (int q = 0; q < nq; ++q) {
            const QueryRow &qr = qrows[(size_t)(at + q)];
            h_users[(size_t)q] = src.ids ? src.ids[qr.row] : (int32_t)(qr.row - row0);
            for (int t = 0; t < RANK_SLOTS; ++t) h_tgt[(size_t)q * RANK_SLOTS + t] = t < qr.n ? item_ids[qr.first + t] : -1;
        }
        PMF_HIP_CHECK(hipMemcpyAsync(d_users, h_users.data(), (size_t)nq * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        PMF_HIP_CHECK(hipMemcpyAsync(d_tgt, h_tgt.data(), (size_t)nq * RANK_SLOTS * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        PMF_HIP_CHECK(hipMemsetAsync(d_cnt, 0, (size_t)nq * RANK_STRIDE * sizeof(int32_t), ctx->stream));
        TopkParams p;
        p.users = d_users;
        p.nq = nq;
        p.n_items = I;
        p.K = ctx->K;
        p.kpad = ctx->kpad;
        RankParams rp;
        rp.tgt = d_tgt;
        rp.th = d_th;
        rp.cnt = d_cnt;
        rp.ex_ptr = r.ex_ptr;
        rp.ex_items = r.ex_ids;
        if ((rc = pmf_with_dtype(ctx, [&](auto t) { return launch_rank<decltype(t)>(ctx, r, p, rp, use_bias, one_slot); }))) return rc;
        PMF_HIP_CHECK(hipGetLastError());
        PMF_HIP_CHECK(hipMemcpyAsync(h_cnt.data(), d_cnt, (size_t)nq * RANK_STRIDE * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        PMF_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        for (int q = 0; q < nq; ++q) {
            const QueryRow &qr = qrows[(size_t)(at + q)];
            const int32_t *cnt = h_cnt.data() + (size_t)q * RANK_STRIDE;
            for (int t = 0; t < qr.n; ++t) out_rank[qr.first + t] = (cnt[RANK_MASK] >> t) & 1 ? -1 : (int64_t)cnt[t];
            if (out_candidates && qr.first == row_ptr[qr.row]) out_candidates[qr.row] = I - cnt[RANK_NAN] - cnt[RANK_EXCL];
        }
    }
    return PMF_OK;
}

static int rank_items_impl(pmf_ctx *ctx, int64_t n_rows, const int32_t *user_ids, const int64_t *row_ptr,
                           const int32_t *item_ids, int use_bias, int exclude_train, int64_t *out_rank,
                           int64_t *out_candidates) {
    const int64_t U = ctx->rows[PMF_SIDE_USER], I = ctx->rows[PMF_SIDE_ITEM];
    PMF_REQUIRE(user_ids && row_ptr, PMF_EINVAL, "pmf_rank_items: null user_ids or row_ptr");
    int rc;
    if ((rc = pmf_check_offsets("pmf_rank_items", "row_ptr", row_ptr, n_rows))) return rc;
    const int64_t n_targets = row_ptr[n_rows];
    PMF_REQUIRE(n_targets == 0 || (item_ids && out_rank), PMF_EINVAL, "pmf_rank_items: null item_ids or out_rank");
    PMF_REQUIRE(use_bias == 0 || use_bias == PMF_PREDICT_BIAS || use_bias == PMF_PREDICT_SCALE, PMF_EINVAL,
                "pmf_rank_items: use_bias must be 0, PMF_PREDICT_BIAS or PMF_PREDICT_SCALE (got %d)", use_bias);
    if ((rc = pmf_require_array(ctx, PMF_SIDE_USER, PMF_ARR_FACTOR, "pmf_rank_items"))) return rc;
    if ((rc = pmf_require_array(ctx, PMF_SIDE_ITEM, PMF_ARR_FACTOR, "pmf_rank_items"))) return rc;
    if (use_bias) {
        const int carr = use_bias == PMF_PREDICT_SCALE ? PMF_ARR_SCALE : PMF_ARR_BIAS;
        if ((rc = pmf_require_array(ctx, PMF_SIDE_USER, carr, "pmf_rank_items"))) return rc;
        if ((rc = pmf_require_array(ctx, PMF_SIDE_ITEM, carr, "pmf_rank_items"))) return rc;
    }
    PMF_REQUIRE(I <= (int64_t)INT32_MAX - 64, PMF_ERANGE, "pmf_rank_items: %lld items; the kernels count items in 32-bit integers",
                (long long)I);
    PMF_REQUIRE(!exclude_train || ctx->index[PMF_SIDE_USER].d_ptr, PMF_EINVAL,
                "pmf_rank_items: exclude_train needs the training ratings (pmf_ctx_set_ratings); the context holds none");
    if ((rc = pmf_check_ids(user_ids, n_rows, U, "pmf_rank_items", "user id"))) return rc;
    if ((rc = pmf_check_ids(item_ids, n_targets, I, "pmf_rank_items", "item id"))) return rc;
    PMF_HIP_CHECK(hipSetDevice(ctx->device));
    if (exclude_train && (rc = pmf_index_distinct(ctx, PMF_SIDE_USER))) return rc;

    const TopkSource src = topk_items_source(ctx, user_ids, use_bias, exclude_train != 0);
    return run_rank(ctx, src, n_rows, row_ptr, item_ids, use_bias, out_rank, out_candidates);
}

extern "C" int pmf_rank_items(pmf_ctx *ctx, int64_t n_rows, const int32_t *user_ids, const int64_t *row_ptr,
                              const int32_t *item_ids, int use_bias, int exclude_train, int64_t *out_rank,
                              int64_t *out_candidates) {
    PMF_REQUIRE(ctx != nullptr, PMF_EINVAL, "pmf_rank_items: null context");
    PMF_REQUIRE(n_rows >= 0, PMF_EINVAL, "pmf_rank_items: negative n_rows");
    if (n_rows == 0) return PMF_OK;
    return pmf_no_throw("pmf_rank_items", [&] {
        return rank_items_impl(ctx, n_rows, user_ids, row_ptr, item_ids, use_bias, exclude_train, out_rank, out_candidates);
    });
}

// ---------------------------------------------------------------------------
// pmf_topk_query / pmf_rank_query: any rows against all rows of one side
// ---------------------------------------------------------------------------
// No scan of their own: the query rows of a round are STAGED into a dense [n x Kpad] table of the context's dtype with
// their coefficients in a dense [n] array, the scan's ids are 0 .. n - 1, and the kernels above run on that source as they
// run on the context's users.  Cosine is the PMF_PREDICT_SCALE arithmetic, dot * (c_q * c_c), on inverse row norms.
// Both calls prepare their source with the same functions (query_check, query_begin, query_stage_rows): a pair has one
// score, whichever call asks.

// staged row q = row ids[q] of `table`, its coefficient = coef_table[ids[q]] (null: none); one 16-byte piece per lane,
// consecutive lanes on consecutive pieces of a row
template <typename T>
__global__ __launch_bounds__(256) void query_gather_kernel(const T *table, const T *coef_table, const int32_t *ids, int n,
                                                           int kpad, T *rows, T *coef) {
    const int pr = kpad * (int)sizeof(T) / 16;        // pieces per row (Kpad is a multiple of 4)
    const int64_t total = (int64_t)n * pr;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int q = (int)(e / pr), pc = (int)(e % pr);
        const int id = ids[q];
        reinterpret_cast<f32x4 *>(rows)[e] = reinterpret_cast<const f32x4 *>(table + (int64_t)id * kpad)[pc];
        if (coef_table && pc == 0) coef[q] = coef_table[id];
    }
}

// coef[q] = coef_table[ids[q]]: the coefficients alone, for a round whose rows are sampled (pmf_topk_sampled)
template <typename T>
__global__ __launch_bounds__(256) void query_gather_coef_kernel(const T *coef_table, const int32_t *ids, int n, T *coef) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n) coef[q] = coef_table[ids[q]];
}

// ids[q] = q: the scan's ids of a staged round
__global__ __launch_bounds__(256) void query_iota_kernel(int32_t *ids, int n) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n) ids[q] = q;
}

// inv[r] = 1 / sqrt(sum_k rows[r][k]^2) in T, correctly rounded square root and division (a zero row gives +inf, a row
// with a NaN gives NaN).  16 lanes per row, 16-byte pieces, a fixed order of additions: two calls give the same bits.
template <typename T>
__global__ __launch_bounds__(256) void query_inv_norm_kernel(const T *rows, int64_t n, int kpad, T *inv) {
    constexpr int PE = 16 / (int)sizeof(T);           // elements per piece
    const int sub = threadIdx.x & 15;
    for (int64_t base = (int64_t)blockIdx.x * 16; base < n; base += (int64_t)gridDim.x * 16) {   // (uniform trips: the shuffles)
        const int64_t r = base + (threadIdx.x >> 4);
        T s = (T)0;
        if (r < n) {
            const T *row = rows + r * kpad;
            for (int k = sub * PE; k < kpad; k += 16 * PE) {
                const f32x4 piece = *reinterpret_cast<const f32x4 *>(row + k);
                T v[PE];
                __builtin_memcpy(v, &piece, 16);
#pragma unroll
                for (int j = 0; j < PE; ++j) s = fma(v[j], v[j], s);
            }
        }
        s += __shfl_xor(s, 8, 64);
        s += __shfl_xor(s, 4, 64);
        s += __shfl_xor(s, 2, 64);
        s += __shfl_xor(s, 1, 64);
        if (sub == 0 && r < n) inv[r] = (T)1 / sqrt(s);
    }
}

template <typename T>
static void launch_inv_norm(pmf_ctx *ctx, const T *rows, int64_t n, T *inv) {
    const unsigned blocks = (unsigned)std::min<int64_t>((n + 15) / 16, 1 << 20);
    hipLaunchKernelGGL((query_inv_norm_kernel<T>), dim3(blocks), dim3(256), 0, ctx->stream, rows, n, ctx->kpad, inv);
}

// where the query rows come from (pmf_topk_query documents the two modes)
struct QueryStage {
    const int32_t *ids = nullptr;                         // ids mode: host [n_query] rows of ...
    const void *table = nullptr, *coef_table = nullptr;   // ... this device table, with this coefficient array (null: none)
    const double *factor = nullptr, *coef = nullptr;      // vector mode: host [n_query x K] and [n_query] (null: none)
    bool cosine = false;                                  // the coefficient is the staged row's inverse norm
    const int64_t *d_ex_ptr = nullptr;                    // device [n_query + 1]: the rows' exclusion lists, or null
    // pmf_topk_sampled (ids mode): the staged rows are not the table's but draw `draw` under `seed` of rows `ids` of this side
    int sample_side = -1;                                 // -1: no sampling
    uint64_t seed = 0;
    int draw = 0;
    void *d_tri = nullptr;                                // the sample kernel's triangles (pmf_gauss_sample_tri_bytes), or null
};

// rows [row0, row0 + n) of `st` into ctx->d_query_rows; round->fa / ca / ex_ptr are theirs
template <typename T>
static int query_stage_rows(pmf_ctx *ctx, const QueryStage &st, int64_t row0, int64_t n, TopkSource *round) {
    const int K = ctx->K, kpad = ctx->kpad;
    const size_t row_bytes = (size_t)kpad * sizeof(T);
    PmfLayout lay;
    const auto rows_at = lay.add<T>((size_t)n * kpad), coef_at = lay.add<T>((size_t)n);
    const auto ids_at = lay.add<int32_t>((size_t)n);
    int rc;
    if ((rc = ctx->d_query_rows.reserve(ctx, lay.bytes(), {ctx->stream}))) return rc;
    void *base = ctx->d_query_rows.as();
    T *d_rows = rows_at.at(base), *d_coef = coef_at.at(base);
    int32_t *d_ids = ids_at.at(base);
    if (st.ids) {
        PMF_HIP_CHECK(hipMemcpyAsync(d_ids, st.ids + row0, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        if (st.sample_side >= 0) {   // the sample kernel writes the rows where the gather would
            if ((rc = pmf_gauss_sample_launch(ctx, st.sample_side, d_ids, n, 1, st.draw, st.seed, nullptr, d_rows, st.d_tri))) return rc;
            if (st.coef_table) {
                PmfProfScope prof(ctx, PMF_KERNEL_TOPK);
                hipLaunchKernelGGL((query_gather_coef_kernel<T>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream,
                                   static_cast<const T *>(st.coef_table), d_ids, (int)n, d_coef);
            }
        } else {
            PmfProfScope prof(ctx, PMF_KERNEL_TOPK);
            const int64_t pieces = n * (int64_t)(row_bytes / 16);
            hipLaunchKernelGGL((query_gather_kernel<T>), dim3((unsigned)std::min<int64_t>((pieces + 255) / 256, 1 << 20)), dim3(256), 0,
                               ctx->stream, static_cast<const T *>(st.table), static_cast<const T *>(st.coef_table), d_ids, (int)n,
                               kpad, d_rows, d_coef);
        }
    } else {
        // the caller's float64 rows -> T, zero-padded to Kpad (the conversion of pmf_set_array_rows), through pinned steps
        const int64_t step = std::max<int64_t>(1, ctx->stage_bytes / (int64_t)row_bytes);
        if ((rc = pmf_ensure_pinned(ctx, (size_t)std::min(step, n) * row_bytes))) return rc;
        T *pin = ctx->h_pinned.as<T>();
        for (int64_t r0 = 0; r0 < n; r0 += step) {
            const int64_t nr = std::min(step, n - r0);
            for (int64_t r = 0; r < nr; ++r) {
                const double *s = st.factor + (row0 + r0 + r) * K;
                T *d = pin + r * kpad;
                for (int k = 0; k < K; ++k) d[k] = (T)s[k];
                for (int k = K; k < kpad; ++k) d[k] = (T)0;
            }
            PMF_HIP_CHECK(hipMemcpyAsync(d_rows + r0 * kpad, pin, (size_t)nr * row_bytes, hipMemcpyHostToDevice, ctx->stream));
            PMF_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        }
        for (int64_t r0 = 0; st.coef && r0 < n; r0 += step * kpad) {
            const int64_t nr = std::min(step * kpad, n - r0);
            for (int64_t r = 0; r < nr; ++r) pin[r] = (T)st.coef[row0 + r0 + r];
            PMF_HIP_CHECK(hipMemcpyAsync(d_coef + r0, pin, (size_t)nr * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
            PMF_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        }
    }
    if (st.cosine) {
        PmfProfScope prof(ctx, PMF_KERNEL_TOPK);
        launch_inv_norm<T>(ctx, d_rows, n, d_coef);
    }
    PMF_HIP_CHECK(hipGetLastError());
    round->fa = d_rows;
    round->ca = (st.cosine || st.coef_table || st.coef) ? d_coef : nullptr;
    round->ex_ptr = st.d_ex_ptr ? st.d_ex_ptr + row0 : nullptr;
    return PMF_OK;
}

static int topk_round_source(pmf_ctx *ctx, const TopkSource &src, int64_t row0, int64_t n, TopkSource *round) {
    *round = src;
    if (!src.staged) return PMF_OK;
    return pmf_with_dtype(ctx, [&](auto t) { return query_stage_rows<decltype(t)>(ctx, *src.staged, row0, n, round); });
}

static int topk_round_ids(pmf_ctx *ctx, const TopkSource &src, int64_t row0, int n, int32_t *d_ids) {
    if (src.ids) {
        PMF_HIP_CHECK(hipMemcpyAsync(d_ids, src.ids + row0, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    } else {
        hipLaunchKernelGGL(query_iota_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_ids, n);
    }
    return PMF_OK;
}

// a call's source, and what it points into
struct QueryCall {
    int mode = 0;                      // the kernels' mode: `score`, with PMF_PREDICT_SCALE for cosine
    QueryStage stage;
    TopkSource src;
    std::vector<int64_t> ex_ptr;       // the exclusion lists, each sorted and without repeats
    std::vector<int32_t> ex_ids;
};

// The checks the two query calls share, and the host side of their source.  Nothing is written anywhere else.
static int query_check(const char *fn, pmf_ctx *ctx, int cand_side, int64_t n_query, int query_side, const int32_t *query_ids,
                       const double *query_factor, const double *query_coef, int score, const int64_t *ex_ptr,
                       const int32_t *ex_ids, QueryCall *qc) {
    PMF_REQUIRE(cand_side == PMF_SIDE_USER || cand_side == PMF_SIDE_ITEM, PMF_EINVAL, "%s: bad cand_side %d", fn, cand_side);
    PMF_REQUIRE(!(query_ids && query_factor), PMF_EINVAL, "%s: both query_ids and query_factor given; exactly one names the query rows", fn);
    PMF_REQUIRE(query_ids || query_factor, PMF_EINVAL, "%s: neither query_ids nor query_factor given; exactly one names the query rows", fn);
    PMF_REQUIRE(score == 0 || score == PMF_PREDICT_BIAS || score == PMF_PREDICT_SCALE || score == PMF_SCORE_COSINE, PMF_EINVAL,
                "%s: score must be 0, PMF_PREDICT_BIAS, PMF_PREDICT_SCALE or PMF_SCORE_COSINE (got %d)", fn, score);
    const bool model_coef = score == PMF_PREDICT_BIAS || score == PMF_PREDICT_SCALE;
    const int carr = score == PMF_PREDICT_SCALE ? PMF_ARR_SCALE : PMF_ARR_BIAS;
    const int64_t C = ctx->rows[cand_side];
    int rc;
    if (query_ids) {
        PMF_REQUIRE(query_side == PMF_SIDE_USER || query_side == PMF_SIDE_ITEM, PMF_EINVAL, "%s: bad query_side %d", fn, query_side);
        PMF_REQUIRE(query_side != cand_side || !model_coef, PMF_EINVAL,
                    "%s: query_side == cand_side needs score 0 or PMF_SCORE_COSINE: a bias or scale of two rows of one side is no model score (got %d)",
                    fn, score);
        if ((rc = pmf_check_ids(query_ids, n_query, ctx->rows[query_side], fn, "query id"))) return rc;
        if ((rc = pmf_require_array(ctx, query_side, PMF_ARR_FACTOR, fn))) return rc;
        if (model_coef && (rc = pmf_require_array(ctx, query_side, carr, fn))) return rc;
    } else {
        PMF_REQUIRE(!model_coef || query_coef, PMF_EINVAL, "%s: null query_coef: the caller's rows need their bias / scale under score %d", fn,
                    score);
    }
    if ((rc = pmf_require_array(ctx, cand_side, PMF_ARR_FACTOR, fn))) return rc;
    if (model_coef && (rc = pmf_require_array(ctx, cand_side, carr, fn))) return rc;
    if (ex_ptr) {
        if ((rc = pmf_check_offsets(fn, "ex_ptr", ex_ptr, n_query))) return rc;
        PMF_REQUIRE(ex_ptr[n_query] == 0 || ex_ids, PMF_EINVAL, "%s: null ex_ids", fn);
        if ((rc = pmf_check_ids(ex_ids, ex_ptr[n_query], C, fn, "excluded id"))) return rc;
        // the fused scan's cursor and the counts of the ranking need ascending distinct ids
        qc->ex_ptr.assign((size_t)n_query + 1, 0);
        qc->ex_ids.reserve((size_t)ex_ptr[n_query]);
        for (int64_t n = 0; n < n_query; ++n) {
            const size_t first = qc->ex_ids.size();
            qc->ex_ids.insert(qc->ex_ids.end(), ex_ids + ex_ptr[n], ex_ids + ex_ptr[n + 1]);
            std::sort(qc->ex_ids.begin() + first, qc->ex_ids.end());
            qc->ex_ids.erase(std::unique(qc->ex_ids.begin() + first, qc->ex_ids.end()), qc->ex_ids.end());
            qc->ex_ptr[(size_t)n + 1] = (int64_t)qc->ex_ids.size();
        }
    }
    qc->mode = score == PMF_SCORE_COSINE ? PMF_PREDICT_SCALE : score;
    qc->stage.cosine = score == PMF_SCORE_COSINE;
    if (query_ids) {
        qc->stage.ids = query_ids;
        qc->stage.table = ctx->arr[query_side][PMF_ARR_FACTOR].as();
        qc->stage.coef_table = model_coef ? ctx->arr[query_side][carr].as() : nullptr;
    } else {
        qc->stage.factor = query_factor;
        qc->stage.coef = model_coef ? query_coef : nullptr;
    }
    qc->src.fb = ctx->arr[cand_side][PMF_ARR_FACTOR].as();
    qc->src.cb = model_coef ? ctx->arr[cand_side][carr].as() : nullptr;
    qc->src.n_cand = C;
    qc->src.staged = &qc->stage;
    return PMF_OK;
}

// The device side of a call's source, once per call into ctx->d_query_call: the exclusion CSR, and for cosine the
// candidates' inverse norms from cand_side's FACTOR as it is now.
template <typename T>
static int query_begin(pmf_ctx *ctx, QueryCall *qc) {
    const bool lists = !qc->ex_ptr.empty();
    PmfLayout lay;
    const auto ptr_at = lay.add<int64_t>(qc->ex_ptr.size());
    const auto ids_at = lay.add<int32_t>(qc->ex_ids.size(), lists);   // (the kernels get the pointer even when every list is empty)
    const auto norm_at = lay.add<T>(qc->stage.cosine ? (size_t)qc->src.n_cand : 0);
    if (lay.bytes() == 0) return PMF_OK;
    int rc;
    if ((rc = ctx->d_query_call.reserve(ctx, lay.bytes(), {ctx->stream}))) return rc;
    void *base = ctx->d_query_call.as();
    if (lists) {
        PMF_HIP_CHECK(hipMemcpyAsync(ptr_at.at(base), qc->ex_ptr.data(), qc->ex_ptr.size() * sizeof(int64_t), hipMemcpyHostToDevice,
                                     ctx->stream));
        if (!qc->ex_ids.empty())
            PMF_HIP_CHECK(hipMemcpyAsync(ids_at.at(base), qc->ex_ids.data(), qc->ex_ids.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                                         ctx->stream));
        qc->stage.d_ex_ptr = ptr_at.at(base);
        qc->src.ex_ids = ids_at.at(base);
    }
    if (qc->stage.cosine) {
        T *inv = norm_at.at(base);
        PmfProfScope prof(ctx, PMF_KERNEL_TOPK);
        launch_inv_norm<T>(ctx, static_cast<const T *>(qc->src.fb), qc->src.n_cand, inv);
        qc->src.cb = inv;
    }
    PMF_HIP_CHECK(hipGetLastError());
    return PMF_OK;
}

extern "C" int pmf_topk_query(pmf_ctx *ctx, int cand_side, int64_t n_query, int query_side, const int32_t *query_ids,
                              const double *query_factor, const double *query_coef, int score, const int64_t *ex_ptr,
                              const int32_t *ex_ids, int k, int32_t *out_ids, double *out_scores) {
    const char *fn = "pmf_topk_query";
    PMF_REQUIRE(ctx != nullptr, PMF_EINVAL, "%s: null context", fn);
    PMF_REQUIRE(n_query >= 0, PMF_EINVAL, "%s: negative n_query", fn);
    if (n_query == 0) return PMF_OK;
    return pmf_no_throw(fn, [&] {
        QueryCall qc;
        PMF_REQUIRE(out_ids && out_scores, PMF_EINVAL, "%s: null out_ids or out_scores", fn);
        if (int rc = query_check(fn, ctx, cand_side, n_query, query_side, query_ids, query_factor, query_coef, score, ex_ptr, ex_ids, &qc))
            return rc;
        PMF_REQUIRE(k >= 1 && k <= 1024 && k <= qc.src.n_cand, PMF_ERANGE, "%s: k=%d outside [1, min(1024, rows of cand_side)]", fn, k);
        // (every refusal comes before the first write)
        PMF_HIP_CHECK(hipSetDevice(ctx->device));
        return pmf_with_dtype(ctx, [&](auto t) {
            if (int rc = query_begin<decltype(t)>(ctx, &qc)) return rc;
            return run_topk<decltype(t)>(ctx, qc.src, n_query, k, qc.mode, out_ids, out_scores);
        });
    });
}

extern "C" int pmf_rank_query(pmf_ctx *ctx, int cand_side, int64_t n_query, int query_side, const int32_t *query_ids,
                              const double *query_factor, const double *query_coef, int score, const int64_t *ex_ptr,
                              const int32_t *ex_ids, const int64_t *tgt_ptr, const int32_t *tgt_ids, int64_t *out_rank,
                              int64_t *out_candidates) {
    const char *fn = "pmf_rank_query";
    PMF_REQUIRE(ctx != nullptr, PMF_EINVAL, "%s: null context", fn);
    PMF_REQUIRE(n_query >= 0, PMF_EINVAL, "%s: negative n_query", fn);
    if (n_query == 0) return PMF_OK;
    return pmf_no_throw(fn, [&] {
        QueryCall qc;
        PMF_REQUIRE(tgt_ptr, PMF_EINVAL, "%s: null tgt_ptr", fn);
        if (int rc = pmf_check_offsets(fn, "tgt_ptr", tgt_ptr, n_query)) return rc;
        PMF_REQUIRE(tgt_ptr[n_query] == 0 || (tgt_ids && out_rank), PMF_EINVAL, "%s: null tgt_ids or out_rank", fn);
        if (int rc = query_check(fn, ctx, cand_side, n_query, query_side, query_ids, query_factor, query_coef, score, ex_ptr, ex_ids, &qc))
            return rc;
        PMF_REQUIRE(qc.src.n_cand <= (int64_t)INT32_MAX - 64, PMF_ERANGE, "%s: %lld candidates; the kernels count them in 32-bit integers", fn,
                    (long long)qc.src.n_cand);
        if (int rc = pmf_check_ids(tgt_ids, tgt_ptr[n_query], qc.src.n_cand, fn, "target id")) return rc;
        PMF_HIP_CHECK(hipSetDevice(ctx->device));
        if (int rc = pmf_with_dtype(ctx, [&](auto t) { return query_begin<decltype(t)>(ctx, &qc); })) return rc;
        return run_rank(ctx, qc.src, n_query, tgt_ptr, tgt_ids, qc.mode, out_rank, out_candidates);
    });
}

// pmf_topk_query in ids mode on ONE joint posterior draw: every row of cand_side is sampled into the context's
// d_sample_table, which becomes the candidates' table, and every round's query rows are sampled into the staged table
// (QueryStage::sample_side).  Checks, exclusion lists, rounds and scans are pmf_topk_query's.
extern "C" int pmf_topk_sampled(pmf_ctx *ctx, int cand_side, int64_t n_query, int query_side, const int32_t *query_ids, int score,
                                const int64_t *ex_ptr, const int32_t *ex_ids, int k, uint64_t seed, int draw, int32_t *out_ids,
                                double *out_scores) {
    const char *fn = "pmf_topk_sampled";
    PMF_REQUIRE(ctx != nullptr, PMF_EINVAL, "%s: null context", fn);
    PMF_REQUIRE(n_query >= 0, PMF_EINVAL, "%s: negative n_query", fn);
    if (n_query == 0) return PMF_OK;
    return pmf_no_throw(fn, [&] {
        QueryCall qc;
        PMF_REQUIRE(out_ids && out_scores, PMF_EINVAL, "%s: null out_ids or out_scores", fn);
        PMF_REQUIRE(query_ids, PMF_EINVAL, "%s: null query_ids", fn);
        PMF_REQUIRE(score == 0 || score == PMF_PREDICT_BIAS, PMF_EINVAL,
                    "%s: score must be 0 or PMF_PREDICT_BIAS (got %d): a draw has no scale, and cosine is no model score", fn, score);
        PMF_REQUIRE(draw >= 0, PMF_EINVAL, "%s: negative draw %d", fn, draw);
        if (int rc = query_check(fn, ctx, cand_side, n_query, query_side, query_ids, nullptr, nullptr, score, ex_ptr, ex_ids, &qc))
            return rc;
        if (int rc = pmf_require_array(ctx, cand_side, PMF_ARR_COV, fn)) return rc;
        if (int rc = pmf_require_array(ctx, query_side, PMF_ARR_COV, fn)) return rc;
        PMF_REQUIRE(k >= 1 && k <= 1024 && k <= qc.src.n_cand, PMF_ERANGE, "%s: k=%d outside [1, min(1024, rows of cand_side)]", fn, k);
        // (every refusal comes before the first write)
        PMF_HIP_CHECK(hipSetDevice(ctx->device));
        const int64_t C = qc.src.n_cand;
        PmfLayout lay;
        const auto table_at = lay.add<unsigned char>((size_t)C * ctx->kpad * ctx->elem);
        const auto tri_at = lay.add<unsigned char>(pmf_gauss_sample_tri_bytes(ctx, std::max(C, n_query)));
        if (int rc = ctx->d_sample_table.reserve(ctx, lay.bytes(), {ctx->stream})) return rc;
        void *base = ctx->d_sample_table.as();
        void *tri = tri_at.offset < lay.bytes() ? tri_at.at(base) : nullptr;
        if (int rc = pmf_gauss_sample_launch(ctx, cand_side, nullptr, C, 1, draw, seed, nullptr, table_at.at(base), tri)) return rc;
        qc.src.fb = table_at.at(base);
        qc.stage.sample_side = query_side;
        qc.stage.seed = seed;
        qc.stage.draw = draw;
        qc.stage.d_tri = tri;
        return pmf_with_dtype(ctx, [&](auto t) {
            if (int rc = query_begin<decltype(t)>(ctx, &qc)) return rc;
            return run_topk<decltype(t)>(ctx, qc.src, n_query, k, qc.mode, out_ids, out_scores);
        });
    });
}
