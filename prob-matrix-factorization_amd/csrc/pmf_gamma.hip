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
    T esum = (T)0;
#pragma unroll
    for (int e = 0; e < PMF_VEC; ++e) {
        const bool ok = active && (koff + e) < p.K;
        T s = p.shape_prior + sum_a.v[e];
        T r = rp + sum_b.v[e];
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
// host side
// ---------------------------------------------------------------------------
struct GammaPriors { double shape = 0, rate = 0; int hierarchical = 0; double hyper_shape = 0, hyper_rate = 0; };

// the sweep kernel over the tasks, then the split kernel over the rows cut into several tasks
template <typename T, int LPR, bool STATS, bool EXT>
static void launch_gamma(pmf_ctx *ctx, const GammaParams<T> &p, const PmfTaskView &tl) {
    constexpr int G = 256 / LPR;
    if (tl.n_tasks > 0) {
        PmfProfScope prof(ctx, PMF_KERNEL_GAMMA_SWEEP);
        hipLaunchKernelGGL((gamma_sweep_kernel<T, LPR, STATS, EXT>), dim3((unsigned)((tl.n_tasks + G - 1) / G)), dim3(256), 0, ctx->stream, p);
    }
    if (tl.n_split > 0) {
        PmfProfScope prof(ctx, PMF_KERNEL_GAMMA_FINAL);
        size_t smem = (size_t)G * 2 * ctx->kpad * sizeof(T);
        hipLaunchKernelGGL((gamma_split_kernel<T, LPR, STATS, EXT>), dim3((unsigned)tl.n_split), dim3(256), smem, ctx->stream, p);
    }
}

// f(std::integral_constant<int, LPR>()) for the context's lanes per row, then the launch error check
template <typename F>
static int gamma_launch(pmf_ctx *ctx, F &&f) {
    const int lpr = pmf_lanes_per_row(ctx->kpad);
    PMF_REQUIRE(lpr <= 64, PMF_ERANGE, "pmf_gamma_sweep: unsupported n_factors %d", ctx->K);
    pmf_with_pow2<1>(lpr, f);
    PMF_HIP_CHECK(hipGetLastError());
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
    if ((rc = check_gamma_inputs(ctx, side))) return rc;
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
    const GammaParams<T> p = gamma_params<T>(ctx, side, tl, stats, pr, pw);
    return gamma_launch(ctx, [&](auto L) {
        constexpr int G = 256 / L;
        if (pass == PMF_PASS_FINALIZE) {
            PmfProfScope prof(ctx, PMF_KERNEL_GAMMA_FINAL);
            if (p.rows > p.row0)
                hipLaunchKernelGGL((gamma_finalize_all_kernel<T, L>), dim3((unsigned)((p.rows - p.row0 + G - 1) / G)), dim3(256), 0,
                                   ctx->stream, p);
        } else if (pass == PMF_PASS_ACCUMULATE) {
            launch_gamma<T, L, true, false>(ctx, p, tl);
        } else if (ext) {
            launch_gamma<T, L, false, true>(ctx, p, tl);
        } else {
            launch_gamma<T, L, false, false>(ctx, p, tl);
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

extern "C" int pmf_gamma_sweep(pmf_ctx *ctx, int side, double shape_prior, double rate_prior,
                               int hierarchical, double hyper_shape, double hyper_rate_prior) {
    PMF_SIDE_ENTRY("pmf_gamma_sweep");
    const GammaPriors pr = {shape_prior, rate_prior, hierarchical, hyper_shape, hyper_rate_prior};
    return pmf_with_dtype(ctx, [&](auto t) {
        using T = decltype(t);
        if (side != PMF_SIDE_ITEM || !pmf_comm_active(ctx)) return run_gamma<T>(ctx, side, PMF_PASS_FUSED, false, nullptr, pr);
        // several ranks (pmf_comm.hip): finalize is element-wise (cheap) and writes 3 Kpad + 2 values per row for 2 Kpad of
        // statistics, so the plain all-reduce is the default exchange here
        const PmfExchange ex = {false, pr.hierarchical ? 5 : 3,
                                {PMF_ARR_FACTOR, PMF_ARR_SHAPE, PMF_ARR_RATE, PMF_ARR_PRIOR_RATE, PMF_ARR_HYPER_RATE}};
        int rc;
        if ((rc = pmf_alloc_array(ctx, side, PMF_ARR_SHAPE))) return rc;   // (the gathers address them before finalize runs)
        if ((rc = pmf_alloc_array(ctx, side, PMF_ARR_RATE))) return rc;
        if (pr.hierarchical && (rc = pmf_alloc_array(ctx, side, PMF_ARR_HYPER_RATE))) return rc;
        return pmf_comm_half_sweep(ctx, side, 0, (size_t)2 * ctx->kpad, true, ex,
                                   [&](void *s) { return run_gamma<T>(ctx, side, PMF_PASS_ACCUMULATE, false, s, GammaPriors()); },
                                   [&](void *s) { return run_gamma<T>(ctx, side, PMF_PASS_FINALIZE, false, s, pr); });
    });
}

extern "C" int pmf_gamma_ext_sweep(pmf_ctx *ctx, int side, double shape_prior, double rate_prior) {
    PMF_SIDE_ENTRY("pmf_gamma_ext_sweep");
    PMF_REQUIRE(!pmf_comm_active(ctx), PMF_EINVAL, "pmf_gamma_ext_sweep: the extended model is not available on several ranks");
    const GammaPriors pr = {shape_prior, rate_prior};
    return pmf_with_dtype(ctx, [&](auto t) { return run_gamma<decltype(t)>(ctx, side, PMF_PASS_FUSED, true, nullptr, pr); });
}

extern "C" int pmf_gamma_accumulate(pmf_ctx *ctx, int side, void *stats_dev) {
    PMF_SIDE_ENTRY("pmf_gamma_accumulate");
    PMF_REQUIRE(stats_dev, PMF_EINVAL, "pmf_gamma_accumulate: null stats buffer");
    return pmf_with_dtype(ctx, [&](auto t) { return run_gamma<decltype(t)>(ctx, side, PMF_PASS_ACCUMULATE, false, stats_dev, {}); });
}

extern "C" int pmf_gamma_finalize(pmf_ctx *ctx, int side, const void *stats_dev, double shape_prior,
                                  double rate_prior, int hierarchical, double hyper_shape,
                                  double hyper_rate_prior) {
    PMF_SIDE_ENTRY("pmf_gamma_finalize");
    PMF_REQUIRE(stats_dev, PMF_EINVAL, "pmf_gamma_finalize: null stats buffer");
    const GammaPriors pr = {shape_prior, rate_prior, hierarchical, hyper_shape, hyper_rate_prior};
    return pmf_with_dtype(ctx, [&](auto t) { return run_gamma<decltype(t)>(ctx, side, PMF_PASS_FINALIZE, false, (void *)stats_dev, pr); });
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
