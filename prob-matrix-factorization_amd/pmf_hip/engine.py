"""`Context`: a thin Python owner of one `pmf_ctx` (one model instance on one GPU).

Every method is a direct call through the C-ABI of include/pmf_hip.h; the
class adds argument conversion (NumPy -> C pointers), error translation and
lifetime management only.
"""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np

from . import (ARR_COV, ELBO_TERMS, EXCHANGE, F32, F64, GAMMA_ELBO_TERMS, GAMMA_PRED_KINDS, GAMMA_PRED_TOTALS, ITEM, KERNEL_NAMES, MAX_LABELS, OP_MAX, OP_SUM, TASK_LISTS, TEST_LIB_PATH,
               UNIQUE_ID_BYTES, USER, ZEROS_MISSING, ZEROS_OBSERVED, PmfError, PmfLibraryError, as_f64, as_i32, check, load, ptr)


def group_rows(row, n):
    """Entries labelled with their row in [0, n) -> (row_ptr int64 [n + 1], order): order[row_ptr[r]:row_ptr[r + 1]] are the
    positions of row r's entries, in input order."""
    row = np.asarray(row).reshape(-1)
    row_ptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=n))]).astype(np.int64)
    return row_ptr, np.argsort(row, kind="stable")


def csr_batch(message, row_ptr, ids=None, what="ids", values=None, n_rows=None):
    """A CSR batch in the ABI's types: [row_ptr as contiguous int64, then `ids` (named `what`) as int32 and `values` as
    float64, each if given].  ValueError(message) unless there are `n_rows` + 1 offsets (None: at least one), the columns
    have one length and the offsets of a batch with rows end at it."""
    rp = np.ascontiguousarray(np.asarray(row_ptr, dtype=np.int64).reshape(-1))
    cols = ([] if ids is None else [as_i32(ids, what)]) + ([] if values is None else [as_f64(values)])
    n = len(rp) - 1 if n_rows is None else n_rows
    if n < 0 or len(rp) != n + 1 or any(len(c) != len(cols[0]) for c in cols) or (cols and n and rp[-1] != len(cols[0])):
        raise ValueError(message)
    return [rp] + cols


def opt_ptr(a, ctype=C.c_double):
    """`ptr`, or None for an array the caller leaves out"""
    return None if a is None else ptr(a, ctype)


def rank_batch(user_ids, item_ids):
    """Flat (user, item) pairs -> the CSR batch `pmf_rank_items` takes: (users, row_ptr, items, order) with `users` the
    sorted distinct user ids, row r holding items[row_ptr[r]:row_ptr[r + 1]] -- user r's items in input order -- and
    `order` the input position of every batch entry: `out[order] = batch_result` undoes the grouping.  Pure NumPy."""
    u, i = np.asarray(user_ids).reshape(-1), np.asarray(item_ids).reshape(-1)
    if len(u) != len(i):
        raise ValueError("user_ids and item_ids must have the same length")
    users, row = np.unique(u, return_inverse=True)
    row_ptr, order = group_rows(row, len(users))
    return users, row_ptr, i[order], order


# what `Context.gamma_predictive` returns: `mean`, `var` [n] and `logp` [n, GAMMA_PRED_KINDS] (None where not asked for or
# not defined), `totals` [GAMMA_PRED_TOTALS]
GammaPredictive = collections.namedtuple("GammaPredictive", "mean var logp totals")


class Context:
    def __init__(self, n_users, n_items, n_factors, dtype="f32", device=0, lib=None):
        """`lib`: another build of the same ABI, already bound (tools/: a yardstick build beside the product's)."""
        self._lib = lib if lib is not None else load()
        self._h = C.c_void_p()
        self.n_users, self.n_items, self.K = int(n_users), int(n_items), int(n_factors)
        self.dtype = {"f32": F32, "f64": F64, F32: F32, F64: F64}[dtype]
        self.np_dtype = np.float64 if self.dtype == F64 else np.float32
        check(self._lib.pmf_ctx_create(int(device), self.n_users, self.n_items, self.K, self.dtype,
                                       C.byref(self._h)), "pmf_ctx_create")
        k = C.c_int(0)
        check(self._lib.pmf_ctx_kpad(self._h, C.byref(k)), "pmf_ctx_kpad")
        self.kpad = k.value
        check(self._lib.pmf_ctx_cov_stride(self._h, C.byref(k)), "pmf_ctx_cov_stride")
        self.cov_stride = k.value
        self.nnz = 0
        self.n_chunks = {USER: 1, ITEM: 1}

    # ---- row chunks (multi-GPU pipelining of a half-sweep) --------------
    def set_row_chunks(self, side, n_chunks):
        """Split `side`'s rows into equal ranges; accumulate / finalize calls then act on the
        range chosen with `select_chunk` (-1 = all rows)."""
        n = max(1, min(int(n_chunks), self.rows(side), 1024))
        check(self._lib.pmf_ctx_set_row_chunks(self._h, side, n), "pmf_ctx_set_row_chunks")
        self.n_chunks[side] = n

    def chunk_rows(self, side, chunk):
        lo, hi = C.c_int64(0), C.c_int64(0)
        check(self._lib.pmf_ctx_chunk_rows(self._h, side, int(chunk), C.byref(lo), C.byref(hi)),
              "pmf_ctx_chunk_rows")
        return lo.value, hi.value

    def select_chunk(self, side, chunk):
        check(self._lib.pmf_ctx_select_chunk(self._h, side, int(chunk)), "pmf_ctx_select_chunk")

    # ---- multi-GPU: the communicator lives inside the library -------------
    @staticmethod
    def comm_unique_id():
        """128 bytes from ncclGetUniqueId (rank 0 creates them, every rank passes them to comm_init)."""
        buf = C.create_string_buffer(UNIQUE_ID_BYTES)
        check(load().pmf_comm_unique_id(buf), "pmf_comm_unique_id")
        return buf.raw

    def comm_init(self, nranks, rank, unique_id, transport="rccl"):
        """Collective.  transport 'rccl' (one rank per GPU), or 'hostshm' -- the rehearsal transport of the TEST build
        of the library (ranks share one GPU), loaded only when the process asked for it (`pmf_hip.wants_test_library`)."""
        if len(unique_id) != UNIQUE_ID_BYTES:
            raise ValueError(f"unique_id must be {UNIQUE_ID_BYTES} bytes")
        if transport == "hostshm":
            if not hasattr(self._lib, "pmf_comm_init_hostshm") or self._lib.pmf_path != TEST_LIB_PATH:
                raise PmfLibraryError("the hostshm transport exists in the test build of the library only: set "
                                      "PMF_COMM_TRANSPORT=hostshm (or PMF_HIP_TEST_LIBRARY=1) before the first engine call")
            fn = self._lib.pmf_comm_init_hostshm
        else:
            fn = {"rccl": self._lib.pmf_comm_init}[transport]
        check(fn(self._h, int(nranks), int(rank), C.c_char_p(bytes(unique_id))), f"pmf_comm_init[{transport}]")

    def comm_set_exchange(self, mode):
        """'auto' (default), 'allreduce' or 'scatter_gather': how an ITEM half-sweep's statistics travel (the same
        on every rank) -- all-reduce + every rank finalises every item, or reduce-scatter -> finalise 1/N of the
        items -> all-gather of the finalised rows."""
        check(self._lib.pmf_comm_set_exchange(self._h, EXCHANGE[mode]), "pmf_comm_set_exchange")

    def comm_attach(self, owner):
        check(self._lib.pmf_comm_attach(self._h, owner._h), "pmf_comm_attach")

    def comm_destroy(self):
        check(self._lib.pmf_comm_destroy(self._h), "pmf_comm_destroy")

    def comm_info(self):
        """(nranks, rank, transport id or -1 without a communicator)"""
        n, r, t = C.c_int(1), C.c_int(0), C.c_int(-1)
        check(self._lib.pmf_comm_info(self._h, C.byref(n), C.byref(r), C.byref(t)), "pmf_comm_info")
        return n.value, r.value, t.value

    def comm_barrier(self):
        check(self._lib.pmf_comm_barrier(self._h), "pmf_comm_barrier")

    def comm_allreduce_host(self, values, op="sum"):
        a = np.array(values, dtype=np.float64, copy=True).reshape(-1)
        check(self._lib.pmf_comm_allreduce_host(self._h, ptr(a, C.c_double), a.size, OP_MAX if op == "max" else OP_SUM),
              "pmf_comm_allreduce_host")
        return a.reshape(np.shape(values))

    def gather_user_rows(self, array, bounds):
        """Every rank's USER rows of `array`, concatenated in rank order (host float64, on every rank)."""
        b = np.ascontiguousarray(np.asarray(bounds, dtype=np.int64))
        total = int(b[-1])
        shape = {2: (total, self.K), 3: (total, self.K, self.K)}.get(len(self._host_shape(USER, array)), (total,))
        out = np.empty(shape, dtype=np.float64)
        check(self._lib.pmf_comm_gather_user_rows(self._h, int(array), ptr(b, C.c_int64), ptr(out, C.c_double)),
              "pmf_comm_gather_user_rows")
        return out

    # ---- lifetime -------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.pmf_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def rows(self, side):
        return self.n_users if side == USER else self.n_items

    def sync(self):
        check(self._lib.pmf_ctx_sync(self._h), "pmf_ctx_sync")

    def set_stream(self, hip_stream):
        check(self._lib.pmf_ctx_set_stream(self._h, C.c_void_p(hip_stream or 0)), "pmf_ctx_set_stream")

    def device_bytes(self):
        n = C.c_int64(0)
        check(self._lib.pmf_ctx_device_bytes(self._h, C.byref(n)), "pmf_ctx_device_bytes")
        return n.value

    def hot_rows(self, side):
        """Row ids of `side` that the opposite side's Gaussian sweep gathers with the default cache policy
        (PMF_GAUSS_HOT_MB), most-rated first."""
        n = C.c_int64(0)
        check(self._lib.pmf_ctx_hot_rows(self._h, side, None, 0, C.byref(n)), "pmf_ctx_hot_rows")
        out = np.empty(n.value, dtype=np.int32)
        check(self._lib.pmf_ctx_hot_rows(self._h, side, out.ctypes.data_as(C.POINTER(C.c_int32)), n.value, C.byref(n)),
              "pmf_ctx_hot_rows")
        return out

    def task_max_len(self, side, kind):
        """Ratings in the longest task of `side`'s work list `kind` ('gamma', 'gauss', 'bias' or 'sgd'): the task
        length in force (by rating count, or PMF_TASK_CHUNK), capped by the longest row."""
        n = C.c_int(0)
        check(self._lib.pmf_ctx_task_max_len(self._h, side, TASK_LISTS[kind], C.byref(n)), "pmf_ctx_task_max_len")
        return n.value

    # ---- data -----------------------------------------------------------
    def set_ratings(self, user_ids, item_ids, ratings, weights=None):
        """`weights` (one per rating, finite and > 0): the Gaussian CAVI calls give rating j the precision
        weights[j] / sigma2 (`pmf_ctx_set_ratings_weighted`); None clears them."""
        u, i, x = as_i32(user_ids, "user_ids"), as_i32(item_ids, "item_ids"), as_f64(ratings)
        if not (len(u) == len(i) == len(x)):
            raise ValueError("user_ids, item_ids and ratings must have the same length")
        if weights is None:
            check(self._lib.pmf_ctx_set_ratings(self._h, len(u), ptr(u, C.c_int32), ptr(i, C.c_int32),
                                                ptr(x, C.c_double)), "pmf_ctx_set_ratings")
        else:
            w = as_f64(weights)
            if len(w) != len(x):
                raise ValueError("weights must have one entry per rating")
            check(self._lib.pmf_ctx_set_ratings_weighted(self._h, len(u), ptr(u, C.c_int32), ptr(i, C.c_int32),
                                                         ptr(x, C.c_double), ptr(w, C.c_double)),
                  "pmf_ctx_set_ratings_weighted")
        self.nnz = len(u)

    @property
    def rating_weights(self):
        """Whether the context's ratings came with weights."""
        has = C.c_int(0)
        check(self._lib.pmf_ctx_has_rating_weights(self._h, C.byref(has)), "pmf_ctx_has_rating_weights")
        return bool(has.value)

    def rating_weight_sums(self, side):
        """C_r of every row of `side`: the sum of its ratings' weights as the kernels read it (summed in double, rounded
        once to the context dtype); the rating counts without weights."""
        out = np.zeros(self.rows(side), dtype=np.float64)
        check(self._lib.pmf_ctx_rating_weight_sums(self._h, side, ptr(out, C.c_double)), "pmf_ctx_rating_weight_sums")
        return out

    def side_ratings(self, side, weights=True):
        """The ratings as `side` holds them, read back from the device (`pmf_ctx_side_ratings`): (row_ptr int64
        [rows + 1], other_ids int32 [nnz], ratings float64 [nnz], weights float64 [nnz] or None without `weights`) --
        after `gauss_logit_refresh(side)` the refreshed values."""
        rp = np.zeros(self.rows(side) + 1, dtype=np.int64)
        other = np.zeros(self.nnz, dtype=np.int32)
        x = np.zeros(self.nnz, dtype=np.float64)
        w = np.zeros(self.nnz, dtype=np.float64) if weights else None
        check(self._lib.pmf_ctx_side_ratings(self._h, side, ptr(rp, C.c_int64), ptr(other, C.c_int32), ptr(x, C.c_double),
                                             opt_ptr(w)), "pmf_ctx_side_ratings")
        return rp, other, x, w

    def _host_shape(self, side, array):
        r = self.rows(side)
        if array in (0, 1, 2):
            return (r, self.K)
        if array == ARR_COV:
            return (r, self.K, self.K)
        return (r,)

    def set_array(self, side, array, host):
        a = as_f64(host)
        if a.shape != self._host_shape(side, array):
            raise ValueError(f"array {array} of side {side}: expected shape "
                             f"{self._host_shape(side, array)}, got {a.shape}")
        check(self._lib.pmf_set_array(self._h, side, array, ptr(a, C.c_double)), "pmf_set_array")

    def get_array(self, side, array):
        out = np.empty(self._host_shape(side, array), dtype=np.float64)
        check(self._lib.pmf_get_array(self._h, side, array, ptr(out, C.c_double)), "pmf_get_array")
        return out

    def get_array_rows(self, side, array, rows):
        """The given rows of `array` as host float64 (len(rows) x K, len(rows) or len(rows) x K x K):
        `V_theta[rows]` without the 32 GB stack."""
        r = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1))
        out = np.empty((len(r),) + self._host_shape(side, array)[1:], dtype=np.float64)
        check(self._lib.pmf_get_array_rows(self._h, side, array, len(r), ptr(r, C.c_int64), ptr(out, C.c_double)),
              "pmf_get_array_rows")
        return out

    def set_array_rows(self, side, array, rows, host):
        r = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).reshape(-1))
        a = as_f64(host)
        want = (len(r),) + self._host_shape(side, array)[1:]
        if a.shape != want:
            raise ValueError(f"array {array} of side {side}: expected shape {want}, got {a.shape}")
        check(self._lib.pmf_set_array_rows(self._h, side, array, len(r), ptr(r, C.c_int64), ptr(a, C.c_double)),
              "pmf_set_array_rows")

    def set_cov_identity(self, side, scale=1.0):
        check(self._lib.pmf_set_cov_identity(self._h, side, float(scale)), "pmf_set_cov_identity")

    # ---- Poisson / HPF --------------------------------------------------
    def gamma_sweep(self, side, shape_prior, rate_prior, hierarchical=False, hyper_shape=0.0,
                    hyper_rate_prior=0.0):
        check(self._lib.pmf_gamma_sweep(self._h, side, float(shape_prior), float(rate_prior),
                                        int(bool(hierarchical)), float(hyper_shape),
                                        float(hyper_rate_prior)), "pmf_gamma_sweep")

    def gamma_ext_sweep(self, side, shape_prior, rate_prior):
        check(self._lib.pmf_gamma_ext_sweep(self._h, side, float(shape_prior), float(rate_prior)),
              "pmf_gamma_ext_sweep")

    def gamma_fold_in(self, side, row_ptr, other_ids, ratings, shape_prior, rate_prior=0.0, hierarchical=False, hyper_shape=0.0,
                      hyper_rate_prior=0.0, n_iter=10, init_factor=None, init_prior_rate=None, want_params=True):
        """Variational parameters of new rows of `side` (CSR batch: `row_ptr`, ids on the opposite side, ratings) after
        `n_iter` row updates against the fitted opposite side (`pmf_gamma_fold_in`; priors as for `gamma_sweep`):
        (factor [n, K], shape [n, K], rate [n, K], prior_rate [n], hyper_rate [n]) as float64.  `shape` and `rate` are None
        unless `want_params`, `prior_rate` and `hyper_rate` are None unless `hierarchical`.  `init_factor` [n, K] /
        `init_prior_rate` [n] warm-start the rows.  The context is only read."""
        rp, o, x = csr_batch("row_ptr must hold n_rows + 1 offsets ending at len(other_ids) == len(ratings)", row_ptr,
                             other_ids, "other_ids", ratings)
        n = len(rp) - 1
        init_f = None if init_factor is None else as_f64(init_factor)
        init_r = None if init_prior_rate is None else as_f64(init_prior_rate)
        if init_f is not None and init_f.shape != (n, self.K):
            raise ValueError(f"init_factor: expected shape {(n, self.K)}, got {init_f.shape}")
        if init_r is not None and init_r.shape != (n,):
            raise ValueError(f"init_prior_rate: expected shape {(n,)}, got {init_r.shape}")
        hier = bool(hierarchical)
        factor = np.zeros((n, self.K), dtype=np.float64)
        shape = np.zeros((n, self.K), dtype=np.float64) if want_params else None
        rate = np.zeros((n, self.K), dtype=np.float64) if want_params else None
        prior_rate = np.zeros(n, dtype=np.float64) if hier else None
        hyper_rate = np.zeros(n, dtype=np.float64) if hier else None
        check(self._lib.pmf_gamma_fold_in(self._h, side, n, ptr(rp, C.c_int64), ptr(o, C.c_int32), ptr(x, C.c_double),
                                          float(shape_prior), float(rate_prior), int(hier), float(hyper_shape),
                                          float(hyper_rate_prior), int(n_iter), opt_ptr(init_f), opt_ptr(init_r), ptr(factor, C.c_double),
                                          opt_ptr(shape), opt_ptr(rate), opt_ptr(prior_rate), opt_ptr(hyper_rate)), "pmf_gamma_fold_in")
        return factor, shape, rate, prior_rate, hyper_rate

    def gamma_fold_in_exact(self, side, row_ptr, other_ids, ratings, shape_prior, rate_prior=0.0, hierarchical=False, hyper_shape=0.0,
                            hyper_rate_prior=0.0, n_iter=10, init_shape=None, init_rate=None, init_prior_rate=None, want_params=True):
        """`gamma_fold_in` with the update of `gamma_exact_sweep` (`pmf_gamma_fold_in_exact`): `n_iter` passes of coordinate
        ascent on the bound against the opposite side's q, read from its SHAPE and RATE (FACTOR is not needed).  The same
        five results.  `init_shape` / `init_rate` [n, K] (both or neither) and `init_prior_rate` [n] warm-start the rows.
        The context is only read."""
        rp, o, x = csr_batch("row_ptr must hold n_rows + 1 offsets ending at len(other_ids) == len(ratings)", row_ptr,
                             other_ids, "other_ids", ratings)
        n = len(rp) - 1
        init_s = None if init_shape is None else as_f64(init_shape)
        init_b = None if init_rate is None else as_f64(init_rate)
        init_r = None if init_prior_rate is None else as_f64(init_prior_rate)
        for name, a in (("init_shape", init_s), ("init_rate", init_b)):
            if a is not None and a.shape != (n, self.K):
                raise ValueError(f"{name}: expected shape {(n, self.K)}, got {a.shape}")
        if init_r is not None and init_r.shape != (n,):
            raise ValueError(f"init_prior_rate: expected shape {(n,)}, got {init_r.shape}")
        hier = bool(hierarchical)
        factor = np.zeros((n, self.K), dtype=np.float64)
        shape = np.zeros((n, self.K), dtype=np.float64) if want_params else None
        rate = np.zeros((n, self.K), dtype=np.float64) if want_params else None
        prior_rate = np.zeros(n, dtype=np.float64) if hier else None
        hyper_rate = np.zeros(n, dtype=np.float64) if hier else None
        check(self._lib.pmf_gamma_fold_in_exact(self._h, side, n, ptr(rp, C.c_int64), ptr(o, C.c_int32), ptr(x, C.c_double),
                                                float(shape_prior), float(rate_prior), int(hier), float(hyper_shape),
                                                float(hyper_rate_prior), int(n_iter), opt_ptr(init_s), opt_ptr(init_b), opt_ptr(init_r),
                                                ptr(factor, C.c_double), opt_ptr(shape), opt_ptr(rate), opt_ptr(prior_rate),
                                                opt_ptr(hyper_rate)), "pmf_gamma_fold_in_exact")
        return factor, shape, rate, prior_rate, hyper_rate

    def gamma_elbo_terms(self, side, with_data=False, hierarchical=False, per_row=False):
        """The sums of `side` the Poisson MF / HPF ELBO is assembled from (`pmf_gamma_elbo_terms`; columns
        `pmf_hip.GAMMA_ELBO_*`): the totals [GAMMA_ELBO_TERMS] as float64 and, when asked, the (rows, GAMMA_ELBO_TERMS)
        per-row array as well.  DATA and LOGFACT are zero unless `with_data`, the three HYPER columns unless
        `hierarchical`.  The context is only read."""
        totals = np.zeros(GAMMA_ELBO_TERMS, dtype=np.float64)
        rows = np.zeros((self.rows(side), GAMMA_ELBO_TERMS), dtype=np.float64) if per_row else None
        check(self._lib.pmf_gamma_elbo_terms(self._h, side, int(bool(with_data)), int(bool(hierarchical)), ptr(totals, C.c_double),
                                             ptr(rows, C.c_double) if per_row else None), "pmf_gamma_elbo_terms")
        return (totals, rows) if per_row else totals

    def gamma_accumulate(self, side, stats_ptr):
        check(self._lib.pmf_gamma_accumulate(self._h, side, C.c_void_p(stats_ptr)), "pmf_gamma_accumulate")

    def gamma_finalize(self, side, stats_ptr, shape_prior, rate_prior, hierarchical=False,
                       hyper_shape=0.0, hyper_rate_prior=0.0):
        check(self._lib.pmf_gamma_finalize(self._h, side, C.c_void_p(stats_ptr), float(shape_prior),
                                           float(rate_prior), int(bool(hierarchical)),
                                           float(hyper_shape), float(hyper_rate_prior)),
              "pmf_gamma_finalize")

    def gamma_exact_sweep(self, side, shape_prior, rate_prior, hierarchical=False, hyper_shape=0.0,
                          hyper_rate_prior=0.0):
        """`gamma_sweep` with the weights of exact coordinate ascent on the bound (`pmf_gamma_exact_sweep`): reads SHAPE
        and RATE of both sides, not FACTOR."""
        check(self._lib.pmf_gamma_exact_sweep(self._h, side, float(shape_prior), float(rate_prior),
                                              int(bool(hierarchical)), float(hyper_shape),
                                              float(hyper_rate_prior)), "pmf_gamma_exact_sweep")

    def gamma_exact_accumulate(self, side, stats_ptr):
        """The raw sums of `gamma_exact_sweep` in `gamma_accumulate`'s layout; `gamma_finalize` finalises them."""
        check(self._lib.pmf_gamma_exact_accumulate(self._h, side, C.c_void_p(stats_ptr)), "pmf_gamma_exact_accumulate")

    # ---- Poisson / HPF with unlisted cells counted as zeros (implicit feedback) ----
    def set_gamma_zeros(self, observed):
        """`observed=True`: the Poisson MF / HPF calls of this context count every (user, item) cell without a rating
        as a count of 0 (`pmf_ctx_set_gamma_zeros`, PMF_ZEROS_OBSERVED) -- the sweeps, the fold-in and the ELBO's data
        term; `False` (the default of a new context): only the listed ratings are data.  Not available with a communicator,
        nor for the accumulate / finalize pair and the extended model."""
        check(self._lib.pmf_ctx_set_gamma_zeros(self._h, ZEROS_OBSERVED if observed else ZEROS_MISSING), "pmf_ctx_set_gamma_zeros")

    @property
    def gamma_zeros(self):
        """True when unlisted cells count as zeros."""
        mode = C.c_int(0)
        check(self._lib.pmf_ctx_get_gamma_zeros(self._h, C.byref(mode)), "pmf_ctx_get_gamma_zeros")
        return mode.value == ZEROS_OBSERVED

    def gamma_column_sums(self, side, from_q=False):
        """[K] float64: the sum over all rows of `side` of FACTOR, or with `from_q` of SHAPE / RATE as the (E log, E)
        tables hold it (`pmf_gamma_column_sums`); summed in double on the device, the same bits on every call."""
        out = np.zeros(self.K, dtype=np.float64)
        check(self._lib.pmf_gamma_column_sums(self._h, side, int(bool(from_q)), ptr(out, C.c_double)), "pmf_gamma_column_sums")
        return out

    def gamma_predictive(self, user_ids, item_ids, ratings=None, with_bound=True, per_pair=True):
        """Posterior predictive of the Poisson MF / HPF models for the pairs (`pmf_gamma_predictive`; q is SHAPE and RATE
        of both sides): a `GammaPredictive` with `mean` = E[theta_u . beta_i] and `var` = Var[theta_u . beta_i] (float64
        [n]), `logp` [n, GAMMA_PRED_KINDS] -- the PLUGIN, BOUND and NEGBIN log densities of `ratings`, columns
        `pmf_hip.GAMMA_PRED_*`; None without ratings -- and `totals` [GAMMA_PRED_TOTALS] = sum of var, then of every
        column (NaN where there is none).  Without `with_bound` no table is built and the BOUND column and total are NaN;
        without `per_pair` only `totals` is formed (`mean`, `var`, `logp` are None).  Every id must lie inside the trained
        dimensions.  The context is only read."""
        u, i = as_i32(user_ids, "user_ids"), as_i32(item_ids, "item_ids")
        if len(u) != len(i):
            raise ValueError("user_ids and item_ids must have the same length")
        x = None if ratings is None else as_f64(ratings)
        if x is not None and x.shape != (len(u),):
            raise ValueError("ratings must have the length of user_ids")
        n = len(u)
        mean = np.zeros(n, dtype=np.float64) if per_pair else None
        var = np.zeros(n, dtype=np.float64) if per_pair else None
        logp = np.zeros((n, GAMMA_PRED_KINDS), dtype=np.float64) if per_pair and x is not None else None
        totals = np.full(GAMMA_PRED_TOTALS, np.nan, dtype=np.float64)
        totals[0] = 0.0
        if x is not None:
            totals[1:] = 0.0
            if not with_bound:
                totals[2] = np.nan
        check(self._lib.pmf_gamma_predictive(self._h, n, ptr(u, C.c_int32), ptr(i, C.c_int32), opt_ptr(x), int(bool(with_bound)),
                                             opt_ptr(mean), opt_ptr(var), opt_ptr(logp), ptr(totals, C.c_double)), "pmf_gamma_predictive")
        return GammaPredictive(mean, var, logp, totals)

    # ---- Gaussian -------------------------------------------------------
    def gauss_factor_sweep(self, side, sigma2, eta2):
        check(self._lib.pmf_gauss_factor_sweep(self._h, side, float(sigma2), float(eta2)),
              "pmf_gauss_factor_sweep")

    def gauss_bias_sweep(self, side, sigma2, eta_bias2):
        check(self._lib.pmf_gauss_bias_sweep(self._h, side, float(sigma2), float(eta_bias2)),
              "pmf_gauss_bias_sweep")

    def gauss_factor_accumulate(self, side, stats_ptr):
        check(self._lib.pmf_gauss_factor_accumulate(self._h, side, C.c_void_p(stats_ptr)),
              "pmf_gauss_factor_accumulate")

    def gauss_factor_finalize(self, side, stats_ptr, sigma2, eta2):
        check(self._lib.pmf_gauss_factor_finalize(self._h, side, C.c_void_p(stats_ptr), float(sigma2),
                                                  float(eta2)), "pmf_gauss_factor_finalize")

    def gauss_bias_accumulate(self, side, stats_ptr):
        check(self._lib.pmf_gauss_bias_accumulate(self._h, side, C.c_void_p(stats_ptr)),
              "pmf_gauss_bias_accumulate")

    def gauss_bias_finalize(self, side, stats_ptr, sigma2, eta_bias2):
        check(self._lib.pmf_gauss_bias_finalize(self._h, side, C.c_void_p(stats_ptr), float(sigma2),
                                                float(eta_bias2)), "pmf_gauss_bias_finalize")

    def gauss_fold_in(self, side, row_ptr, other_ids, ratings, sigma2, eta2, eta_bias2=1.0, n_iter=1, want_cov=True,
                      weights=None):
        """Posterior of new rows of `side` (CSR batch: `row_ptr`, ids on the opposite side, ratings) against the
        fitted opposite side: (factor [n, K], cov [n, K, K] or None, bias [n]) as float64.  The context is only read.
        `weights`: one confidence weight per rating of the batch (`pmf_gauss_fold_in_weighted`)."""
        rp, o, x = csr_batch("row_ptr must hold n_rows + 1 offsets ending at len(other_ids) == len(ratings)", row_ptr,
                             other_ids, "other_ids", ratings)
        n = len(rp) - 1
        factor = np.zeros((n, self.K), dtype=np.float64)
        cov = np.zeros((n, self.K, self.K), dtype=np.float64) if want_cov else None
        bias = np.zeros(n, dtype=np.float64)
        if weights is not None:
            w = as_f64(weights)
            if len(w) != len(x):
                raise ValueError("weights must have one entry per rating of the batch")
            check(self._lib.pmf_gauss_fold_in_weighted(self._h, side, n, ptr(rp, C.c_int64), ptr(o, C.c_int32),
                                                       ptr(x, C.c_double), ptr(w, C.c_double), float(sigma2), float(eta2),
                                                       float(eta_bias2), int(n_iter), ptr(factor, C.c_double),
                                                       ptr(cov, C.c_double) if want_cov else None, ptr(bias, C.c_double)),
                  "pmf_gauss_fold_in_weighted")
            return factor, cov, bias
        check(self._lib.pmf_gauss_fold_in(self._h, side, n, ptr(rp, C.c_int64), ptr(o, C.c_int32), ptr(x, C.c_double),
                                          float(sigma2), float(eta2), float(eta_bias2), int(n_iter), ptr(factor, C.c_double),
                                          ptr(cov, C.c_double) if want_cov else None, ptr(bias, C.c_double)),
              "pmf_gauss_fold_in")
        return factor, cov, bias

    def gauss_elbo_terms(self, side, with_data=False, per_row=False):
        """The sums of `side` the Gaussian ELBO is assembled from (`pmf_gauss_elbo_terms`; columns `pmf_hip.ELBO_*`):
        the totals [ELBO_TERMS] as float64 and, when asked, the (rows, ELBO_TERMS) per-row array as well.  The ESS column
        is the data term and is zero unless `with_data`.  The context is only read."""
        totals = np.zeros(ELBO_TERMS, dtype=np.float64)
        rows = np.zeros((self.rows(side), ELBO_TERMS), dtype=np.float64) if per_row else None
        check(self._lib.pmf_gauss_elbo_terms(self._h, side, int(bool(with_data)), ptr(totals, C.c_double),
                                             ptr(rows, C.c_double) if per_row else None), "pmf_gauss_elbo_terms")
        return (totals, rows) if per_row else totals

    def gauss_logit_refresh(self, side, want_data_term=True):
        """Logistic model on the Gaussian path (`pmf_gauss_logit_refresh`): every Jaakkola-Jordan parameter of `side`'s
        stream to its optimum under the current FACTOR / COV, the stream's weights and ratings rewritten to c_j = 2
        lambda(xi_j) and (x_j - 1/2) / c_j, so that `gauss_factor_sweep(side, 1.0, eta2)` is the logistic factor update.
        Returns the data term of the bound (float), or None without `want_data_term` (the call then does not wait)."""
        d = np.zeros(1, dtype=np.float64)
        check(self._lib.pmf_gauss_logit_refresh(self._h, side, ptr(d, C.c_double) if want_data_term else None),
              "pmf_gauss_logit_refresh")
        return float(d[0]) if want_data_term else None

    def gauss_sample_rows(self, side, rows, n_draws=1, draw0=0, seed=0, z=None):
        """Posterior draws x = FACTOR[r] + chol(COV[r]) z of the given rows of `side` (`pmf_gauss_sample_rows`): float64
        [len(rows), n_draws, K].  Draw d has draw index `draw0` + d of the counter-based stream under `seed` (any integer
        in [0, 2^64)); the normals are a function of (seed, side, row id, draw index, k) alone.  `z` [len(rows), n_draws,
        K] replaces the stream.  Rows may repeat.  Biases are not sampled.  The context is only read."""
        r = as_i32(np.asarray(rows).reshape(-1), "rows")
        n_draws = int(n_draws)
        zz = None
        if z is not None:
            zz = as_f64(z)
            if zz.shape != (len(r), n_draws, self.K):
                raise ValueError(f"z: expected shape {(len(r), n_draws, self.K)}, got {zz.shape}")
        out = np.empty((len(r), max(n_draws, 0), self.K), dtype=np.float64)
        check(self._lib.pmf_gauss_sample_rows(self._h, side, len(r), ptr(r, C.c_int32), n_draws, int(draw0), C.c_uint64(int(seed)),
                                              opt_ptr(zz), ptr(out, C.c_double)), "pmf_gauss_sample_rows")
        return out

    # ---- bias-free Gaussian model with unlisted cells counted as weighted zeros (implicit feedback) ----
    def set_gauss_zeros(self, observed, weight=1.0):
        """`observed=True`: `gauss_factor_sweep`, `gauss_fold_in` and `gauss_elbo_terms(with_data=True)` of this context
        count every (user, item) cell without a rating as an observation of 0 with variance sigma2 / `weight`, `weight`
        in (0, 1] (`pmf_ctx_set_gauss_zeros`, PMF_ZEROS_OBSERVED); `False` (the default of a new context): only the listed
        ratings are data, and `weight` is ignored.  Not available with a communicator, for the bias model, the
        accumulate / finalize pairs and the gradient mode."""
        check(self._lib.pmf_ctx_set_gauss_zeros(self._h, ZEROS_OBSERVED if observed else ZEROS_MISSING, float(weight)),
              "pmf_ctx_set_gauss_zeros")

    @property
    def gauss_zeros(self):
        """(observed, weight): whether unlisted cells count as weighted zeros, and the stored weight (1.0 by default)."""
        mode = C.c_int(0)
        weight = np.zeros(1, dtype=np.float64)
        check(self._lib.pmf_ctx_get_gauss_zeros(self._h, C.byref(mode), ptr(weight, C.c_double)), "pmf_ctx_get_gauss_zeros")
        return mode.value == ZEROS_OBSERVED, float(weight[0])

    def gauss_gram(self, side):
        """(K, K) float64, symmetric: the sum over ALL rows of `side` of COV[r] + FACTOR[r] FACTOR[r]^T (`pmf_gauss_gram`);
        summed in double on the device, the same bits on every call.  The context is only read."""
        out = np.zeros((self.K, self.K), dtype=np.float64)
        check(self._lib.pmf_gauss_gram(self._h, side, ptr(out, C.c_double)), "pmf_gauss_gram")
        return out

    # ---- Gaussian MAP by gradient steps (no reference counterpart) -------
    def gauss_sgd_sweep(self, side, lr, sigma2, eta2, eta_bias2=1.0):
        check(self._lib.pmf_gauss_sgd_sweep(self._h, side, float(lr), float(sigma2), float(eta2), float(eta_bias2)),
              "pmf_gauss_sgd_sweep")

    @property
    def sgd_stats_width(self):
        w = C.c_int(0)
        check(self._lib.pmf_ctx_sgd_stats_width(self._h, C.byref(w)), "pmf_ctx_sgd_stats_width")
        return w.value

    def gauss_sgd_accumulate(self, side, stats_ptr, lr, sigma2, eta2, eta_bias2=1.0):
        check(self._lib.pmf_gauss_sgd_accumulate(self._h, side, C.c_void_p(stats_ptr), float(lr), float(sigma2),
                                                 float(eta2), float(eta_bias2)), "pmf_gauss_sgd_accumulate")

    def gauss_sgd_finalize(self, side, stats_ptr):
        check(self._lib.pmf_gauss_sgd_finalize(self._h, side, C.c_void_p(stats_ptr)), "pmf_gauss_sgd_finalize")

    # ---- predict / evaluate --------------------------------------------
    @staticmethod
    def _clip_ids(ids):
        """Ids beyond int32 cannot be valid rows; map them to an id that is
        out of range for every table so they predict 0 like the reference."""
        a = np.asarray(ids, dtype=np.int64)
        big = np.iinfo(np.int32).max
        return np.ascontiguousarray(np.where((a > big) | (a < 0), big, a).astype(np.int32))

    def predict(self, user_ids, item_ids, use_bias=False, offset=0.0):
        u, i = self._clip_ids(user_ids), self._clip_ids(item_ids)
        if len(u) != len(i):
            raise ValueError("user_ids and item_ids must have the same length")
        out = np.zeros(len(u), dtype=np.float64)
        if len(u):
            check(self._lib.pmf_predict(self._h, len(u), ptr(u, C.c_int32), ptr(i, C.c_int32),
                                        int(use_bias), float(offset), ptr(out, C.c_double)),
                  "pmf_predict")
        return out

    def eval_set(self, user_ids, item_ids, y_true, labels=None):
        """Store a validation set on the device.  Returns False (and stores
        nothing) when y_true has more than MAX_LABELS distinct values -- the
        caller then evaluates through `predict`.  `labels` (sorted distinct
        values) fixes the label set, e.g. to the global one of a sharded run."""
        y = as_f64(y_true)
        if labels is None:
            labels, inverse = np.unique(y, return_inverse=True)
        else:
            labels = np.asarray(labels, dtype=np.float64)
            inverse = np.searchsorted(labels, y)
        if len(labels) > MAX_LABELS or len(y) == 0:
            return False
        u, i = self._clip_ids(user_ids), self._clip_ids(item_ids)
        lab = np.ascontiguousarray(inverse.astype(np.int32))
        check(self._lib.pmf_eval_set(self._h, len(y), ptr(u, C.c_int32), ptr(i, C.c_int32),
                                     ptr(y, C.c_double), ptr(lab, C.c_int32), len(labels)),
              "pmf_eval_set")
        self._eval_n, self._eval_labels = len(y), len(labels)
        return True

    def eval_sums(self, use_bias=False, offset=0.0):
        """Raw reductions over the stored validation set: [n, sum sq err, per-label
        sum |err| (MAX_LABELS), per-label count (MAX_LABELS)] as one float64 vector
        (additive across the shards of a multi-GPU run)."""
        sse = C.c_double(0.0)
        abs_l = np.zeros(MAX_LABELS, dtype=np.float64)
        cnt_l = np.zeros(MAX_LABELS, dtype=np.int64)
        check(self._lib.pmf_eval_run(self._h, int(use_bias), float(offset), C.byref(sse),
                                     ptr(abs_l, C.c_double), ptr(cnt_l, C.c_int64)), "pmf_eval_run")
        return np.concatenate([[float(self._eval_n), sse.value], abs_l, cnt_l.astype(np.float64)])

    @staticmethod
    def metrics_from_sums(sums):
        """(rmse, macro_mae) from an `eval_sums` vector (metrics.py:6-10, :37-51)."""
        n, sse = sums[0], sums[1]
        abs_l, cnt_l = sums[2:2 + MAX_LABELS], sums[2 + MAX_LABELS:2 + 2 * MAX_LABELS]
        seen = cnt_l > 0
        return float(np.sqrt(sse / n)), float(np.mean(abs_l[seen] / cnt_l[seen]))

    def eval_run(self, use_bias=False, offset=0.0):
        """(rmse, macro_mae) over the stored validation set."""
        return self.metrics_from_sums(self.eval_sums(use_bias, offset))

    def predict_var(self, user_ids, item_ids):
        """Var[theta_u . beta_i] under the Gaussian posterior (FACTOR and COV of both sides), float64; 0 for ids
        outside the trained dimensions.  The rating's predictive variance adds sigma2."""
        u, i = self._clip_ids(user_ids), self._clip_ids(item_ids)
        if len(u) != len(i):
            raise ValueError("user_ids and item_ids must have the same length")
        out = np.zeros(len(u), dtype=np.float64)
        if len(u):
            check(self._lib.pmf_predict_var(self._h, len(u), ptr(u, C.c_int32), ptr(i, C.c_int32), ptr(out, C.c_double)),
                  "pmf_predict_var")
        return out

    def eval_var_sums(self, use_bias=False, offset=0.0, sigma2=1.0):
        """(n, sum of Var[f], sum of the log predictive density N(y; predict, sigma2 + Var[f])) over the stored
        validation set (additive across the shards of a multi-GPU run)."""
        sv, sl = C.c_double(0.0), C.c_double(0.0)
        check(self._lib.pmf_eval_run_var(self._h, int(use_bias), float(offset), float(sigma2), C.byref(sv), C.byref(sl)),
              "pmf_eval_run_var")
        return getattr(self, "_eval_n", 0), sv.value, sl.value

    def topk_items(self, user_ids, k, use_bias=False, exclude_train=False):
        """`use_bias`: False / 0, PREDICT_BIAS (scores + b_u + b_i) or PREDICT_SCALE (scores * s_u * s_i):
        the same flag `predict` takes, so the ranking follows the model's own score.  Returns (items int32 [n, k],
        scores float64 [n, k]), best first, -1 / 0.0 where fewer than k items rank.  `exclude_train`: the user's training
        items (each once) are no candidates (`pmf_topk_items_excluding`): column p holds the item whose
        `rank_items(.., exclude_train=True)` rank is p."""
        u = as_i32(user_ids, "user_ids")
        items = np.empty((len(u), k), dtype=np.int32)
        scores = np.empty((len(u), k), dtype=np.float64)
        if exclude_train:
            check(self._lib.pmf_topk_items_excluding(self._h, len(u), ptr(u, C.c_int32), int(k), int(use_bias), 1,
                                                     ptr(items, C.c_int32), ptr(scores, C.c_double)), "pmf_topk_items_excluding")
        else:
            check(self._lib.pmf_topk_items(self._h, len(u), ptr(u, C.c_int32), int(k), int(use_bias),
                                           ptr(items, C.c_int32), ptr(scores, C.c_double)), "pmf_topk_items")
        return items, scores

    def rank_rows(self, user_ids, row_ptr, item_ids, use_bias=False, exclude_train=False):
        """`pmf_rank_items` on a CSR batch: row r is user user_ids[r] (repeats allowed) with the targets
        item_ids[row_ptr[r]:row_ptr[r + 1]].  Returns (ranks int64 [len(item_ids)], candidates int64 [len(user_ids)])."""
        u, i = as_i32(user_ids, "user_ids"), as_i32(item_ids, "item_ids")
        rp, = csr_batch("row_ptr must hold len(user_ids) + 1 offsets", row_ptr, n_rows=len(u))
        ranks = np.empty(len(i), dtype=np.int64)
        cand = np.empty(len(u), dtype=np.int64)
        check(self._lib.pmf_rank_items(self._h, len(u), ptr(u, C.c_int32), ptr(rp, C.c_int64), ptr(i, C.c_int32), int(use_bias),
                                       int(bool(exclude_train)), ptr(ranks, C.c_int64), ptr(cand, C.c_int64)), "pmf_rank_items")
        return ranks, cand

    def rank_items(self, user_ids, item_ids, use_bias=False, exclude_train=False):
        """0-based rank of every pair's item among its user's candidate items under `predict`'s score (`use_bias` as for
        `topk_items`; ties to the lower item id; -1 where the pair's own score is NaN) and the user's number of
        candidates, both int64 and aligned with the input pairs.  `exclude_train`: the user's training items (each once)
        are no competitors and no candidates."""
        users, row_ptr, items, order = rank_batch(user_ids, item_ids)
        r, c = self.rank_rows(users, row_ptr, items, use_bias, exclude_train)
        ranks = np.empty(len(order), dtype=np.int64)
        cand = np.empty(len(order), dtype=np.int64)
        ranks[order] = r
        cand[order] = np.repeat(c, np.diff(row_ptr))
        return ranks, cand

    # ---- any query rows against one side --------------------------------
    def _query_args(self, cand_side, ids, query_side, factor, coef, exclude):
        """The arguments `pmf_topk_query` and `pmf_rank_query` share (the arrays are returned too: ctypes keeps no
        reference to them)."""
        if (ids is None) == (factor is None):
            raise ValueError("exactly one of `ids` (rows of the context) and `factor` (the caller's rows) names the query rows")
        keep = []
        if ids is not None:
            q = as_i32(np.asarray(ids).reshape(-1), "ids")
            n, side = len(q), (1 - cand_side) if query_side is None else int(query_side)
            q_ids, q_factor, q_coef = ptr(q, C.c_int32), None, None
            keep.append(q)
        else:
            f = as_f64(factor)
            if f.ndim != 2 or f.shape[1] != self.K:
                raise ValueError(f"factor must be [n, {self.K}], got {f.shape}")
            n, side, q_ids, q_factor, q_coef = len(f), 0, None, ptr(f, C.c_double), None
            keep.append(f)
            if coef is not None:
                c = as_f64(np.asarray(coef).reshape(-1))
                if len(c) != n:
                    raise ValueError("coef must hold one value per row of factor")
                q_coef = ptr(c, C.c_double)
                keep.append(c)
        ex_ptr = ex_ids = None
        if exclude is not None:
            ep, ei = csr_batch("exclude must be (row_ptr, ids): one offset per query row and one more, ending at len(ids)", exclude[0],
                               np.asarray(exclude[1]).reshape(-1), "exclude ids", n_rows=n)
            ex_ptr, ex_ids = ptr(ep, C.c_int64), ptr(ei, C.c_int32)
            keep += [ep, ei]
        return n, (int(cand_side), n, side, q_ids, q_factor, q_coef), (ex_ptr, ex_ids), keep

    def topk_query(self, cand_side, k, *, ids=None, query_side=None, factor=None, coef=None, score=0, exclude=None):
        """The k best rows of `cand_side` for every query row (`pmf_topk_query`): (ids int32 [n, k], scores float64 [n, k]),
        best first, -1 / 0.0 where fewer than k rank.  The query rows are rows `ids` of `query_side` (default: the side
        opposite to `cand_side`) or the caller's `factor` [n, K] with `coef` [n] as their bias / scale.  `score`: 0,
        PREDICT_BIAS, PREDICT_SCALE or SCORE_COSINE.  `exclude` = (row_ptr, ids): candidate ids that are no candidates of
        query ROW q, in any order."""
        n, query, ex, keep = self._query_args(cand_side, ids, query_side, factor, coef, exclude)
        out_ids = np.empty((n, k), dtype=np.int32)
        out_scores = np.empty((n, k), dtype=np.float64)
        check(self._lib.pmf_topk_query(self._h, *query, int(score), *ex, int(k), ptr(out_ids, C.c_int32),
                                       ptr(out_scores, C.c_double)), "pmf_topk_query")
        return out_ids, out_scores

    def topk_sampled(self, cand_side, k, ids, *, query_side=None, score=0, exclude=None, seed=0, draw=0):
        """`topk_query` in ids mode scored on one joint posterior draw of the Gaussian factors (`pmf_topk_sampled`): every
        row of `cand_side` and the query rows `ids` of `query_side` are replaced by their draw with index `draw` under
        `seed` -- row (side, id) by `gauss_sample_rows(side, [id], 1, draw, seed)` to the bit -- and biases stay at their
        means.  `score`: 0 or PREDICT_BIAS.  Returns (ids int32 [n, k], scores float64 [n, k])."""
        n, query, ex, keep = self._query_args(cand_side, ids, query_side, None, None, exclude)
        out_ids = np.empty((n, k), dtype=np.int32)
        out_scores = np.empty((n, k), dtype=np.float64)
        check(self._lib.pmf_topk_sampled(self._h, *query[:4], int(score), *ex, int(k), C.c_uint64(int(seed)), int(draw),
                                         ptr(out_ids, C.c_int32), ptr(out_scores, C.c_double)), "pmf_topk_sampled")
        return out_ids, out_scores

    def rank_query(self, cand_side, targets, *, ids=None, query_side=None, factor=None, coef=None, score=0, exclude=None):
        """`pmf_rank_query`: `targets` = (row_ptr, ids), the rows of `cand_side` whose ranks query row q asks for.  Returns
        (ranks int64 [len(target ids)], candidates int64 [n]); the other arguments are those of `topk_query`."""
        n, query, ex, keep = self._query_args(cand_side, ids, query_side, factor, coef, exclude)
        tp, ti = csr_batch("targets must be (row_ptr, ids): one offset per query row and one more, ending at len(ids)", targets[0],
                           np.asarray(targets[1]).reshape(-1), "target ids", n_rows=n)
        ranks = np.empty(len(ti), dtype=np.int64)
        cand = np.empty(n, dtype=np.int64)
        check(self._lib.pmf_rank_query(self._h, *query, int(score), *ex, ptr(tp, C.c_int64), ptr(ti, C.c_int32),
                                       ptr(ranks, C.c_int64), ptr(cand, C.c_int64)), "pmf_rank_query")
        return ranks, cand

    def rank_query_pairs(self, cand_side, rows, target_ids, *, ids=None, query_side=None, factor=None, coef=None, score=0,
                         exclude=None):
        """`rank_query` on flat pairs, in the manner of `rank_items`: pair p asks for the rank of candidate target_ids[p]
        for query row rows[p] (an index into `ids` / `factor`).  Returns (ranks, candidates), int64, aligned with the pairs."""
        rows = np.asarray(rows, dtype=np.int64).reshape(-1)
        tgt = np.asarray(target_ids).reshape(-1)
        if len(rows) != len(tgt):
            raise ValueError("rows and target_ids must have the same length")
        n = len(ids) if ids is not None else len(factor)
        if len(rows) and (rows.min() < 0 or rows.max() >= n):
            raise ValueError("rows must index the query rows")
        row_ptr, order = group_rows(rows, n)
        r, c = self.rank_query(cand_side, (row_ptr, tgt[order]), ids=ids, query_side=query_side, factor=factor, coef=coef,
                               score=score, exclude=exclude)
        ranks = np.empty(len(rows), dtype=np.int64)
        ranks[order] = r
        return ranks, c[rows]

    # ---- profiling ------------------------------------------------------
    def prof_enable(self, on=True):
        check(self._lib.pmf_prof_enable(self._h, int(bool(on))), "pmf_prof_enable")

    def prof_reset(self):
        check(self._lib.pmf_prof_reset(self._h), "pmf_prof_reset")

    def gather_ceiling_ms(self, side, repeats=5):
        """Average ms of the gather-only twin of the Poisson/HPF half-sweep of `side` (its roofline)."""
        ms = C.c_double(0.0)
        check(self._lib.pmf_prof_gather_ceiling(self._h, side, int(repeats), C.byref(ms)), "pmf_prof_gather_ceiling")
        return ms.value

    def prof_get(self):
        """{kernel_name: (total_ms, launches)} since the last reset."""
        out = {}
        for k, name in enumerate(KERNEL_NAMES):
            ms, n = C.c_double(0.0), C.c_int64(0)
            check(self._lib.pmf_prof_get(self._h, k, C.byref(ms), C.byref(n)), "pmf_prof_get")
            out[name] = (ms.value, n.value)
        return out


__all__ = ["Context", "GammaPredictive", "PmfError", "USER", "ITEM", "rank_batch"]
