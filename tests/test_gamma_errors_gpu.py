"""Every state and argument error the pmf_gamma_* entry points document (include/pmf_hip.h): the return code, the
COMPLETE pmf_last_error() text, and nothing written -- the model arrays bit for bit as they were, the output and
statistics buffers at their fill value.  The per-feature tests assert fragments of these messages next to the numbers;
this file pins the whole strings and the order in which a call names what it misses, which is what the shared host
code of csrc/pmf_gamma.hip (array requirements, id checks, the launch dispatch) could change without any number moving.

One context shape throughout: 5 users x 4 items, K = 6 (padded to 8: the second lane of a group carries pad
elements), 12 ratings, fp32."""
import ctypes as C

import numpy as np
import pytest

from helpers import DeviceStats

pytestmark = pytest.mark.gpu

PMF_EINVAL, PMF_ERANGE = -1, -4
U, I, K = 5, 4, 6
RU = np.array([0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 4], np.int32)
RI = np.array([0, 1, 3, 1, 2, 0, 3, 2, 3, 0, 1, 2], np.int32)
RX = np.array([1.0, 0.0, 3.0, 2.0, 1.0, 4.0, 1.0, 0.0, 2.0, 5.0, 1.0, 1.0])
FILL = 777.0


class Harness:
    """A context, the arrays put into it so far (side, array) -> bits, and a statistics buffer at FILL."""

    def __init__(self):
        import torch
        import pmf_hip
        self.lib = pmf_hip.load()
        self.ctx = pmf_hip.Context(U, I, K)
        self.h = self.ctx._h
        self.stats = DeviceStats(max(U, I) * 2 * self.ctx.kpad, self.ctx.np_dtype, torch.device("cuda", 0))   # either side's
        self.stats.tensor.fill_(FILL)
        self.sp = C.c_void_p(self.stats.ptr)
        self.held = {}
        self.rng = np.random.default_rng(3)

    def put(self, side, array):
        from pmf_hip import ARR_FACTOR, ARR_RATE, ARR_SHAPE
        rows = (U, I)[side]
        shape = (rows, K) if array in (ARR_FACTOR, ARR_SHAPE, ARR_RATE) else (rows,)
        self.ctx.set_array(side, array, 0.5 + self.rng.random(shape))
        self.held[(side, array)] = self.ctx.get_array(side, array).tobytes()

    def refused(self, rc, code, text):
        """`rc` is what a call just returned: the code, the whole message, and nothing written."""
        assert (rc, self.lib.pmf_last_error().decode()) == (code, text)
        for (side, array), bits in self.held.items():
            assert self.ctx.get_array(side, array).tobytes() == bits, (text, side, array)
        assert bool((self.stats.tensor == FILL).all()), text


@pytest.fixture()
def hx():
    h = Harness()
    yield h
    h.ctx.close()


def _p(a, t):
    from pmf_hip import ptr
    return None if a is None else ptr(a, t)


PRIOR, HIER = (0.3, 1.0, 0, 0.0, 0.0), (0.3, 0.0, 1, 2.1, 1.0)


def test_null_context_and_bad_side(hx):
    lib, sp = hx.lib, hx.sp
    tot = np.full(8, FILL)
    per_side = {
        "pmf_gamma_sweep": lambda h, s: lib.pmf_gamma_sweep(h, s, *PRIOR),
        "pmf_gamma_ext_sweep": lambda h, s: lib.pmf_gamma_ext_sweep(h, s, 0.3, 1.0),
        "pmf_gamma_accumulate": lambda h, s: lib.pmf_gamma_accumulate(h, s, sp),
        "pmf_gamma_finalize": lambda h, s: lib.pmf_gamma_finalize(h, s, sp, *PRIOR),
        "pmf_gamma_exact_sweep": lambda h, s: lib.pmf_gamma_exact_sweep(h, s, *PRIOR),
        "pmf_gamma_exact_accumulate": lambda h, s: lib.pmf_gamma_exact_accumulate(h, s, sp),
        "pmf_gamma_elbo_terms": lambda h, s: lib.pmf_gamma_elbo_terms(h, s, 1, 0, _p(tot, C.c_double), None),
        "pmf_gamma_fold_in": lambda h, s: lib.pmf_gamma_fold_in(h, s, 0, None, None, None, *PRIOR, 1, None, None, None, None, None, None, None),
    }
    for name, call in per_side.items():
        hx.refused(call(None, 0), PMF_EINVAL, f"{name}: null context")
        hx.refused(call(hx.h, 2), PMF_EINVAL, f"{name}: bad side 2")
        hx.refused(call(hx.h, -1), PMF_EINVAL, f"{name}: bad side -1")
    hx.refused(lib.pmf_gamma_predictive(None, 0, None, None, None, 1, None, None, None, None), PMF_EINVAL,
               "pmf_gamma_predictive: null context")
    for name in ("pmf_gamma_accumulate", "pmf_gamma_exact_accumulate"):
        hx.refused(getattr(lib, name)(hx.h, 0, None), PMF_EINVAL, f"{name}: null stats buffer")
    hx.refused(lib.pmf_gamma_finalize(hx.h, 0, None, *PRIOR), PMF_EINVAL, "pmf_gamma_finalize: null stats buffer")
    assert (tot == FILL).all()


def test_reference_sweep_names_what_it_misses_in_order(hx):
    """pmf_gamma_sweep, _ext_sweep and _accumulate share their checks, which speak as pmf_gamma_sweep."""
    from pmf_hip import ARR_FACTOR, ARR_SCALE, ITEM, USER
    lib, h, sp = hx.lib, hx.h, hx.sp

    def all_three(side, text):
        hx.refused(lib.pmf_gamma_sweep(h, side, *PRIOR), PMF_EINVAL, text)
        hx.refused(lib.pmf_gamma_sweep(h, side, *HIER), PMF_EINVAL, text)
        hx.refused(lib.pmf_gamma_ext_sweep(h, side, 0.3, 1.0), PMF_EINVAL, text)
        hx.refused(lib.pmf_gamma_accumulate(h, side, sp), PMF_EINVAL, text)
    all_three(USER, "pmf_gamma_sweep: array FACTOR of side 0 has not been set")
    all_three(ITEM, "pmf_gamma_sweep: array FACTOR of side 1 has not been set")
    hx.put(USER, ARR_FACTOR)
    all_three(USER, "pmf_gamma_sweep: array FACTOR of side 1 has not been set")
    all_three(ITEM, "pmf_gamma_sweep: array FACTOR of side 1 has not been set")
    hx.put(ITEM, ARR_FACTOR)
    all_three(USER, "pmf_gamma_sweep: ratings have not been set")
    all_three(ITEM, "pmf_gamma_sweep: ratings have not been set")
    hx.ctx.set_ratings(RU, RI, RX)
    for side in (USER, ITEM):
        text = f"pmf_gamma_sweep (hierarchical): array PRIOR_RATE of side {side} has not been set"
        hx.refused(lib.pmf_gamma_sweep(h, side, *HIER), PMF_EINVAL, text)
        hx.refused(lib.pmf_gamma_finalize(h, side, sp, *HIER), PMF_EINVAL, text)
    hx.refused(lib.pmf_gamma_ext_sweep(h, USER, 0.3, 1.0), PMF_EINVAL, "pmf_gamma_ext_sweep: array SCALE of side 0 has not been set")
    hx.put(USER, ARR_SCALE)
    hx.refused(lib.pmf_gamma_ext_sweep(h, USER, 0.3, 1.0), PMF_EINVAL, "pmf_gamma_ext_sweep: array SCALE of side 1 has not been set")
    hx.refused(lib.pmf_gamma_ext_sweep(h, ITEM, 0.3, 1.0), PMF_EINVAL, "pmf_gamma_ext_sweep: array SCALE of side 1 has not been set")


def test_exact_elbo_and_predictive_name_what_they_miss_in_order(hx):
    """The three entries that read q = (SHAPE, RATE): the user side's pair first, then the item side's, then the
    ratings, then the hierarchical array -- each under the caller's own name."""
    from pmf_hip import ARR_RATE, ARR_SHAPE, ITEM, USER
    lib, h, sp = hx.lib, hx.h, hx.sp
    tot, rows = np.full(8, FILL), np.full(U * 8, FILL)
    u, i = np.array([0, 1, 2], np.int32), np.array([0, 1, 2], np.int32)
    x, outs = np.array([1.0, 0.0, 3.5]), [np.full(3, FILL), np.full(3, FILL), np.full(9, FILL), np.full(4, FILL)]

    def elbo(side, with_data, hier):
        return lib.pmf_gamma_elbo_terms(h, side, with_data, hier, _p(tot, C.c_double), _p(rows, C.c_double))

    def everyone(text, predictive=True, side=USER):
        hx.refused(lib.pmf_gamma_exact_sweep(h, side, *PRIOR), PMF_EINVAL, "pmf_gamma_exact_sweep: " + text)
        hx.refused(lib.pmf_gamma_exact_sweep(h, side, *HIER), PMF_EINVAL, "pmf_gamma_exact_sweep: " + text)
        hx.refused(lib.pmf_gamma_exact_accumulate(h, side, sp), PMF_EINVAL, "pmf_gamma_exact_accumulate: " + text)
        hx.refused(elbo(side, 1, 1), PMF_EINVAL, "pmf_gamma_elbo_terms: " + text)
        if predictive:
            rc = lib.pmf_gamma_predictive(h, 3, _p(u, C.c_int32), _p(i, C.c_int32), _p(x, C.c_double), 1, *[_p(o, C.c_double) for o in outs])
            hx.refused(rc, PMF_EINVAL, "pmf_gamma_predictive: " + text)
    hx.refused(lib.pmf_gamma_elbo_terms(h, USER, 1, 1, None, _p(rows, C.c_double)), PMF_EINVAL, "pmf_gamma_elbo_terms: null totals")
    everyone("array SHAPE of side 0 has not been set")
    everyone("array SHAPE of side 1 has not been set", predictive=False, side=ITEM)
    hx.put(USER, ARR_SHAPE)
    everyone("array RATE of side 0 has not been set")
    hx.refused(elbo(USER, 0, 0), PMF_EINVAL, "pmf_gamma_elbo_terms: array RATE of side 0 has not been set")
    hx.put(USER, ARR_RATE)
    everyone("array SHAPE of side 1 has not been set")
    hx.refused(elbo(USER, 0, 1), PMF_EINVAL, "pmf_gamma_elbo_terms (hierarchical): array HYPER_RATE of side 0 has not been set")
    hx.put(ITEM, ARR_SHAPE)
    everyone("array RATE of side 1 has not been set")
    everyone("array RATE of side 1 has not been set", predictive=False, side=ITEM)
    hx.put(ITEM, ARR_RATE)
    everyone("ratings have not been set", predictive=False)
    hx.ctx.set_ratings(RU, RI, RX)
    for side in (USER, ITEM):
        hx.refused(lib.pmf_gamma_exact_sweep(h, side, *HIER), PMF_EINVAL,
                   f"pmf_gamma_exact_sweep (hierarchical): array PRIOR_RATE of side {side} has not been set")
        hx.refused(elbo(side, 1, 1), PMF_EINVAL, f"pmf_gamma_elbo_terms (hierarchical): array HYPER_RATE of side {side} has not been set")
    # FACTOR was never set: the fold-in names the OPPOSITE side's
    ptr_, ids, val, out = np.array([0, 2], np.int64), np.array([0, 1], np.int32), np.array([1.0, 2.0]), np.full(K, FILL)
    for side in (USER, ITEM):
        rc = lib.pmf_gamma_fold_in(h, side, 1, _p(ptr_, C.c_int64), _p(ids, C.c_int32), _p(val, C.c_double), *PRIOR, 2, None, None,
                                   _p(out, C.c_double), None, None, None, None)
        hx.refused(rc, PMF_EINVAL, f"pmf_gamma_fold_in: array FACTOR of side {1 - side} has not been set")
    assert all((a == FILL).all() for a in [tot, rows, out] + outs)


def _full(hx):
    from pmf_hip import ARR_FACTOR, ARR_HYPER_RATE, ARR_PRIOR_RATE, ARR_RATE, ARR_SHAPE, ITEM, USER
    for side in (USER, ITEM):
        for array in (ARR_FACTOR, ARR_SHAPE, ARR_RATE, ARR_PRIOR_RATE, ARR_HYPER_RATE):
            hx.put(side, array)
    hx.ctx.set_ratings(RU, RI, RX)


def test_fold_in_argument_errors(hx):
    from pmf_hip import ITEM, USER
    _full(hx)
    lib, h = hx.lib, hx.h
    good_ptr, ids, val = np.array([0, 3, 3, 5], np.int64), np.array([0, 1, 3, 2, 0], np.int32), np.array([1.0, 2.0, 0.0, 1.0, 4.0])
    outs = [np.full(3 * K, FILL), np.full(3 * K, FILL), np.full(3 * K, FILL), np.full(3, FILL), np.full(3, FILL)]

    def call(side=USER, n_rows=3, row_ptr=good_ptr, other=ids, ratings=val, prior=PRIOR, n_iter=2, out_factor=outs[0]):
        return lib.pmf_gamma_fold_in(h, side, n_rows, _p(row_ptr, C.c_int64), _p(other, C.c_int32), _p(ratings, C.c_double), *prior, n_iter,
                                     None, None, _p(out_factor, C.c_double), *[_p(o, C.c_double) for o in outs[1:]])
    for kw, code, text in (
            (dict(n_rows=-1), PMF_EINVAL, "negative row count"),
            (dict(row_ptr=None), PMF_EINVAL, "null argument"),
            (dict(out_factor=None), PMF_EINVAL, "null argument"),
            (dict(row_ptr=np.array([1, 3, 3, 5], np.int64)), PMF_EINVAL, "row_ptr[0] = 1, not 0"),
            (dict(row_ptr=np.array([0, 3, 2, 5], np.int64)), PMF_EINVAL, "row_ptr decreases at row 1"),
            (dict(other=None), PMF_EINVAL, "null argument"),
            (dict(ratings=None), PMF_EINVAL, "null argument"),
            (dict(prior=(0.0, 1.0, 0, 0.0, 0.0)), PMF_EINVAL, "shape_prior must be positive"),
            (dict(prior=(-0.3, 0.0, 1, 2.1, 1.0)), PMF_EINVAL, "shape_prior must be positive"),
            (dict(prior=(0.3, 0.0, 0, 2.1, 1.0)), PMF_EINVAL, "rate_prior must be positive"),
            (dict(prior=(0.3, 1.0, 1, 0.0, 1.0)), PMF_EINVAL, "hyper_shape and hyper_rate_prior must be positive"),
            (dict(prior=(0.3, 1.0, 1, 2.1, -1.0)), PMF_EINVAL, "hyper_shape and hyper_rate_prior must be positive"),
            (dict(n_iter=0), PMF_EINVAL, "n_iter = 0, must be at least 1"),
            (dict(other=np.array([0, 1, I, 2, 0], np.int32)), PMF_ERANGE, f"id {I} at position 2 outside [0, {I})"),
            (dict(other=np.array([0, 1, 3, 2, -1], np.int32)), PMF_ERANGE, f"id -1 at position 4 outside [0, {I})"),
            (dict(side=ITEM, other=np.array([0, U, 3, 2, 0], np.int32)), PMF_ERANGE, f"id {U} at position 1 outside [0, {U})")):
        hx.refused(call(**kw), code, "pmf_gamma_fold_in: " + text)
        assert all((o == FILL).all() for o in outs), text
    assert call(n_rows=0, row_ptr=None, other=None, ratings=None, out_factor=None) == 0      # touches nothing
    assert call() == 0 and not (outs[0] == FILL).any()


def test_predictive_argument_errors(hx):
    _full(hx)
    lib, h = hx.lib, hx.h
    u, i, x = np.array([0, 1, 2], np.int32), np.array([0, 1, 2], np.int32), np.array([1.0, 0.0, 3.5])
    outs = [np.full(3, FILL), np.full(3, FILL), np.full(9, FILL), np.full(4, FILL)]

    def call(n=3, u=u, i=i, x=x, outs=outs):
        return lib.pmf_gamma_predictive(h, n, _p(u, C.c_int32), _p(i, C.c_int32), _p(x, C.c_double), 1, *[_p(o, C.c_double) for o in outs])
    for kw, code, text in (
            (dict(n=-1), PMF_EINVAL, "negative n"),
            (dict(u=None), PMF_EINVAL, "null user_ids"),
            (dict(i=None), PMF_EINVAL, "null item_ids"),
            (dict(outs=[None] * 4), PMF_EINVAL, "no output (out_mean, out_var, out_logp and totals are all null)"),
            (dict(x=None), PMF_EINVAL, "out_logp without ratings"),
            (dict(u=np.array([0, U, 2], np.int32)), PMF_ERANGE, f"user id {U} at position 1 outside [0, {U})"),
            (dict(u=np.array([0, 1, -1], np.int32)), PMF_ERANGE, f"user id -1 at position 2 outside [0, {U})"),
            (dict(i=np.array([0, 1, I], np.int32)), PMF_ERANGE, f"item id {I} at position 2 outside [0, {I})"),
            (dict(i=np.array([-7, 1, 2], np.int32)), PMF_ERANGE, f"item id -7 at position 0 outside [0, {I})"),
            # the pairs are checked in order, a pair's user first
            (dict(u=np.array([0, 1, U], np.int32), i=np.array([0, I, 2], np.int32)), PMF_ERANGE, f"item id {I} at position 1 outside [0, {I})"),
            (dict(u=np.array([0, U, 2], np.int32), i=np.array([0, I, 2], np.int32)), PMF_ERANGE, f"user id {U} at position 1 outside [0, {U})")):
        hx.refused(call(**kw), code, "pmf_gamma_predictive: " + text)
        assert all((o == FILL).all() for o in outs), text
    assert call(n=0, u=None, i=None, x=None, outs=[None] * 4) == 0      # touches nothing
    assert call() == 0 and not any((o == FILL).any() for o in outs)
