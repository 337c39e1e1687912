"""The exact coordinate-ascent update of the Poisson MF / HPF classes, the part that needs no GPU: `fit(update=)` refuses
an unknown mode and, under "exact", a negative rating, both before a context is opened; the header declares the two
entry points and the binding lists them."""
import os
import re

import pandas as pd
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _models():
    from src.models.hpf_cavi import HPF_CAVI, HPF_CAVI_Config
    from src.models.poisson_mf_cavi import PoissonMFCAVI, PoissonMFCAVIConfig
    return ((PoissonMFCAVI, PoissonMFCAVIConfig), (HPF_CAVI, HPF_CAVI_Config))


def _frame(ratings=(1.0, 2.0)):
    return pd.DataFrame({"u": [0, 1], "i": [1, 0], "rating": list(ratings)})


@pytest.mark.parametrize("which", [0, 1], ids=["poisson", "hpf"])
def test_unknown_update_is_refused_before_a_context_is_opened(which):
    cls, cfg = _models()[which]
    model = cls(cfg(n_factors=4, verbose=False))
    for bad in ("bogus", "Exact", None, 1):
        with pytest.raises(ValueError, match="update must be"):
            model.fit(_frame(), update=bad)
    assert model._ctx is None


@pytest.mark.parametrize("which", [0, 1], ids=["poisson", "hpf"])
def test_exact_update_refuses_a_negative_rating_before_a_context_is_opened(which):
    cls, cfg = _models()[which]
    model = cls(cfg(n_factors=4, verbose=False))
    with pytest.raises(ValueError, match="negative"):
        model.fit(_frame((1.0, -2.0)), update="exact")
    assert model._ctx is None


@pytest.mark.parametrize("which", [0, 1], ids=["poisson", "hpf"])
def test_update_is_keyword_only_and_defaults_to_the_reference(which):
    import inspect
    cls, cfg = _models()[which]
    param = inspect.signature(cls(cfg(n_factors=4, verbose=False)).fit).parameters["update"]
    assert param.kind is inspect.Parameter.KEYWORD_ONLY and param.default == "reference"


def test_header_declares_and_binding_lists_the_two_entry_points():
    import ctypes as C
    import pmf_hip
    with open(os.path.join(ROOT, "include", "pmf_hip.h")) as f:
        header = f.read()
    assert re.search(r"^int pmf_gamma_exact_sweep\(pmf_ctx \*ctx, int side, double shape_prior, double rate_prior,\s+"
                     r"int hierarchical, double hyper_shape, double hyper_rate_prior\);", header, re.M)
    assert re.search(r"^int pmf_gamma_exact_accumulate\(pmf_ctx \*ctx, int side, void \*stats_dev\);", header, re.M)
    assert pmf_hip.SIGNATURES["pmf_gamma_exact_sweep"] == pmf_hip.SIGNATURES["pmf_gamma_sweep"]
    assert pmf_hip.SIGNATURES["pmf_gamma_exact_accumulate"] == (C.c_int, [C.c_void_p, C.c_int, C.c_void_p])
    assert "#define PMF_ABI_VERSION 3" in header


def test_dist_iteration_picks_the_exact_calls():
    """`gamma_iteration(exact=)` on a recording engine: the fused form and the external-collective form."""
    from pmf_hip import ITEM, USER, dist as pdist

    class Engine:
        kpad, n_chunks = 4, {}

        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            return lambda side, *a: self.calls.append((name, side))

    class Stats:
        ptr, tensor = 0, None

    class External:      # a communicator outside the library
        world, in_library = 2, False

        def all_reduce(self, tensor):
            pass
    prior = (0.3, 1.0, False, 0.0, 0.0)
    for exact, sweep, accumulate in ((False, "gamma_sweep", "gamma_accumulate"), (True, "gamma_exact_sweep", "gamma_exact_accumulate")):
        e = Engine()
        pdist.gamma_iteration(e, None, None, prior, prior, exact=exact)
        assert e.calls == [(sweep, USER), (sweep, ITEM)]
        e = Engine()
        pdist.gamma_iteration(e, External(), Stats(), prior, prior, exact=exact)
        assert e.calls == [(sweep, USER), (accumulate, ITEM), ("gamma_finalize", ITEM)]
    e = Engine()
    pdist.gamma_iteration(e, None, None, prior, prior)
    assert e.calls == [("gamma_sweep", USER), ("gamma_sweep", ITEM)]
