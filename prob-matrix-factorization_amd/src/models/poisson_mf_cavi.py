"""Poisson matrix factorisation, CAVI on observed entries -- MI355X engine.

Drop-in for the reference's `src/models/poisson_mf_cavi.py`: same config
dataclass, same `fit` / `predict` / `evaluate_*` signatures, same attributes
(`a_theta, b_theta, a_beta, b_beta, E_theta, E_beta`, float64 NumPy), same
verbose output.  The two half-sweeps per iteration run as HIP kernels
(`pmf_gamma_sweep`)."""
from dataclasses import dataclass
from typing import Optional

import numpy as np

from src.models._device_model import ITEM, USER
from src.models._gamma_host import GammaModel
from pmf_hip import ARR_FACTOR, ARR_RATE, ARR_SHAPE


@dataclass
class PoissonMFCAVIConfig:
    n_factors: int = 20
    a0: float = 0.3
    b0: float = 1.0
    max_iter: int = 100
    tol: Optional[float] = 1e-4
    random_state: int = 42
    verbose: bool = True


class PoissonMFCAVI(GammaModel):
    """x_ij ~ Poisson(theta_i . beta_j), theta, beta ~ Gamma(a0, b0)."""
    _iteration_label = "CAVI iteration"

    def __init__(self, config: PoissonMFCAVIConfig, dtype=None, device=None, comm=None, presharded=False):
        super().__init__(config, dtype, device, comm, presharded)
        self.a_theta = self.b_theta = self.a_beta = self.b_beta = None
        self.E_theta = self.E_beta = None

    def _initialize_variational_params(self):
        """Reference draw order (poisson_mf_cavi.py:50-71): user shapes, item shapes."""
        cfg = self.config
        rng = np.random.default_rng(cfg.random_state)
        self.a_theta = cfg.a0 + self._user_rows(lambda n: rng.gamma(1.0, 0.1, size=(n, cfg.n_factors)))
        self.a_beta = cfg.a0 + rng.gamma(1.0, 0.1, size=(self.n_items, cfg.n_factors))
        self.b_theta = np.full(self.a_theta.shape, float(cfg.b0))
        self.b_beta = np.full((self.n_items, cfg.n_factors), float(cfg.b0))
        self.E_theta = self.a_theta / self.b_theta
        self.E_beta = self.a_beta / self.b_beta

    _draw_start = _initialize_variational_params

    def _upload_start(self, ctx, exact):
        ctx.set_array(USER, ARR_FACTOR, self._mine(self.E_theta))
        ctx.set_array(ITEM, ARR_FACTOR, self.E_beta)
        if exact:      # q is its shapes and rates: the exact update reads them, not FACTOR
            ctx.set_array(USER, ARR_SHAPE, self._mine(self.a_theta))
            ctx.set_array(USER, ARR_RATE, self._mine(self.b_theta))
            ctx.set_array(ITEM, ARR_SHAPE, self.a_beta)
            ctx.set_array(ITEM, ARR_RATE, self.b_beta)

    def _priors(self):
        """(user, item) prior tuples of `pmf_gamma_sweep` and `pmf_gamma_fold_in`."""
        prior = (self.config.a0, self.config.b0, False, 0.0, 0.0)
        return prior, prior

    def _pull_state(self):
        ctx, g = self._ctx, self._user_array
        self.a_theta, self.b_theta = g(ARR_SHAPE), g(ARR_RATE)
        self.a_beta, self.b_beta = ctx.get_array(ITEM, ARR_SHAPE), ctx.get_array(ITEM, ARR_RATE)
        self.E_theta, self.E_beta = g(ARR_FACTOR), ctx.get_array(ITEM, ARR_FACTOR)
        if self._comm is not None:
            self._finish_sharded([(USER, ARR_FACTOR, self.E_theta), (ITEM, ARR_FACTOR, self.E_beta)])

    def _elbo_priors(self):
        cfg = self.config
        return (cfg.a0, cfg.b0), (cfg.a0, cfg.b0), False
