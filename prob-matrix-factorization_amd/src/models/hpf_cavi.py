"""Hierarchical Poisson factorisation, CAVI on observed entries -- MI355X engine.

Drop-in for the reference's `src/models/hpf_cavi.py`: same config dataclass,
methods and attributes (`gamma_a_theta, gamma_b_theta, gamma_a_beta,
gamma_b_beta, gamma_a_xi (scalar), gamma_b_xi, gamma_a_eta (scalar),
gamma_b_eta, E_theta, E_beta, E_xi, E_eta`).  Each half-sweep, including the
xi / eta update that follows it, is one `pmf_gamma_sweep(hierarchical=1)`."""
from dataclasses import dataclass
from typing import Optional

import numpy as np

from src.models._device_model import ITEM, USER
from src.models._gamma_host import GammaModel
from pmf_hip import ARR_FACTOR, ARR_HYPER_RATE, ARR_PRIOR_RATE, ARR_RATE, ARR_SHAPE


@dataclass
class HPF_CAVI_Config:
    n_factors: int = 20
    a: float = 0.3
    a_prime: float = 0.3
    b_prime: float = 1.0
    c: float = 0.3
    c_prime: float = 0.3
    d_prime: float = 1.0
    max_iter: int = 100
    tol: Optional[float] = 1e-4
    random_state: int = 42
    verbose: bool = True


class HPF_CAVI(GammaModel):
    """x_ui ~ Poisson(theta_u . beta_i); theta_uk ~ Gamma(a, xi_u), xi_u ~ Gamma(a', b');
    beta_ik ~ Gamma(c, eta_i), eta_i ~ Gamma(c', d')."""
    _iteration_label = "HPF_CAVI iteration"

    def __init__(self, config: HPF_CAVI_Config, dtype=None, device=None, comm=None, presharded=False):
        super().__init__(config, dtype, device, comm, presharded)
        self.gamma_a_theta = self.gamma_b_theta = None
        self.gamma_a_beta = self.gamma_b_beta = None
        self.gamma_a_xi = self.gamma_b_xi = None
        self.gamma_a_eta = self.gamma_b_eta = None
        self.E_theta = self.E_beta = self.E_xi = self.E_eta = None

    def _initialize(self):
        """Reference draw order (hpf_cavi.py:66-89): a_theta, b_theta, a_beta, b_beta."""
        cfg = self.config
        K, N, M = cfg.n_factors, self.n_users, self.n_items
        rng = np.random.default_rng(cfg.random_state)
        users = lambda n: rng.gamma(1.0, 0.1, size=(n, K))      # (a sharded fit keeps this rank's rows only)
        noise = [self._user_rows(users), self._user_rows(users), rng.gamma(1.0, 0.1, size=(M, K)),
                 rng.gamma(1.0, 0.1, size=(M, K))]
        self.gamma_a_theta = cfg.a + noise[0]
        self.gamma_b_theta = cfg.b_prime + noise[1]
        self.gamma_a_beta = cfg.c + noise[2]
        self.gamma_b_beta = cfg.d_prime + noise[3]
        self.gamma_a_xi = cfg.a_prime + K * cfg.a
        self.gamma_b_xi = cfg.b_prime * np.ones(len(noise[0]))
        self.gamma_a_eta = cfg.c_prime + K * cfg.c
        self.gamma_b_eta = cfg.d_prime * np.ones(M)
        self._update_expectations()

    _draw_start = _initialize

    def _update_expectations(self):
        self.E_theta = self.gamma_a_theta / self.gamma_b_theta
        self.E_beta = self.gamma_a_beta / self.gamma_b_beta
        self.E_xi = self.gamma_a_xi / self.gamma_b_xi
        self.E_eta = self.gamma_a_eta / self.gamma_b_eta

    def _upload_start(self, ctx, exact):
        ctx.set_array(USER, ARR_FACTOR, self._mine(self.E_theta))
        ctx.set_array(ITEM, ARR_FACTOR, self.E_beta)
        ctx.set_array(USER, ARR_PRIOR_RATE, self._mine(self.E_xi))
        ctx.set_array(ITEM, ARR_PRIOR_RATE, self.E_eta)
        if exact:      # q is its shapes and rates: the exact update reads them, not FACTOR
            ctx.set_array(USER, ARR_SHAPE, self._mine(self.gamma_a_theta))
            ctx.set_array(USER, ARR_RATE, self._mine(self.gamma_b_theta))
            ctx.set_array(ITEM, ARR_SHAPE, self.gamma_a_beta)
            ctx.set_array(ITEM, ARR_RATE, self.gamma_b_beta)

    def _priors(self):
        """(user, item) prior tuples of `pmf_gamma_sweep` and `pmf_gamma_fold_in`: the shapes of q(xi), q(eta) are fixed."""
        cfg = self.config
        return ((cfg.a, 0.0, True, cfg.a_prime + cfg.n_factors * cfg.a, cfg.b_prime),
                (cfg.c, 0.0, True, cfg.c_prime + cfg.n_factors * cfg.c, cfg.d_prime))

    def _pull_state(self):
        ctx, g = self._ctx, self._user_array
        self.gamma_a_theta, self.gamma_b_theta = g(ARR_SHAPE), g(ARR_RATE)
        self.gamma_a_beta, self.gamma_b_beta = ctx.get_array(ITEM, ARR_SHAPE), ctx.get_array(ITEM, ARR_RATE)
        self.E_theta, self.E_beta = g(ARR_FACTOR), ctx.get_array(ITEM, ARR_FACTOR)
        self.gamma_b_xi, self.gamma_b_eta = g(ARR_HYPER_RATE), ctx.get_array(ITEM, ARR_HYPER_RATE)
        self.E_xi, self.E_eta = g(ARR_PRIOR_RATE), ctx.get_array(ITEM, ARR_PRIOR_RATE)
        if self._comm is not None:
            self._finish_sharded([(USER, ARR_FACTOR, self.E_theta), (ITEM, ARR_FACTOR, self.E_beta)])

    def _elbo_priors(self):
        cfg = self.config
        return (cfg.a, cfg.a_prime, cfg.b_prime), (cfg.c, cfg.c_prime, cfg.d_prime), True
