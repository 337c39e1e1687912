"""Fold-in of unseen users / items for the Poisson MF and HPF classes (extension: the reference serves an unseen id by
refitting).  The rows' updates run on the device (`pmf_gamma_fold_in`, or `pmf_gamma_fold_in_exact` under
`update="exact"`); this module turns a frame into the CSR batch and the result into a `GammaFoldIn` record."""
from dataclasses import dataclass
from typing import Optional

import numpy as np

from src.models._device_model import USER, fold_in_batch


@dataclass
class GammaFoldIn:
    """Variational parameters of folded-in rows (`fold_in_users` / `fold_in_items`): row r belongs to label `ids[r]`."""
    ids: np.ndarray                   # the new side's labels, sorted
    E: np.ndarray                     # (n, K) expected factors, shape / rate
    shape: np.ndarray                 # (n, K)
    rate: np.ndarray                  # (n, K)
    prior_rate: Optional[np.ndarray]  # (n,) E_xi / E_eta of the rows (HPF), None for Poisson MF
    E_other: np.ndarray               # the fitted opposite side's expected factors
    side: int = USER                          # the side the rows belong to
    seen_ptr: Optional[np.ndarray] = None     # the batch `fold_in_batch` built: row r's own ratings are of the ids
    seen_ids: Optional[np.ndarray] = None     # seen_ids[seen_ptr[r]:seen_ptr[r + 1]] on the opposite side
    update: str = "reference"                 # the row update that ran: "reference" or "exact"

    def predict(self, rows, other_ids):
        """E[rows] . E_other[other_ids], on the host."""
        rows, other_ids = np.asarray(rows, dtype=int), np.asarray(other_ids, dtype=int)
        return np.einsum("nk,nk->n", self.E[rows], self.E_other[other_ids])


UPDATES = ("reference", "exact")


def gamma_fold_in(model, side, df, n_iter, prior, update="reference"):
    """`prior` = (shape_prior, rate_prior, hierarchical, hyper_shape, hyper_rate_prior) of `side`, as the model's `fit`
    passes to its half-sweeps.  After a sharded fit `_need_ctx` is the full-size context, which holds both FACTORs and
    nothing else: "reference" runs on it, "exact" -- which reads the opposite side's SHAPE and RATE -- raises
    NotImplementedError."""
    if update not in UPDATES:
        raise ValueError(f"update must be one of {UPDATES}, got {update!r}")
    ctx = model._need_ctx()
    if update == "exact":
        if model._shard_ctx is not None or model._comm is not None:
            raise NotImplementedError('fold-in with update="exact" after a sharded fit: the full-size context holds FACTOR only, '
                                      "not the SHAPE and RATE the exact update reads; the exact fold-in of a sharded fit is not implemented")
        if model.history_["iterations"] == 0:
            raise RuntimeError(f"{type(model).__name__} has run no iteration: SHAPE and RATE were never written, q is not defined")
    ids, row_ptr, other, x = fold_in_batch(df, side, model.n_items if side == USER else model.n_users)
    run = ctx.gamma_fold_in_exact if update == "exact" else ctx.gamma_fold_in
    E, shape, rate, prior_rate, _ = run(side, row_ptr, other, x, *prior, n_iter=n_iter)
    return GammaFoldIn(ids, E, shape, rate, prior_rate, model.E_beta if side == USER else model.E_theta, side, row_ptr, other, update)
