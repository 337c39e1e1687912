"""fp64 NumPy forms of one Gaussian bias half-sweep (gaussian_mf_cavi_bias.py:206-263), for the tests of the
device's sums form (gauss_bias_sums_kernel).

  residual form : num_r = sum_j (x_j - b_o(j) - m_o(j) . m_r)            -- the model's text, one dot per rating
  sums form     : num_r = sum_j (x_j - b_o(j)) - m_r . H_r,  H_r = sum_j m_o(j)

j runs over the ratings of row r AS LISTED: a pair that occurs twice is two ratings and adds its mean row to H twice.
"""
import numpy as np


def bias_numerator_residual(rows, other, x, n_rows, m_self, m_other, b_other):
    """`rows[j]`, `other[j]`: the ids of rating j on this side and on the other one."""
    resid = x - b_other[other] - np.einsum("nk,nk->n", m_other[other], m_self[rows])
    return np.bincount(rows, weights=resid, minlength=n_rows)


def mean_sums(rows, other, n_rows, m_other):
    H = np.zeros((n_rows, m_other.shape[1]))
    np.add.at(H, rows, m_other[other])
    return H


def bias_numerator_sums(rows, other, x, n_rows, m_self, m_other, b_other):
    first = np.bincount(rows, weights=x - b_other[other], minlength=n_rows)
    return first - np.einsum("rk,rk->r", m_self, mean_sums(rows, other, n_rows, m_other))


def bias_from_numerator(num, rows, n_rows, b_self, sigma2, eta_bias2):
    """var = 1 / (1/eta_bias2 + n_r/sigma2), b_r = var/sigma2 * num_r; rows without ratings keep their bias."""
    cnt = np.bincount(rows, minlength=n_rows)
    out = np.array(b_self, dtype=np.float64)
    nz = cnt > 0
    out[nz] = num[nz] / (sigma2 * (1.0 / eta_bias2 + cnt[nz] / sigma2))
    return out


def bias_sweep(rows, other, x, n_rows, m_self, m_other, b_self, b_other, sigma2, eta_bias2, form="residual"):
    f = bias_numerator_residual if form == "residual" else bias_numerator_sums
    num = f(rows, other, np.asarray(x, dtype=np.float64), n_rows, m_self, m_other, b_other)
    return bias_from_numerator(num, rows, n_rows, b_self, sigma2, eta_bias2)
