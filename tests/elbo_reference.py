"""Dense NumPy references for the evidence lower bound of the Gaussian models (tests/test_elbo_cpu.py,
tests/test_elbo_gpu.py).  Everything here works on full K x K matrices, per-row or per-rating Python loops and
`np.linalg.slogdet`; nothing is shared with the packed walk of csrc/pmf_gauss.hip or with `elbo_from_terms`."""
import numpy as np

SQNORM, LOGDET, BIAS_SQ, ESS = 0, 1, 2, 3


def row_lists(ids, n_rows):
    """positions of every row's ratings, in input order"""
    order = np.argsort(np.asarray(ids, dtype=np.int64), kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=n_rows))])
    return [order[ptr[r]:ptr[r + 1]] for r in range(n_rows)]


def row_stats(m_o, V_o, ids, other_ids, n_rows, acc=np.float64):
    """per row of a side: (S_r, sum_j |V_o| + |m_o m_o'|) over its ratings, or None for a row without ratings -- the part
    of the statistics that does not depend on the biases"""
    m_o, V_o = np.asarray(m_o).astype(acc), np.asarray(V_o).astype(acc)
    aV, out = np.abs(V_o), []
    for sel in row_lists(ids, n_rows):
        if len(sel) == 0:
            out.append(None)
            continue
        o = other_ids[sel]
        times = np.bincount(o, minlength=len(m_o)).astype(acc)      # a pair rated twice counts twice
        mo = m_o[o]
        out.append((np.tensordot(times, V_o, 1) + mo.T @ mo,
                    (np.tensordot(times, aV, 1) + np.abs(mo).T @ np.abs(mo)).astype(np.float64)))
    return out


def side_terms(m, V, b, m_o, V_o, b_o, ids, other_ids, x, acc=np.float64, stats=None):
    """(rows, 4) per-row terms of one side from the row statistics S_r, w_r, c_r, and the (rows,) magnitude of the ESS:
    the sum of the absolute values of every product that enters it, with the rating-level sums behind S, w and c taken
    in absolute value too.  `b` / `b_o` are zeros for the bias-free model.  Sums in `acc`.  `stats` = row_stats(...)
    of the same state, to share it between calls that differ in the biases only."""
    rows, K = m.shape
    stats = row_stats(m_o, V_o, ids, other_ids, rows, acc) if stats is None else stats
    m, V, b, m_o, b_o, x = (np.asarray(t).astype(acc) for t in (m, V, b, m_o, b_o, x))
    out, mag = np.zeros((rows, 4), acc), np.zeros(rows)
    for r, sel in enumerate(row_lists(ids, rows)):
        out[r, SQNORM] = (m[r] * m[r]).sum() + np.trace(V[r])
        sign, ld = np.linalg.slogdet(V[r].astype(np.float64))
        out[r, LOGDET] = ld if sign > 0 else np.nan
        out[r, BIAS_SQ] = b[r] * b[r]
        if len(sel) == 0:
            continue
        o = other_ids[sel]
        e = x[sel] - b[r] - b_o[o]
        mo = m_o[o]
        S, Sa = stats[r]
        w = (mo * e[:, None]).sum(axis=0)
        c = (e * e).sum()
        second = V[r] + np.multiply.outer(m[r], m[r])
        out[r, ESS] = c - 2.0 * (m[r] * w).sum() + (second * S).sum()
        ea = np.abs(x[sel]) + np.abs(b[r]) + np.abs(b_o[o])
        wa = (np.abs(mo) * ea[:, None]).sum(axis=0)
        seconda = np.abs(V[r]) + np.abs(np.multiply.outer(m[r], m[r]))
        mag[r] = float((ea * ea).sum() + 2.0 * (np.abs(m[r]) * wa).sum() + (seconda * Sa).sum())
    return out, mag


def ess_per_rating(mu, Vu, bu, mi, Vi, bi, u, i, x, acc=np.float64):
    """sum over the ratings of  e_j^2 + Var_j:  e_j = x_j - b_u - b_i - m_u . m_i,
    Var_j = m_u' V_i m_u + m_i' V_u m_i + tr(V_u V_i)"""
    mu, Vu, bu, mi, Vi, bi, x = (np.asarray(t).astype(acc) for t in (mu, Vu, bu, mi, Vi, bi, x))
    total = acc(0)
    for a, c, y in zip(u, i, x):
        e = y - bu[a] - bi[c] - (mu[a] * mi[c]).sum()
        var = mu[a] @ Vi[c] @ mu[a] + mi[c] @ Vu[a] @ mi[c] + (Vu[a] * Vi[c].T).sum()
        total += e * e + var
    return total


def elbo(st, u, i, x, sigma2, eta_theta2, eta_beta2, eta_bias2=None, data="ratings"):
    """The ELBO of the state `st` (m_theta, V_theta, m_beta, V_beta and, with `eta_bias2`, m_user_bias / m_item_bias),
    written out block by block: E_q log p(x | .) + sum over blocks of E_q log p(block) + H[q(block)].  `data` picks
    how the expected squared residual is formed: per rating, or from the user / item row statistics."""
    mu, Vu, mi, Vi = st["m_theta"], st["V_theta"], st["m_beta"], st["V_beta"]
    U, K = mu.shape
    I = mi.shape[0]
    bias = eta_bias2 is not None
    bu = st["m_user_bias"] if bias else np.zeros(U)
    bi = st["m_item_bias"] if bias else np.zeros(I)
    nu, ni = np.bincount(u, minlength=U), np.bincount(i, minlength=I)
    if data == "ratings":
        ess = float(ess_per_rating(mu, Vu, bu, mi, Vi, bi, u, i, x))
    elif data == "user":
        ess = float(side_terms(mu, Vu, bu, mi, Vi, bi, u, i, x)[0][:, ESS].sum())
    else:
        ess = float(side_terms(mi, Vi, bi, mu, Vu, bu, i, u, x)[0][:, ESS].sum())
    if bias:
        vu, vi = 1.0 / (1.0 / eta_bias2 + nu / sigma2), 1.0 / (1.0 / eta_bias2 + ni / sigma2)
        ess += float((nu * vu).sum() + (ni * vi).sum())
    L = -0.5 * len(x) * np.log(2 * np.pi * sigma2) - ess / (2 * sigma2)
    for m, V, eta2 in ((mu, Vu, eta_theta2), (mi, Vi, eta_beta2)):
        for r in range(len(m)):
            second = (m[r] * m[r]).sum() + np.trace(V[r])
            L += -0.5 * K * np.log(2 * np.pi * eta2) - second / (2 * eta2)              # E_q log N(row; 0, eta2 I)
            L += 0.5 * K * (1 + np.log(2 * np.pi)) + 0.5 * np.linalg.slogdet(V[r])[1]   # entropy of N(m, V)
    if bias:
        for b, v in ((bu, vu), (bi, vi)):
            L += float((-0.5 * np.log(2 * np.pi * eta_bias2) - (b * b + v) / (2 * eta_bias2)).sum())
            L += float((0.5 * (1 + np.log(2 * np.pi * v))).sum())
    return float(L)
