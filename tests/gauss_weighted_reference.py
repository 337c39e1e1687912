"""Dense float64 NumPy restatement of the Gaussian CAVI calls with a confidence weight per rating
(`pmf_ctx_set_ratings_weighted`, include/pmf_hip.h): rating j has precision c_j / sigma2,

    x_j ~ N(b_r + b_o + theta_r . beta_o, sigma2 / c_j),   c_j > 0.

Written from the formulae there with full K x K matrices and Python loops over rows and ratings; nothing is shared with
the packed walk of csrc/pmf_gauss.hip, with `elbo_from_terms` or with oracle/cavi_oracle.py.  With A_o = V_o + m_o m_o':

    S_r = sum_j c_j A_{o_j}     w_r = sum_j c_j m_{o_j} (x_j - b_r - b_{o_j})     C_r = sum_j c_j
    V_r = inv(I / eta2 + S_r / sigma2)     m_r = V_r w_r / sigma2                  (rows without ratings keep their state)
    var_r = 1 / (1 / eta_bias2 + C_r / sigma2)     b_r = var_r / sigma2 * sum_j c_j (x_j - b_{o_j} - m_{o_j} . m_r)
    c_r = sum_j c_j (x_j - b_r - b_{o_j})^2        ESS_r = c_r - 2 m_r . w_r + <V_r + m_r m_r', S_r>

and, with unlisted cells counted as zeros of weight w0 (bias-free): S'_r = sum_j (c_j - w0) A_{o_j} + w0 G for EVERY row.

A state is a dict m_theta, V_theta, m_beta, V_beta, b_user, b_item (the biases are zeros in the bias-free model)."""
import numpy as np

SQNORM, LOGDET, BIAS_SQ, ESS = 0, 1, 2, 3
WEIGHTS = (0.25, 0.5, 1.0, 2.0, 4.0)   # exact in fp32: converting them adds no error


def rows_of(ids, n_rows):
    """positions of every row's ratings, in input order"""
    out = [[] for _ in range(n_rows)]
    for k, r in enumerate(ids):
        out[int(r)].append(k)
    return out


def problem(seed, U=90, I=70, N=4000, unique=False):
    """(u, i, x, c): N ratings (duplicate pairs unless `unique`), centred real ratings, weights from WEIGHTS; user 1 and
    item 2 have no ratings, the last ids occur."""
    rng = np.random.default_rng(seed)
    u, i = rng.integers(0, U, N), rng.integers(0, I, N)
    u[u == 1], i[i == 2] = 0, 0
    u[0], i[0] = U - 1, I - 1
    if unique:
        _, first = np.unique(u * I + i, return_index=True)
        u, i = u[np.sort(first)], i[np.sort(first)]
    x = rng.normal(0.0, 1.0, len(u))
    c = rng.choice(WEIGHTS, len(u))
    return u.astype(np.int64), i.astype(np.int64), x - x.mean(), c


def initial_state(seed, U, I, K, bias=False):
    rng = np.random.default_rng(seed)
    st = {"m_theta": 0.1 * rng.standard_normal((U, K)), "V_theta": np.tile(np.eye(K), (U, 1, 1)),
          "m_beta": 0.1 * rng.standard_normal((I, K)), "V_beta": np.tile(np.eye(K), (I, 1, 1)),
          "b_user": np.zeros(U), "b_item": np.zeros(I)}
    if bias:
        st["b_user"], st["b_item"] = 0.1 * rng.standard_normal(U), 0.1 * rng.standard_normal(I)
    return st


def row_stats(m_o, V_o, b_self, b_o, ids, other_ids, x, c, n_rows, w0=0.0):
    """per row a dict: n, S = sum (c_j - w0) A_j, Sa = sum |c_j - w0| (|V_j| + |m_j| |m_j|'), w, wa = sum c_j |m_j| (|x_j|
    + |b_r| + |b_o|), C = sum c_j, csq = sum c_j e_j^2, csqa = sum c_j (|x_j| + |b_r| + |b_o|)^2 -- rating by rating."""
    K = m_o.shape[1]
    out = []
    for r, sel in enumerate(rows_of(ids, n_rows)):
        S, Sa, w, wa = np.zeros((K, K)), np.zeros((K, K)), np.zeros(K), np.zeros(K)
        C = csq = csqa = 0.0
        for k in sel:
            o = int(other_ids[k])
            outer = np.multiply.outer(m_o[o], m_o[o])
            S += (c[k] - w0) * (V_o[o] + outer)
            Sa += abs(c[k] - w0) * (np.abs(V_o[o]) + np.abs(outer))
            e = x[k] - b_self[r] - b_o[o]
            ea = abs(x[k]) + abs(b_self[r]) + abs(b_o[o])
            w += c[k] * m_o[o] * e
            wa += c[k] * np.abs(m_o[o]) * ea
            C += c[k]
            csq += c[k] * e * e
            csqa += c[k] * ea * ea
        out.append({"n": len(sel), "S": S, "Sa": Sa, "w": w, "wa": wa, "C": C, "csq": csq, "csqa": csqa})
    return out


def gram(m, V):
    """(G, sum_r |V_r| + |m_r| |m_r|'): G = sum over ALL rows of V_r + m_r m_r'"""
    K = m.shape[1]
    G, Ga = np.zeros((K, K)), np.zeros((K, K))
    for r in range(len(m)):
        outer = np.multiply.outer(m[r], m[r])
        G += V[r] + outer
        Ga += np.abs(V[r]) + np.abs(outer)
    return G, Ga


def solve_row(S, w, sigma2, eta2):
    V = np.linalg.inv(np.eye(len(w)) / eta2 + S / sigma2)
    V = 0.5 * (V + V.T)
    return V @ w / sigma2, V


def factor_sweep(m, V, m_o, V_o, b_self, b_o, ids, other_ids, x, c, sigma2, eta2, w0=None):
    """one side's factor half-sweep; w0 = None: the default mode (rows without ratings keep their state), else zero mode
    with weight w0: every row, S' = sum (c_j - w0) A_j + w0 G"""
    m, V = m.copy(), V.copy()
    G = gram(m_o, V_o)[0] if w0 is not None else None
    for r, s in enumerate(row_stats(m_o, V_o, b_self, b_o, ids, other_ids, x, c, len(m), w0 or 0.0)):
        if w0 is not None:
            m[r], V[r] = solve_row(s["S"] + w0 * G, s["w"], sigma2, eta2)
        elif s["n"]:
            m[r], V[r] = solve_row(s["S"], s["w"], sigma2, eta2)
    return m, V


def bias_sweep(b_self, b_o, m_self, m_o, ids, other_ids, x, c, sigma2, eta_bias2):
    out = b_self.copy()
    for r, sel in enumerate(rows_of(ids, len(b_self))):
        if not sel:
            continue
        C = tot = 0.0
        for k in sel:
            o = int(other_ids[k])
            C += c[k]
            tot += c[k] * (x[k] - b_o[o] - (m_o[o] * m_self[r]).sum())
        var = 1.0 / (1.0 / eta_bias2 + C / sigma2)
        out[r] = var / sigma2 * tot
    return out


def half_steps(st, u, i, x, c, sigma2, eta_theta2, eta_beta2, eta_bias2=None, w0=None):
    """the states after every half-sweep of one iteration, in the models' order: user factors, item factors, then (bias
    model) user biases, item biases"""
    st = dict(st)
    for name, other, b, bo, ids, oids, eta2 in (("theta", "beta", "b_user", "b_item", u, i, eta_theta2),
                                              ("beta", "theta", "b_item", "b_user", i, u, eta_beta2)):
        st["m_" + name], st["V_" + name] = factor_sweep(st["m_" + name], st["V_" + name], st["m_" + other], st["V_" + other],
                                                        st[b], st[bo], ids, oids, x, c, sigma2, eta2, w0)
        yield dict(st)
    if eta_bias2 is not None:
        st["b_user"] = bias_sweep(st["b_user"], st["b_item"], st["m_theta"], st["m_beta"], u, i, x, c, sigma2, eta_bias2)
        yield dict(st)
        st["b_item"] = bias_sweep(st["b_item"], st["b_user"], st["m_beta"], st["m_theta"], i, u, x, c, sigma2, eta_bias2)
        yield dict(st)


def iterate(st, *args, **kw):
    for st in half_steps(st, *args, **kw):
        pass
    return st


def fold_in(m_o, V_o, b_o, row_ptr, other_ids, x, c, sigma2, eta2, eta_bias2=None, n_iter=1, w0=None):
    """(m [n, K], V [n, K, K], b [n]) of the rows of a CSR batch against the other side, by the literal alternation:
    b = 0; n_iter times: m = V sum_j c_j m_j (x_j - b - b_o) / sigma2, then (bias model) b = kappa sum_j c_j (x_j - b_o -
    m_j . m).  A row without ratings gets the prior (zero mode: inv(I / eta2 + w0 G / sigma2), mean 0)."""
    n, K = len(row_ptr) - 1, m_o.shape[1]
    G = gram(m_o, V_o)[0] if w0 is not None else None
    m, V, b = np.zeros((n, K)), np.zeros((n, K, K)), np.zeros(n)
    for r in range(n):
        sel = range(int(row_ptr[r]), int(row_ptr[r + 1]))
        S = np.zeros((K, K)) if w0 is None else w0 * G
        for k in sel:
            o = int(other_ids[k])
            S = S + (c[k] - (w0 or 0.0)) * (V_o[o] + np.multiply.outer(m_o[o], m_o[o]))
        if len(sel) == 0 and w0 is None:
            V[r] = eta2 * np.eye(K)
            continue
        V[r] = solve_row(S, np.zeros(K), sigma2, eta2)[1]
        C = sum(c[k] for k in sel)
        for _ in range(n_iter if eta_bias2 is not None else 1):
            w = np.zeros(K)
            for k in sel:
                o = int(other_ids[k])
                w += c[k] * m_o[o] * (x[k] - b[r] - b_o[o])
            m[r] = V[r] @ w / sigma2
            if eta_bias2 is not None:
                tot = sum(c[k] * (x[k] - b_o[int(other_ids[k])] - (m_o[int(other_ids[k])] * m[r]).sum()) for k in sel)
                b[r] = tot / (sigma2 * (1.0 / eta_bias2 + C / sigma2))
    return m, V, b


def side_terms(m, V, b, m_o, V_o, b_o, ids, other_ids, x, c, w0=None):
    """(rows, 4) per-row ELBO terms of a side and the (rows,) magnitude of the ESS: the sum of the absolute values of
    every product that enters it (the rating-level sums behind S, w and c_r in absolute value too).  Default mode: a row
    without ratings has ESS 0; zero mode: every row, with S' = S + w0 G."""
    rows = len(m)
    out, mag = np.zeros((rows, 4)), np.zeros(rows)
    G, Ga = gram(m_o, V_o) if w0 is not None else (0.0, 0.0)
    for r, s in enumerate(row_stats(m_o, V_o, b, b_o, ids, other_ids, x, c, rows, w0 or 0.0)):
        out[r, SQNORM] = (m[r] * m[r]).sum() + np.trace(V[r])
        sign, ld = np.linalg.slogdet(V[r])
        out[r, LOGDET] = ld if sign > 0 else np.nan
        out[r, BIAS_SQ] = b[r] * b[r]
        if s["n"] == 0 and w0 is None:
            continue
        second = V[r] + np.multiply.outer(m[r], m[r])
        seconda = np.abs(V[r]) + np.abs(np.multiply.outer(m[r], m[r]))
        Sp, Spa = (s["S"], s["Sa"]) if w0 is None else (s["S"] + w0 * G, s["Sa"] + w0 * Ga)
        out[r, ESS] = s["csq"] - 2.0 * (m[r] * s["w"]).sum() + (second * Sp).sum()
        mag[r] = s["csqa"] + 2.0 * (np.abs(m[r]) * s["wa"]).sum() + (seconda * Spa).sum()
    return out, mag


def weight_sums(ids, c, n_rows):
    return np.array([sum(c[k] for k in sel) for sel in rows_of(ids, n_rows)], dtype=np.float64)


def _prior_entropy(st, u, i, c, sigma2, eta_theta2, eta_beta2, eta_bias2):
    L = 0.0
    for m, V, eta2 in ((st["m_theta"], st["V_theta"], eta_theta2), (st["m_beta"], st["V_beta"], eta_beta2)):
        K = m.shape[1]
        for r in range(len(m)):
            second = (m[r] * m[r]).sum() + np.trace(V[r])
            L += -0.5 * K * np.log(2 * np.pi * eta2) - second / (2 * eta2)              # E_q log N(row; 0, eta2 I)
            L += 0.5 * K * (1 + np.log(2 * np.pi)) + 0.5 * np.linalg.slogdet(V[r])[1]   # entropy of N(m, V)
    if eta_bias2 is not None:
        for b, ids in ((st["b_user"], u), (st["b_item"], i)):
            v = bias_variances(ids, c, len(b), sigma2, eta_bias2)
            L += float((-0.5 * np.log(2 * np.pi * eta_bias2) - (b * b + v) / (2 * eta_bias2)).sum())
            L += float((0.5 * (1 + np.log(2 * np.pi * v))).sum())
    return L


def bias_variances(ids, c, n_rows, sigma2, eta_bias2):
    """v_r = 1 / (1 / eta_bias2 + C_r / sigma2): eta_bias2 for a row without ratings"""
    return 1.0 / (1.0 / eta_bias2 + weight_sums(ids, c, n_rows) / sigma2)


def elbo_ratings(st, u, i, x, c, sigma2, eta_theta2, eta_beta2, eta_bias2=None, w0=None):
    """The bound with the data term formed rating by rating (and, in zero mode, cell by cell): every observation y with
    weight c contributes  -1/2 log(2 pi sigma2 / c) - c / (2 sigma2) [ (y - mu)^2 + Var[f] + v_u + v_i ],  Var[f] =
    m_u' V_i m_u + m_i' V_u m_i + tr(V_u V_i) (`pmf_predict_var`'s formula), v = the bias variances (0 without biases)."""
    mu, Vu, mi, Vi, bu, bi = (st[k] for k in ("m_theta", "V_theta", "m_beta", "V_beta", "b_user", "b_item"))
    U, I = len(mu), len(mi)
    vu = bias_variances(u, c, U, sigma2, eta_bias2) if eta_bias2 is not None else np.zeros(U)
    vi = bias_variances(i, c, I, sigma2, eta_bias2) if eta_bias2 is not None else np.zeros(I)

    def cell(a, b, y, cw):
        e = y - bu[a] - bi[b] - (mu[a] * mi[b]).sum()
        var = mu[a] @ Vi[b] @ mu[a] + mi[b] @ Vu[a] @ mi[b] + (Vu[a] * Vi[b].T).sum()
        return -0.5 * np.log(2 * np.pi * sigma2 / cw) - cw * (e * e + var + vu[a] + vi[b]) / (2 * sigma2)

    L = sum(cell(int(a), int(b), y, cw) for a, b, y, cw in zip(u, i, x, c))
    if w0 is not None:
        listed = np.zeros((U, I), dtype=bool)
        listed[u, i] = True
        L += sum(cell(a, b, 0.0, w0) for a in range(U) for b in range(I) if not listed[a, b])
    return float(L + _prior_entropy(st, u, i, c, sigma2, eta_theta2, eta_beta2, eta_bias2))


def elbo_rows(st, u, i, x, c, sigma2, eta_theta2, eta_beta2, eta_bias2=None, w0=None, side=0):
    """The same bound from the per-row ESS of `side` (the S / w route):
    data = -1/2 [sum_j log(2 pi sigma2 / c_j) + (U I - N) log(2 pi sigma2 / w0)] - (ESS + sum_u C_u v_u + sum_i C_i v_i) / (2 sigma2)"""
    mu, Vu, mi, Vi, bu, bi = (st[k] for k in ("m_theta", "V_theta", "m_beta", "V_beta", "b_user", "b_item"))
    if side == 0:
        terms, _ = side_terms(mu, Vu, bu, mi, Vi, bi, u, i, x, c, w0)
    else:
        terms, _ = side_terms(mi, Vi, bi, mu, Vu, bu, i, u, x, c, w0)
    ess = terms[:, ESS].sum()
    if eta_bias2 is not None:
        for ids, n in ((u, len(mu)), (i, len(mi))):
            ess += (weight_sums(ids, c, n) * bias_variances(ids, c, n, sigma2, eta_bias2)).sum()
    L = -0.5 * np.sum(np.log(2 * np.pi * sigma2 / c)) - ess / (2 * sigma2)
    if w0 is not None:
        L -= 0.5 * (len(mu) * len(mi) - len(x)) * np.log(2 * np.pi * sigma2 / w0)
    return float(L + _prior_entropy(st, u, i, c, sigma2, eta_theta2, eta_beta2, eta_bias2))


def dense_completion(u, i, x, c, U, I):
    """the listed cells with their weights, then an explicit 0 of weight 1 for every other cell (row-major)"""
    listed = np.zeros((U, I), dtype=bool)
    listed[u, i] = True
    mu, mi = np.nonzero(~listed)
    return (np.concatenate([u, mu]).astype(np.int64), np.concatenate([i, mi]).astype(np.int64),
            np.concatenate([x, np.zeros(len(mu))]), np.concatenate([c, np.ones(len(mu))]))
