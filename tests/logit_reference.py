"""Dense float64 NumPy restatement of logistic matrix factorisation under the Jaakkola-Jordan bound (include/pmf_hip.h,
pmf_gauss_logit_refresh), with full K x K matrices and Python loops over rows and ratings.
Nothing is shared with the packed walk of csrc/pmf_logit.hip or with src/models/logistic_mf_cavi.py.

    x_j in {0, 1},  s_j = theta_u . beta_i,  p(x_j = 1) = sigmoid(s_j),  theta_u, beta_i ~ N(0, eta2 I),  q(row) = N(m, V)
    S_r = V_r + m_r m_r'      E[s_j^2] = <S_u, S_i>      xi_j = sqrt(E[s_j^2])      lambda(xi) = tanh(xi / 2) / (4 xi)
    c_j = 2 lambda(xi_j)      y_j = (x_j - 1/2) / c_j
    D = sum_j [ log sigmoid(xi_j) - xi_j / 2 + (x_j - 1/2) m_u . m_i ]
    row update:  V_r = inv(I / eta2 + sum_j c_j S_{o_j}),   m_r = V_r sum_j (x_j - 1/2) m_{o_j}
    L = D + sum over both sides of -KL(q || prior)."""
import numpy as np

SERIES_BELOW = 1e-3


def lam(xi):
    """lambda(xi), lambda(0) = 1/8; the series 1/8 - xi^2/96 + xi^4/960 below SERIES_BELOW"""
    xi = np.abs(np.asarray(xi, dtype=np.float64))
    x2 = xi * xi
    safe = np.where(xi < SERIES_BELOW, 1.0, xi)
    return np.where(xi < SERIES_BELOW, 0.125 - x2 / 96.0 + x2 * x2 / 960.0, np.tanh(0.5 * safe) / (4.0 * safe))


def log_sigmoid(z):
    z = np.asarray(z, dtype=np.float64)
    return np.where(z >= 0, -np.log1p(np.exp(-np.abs(z))), z - np.log1p(np.exp(-np.abs(z))))


def refresh(m_u, V_u, m_i, V_i, u, i, x):
    """(xi, c, y, D, abs_terms) for the ratings (u, i, x): abs_terms[j] = sum over the K x K entries of
    (|V_u| + |m_u| |m_u|') (|V_i| + |m_i| |m_i|'), the sum of the magnitudes of every product that enters E[s_j^2]."""
    n = len(u)
    e, abs_terms, dot = np.zeros(n), np.zeros(n), np.zeros(n)
    for j in range(n):
        a, b = int(u[j]), int(i[j])
        ou, oi = np.multiply.outer(m_u[a], m_u[a]), np.multiply.outer(m_i[b], m_i[b])
        e[j] = ((V_u[a] + ou) * (V_i[b] + oi)).sum()
        abs_terms[j] = ((np.abs(V_u[a]) + np.abs(ou)) * (np.abs(V_i[b]) + np.abs(oi))).sum()
        dot[j] = (m_u[a] * m_i[b]).sum()
    xi = np.sqrt(e)
    c = 2.0 * lam(xi)
    half = np.asarray(x, dtype=np.float64) - 0.5
    D = float(np.sum(log_sigmoid(xi) - 0.5 * xi + half * dot))
    return xi, c, half / c, D, abs_terms


def sweep(m, V, m_o, V_o, ids, other_ids, x, c, eta2):
    """one side's factor update by direct K x K solves; rows without ratings keep their state"""
    m, V = m.copy(), V.copy()
    K = m.shape[1]
    rows = [[] for _ in range(len(m))]
    for k, r in enumerate(ids):
        rows[int(r)].append(k)
    for r, sel in enumerate(rows):
        if not sel:
            continue
        S, w = np.zeros((K, K)), np.zeros(K)
        for k in sel:
            o = int(other_ids[k])
            S += c[k] * (V_o[o] + np.multiply.outer(m_o[o], m_o[o]))
            w += (x[k] - 0.5) * m_o[o]
        Vr = np.linalg.inv(np.eye(K) / eta2 + S)
        V[r] = 0.5 * (Vr + Vr.T)
        m[r] = V[r] @ w
    return m, V


def neg_kl(m, V, eta2):
    """-KL(q || prior) of one side"""
    rows, K = m.shape
    logdet = sum(np.linalg.slogdet(V[r])[1] for r in range(rows))
    sqnorm = float((m * m).sum() + np.trace(V, axis1=1, axis2=2).sum())
    return 0.5 * logdet - sqnorm / (2.0 * eta2) - 0.5 * rows * K * np.log(eta2) + 0.5 * rows * K


def bound(m_u, V_u, m_i, V_i, u, i, x, eta2):
    """L at the optimal xi of the given q"""
    return refresh(m_u, V_u, m_i, V_i, u, i, x)[3] + neg_kl(m_u, V_u, eta2) + neg_kl(m_i, V_i, eta2)


def initial_state(seed, U, I, K):
    """the model classes' draw: user means, then item means, 0.1 N(0, 1); identity covariances"""
    rng = np.random.default_rng(seed)
    return (0.1 * rng.standard_normal((U, K)), np.tile(np.eye(K), (U, 1, 1)),
            0.1 * rng.standard_normal((I, K)), np.tile(np.eye(K), (I, 1, 1)))


def fit(u, i, x, U, I, K, eta2, n_iter, seed):
    """n_iter iterations of: refresh (user stream), user sweep, refresh (item stream), item sweep.  Returns the state
    (m_u, V_u, m_i, V_i) and the bound of every iteration at its item-side refresh."""
    m_u, V_u, m_i, V_i = initial_state(seed, U, I, K)
    trace = []
    for _ in range(n_iter):
        c = refresh(m_u, V_u, m_i, V_i, u, i, x)[1]
        m_u, V_u = sweep(m_u, V_u, m_i, V_i, u, i, x, c, eta2)
        _, c, _, D, _ = refresh(m_u, V_u, m_i, V_i, u, i, x)
        trace.append(D + neg_kl(m_u, V_u, eta2) + neg_kl(m_i, V_i, eta2))
        m_i, V_i = sweep(m_i, V_i, m_u, V_u, i, u, x, c, eta2)
    return (m_u, V_u, m_i, V_i), trace


def planted(seed, U, I, K, N, scale=1.5, unique=True):
    """(u, i, x, theta, beta): N distinct pairs with labels drawn from sigmoid(theta . beta), planted factors of standard
    deviation `scale` / sqrt(sqrt(K)); the last ids occur"""
    rng = np.random.default_rng(seed)
    theta = rng.standard_normal((U, K)) * scale / K ** 0.25
    beta = rng.standard_normal((I, K)) * scale / K ** 0.25
    cells = rng.permutation(U * I)[:N] if unique else rng.integers(0, U * I, N)
    cells[0] = U * I - 1
    u, i = cells // I, cells % I
    p = 1.0 / (1.0 + np.exp(-(theta[u] * beta[i]).sum(axis=1)))
    x = (rng.uniform(size=N) < p).astype(np.float64)
    return u.astype(np.int64), i.astype(np.int64), x, theta, beta


def max_fall(trace):
    """the largest decrease between consecutive entries (0.0 for a non-decreasing trace)"""
    t = np.asarray(trace, dtype=np.float64)
    return float(max(0.0, np.max(t[:-1] - t[1:]))) if len(t) > 1 else 0.0
