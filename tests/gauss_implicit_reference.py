"""Dense float64 NumPy restatement of the bias-free Gaussian calls with every unlisted (user, item) cell counted as an
observation of 0 with variance sigma2 / w0 (PMF_ZEROS_OBSERVED of pmf_ctx_set_gauss_zeros, include/pmf_hip.h), written
from the formulae there with full K x K matrices and Python loops over rows, ratings and cells.  Nothing is shared with
the packed walk of csrc/pmf_gauss.hip or with `elbo_from_terms`.

With A_o = V_o + m_o m_o' of a row of the other side, S_r = sum over the listed ratings of A_o, w_r = sum m_o x and
G = sum over ALL rows of the other side of A_o:
    S'_r = (1 - w0) S_r + w0 G,   V_r = inv(I / eta2 + S'_r / sigma2),   m_r = V_r w_r / sigma2     for every row
    ESS_r = c_r - 2 m_r . w_r + <V_r + m_r m_r', S'_r>
A state is a dict m_theta, V_theta, m_beta, V_beta; `u, i, x` list each cell at most once."""
import numpy as np

SQNORM, LOGDET, BIAS_SQ, ESS = 0, 1, 2, 3


def problem_p(seed=5, U=90, I=70, N=4000):
    """The sparse problem P: `gamma_implicit_reference.problem_p` (duplicates dropped, every eleventh rating 0) with the
    ratings shifted by -1, so that some are negative and some exactly 0."""
    import gamma_implicit_reference as g
    u, i, x = g.problem_p(seed, U, I, N)
    return u.astype(np.int64), i.astype(np.int64), x - 1.0


def dense_completion(u, i, x, U, I):
    """D: the same ratings, then an explicit 0 for every cell of the U x I matrix that is not listed (row-major)."""
    listed = np.zeros((U, I), dtype=bool)
    listed[u, i] = True
    mu, mi = np.nonzero(~listed)
    return np.concatenate([u, mu]).astype(np.int64), np.concatenate([i, mi]).astype(np.int64), np.concatenate([x, np.zeros(len(mu))])


def initial_state(seed, U, I, K):
    rng = np.random.default_rng(seed)
    return {"m_theta": 0.1 * rng.standard_normal((U, K)), "V_theta": np.tile(np.eye(K), (U, 1, 1)),
            "m_beta": 0.1 * rng.standard_normal((I, K)), "V_beta": np.tile(np.eye(K), (I, 1, 1))}


def gram(m, V):
    """(G, sum_r |V_r| + |m_r m_r'|): G = sum over all rows of V_r + m_r m_r', added row by row"""
    K = m.shape[1]
    G, mag = np.zeros((K, K)), np.zeros((K, K))
    for r in range(len(m)):
        outer = np.multiply.outer(m[r], m[r])
        G += V[r] + outer
        mag += np.abs(V[r]) + np.abs(outer)
    return G, mag


def _rows_of(ids, n_rows):
    out = [[] for _ in range(n_rows)]
    for k, r in enumerate(ids):
        out[int(r)].append(k)
    return out


def listed_stats(m_o, V_o, ids, other_ids, x, n_rows):
    """per row: (S_r, w_r, c_r, sum |A_o|) over its listed ratings, rating by rating; zeros for a row without ratings"""
    K = m_o.shape[1]
    out = []
    for sel in _rows_of(ids, n_rows):
        S, Sa, w, c = np.zeros((K, K)), np.zeros((K, K)), np.zeros(K), 0.0
        for k in sel:
            o = int(other_ids[k])
            outer = np.multiply.outer(m_o[o], m_o[o])
            S += V_o[o] + outer
            Sa += np.abs(V_o[o]) + np.abs(outer)
            w += m_o[o] * x[k]
            c += x[k] * x[k]
        out.append((S, w, c, Sa))
    return out


def solve_row(S, w, sigma2, eta2):
    V = np.linalg.inv(np.eye(len(w)) / eta2 + S / sigma2)
    V = 0.5 * (V + V.T)
    return V @ w / sigma2, V


def half_sweep(m_o, V_o, ids, other_ids, x, n_rows, sigma2, eta2, w0):
    """(m [rows, K], V [rows, K, K]) of EVERY row of the side, zero mode with weight w0"""
    G, _ = gram(m_o, V_o)
    K = m_o.shape[1]
    m, V = np.zeros((n_rows, K)), np.zeros((n_rows, K, K))
    for r, (S, w, _, _) in enumerate(listed_stats(m_o, V_o, ids, other_ids, x, n_rows)):
        m[r], V[r] = solve_row((1.0 - w0) * S + w0 * G, w, sigma2, eta2)
    return m, V


def default_half_sweep(m, V, m_o, V_o, ids, other_ids, x, sigma2, eta2):
    """The default update (include/pmf_hip.h, pmf_gauss_factor_sweep): rows with ratings from their listed sums, rows
    without keep their state."""
    m, V = m.copy(), V.copy()
    for r, (S, w, _, _) in enumerate(listed_stats(m_o, V_o, ids, other_ids, x, len(m))):
        if S[0, 0] != 0.0:
            m[r], V[r] = solve_row(S, w, sigma2, eta2)
    return m, V


def half_steps(st, u, i, x, sigma2, eta_theta2, eta_beta2, w0):
    """the states after the user and after the item half-sweep of one iteration; w0 = None: the default mode"""
    st = dict(st)
    for name, other, ids, oids, eta2 in (("theta", "beta", u, i, eta_theta2), ("beta", "theta", i, u, eta_beta2)):
        if w0 is None:
            m, V = default_half_sweep(st["m_" + name], st["V_" + name], st["m_" + other], st["V_" + other], ids, oids, x, sigma2, eta2)
        else:
            m, V = half_sweep(st["m_" + other], st["V_" + other], ids, oids, x, len(st["m_" + name]), sigma2, eta2, w0)
        st["m_" + name], st["V_" + name] = m, V
        yield dict(st)


def fold_in(m_o, V_o, row_ptr, other_ids, x, sigma2, eta2, w0):
    """(m [n, K], V [n, K, K]) of the rows of a CSR batch against the other side; a row without ratings is
    inv(I / eta2 + w0 G / sigma2) with mean 0"""
    n = len(row_ptr) - 1
    ids = np.repeat(np.arange(n), np.diff(row_ptr))
    return half_sweep(m_o, V_o, ids, other_ids, x, n, sigma2, eta2, w0)


def side_terms(m, V, m_o, V_o, ids, other_ids, x, w0):
    """(rows, 4) per-row ELBO terms of a side in zero mode and the (rows,) magnitude of the ESS: the sum of the absolute
    values of every product that enters it, with (1 - w0) |S| + w0 |G| (sums of absolute values) in the place of S'."""
    rows, K = m.shape
    G, Ga = gram(m_o, V_o)
    out, mag = np.zeros((rows, 4)), np.zeros(rows)
    absx = np.abs(x)
    for r, (S, w, c, Sa) in enumerate(listed_stats(m_o, V_o, ids, other_ids, x, rows)):
        out[r, SQNORM] = (m[r] * m[r]).sum() + np.trace(V[r])
        sign, ld = np.linalg.slogdet(V[r])
        out[r, LOGDET] = ld if sign > 0 else np.nan
        second = V[r] + np.multiply.outer(m[r], m[r])
        Sp = (1.0 - w0) * S + w0 * G
        out[r, ESS] = c - 2.0 * (m[r] * w).sum() + (second * Sp).sum()
        wa = np.zeros(K)
        for k in np.flatnonzero(ids == r):
            wa += np.abs(m_o[int(other_ids[k])]) * absx[k]
        seconda = np.abs(V[r]) + np.abs(np.multiply.outer(m[r], m[r]))
        mag[r] = c + 2.0 * (np.abs(m[r]) * wa).sum() + (seconda * ((1.0 - w0) * Sa + w0 * Ga)).sum()
    return out, mag


def _prior_entropy(st, eta_theta2, eta_beta2):
    L = 0.0
    for m, V, eta2 in ((st["m_theta"], st["V_theta"], eta_theta2), (st["m_beta"], st["V_beta"], eta_beta2)):
        K = m.shape[1]
        for r in range(len(m)):
            second = (m[r] * m[r]).sum() + np.trace(V[r])
            L += -0.5 * K * np.log(2 * np.pi * eta2) - second / (2 * eta2)              # E_q log N(row; 0, eta2 I)
            L += 0.5 * K * (1 + np.log(2 * np.pi)) + 0.5 * np.linalg.slogdet(V[r])[1]   # entropy of N(m, V)
    return L


def elbo_cells(st, u, i, x, sigma2, eta_theta2, eta_beta2, w0):
    """The bound written cell by cell: every one of the U x I cells is an observation y (the rating, or 0) with variance
    sigma2 / c (c = 1 listed, w0 unlisted):  E_q log N(y; theta_u . beta_i, sigma2 / c)
    = -1/2 log(2 pi sigma2 / c) - c / (2 sigma2) [(y - m_u . m_i)^2 + m_u' V_i m_u + m_i' V_u m_i + tr(V_u V_i)]."""
    mu, Vu, mi, Vi = st["m_theta"], st["V_theta"], st["m_beta"], st["V_beta"]
    U, I = len(mu), len(mi)
    y, c = np.zeros((U, I)), np.full((U, I), float(w0))
    y[u, i], c[u, i] = x, 1.0
    L = 0.0
    for a in range(U):
        for b in range(I):
            e = y[a, b] - (mu[a] * mi[b]).sum()
            var = mu[a] @ Vi[b] @ mu[a] + mi[b] @ Vu[a] @ mi[b] + (Vu[a] * Vi[b].T).sum()
            L += -0.5 * np.log(2 * np.pi * sigma2 / c[a, b]) - c[a, b] * (e * e + var) / (2 * sigma2)
    return float(L + _prior_entropy(st, eta_theta2, eta_beta2))


def elbo_rows(st, u, i, x, sigma2, eta_theta2, eta_beta2, w0, side=0):
    """The same bound from the per-row ESS of `side`."""
    mu, Vu, mi, Vi = st["m_theta"], st["V_theta"], st["m_beta"], st["V_beta"]
    if side == 0:
        terms, _ = side_terms(mu, Vu, mi, Vi, u, i, x, w0)
    else:
        terms, _ = side_terms(mi, Vi, mu, Vu, i, u, x, w0)
    N, cells = len(x), len(mu) * len(mi)
    L = -0.5 * (N * np.log(2 * np.pi * sigma2) + (cells - N) * np.log(2 * np.pi * sigma2 / w0)) - terms[:, ESS].sum() / (2 * sigma2)
    return float(L + _prior_entropy(st, eta_theta2, eta_beta2))


def planted_problem(seed, U=120, I=80, groups=3, p_in=0.6, p_out=0.03, held_out=2):
    """Implicit feedback with planted structure: user and item groups, P(listed) = p_in inside a group and p_out outside,
    every listed rating 1; `held_out` listed items per user (where the user has more than that) go to the test frame.
    Returns (train (u, i, x), test (u, i))."""
    rng = np.random.default_rng(seed)
    gu, gi = rng.integers(0, groups, U), rng.integers(0, groups, I)
    listed = rng.random((U, I)) < np.where(gu[:, None] == gi[None, :], p_in, p_out)
    listed[U - 1, I - 1] = True
    tu, ti, hu, hi = [], [], [], []
    for a in range(U):
        items = rng.permutation(np.flatnonzero(listed[a]))
        if a == U - 1:                                 # the last ids define the dimensions: (U - 1, I - 1) stays in train
            items = np.concatenate([items[items != I - 1], [I - 1]])
        n_held = held_out if len(items) > held_out else 0
        hu += [a] * n_held
        hi += list(items[:n_held])
        tu += [a] * (len(items) - n_held)
        ti += list(items[n_held:])
    tu, ti = np.array(tu, dtype=np.int64), np.array(ti, dtype=np.int64)
    return (tu, ti, np.ones(len(tu))), (np.array(hu, dtype=np.int64), np.array(hi, dtype=np.int64))
