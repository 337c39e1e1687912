"""The Gaussian row solve  V = (S / sigma2 + I / eta2)^-1,  m = V w / sigma2  on chosen matrices: the battery of
matrices, the float64 / long double reference, the scaled error measure with its bound, and a NumPy restatement of
the unpivoted Jacobi-scaled symmetric sweep in float32 / float64 (tests/test_gauss_solver_cpu.py,
tests/test_gauss_solver_gpu.py).  Dense K x K NumPy throughout; nothing here is shared with csrc/pmf_gauss.hip."""
import numpy as np

# (sigma2, eta2): the reference grid's two corners, then a wide pair each way
PAIRS = ((0.3, 0.5), (0.7, 2.0), (0.05, 10.0), (2.0, 0.05))
NP_DTYPE = {"f32": np.float32, "f64": np.float64}
EPS = {"f32": float(np.finfo(np.float32).eps), "f64": float(np.finfo(np.float64).eps)}

# The bound on both scaled errors is  C * eps_T * (kappa + K)  (see `errors`).  C = 4 x the largest ratio
# error / (eps_T (kappa + K)) that `sweep_restatement` reaches over DEFAULT_K and all four PAIRS; the 4 covers what
# the device does differently from the restatement (rank-4 block pivots on the matrix cores, fma contraction, rcp + one
# Newton step, one fp32 rounding of S in the accumulate, the mean's reduction order).  Measured ratios of the
# restatement (tests/test_gauss_solver_cpu.py re-measures them and asserts ratio <= C / 4):
#     fp32  V 0.76   m 0.99  (both K = 2, tail4, (0.7, 2.0))        fp64  V 0.71 (K = 2, tail4)   m 0.81 (K = 1, arrow)
C = 4.0
CAP = {"f32": 1e-2, "f64": 1e-6}      # no case's bound is looser than this

# every K of the default path: the fused homes at every width, then the LDS-to-scratch edge of the block-per-row kernel
DEFAULT_K = {"f32": tuple(range(1, 129)) + (129, 136, 200, 201, 256),
             "f64": tuple(range(1, 65)) + (65, 100, 128, 141, 142, 200, 256)}
BLOCK_BOUNDS = (0, 3, 18, 35, 70, 113)


class Case:
    """One row: S (K x K, float64), the planted mean m_r (zero where S must arrive exactly) and rating x_r; the
    right-hand side of the sweep route is w = x_r m_r."""

    def __init__(self, name, S, m, x, n=1.0):
        self.name, self.S, self.m, self.x, self.n = name, S, m, float(x), float(n)

    @property
    def exact(self):
        return self.name in ("diag", "blocks")


def _spec(rng, K, c, n=1.0):
    """n Q diag(lambda) Q', lambda log-spaced from 1 to 1 / c"""
    q, _ = np.linalg.qr(rng.normal(size=(K, K)))
    lam = np.logspace(0.0, -np.log10(c), K)
    s = (q * lam) @ q.T
    return n * 0.5 * (s + s.T)


def _equi_block(K, lo, width, rho):
    s = np.eye(K)
    s[lo:lo + width, lo:lo + width] = (1 - rho) * np.eye(width) + rho
    return s


def block_ranges(K):
    b = sorted({min(x, K) for x in BLOCK_BOUNDS} | {K})
    return [(lo, hi) for lo, hi in zip(b[:-1], b[1:])]


def battery(K, dtype):
    """The cases of one (K, dtype), seeded by K.  S = n Sigma throughout."""
    rng = np.random.default_rng(K)
    mats = [(f"spec{c:g}", _spec(rng, K, c, n), n) for c, n in ((10, 1), (1e2, 1e3), (1e3, 1e3), (1e4, 1e3))]
    if dtype == "f64":
        mats += [(f"spec{c:g}", _spec(rng, K, c, n), n) for c, n in ((1e6, 1e6), (1e8, 1e6))]
    d = np.logspace(0, 3, K)
    mats.append(("scaled", _spec(rng, K, 1e2) * np.multiply.outer(d, d), 1))
    mats.append(("equicorr", 1e3 * ((1 - 0.98) * np.eye(K) + 0.98), 1e3))
    w4 = min(4, K)
    mats.append(("lead4", 1e3 * _equi_block(K, 0, w4, 0.999), 1e3))
    mats.append(("tail4", 1e3 * _equi_block(K, K - w4, w4, 0.999), 1e3))
    arrow = np.eye(K)
    arrow[0, K - 1] += 0.9
    arrow[K - 1, 0] += 0.9
    mats.append(("arrow", 1e3 * arrow, 1e3))
    M = 0.3 * rng.normal(size=(2000, K)) + 0.5
    mats.append(("datalike", M.T @ M + 100.0 * np.eye(K), 1))
    mats.append(("diag", np.diag(np.logspace(0, 6, K)), 1))
    blocks = np.zeros((K, K))
    for lo, hi in block_ranges(K):
        blocks[lo:hi, lo:hi] = 1e3 * _spec(rng, hi - lo, 1e2)
    mats.append(("blocks", blocks, 1e3))
    cases = []
    for name, S, n in mats:
        m = 0.3 * rng.normal(size=K)
        x = rng.integers(-2, 3)
        if name in ("diag", "blocks"):
            m = np.zeros(K)
        cases.append(Case(name, S, m, x, n))
    return cases


def covariance_rows(K, dtype):
    """[(name, Sigma)]: the battery's matrices with n = 1, as covariances for the log det (`diag` left out)"""
    return [(c.name, c.S / c.n) for c in battery(K, dtype) if c.name != "diag"]


def precision_matrix(S, sigma2, eta2):
    return np.asarray(S, dtype=np.float64) / sigma2 + np.eye(len(S)) / eta2


def scaled_cond(P):
    """cond_2 of P with its diagonal scaled to one"""
    g = 1.0 / np.sqrt(np.diag(P))
    return float(np.linalg.cond(P * g[:, None] * g[None, :]))


def reference(S, w, sigma2, eta2):
    """(V, m, kappa) in float64 of the exact S and w given: the float64 inverse refined by two Newton-Schulz steps
    V <- V + V (I - P V), with V and the residual I - P V in long double.  (The correction V (I - P V) is a float64
    product: the residual is of the order of 1e-16 kappa, so its rounding there is far below the long double's.)"""
    P = precision_matrix(S, sigma2, eta2)
    Pl = P.astype(np.longdouble)
    V = np.linalg.inv(P).astype(np.longdouble)
    eye = np.eye(len(P), dtype=np.longdouble)
    for _ in range(2):
        R = eye - np.dot(Pl, V)
        V = V + (V.astype(np.float64) @ R.astype(np.float64))
    V = 0.5 * (V + V.T)
    m = np.dot(V, np.asarray(w, dtype=np.longdouble)) / np.longdouble(sigma2)
    return V.astype(np.float64), m.astype(np.float64), scaled_cond(P)


def reference_blocks(S, w, sigma2, eta2, ranges):
    """`reference` of a block-diagonal S, every block inverted alone"""
    K = len(S)
    V, m = np.zeros((K, K)), np.zeros(K)
    for lo, hi in ranges:
        V[lo:hi, lo:hi], m[lo:hi], _ = reference(S[lo:hi, lo:hi], np.asarray(w)[lo:hi], sigma2, eta2)
    return V, m, scaled_cond(precision_matrix(S, sigma2, eta2))


def errors(V, m, V_ref, m_ref, w, sigma2):
    """The two scaled errors, with d_i = sqrt(V_ref[i][i]):
        eV = max_ij |dV_ij| / (d_i d_j)        em = max_i |dm_i| / (d_i |diag(d) w|_2 / sigma2)
    For w = 0 the mean must be exactly zero: em is then 0, or inf if it is not."""
    d = np.sqrt(np.diag(V_ref))
    eV = float(np.max(np.abs(np.asarray(V, dtype=np.float64) - V_ref) / (d[:, None] * d[None, :])))
    scale = float(np.linalg.norm(d * np.asarray(w, dtype=np.float64))) / sigma2
    dm = np.abs(np.asarray(m, dtype=np.float64) - m_ref)
    if scale == 0.0:
        em = 0.0 if not dm.any() else float("inf")
    else:
        em = float(np.max(dm / (d * scale)))
    return eV, em


def bound(dtype, kappa, K):
    return C * EPS[dtype] * (kappa + K)


def sweep_restatement(S, w, sigma2, eta2, dtype):
    """The unpivoted symmetric sweep of the Jacobi-scaled P in the arithmetic of `dtype`, one scalar pivot at a time:
    (V, m, pivots, g) with the pivots of the scaled matrix in elimination order and the scales g = diag(P)^-1/2, so
    that log det P = sum log pivots - 2 sum log g."""
    T = NP_DTYPE[dtype]
    K = len(S)
    is2, ie2 = T(1.0 / sigma2), T(1.0 / eta2)
    B = np.asarray(S).astype(T) * is2
    B[np.diag_indices(K)] += ie2
    g = (T(1) / np.sqrt(np.diag(B))).astype(T)
    B = B * g[:, None] * g[None, :]
    pivots = np.empty(K, dtype=T)
    for k in range(K):
        pivots[k] = B[k, k]
        pinv = T(1) / B[k, k]
        col = B[:, k].copy()
        row = B[k, :] * pinv
        B -= np.multiply.outer(col, row)
        B[k, :] = row
        B[:, k] = col * pinv
        B[k, k] = -pinv
    assert B.dtype == T
    V = -B * g[:, None] * g[None, :]
    V = np.tril(V) + np.tril(V, -1).T      # the packed lower triangle is what a solver hands back
    wT, m = np.asarray(w).astype(T), np.zeros(K, dtype=T)
    for j in range(K):                 # one rounding per product and per sum, in index order
        m += V[:, j] * wT[j]
    return V, m * is2, pivots, g


def restatement_logdet_V(S, dtype):
    """log det of a covariance S by the same elimination (no hyperparameters: the matrix itself is eliminated); the
    logarithms in float64, as the device takes them"""
    _, _, piv, g = sweep_restatement(S, np.zeros(len(S)), 1.0, np.inf, dtype)
    if not (piv > 0).all():
        return float("nan")
    return float(np.log(piv.astype(np.float64)).sum() - 2.0 * np.log(g.astype(np.float64)).sum())


def logdet_bound(dtype, kappa, K):
    return K * bound(dtype, kappa, K)


def diag_ulps(V, s, sigma2, eta2, dtype):
    """`diag` case: the off-diagonal entries of V are exactly zero, and the largest distance of a diagonal entry from
    1 / (s / sigma2 + 1 / eta2) in units in the last place of `dtype`"""
    T = NP_DTYPE[dtype]
    V = np.asarray(V, dtype=np.float64)
    off = V - np.diag(np.diag(V))
    want = 1.0 / (np.asarray(s, dtype=np.float64) / sigma2 + 1.0 / eta2)
    ulp = np.spacing(want.astype(T)).astype(np.float64)
    return bool((off == 0).all()), float(np.max(np.abs(np.diag(V) - want) / ulp))


def cross_block_zero(V, ranges):
    mask = np.ones(np.shape(V), dtype=bool)
    for lo, hi in ranges:
        mask[lo:hi, lo:hi] = False
    return bool((np.asarray(V)[mask] == 0).all())


def pack_lower(S):
    """the packed lower triangle: (r, c), c <= r, at r (r + 1) / 2 + c"""
    r, c = np.tril_indices(len(S))
    return np.asarray(S)[r, c]


# ---- the other homes of the solver (tests/test_gauss_solver_gpu.py) and what both test modules share -------------------
SMALL_EDGE_K = (1, 7, 8, 9, 16, 17, 32, 33, 48, 49, 56, 57, 64)          # the class edges of the one-wavefront kernels
PAIR_EDGE_K = (65, 80, 81, 95, 96, 112, 113, 114, 115, 128)              # ... of the two-wavefront kernels
FINALIZE_K = {"f32": (8, 33, 64, 70, 114, 128, 150), "f64": (16, 64, 100)}
LOGDET_K = (1, 5, 8, 9, 16, 33, 64, 65, 100, 128, 141, 142)
DIAG_ULPS = 4.0


def finalize_rhs(K, n_rows):
    """right-hand sides of the finalize route: nothing to do with the matrices"""
    return np.random.default_rng(1000 + K).normal(size=(n_rows, K)) * 3.0


def rounded(a, dtype):
    """`a` as the context holds it, in float64"""
    return np.asarray(a, dtype=np.float64).astype(NP_DTYPE[dtype]).astype(np.float64)


_REFERENCES = {}


def cached_reference(key, name, S, w, sigma2, eta2):
    """`reference` (block by block for `blocks`) of the row `key` names, computed once per process"""
    if key not in _REFERENCES:
        if name == "blocks":
            _REFERENCES[key] = reference_blocks(S, w, sigma2, eta2, block_ranges(len(S)))
        else:
            _REFERENCES[key] = reference(S, w, sigma2, eta2)
    return _REFERENCES[key]


def judge(dtype, name, V, m, S, w, sigma2, eta2, key):
    """One solved row against the reference of the S and w it was given: (figures, failures).  figures = (ratio of eV
    to eps (kappa + K), the same of em, kappa, ulps of the `diag` case or 0); failures = what breaks the contract: a
    scaled error above C eps (kappa + K), and for the exact cases a non-zero where only zeros were ever multiplied or a
    diagonal entry further than DIAG_ULPS from its closed form."""
    K = len(S)
    V_ref, m_ref, kappa = cached_reference(key, name, S, w, sigma2, eta2)
    eV, em = errors(V, m, V_ref, m_ref, w, sigma2)
    unit = EPS[dtype] * (kappa + K)
    fails, ulps = [], 0.0
    if not (eV <= C * unit):
        fails.append(f"eV {eV:.3e} > {C * unit:.3e}")
    if not (em <= C * unit):
        fails.append(f"em {em:.3e} > {C * unit:.3e}")
    if name == "diag":
        zero, ulps = diag_ulps(V, np.diag(S), sigma2, eta2, dtype)
        if not zero:
            fails.append("off-diagonal entry of a diagonal matrix's inverse is not zero")
        if not (ulps <= DIAG_ULPS):
            fails.append(f"diagonal entry {ulps:.2f} ulp from 1 / (s / sigma2 + 1 / eta2)")
    if name == "blocks" and not cross_block_zero(V, block_ranges(K)):
        fails.append("cross-block entry is not zero")
    return (eV / unit, em / unit, kappa, ulps), fails
