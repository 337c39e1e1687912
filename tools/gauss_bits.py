"""SHA-256 digests of what the Gaussian host paths compute, for comparing two builds of the library bit by bit: the
factor sweeps, `gauss_elbo_terms(with_data=True, per_row=True)`, `gauss_fold_in`, `gauss_sample_rows` (1 and 9 draws of
the stream, 2 draws of given normals; 16 user rows, one of them twice) and the accumulate / finalize pair, in the
default mode and (bias-free cases) with unlisted cells as weighted zeros.  Only the public `Context` API is used, so
the script runs unchanged on any build of the same ABI; `PMF_HIP_LIBRARY` selects the build.

Problem: `tests/helpers.skewed_problem` at 600 x 120 x 12000 (split rows, empty rows), a fixed drawn state.  Cases: K in
(20, 64, 100) x (f32, f64) x (without, with bias), and without bias K = 150 in f32 (the block-per-row solver with its
matrix in LDS) and K = 200 in f64 (solver, ELBO row pass and draws with the matrix in global scratch), each once with PMF_ELBO_ROWS / PMF_FOLD_IN_ROWS unset and once with
both set to 17 (many windows and blocks).  One digest per step; two builds agree when the two files are equal.

    python tools/gauss_bits.py out.json
"""
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  (before the engine: pmf_hip.load() explains)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "prob-matrix-factorization_amd"), os.path.join(ROOT, "tests")]
import pmf_hip  # noqa: E402
from helpers import gauss_stats, skewed_problem  # noqa: E402
from pmf_hip import ARR_BIAS, ARR_COV, ARR_FACTOR, ITEM, USER  # noqa: E402

U, I, N = 600, 120, 12000
SIGMA2, ETA2, ETA_B2, W0 = 0.4, 0.7, 1.3, 0.25
FOLD_ROWS = 40
SAMPLE_ROWS = np.r_[np.arange(0, U, U // 15)[:15], 40].astype(np.int32)   # row 40 twice


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def fold_batch(rng, long_len):
    """40 new user rows: row 3 empty, row 5 longer than the task length, the rest 1 .. 30 ratings"""
    lens = rng.integers(1, 31, FOLD_ROWS)
    lens[3], lens[5] = 0, long_len
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return ptr, rng.integers(0, I, ptr[-1]).astype(np.int32), rng.standard_normal(ptr[-1])


def steps(ctx, out, tag, batch, bias):
    for side, name in ((USER, "user"), (ITEM, "item")):
        ctx.gauss_factor_sweep(side, SIGMA2, ETA2)
        out[f"{tag}sweep_{name}"] = sha(ctx.get_array(side, ARR_FACTOR), ctx.get_array(side, ARR_COV))
    for side, name in ((USER, "user"), (ITEM, "item")):
        out[f"{tag}elbo_{name}"] = sha(*ctx.gauss_elbo_terms(side, with_data=True, per_row=True))
    out[f"{tag}fold_in"] = sha(*ctx.gauss_fold_in(USER, *batch, SIGMA2, ETA2, ETA_B2, n_iter=2 if bias else 1))
    for n_draws in (1, 9):
        out[f"{tag}sample_{n_draws}"] = sha(ctx.gauss_sample_rows(USER, SAMPLE_ROWS, n_draws, draw0=3, seed=2 ** 40 + 5))
    z = np.random.default_rng(5).standard_normal((len(SAMPLE_ROWS), 2, ctx.K))
    out[f"{tag}sample_z"] = sha(ctx.gauss_sample_rows(USER, SAMPLE_ROWS, 2, z=z))


def case(K, dtype, bias, u, i, r):
    rng = np.random.default_rng(7)
    out = {}
    with pmf_hip.Context(U, I, K, dtype=dtype) as ctx:
        ctx.set_ratings(u, i, r)
        ctx.set_array(USER, ARR_FACTOR, 0.3 * rng.standard_normal((U, K)))
        ctx.set_array(ITEM, ARR_FACTOR, 0.3 * rng.standard_normal((I, K)))
        ctx.set_cov_identity(USER, 0.5)
        ctx.set_cov_identity(ITEM, 0.25)
        if bias:
            ctx.set_array(USER, ARR_BIAS, 0.1 * rng.standard_normal(U))
            ctx.set_array(ITEM, ARR_BIAS, 0.1 * rng.standard_normal(I))
        batch = fold_batch(rng, 3 * ctx.task_max_len(USER, "gauss") + 5)
        steps(ctx, out, "", batch, bias)
        fs, _ = gauss_stats(ctx, "cuda:0")
        ctx.gauss_factor_accumulate(ITEM, fs.ptr)
        ctx.sync()
        out["accumulate_item"] = sha(fs.tensor.cpu().numpy())
        ctx.gauss_factor_finalize(ITEM, fs.ptr, SIGMA2, ETA2)
        out["finalize_item"] = sha(ctx.get_array(ITEM, ARR_FACTOR), ctx.get_array(ITEM, ARR_COV))
        if not bias:
            ctx.set_gauss_zeros(True, W0)
            steps(ctx, out, "zeros_", batch, bias)
    return out


def main(path):
    u, i, r = skewed_problem(11, U, I, N, rating_kind="centered")
    result = {}
    for rows in (None, "17"):
        for name in ("PMF_ELBO_ROWS", "PMF_FOLD_IN_ROWS"):      # read when a context is created
            os.environ.pop(name, None)
            if rows:
                os.environ[name] = rows
        cases = [(K, dtype, bias) for K in (20, 64, 100) for dtype in ("f32", "f64") for bias in (False, True)]
        for K, dtype, bias in cases + [(150, "f32", False), (200, "f64", False)]:
            key = f"rows={rows or 'unset'} K={K} {dtype} {'bias' if bias else 'plain'}"
            t0 = time.perf_counter()
            result[key] = case(K, dtype, bias, u, i, r)
            print(key, len(result[key]), "digests", f"{time.perf_counter() - t0:.1f} s", flush=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main(sys.argv[1])
