"""CPU checks of the posterior draws: the NumPy reference of the stream (tests/gauss_sample_reference.py) against the
Philox4x32-10 known answers and the moments of its normals, the new entry points in library and binding, and the host-side
argument check and round planning of pmf_gauss_sample_rows (csrc/pmf_batch.h) in a stand-alone program under the address
and undefined-behaviour sanitizers (tests/sample_host_main.cpp; nothing preloaded, no GPU)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import gauss_sample_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prob-matrix-factorization_amd", "csrc")

# (counter, key, output) of Philox4x32-10: the Random123 known-answer vectors
KAT = [
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_reference_reproduces_the_known_answers(counter, key, want):
    assert ref.philox4x32_10(counter, key).tolist() == want


def test_counter_layout_is_row_draw_block_side_under_the_seed_words():
    """words(seed, side, rows, draws, blocks)[r, d, b] is the generator on (row, draw, b, side) with key (seed low, seed
    high): the third known answer read back through the layout."""
    c, k, want = KAT[2]
    seed = k[0] | (k[1] << 32)
    w = ref.words(seed, c[3], [7, c[0]], [c[1]], [0, c[2]])
    assert w.shape == (2, 1, 2, 4)
    assert w[1, 0, 1].tolist() == want


def test_stream_is_finite_and_standard_normal():
    """2^16 normals at seed 1: no NaN or inf (u = (word + 0.5) 2^-32 is never 0 or 1), and mean, variance and lag-1
    correlation within 5 / sqrt(n) of 0, 1 and 0 -- five standard errors of the mean and of the correlation, and 3.5 of the
    variance's sqrt(2 / n).  Deterministic at the fixed seed."""
    z = ref.normals(1, 0, np.arange(256), np.arange(4), 64).reshape(-1)
    n = z.size
    assert n == 1 << 16 and np.isfinite(z).all()
    tol = 5.0 / np.sqrt(n)
    zc = z - z.mean()
    lag1 = float(np.dot(zc[:-1], zc[1:]) / np.dot(zc, zc))
    print(f"mean {z.mean():.3e} var-1 {z.var() - 1.0:.3e} lag1 {lag1:.3e} tol {tol:.3e}")
    assert abs(z.mean()) <= tol and abs(z.var() - 1.0) <= tol and abs(lag1) <= tol


def test_different_counters_give_different_words():
    """Every (side, row, draw, block) of a small grid has its own four words, and the seed's high half matters."""
    w = np.concatenate([ref.words(5, side, np.arange(6), np.arange(5), 4).reshape(-1, 4) for side in (0, 1)])
    assert len(np.unique(w, axis=0)) == len(w) == 2 * 6 * 5 * 4
    assert len(np.unique(w.reshape(-1))) == w.size
    assert (ref.words(5, 0, [3], [2], 1) != ref.words(5 + (1 << 32), 0, [3], [2], 1)).all()


def test_normals_use_the_cosine_then_the_sine_of_each_word_pair():
    w = ref.words(9, 1, [4], [0], 1)[0, 0, 0].astype(np.float64)
    u = (w + 0.5) / 4294967296.0
    want = [np.sqrt(-2 * np.log(u[0])) * np.cos(2 * np.pi * u[1]), np.sqrt(-2 * np.log(u[0])) * np.sin(2 * np.pi * u[1]),
            np.sqrt(-2 * np.log(u[2])) * np.cos(2 * np.pi * u[3]), np.sqrt(-2 * np.log(u[2])) * np.sin(2 * np.pi * u[3])]
    np.testing.assert_array_equal(ref.normals(9, 1, [4], [0], 4)[0, 0], want)
    np.testing.assert_array_equal(ref.normals(9, 1, [4], [0], 3)[0, 0], want[:3])     # K that is no multiple of 4


def test_reference_draws_have_the_covariance_as_their_second_moment():
    rng = np.random.default_rng(0)
    a = rng.standard_normal((2, 5, 5))
    V = a @ a.transpose(0, 2, 1) + 0.1 * np.eye(5)
    m = rng.standard_normal((2, 5))
    C = ref.draws(m, V, np.broadcast_to(np.eye(5), (2, 5, 5))) - m[:, None, :]    # draw k = m + C e_k: C transposed
    np.testing.assert_allclose(np.einsum("nki,nkj->nij", C, C), V, rtol=1e-12, atol=1e-12)


def test_library_and_binding_expose_the_new_entry_points():
    import __graft_entry__ as g
    g.build()
    import pmf_hip
    from pmf_hip.engine import Context
    lib = pmf_hip.load()
    for name in ("pmf_gauss_sample_rows", "pmf_topk_sampled"):
        assert name in pmf_hip.SIGNATURES and hasattr(lib, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", pmf_hip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T pmf_gauss_sample_rows" in out and " T pmf_topk_sampled" in out
    assert callable(Context.gauss_sample_rows) and callable(Context.topk_sampled)
    assert lib.pmf_abi_version() == 3
    # a null context is an argument error, not a crash, with or without a GPU
    assert lib.pmf_gauss_sample_rows(None, 0, 0, None, 1, 0, 0, None, None) == -1
    assert b"pmf_gauss_sample_rows" in lib.pmf_last_error()
    assert lib.pmf_topk_sampled(None, 1, 0, 0, None, 0, None, None, 1, 0, 0, None, None) == -1


def test_model_classes_refuse_draws_where_there_is_no_posterior():
    """The count models and the gradient class raise before any device call; so does a CAVI class that has not been fitted."""
    from src.models.gaussian_mf_sgd import GaussianMFSGD, GaussianMFSGDConfig
    from src.models.hpf_cavi import HPF_CAVI, HPF_CAVI_Config
    from src.models.poisson_mf_cavi import PoissonMFCAVI, PoissonMFCAVIConfig
    for model in (HPF_CAVI(HPF_CAVI_Config(n_factors=4, verbose=False)), PoissonMFCAVI(PoissonMFCAVIConfig(n_factors=4, verbose=False)),
                  GaussianMFSGD(GaussianMFSGDConfig(n_factors=4, verbose=False))):
        for call in (lambda: model.sample_factors("user", [0]), lambda: model.predict_draws([0], [0], 2),
                     lambda: model.top_k_items([0], k=1, sample_seed=3)):
            with pytest.raises(NotImplementedError, match="covariances"):
                call()


def _compiler():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++"):
        if os.path.exists(c):
            return c
    return shutil.which("amdclang++") or shutil.which("clang++") or shutil.which("g++")


def test_sample_host_checks_under_sanitizers(tmp_path):
    """pmf_sample_check and pmf_sample_round_rows with bad, empty and huge inputs, in a program of their own."""
    exe = str(tmp_path / "sample_host")
    subprocess.run([_compiler(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                    os.path.join(ROOT, "tests", "sample_host_main.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sample host helpers ok" in r.stdout
