"""The host helpers of the batched entry points (csrc/pmf_batch.h: offsets check, scratch layout, block cut) in a
stand-alone program, tests/batch_host_main.cpp, built with the host compiler under AddressSanitizer and
UndefinedBehaviorSanitizer and run as a child process.  No HIP, no GPU, nothing preloaded: the header stands alone.

The program's block-cut cases are exhaustive over small batches and caps that no GPU test lowers (the staged-ratings cap
and the Gaussian statistics units), and its three properties -- the blocks partition the rows, a block of more than one
row respects every cap, the next row would have broken one -- leave the greedy cut as the only answer.

The binding's counterpart of the offsets check, `pmf_hip.engine.csr_batch`, is pure NumPy and is tested here too."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "prob-matrix-factorization_amd", "csrc")


def _compiler():
    for c in ("/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++"):
        if os.path.exists(c):
            return c
    return shutil.which("amdclang++")


@pytest.mark.parametrize("seq", [list, tuple, np.array])
def test_csr_batch_takes_any_sequence_for_every_column(seq):
    """The binding's batch conversion: offsets, ids and ratings given as lists, tuples or arrays (two and three entries: a
    tuple must never be read as anything but the column's values) come back as contiguous int64 / int32 / float64, and a
    length that does not fit raises the caller's message."""
    from pmf_hip.engine import csr_batch
    for ids, x in (([1, 2], [3.0, 4.0]), ([5, 1, 2], [3.0, 4.0, 0.5])):
        rp, o, v = csr_batch("the message", seq([0, 1, len(ids)]), seq(ids), "other_ids", seq(x))
        assert (rp.dtype, o.dtype, v.dtype) == (np.int64, np.int32, np.float64)
        assert rp.tolist() == [0, 1, len(ids)] and o.tolist() == ids and v.tolist() == x
        assert all(a.flags["C_CONTIGUOUS"] for a in (rp, o, v))
        for bad in ((seq([0, 1, len(ids) + 1]), seq(ids), seq(x)), (seq([0, 1, len(ids)]), seq(ids), seq(x[:-1])), (seq([]), seq(ids), seq(x))):
            with pytest.raises(ValueError, match="^the message$"):
                csr_batch("the message", bad[0], bad[1], "other_ids", bad[2])
    rp, = csr_batch("the message", seq([0, 7]), n_rows=1)          # offsets alone: their count only
    assert rp.tolist() == [0, 7]
    with pytest.raises(ValueError, match="^the message$"):
        csr_batch("the message", seq([0, 7]), n_rows=2)
    with pytest.raises(ValueError, match="other_ids: values do not fit int32"):
        csr_batch("the message", seq([0, 1]), seq([2 ** 40]), "other_ids", seq([1.0]))


def test_batch_host_helpers_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no ROCm clang++ found")
    exe = str(tmp_path / "batch_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC,
                    os.path.join(ROOT, "tests", "batch_host_main.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "batch host helpers ok" in r.stdout
