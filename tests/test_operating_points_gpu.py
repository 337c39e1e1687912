"""The device path at the reference's published operating points (model_comparison_params.txt / best_hyperparams.txt:3-5),
against what THE REFERENCE computed there (tests/golden/op_*.npz, written by `tests/golden/make_golden.py op_*`):

  * Gaussian MF with biases, K = 30, max_iter = 100, tol = 1e-3 -- three runs: the early stop on validation + test
    (iteration 9, both neighbouring improvements more than 2e-4 away from 0 and from tol), the sharp early stop on the
    validation frame (iteration 10, on an improvement of +1.02e-5: float64 only) and all 100 iterations (tol = 0.0);
  * HPF, K = 20, 100 iterations, ratings + 1;
  * Poisson MF, K = 40, 150 iterations.

Every case is ONE fit of the product class on `recipe_standin()`'s train frame (272,255 ratings, 11,780 x 13,000): the
operating point itself, not a scaled-down copy.  The fixtures hold the reference's validation RMSE / MacroMAE of every
iteration at full precision, so a drift that needs many iterations and realistic row lengths to show is caught at the
iteration where it starts."""
import json
import os
import time

import numpy as np
import pandas as pd
import pytest

from helpers import GOLDEN, recipe_standin

pytestmark = pytest.mark.gpu

TABLES = {"gauss_bias": (("m_theta", "m_user_bias"), ("m_beta", "m_item_bias")),
          "hpf": (("E_theta", "E_xi"), ("E_beta", "E_eta")),
          "poisson": (("E_theta",), ("E_beta",))}
STATEFUL = ["op_gauss_bias_k30_stop", "op_gauss_bias_k30_long", "op_hpf_k20", "op_poisson_k40"]
ALL = STATEFUL[:1] + ["op_gauss_bias_k30_stop_sharp"] + STATEFUL[1:]


@pytest.fixture(scope="module")
def standin():
    frames = dict(zip(("train", "validation", "test"), recipe_standin()))
    before = {name: f["rating"].to_numpy().copy() for name, f in frames.items()}
    yield frames
    for name, f in frames.items():       # every case reads the same frames: none may have shifted them in place
        assert np.array_equal(f["rating"].to_numpy(), before[name]), name


def _fit(stem, dtype, standin):
    """(reference fixture, fitted model, test frame, global mean): the fixture's run, through the product class."""
    ref = np.load(os.path.join(GOLDEN, stem + ".npz"))
    kind, cfg = str(ref["kind"]), json.loads(str(ref["cfg"]))
    train, test = standin["train"], standin["test"]
    val = pd.concat([standin[p] for p in str(ref["val_frames"]).split("+")], ignore_index=True)
    assert (len(train), len(val), len(test)) == (int(ref["n_train_rows"]), int(ref["n_val_rows"]), int(ref["n_test_rows"]))
    gm = 0.0
    if kind == "gauss_bias":                       # the drivers' centring (compare_models.py:54-65)
        gm = float(train["rating"].mean())
        assert gm == float(ref["global_mean"])
    shift = -gm if kind == "gauss_bias" else 1.0 if kind == "hpf" else 0.0     # the drivers' +1 shift (compare_models.py:180-185)
    # new frames: the stand-in is shared by every case of the module and must stay as it is (a concat of ONE frame
    # shares its columns with it)
    train, val, test = (f.assign(rating=f["rating"].to_numpy(dtype=float) + shift) for f in (train, val, test))
    t0 = time.perf_counter()
    if kind == "gauss_bias":
        from src.models.gaussian_mf_cavi_bias import GaussianMFCAVI, GaussianMFCAVIConfig
        m = GaussianMFCAVI(GaussianMFCAVIConfig(verbose=False, **cfg), dtype=dtype).fit(train, val_df=val, global_mean=gm)
    elif kind == "hpf":
        from src.models.hpf_cavi import HPF_CAVI, HPF_CAVI_Config
        m = HPF_CAVI(HPF_CAVI_Config(verbose=False, **cfg), dtype=dtype).fit(train, val_df=val)
    else:
        from src.models.poisson_mf_cavi import PoissonMFCAVI, PoissonMFCAVIConfig
        m = PoissonMFCAVI(PoissonMFCAVIConfig(verbose=False, **cfg), dtype=dtype).fit(train, val_df=val)
    print(f"\n{stem} {dtype}: fit {time.perf_counter() - t0:.2f} s, {m.history_['iterations']} iterations")
    return ref, m, test, gm


def _final_state(ref, m, test, gm):
    """What the fixture stores of the final state, from the fitted model: name -> (device value, reference value)."""
    kind = str(ref["kind"])
    got = {}
    for ids, names in zip((ref["users"], ref["items"]), TABLES[kind]):
        for name in names:
            table = np.asarray(getattr(m, name))
            got[name + "_rows"] = (table[ids], ref[name + "_rows"])
            got[name + "_sum"] = (table.sum(), float(ref[name + "_sum"]))
    tu, ti = test["u"].to_numpy(), test["i"].to_numpy()
    if kind == "gauss_bias":
        got["test_pred"] = (m.predict(tu, ti, gm), ref["test_pred"])
        got["test_rmse"] = (m.evaluate_rmse(test, gm), float(ref["test_rmse"]))
    else:
        got["test_pred"] = (m.predict(tu, ti), ref["test_pred"])
        got["test_rmse"] = (m.evaluate_rmse(test), float(ref["test_rmse"]))
    return got


def _max_rel(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / np.abs(want)))


def _first_out(got, want, bar, relative):
    """Index of the first entry that leaves the bar, for the failure message."""
    d = np.abs(np.asarray(got) - np.asarray(want)) / (np.abs(want) if relative else 1.0)
    return int(np.argmax(d > bar)) + 1 if np.any(d > bar) else None


@pytest.mark.parametrize("stem", ALL)
def test_f64_run_equals_the_reference_run(stem, standin):
    """The engine's float64 mode is the reference's own arithmetic up to summation order: the same number of
    iterations and the same early stop; every iteration's validation RMSE and MacroMAE, the sampled factor (and bias /
    prior-rate) rows, the sums of every table, the test predictions and the test RMSE at rtol 1e-8 with no absolute
    slack (the bar of test_drivers_gpu.py's 150-iteration float64 run); and the top-10 list of every one of the 300
    sampled users equal to the reference's, in order, with no tie tolerance.  The Gaussian lists come from
    `top_k_items` in bias mode: the fused scan's bias path on a fitted model."""
    ref, m, test, gm = _fit(stem, "f64", standin)
    try:
        hist = m.history_
        n = min(len(hist["val_rmse"]), len(ref["val_rmse"]))
        devs = {"val_rmse": _max_rel(hist["val_rmse"][:n], ref["val_rmse"][:n]),
                "val_macro_mae": _max_rel(hist["val_macro_mae"][:n], ref["val_macro_mae"][:n])}
        state = _final_state(ref, m, test, gm) if "users" in ref else {}
        devs.update({name: _max_rel(a, b) for name, (a, b) in state.items()})
        if state:
            items, scores = m.top_k_items(ref["users"], 10)
            devs["top10_scores"] = _max_rel(scores, ref["top11_scores"][:, :10])
            print("top-10 lists equal to the reference's, in order:", int(np.all(items == ref["top11"][:, :10], axis=1).sum()), "/ 300")
        print(f"{stem} f64 largest relative deviations:", json.dumps({k: float(f"{v:.3g}") for k, v in devs.items()}))
        assert hist["iterations"] == int(ref["iterations"]) and hist["stopped_early"] == bool(ref["stopped_early"])
        for key in ("val_rmse", "val_macro_mae"):
            assert devs[key] <= 1e-8, f"{key} leaves 1e-8 at iteration {_first_out(hist[key], ref[key], 1e-8, True)}"
        for name, (a, b) in state.items():
            np.testing.assert_allclose(a, b, rtol=1e-8, atol=0, err_msg=name)
        if state:
            assert len(ref["users"]) == 300
            np.testing.assert_array_equal(items, ref["top11"][:, :10])          # 300 / 300, in order, no tolerance
            np.testing.assert_allclose(scores, ref["top11_scores"][:, :10], rtol=1e-8, atol=0)
    finally:
        m.close()


@pytest.mark.parametrize("stem", STATEFUL)
def test_f32_run_stays_within_the_parity_bar_of_the_reference_run(stem, standin):
    """The default float32 storage against the reference's float64 run, at the bars of BASELINE.md section 3 and
    test_parity_bar_gpu.py: |dRMSE| <= 1e-4 at every iteration of the validation trajectory and on the test frame;
    sampled rows within 1e-3 of the reference, relative to the largest entry of the reference's rows of that table;
    the top-10 list of at least 297 of the 300 sampled users agrees, where an item whose reference score lies within
    1e-4 (relative) of the reference's 10th score does not count as a difference (`_topk_agree`'s rule; the fixture lists
    those items).  The early-stop fixture also fixes the stop: iteration 9, both neighbouring improvements more than
    twice the RMSE bar away from 0 and from tol (the sharp fixture is float64 only: +1.02e-5 cannot be decided here)."""
    ref, m, test, gm = _fit(stem, "f32", standin)
    try:
        hist = m.history_
        n = min(len(hist["val_rmse"]), len(ref["val_rmse"]))
        d_rmse = np.abs(np.asarray(hist["val_rmse"][:n]) - ref["val_rmse"][:n])
        d_mae = np.abs(np.asarray(hist["val_macro_mae"][:n]) - ref["val_macro_mae"][:n])
        state = _final_state(ref, m, test, gm)
        devs = {"val_rmse_abs": float(d_rmse.max()), "val_macro_mae_abs": float(d_mae.max()),
                "test_rmse_abs": abs(state["test_rmse"][0] - state["test_rmse"][1])}
        rows = {name: float(np.max(np.abs(a - b)) / np.max(np.abs(b))) for name, (a, b) in state.items() if name.endswith("_rows")}
        devs.update(rows)
        items, _ = m.top_k_items(ref["users"], 10)
        ptr, near = ref["near10_ptr"], ref["near10_items"]
        same = 0
        for row, got in enumerate(items):
            allowed = set(map(int, ref["top11"][row, :10])) | set(map(int, near[ptr[row]:ptr[row + 1]]))
            same += set(map(int, got)) <= allowed
        print(f"{stem} f32 largest deviations:", json.dumps({k: float(f"{v:.3g}") for k, v in devs.items()}),
              "top-10 agreement", same, "/ 300")
        assert hist["iterations"] == int(ref["iterations"]) and hist["stopped_early"] == bool(ref["stopped_early"])
        if stem.endswith("_stop"):
            assert hist["iterations"] == 9 and hist["stopped_early"]
        assert devs["val_rmse_abs"] <= 1e-4, f"validation RMSE leaves 1e-4 at iteration {_first_out(hist['val_rmse'][:n], ref['val_rmse'][:n], 1e-4, False)}"
        assert devs["test_rmse_abs"] <= 1e-4
        for name, dev in rows.items():
            assert dev <= 1e-3, name
        assert len(items) == 300 and same >= 297
    finally:
        m.close()
