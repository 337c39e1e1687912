"""The CPU oracle (oracle/cavi_oracle.py, vectorised form) at the reference's published operating points, against
the reference's own runs (tests/golden/op_*.npz; tests/test_operating_points_gpu.py holds the device to the same files),
and a check that the float64 bar of that GPU test has teeth at this problem's conditioning.

The 100- and 150-iteration states stay GPU-only: here the Gaussian early-stop runs (9 and 10 iterations) and the
20-iteration states of the HPF and Poisson fixtures."""
import glob
import json
import os

import numpy as np
import pandas as pd
import pytest

from helpers import GOLDEN, recipe_standin
from oracle import cavi_oracle as orc

STATE = dict(rtol=1e-9, atol=1e-12)      # the oracle's state bar of tests/test_oracle_golden.py


def _ref(stem):
    ref = np.load(os.path.join(GOLDEN, stem + ".npz"))
    return ref, json.loads(str(ref["cfg"]))


@pytest.fixture(scope="module")
def standin():
    return dict(zip(("train", "validation", "test"), recipe_standin()))


def _arrays(frame, shift=0.0):
    return frame["u"].to_numpy(), frame["i"].to_numpy(), frame["rating"].to_numpy(dtype=float) + shift


def _gauss_fit(standin, stem, **override):
    """The oracle's run of a Gaussian fixture's problem: (fixture, state, history, global mean)."""
    ref, cfg = _ref(stem)
    gm = float(standin["train"]["rating"].mean())
    assert gm == float(ref["global_mean"])
    val = pd.concat([standin[p] for p in str(ref["val_frames"]).split("+")], ignore_index=True)
    assert (len(standin["train"]), len(val)) == (int(ref["n_train_rows"]), int(ref["n_val_rows"]))
    st, hist = orc.fit("gauss_bias", *_arrays(standin["train"], -gm), dict(cfg, **override), val=_arrays(val, -gm),
                       global_mean=gm, vectorised=True)
    return ref, st, hist, gm


def _gauss_rows(ref, st):
    """name -> (oracle value, reference value) of the sampled rows."""
    users, items = ref["users"], ref["items"]
    return {"m_theta_rows": (st["m_theta"][users], ref["m_theta_rows"]), "m_beta_rows": (st["m_beta"][items], ref["m_beta_rows"]),
            "m_user_bias_rows": (st["m_user_bias"][users], ref["m_user_bias_rows"]),
            "m_item_bias_rows": (st["m_item_bias"][items], ref["m_item_bias_rows"])}


def _max_rel(got, want):
    return float(np.max(np.abs(np.asarray(got) - want) / np.abs(want)))


@pytest.fixture(scope="module")
def stop_run(standin):
    return _gauss_fit(standin, "op_gauss_bias_k30_stop")


def test_operating_point_fixtures_are_complete_and_small():
    names = {os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "op_*.npz"))}
    assert names == {"op_gauss_bias_k30_stop", "op_gauss_bias_k30_stop_sharp", "op_gauss_bias_k30_long", "op_hpf_k20",
                     "op_poisson_k40"}
    for name in names:
        ref, cfg = _ref(name)
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 1 << 20
        assert len(ref["val_rmse"]) == len(ref["val_macro_mae"]) == int(ref["iterations"])
        assert bool(ref["stopped_early"]) == (int(ref["iterations"]) < cfg["max_iter"])
        assert ("users" in ref) == (name != "op_gauss_bias_k30_stop_sharp")
    # the three Gaussian runs train on the same frame: their validation-frame trajectories share a prefix, bit for bit
    stop, sharp, long_ = (_ref("op_gauss_bias_k30_" + n)[0] for n in ("stop", "stop_sharp", "long"))
    assert (int(stop["iterations"]), int(sharp["iterations"]), int(long_["iterations"])) == (9, 10, 100)
    for key, own in (("val_rmse", "validation_rmse"), ("val_macro_mae", "validation_macro_mae")):
        assert np.array_equal(sharp[key], long_[key][:10]) and np.array_equal(stop[own], long_[key][:9])
    # the margins the stop fixtures were chosen for
    imp = -np.diff(stop["val_rmse"])
    assert imp[-1] > 2e-4 and imp[-1] < 1e-3 - 2e-4 and imp[-2] < -2e-4
    assert 0 < -np.diff(sharp["val_rmse"])[-1] < 2e-5


def test_oracle_reproduces_the_gaussian_early_stop_run_in_full(stop_run, standin):
    """Published Gaussian configuration, val_df = validation + test: trajectory at rtol 1e-10, the stop at iteration 9,
    sampled rows, table sums, test predictions and the top-10 lists."""
    ref, st, hist, gm = stop_run
    assert hist["iterations"] == 9 == int(ref["iterations"]) and hist["stopped_early"] and bool(ref["stopped_early"])
    np.testing.assert_allclose(hist["val_rmse"], ref["val_rmse"], rtol=1e-10, atol=0)
    np.testing.assert_allclose(hist["val_macro_mae"], ref["val_macro_mae"], rtol=1e-10, atol=0)
    for name, (got, want) in _gauss_rows(ref, st).items():
        np.testing.assert_allclose(got, want, err_msg=name, **STATE)
    for name in ("m_theta", "m_beta", "m_user_bias", "m_item_bias"):
        np.testing.assert_allclose(st[name].sum(), float(ref[name + "_sum"]), rtol=1e-9)
    test = standin["test"]
    pred = orc.predict_dot(st["m_theta"], st["m_beta"], test["u"].to_numpy(), test["i"].to_numpy(), st["m_user_bias"],
                           st["m_item_bias"], gm)
    np.testing.assert_allclose(pred, ref["test_pred"], **STATE)
    np.testing.assert_allclose(orc.rmse(test["rating"].to_numpy(dtype=float), pred), float(ref["test_rmse"]), rtol=1e-10)
    users = ref["users"]
    scores = st["m_theta"][users] @ st["m_beta"].T + st["m_user_bias"][users][:, None] + st["m_item_bias"][None, :]
    top = np.argsort(-scores, axis=1, kind="stable")[:, :10]
    np.testing.assert_array_equal(top, ref["top11"][:, :10])


def test_oracle_reproduces_the_sharp_gaussian_early_stop(standin):
    """val_df = the validation frame: the stop at iteration 10 hangs on an improvement of +1.02e-5."""
    ref, st, hist, _ = _gauss_fit(standin, "op_gauss_bias_k30_stop_sharp")
    assert hist["iterations"] == 10 == int(ref["iterations"]) and hist["stopped_early"]
    np.testing.assert_allclose(hist["val_rmse"], ref["val_rmse"], rtol=1e-10, atol=0)
    np.testing.assert_allclose(hist["val_macro_mae"], ref["val_macro_mae"], rtol=1e-10, atol=0)


def test_the_f64_bar_catches_a_relative_error_of_1e_6_in_sigma2(standin, stop_run):
    """The bar has teeth: the same run with sigma2 scaled by (1 + 1e-6) -- a stand-in for a kernel whose arithmetic is
    off by that much -- must FAIL the float64 comparison of tests/test_operating_points_gpu.py (rtol 1e-8, no absolute
    slack) on the trajectory and on the sampled rows, while the unperturbed oracle passes it."""
    ref, st, hist, _ = stop_run
    assert max(_max_rel(hist[k], ref[k]) for k in ("val_rmse", "val_macro_mae")) <= 1e-8
    assert max(_max_rel(a, b) for a, b in _gauss_rows(ref, st).values()) <= 1e-8
    sigma2 = json.loads(str(ref["cfg"]))["sigma2"]
    _, st_p, hist_p, _ = _gauss_fit(standin, "op_gauss_bias_k30_stop", sigma2=sigma2 * (1 + 1e-6))
    n = min(len(hist_p["val_rmse"]), len(ref["val_rmse"]))
    traj = _max_rel(hist_p["val_rmse"][:n], ref["val_rmse"][:n])
    rows = {name: _max_rel(a, b) for name, (a, b) in _gauss_rows(ref, st_p).items()}
    print("sigma2 * (1 + 1e-6): validation RMSE off by", traj, "rows by", rows)
    assert traj > 1e-8
    assert all(v > 1e-8 for v in rows.values()), rows


@pytest.mark.parametrize("stem,kind", [("op_hpf_k20", "hpf"), ("op_poisson_k40", "poisson")])
def test_oracle_reproduces_the_20_iteration_state_of_the_gamma_fixtures(stem, kind, standin):
    ref, cfg = _ref(stem)
    shift = 1.0 if kind == "hpf" else 0.0        # the drivers' +1 shift (compare_models.py:180-185)
    n_it = int(ref["early_iterations"])
    assert (len(standin["train"]), len(standin["validation"])) == (int(ref["n_train_rows"]), int(ref["n_val_rows"]))
    st, hist = orc.fit(kind, *_arrays(standin["train"], shift), dict(cfg, max_iter=n_it),
                       val=_arrays(standin["validation"], shift), vectorised=True)
    assert hist["iterations"] == n_it == 20 and not hist["stopped_early"]
    np.testing.assert_allclose(hist["val_rmse"], ref["val_rmse"][:n_it], rtol=1e-10, atol=0)
    np.testing.assert_allclose(hist["val_macro_mae"], ref["val_macro_mae"][:n_it], rtol=1e-10, atol=0)
    users, items = ref["users"], ref["items"]
    for name, ids in (("E_theta", users), ("E_beta", items)) + ((("E_xi", users), ("E_eta", items)) if kind == "hpf" else ()):
        np.testing.assert_allclose(st[name][ids], ref[f"{name}_rows_it{n_it}"], err_msg=name, **STATE)
    test = standin["test"]
    pred = orc.predict_dot(st["E_theta"], st["E_beta"], test["u"].to_numpy(), test["i"].to_numpy())
    np.testing.assert_allclose(pred, ref[f"test_pred_it{n_it}"], **STATE)
