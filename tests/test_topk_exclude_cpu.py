"""Host side of top-k without the user's training items (`pmf_topk_items_excluding`): the NumPy reference the GPU tests
compare with, pinned on a hand-written case; the binding; and what the model method raises without a GPU."""
import numpy as np
import pandas as pd
import pytest

from topk_exclude_reference import topk_excluding, train_sets


def test_reference_on_a_hand_written_case():
    nan = float("nan")
    #            item 0    1    2    3    4    5
    full = np.array([[5.0, 7.0, 7.0, nan, 7.0, 1.0],     # user 0: tie group {1, 2, 4} on top, its lowest id excluded
                     [3.0, 9.0, nan, 2.0, 2.0, 8.0],     # user 1: fewer than k candidates
                     [0.0, -0.0, 1.0, nan, -1.0, 0.0]])  # user 2: nothing excluded; zeros of both signs tie
    train = {0: [1, 1], 1: {1, 5, 0, 2}}                 # (a repeated item; user 1's list holds the NaN item too)
    items, scores = topk_excluding(full, [0, 1, 2, 0], train, 4)
    assert items.dtype == np.int32 and scores.dtype == np.float64
    assert items.tolist() == [[2, 4, 0, 5], [3, 4, -1, -1], [2, 0, 1, 5], [2, 4, 0, 5]]
    assert scores.tolist() == [[7.0, 7.0, 5.0, 1.0], [2.0, 2.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [7.0, 7.0, 5.0, 1.0]]
    plain, _ = topk_excluding(full, [0, 1], None, 3)
    assert plain.tolist() == [[1, 2, 4], [1, 5, 0]]      # the NaN item never ranks, excluded or not
    everything, s = topk_excluding(full, [1], {1: range(6)}, 2)
    assert everything.tolist() == [[-1, -1]] and s.tolist() == [[0.0, 0.0]]
    assert train_sets([3, 3, 1, 3], [2, 2, 0, 5]) == {3: {2, 5}, 1: {0}}


def test_binding_declares_the_new_entry_point():
    import ctypes as C

    import pmf_hip
    restype, argtypes = pmf_hip.SIGNATURES["pmf_topk_items_excluding"]
    plain = pmf_hip.SIGNATURES["pmf_topk_items"][1]
    assert restype is C.c_int and argtypes == plain[:5] + [C.c_int] + plain[5:]      # `exclude_train` after `use_bias`


def _unfitted():
    from src.models.hpf_cavi import HPF_CAVI, HPF_CAVI_Config
    return HPF_CAVI(HPF_CAVI_Config(n_factors=4, max_iter=1, verbose=False))


def test_top_k_items_of_an_unfitted_model_raises_as_before():
    m = _unfitted()
    with pytest.raises(RuntimeError, match="has not been fitted"):
        m.top_k_items([0], 3)
    with pytest.raises(RuntimeError, match="has not been fitted"):
        m.top_k_items([0], 3, exclude_train=True)


def test_exclude_train_after_a_sharded_fit_is_refused_like_heldout_ranks():
    """After a sharded fit the full-size context holds no ratings: both methods refuse with one message."""
    m = _unfitted()
    m._ctx, m._shard_ctx = object(), object()            # (what _finish_sharded leaves behind; neither is touched)
    with pytest.raises(NotImplementedError, match="exclude_train=True is not available") as topk:
        m.top_k_items([0], 3, exclude_train=True)
    with pytest.raises(NotImplementedError) as ranks:
        m.heldout_ranks(pd.DataFrame({"u": [0], "i": [0], "rating": [1.0]}))
    assert str(topk.value) == str(ranks.value)
    m._ctx = m._shard_ctx = None                          # (nothing for close() to release)
