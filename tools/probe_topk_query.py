"""What the query calls cost beside the item calls, at the shape of `bench.py --workload topk`:
top-10 of 100k items for 262,144 query users of 1M, K = 64, fp32.
    python tools/probe_topk_query.py [--steps N] [--small]
Per variant: wall ms per call (ids in, lists out) and the device ms per call under PMF_KERNEL_TOPK (for the query calls
that includes the staging kernels), then the ratios DESIGN.md quotes.  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "prob-matrix-factorization_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    import pmf_hip
    from pmf_hip import ARR_FACTOR, ARR_SCALE, ITEM, USER
    U, I, K, k, Q = (100_000, 10_000, 64, 10, 32_768) if args.small else (1_000_000, 100_000, 64, 10, 262_144)
    rng = np.random.default_rng(0)
    ctx = pmf_hip.Context(U, I, K, dtype="f32")
    ctx.set_array(USER, ARR_FACTOR, rng.gamma(0.5, 1.0, (U, K)))
    ctx.set_array(ITEM, ARR_FACTOR, rng.gamma(0.5, 1.0, (I, K)))
    ctx.set_array(USER, ARR_SCALE, rng.gamma(2.0, 1.0, U))
    ctx.set_array(ITEM, ARR_SCALE, rng.gamma(2.0, 1.0, I))
    users = rng.permutation(U)[:Q].astype(np.int32)
    factor = ctx.get_array(USER, ARR_FACTOR)[users]
    variants = {
        "topk_items": lambda: ctx.topk_items(users, k),
        "query_ids": lambda: ctx.topk_query(ITEM, k, ids=users, query_side=USER),
        "query_vector": lambda: ctx.topk_query(ITEM, k, factor=factor),
        "topk_items_scale": lambda: ctx.topk_items(users, k, use_bias=pmf_hip.PREDICT_SCALE),
        "query_ids_cosine": lambda: ctx.topk_query(ITEM, k, ids=users, query_side=USER, score=pmf_hip.SCORE_COSINE),
    }
    out = {"shape": {"U": U, "I": I, "K": K, "k": k, "Q": Q}, "steps": args.steps}
    ctx.prof_enable(True)
    for _ in range(2):                                   # two passes over the variants: the second is what is reported
        for name, call in variants.items():
            call()
            ctx.prof_reset()
            wall = []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                call()
                wall.append((time.perf_counter() - t0) * 1e3)
            ms, launches = ctx.prof_get()["topk"]
            out[name] = {"wall_ms": [round(w, 2) for w in wall], "wall_ms_median": float(np.median(wall)),
                         "device_ms": ms / args.steps, "launches_per_call": launches / args.steps}
    dev = lambda n: out[n]["device_ms"]
    wall = lambda n: out[n]["wall_ms_median"]
    out["ratios"] = {
        "ids_over_topk_items_device": dev("query_ids") / dev("topk_items"),
        "ids_over_topk_items_wall": wall("query_ids") / wall("topk_items"),
        "vector_over_ids_device": dev("query_vector") / dev("query_ids"),
        "vector_over_ids_wall": wall("query_vector") / wall("query_ids"),
        "cosine_over_scale_device": dev("query_ids_cosine") / dev("topk_items_scale"),
        "cosine_over_scale_wall": wall("query_ids_cosine") / wall("topk_items_scale"),
    }
    ctx.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
