#!/usr/bin/env python3
"""Time the fp32 HIP training step on ONE GPU with conv2 on its direct kernels (csrc/kernels/f32_conv.hip)
against the same step with conv2 on the implicit GEMM:
   python tools/f32_conv_ab.py [--stage conv2|conv1|fc] [--batches 256,128] [--steps 300] [--rounds 3] [--out FILE]
Per batch size, one hip_f32 EagerTrainer per path on the same synthetic data and seed -- conv2_impl="gemm",
"direct" (forward and data gradient on k_f32_conv2) and "direct_all" (the weight gradient on
k_f32_conv2_wgrad as well) --, all graph-captured; after warm-up, --steps steps per path are timed in
interleaved rounds (gemm, direct, direct_all, direct_all, direct, gemm, ...), each window between two device
syncs; the minimum per path is kept and the per-round figures give the spread.  All trainers have then run
the same number of steps: the relative difference of their flat parameters to the GEMM path's is reported
too.  Prints one JSON line per measurement and a summary line per batch size, and writes the summaries to
--out.  ops/f32.py CONV2_IMPL_F32 follows "direct_wins_beyond_spread" (direct against gemm) and
"direct_all_wins_beyond_spread" (direct_all against direct, by more than the larger spread of those two) at
B = 256.
--stage conv1 times conv1's backward instead (conv2 on its default): conv1_impl="gemm" (f32_relu_pool_bwd + the
implicit GEMM) against "direct" (one launch of k_f32_conv1_wgrad, csrc/kernels/f32_conv1.hip); ops/f32.py
CONV1_IMPL_F32 follows its "direct_wins_beyond_spread" at B = 256.
--stage fc times the fc stack (the convs on their defaults): fc_impl="gemm" (the _Linear GEMM chain, f32_colsum and the
PyTorch ReLUs) against "fused" (csrc/kernels/f32_fc.hip); ops/f32.py FC_IMPL_F32 follows its
"fused_wins_beyond_spread" at B = 256."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import dmlc  # noqa: E402,F401
from dmlc.engine.eager import EagerTrainer  # noqa: E402

STAGES = {"conv2": ("conv2_impl", ("gemm", "direct", "direct_all")), "conv1": ("conv1_impl", ("gemm", "direct")),
          "fc": ("fc_impl", ("gemm", "fused"))}


def run(batch, steps, rounds, data, labels, stage="conv2"):
    key, PATHS = STAGES[stage]
    kw = dict(device="cuda:0", dtype="fp32", lr=1e-5, seed=1, backend="hip_f32", graph=True)
    trs = {name: EagerTrainer("cifar_cnn", batch, data, labels, **{key: name}, **kw) for name in PATHS}
    for tr in trs.values():                                   # 3 eager warm-up steps, capture, replays
        for _ in range(20):
            tr.step()
    torch.cuda.synchronize()
    assert all(tr.graph is not None for tr in trs.values())
    per_round = {k: [] for k in PATHS}
    for r in range(rounds):
        for name in (PATHS if r % 2 == 0 else PATHS[::-1]):
            tr = trs[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.step()
            torch.cuda.synchronize()
            ms = 1e3 * (time.perf_counter() - t0) / steps
            per_round[name].append(round(ms, 4))
            print(json.dumps({"batch": batch, "stage": stage, "path": name, "round": r, "ms_per_step": round(ms, 4)}), flush=True)
    best = {k: min(v) for k, v in per_round.items()}
    spread = {k: round(max(v) - min(v), 4) for k, v in per_round.items()}
    flat = {k: tr.model.flat.detach().double() for k, tr in trs.items()}
    out = {"batch": batch, "stage": stage, "dtype": "fp32", "steps": steps, "rounds": rounds, "graph": True,
           "ms_per_step_by_round": per_round, "min_ms_per_step": best, "spread_ms": spread,
           "images_per_s": {k: round(batch / v * 1e3) for k, v in best.items()},
           f"speedup_{PATHS[1]}_over_gemm": round(best["gemm"] / best[PATHS[1]], 3),
           f"{PATHS[1]}_wins_beyond_spread": best["gemm"] - best[PATHS[1]] > max(spread["gemm"], spread[PATHS[1]])}
    if stage == "conv2":
        out.update({"speedup_direct_all_over_direct": round(best["direct"] / best["direct_all"], 3),
                    "direct_all_wins_beyond_spread":
                        best["direct"] - best["direct_all"] > max(spread["direct"], spread["direct_all"])})
    out.update({"steps_run_per_path": 20 + steps * rounds,
                "flat_params_rel_diff": {k: float((flat[k] - flat["gemm"]).norm() / flat["gemm"].norm())
                                         for k in PATHS[1:]},
                "last_loss": {k: float(tr.last_loss) for k, tr in trs.items()}})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stage", default="conv2", choices=sorted(STAGES))
    ap.add_argument("--batches", default="256,128")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(0)
    data = torch.randint(0, 256, (8192, 32, 32, 3), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (8192,), dtype=torch.int32, generator=g)
    summaries = [run(int(b), a.steps, a.rounds, data, labels, a.stage) for b in a.batches.split(",")]
    for s in summaries:
        print(json.dumps(s), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.writelines(json.dumps(s) + "\n" for s in summaries)


if __name__ == "__main__":
    main()
