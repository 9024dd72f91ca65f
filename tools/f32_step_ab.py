#!/usr/bin/env python3
"""Time the fp32 HIP training step on ONE GPU, ReLU + pool and the loss head on their HIP kernels (fused)
against the same step with those as PyTorch ops (unfused):
   python tools/f32_step_ab.py [--batch 256] [--steps 300] [--rounds 3] [--out FILE]
Two hip_f32 EagerTrainers on the same synthetic data and seed, both graph-captured; after warm-up, --steps
steps per path are timed in interleaved rounds (unfused, fused, fused, unfused, ...), each window between two
device syncs; the minimum per path is kept and the per-round figures give the spread.  Before that, one eager
(uncaptured) step per path gives the peak of torch.cuda.max_memory_allocated over a step.  Prints one JSON
line per measurement and a summary line, and writes the summary to --out."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import dmlc  # noqa: E402,F401
from dmlc.engine.eager import EagerTrainer  # noqa: E402

PATHS = {"unfused": False, "fused": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(0)
    data = torch.randint(0, 256, (8192, 32, 32, 3), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (8192,), dtype=torch.int32, generator=g)
    kw = dict(device="cuda:0", dtype="fp32", lr=1e-5, seed=1, backend="hip_f32")

    peak = {}
    for name, fused in PATHS.items():                         # peak memory of one uncaptured step
        tr = EagerTrainer("cifar_cnn", a.batch, data, labels, fused=fused, **kw)
        for _ in range(2):
            tr.step()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        tr.step()
        torch.cuda.synchronize()
        peak[name] = {"peak_bytes": torch.cuda.max_memory_allocated(),
                      "above_resident_bytes": torch.cuda.max_memory_allocated() - base}
        print(json.dumps({"path": name, **peak[name]}), flush=True)
        del tr
        torch.cuda.empty_cache()

    trs = {name: EagerTrainer("cifar_cnn", a.batch, data, labels, fused=fused, graph=True, **kw)
           for name, fused in PATHS.items()}
    for tr in trs.values():                                   # 3 eager warm-up steps, capture, replays
        for _ in range(20):
            tr.step()
    torch.cuda.synchronize()
    assert all(tr.graph is not None for tr in trs.values())
    names = tuple(PATHS)
    rounds = {k: [] for k in names}
    for r in range(a.rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            tr = trs[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                tr.step()
            torch.cuda.synchronize()
            ms = 1e3 * (time.perf_counter() - t0) / a.steps
            rounds[name].append(round(ms, 4))
            print(json.dumps({"path": name, "round": r, "ms_per_step": round(ms, 4)}), flush=True)
    best = {k: min(v) for k, v in rounds.items()}
    spread = {k: round(max(v) - min(v), 4) for k, v in rounds.items()}
    summary = {"batch": a.batch, "dtype": "fp32", "steps": a.steps, "rounds": a.rounds, "graph": True,
               "ms_per_step_by_round": rounds, "min_ms_per_step": best, "spread_ms": spread,
               "images_per_s": {k: round(a.batch / v * 1e3) for k, v in best.items()},
               "speedup_fused_over_unfused": round(best["unfused"] / best["fused"], 3),
               "fused_wins_beyond_spread": best["unfused"] - best["fused"] > max(spread.values()),
               "eager_step_memory": peak,
               "last_loss": {k: float(tr.last_loss) for k, tr in trs.items()}}
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(summary) + "\n")


if __name__ == "__main__":
    main()
