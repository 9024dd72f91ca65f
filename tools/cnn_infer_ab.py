#!/usr/bin/env python3
"""Time FusedCifarEngine.evaluate on ONE GPU, the batched training-forward path against the one-launch kernel:
   python tools/cnn_infer_ab.py [--images 10000] [--batch 256] [--reps 5] [--rounds 3] [--fp8] [--out FILE]
One engine (batch 256, a few training steps so that the weights are a step's), a device-resident
synthetic test set; both paths are warmed up, then --reps evaluate() calls per path are timed in
interleaved rounds (batched, hip, hip, batched, ...), each call ending in the device sync of its accuracy
read-back; the minimum per path is kept and the per-round figures give the spread.  Prints one JSON line
per measurement and a summary line, and writes the summary to --out.  --fp8: the engine is a --dtype fp8
one (batched: its per-batch-scale fp8 conv2 forward; hip: the one-launch kernel's fp8 variant), and a bf16
engine trained the same way adds the bf16 one-launch kernel as a third, recorded path (hip_bf16)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import dmlc  # noqa: E402,F401
from dmlc.engine.fused import FusedCifarEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fp8", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(0)
    data = torch.randint(0, 256, (4096, 32, 32, 3), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (4096,), dtype=torch.int32, generator=g)
    engs = {}
    for dt in (("fp8", "bf16") if a.fp8 else ("bf16",)):
        engs[dt] = FusedCifarEngine(a.batch, data, labels, device="cuda:0", lr=1e-4, dtype=dt)
        engs[dt].capture(steps_per_graph=8)
        engs[dt].run(16)
    eng = engs["fp8" if a.fp8 else "bf16"]
    # path -> (engine, evaluate's impl)
    paths = {"batched": (eng, "batched"), "hip": (eng, "hip")}
    if a.fp8:
        paths["hip_bf16"] = (engs["bf16"], "hip")
    tx = torch.randint(0, 256, (a.images, 32, 32, 3), dtype=torch.uint8, generator=g).cuda()
    ty = torch.randint(0, 10, (a.images,), dtype=torch.int32, generator=g).cuda()
    acc = {}
    for impl in 2 * tuple(paths):                          # warm-up: code objects, the scratch slabs
        acc[impl] = paths[impl][0].evaluate(tx, ty, impl=paths[impl][1])
    torch.cuda.synchronize()
    rounds = {k: [] for k in paths}
    for r in range(a.rounds):
        for impl in (tuple(paths) if r % 2 == 0 else tuple(paths)[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                paths[impl][0].evaluate(tx, ty, impl=paths[impl][1])   # ends in a device sync (the accuracy read-back)
            ms = 1e3 * (time.perf_counter() - t0) / a.reps
            rounds[impl].append(round(ms, 3))
            print(json.dumps({"impl": impl, "round": r, "ms_per_evaluate": round(ms, 3)}), flush=True)
    best = {k: min(v) for k, v in rounds.items()}
    summary = {"images": a.images, "batch": a.batch, "dtype": "fp8" if a.fp8 else "bf16", "reps": a.reps, "rounds": a.rounds,
               "ms_per_evaluate_by_round": rounds, "min_ms_per_evaluate": best,
               "spread_ms": {k: round(max(v) - min(v), 3) for k, v in rounds.items()},
               "images_per_s": {k: round(a.images / v * 1e3) for k, v in best.items()},
               "speedup_hip_over_batched": round(best["batched"] / best["hip"], 2), "accuracy": acc}
    if a.fp8:
        summary["speedup_hip_fp8_over_hip_bf16"] = round(best["hip_bf16"] / best["hip"], 2)
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(summary) + "\n")


if __name__ == "__main__":
    main()
