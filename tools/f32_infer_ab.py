#!/usr/bin/env python3
"""Time EagerTrainer.evaluate of the hip_f32 backend on ONE GPU, the batch walk against the one-launch kernel:
   python tools/f32_infer_ab.py [--images 10000] [--batch 128] [--reps 20] [--rounds 3] [--out FILE]
One trainer (a few training steps so that the weights are a step's), a device-resident synthetic test
set; both paths are warmed up, then --reps evaluate() calls per path are timed in interleaved rounds
(batched, hip, hip, batched, ...), each call ending in the device sync of its accuracy read-back; the
minimum per path is kept and the per-round figures give the spread.  Prints one JSON line per
measurement and a summary line (with both paths' hit counts), and writes the summary to --out."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import dmlc  # noqa: E402,F401
from dmlc.engine.eager import EagerTrainer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(0)
    data = torch.randint(0, 256, (4096, 32, 32, 3), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (4096,), dtype=torch.int32, generator=g)
    tr = EagerTrainer("cifar_cnn", a.batch, data, labels, device="cuda:0", dtype="fp32", lr=1e-6, backend="hip_f32")
    for _ in range(4):
        tr.step()
    tx = torch.randint(0, 256, (a.images, 32, 32, 3), dtype=torch.uint8, generator=g).cuda()
    ty = torch.randint(0, 10, (a.images,), dtype=torch.int32, generator=g).cuda()
    paths = ("batched", "hip")
    acc = {}
    for impl in 2 * paths:                                  # warm-up: code objects, allocator, the scratch slabs
        acc[impl] = tr.evaluate(tx, ty, impl=impl)
    torch.cuda.synchronize()
    rounds = {k: [] for k in paths}
    for r in range(a.rounds):
        for impl in (paths if r % 2 == 0 else paths[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                tr.evaluate(tx, ty, impl=impl)              # ends in a device sync (the accuracy read-back)
            ms = 1e3 * (time.perf_counter() - t0) / a.reps
            rounds[impl].append(round(ms, 3))
            print(json.dumps({"impl": impl, "round": r, "ms_per_evaluate": round(ms, 3)}), flush=True)
    best = {k: min(v) for k, v in rounds.items()}
    summary = {"images": a.images, "batch": a.batch, "dtype": "fp32", "reps": a.reps, "rounds": a.rounds,
               "ms_per_evaluate_by_round": rounds, "min_ms_per_evaluate": best,
               "spread_ms": {k: round(max(v) - min(v), 3) for k, v in rounds.items()},
               "images_per_s": {k: round(a.images / v * 1e3) for k, v in best.items()},
               "speedup_hip_over_batched": round(best["batched"] / best["hip"], 2),
               "hits": {k: round(v * a.images) for k, v in acc.items()}}
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(summary) + "\n")


if __name__ == "__main__":
    main()
