#!/usr/bin/env python3
"""Time the augmented training step against the plain one on ONE GPU:
   python tools/aug_ab.py [--batches 256,128] [--steps 300] [--rounds 3]
Two engines per batch size in one process -- ``augment`` off and on, the bench's settings (lr 1e-4,
no logit ReLU, synthetic data, chained step graphs) -- each settled for 256 steps, then --steps timed
in interleaved rounds (off, on, on, off, ...); the minimum per engine is kept.
Prints one JSON line per measurement and one summary line per batch size."""
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
    ap.add_argument("--batches", default="256,128")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--dtype", choices=["bf16", "fp8"], default="bf16")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(0)
    data = torch.randint(0, 256, (50000, 32, 32, 3), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (50000,), dtype=torch.int32, generator=g)
    for B in (int(b) for b in a.batches.split(",")):
        engines = {}
        for name in ("plain", "augment"):
            eng = FusedCifarEngine(B, data, labels, device="cuda:0", lr=1e-4, relu_logits=False, dtype=a.dtype,
                                   augment=name == "augment")
            eng.step()
            eng.capture(steps_per_graph=32)
            eng.run(256)
            engines[name] = eng
        torch.cuda.synchronize()
        best = {}
        for r in range(a.rounds):
            for name in (("plain", "augment") if r % 2 == 0 else ("augment", "plain")):
                eng = engines[name]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.run(a.steps)
                torch.cuda.synchronize()
                us = 1e6 * (time.perf_counter() - t0) / a.steps
                eng.check_barriers()
                assert torch.isfinite(eng.master).all()
                best[name] = min(best.get(name, 1e30), us)
                print(json.dumps({"batch": B, "engine": name, "round": r, "us_per_step": round(us, 2)}), flush=True)
        print(json.dumps({"batch": B, "dtype": a.dtype, "steps": a.steps, "rounds": a.rounds,
                          "min_us_per_step": {k: round(v, 2) for k, v in best.items()},
                          "augment_cost_us": round(best["augment"] - best["plain"], 2)}), flush=True)
        del engines
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
