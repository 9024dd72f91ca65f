#!/usr/bin/env python3
"""Time the fused ResNet-20 step with SGD momentum + weight decay against the plain one on ONE GPU:
   python tools/rn_momentum_ab.py [--batches 256] [--steps 300] [--rounds 3] [--first plain|momentum]
Two engines per batch size in one process -- momentum / weight decay off and on (0.9 / 5e-4), the
bench's settings otherwise (lr 0.01, synthetic data, chained step graphs) -- each settled for 256
steps, then --steps timed in interleaved rounds (off, on, on, off, ...); the minimum per engine is kept.
--first picks which engine is built first: two engines of one process differ by where their buffers
landed, so a difference that follows the build order is placement, not the optimizer.
Prints one JSON line per measurement and one summary line per batch size."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import dmlc  # noqa: E402,F401
from dmlc.engine.fused_resnet import FusedResNetEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--momentum", type=float, default=0.9)
    ap.add_argument("--weight_decay", type=float, default=5e-4)
    ap.add_argument("--first", choices=["plain", "momentum"], default="plain", help="the engine built first")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(0)
    data = torch.randint(0, 256, (50000, 32, 32, 3), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (50000,), dtype=torch.int32, generator=g)
    for B in (int(b) for b in a.batches.split(",")):
        engines = {}
        for name in (("plain", "momentum") if a.first == "plain" else ("momentum", "plain")):
            on = name == "momentum"
            eng = FusedResNetEngine(B, data, labels, device="cuda:0", lr=0.01, momentum=a.momentum if on else 0.0,
                                    weight_decay=a.weight_decay if on else 0.0)
            eng.step()
            eng.capture(steps_per_graph=32)
            eng.run(256)
            engines[name] = eng
        torch.cuda.synchronize()
        best = {}
        for r in range(a.rounds):
            for name in (("plain", "momentum") if r % 2 == 0 else ("momentum", "plain")):
                eng = engines[name]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.run(a.steps)
                torch.cuda.synchronize()
                us = 1e6 * (time.perf_counter() - t0) / a.steps
                assert torch.isfinite(eng.master).all()
                best[name] = min(best.get(name, 1e30), us)
                print(json.dumps({"batch": B, "engine": name, "round": r, "us_per_step": round(us, 2)}), flush=True)
        print(json.dumps({"batch": B, "steps": a.steps, "rounds": a.rounds, "momentum": a.momentum,
                          "weight_decay": a.weight_decay, "built_first": a.first,
                          "min_us_per_step": {k: round(v, 2) for k, v in best.items()},
                          "momentum_cost_us": round(best["momentum"] - best["plain"], 2)}), flush=True)
        del engines
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
