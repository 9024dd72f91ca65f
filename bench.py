#!/usr/bin/env python3
"""Headline benchmark: whole-node CIFAR-10 CNN training throughput (images/sec) on MI355X.

Metric/config from BASELINE.json: "images/sec (whole node) CIFAR-10 CNN training at 1/2/4/8
MI355X"; model = the reference CNN (/root/reference/cifar10cnn.py:94-147, 24x24 center crop of
32x32x3 inputs), bf16 compute with fp32 master weights, per-GPU batch 256 (global 256*N), synthetic
uint8 images + random labels (no network), random-init weights.  Weak scaling: per-GPU work fixed.

Every timed step is a complete training step: gather/crop, forward, loss, backward, gradient
all-reduce (N>1, RCCL), SGD update with the on-device LR schedule.

  python bench.py --gpus N --steps K --warmup W
  torchrun --nproc-per-node N bench.py --gpus N ...     (the driver's launch for N > 1)
  python bench.py --impl eager                          (framework-default PyTorch eager line)
  python bench.py ... --dump-outputs DIR                (what the last timed step computed, as DIR/*.npy)

A plain run does only what the headline figure needs: set-up, warm-up, the timed steps, the result
line.  ``--full`` is the switch for measurements beyond the headline figure that take runs of their
own; this benchmark has none (every other configuration is a run with its own flags), so ``--full``
runs the same steps and says so in the result line.

``python bench.py --gpus N`` started WITHOUT a torchrun environment becomes a launcher: before any
GPU call it starts N rank processes of itself (RANK/LOCAL_RANK/WORLD_SIZE/MASTER_* set, rendezvous
on 127.0.0.1) and exits with their status, so --gpus N always measures N ranks.  Every rank checks
that the process group it joined really has --gpus ranks and exits non-zero otherwise.
"""
import argparse
import json
import os
import signal
import socket
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

BASELINE_VALUE = None   # the reference publishes no number


def _launch_ranks(n: int) -> int:
    """Launcher parent (never touches the GPU): N children of this script, one per GPU."""
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env,
                                      start_new_session=True))
    rc = 0
    try:
        live = list(procs)
        while live:
            for p in list(live):
                c = p.poll()
                if c is None:
                    continue
                live.remove(p)
                if c != 0 and rc == 0:
                    rc = c
                    for q in live:                   # a failed rank: stop the others, report its code
                        try:
                            os.killpg(q.pid, signal.SIGTERM)
                        except ProcessLookupError:
                            pass
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                try:
                    os.killpg(p.pid, signal.SIGKILL)
                except ProcessLookupError:
                    pass
                p.wait()
    return rc if rc >= 0 else 128 - rc


def _want_gpus(argv) -> int:
    for i, a in enumerate(argv):
        if a == "--gpus" and i + 1 < len(argv):
            return int(argv[i + 1])
        if a.startswith("--gpus="):
            return int(a.split("=", 1)[1])
    return 1


if __name__ == "__main__" and "WORLD_SIZE" not in os.environ and _want_gpus(sys.argv[1:]) > 1:
    sys.exit(_launch_ranks(_want_gpus(sys.argv[1:])))

import torch  # noqa: E402

import dmlc  # noqa: E402,F401
from dmlc.parallel import dist as D  # noqa: E402


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256, help="per-GPU batch")
    ap.add_argument("--impl", choices=["auto", "fused", "eager", "hipf32"], default="auto",
                    help="fused = hand-written HIP kernels + HIP graph (cifar_cnn); eager = PyTorch ops; "
                         "hipf32 = the fp32-accurate CNN on the fp32 MFMA HIP kernels (--dtype fp32)")
    ap.add_argument("--model", choices=["cifar_cnn", "resnet20"], default="cifar_cnn")
    ap.add_argument("--crop", type=int, default=None, help="input crop (default 24 for cifar_cnn, 32 for resnet20)")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--eager-graph", action="store_true",
                    help="capture the eager (PyTorch-op) step into a HIP graph (ResNet-20 path; the "
                         "framework-default comparison line is measured without it)")
    # the gradient wire of N > 1 (bf16 since r6: half the link bytes; 300-step DP-2 loss-curve parity
    # with the fp32 wire, tests/test_fused_dp_gpu.py::test_dp2_bf16_wire_loss_curve_tracks_fp32_wire)
    ap.add_argument("--comm-dtype", choices=["fp32", "bf16"], default="bf16")
    ap.add_argument("--allreduce", choices=["auto", "rccl", "xgmi"], default="auto",
                    help="gradient all-reduce (N>1): auto = xGMI peer-to-peer kernel when it self-tests "
                         "and measures faster than RCCL, else RCCL")
    ap.add_argument("--dp-schedule", choices=["auto", "overlap", "serial"], default="auto",
                    help="N>1 fused CNN step: overlap = fc all-reduce + fc SGD on a comm stream under the "
                         "conv backward; serial = one stream, one all-reduce; auto = measure both (before "
                         "the timed region) and keep the faster")
    ap.add_argument("--capture-comm", choices=["auto", "on", "off"], default="auto",
                    help="RCCL all-reduce inside the step HIP graph (auto: on over nccl)")
    ap.add_argument("--rccl-channels", type=int, default=0,
                    help="NCCL_MIN_NCHANNELS for RCCL over the 7 xGMI links (0 = RCCL's topology choice)")
    ap.add_argument("--settle-steps", type=int, default=256,
                    help="untimed replayed steps (graph rehearsal included) before the timed region")
    ap.add_argument("--steps-per-graph", type=int, default=32, help="longest chain of steps per graph replay")
    ap.add_argument("--dtype", choices=["bf16", "fp8", "fp32"], default="bf16",
                    help="fp8 = OCP e4m3 MFMA conv2 forward with delayed per-tensor scaling (config 5)")
    ap.add_argument("--dataset-size", type=int, default=50000)
    # The timed steps must train a LIVE network.  With the reference's lr 0.1 on raw 0..255 pixels and
    # random labels the weights are NaN within ~300 steps (every activation zero: profiles/
    # r4_settle_probe.jsonl), and with the reference's ReLU on the logits (D4) the logits die and every
    # gradient is exactly zero.  lr 1e-4 without the logit ReLU keeps activations AND gradients live
    # (loss 2.71 -> 2.46 over 2k steps).  The step time is the same in all of these regimes (80.5-82 us
    # at B=256 in every window of the probe): the number does not depend on it, but the run is valid.
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--relu-logits", action="store_true", help="the reference's ReLU on the logits (D4)")
    ap.add_argument("--variant", default="",
                    help="engine path choices for A/B runs, key=0|1,... (engine/fused.py VARIANT_DEFAULTS)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed to DIR/<name>.npy: "
                         "params (the fp32 flat weights after the step) and stats (global_step, loss, "
                         "accuracy, lr of the step); same arguments = same inputs, run to run")
    ap.add_argument("--full", action="store_true",
                    help="also run the measurements beyond the headline figure (none here: a plain run "
                         "already is the whole benchmark)")
    return ap.parse_args()


def _variant(spec: str) -> dict:
    out = {}
    for kv in filter(None, spec.split(",")):
        k, v = kv.split("=")
        out[k] = bool(int(v))
    return out


def make_data(n, device, seed=0):
    g = torch.Generator().manual_seed(seed)
    data = torch.randint(0, 256, (n, 32, 32, 3), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (n,), dtype=torch.int32, generator=g)
    return data.to(device), labels.to(device)


DUMP_CAP_BYTES = 60 << 20      # --dump-outputs writes at most this much in all


def dump_outputs(path, eng, step_no):
    """What a caller of the timed step holds after the last timed step: the updated fp32 weights
    (``params.npy``, float32) and the step's published statistics (``stats.npy``, float64:
    global_step, loss, accuracy, lr).  An output over the size cap is stored as a fixed, seeded
    sample of its elements (in index order)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    params = eng.flat_params().to(torch.float32).contiguous().numpy().reshape(-1)
    if params.nbytes > DUMP_CAP_BYTES:
        keep = np.random.default_rng(0).choice(params.size, DUMP_CAP_BYTES // params.itemsize, replace=False)
        params = params[np.sort(keep)]
    if hasattr(eng, "read_stats"):
        st = eng.read_stats(step_no)
        stats = [st["global_step"], st["loss"], st["accuracy"], st["lr"]]
    else:
        stats = [step_no, float(eng.last_loss), float(eng.last_acc), eng.lr(step_no - 1)]
    np.save(os.path.join(path, "params.npy"), params)
    np.save(os.path.join(path, "stats.npy"), np.asarray(stats, dtype=np.float64))


def build_fused(args, info, data, labels):
    if args.model == "resnet20":
        from dmlc.engine.fused_resnet import FusedResNetEngine
        eng = FusedResNetEngine(args.batch, data, labels, device=info.device, world_size=info.world_size,
                                rank=info.rank, seed=0, lr=min(args.lr, 0.01), comm_dtype=args.comm_dtype,
                                allreduce=args.allreduce, capture_comm=_capture_comm(args))
        return eng, eng.step, (None if args.no_graph else lambda: eng.capture(args.steps_per_graph))
    from dmlc.engine.fused import FusedCifarEngine
    eng = FusedCifarEngine(args.batch, data, labels, device=info.device, world_size=info.world_size,
                           rank=info.rank, seed=0, lr=args.lr, relu_logits=args.relu_logits,
                           comm_dtype=args.comm_dtype, dtype=args.dtype,
                           allreduce=args.allreduce, capture_comm=_capture_comm(args),
                           dp_schedule="serial" if args.dp_schedule == "auto" else args.dp_schedule,
                           variant=_variant(args.variant))
    step = eng.step
    return eng, step, (None if args.no_graph else lambda: eng.capture(args.steps_per_graph))


def _capture_comm(args):
    return None if args.capture_comm == "auto" else args.capture_comm == "on"


def build_eager(args, info, data, labels):
    from dmlc.engine.eager import EagerTrainer
    hipf32 = args.impl == "hipf32"
    tr = EagerTrainer(args.model, args.batch, data, labels, device=info.device, world_size=info.world_size,
                      rank=info.rank, dtype="fp32" if hipf32 or args.dtype == "fp32" else "bf16", crop=args.crop,
                      lr=min(args.lr, 0.01), relu_logits=args.relu_logits, graph=args.eager_graph or hipf32,
                      backend="hip_f32" if hipf32 else "torch")
    return tr, tr.step, None


def main():
    args = parse()
    info = D.init(D.env_info(), device="auto", rccl_channels=args.rccl_channels)
    import torch.distributed as dist
    seen = dist.get_world_size() if dist.is_initialized() else 1
    if seen != args.gpus or info.world_size != args.gpus:
        print(f"bench: --gpus {args.gpus} but this rank joined a world of {seen} (WORLD_SIZE={info.world_size})",
              file=sys.stderr, flush=True)
        D.shutdown(info)
        sys.exit(3)
    if args.impl == "auto":
        if args.dtype == "fp32":
            args.impl = "hipf32" if args.model == "cifar_cnn" and info.device.type == "cuda" else "eager"
        else:
            args.impl = "fused" if args.model == "cifar_cnn" or args.dtype == "bf16" else "eager"
    if args.impl == "hipf32":
        if args.model != "cifar_cnn" or info.world_size != 1:
            raise SystemExit("--impl hipf32 is the single-GPU fp32 reference-precision CNN path")
        args.dtype = "fp32"
    if args.crop is None:
        args.crop = 24 if args.model == "cifar_cnn" else 32
    if args.impl == "fused" and args.model == "cifar_cnn" and args.crop != 24:
        raise SystemExit("the fused HIP CNN engine implements the reference CNN at the 24x24 crop")
    if args.impl == "fused" and args.model == "resnet20" and (args.crop != 32 or args.dtype != "bf16"):
        raise SystemExit("the fused HIP ResNet-20 engine takes full 32x32 images in bf16")
    data, labels = make_data(args.dataset_size, info.device)
    builder = build_fused if args.impl == "fused" else build_eager
    eng, step, capture = builder(args, info, data, labels)

    def sync():
        if info.device.type == "cuda":
            torch.cuda.synchronize(info.device)

    n_eager = max(1, min(3, args.warmup))
    for _ in range(n_eager):                          # eager warm-up before capture
        step()
    graph_warm = 0
    if capture is not None:
        capture()
        if args.dp_schedule == "auto" and hasattr(eng, "tune_schedule") and info.world_size > 1:
            eng.tune_schedule(iters=max(10, args.warmup), steps_per_graph=args.steps_per_graph)
        # a short timed region replays as ONE graph of exactly --steps steps
        if args.steps <= 2 * args.steps_per_graph and hasattr(eng, "add_chain"):
            eng.add_chain(args.steps)
        # replay every captured chain once (first launches of a graph pay its upload): untimed
        # training steps on top of the W warm-up steps, reported as graph_warmup_steps
        for k in sorted(getattr(eng, "chains", {}) or {}):
            eng.run(k)
            graph_warm += k
        # ... and rehearse the timed region's own replay sequence once (short runs only)
        if args.steps <= 64:
            eng.run(args.steps)
            graph_warm += args.steps
        # ... and keep the GPU at sustained load for --settle-steps replayed steps in all (clocks /
        # power settle over ~10-20 ms: 20-step runs measured 2.98-3.02 M after ~110 untimed steps,
        # 3.05 M after ~300).  Untimed, counted in graph_warmup_steps.
        if args.settle_steps > graph_warm and hasattr(eng, "run"):
            eng.run(args.settle_steps - graph_warm)
            graph_warm = args.settle_steps
    # run(n): n complete steps, as chained graph replays (fused engines) or n step() calls
    run = getattr(eng, "run", None) if capture is not None else None
    if run is None:
        def run(n):
            for _ in range(n):
                step()
    run(max(0, args.warmup - n_eager))
    sync()
    def device_step():
        gs = getattr(eng, "global_step", None)
        return gs() if callable(gs) else gs

    gs0 = device_step()
    D.barrier(info)
    sync()
    t0 = time.perf_counter()
    run(args.steps)
    sync()
    D.barrier(info)
    sync()
    elapsed = D.all_max(time.perf_counter() - t0, info)
    if gs0 is not None:     # every timed step really ran: the device step counter agrees
        assert device_step() == gs0 + args.steps, (device_step(), gs0, args.steps)
    if hasattr(eng, "check_comm"):
        eng.check_comm()
    if hasattr(eng, "check_barriers"):
        eng.check_barriers()             # a timed-out wgrad+SGD barrier would make the numbers invalid
    comm = dict(getattr(eng, "comm_info", None) or {})
    comm.update(backend=info.backend if seen > 1 else "none", world_size_seen=seen,
                device_count=torch.cuda.device_count() if info.device.type == "cuda" else 0, device=str(info.device))
    if info.backend == "nccl" and seen > 1:
        comm["rccl_env"] = D.rccl_env()

    # the network the timed steps trained: finite weights, the last step's loss (device stats ring)
    net = {"lr": args.lr, "relu_logits": bool(args.relu_logits)}
    master = getattr(eng, "master", None)
    if master is not None:
        net["finite"] = bool(torch.isfinite(master).all())
        if not net["finite"]:
            raise SystemExit("bench: the weights went non-finite during the run (invalid measurement)")
    if hasattr(eng, "read_stats") and gs0 is not None:
        try:
            net["loss_last_step"] = round(float(eng.read_stats(device_step())["loss"]), 4)
        except Exception:
            pass
    if args.dump_outputs and info.rank == 0:     # the replicas hold the same weights: rank 0 writes
        dump_outputs(args.dump_outputs, eng, device_step())
    n = info.world_size
    ms = elapsed * 1000.0 / args.steps
    gbatch = args.batch * n
    value = gbatch * args.steps / elapsed
    if info.rank == 0:
        line = {
            "metric": "images/sec (whole node) CIFAR-10 CNN training at 1/2/4/8 MI355X",
            "value": round(value, 1),
            "unit": "images/sec",
            "n_gpus": n,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None if BASELINE_VALUE is None else round(value / BASELINE_VALUE, 4),
            "dtype": args.dtype,
            "data": "synthetic uint8 32x32x3 (50k images, device resident), random labels, random-init weights",
            "config": {
                "model": ("cifar10_cnn (conv5x5-64, pool, conv5x5-64, pool, fc384, fc192, fc10; 24x24 center crop)"
                          if args.model == "cifar_cnn" else f"resnet20 ({args.crop}x{args.crop} input)"),
                "global_batch": gbatch,
                "per_gpu_batch": args.batch,
                "seq_len": None,
                "parallelism": f"dp{n}",
                "impl": args.impl + ("+hipgraph" if (args.impl == "fused" and not args.no_graph)
                                     or (args.impl == "eager" and args.eager_graph) or args.impl == "hipf32"
                                     else ""),
                "comm_dtype": args.comm_dtype,
                "comm": comm,
                "graph_warmup_steps": graph_warm,
                "network": net,
                "steps_per_graph": args.steps_per_graph if capture is not None else None,
                **({"variant": args.variant} if args.variant else {}),
                **({"full": True} if args.full else {}),
            },
        }
        print(json.dumps(line), flush=True)
    D.shutdown(info)


if __name__ == "__main__":
    main()
