"""What the fused engines (engine/fused.py, engine/fused_resnet.py) do the same way: the process and
schedule fields, the device-resident data and its generated order, the step counters and stats ring,
the choice of the gradient all-reduce, and the capture of the step into HIP graphs with their replay.

An engine provides ``_eager_step`` (one step's launches on the current stream) and, for a step that
is several graphs around eager collectives, ``_segments`` and ``_replay_segments``.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from ..data.order import OrderSpec
from ..ops import _ext
from ..parallel.dist import quiesce_for_capture
from .plan import TICKET_WORDS

OPS = None


def _ops():
    global OPS
    if OPS is None:
        _ext.hip()
        OPS = torch.ops.dmlc
    return OPS


class FusedEngineBase:
    def __init__(self, *, device, world_size: int, rank: int, process_group, seed: int, comm_dtype: str, lr: float,
                 lr_decay: float, decay_steps: float, staircase: bool, warmup_steps: int, dp_force: bool,
                 capture_comm: Optional[bool], stats_len: int):
        self.ops = _ops()
        self.device = dev = torch.device(device or "cuda")
        self.world_size, self.rank, self.pg = world_size, rank, process_group
        self.lr0, self.decay, self.decay_steps, self.staircase = lr, lr_decay, decay_steps, staircase
        self.warmup = float(warmup_steps)      # linear LR warm-up (large-batch recipe), in the SGD kernel
        self.seed, self.comm_dtype = seed, comm_dtype
        # dp_force: run the data-parallel step (all-reduce + apply) even at world_size 1 (tests)
        self.dp = world_size > 1 or dp_force
        if capture_comm is None:     # RCCL collectives go into the step graph unless told otherwise
            capture_comm = self.dp and self._pg_backend() == "nccl"
        self.capture_comm = bool(capture_comm)
        self.xgmi, self.comm_info = None, {"allreduce": "rccl" if self.dp else "none"}
        self.step_t = torch.zeros(1, dtype=torch.int64, device=dev)
        # the head kernel copies the step counter here for the SGD (cnn_sgd.hip; the ResNet-20 SGD takes
        # an arrival ticket instead, see fused_resnet.py)
        self.step_sgd = torch.zeros(1, dtype=torch.int64, device=dev)
        self.ticket = torch.zeros(TICKET_WORDS, dtype=torch.int32, device=dev)   # two-level arrival counters
        self.stats = torch.zeros(stats_len, 4, dtype=torch.float32, device=dev)
        self.graphs: List[torch.cuda.CUDAGraph] = []
        self.chains: Dict[int, Optional[torch.cuda.CUDAGraph]] = {}   # k -> graph of k chained steps
        self.host_step = 0

    def _select_xgmi(self, n_flat: int, pattern, allreduce: str):
        """Gradient all-reduce (N > 1): the xGMI peer-to-peer kernel over an IPC-shared gradient buffer
        when every rank can map every peer and it measures faster than RCCL (parallel/xgmi.py), else
        RCCL.  ``pattern``: the (offset, count) calls one step issues, which is what gets timed."""
        if (self.world_size > 1 and self.device.type == "cuda" and self.comm_dtype in ("fp32", "bf16")
                and allreduce != "rccl"):
            from ..parallel import xgmi as X
            self.xgmi, self.comm_info = X.select(n_flat, self.rank, self.world_size, self.device, pattern,
                                                 mode=allreduce, group=self.pg, wire=self.comm_dtype,
                                                 captured=self.capture_comm)

    def _flat_grad(self, master: torch.Tensor, always: bool) -> Optional[torch.Tensor]:
        """The flat gradient: a view of the xGMI buffer where that exchanges it, else a buffer of its own
        (``always``, or only for the data-parallel step)."""
        if self.xgmi is not None:
            grad = self.xgmi.buf[:master.numel()]
            grad.zero_()
            return grad
        return torch.zeros_like(master) if always or self.dp else None

    def _init_batch(self, data: torch.Tensor, labels: torch.Tensor, B: int, Bv: int):
        """The device-resident data set, its generated order (data/order.py) and the logits of one
        kernel batch of ``B`` rows, ``Bv`` of them real."""
        dev = self.device
        self.B, self.Bv = B, Bv
        assert data.dtype == torch.uint8 and tuple(data.shape[1:]) == (32, 32, 3)
        self.data = data.to(dev).contiguous()
        self.labels = labels.to(dev, torch.int32).contiguous()
        self.n_data = self.data.shape[0]
        self.order = OrderSpec(self.n_data, Bv, self.world_size, self.rank, self.seed)
        self.period = self.order.period             # steps per epoch
        self.order_desc = self.order.descriptor()   # host int64 [6]: the generated order
        self.logits_buf = torch.zeros(B, 10, dtype=torch.float32, device=dev)

    # --- data order ---------------------------------------------------------------------------
    def epoch_permutation(self, epoch: int) -> torch.Tensor:
        """This rank's dataset rows for ``epoch`` (int32 [period * Bv], batch after batch): the
        generated order the kernels evaluate in place (data/order.py; D6: disjoint rank shards)."""
        return self.order.epoch_shard(epoch).to(torch.int32)

    def batch_indices(self, step: int) -> torch.Tensor:
        """Dataset rows (int32 [Bv]) this rank trains on at global step ``step``."""
        return self.order.batch(step).to(torch.int32)

    def _padded(self, idx: torch.Tensor) -> torch.Tensor:
        """An explicit index list of up to B rows padded to the kernel batch (last row repeated)."""
        idx = idx.to(self.device, torch.int32).reshape(-1)
        if idx.numel() == self.B:
            return idx.contiguous()
        assert 1 <= idx.numel() <= self.B, idx.numel()
        return torch.cat([idx, idx[-1:].expand(self.B - idx.numel())]).contiguous()

    # --- state ----------------------------------------------------------------------------------
    def set_step(self, step: int):
        self.step_t.fill_(int(step))
        self.step_sgd.fill_(int(step))
        self.host_step = int(step)

    def read_stats(self, step: int) -> Dict[str, float]:
        """Stats published by the SGD kernel for the step that produced global_step == ``step``."""
        row = self.stats[(step - 1) % self.stats.shape[0]].tolist()
        return {"global_step": int(row[0]), "loss": row[1], "accuracy": row[2], "lr": row[3]}

    def global_step(self) -> int:
        return int(self.step_t.item())

    def flat_params(self) -> torch.Tensor:
        return self.master.detach().cpu()

    def _sched(self, scale: float = 1.0) -> list:
        """{lr0, decay, decay_steps, staircase, warmup, grad_scale} of the SGD ops and the fc chain."""
        return [self.lr0, self.decay, self.decay_steps, 1.0 if self.staircase else 0.0, self.warmup, scale]

    # --- communication --------------------------------------------------------------------------
    def _pg_backend(self) -> str:
        import torch.distributed as dist
        return dist.get_backend(self.pg) if dist.is_available() and dist.is_initialized() else "none"

    def _allreduce(self, t: torch.Tensor):
        """RCCL all-reduce of ``t`` on the wire's dtype."""
        import torch.distributed as dist
        if t.dtype != torch.bfloat16 and self.comm_dtype == "bf16":
            tb = t.to(torch.bfloat16)
            dist.all_reduce(tb, group=self.pg)
            t.copy_(tb)
        else:                                    # fp32 wire, or grad16: already on the wire's dtype
            dist.all_reduce(t, group=self.pg)

    def queue_error_copy(self):
        """Enqueue a host copy of the device error word for ``check_barriers(cached=True)``; an engine
        without bounded in-launch waits has none."""

    def check_barriers(self, cached: bool = False):
        """Raise if a bounded in-launch wait timed out; an engine without such waits never does."""

    def check_comm(self):
        """Raise if the xGMI all-reduce saw a peer stop participating (sticky device error word) or an
        in-launch wait timed out (device read: callers that must not sync use
        ``check_barriers(cached=True)``)."""
        self.check_barriers()
        if self.xgmi is not None:
            self.xgmi.check()

    # --- graph capture and replay ---------------------------------------------------------------
    @property
    def single_graph(self) -> bool:
        """The whole step (collectives included) is one capturable launch sequence."""
        return not self.dp or self.capture_comm or self.xgmi is not None

    def _reset_step_state(self):
        """Forget a half-issued step before a capture (an engine with state between launches)."""

    def _join_comm(self):
        """The current stream waits for work a step left on another stream (an engine that leaves any)."""

    def _steps_joined(self, k: int):
        """``k`` steps, then the other streams joined (a captured graph must end on its origin stream)."""
        for _ in range(k):
            self._eager_step()
        self._join_comm()

    def _capture_one(self, fn, pool):
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream(device=self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            # thread_local: the capture forbids unsafe calls on THIS thread only -- the process group's
            # watchdog thread polls the events of earlier (eager) collectives, and under the default
            # global mode one such poll invalidates the capture (seen on a 1-rank nccl group)
            with torch.cuda.graph(g, pool=pool, stream=s, capture_error_mode="thread_local"):
                fn()
        torch.cuda.current_stream(self.device).wait_stream(s)
        return g

    def capture(self, steps_per_graph: int = 8):
        """Capture the step into HIP graph(s).  N=1, N>1 over xGMI and N>1 over RCCL with
        ``capture_comm`` (the default): the whole step -- compute, all-reduce, SGD, on one or two
        streams -- is one graph, and further graphs chain 2, 4, ... ``steps_per_graph`` complete
        steps (every step reads its batch and LR through the device step counter, so consecutive
        steps need no host work, across epoch boundaries too).  :meth:`run` replays any step count
        as a sum of chains -- no single-step tails, no host gap between the chained steps.
        RCCL without ``capture_comm``: the graphs of ``_segments`` around eager collectives (no chains)."""
        quiesce_for_capture(self.device, self.pg if self.dp else None)
        self._reset_step_state()
        self.graphs, self.chains = [], {}
        self._pool = pool = torch.cuda.graph_pool_handle()
        # a capture records launches without running them: the step counter and weights are
        # identical before and after
        for fn in [lambda: self._steps_joined(1)] if self.single_graph else self._segments():
            self.graphs.append(self._capture_one(fn, pool))
        if self.single_graph:
            self.chains[1] = self.graphs[0]
            k = 2
            while k <= int(steps_per_graph):
                self.chains[k] = self._capture_one(lambda k=k: self._steps_joined(k), pool)
                k *= 2
        torch.cuda.synchronize(self.device)

    def run(self, n: int):
        """``n`` complete training steps (asynchronous): the longest captured chains first, then the
        binary decomposition of the remainder (e.g. 21 = 8 + 8 + 4 + 1 replays)."""
        n = int(n)
        chains = {k: g for k, g in self.chains.items() if g is not None}
        if not self.graphs or not chains:
            for _ in range(n):
                self.step()
            return
        self._join_comm()
        for k in sorted(chains, reverse=True):
            while n >= k:
                chains[k].replay()
                self.host_step += k
                n -= k

    def step(self):
        """One training step (asynchronous: returns once launched)."""
        if not self.graphs:
            self._eager_step()
        elif len(self.graphs) == 1:
            self._join_comm()
            self.graphs[0].replay()
        else:
            self._replay_segments()
        self.host_step += 1
