"""Fused MI355X training engine for ResNet-20 (BASELINE.json config 4; model: models/resnet.py).

Not in the reference (/root/reference/cifar10cnn.py only has the 2-conv CNN); SURVEY.md §2.C lists
ResNet-20 as the "extra kernels" configuration: conv3x3 stride 1/2, train-mode BatchNorm, residual
add, global average pool.  One step is 19 forward convs + 1 head + 18 dgrads + 19 wgrads + 1 SGD,
all HIP kernels of csrc/kernels/resnet.hip, captured as one HIP graph:

  fwd  l=0..18   z_l = conv_l(a_{l-1}); the prologue of conv_l applies BN_{l-1} (+ReLU, + option-A
                 shortcut) from the fp64 batch statistics conv_{l-1}'s epilogue accumulated, and
                 materialises a_{l-1} for the backward.  Conv_0 gathers the uint8 batch itself.
  head           BN_18 + residual + ReLU + global average pool + fc + softmax-xent + its backward
  bwd  l=18..1   dgrad_l: g_z_l (BN backward, prologue) -> g_a_{l-1} (+ shortcut grad) -> ReLU mask
                 -> g_y_{l-1} and the BN_{l-1} reductions (epilogue)
       l=18..0   wgrad_l, split-K fp32 slabs: in the same launch as dgrad_l (block roles), or on a
                 side stream (a second graph branch, wgrad_branch=True)
  sgd            slab reduction + SGD (conv, BN gamma/beta, fc) + BN running statistics (momentum 0.1)
                 + bf16 weight shadows + global_step++ + stats ring; with ``momentum`` /
                 ``weight_decay`` the same kernel keeps the velocity and adds the L2 term

Batch statistics are per rank (as in the eager model under DP).  With data parallelism the SGD runs
in two halves around ONE all-reduce of the 1.1 MB flat gradient (mode 1 -> RCCL -> mode 2).

Which path a configuration takes and which layer reads which shortcut is decided by the pure function
engine/plan_resnet.py plan_resnet_step; the constructor keeps the result as ``self.plan`` and
allocates from it, and the per-layer launchers (_fwd, _dgrad, _bwd, _wgrad) read their wiring there.
What this engine shares with the CNN engine (process fields, data order, graphs) is engine/base.py.
"""
from __future__ import annotations

import math
from typing import List, Optional

import torch

from .. import config as C
from ..models import resnet as R
from .base import FusedEngineBase
from .plan_resnet import (LAYERS, NL, _block_sc_mode, _kp, _kpd, _pick_groups, layer_table,  # noqa: F401
                          plan_resnet_step)

NSLOT = 8            # BN statistics slots per layer (resnet.hip)
FX_ONE = float(2 ** 48)   # fraction unit of the fixed-point BN statistics (resnet.hip fx_add)


def fx_encode(x: torch.Tensor):
    """Host mirror of resnet.hip fx_add for finite |x| < 2^50: (integer part, 48-bit fraction)."""
    x = x.double()
    f = torch.floor(x)
    return f.long(), torch.round((x - f) * FX_ONE).long()


def fx_decode(slots: torch.Tensor) -> torch.Tensor:
    """Totals of fixed-point statistic slots [..., NSLOT, 256] int64 -> fp64 [..., 128] (resnet.hip
    fx_total; a slot at or beyond the poison bound 2^55 decodes to NaN)."""
    hi, lo = slots[..., :128], slots[..., 128:]
    bad = (hi.abs() >= 2 ** 55).any(-2)
    tot = hi.sum(-2).double() + lo.sum(-2).double() / FX_ONE
    return torch.where(bad, torch.full_like(tot, float("nan")), tot)


class FusedResNetEngine(FusedEngineBase):
    """Owns every device buffer of the fused ResNet-20 step.  Parameters: one flat fp32 buffer in the
    TF layout of models/resnet.py (HWIO kernels), BN moving statistics in a second flat buffer."""

    _pick_groups = staticmethod(_pick_groups)

    def __init__(self, batch_size: int, data: torch.Tensor, labels: torch.Tensor, *, device=None,
                 flat_params: Optional[torch.Tensor] = None, state: Optional[torch.Tensor] = None,
                 lr: float = C.LEARNING_RATE, lr_decay: float = C.LR_DECAY,
                 decay_steps: float = C.NUM_GENS_TO_WAIT, staircase: bool = True, world_size: int = 1,
                 rank: int = 0, process_group=None, seed: int = 0, groups: Optional[List[int]] = None,
                 stats_len: int = 4096, comm_dtype: str = "fp32", wgrad_branch: Optional[bool] = None,
                 allreduce: str = "auto", capture_comm: Optional[bool] = None, dp_force: bool = False,
                 warmup_steps: int = 0,
                 merged_bwd: Optional[bool] = None, bwd_img_level: int = 1, sgd_split: bool = False,
                 momentum: float = 0.0, weight_decay: float = 0.0, velocity: Optional[torch.Tensor] = None):
        if not 0.0 <= momentum < 1.0 or weight_decay < 0.0:
            raise ValueError("momentum must be in [0, 1) and weight_decay >= 0")
        # every path decision and the layer wiring (engine/plan_resnet.py), then as plain attributes
        self.plan = plan = plan_resnet_step(batch_size=batch_size, world_size=world_size, dp_force=dp_force,
                                            groups=groups, wgrad_branch=wgrad_branch, merged_bwd=merged_bwd,
                                            bwd_img_level=bwd_img_level, sgd_split=sgd_split)
        super().__init__(device=device, world_size=world_size, rank=rank, process_group=process_group, seed=seed,
                         comm_dtype=comm_dtype, lr=lr, lr_decay=lr_decay, decay_steps=decay_steps,
                         staircase=staircase, warmup_steps=warmup_steps, dp_force=dp_force,
                         capture_comm=capture_comm, stats_len=stats_len)
        dev, B = self.device, plan.B
        self._init_batch(data, labels, B, plan.Bv)
        self.bwd_img_level, self.groups = int(bwd_img_level), list(plan.groups)
        self.wgrad_branch, self.merged_bwd, self.sgd_split = plan.wgrad_branch, plan.merged_bwd, plan.sgd_split
        self._sgd_points = plan.sgd_points

        f0, s0 = R.init_flat_params(torch.Generator().manual_seed(seed))
        if flat_params is not None:
            f0 = flat_params
        if state is not None:
            s0 = state
        self.master = f0.to(dev, torch.float32).contiguous().clone()
        self.state = s0.to(dev, torch.float32).contiguous().clone()
        # SGD momentum / L2 weight decay, applied by the SGD kernel (v <- momentum * v + (g + wd_eff * w),
        # w <- w - lr * v; wd_eff = weight_decay on the conv kernels and the fc weights only).  The
        # velocity lives in the layout of master; a static buffer, so graphs and chains capture it, and
        # under data parallelism every replica applies the same reduced gradient to the same velocity
        self.momentum, self.weight_decay = float(momentum), float(weight_decay)
        self.vel = torch.zeros_like(self.master) if self.momentum else None
        if velocity is not None and self.vel is not None:
            self.vel.copy_(velocity.to(dev, torch.float32))
        # one all-reduce of the whole flat gradient per step
        self._select_xgmi(self.master.numel(), [(0, self.master.numel())], allreduce)
        self.grad = self._flat_grad(self.master, always=False)
        P = {s.name[len(R.SCOPE) + 1:]: s for s in R.PARAM_SPECS}
        S = {s.name[len(R.SCOPE) + 1:]: s for s in R.STATE_SPECS}
        view = lambda buf, s: buf[s.offset:s.offset + s.numel]
        self.conv_off = [P[f"{n}/conv/kernel"].offset for n, *_ in LAYERS]
        self.gamma_off = [P[f"{n}/bn/gamma"].offset for n, *_ in LAYERS]
        self.beta_off = [P[f"{n}/bn/beta"].offset for n, *_ in LAYERS]
        self.mm_off = [S[f"{n}/bn/moving_mean"].offset for n, *_ in LAYERS]
        self.mv_off = [S[f"{n}/bn/moving_variance"].offset for n, *_ in LAYERS]
        self.gamma = [view(self.master, P[f"{n}/bn/gamma"]) for n, *_ in LAYERS]
        self.beta = [view(self.master, P[f"{n}/bn/beta"]) for n, *_ in LAYERS]
        self.fcw_off, self.fcb_off = P["fc/weights"].offset, P["fc/biases"].offset
        self.fcw, self.fcb = view(self.master, P["fc/weights"]), view(self.master, P["fc/biases"])

        bf = torch.bfloat16
        z = lambda *s, dt=bf: torch.zeros(*s, dtype=dt, device=dev)
        self.wf = [z(co, _kp(ci)) for _, ci, co, _, _ in LAYERS]
        self.wd = [z(co, _kp(ci)) if l == 0 else z(ci, _kpd(co)) for l, (_, ci, co, _, _) in enumerate(LAYERS)]
        hout = [h // s for _, _, _, h, s in LAYERS]
        self.z = [z(B, ho, ho, co) for ho, (_, _, co, _, _) in zip(hout, LAYERS)]
        self.gy = [z(B, ho, ho, co) for ho, (_, _, co, _, _) in zip(hout, LAYERS)]
        self.a = [z(B, ho, ho, co) for ho, (_, _, co, _, _) in zip(hout[:-1], LAYERS[:-1])]   # a_0 .. a_17
        # [stat | red] BatchNorm sums, NSLOT fixed-point copies per layer (resnet.hip fx_add): per statistic
        # an int64 integer part [0, 128) and a 48-bit fraction [128, 256), added with 64-bit integer
        # atomics -- order independent, so every step is bitwise reproducible (graph replay == eager);
        # zeroed at the start of each forward
        self.acc = torch.zeros(2, NL, NSLOT, 256, dtype=torch.int64, device=dev)
        self.stat, self.red = self.acc[0], self.acc[1]
        self.part = [z(g, _kp(ci), co, dt=torch.float32) for g, (_, ci, co, _, _) in zip(self.groups, LAYERS)]
        self.fc_part = z(B, 656, dt=torch.float32)
        self.loss_img = z(B, dt=torch.float32)
        self.correct_img = z(B, dt=torch.int32)
        # (The SGD finds the last arriver with the ticket; the CNN engine's ticketless form -- the head
        # copies the step counter for the SGD -- measured no better here in r3: 0.679 / 0.682 ms vs
        # 0.675 / 0.678 with the ticket; step_sgd is the kernel argument that form would use)
        if self.dp:
            self.comm_info.update(captured_comm=bool(self.capture_comm or self.xgmi is not None))
        self.side_stream = torch.cuda.Stream(device=dev)
        self._stem_src = None          # explicit (idx, counter, period) of the stem wgrad, else generated
        self.refresh_shadows()

    # ------------------------------------------------------------------------------------------
    def refresh_shadows(self):
        self._sgd(mode=3)

    def bn_sums(self) -> torch.Tensor:
        """Decoded BatchNorm sums of the last step, fp64 [2, NL, 128]: [0] sum z / sum z^2, [1] R1 / R2
        (channels at [0, cout) and [64, 64 + cout))."""
        return fx_decode(self.acc)

    def _padded(self, idx: torch.Tensor) -> torch.Tensor:
        """An explicit list of exactly Bv dataset rows, padded to the kernel batch."""
        assert idx.numel() == self.Bv, (idx.numel(), self.Bv)
        return super()._padded(idx)

    # --- kernels: one launcher per layer, wired by the plan --------------------------------------
    def _fwd(self, l, src):
        """conv_l with the BN-apply (+ shortcut) prologue of layer l - 1; ``src``: the batch's
        (idx, counter, period), which only the stem reads."""
        _, ci, co, h, s = LAYERS[l]
        if l == 0:
            idx, counter, period = src
            self.ops.rn_fwd(ci, co, h, s, self.data, idx, counter, period, 0, 0, None, None, None, None, None, 0,
                            None, self.wf[0], self.z[0], self.stat[0], self.Bv)
            return
        p = l - 1
        sc_mode, sc = self.plan.fwd_sc[l]
        self.ops.rn_fwd(ci, co, h, s, None, None, None, 1, 0, 0, self.z[p], self.stat[p], self.gamma[p],
                        self.beta[p], None if sc is None else self.a[sc], sc_mode, self.a[p], self.wf[l], self.z[l],
                        self.stat[l], self.Bv)

    def _dgrad_args(self, l):
        _, ci, co, h, s = LAYERS[l]
        p = l - 1
        sc_mode = self.plan.bwd_sc[l]
        return (ci, co, h, s, self.gy[l], self.z[l], self.stat[l], self.red[l], self.gamma[l], self.wd[l], self.a[p],
                self.z[p], self.stat[p], self.gy[l + 1] if sc_mode else None, sc_mode, self.gy[p], self.red[p])

    def _dgrad(self, l):
        self.ops.rn_dgrad(*self._dgrad_args(l), self.Bv)

    def _bwd(self, l):
        """dgrad_l and wgrad_l in one launch: both only read what dgrad_{l+1} produced."""
        self.ops.rn_bwd(*self._dgrad_args(l), self.part[l], self.Bv, self.plan.per_image[l])

    def _per_image(self, l) -> bool:
        """Layer l's merged launch runs one workgroup per image (k_rn_bwd_img; plan_resnet.py)."""
        return self.plan.per_image[l]

    def _wgrad(self, l):
        _, ci, co, h, s = LAYERS[l]
        if l == 0:
            idx, counter, period = self._stem_src or (self.order_desc, self.step_t, self.period)
            self.ops.rn_wgrad(ci, co, h, s, self.data, idx, counter, period, 0, 0, None, self.gy[0],
                              self.z[0], self.stat[0], self.red[0], self.gamma[0], self.part[0], self.Bv)
        else:
            self.ops.rn_wgrad(ci, co, h, s, None, None, None, 1, 0, 0, self.a[l - 1], self.gy[l], self.z[l],
                              self.stat[l], self.red[l], self.gamma[l], self.part[l], self.Bv)

    def _forward(self, idx, counter, period, logits_out=None):
        self.acc.zero_()
        for l in range(NL):
            self._fwd(l, (idx, counter, period))
        self.ops.rn_head(self.z[18], self.stat[18], self.gamma[18], self.beta[18], self.a[16], self.fcw, self.fcb,
                         self.labels, idx, counter, period, 1.0 / (self.Bv * self.world_size), self.gy[18],
                         self.red[18], self.fc_part, self.loss_img, self.correct_img, logits_out, self.Bv,
                         self.step_t, self.step_sgd)

    def _backward(self):
        main = torch.cuda.current_stream(self.device)
        side = self.side_stream if self.wgrad_branch else main
        if side is main and self.merged_bwd:
            for l in range(NL - 1, 0, -1):
                self._bwd(l)
                if self.sgd_split and l in self._sgd_points:
                    # layers >= l: slabs complete, weights no longer read this step
                    self.side_stream.wait_stream(main)
                    with torch.cuda.stream(self.side_stream):
                        self._sgd(mode=0, layers=self._sgd_points[l], tail=False)
            self._wgrad(0)
            return
        for l in range(NL - 1, -1, -1):
            # gy_l and red_l are complete here (head or dgrad_{l+1}): fork wgrad_l onto the side branch
            if side is not main:
                ev = torch.cuda.Event()
                ev.record(main)
                side.wait_event(ev)
            with torch.cuda.stream(side):
                self._wgrad(l)
            if l > 0:
                self._dgrad(l)
        if side is not main:
            main.wait_stream(side)

    def _sgd(self, mode: int, scale: float = 1.0, layers=(0, NL), tail: bool = True):
        self.ops.rn_sgd(self.master, self.grad, scale, self.state, self.conv_off, self.gamma_off, self.beta_off,
                        self.mm_off, self.mv_off, self.fcw_off, self.fcb_off, self.part, self.wf, self.wd, self.stat,
                        self.red, self.fc_part, self.loss_img, self.correct_img, self.step_t, self.ticket, self.stats,
                        mode, self.lr0, self.decay, self.decay_steps, self.staircase, R.BN_MOMENTUM, self.warmup,
                        layers[0], layers[1], tail, self.Bv,
                        None, self.vel, self.momentum, self.weight_decay)

    def _allreduce(self, t: torch.Tensor):
        if self.xgmi is not None:
            self.xgmi.all_reduce(0, t.numel())
        else:
            super()._allreduce(t)

    def _seg_compute(self):
        self._forward(self.order_desc, self.step_t, self.period)
        self._backward()
        if self.sgd_split:
            # the branch SGDs read the step counter the tail increments: join first
            torch.cuda.current_stream(self.device).wait_stream(self.side_stream)
            self._sgd(mode=0, layers=(0, min(lo for lo, _ in self._sgd_points.values())))
        else:
            self._sgd(mode=1 if self.dp else 0)

    def _seg_apply(self):
        self._sgd(mode=2, scale=1.0)

    def _eager_step(self):
        self._seg_compute()
        if self.dp:
            self._allreduce(self.grad)
            self._seg_apply()

    def _segments(self):
        """RCCL without ``capture_comm``: compute and apply graphs around an eager all-reduce."""
        return [self._seg_compute, self._seg_apply]

    def _replay_segments(self):
        self.graphs[0].replay()
        self._allreduce(self.grad)
        self.graphs[1].replay()

    def compute_gradients(self, idx: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Forward + backward + slab reduction only (no update); the flat gradient lands in ``grad``.
        ``idx``: explicit dataset rows (int32 [B]) instead of this step's generated batch."""
        if self.grad is None:
            self.grad = torch.zeros_like(self.master)
        if idx is not None:
            ids = self._padded(idx)
            self._stem_src = (ids, None, 1)
            try:
                self._forward(ids, None, 1)
                self._backward()
                self._sgd(mode=1)
            finally:
                self._stem_src = None
            return self.grad
        self._forward(self.order_desc, self.step_t, self.period)
        self._backward()
        self._sgd(mode=1)
        return self.grad

    # --- evaluation -----------------------------------------------------------------------------
    def eval_model(self):
        m = R.ResNet20(flat=self.master.detach()).to(self.device)
        m.state.copy_(self.state)
        m.eval()
        return m

    @torch.no_grad()
    def evaluate(self, data: torch.Tensor, labels: torch.Tensor, max_batches: int = 0) -> float:
        """Test accuracy with the BN moving statistics (eval-mode forward of the same weights)."""
        m = self.eval_model()
        n = data.shape[0]
        nb = math.ceil(n / self.Bv)
        if max_batches:
            nb = min(nb, max_batches)
        correct = total = 0
        for i in range(nb):
            x = data[i * self.Bv:(i + 1) * self.Bv].to(self.device).float()
            y = labels[i * self.Bv:(i + 1) * self.Bv].to(self.device).long()
            correct += int((m(x).argmax(1) == y).sum())
            total += y.numel()
        return correct / max(1, total)

    @torch.no_grad()
    def forward_logits(self, idx: torch.Tensor) -> torch.Tensor:
        """Train-mode (batch statistics) logits of the Bv dataset rows ``idx`` via the fused kernels —
        for tests.  Writes activations / statistics but updates nothing."""
        self._forward(self._padded(idx), None, 1, logits_out=self.logits_buf)
        return self.logits_buf[:self.Bv].clone()

    # --- state ----------------------------------------------------------------------------------
    def velocity_params(self) -> Optional[torch.Tensor]:
        """The momentum velocity in the layout of :meth:`flat_params` (CPU copy); None without momentum."""
        return None if self.vel is None else self.vel.detach().cpu()

    def load_flat_params(self, flat: torch.Tensor, step: Optional[int] = None, state: Optional[torch.Tensor] = None,
                         velocity: Optional[torch.Tensor] = None):
        self.master.copy_(flat.to(self.device, torch.float32))
        if state is not None:
            self.state.copy_(state.to(self.device, torch.float32))
        if velocity is not None and self.vel is not None:
            self.vel.copy_(velocity.to(self.device, torch.float32))
        if step is not None:
            self.set_step(step)
        self.refresh_shadows()
