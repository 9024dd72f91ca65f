"""Fused MI355X training engine for the reference CNN (hand-written HIP kernels + HIP graphs + RCCL).

One training step (= one ``mon_sess.run([train_op, loss])`` of /root/reference/cifar10cnn.py:230,
SURVEY.md §3.3) is THREE kernel launches on the single-GPU bf16 path at 128 < B <= 256, all reading
their inputs from device memory:

  1 conv12_fwd   uint8 gather + center crop + conv1 + bias + ReLU + pool1 (+argmax), handed through
                 LDS to conv2 + bias + ReLU + pool2 (+argmax) -- one workgroup per image
  2 fc_chain     one persistent launch (cnn_fc.hip): fc1 forward (split-K tiles) -> MLP head (fc1
                 reduce / bias / ReLU, fc2, fc3, ReLU logits, softmax xent, accuracy, dlogits -> dh2 ->
                 dh1) -> dp2 = dh1 W1^T tiles + the fc weight-gradient tiles with the fc1 SGD in their
                 epilogue -> the conv2 input gradient of each workgroup's image (pool2/ReLU backward
                 gather + conv2 dgrad, conv2_core.h) once its dp2 row tile is published
  3 wgrad        pool1/ReLU backward + conv1 weight/bias gradients and conv2 weight/bias gradients
                 (split-K slabs), then -- on one GPU -- the whole rest of the SGD in the same launch
                 (sub-grid barrier per slab family, every block reduces its share in the SGD kernel's
                 order and applies the update + bf16 shadows; the stats, global_step and the next
                 step's batch rows too)

At B <= 128 launch 1 is k_conv12_fwd_split (cnn_split.hip: conv1 -> pool1 -> conv2 -> pool2 in ONE
launch with two workgroups per image that swap their pool1 channel halves through write-through
stores + a flag, so a small batch fills the 256 CUs) and the fc chain's 256 workgroups run the conv2
input gradient two per image (cnn_split.hip's channel halves): three launches as well.  B > 256 (and
ranks sharing one GPU) use the three-launch fc path (grouped fc1 GEMM, head, grouped backward GEMM).
The fp8 path (BASELINE config 5) runs conv1 and the fp8 conv2 forward as two launches, the fp8 conv2
dgrad as its own launch and the SGD as its own launch.

Data parallel (N > 1): the wgrad launch reduces the conv slabs into the flat gradient instead of
applying them, then the gradient is exchanged and applied -- serial schedule: one all-reduce of the
whole flat gradient (xGMI peer-to-peer kernel or RCCL) and one SGD launch; overlap schedule: the fc
bucket's all-reduce on a comm stream beside the wgrad launch, the conv bucket after it on the same
stream, the conv SGD on the main stream and the fc SGD on the comm stream beside the NEXT step's
forward (_dp_step).  bench.py times both before the timed region and keeps the
faster (tune_schedule).

Every data-consuming kernel computes its batch rows from the device-resident global_step and the
generated epoch order (data/order.py: a keyed Feistel permutation per epoch, no index buffer), so
the whole step is a static HIP graph and ``k`` consecutive steps -- across epoch boundaries -- are
one graph replay.  Any batch size works: the kernels run on the batch padded to the 16-row tile and
the head gives padding rows zero loss weight (their gradients are exactly zero).

Variants: every default below is the measured-fastest path of its configuration; the alternatives
that stay are the bitwise references the tests compare against, selected with the ``variant``
dict of the constructor (VARIANT_DEFAULTS).  Which path a configuration takes is decided by the pure
function engine/plan.py plan_step; the constructor collects its inputs, keeps the result as
``self.plan`` and allocates from it.  Three environment switches turn a persistent,
co-residency-dependent launch off without code changes (a training run builds the engine without a
``variant``): DMLC_FC_FUSED=0 (the fc chain), DMLC_WGRAD_SGD=0 (the in-launch SGD / slab reduction of
the wgrad launch) and DMLC_FWD12_SPLIT=0 (the B <= 128 forward whose two workgroups per image wait on
each other).

Bindings: the launches that touch most of the engine's state (fc_chain, sgd, xgmi_allreduce_sgd,
wgrad_sgd and backward_fused, the whole backward as one call) take ``self.buf``, the device buffers
keyed by attribute name, plus the switches that differ from call to call; the binding checks every
buffer it reads by name and keeps no state between calls (csrc/bindings/torch_ops.cpp).
"""
from __future__ import annotations

import dataclasses
import math
import os
from typing import Optional

import torch

from .. import config as C
from ..parallel.dist import quiesce_for_capture
from ..models import cifar_cnn as M
from .base import FusedEngineBase
from .plan import (ERR_WORD, FC_SYNC_WORDS, HAND_WORDS, TICKET_WORDS, VARIANT_DEFAULTS, WBAR_WORDS,  # noqa: F401
                   head_rows, plan_step)

SEG_OFF = [s.offset for s in M.PARAM_SPECS]
# the engine attributes the dict-taking ops read by name (FusedCifarEngine.buf)
BUF_NAMES = ("master", "grad", "grad16", "part1", "partb1", "part2", "partb2", "w1f", "w2f", "w2d", "fc1n", "fc2t",
             "fc2n", "fc3t", "fc3d", "step_t", "step_sgd", "ticket", "loss_part", "correct_part", "stats", "bidx",
             "xraw", "data", "labels", "p1", "p2", "am1", "am2", "dp1", "dp2", "dy2", "h1part8", "h1", "h2", "dl",
             "dh1", "dh2", "fc_sync", "wbar", "bwd_hand", "w2f8", "amax_w", "scale_w", "p1f8", "dy2f8", "sx8",
             "sy_img", "aug")
SEG = {M.short(s.name): s for s in M.PARAM_SPECS}


def _gemm_params(M_, N_, K_, lda, a_kmajor, ldb, b_kmajor, ldc, c_mode, ksplit=1, relu=0, nvalid=None, b_par=0,
                 s_par=0):
    return [M_, N_, K_, lda, a_kmajor, ldb, b_kmajor, ldc, c_mode, ksplit, relu, N_ if nvalid is None else nvalid,
            b_par, s_par]


FC1_NUMEL = 2304 * 384


class FusedCifarEngine(FusedEngineBase):
    """Owns every device buffer of the fused step.  Not an nn.Module: parameters live in one flat
    fp32 buffer (``self.master``) in the TF checkpoint layout; see models/cifar_cnn.py."""

    def __init__(self, batch_size: int, data: torch.Tensor, labels: torch.Tensor, *, device=None,
                 flat_params: Optional[torch.Tensor] = None, lr: float = C.LEARNING_RATE,
                 lr_decay: float = C.LR_DECAY, decay_steps: float = C.NUM_GENS_TO_WAIT, staircase: bool = True,
                 relu_logits: bool = True, crop_offset=(4, 4), world_size: int = 1, rank: int = 0,
                 process_group=None, seed: int = 0, fc1_split: Optional[int] = None, g1: Optional[int] = None,
                 g2: Optional[int] = None, stats_len: int = 4096, comm_dtype: str = "fp32",
                 capture_comm: Optional[bool] = None, dtype: str = "bf16", allreduce: str = "auto",
                 dp_schedule: str = "serial", dp_force: bool = False, warmup_steps: int = 0,
                 conv_split: Optional[int] = None, conv1_split: Optional[int] = None,
                 dgrad_split: Optional[int] = None, variant: Optional[dict] = None, augment: bool = False):
        super().__init__(device=device, world_size=world_size, rank=rank, process_group=process_group, seed=seed,
                         comm_dtype=comm_dtype, lr=lr, lr_decay=lr_decay, decay_steps=decay_steps,
                         staircase=staircase, warmup_steps=warmup_steps, dp_force=dp_force,
                         capture_comm=capture_comm, stats_len=stats_len)
        dev = self.device
        self.relu_logits = relu_logits
        self.cy, self.cx = crop_offset
        # per-image random crop + flip of the training batches (api.h DmlcConv1FwdArgs::aug); the
        # evaluation forwards keep the constructor's crop
        self.augment = bool(augment)
        if self.augment and tuple(crop_offset) != (4, 4):
            raise ValueError("augment needs the 24x24 crop: crop_offset must be (4, 4)")
        self.dtype = dtype

        # --- the planner's inputs: everything read from the process, the device and the fabric -------
        on_gpu = dev.type == "cuda"
        cus = torch.cuda.get_device_properties(dev).multi_processor_count if on_gpu else 0
        ndev = torch.cuda.device_count() if on_gpu else 0
        local_world = int(os.environ.get("LOCAL_WORLD_SIZE", world_size))
        if flat_params is None:
            flat_params = M.init_flat_params(torch.Generator().manual_seed(seed))
        n_flat = flat_params.numel()
        self._buckets = {True: (M.FC_BUCKET_OFFSET, n_flat - M.FC_BUCKET_OFFSET), False: (0, M.FC_BUCKET_OFFSET)}
        # the call pattern the step will issue: one whole-buffer all-reduce (serial) or the fc bucket
        # then the conv bucket (overlap)
        self._select_xgmi(n_flat, [(0, n_flat)] if dp_schedule == "serial"
                          else [self._buckets[True], self._buckets[False]], allreduce)
        if dp_force and world_size == 1 and allreduce == "xgmi" and on_gpu:
            # a one-rank xGMI context (no peers): the DP step's exchange kernel on a single GPU
            from ..parallel import xgmi as X
            self.xgmi = X.XgmiAllReduce(n_flat, 0, 1, None, wire=comm_dtype)
            self.comm_info = {"allreduce": "xgmi", "wire": comm_dtype}
        self.plan_inputs = dict(batch_size=batch_size, dtype=dtype, world_size=world_size, dp_force=dp_force,
                                local_world=local_world, ndev=ndev, cus=cus, have_xgmi=self.xgmi is not None,
                                comm_dtype=comm_dtype, conv_split=conv_split, conv1_split=conv1_split,
                                dgrad_split=dgrad_split, g1=g1, g2=g2, fc1_split=fc1_split, variant=variant)

        # --- every path decision (engine/plan.py), then as plain attributes: tests flip some ----------
        self.plan = plan_step(**self.plan_inputs)
        for f in dataclasses.fields(self.plan):
            setattr(self, f.name, getattr(self.plan, f.name))
        B = self.B
        self.keep_dp1 = False          # tests: also write the pool1 gradient to global memory

        # --- data (device resident) ---------------------------------------------------------
        self._init_batch(data, labels, B, self.Bv)
        # this step's batch rows (int32 [B], rows >= Bv repeat the last): written for step s+1 by the
        # finalizing SGD launch of step s (cnn_sgd.hip), so each data kernel reads one index per row;
        # set from the host whenever the step counter is set from the host
        self.bidx = torch.zeros(B, dtype=torch.int32, device=dev)
        # raw uint8 images of the step's rows, written by the forward for the conv1 weight gradient
        self.xraw = torch.zeros(B, 3072, dtype=torch.uint8, device=dev)
        # this step's augmentation words by batch row (int32 [B]), kept like bidx: the finalizer of
        # step s writes those of step s+1, the host writes them whenever it sets the step
        self.aug = torch.zeros(B, dtype=torch.int32, device=dev) if self.augment else None

        # --- parameters + shadows -------------------------------------------------------------
        self.master = flat_params.to(dev, torch.float32).contiguous().clone()
        self.grad = self._flat_grad(self.master, always=True)
        bf = torch.bfloat16
        z = lambda *s, dt=bf: torch.zeros(*s, dtype=dt, device=dev)
        self.w1f, self.w2f, self.w2d = z(64, 96), z(64, 1600), z(64, 1600)
        # fc1's bf16 shadow is double-buffered by step parity ([2][2304][384]): the kernels of step s
        # read fc1n[s & 1] and the update writes fc1n[(s + 1) & 1], so at N=1 the dW1 GEMM can apply
        # the fc1 update in its epilogue while the dp2 problem of the same launch still reads the
        # current weights (fc1_epilogue)
        self.fc1n, self.fc2t, self.fc2n = z(2, 2304, 384), z(192, 384), z(384, 192)
        self.fc3t, self.fc3d = z(16, 192), z(192, 32)
        if self.fp8:         # e4m3 conv2 weight shadows ([0] forward, [1] the dgrad's) + their scales
            self.w2f8 = z(2, 64, 1600, dt=torch.uint8)
            self.amax_x = z(B, dt=torch.float32)      # per-image activation maxima (conv1 -> conv2)
            self.amax_w = z(2, 400, dt=torch.float32)  # [slot][SGD conv2-row block] weight maxima
            self.scale_w = z(2, dt=torch.float32)
        if self.fp8_wgrad:   # the e4m3 X / dY2 of the fp8 conv2 weight gradient and their scales
            self.p1f8, self.dy2f8 = z(B, 144, 64, dt=torch.uint8), z(B, 144, 64, dt=torch.uint8)
            self.sx8, self.sy_img = z(1, dt=torch.float32), torch.ones(B, dtype=torch.float32, device=dev)
        self._w8 = dict(fp8=[self.p1f8, self.dy2f8, self.sx8, self.sy_img]) if self.fp8_wgrad else {}

        # --- activations / workspaces -------------------------------------------------------
        self.p1, self.am1 = z(B, 12, 12, 64), z(B, 12, 12, 64, dt=torch.uint8)
        self.p2, self.am2 = z(B, 6, 6, 64), z(B, 6, 6, 64, dt=torch.uint8)
        self.h1part = z(self.fc1_split, B, 384, dt=torch.float32)
        self.h1, self.h2, self.dl = z(B, 384), z(B, 192), z(B, 16)
        self.dh1, self.dh2 = z(B, 384), z(B, 192)
        self.dp2 = z(B, 6, 6, 64)
        self.dp1, self.dy2 = z(B, 12, 12, 64), z(B, 144, 64)
        # conv weight-gradient slabs: fp32 partial sums over 1/g of the batch each, summed in fixed
        # order.  (bf16 conv2 slabs measured 1.3 us/step faster in r3 but added a 4e-4 relative error
        # to the conv2 weight gradient and a 7 % drift in the loss-curve parity test: not kept.)
        self.part2, self.partb2 = z(self.g2, 1600, 64, dt=torch.float32), z(self.g2, 64, dt=torch.float32)
        self.part1, self.partb1 = z(self.g1, 80, 64, dt=torch.float32), z(self.g1, 64, dt=torch.float32)
        self.h1part8 = z(8, B, 384, dt=torch.float32) if self.has_h1part8 else None
        self.fc_sync = torch.zeros(FC_SYNC_WORDS, dtype=torch.int32, device=dev)
        self._fc_src = None
        self.loss_part = z(self.loss_parts, dt=torch.float32)
        self.correct_part = z(self.loss_parts, dt=torch.int32)
        # (step_sgd: the head kernel copies the step counter there; the SGD, launch or in-launch, reads
        # the copy, so one of its workgroups can bump step_t without an arrival ticket, cnn_sgd.hip)

        p = {k: self.master[s.offset:s.offset + s.numel] for k, s in SEG.items()}
        self.pv = p
        gv = {k: self.grad[s.offset:s.offset + s.numel] for k, s in SEG.items()}
        self.gv = gv
        # the bf16 flat gradient of the RCCL bf16 wire (has_grad16)
        self.grad16 = (torch.zeros(self.master.numel(), dtype=torch.bfloat16, device=dev) if self.has_grad16
                       else None)

        # grouped GEMM problem lists (the three-launch fc path)
        self._fc1_fwd = dict(A=[self.p2.view(B, 2304)], B=[self.fc1n], C=[self.h1part], bias=[None],
                             params=_gemm_params(B, 384, 2304, 2304, 1, 384, 0, 384, 2, self.fc1_split,
                                                 b_par=FC1_NUMEL))
        self._fc_bwd = dict(
            A=[self.dh1, self.p2.view(B, 2304), self.h1, self.h2, self.dh1, self.dh2, self.dl],
            B=[self.fc1n, self.dh1, self.dh2, self.dl, self.dh1, self.dh2, self.dl],
            C=[self.dp2.view(B, 2304), gv["full_weight_1"], gv["full_weight_2"], gv["full_weight_3"],
               gv["full_bias_1"], gv["full_bias_2"], gv["full_bias_3"]],
            bias=[None] * 7,
            params=(_gemm_params(B, 2304, 384, 384, 1, 384, 1, 2304, 1, b_par=FC1_NUMEL)  # dp2 = dh1 W1^T
                    + _gemm_params(2304, 384, B, 2304, 0, 384, 0, 384, 0)          # dW1 = p2^T dh1
                    + _gemm_params(384, 192, B, 384, 0, 192, 0, 192, 0)            # dW2 = h1^T dh2
                    + _gemm_params(192, 16, B, 192, 0, 16, 0, 10, 0, nvalid=10)    # dW3 = h2^T dl
                    + _gemm_params(384, 8, B, 384, 0, 8, 0, 1, 3, nvalid=384)      # db1
                    + _gemm_params(192, 8, B, 192, 0, 8, 0, 1, 3, nvalid=192)      # db2
                    + _gemm_params(16, 8, B, 16, 0, 8, 0, 1, 3, nvalid=10)))       # db3
        fb = self._fc_bwd
        # single GPU (fc1_epilogue): the same launch with dW1 as a fused SGD epilogue (c_mode 4)
        self._fc_bwd_sgd = dict(fb, C=[fb["C"][0], p["full_weight_1"]] + fb["C"][2:],
                                params=fb["params"][:14] + _gemm_params(2304, 384, B, 2304, 0, 384, 0, 384, 4,
                                                                        s_par=FC1_NUMEL)
                                + fb["params"][28:])
        self.c12_flags = torch.zeros(self.c12_flags_words, dtype=torch.int32, device=dev)
        self.wbar = torch.zeros(WBAR_WORDS, dtype=torch.int32, device=dev)   # barrier words + error word
        # pinned host copy of the barrier error word, refreshed by queue_error_copy() behind each
        # chunk of steps (the trainer checks it at every progress point without a device sync)
        self._err_host = (torch.zeros(1, dtype=torch.int32).pin_memory() if on_gpu
                          else torch.zeros(1, dtype=torch.int32))
        self._dgrad_done = False
        self.bwd_hand = torch.zeros(self.bwd_hand_words, dtype=torch.int32, device=dev)

        self.comm_stream = torch.cuda.Stream(device=dev) if self.dp else None
        # N>1 step schedule: "overlap" = two buckets, fc all-reduce + fc SGD on the comm stream under
        # the conv backward; "serial" = one stream, one all-reduce of the whole flat gradient, one SGD
        # launch (no fork/join, no co-resident comm/SGD blocks slowing the conv kernels).
        # tune_schedule() measures both and keeps the faster.
        assert dp_schedule in ("overlap", "serial"), dp_schedule
        self.dp_schedule = dp_schedule
        self._captured_schedule = None
        if self.dp:
            self.comm_info.update(schedule=dp_schedule, backend=self._backend(),
                                  captured_comm=bool(self.capture_comm or self.xgmi is not None),
                                  grad_dtype="bf16" if self.grad16 is not None else "fp32")
        # the device buffers by attribute name, for the ops that take them as one dict (csrc/bindings/
        # torch_ops.cpp: fc_chain, sgd, xgmi_allreduce_sgd, wgrad_sgd, backward_fused); a buffer this
        # configuration does not have is an absent key.  Nothing rebinds these attributes afterwards
        # (evaluate() swaps data / labels only around eval forwards, which take them as arguments).
        self.buf = {k: t for k in BUF_NAMES if (t := getattr(self, k, None)) is not None}
        self._sync_bidx()
        self.refresh_shadows()

    # ------------------------------------------------------------------------------------------
    def refresh_shadows(self):
        if self.fp8:    # exact amax of the current W2 for the shadow quantisation at this step
            s = self.host_step & 1
            w2 = self.master[SEG["conv2_kernel"].offset:SEG["conv2_kernel"].offset + SEG["conv2_kernel"].numel]
            self.amax_w[s] = w2.abs().max()
            self.amax_w[s ^ 1] = 0.0
        self._sgd(mode=3)

    def set_step(self, step: int):
        old = int(self.step_t.item())
        if (old ^ int(step)) & 1:      # the current fc1 shadow moves to the new step's parity slot
            self.fc1n[int(step) & 1].copy_(self.fc1n[old & 1])
        super().set_step(step)
        self._sync_bidx()

    def _sync_bidx(self):
        self.bidx.copy_(self._padded(self.batch_indices(self.host_step)))
        if self.aug is not None:
            self.aug.copy_(self.order.augment(self.host_step, pad_to=self.B))
        self._sync_xraw()

    def _sync_xraw(self):
        """The current step's raw images into xraw (the prefetching forward reads them there)."""
        if getattr(self, "xraw_prefetch", False):
            self.xraw.copy_(self.data.index_select(0, self.bidx.long()).view(self.B, 3072))

    # --- kernels ------------------------------------------------------------------------------
    def _forward(self, idx, counter, period, train=True, logits_out=None):
        o, p = self.ops, self.pv
        aug = dict(aug=self.aug) if train and self.aug is not None else {}
        if self.fwd12_split:                       # one launch, two workgroups per image (cnn_split.hip)
            o.conv12_fwd(self.data, idx, counter, period, self.cy, self.cx, self.w1f, p["conv1_bias"], self.p1,
                         self.am1, self.w2f, p["conv2_bias"], self.p2, self.am2, self.xraw if train else None, False,
                         self.c12_flags, self.wbar[ERR_WORD:ERR_WORD + 1], **aug)
        elif self.conv_split == 2 and not self.fp8:  # channel-split: B * nsplit workgroups per conv
            o.conv1_fwd_split(self.data, idx, counter, period, self.cy, self.cx, self.w1f, p["conv1_bias"], self.p1,
                              self.am1, self.xraw if train else None, self.conv1_split, **aug)
            o.conv2_fwd_split(self.p1, self.w2f, p["conv2_bias"], self.p2, self.am2)
        elif self.fused_fwd and not self.fp8:      # conv1 + pool1 + conv2 + pool2 in one launch
            pre = train and self.xraw_prefetch and idx is self.bidx   # the step's own (prefetched) batch
            o.conv12_fwd(self.data, idx, counter, period, self.cy, self.cx, self.w1f, p["conv1_bias"], self.p1,
                         self.am1, self.w2f, p["conv2_bias"], self.p2, self.am2, self.xraw if train else None, pre,
                         **aug)
        else:
            o.conv1_fwd(self.data, idx, counter, period, self.cy, self.cx, self.w1f, p["conv1_bias"], self.p1,
                        self.am1, self.amax_x if self.fp8 else None, self.xraw if train else None, **aug)
        if self.fp8:
            o.conv2_fwd_fp8(self.p1, self.w2f8[0], p["conv2_bias"], self.amax_x, self.scale_w, counter, self.p2, self.am2,
                            *((self.p1f8, self.sx8) if train and self.fp8_wgrad else (None, None)))
        elif not self.fused_fwd and self.conv_split == 1:
            o.conv2_fwd(self.p1, self.w2f, p["conv2_bias"], self.p2, self.am2)
        if train and self.fc_fused:
            self._fc_src = (idx, counter, period)    # fc forward + head run in _fc_backward's launch
            return
        self._gemm(self._fc1_fwd)
        o.head(self.h1part, p["full_bias_1"], self.fc2t, p["full_bias_2"], self.fc3t, p["full_bias_3"], self.fc3d,
               self.fc2n, self.labels, idx, counter, period, 1.0 / (self.Bv * self.world_size), self.relu_logits,
               train, self.h1, self.h2, self.dl, self.dh1, self.dh2, self.loss_part, self.correct_part, logits_out,
               self.Bv, self.step_t, self.step_sgd)

    def _gemm(self, f, sgd: bool = False):
        if sgd:
            self.ops.gemm_grouped(f["A"], f["B"], f["C"], f["bias"], f["params"], self.step_t, self.fc1n,
                                  self._sched())
        else:
            self.ops.gemm_grouped(f["A"], f["B"], f["C"], f["bias"], f["params"], self.step_t)

    def _fc_backward(self, fused_sgd: bool = False):
        if self.fc_fused:
            self._fc_chain(fused_sgd)
            return
        self._gemm(self._fc_bwd_sgd if fused_sgd else self._fc_bwd, sgd=fused_sgd)

    def _fc_chain(self, fused_sgd: bool):
        """fc1 forward + head + fc backward in one persistent launch (cnn_fc.hip), for the batch of
        the preceding _forward(train=True).  fused_sgd: the fc1 weights are updated in the dW1
        epilogue (single GPU), else the fc1 weight gradient goes to the flat gradient."""
        if self._fc_src is None:
            raise RuntimeError("_fc_chain must follow a training _forward")
        if self._dgrad_done:
            raise RuntimeError("the previous fc chain's conv backward never ran")
        idx, counter, period = self._fc_src
        self._fc_src = None
        # the binding picks the flat views the chain writes from the switches: master where an SGD is
        # fused (fc1: fuse_sgd, the rest: fc_sgd), else grad (grad16 on the RCCL bf16 wire)
        self.ops.fc_chain(self.master, self.buf, idx, counter, period, SEG_OFF, self._sched(), self.Bv,
                          1.0 / (self.Bv * self.world_size), self.relu_logits, fuse_sgd=fused_sgd,
                          dw_tasks=not (fused_sgd and self.fc_dw_in_wgrad), dgrad=self.fc_dgrad,
                          fc_sgd=fused_sgd and self.fc_sgd_in_chain)
        self._dgrad_done = self.fc_dgrad

    def _backward_fused(self):
        """The training step's whole backward + SGD as one launch (bwd_fused; cnn_bwd.hip), for the
        batch of the preceding _forward(train=True)."""
        if self._fc_src is None:
            raise RuntimeError("_backward_fused must follow a training _forward")
        if self._dgrad_done:
            raise RuntimeError("the previous fc chain's conv backward never ran")
        idx, counter, period = self._fc_src
        self._fc_src = None
        self.ops.backward_fused(self.master, self.buf, idx, counter, period, SEG_OFF, self._sched(),
                                self.order_desc, self.cy, self.cx, self.groups2, self.Bv,
                                1.0 / (self.Bv * self.world_size), self.relu_logits)

    def _conv_backward(self, src=None, apply: bool = False, reduce: bool = False):
        """apply: + the whole SGD in the wgrad launch (single GPU); reduce: + the conv slab reduction
        into the flat gradient (SGD mode 1) in the wgrad launch."""
        o = self.ops
        idx, counter, period = src or (self.bidx, None, 1)
        assert not apply or (self.wgrad_apply and src is None), "apply mode: the training step only"
        assert not reduce or self._grad_in_launch
        if self._dgrad_done:
            self._dgrad_done = False                 # the fc chain launch did it (fc_dgrad)
        elif self.fp8_dgrad:
            o.conv2_dgrad_fp8(self.dp2, self.am2, self.w2f8[1], self.scale_w, self.dp1, self.dy2,
                              *((self.dy2f8, self.sy_img) if self.fp8_wgrad else (None, None)))
        elif self.dgrad_split == 2:
            o.conv2_dgrad_split(self.dp2, self.am2, self.w2d, self.dp1, self.dy2)
        else:
            o.conv2_dgrad(self.dp2, self.am2, self.w2d, self.dp1, self.dy2)
        if apply or reduce:
            mode = 0 if apply else 1
            o.wgrad_sgd(self.master, self.buf, idx, counter, period, SEG_OFF, self._sched(), self.order_desc, mode,
                        self.cy, self.cx, self.groups2, self.Bv, prefetch=self._prefetch_next(mode),
                        fc_dw=bool(apply and self.fc_dw_in_wgrad), fc_sgd_done=bool(apply and self.fc_sgd_in_chain))
            return
        o.wgrad(self.data, idx, counter, period, self.cy, self.cx, self.dp1, self.am1,
                self.part1, self.partb1, self.p1, self.dy2, self.part2, self.partb2, self.groups2, self.xraw,
                **self._w8, **({"aug": self.aug} if self.aug is not None else {}))

    def _prefetch_next(self, mode: int, finalize: bool = True) -> bool:
        """Whether an SGD of this mode also gathers the next step's raw images into xraw."""
        return bool(self.xraw_prefetch and mode in (0, 2) and finalize)

    def _sgd(self, mode: int, scale: float = 1.0, roles: int = 0, finalize: bool = True, fc1_fused: bool = False):
        # (the binding takes grad16 for the flat gradient in modes 1 / 2 where the engine has one, and
        # the head's step copy in every mode but 3)
        self.ops.sgd(self.master, self.buf, SEG_OFF, self._sched(scale), self.order_desc, mode, roles, finalize,
                     fc1_fused, self.Bv, self._prefetch_next(mode, finalize))

    @property
    def barriers_in_use(self) -> bool:
        """The wgrad launch meets at sub-grid barriers: apply mode (single-GPU SGD) or the in-launch
        conv-slab reduction (data parallel / compute_gradients)."""
        return bool(self.wgrad_apply or self._grad_in_launch or self.fc_fused or self.fwd12_split)

    def queue_error_copy(self):
        """Enqueue a copy of the barrier error word into pinned host memory (stream-ordered: valid once
        an event recorded after this call has completed)."""
        if self.barriers_in_use:
            self._err_host.copy_(self.wbar[ERR_WORD:ERR_WORD + 1], non_blocking=True)

    def check_barriers(self, cached: bool = False):
        """Raise if a sub-grid barrier of the wgrad launch timed out (sticky device error word): apply
        mode would have updated the weights, the reduce mode would have reduced (and all-reduced)
        partial conv gradients -- every replica would agree on them, so the replica check cannot see
        it.  ``cached``: read the pinned copy of :meth:`queue_error_copy` (no device sync)."""
        if not self.barriers_in_use:
            return
        e = int(self._err_host[0]) if cached else int(self.wbar[ERR_WORD].item())
        if e != 0:
            # error word: value 1 = a wgrad sub-grid barrier, value 2 = an fc chain hand-off timed out
            mode = "apply" if self.wgrad_apply else "reduce"
            parts = []
            if e & 1:
                parts.append(f"k_wgrad ({mode} mode): a sub-grid barrier timed out; rerun with DMLC_WGRAD_SGD=0")
            if e & 2:
                parts.append("k_fc_chain / k_conv12_fwd_split: a hand-off wait timed out; rerun with "
                             "DMLC_FC_FUSED=0 / DMLC_FWD12_SPLIT=0")
            if e & 4:                      # (generation-valued words: nothing to re-arm)
                parts.append("k_backward: a per-image dY2 / dP1 hand-off wait timed out; rerun with the engine "
                             "variant bwd_fused=0")
            if self.fwd12_split:
                self.c12_flags.zero_()     # a timed-out hand-off can leave a partner's flag raised
            raise RuntimeError("; ".join(parts) + f" (blocks not co-resident, error word {e})")

    def _allreduce_bucket(self, fc: bool):
        off, n = self._buckets[fc]
        if self.xgmi is not None:
            self.xgmi.all_reduce(off, n)
        elif fc or self.grad16 is not None:
            self._allreduce(self._wire_grad()[off:off + n])
        else:
            # the 0.43 MB conv bucket sits on the step's critical path: fp32 on any wire (latency-bound
            # at this size; the bf16 wire's two cast kernels would cost more than the bytes it saves)
            import torch.distributed as dist
            dist.all_reduce(self.grad[off:off + n], group=self.pg)

    def _wire_grad(self) -> torch.Tensor:
        """The flat gradient the collectives run on (grad16 on the RCCL bf16 wire)."""
        return self.grad16 if self.grad16 is not None else self.grad

    def _backend(self) -> str:
        if self.xgmi is not None:
            return "xgmi"
        if not self.dp:
            return "none"
        return self._pg_backend()

    # segments of one step: each is a capturable list of launches on the current stream
    def _seg_compute_a(self):
        self._forward(self.bidx, None, 1, train=True)
        self._fc_backward()

    def _seg_forward(self):
        self._forward(self.bidx, None, 1, train=True)

    def _seg_fc(self):
        self._fc_backward()

    def _seg_compute_b(self):
        if self.wgrad_reduce:                   # conv slabs reduced inside the wgrad launch
            self._conv_backward(reduce=True)
            return
        self._seg_compute_b_launch()

    def _seg_compute_b_launch(self):
        """conv backward + the slab reduction as its own SGD launch.  The overlap schedule always uses
        it: its wgrad launch runs beside the comm stream's collective, and sub-grid barriers there
        could close a cycle across GPUs -- a collective partly resident on each of two GPUs, each
        GPU's missing collective blocks waiting for CUs held by wgrad blocks that spin for their own
        missing blocks, which wait for the CUs of the resident collective blocks, which wait on the
        other GPU.  The bounded spin would turn that into a timeout (a wrong step), so no in-launch
        barrier ever runs beside a collective."""
        self._conv_backward()
        self._sgd(mode=1 if self.dp else 0)

    def _seg_apply(self):
        self._sgd(mode=2, scale=1.0)

    def _seg_apply_fc(self):
        # fc parameters: SGD from the all-reduced fc bucket; runs on the comm stream while the conv
        # backward still runs on the main stream (it touches no conv weights / conv gradients)
        self._sgd(mode=2, scale=1.0, roles=2, finalize=False)

    def _seg_apply_conv(self):
        self._sgd(mode=2, scale=1.0, roles=1, finalize=True)

    def compute_gradients(self, idx: Optional[torch.Tensor] = None, check: bool = True):
        """Forward + backward only (no update); the full gradient lands in ``self.grad``.
        ``idx``: explicit dataset rows (int32 [Bv]) instead of this step's generated batch.
        ``check`` (default True): SYNCHRONISES the device (one read of the error word) and raises if a
        persistent launch's hand-off timed out (the gradient would be partial); loops that call this
        repeatedly should pass False -- the call is then asynchronous -- and call check_barriers() at
        their own sync point."""
        g = self._compute_gradients(idx)
        if check:
            self.check_barriers()
        return g if self.grad16 is None else self.grad16.float()   # (grad16: a converted copy)

    def _compute_gradients(self, idx: Optional[torch.Tensor] = None):
        if idx is None:
            self._seg_compute_a()
            if self._grad_in_launch:
                self._conv_backward(reduce=True)
                return self.grad
            self._conv_backward()
        else:
            ids = self._padded(idx)
            self._forward(ids, None, 1, train=True)
            self._fc_backward()
            if self._grad_in_launch:
                self._conv_backward(src=(ids, None, 1), reduce=True)
                self._sync_xraw()                    # the explicit rows went through xraw
                return self.grad
            self._conv_backward(src=(ids, None, 1))
            self._sync_xraw()
        self._sgd(mode=1)
        return self.grad

    def _reset_step_state(self):
        """Forget a half-issued step (an exception between the fc chain and the conv backward, an
        interrupted capture): the next step starts clean instead of failing the pairing checks."""
        self._fc_src = None
        self._dgrad_done = False
        self._pending_comm = None          # callers synchronise the device first (capture())
        if self.fwd12_split and not torch.cuda.is_current_stream_capturing():
            self.c12_flags.zero_()         # stream-ordered: no half-finished hand-off carries over

    def _eager_step(self):
        try:
            self._eager_step_body()
        except BaseException:
            self._reset_step_state()
            raise
        if not torch.cuda.is_current_stream_capturing():
            self._join_comm()             # an eager step ends joined (captures join at the chain's end)

    def _eager_step_body(self):
        if not self.dp:
            if self.fc1_epilogue:
                self._forward(self.bidx, None, 1, train=True)
                if self.bwd_fused:                  # fc chain + dgrad + wgrad + SGD: one launch
                    self._backward_fused()
                    return
                self._fc_backward(fused_sgd=True)
                if self.wgrad_apply:                # the SGD runs inside the wgrad launch
                    self._conv_backward(apply=True)
                    return
                self._conv_backward()
                self._sgd(mode=0, fc1_fused=True)
                return
            self._seg_compute_a()
            self._seg_compute_b()
            return
        (self._serial_dp_step if self.dp_schedule == "serial" else self._dp_step)(self._segments())

    def _segments(self):
        """The data-parallel step's capturable pieces, between which its collectives run."""
        if self.dp_schedule == "serial":
            return [self._seg_compute_ab, self._seg_apply]
        return [self._seg_forward, self._seg_fc, self._seg_compute_b_launch, self._seg_apply_fc, self._seg_apply_conv]

    def _seg_compute_ab(self):
        self._seg_compute_a()
        self._seg_compute_b()

    def _serial_dp_step(self, seg):
        """Single-stream data-parallel step: fwd + bwd + conv-grad reduction | ONE all-reduce of the
        whole flat gradient (4.27 MB fp32; the two buckets are contiguous) | one SGD launch -- or, over
        xGMI (comm_sgd), the exchange kernel that applies the SGD itself."""
        seg[0]()
        n = self.master.numel()
        if self.comm_sgd:           # (xGMI: the whole step is one graph, seg is never a replay list)
            self.xgmi.all_reduce_sgd(self.master, self.buf, SEG_OFF, self._sched(), self.order_desc, self.Bv,
                                     self._prefetch_next(2), blocks=self._comm_blocks)
            return
        if self.xgmi is not None:
            self.xgmi.all_reduce(0, n)
        else:
            self._allreduce(self._wire_grad()[:n])
        seg[1]()

    def _dp_step(self, seg):
        """Data-parallel step around two all-reduce buckets, two streams:
            main: fwd | [join s-1] fc chain | wgrad, slab-reduction launch |     [wait] conv SGD (+ finalize)
            comm:                  [wait] all-reduce fc | [wait] all-reduce conv -> fc SGD
        Both collectives go through ONE stream in one order (one communicator, the same issue order on
        every rank).  The fc bucket (90 % of the bytes) crosses the links while the wgrad launch runs;
        only the 0.43 MB conv bucket and the conv SGD stay on the step's critical path.  The fc SGD
        (fc weights + shadows) is NOT joined at the end of the step: the next step's forward does not
        read an fc parameter, so the join sits before the next fc chain (the fc SGD runs beside the
        next conv12 forward) -- :meth:`_join_comm` closes a sequence (end of a captured chain, an eager
        step, before a graph replay).
        seg: [forward, fc chain, conv backward, fc apply, conv apply] (eager launchers or, with eager
        collectives, replays of the segment graphs)."""
        main = torch.cuda.current_stream(self.device)
        seg[0]()
        self._join_comm()                       # step s-1's fc SGD wrote the shadows the chain reads
        seg[1]()
        ev_fc = torch.cuda.Event()
        ev_fc.record(main)
        self.comm_stream.wait_event(ev_fc)
        with torch.cuda.stream(self.comm_stream):
            self._allreduce_bucket(fc=True)
        seg[2]()
        ev_wg = torch.cuda.Event()
        ev_wg.record(main)
        self.comm_stream.wait_event(ev_wg)
        ev_conv, ev_done = torch.cuda.Event(), torch.cuda.Event()
        with torch.cuda.stream(self.comm_stream):
            self._allreduce_bucket(fc=False)
            ev_conv.record(self.comm_stream)
            seg[3]()
            ev_done.record(self.comm_stream)
        main.wait_event(ev_conv)
        seg[4]()
        self._pending_comm = ev_done

    def _join_comm(self):
        """The current stream waits for the last step's comm-stream work (the fc SGD)."""
        ev = getattr(self, "_pending_comm", None)
        if ev is not None:
            torch.cuda.current_stream(self.device).wait_event(ev)
            self._pending_comm = None

    # --- graph capture (capture / run / step: engine/base.py) --------------------------------------
    def _replay_segments(self):
        """RCCL without ``capture_comm``: the graphs of ``_segments`` around eager collectives."""
        if self._captured_schedule == "serial":
            self._serial_dp_step([g.replay for g in self.graphs])
        else:
            self._dp_step([g.replay for g in self.graphs])
            self._join_comm()

    def capture(self, steps_per_graph: int = 8):
        self._captured_schedule = self.dp_schedule
        super().capture(steps_per_graph)
        self.chains.setdefault(1, None)    # (several graphs: no chains)

    def add_chain(self, k: int) -> bool:
        """Also capture a chain of exactly ``k`` steps, so :meth:`run` (k) is ONE graph replay (a
        short timed region otherwise pays one graph-launch boundary per power-of-two piece)."""
        k = int(k)
        if not self.single_graph or not self.graphs or k < 2 or self.chains.get(k) is not None:
            return False
        quiesce_for_capture(self.device, self.pg if self.dp else None)
        self.chains[k] = self._capture_one(lambda: self._steps_joined(k), self._pool)
        torch.cuda.synchronize(self.device)
        return True

    def tune_schedule(self, iters: int = 30, steps_per_graph: int = 8, rounds: int = 2, log=None) -> str:
        """Data-parallel step: capture each schedule (overlap / serial), time ``iters`` real
        training steps of each (max over ranks, so every rank takes the same decision) over
        ``rounds`` alternating rounds (overlap, serial, serial, overlap, ...), keep the minimum per
        schedule and the faster schedule captured.  Both windows replay the same chain
        decomposition and cross no host work (the data order is generated in-kernel), so neither
        pays for anything the other does not.  The timed steps are ordinary training steps."""
        if not self.dp:
            return self.dp_schedule
        import time
        import torch.distributed as dist
        nccl = self._backend() == "nccl" or (self.xgmi is not None and dist.get_backend(self.pg) == "nccl")
        bdev = self.device if nccl else torch.device("cpu")
        times = {"overlap": [], "serial": []}
        order = []
        for r in range(max(1, rounds)):
            order += ["overlap", "serial"] if r % 2 == 0 else ["serial", "overlap"]
        for sched in order:
            self.dp_schedule = sched
            self.capture(steps_per_graph)
            self.run(steps_per_graph)
            torch.cuda.synchronize(self.device)
            dist.barrier(group=self.pg)
            t0 = time.perf_counter()
            self.run(iters)
            torch.cuda.synchronize(self.device)
            t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=bdev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX, group=self.pg)
            # a persistent launch's bounded wait timed out on some rank: that schedule is out (the
            # sticky word is cleared for the run that follows; every rank sees the same MAX)
            e = torch.tensor([int(self.wbar[ERR_WORD].item()) if self.barriers_in_use else 0],
                             dtype=torch.float64, device=bdev)
            dist.all_reduce(e, op=dist.ReduceOp.MAX, group=self.pg)
            if self.xgmi is not None:
                self.xgmi.check()      # a timed-out exchange leaves no consistent epoch to resume from
            if float(e.item()) != 0.0:
                if log:
                    log(f"dp schedule {sched}: a persistent launch's wait timed out -- not eligible")
                self.wbar[ERR_WORD].zero_()
                times[sched].append(math.inf)
                continue
            times[sched].append(float(t.item()) / iters)
        best_t = {k: min(v) for k, v in times.items()}
        best = min(best_t, key=best_t.get)
        self.comm_info.update(schedule=best, schedule_us={k: round(v * 1e6, 1) for k, v in best_t.items()
                                                          if v != math.inf})
        if log:
            log(f"dp schedule: {best} ({self.comm_info['schedule_us']})")
        if best != self.dp_schedule:
            self.dp_schedule = best
            self.capture(steps_per_graph)
        return best

    # --- evaluation -----------------------------------------------------------------------------
    @torch.no_grad()
    def evaluate(self, data: torch.Tensor, labels: torch.Tensor, max_batches: int = 0) -> float:
        """Test accuracy over ``data`` (uint8 [N,32,32,3]) with the fused forward kernels."""
        data = data.to(self.device).contiguous()
        labels = labels.to(self.device, torch.int32).contiguous()
        saved = (self.data, self.labels)
        self.data, self.labels = data, labels
        if self.fp8:    # eval launches carry no step counter: they read scale slot 0 (see cnn_fp8.hip)
            self.scale_w[0] = self.scale_w[self.host_step & 1]
        n = data.shape[0]
        nb = math.ceil(n / self.Bv)
        if max_batches:
            nb = min(nb, max_batches)
        correct, total = 0, 0
        try:
            for i in range(nb):
                ids = torch.arange(i * self.Bv, i * self.Bv + self.B, device=self.device, dtype=torch.int32)
                valid = int(min(self.Bv, n - i * self.Bv))
                ids = torch.clamp(ids, max=n - 1)
                self._forward(ids, None, 1, train=False, logits_out=self.logits_buf)
                pred = self.logits_buf[:valid].argmax(dim=1)
                correct += int((pred == labels[i * self.Bv:i * self.Bv + valid].long()).sum())
                total += valid
        finally:
            self.data, self.labels = saved
        return correct / max(1, total)

    @torch.no_grad()
    def forward_logits(self, idx: torch.Tensor) -> torch.Tensor:
        """Logits (fp32 [n,10]) of dataset rows ``idx`` (int32 [n], n <= B) — for tests."""
        if self.fp8:
            self.scale_w[0] = self.scale_w[self.host_step & 1]
        n = idx.numel()
        self._forward(self._padded(idx), None, 1, train=False, logits_out=self.logits_buf)
        return self.logits_buf[:n].clone()

    # --- state ----------------------------------------------------------------------------------
    def fc1n_current(self) -> torch.Tensor:
        """The bf16 fc1 weight shadow the kernels of the current step read ([2304][384])."""
        return self.fc1n[self.global_step() & 1]

    def load_flat_params(self, flat: torch.Tensor, step: Optional[int] = None):
        self.master.copy_(flat.to(self.device, torch.float32))
        if step is not None:
            self.set_step(step)
        self.refresh_shadows()
