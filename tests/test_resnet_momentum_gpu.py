"""SGD momentum + L2 weight decay inside the fused ResNet-20 SGD kernel (k_rn_sgd, csrc/kernels/resnet_sgd.hip):

    v <- mu * v + (g + wd_eff * w);  w <- w - lr * v;  wd_eff = wd on conv kernels / fc weights, else 0

exact against the host formula on dyadic inputs, every applying mode against the others, graph replay
against eager launches, checkpoint slots and bitwise resume through the CLI, and the binding's checks."""
import os
import subprocess
import sys

import pytest
import torch

from dmlc import checkpoint as CK
from dmlc.engine.eager import EagerTrainer
from dmlc.engine.fused_resnet import FusedResNetEngine
from dmlc.models import resnet as R
from dmlc.models.cifar_cnn import decay_mask

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _data(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, (n, 32, 32, 3), dtype=torch.uint8, generator=g),
            torch.randint(0, 10, (n,), dtype=torch.int32, generator=g))


def _spec_fill(gen, pad):
    """A flat buffer with seeded integers in [-8, 8] over every spec range and ``pad`` elsewhere."""
    t = torch.full((R.FLAT_SIZE,), float(pad))
    for s in R.PARAM_SPECS:
        t[s.offset:s.offset + s.numel] = torch.randint(-8, 9, (s.numel,), generator=gen).float()
    return t


def test_dyadic_inputs_match_host_formula_bitwise():
    """lr 0.5, momentum 0.5, decay 0.25 on integers in [-8, 8]: after two steps every value is a
    multiple of 1/64 below 32 in magnitude, so every product and partial sum is representable and
    the result is exact whatever the compiler fuses (the fp32 host formula equals its fp64 twin,
    asserted here).  master and vel must equal it bit for bit over every spec range, the alignment
    padding must be untouched, and the bf16 shadows must come from the updated weights."""
    lr, mu, wd = 0.5, 0.5, 0.25
    data, labels = _data(64, seed=1)
    eng = FusedResNetEngine(16, data, labels, seed=3, lr=lr, staircase=False, warmup_steps=0, momentum=mu,
                            weight_decay=wd)
    dev = eng.device
    gen = torch.Generator().manual_seed(11)
    w, v = _spec_fill(gen, 3.0), _spec_fill(gen, 5.0)
    eng.master.copy_(w)
    eng.vel.copy_(v)
    eng.grad = torch.zeros_like(eng.master)
    mask = decay_mask(R.PARAM_SPECS)
    inside = torch.zeros(R.FLAT_SIZE, dtype=torch.bool)
    for s in R.PARAM_SPECS:
        inside[s.offset:s.offset + s.numel] = True
    w64, v64 = w.double(), v.double()
    for step in range(2):
        g = _spec_fill(gen, 7.0)
        eng.grad.copy_(g)
        eng._sgd(mode=2, scale=1.0)
        torch.cuda.synchronize()
        v = mu * v + (g + wd * mask * w)                      # fp32 torch ops
        w = w - lr * v
        v64 = mu * v64 + (g.double() + wd * mask.double() * w64)
        w64 = w64 - lr * v64
        assert torch.equal(w.double(), w64) and torch.equal(v.double(), v64)     # exact by construction
        got_w, got_v = eng.master.cpu(), eng.vel.cpu()
        for s in R.PARAM_SPECS:
            sl = slice(s.offset, s.offset + s.numel)
            assert torch.equal(got_v[sl], v[sl]), (step, s.name)
            assert torch.equal(got_w[sl], w[sl]), (step, s.name)
        assert bool((got_w[~inside] == 3.0).all()) and bool((got_v[~inside] == 5.0).all())
        assert bool((eng.grad.cpu()[~inside] == 7.0).all())
        assert eng.global_step() == step + 1
        wf = [t.clone() for t in eng.wf]
        wdg = [t.clone() for t in eng.wd]
        eng.refresh_shadows()
        torch.cuda.synchronize()
        for l in range(len(wf)):
            assert torch.equal(wf[l], eng.wf[l]), (step, l)
            if l > 0:
                assert torch.equal(wdg[l], eng.wd[l]), (step, l)
    assert float(w.abs().max()) < 32 and bool(((w * 64).frac() == 0).all())


@pytest.mark.parametrize("B", [32, 20])
def test_mode0_equals_mode1_then_mode2(B):
    """step() (mode 0: reduce + apply) against compute_gradients() + the apply half (mode 1, mode 2
    with scale 1): the gradient is materialised before the pinned fmaf chain, so both round alike."""
    data, labels = _data(8 * 32, seed=5)
    kw = dict(seed=9, lr=0.05, momentum=0.9, weight_decay=5e-4)
    one = FusedResNetEngine(B, data, labels, **kw)
    two = FusedResNetEngine(B, data, labels, **kw)
    for _ in range(3):
        one.step()
        two.compute_gradients()
        two._sgd(mode=2, scale=1.0)
    torch.cuda.synchronize()
    assert one.global_step() == two.global_step() == 3
    assert torch.equal(one.master, two.master)
    assert torch.equal(one.vel, two.vel)
    assert torch.equal(one.state, two.state)
    assert float(one.vel.abs().max()) > 0 and bool(torch.isfinite(one.master).all())


def test_first_step_velocity_is_the_gradient():
    data, labels = _data(4 * 32, seed=6)
    lr = 0.05
    eng = FusedResNetEngine(32, data, labels, seed=4, lr=lr, momentum=0.9)
    twin = FusedResNetEngine(32, data, labels, seed=4, lr=lr, momentum=0.9)
    w0 = eng.flat_params().clone()
    assert float(eng.vel.abs().max()) == 0
    g = twin.compute_gradients().cpu().clone()
    eng.step()
    torch.cuda.synchronize()
    vel = eng.velocity_params()
    assert torch.equal(vel, g)
    want = w0.double() - lr * vel.double()
    got = eng.flat_params().double()
    assert float((got - want).norm() / want.norm()) < 1e-6
    assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max())


def _same(a, b, steps):
    assert a.global_step() == b.global_step() == steps
    assert torch.equal(a.master, b.master)
    assert torch.equal(a.vel, b.vel)
    assert torch.equal(a.state, b.state)
    assert torch.equal(a.stats[:steps], b.stats[:steps])


def test_graph_replay_equals_eager_launches_with_momentum():
    """One eager step (code-object load), then capture() + run(6) against six step() calls, and the
    same with the stage-wise SGD launches on a graph branch (sgd_split) against one SGD launch."""
    B = 32
    data, labels = _data(8 * B, seed=21)
    kw = dict(seed=5, lr=0.05, momentum=0.9, weight_decay=5e-4)
    eager = FusedResNetEngine(B, data, labels, **kw)
    graph = FusedResNetEngine(B, data, labels, **kw)
    split = FusedResNetEngine(B, data, labels, sgd_split=True, **kw)
    assert split.sgd_split and not graph.sgd_split
    for e in (eager, graph, split):
        e.step()
    for _ in range(6):
        eager.step()
    for e in (graph, split):
        e.capture()
        e.run(6)
    torch.cuda.synchronize()
    assert graph.chains and split.chains
    _same(graph, eager, 7)
    _same(split, eager, 7)
    assert float(eager.vel.abs().max()) > 0 and bool(torch.isfinite(eager.master).all())


def _cli(log_dir, generations):
    cmd = [sys.executable, os.path.join(REPO, "cifar10cnn.py"), "--model=resnet20", "--synthetic",
           "--synthetic_size=1024", "--batch_size=64", "--momentum=0.9", "--weight_decay=5e-4",
           "--learning_rate=0.05", "--output_every=3", "--eval_every=100", "--eval_batches=1",
           "--checkpoint_secs=0", "--steps_per_graph=2", f"--generations={generations}", f"--log_dir={log_dir}"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout, CK.read_bundle(CK.latest_checkpoint(str(log_dir)))


@pytest.mark.timeout(600)
def test_cli_fused_resnet20_momentum_checkpoint_resume(tmp_path):
    parts, whole = tmp_path / "parts", tmp_path / "whole"
    out, t6 = _cli(parts, 6)
    assert "engine=fused model=resnet20" in out and "momentum=0.9 weight_decay=0.0005" in out, out[-2000:]
    assert os.path.exists(parts / "model.ckpt-3.index")             # a checkpoint at step 3 too
    assert int(t6["global_step"]) == 6
    slot = t6["resnet20/stem/conv/kernel/Momentum"]
    assert slot.dtype == torch.float32 and tuple(slot.shape) == (3, 3, 3, 16) and float(slot.abs().max()) > 0
    assert sorted(k for k in t6 if k.endswith("/Momentum")) == sorted(s.name + "/Momentum" for s in R.PARAM_SPECS)
    out2, t9 = _cli(parts, 9)
    assert "Restored" in out2 and "no */Momentum slots" not in out2, out2[-2000:]
    _, w9 = _cli(whole, 9)
    assert int(t9["global_step"]) == int(w9["global_step"]) == 9
    assert set(t9) == set(w9)
    for k in w9:
        assert torch.equal(t9[k], w9[k]), k


def test_binding_rejects_bad_momentum_arguments():
    data, labels = _data(64, seed=2)
    eng = FusedResNetEngine(16, data, labels, seed=1, momentum=0.9, weight_decay=5e-4)
    eng.grad = torch.zeros_like(eng.master)
    good = eng.vel
    w0 = eng.master.clone()

    def rejected(mode=0, **attrs):
        for k, val in attrs.items():
            setattr(eng, k, val)
        try:
            with pytest.raises(RuntimeError):
                eng._sgd(mode=mode, scale=1.0)
        finally:
            eng.vel, eng.momentum, eng.weight_decay = good, 0.9, 5e-4

    rejected(vel=good.to(torch.bfloat16))
    rejected(vel=good.double())
    rejected(vel=good[:-64])
    rejected(vel=torch.zeros(good.numel() + 64, device=good.device))
    rejected(vel=good.cpu())
    rejected(momentum=1.0)
    rejected(momentum=1.5)
    rejected(momentum=-0.1)
    rejected(weight_decay=-1e-4)
    rejected(mode=0, vel=None)
    rejected(mode=2, vel=None)
    torch.cuda.synchronize()
    assert eng.global_step() == 0 and torch.equal(eng.master, w0) and float(good.abs().max()) == 0   # nothing launched
    eng.vel = None                                   # the non-applying modes need no velocity
    eng._sgd(mode=3)
    eng._sgd(mode=1)
    eng.vel = good
    eng._sgd(mode=2, scale=1.0)
    torch.cuda.synchronize()
    assert eng.global_step() == 1


def test_engine_without_momentum_has_no_velocity():
    data, labels = _data(64, seed=2)
    eng = FusedResNetEngine(16, data, labels, seed=1)
    assert eng.vel is None and eng.velocity_params() is None
    dec = FusedResNetEngine(16, data, labels, seed=1, weight_decay=0.25, lr=0.5, staircase=False)
    assert dec.vel is None                           # decay alone keeps no velocity
    w0 = dec.flat_params().clone()
    dec.grad = torch.zeros_like(dec.master)
    dec._sgd(mode=2, scale=1.0)
    torch.cuda.synchronize()
    want = w0 - 0.5 * (0.25 * decay_mask(R.PARAM_SPECS) * w0)
    assert float((dec.flat_params() - want).abs().max()) <= 1e-6 * float(w0.abs().max())


def test_eager_graph_step_with_momentum_follows_the_formula():
    """The eager engine's captured step (fp32 GPU path) with the options on: the velocity and the
    decay mask are created in the warm-up steps, so the captured update stays valid across replays.
    5 replays after the 3 warm-up steps against the formula in fp64, driven by the gradients the
    trainer itself computed (``flat.grad`` is the captured step's static gradient): a few fp32 roundings per
    element and step, far below 1e-5 (two trainers cannot be compared this tightly: the fp32 conv
    backward is not reproducible run to run, and eight steps amplify that)."""
    from dmlc.data import synthetic
    from dmlc.models import cifar_cnn as M
    x, y = synthetic(512, seed=4, learnable=True)
    lr, mu, wd = 1e-4, 0.9, 5e-4
    tr = EagerTrainer("cifar_cnn", 64, x, y, graph=True, device="cuda", dtype="fp32", crop=24, seed=2, lr=lr,
                      relu_logits=False, momentum=mu, weight_decay=wd)
    mask = decay_mask(M.PARAM_SPECS).double()
    for _ in range(3):                             # warm-up; the third call also captures the step
        tr.step()
    torch.cuda.synchronize()
    assert tr.graph is not None
    w, v = tr.flat_params().double(), tr.velocity_params().double()
    assert float(v.abs().max()) > 0
    for _ in range(5):
        tr.step()
        torch.cuda.synchronize()
        g = tr.model.flat.grad.detach().double().cpu()
        v = mu * v + (g + wd * mask * w)
        w = w - lr * v
    assert tr.graph is not None and tr.global_step == 8
    rel = lambda a, b: float((a - b).norm() / b.norm())
    assert rel(tr.flat_params().double(), w) < 1e-5
    assert rel(tr.velocity_params().double(), v) < 1e-5
