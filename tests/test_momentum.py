"""SGD momentum + L2 weight decay (--momentum / --weight_decay) without a GPU: the eager engine against
an fp64 twin of the formula, checkpoint slots and bitwise resume through the CLI, the engine routing
and the rank-based decay mask.

    v <- mu * v + (g + wd_eff * w);  w <- w - lr * v;  wd_eff = wd on rank >= 2 specs, 0 on rank 1
"""
import os
import subprocess
import sys

import pytest
import torch

from dmlc import checkpoint as CK
from dmlc.config import TrainConfig
from dmlc.engine.eager import EagerTrainer
from dmlc.engine.trainer import pick_impl
from dmlc.models import cifar_cnn as M
from dmlc.models import resnet as R
from dmlc.models.cifar_cnn import decay_mask

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = os.path.join(REPO, "cifar10cnn.py")
MU, WD = 0.9, 5e-4


def _data(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, (n, 32, 32, 3), dtype=torch.uint8, generator=g),
            torch.randint(0, 10, (n,), dtype=torch.int32, generator=g))


# ---- 1. fp64 twin ----------------------------------------------------------------------------------
@pytest.mark.parametrize("model,batch,crop,lr,specs", [("cifar_cnn", 8, 24, 1e-4, M.PARAM_SPECS),
                                                       ("resnet20", 4, 32, 0.05, R.PARAM_SPECS)])
def test_eager_matches_fp64_twin(model, batch, crop, lr, specs):
    """3 CPU fp32 steps with momentum 0.9 / decay 5e-4 against the formula in fp64, driven by the
    gradients the trainer itself computed (left in ``flat.grad`` after each step).  A few fp32
    roundings per element and step sit far below 1e-5; a missing mask or a wrong sign is O(1).  (The
    raw-pixel CNN's gradients dwarf a 5e-4 decay term: test_decay_without_momentum_keeps_no_velocity
    shows the term and its mask with a decay large enough to see.)"""
    data, labels = _data(64, seed=3)
    tr = EagerTrainer(model, batch, data, labels, device="cpu", dtype="fp32", lr=lr, staircase=False,
                      relu_logits=False, crop=crop, seed=1, momentum=MU, weight_decay=WD)
    mask = decay_mask(specs).double()
    w = tr.flat_params().double()
    v = torch.zeros_like(w)
    v_nodecay = torch.zeros_like(w)              # the same recursion without any decay term
    for _ in range(3):
        tr.step()
        g = tr.model.flat.grad.detach().double()
        v = MU * v + (g + WD * mask * w)
        v_nodecay = MU * v_nodecay + g
        w = w - lr * v
    got_w, got_v = tr.flat_params().double(), tr.velocity_params().double()
    rel = lambda a, b: float((a - b).norm() / b.norm())
    assert rel(got_w, w) < 1e-5, rel(got_w, w)
    assert rel(got_v, v) < 1e-5, rel(got_v, v)
    for s in specs:
        sl = slice(s.offset, s.offset + s.numel)
        assert rel(got_w[sl], w[sl]) < 1e-5 or float((got_w[sl] - w[sl]).abs().max()) < 1e-7, s.name
        if len(s.shape) == 1:                    # rank 1: the velocity is the pure gradient recursion
            assert float((got_v[sl] - v_nodecay[sl]).abs().max()) <= 1e-5 * float(v_nodecay[sl].abs().max()) + 1e-12, s.name


def test_zero_options_are_the_plain_update():
    data, labels = _data(64, seed=4)
    a = EagerTrainer("cifar_cnn", 8, data, labels, device="cpu", seed=2, lr=0.01)
    b = EagerTrainer("cifar_cnn", 8, data, labels, device="cpu", seed=2, lr=0.01, momentum=0.0, weight_decay=0.0)
    for _ in range(2):
        a.step()
        b.step()
    assert torch.equal(a.flat_params(), b.flat_params())
    assert b.velocity_params() is None and not b._vel


def test_decay_without_momentum_keeps_no_velocity():
    data, labels = _data(64, seed=4)
    tr = EagerTrainer("cifar_cnn", 8, data, labels, device="cpu", seed=2, lr=0.01, weight_decay=0.1)
    w0 = tr.flat_params().double()
    tr.step()
    g = tr.model.flat.grad.double()
    want = w0 - 0.01 * (g + 0.1 * decay_mask(M.PARAM_SPECS).double() * w0)
    assert not tr._vel
    assert float((tr.flat_params().double() - want).abs().max()) < 1e-6


def test_bad_options_are_rejected():
    data, labels = _data(16)
    for kw in (dict(momentum=1.0), dict(momentum=-0.1), dict(weight_decay=-1e-4)):
        with pytest.raises(ValueError):
            EagerTrainer("cifar_cnn", 8, data, labels, device="cpu", **kw)


# ---- 2.-4. checkpoints through the CLI -------------------------------------------------------------
COMMON = ["--synthetic", "--synthetic_size=256", "--batch_size=16", "--device=cpu", "--learning_rate=0.0001",
          "--relu_logits=false", "--output_every=3", "--eval_every=100", "--eval_batches=1"]
OPT = [f"--momentum={MU}", f"--weight_decay={WD}"]


def _cli(log_dir, generations, extra):
    env = dict(os.environ, OMP_NUM_THREADS="2")
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, ENTRY] + COMMON + extra + [f"--log_dir={log_dir}", f"--generations={generations}"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:]
    return r.stdout, CK.read_bundle(CK.latest_checkpoint(str(log_dir)))


@pytest.mark.timeout(300)
def test_cli_resume_equals_uninterrupted_run_bitwise(tmp_path):
    """6 steps in one run == 3 steps, a checkpoint, and 3 more from it: parameters and every
    ``*/Momentum`` slot bit for bit (the CPU eager engine is deterministic)."""
    out, whole = _cli(tmp_path / "whole", 6, OPT)
    assert "momentum=0.9 weight_decay=0.0005" in out
    _, half = _cli(tmp_path / "parts", 3, OPT)
    assert int(half["global_step"]) == 3
    out2, parts = _cli(tmp_path / "parts", 6, OPT)
    assert "Restored" in out2 and "no */Momentum slots" not in out2
    assert int(whole["global_step"]) == int(parts["global_step"]) == 6
    assert set(whole) == set(parts)
    slots = [k for k in whole if k.endswith("/Momentum")]
    assert sorted(slots) == sorted(s.name + "/Momentum" for s in M.PARAM_SPECS)
    for s in M.PARAM_SPECS:
        slot = whole[s.name + "/Momentum"]
        assert slot.dtype == torch.float32 and tuple(slot.shape) == tuple(s.shape)
        assert float(slot.abs().max()) > 0
    for k in whole:
        assert torch.equal(whole[k], parts[k]), k


@pytest.mark.timeout(300)
def test_cli_default_checkpoint_has_no_slots_and_momentum_can_continue_it(tmp_path):
    """The default run's checkpoint holds no ``/Momentum`` tensor; continuing it with --momentum starts
    from zero velocity, says so, and runs; the slots in a checkpoint are ignored without --momentum."""
    out, t = _cli(tmp_path, 2, [])
    assert "momentum=" not in out
    assert not [k for k in t if k.endswith("/Momentum")]
    assert sorted(t) == sorted([s.name for s in M.PARAM_SPECS] + ["global_step", "Variable"])
    out2, t2 = _cli(tmp_path, 4, ["--momentum=0.9"])
    assert "Restored" in out2 and "no */Momentum slots" in out2 and "velocity starts from zero" in out2
    assert int(t2["global_step"]) == 4
    assert float(t2[M.PARAM_SPECS[0].name + "/Momentum"].abs().max()) > 0
    out3, t3 = _cli(tmp_path, 5, [])                # slots present, no momentum: ignored, and not re-saved
    assert "Restored" in out3 and int(t3["global_step"]) == 5
    assert not [k for k in t3 if k.endswith("/Momentum")]


# ---- 5. routing --------------------------------------------------------------------------------------
def test_pick_impl_with_momentum_or_decay():
    cuda, cpu = torch.device("cuda"), torch.device("cpu")
    for opt in (dict(momentum=0.9), dict(weight_decay=5e-4), dict(momentum=0.9, weight_decay=5e-4)):
        rn = TrainConfig(model="resnet20", crop=32, **opt)
        assert pick_impl(rn, cuda) == "fused"
        assert pick_impl(rn.replace(augment=True), cuda) == "eager"
        assert pick_impl(rn, cpu) == "eager"
        assert pick_impl(TrainConfig(dtype="bf16", **opt), cuda) == "eager"
        assert pick_impl(TrainConfig(dtype="fp8", **opt), cuda) == "eager"
        assert pick_impl(TrainConfig(dtype="fp32", **opt), cuda) == "hipf32"
        assert pick_impl(TrainConfig(dtype="bf16", **opt), cpu) == "eager"
        assert pick_impl(TrainConfig(impl="fused", **opt), cuda) == "fused"      # explicit: the adapter refuses


def test_explicit_fused_cnn_with_momentum_raises():
    from dmlc.engine.trainer import _FusedAdapter
    for opt in (dict(momentum=0.9), dict(weight_decay=5e-4)):
        with pytest.raises(ValueError, match="momentum"):
            _FusedAdapter(TrainConfig(impl="fused", **opt), None, None, None)


def test_pick_impl_unchanged_with_zero_options():
    cuda, cpu = torch.device("cuda"), torch.device("cpu")
    z = dict(momentum=0.0, weight_decay=0.0)
    assert pick_impl(TrainConfig(**z), cuda) == "fused"
    assert pick_impl(TrainConfig(dtype="fp8", **z), cuda) == "fused"
    assert pick_impl(TrainConfig(augment=True, **z), cuda) == "fused"
    assert pick_impl(TrainConfig(dtype="fp32", **z), cuda) == "hipf32"
    assert pick_impl(TrainConfig(crop=32, **z), cuda) == "eager"
    assert pick_impl(TrainConfig(model="resnet20", crop=32, **z), cuda) == "fused"
    assert pick_impl(TrainConfig(model="resnet20", crop=32, augment=True, **z), cuda) == "eager"
    assert pick_impl(TrainConfig(model="resnet20", crop=32, dtype="fp32", **z), cuda) == "eager"
    assert pick_impl(TrainConfig(**z), cpu) == "eager"


def test_flags_parse():
    from dmlc import cli
    cfg, _ = cli.parse(["--momentum=0.9", "--weight_decay=5e-4"])
    assert cfg.momentum == 0.9 and cfg.weight_decay == 5e-4
    cfg, _ = cli.parse([])
    assert cfg.momentum == 0.0 and cfg.weight_decay == 0.0


# ---- 6. the mask ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("specs,size", [(M.PARAM_SPECS, M.FLAT_SIZE), (R.PARAM_SPECS, R.FLAT_SIZE)])
def test_decay_mask_marks_exactly_the_rank2_specs(specs, size):
    mask = decay_mask(specs)
    assert mask.dtype == torch.float32 and mask.numel() == size
    want = torch.zeros(size)
    for s in specs:
        sl = slice(s.offset, s.offset + s.numel)
        if len(s.shape) >= 2:
            want[sl] = 1.0
            assert bool((mask[sl] == 1).all()), s.name
        else:
            assert bool((mask[sl] == 0).all()), s.name
    assert torch.equal(mask, want)                       # the alignment padding is 0 too
    assert any(len(s.shape) == 1 for s in specs) and any(len(s.shape) >= 2 for s in specs)
    assert int(mask.sum()) == sum(s.numel for s in specs if len(s.shape) >= 2)
