"""The fused ResNet-20 engine's path selection and layer wiring (engine/plan_resnet.py) against what
the constructor that decided them inline decided, and the engine's launch sequence against the one that
constructor's engine issued.

tests/rn_plan_table.json was recorded from that engine, run without a GPU under the stand-ins of
tests/rn_stubs.py (a recording op namespace, fake streams and events), before the decisions moved into
``plan_resnet_step`` and the three wiring loops into the per-layer launchers.  Every expected value is
what that constructor decided or allocated -- ``B``, ``groups``, ``wgrad_branch``, ``merged_bwd``,
``sgd_split``, ``_per_image(l)`` and ``part[l].shape[0]`` -- and every expected launch list is what
its ``_eager_step()`` / ``compute_gradients(idx)`` issued; none comes from the code under test.
``rows``: [input overrides over ``base_inputs``, B, the three booleans and the 19 per-image flags as
0/1 strings, groups and slab counts as indices into ``lists``].  ``launches``: per configuration
[op, arguments (tensors by engine buffer name), stream]; ``wait_stream`` / ``wait_event`` rows are the
fork and join edges ("waiting<-awaited").
"""
import dataclasses
import json
import os
import subprocess
import sys

import pytest
import torch

import rn_stubs as S
from dmlc.engine import plan_resnet as P

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

with open(os.path.join(HERE, "rn_plan_table.json")) as f:
    TABLE = json.load(f)


def _rows():
    for over, B, flags, per_image, gi, pi in TABLE["rows"]:
        want = dict(B=B, per_image=tuple(c == "1" for c in per_image), groups=tuple(TABLE["lists"][gi]),
                    part_rows=tuple(TABLE["lists"][pi]))
        want.update(zip(("wgrad_branch", "merged_bwd", "sgd_split"), (c == "1" for c in flags)))
        yield dict(TABLE["base_inputs"], **over), want


ROWS = list(_rows())


def test_table_spans_the_grid_and_is_not_vacuous():
    ins = [i for i, _ in ROWS]
    assert {i["batch_size"] for i in ins} == {1, 8, 16, 100, 128, 256, 257, 512, 1024}
    assert {i["bwd_img_level"] for i in ins} == {0, 1, 2}
    for k in ("wgrad_branch", "merged_bwd"):
        assert {i[k] for i in ins} == {None, True, False}
        assert {w[k] for _, w in ROWS} == {False, True}
    assert {i["sgd_split"] for i in ins} == {False, True} and {w["sgd_split"] for _, w in ROWS} == {False, True}
    assert {(i["world_size"], i["dp_force"]) for i in ins} == {(1, False), (1, True), (2, False)}
    assert sum(i["groups"] is not None for i in ins) == 1 and len(ROWS) == 9 * 3 * 3 * 3 * 2 * 3 + 1
    grid = [(i, w) for i, w in ROWS if i["groups"] is None]
    for i, w in grid:
        B, lvl = w["B"], i["bwd_img_level"]
        assert B == -(-i["batch_size"] // 16) * 16
        # the 16->16 layers keep one slab per image up to B = 256 (_pick_groups(B, 16, 16) = min(B, 256))
        assert all(w["per_image"][1:7]) == (lvl >= 1 and B <= 256) == any(w["per_image"][1:7])
        # the 32->32 stride-1 layers only at level 2
        assert all(w["per_image"][l] for l in (8, 9, 10, 11, 12)) == (lvl == 2 and B <= 256)
        assert not any(w["per_image"][l] for l in (0, 7, 13, 14, 15, 16, 17, 18))
    assert any(not any(w["per_image"]) for i, w in grid if i["batch_size"] == 512)
    assert len({g for _, w in ROWS for g in w["groups"]}) >= 3
    # every field of the plan is pinned: by the table, or (the wiring) by test_wiring_is_the_block_structure
    assert {f.name for f in dataclasses.fields(P.ResNetPlan)} == {
        "B", "Bv", "dp", "groups", "wgrad_branch", "merged_bwd", "sgd_split", "per_image", "fwd_sc", "bwd_sc",
        "sgd_points"}


def test_plan_equals_the_recorded_constructor_decisions():
    for inputs, want in ROWS:
        p = P.plan_resnet_step(**inputs)
        assert p.Bv == inputs["batch_size"] and p.dp == (inputs["world_size"] > 1 or inputs["dp_force"])
        for k, v in want.items():
            g = getattr(p, "groups" if k == "part_rows" else k)
            assert g == v and type(g) is type(v), (inputs, k, g, v)
            assert all(type(x) is type(y) for x, y in zip(g, v)) if isinstance(v, tuple) else True, (inputs, k)


def test_wiring_is_the_block_structure():
    """Forward: layer l applies BN of l - 1, and an even l - 1 >= 2 closes the block that a[l - 3] entered.
    Backward: an odd l opens a block, so its dgrad adds the gradient of the block's output."""
    p = P.plan_resnet_step(batch_size=16)
    assert len(p.fwd_sc) == len(p.bwd_sc) == P.NL == 19
    assert [l for l, (m, _) in enumerate(p.fwd_sc) if m] == list(range(3, 19, 2))
    assert all(src == l - 3 for l, (m, src) in enumerate(p.fwd_sc) if m) and p.fwd_sc[0] == (0, None)
    assert [m for m, _ in p.fwd_sc[3::2]] == [1, 1, 1, 2, 1, 1, 2, 1]      # mode 2 one block after a strided conv
    assert [l for l, m in enumerate(p.bwd_sc) if m] == list(range(1, 18, 2))
    assert [l for l, m in enumerate(p.bwd_sc) if m == 2] == [7, 13]        # the strided convs themselves
    assert p.sgd_points == {13: (13, 19), 7: (7, 13)}
    with pytest.raises(ValueError, match="batch size must be >= 1"):
        P.plan_resnet_step(batch_size=0)
    with pytest.raises(dataclasses.FrozenInstanceError):
        p.merged_bwd = False


@pytest.mark.parametrize("name", sorted(TABLE["launches"]))
def test_engine_issues_the_recorded_launch_sequence(name):
    from dmlc.engine.fused_resnet import FusedResNetEngine
    rec = TABLE["launches"][name]
    kw = dict(TABLE["base_inputs"], **rec["inputs"])
    g = torch.Generator().manual_seed(0)
    data = torch.randint(0, 256, (2048, 32, 32, 3), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (2048,), dtype=torch.int32, generator=g)
    with S.stubbed() as ops:
        eng = FusedResNetEngine(kw.pop("batch_size"), data, labels, device="cpu", **kw)
        got = {}
        del ops.log[:]
        eng._eager_step()
        got["eager_step"] = S.launches(eng, ops.log)
        del ops.log[:]
        eng.compute_gradients(torch.arange(eng.Bv, dtype=torch.int32))
        got["compute_gradients"] = S.launches(eng, ops.log)
    for k, rows in got.items():
        rows = json.loads(json.dumps(rows))
        assert len(rows) == len(rec[k]), (k, len(rows), len(rec[k]))
        for i, (a, b) in enumerate(zip(rows, rec[k])):
            assert a == b, (name, k, i, a, b)
    ops_seen = {r[0] for r in rec["eager_step"]}
    assert {"rn_fwd", "rn_head", "rn_sgd", "rn_wgrad"} <= ops_seen and ops_seen & {"rn_bwd", "rn_dgrad"}


def test_launch_configurations_take_different_paths():
    L = TABLE["launches"]
    assert set(L) == {"b256", "level0", "two_launch", "b512", "sgd_split", "dp_force"}
    count = lambda n, op: sum(r[0] == op for r in L[n]["eager_step"])
    assert count("b256", "rn_bwd") == 18 and count("b256", "rn_dgrad") == 0 and count("b256", "rn_wgrad") == 1
    assert sum(r[0] == "rn_bwd" and r[1][-1] is True for r in L["b256"]["eager_step"]) == 6
    assert not any(r[0] == "rn_bwd" and r[1][-1] for r in L["level0"]["eager_step"])
    assert count("two_launch", "rn_dgrad") == 18 and count("two_launch", "rn_wgrad") == 19
    assert {r[2] for r in L["two_launch"]["eager_step"]} == {"main"}
    assert {r[2] for r in L["b512"]["eager_step"] if r[0] == "rn_wgrad"} == {"s1"} and count("b512", "wait_event") == 19
    assert count("sgd_split", "rn_sgd") == 3
    assert count("dp_force", "rn_sgd") == 2 and count("dp_force", "all_reduce") == 1


def test_plan_imports_without_a_gpu_or_the_extension():
    """plan_resnet.py needs neither torch.cuda nor the native extension: importing it and planning with
    it pulls in neither the extension loader nor an engine."""
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import dmlc; from dmlc.engine import plan_resnet as P\n"
            "p = P.plan_resnet_step(batch_size=100)\n"
            "assert p.B == 112 and p.Bv == 100 and p.merged_bwd and not p.wgrad_branch\n"
            "bad = [m for m in sys.modules if m.endswith('ops._ext') or m.endswith('engine.fused') "
            "or m.endswith('engine.fused_resnet') or m.endswith('engine.base')]\n"
            "assert not bad, bad\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code, REPO], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]
