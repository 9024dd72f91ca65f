"""The fused engine's path selection (engine/plan.py) against a table recorded from the constructor
that made these decisions inline, before they moved into ``plan_step``.

tests/plan_table.json was dumped from that constructor, run without a GPU under stubs (a mock op
namespace, fake tensors, patched ``torch.cuda`` properties and environment), for a grid of batch
sizes, dtypes, topologies, wires, environment switches, variants and explicit overrides.  Every
expected value is what that constructor decided or allocated -- none comes from ``plan_step``.
Format: ``rows`` = [input overrides over ``base_inputs``, the ``bool_fields`` as a 0/1 string, the
``int_fields``]; the recorded ``variant`` was ``variant_defaults`` plus the row's overrides in every
row.  ``has_w2f8`` / ``has_p1f8`` record whether the fp8 buffers existed (the plan's ``fp8`` /
``fp8_wgrad``); ``has_grad16`` / ``has_h1part8`` / ``*_words`` / ``loss_parts`` the other buffers.
"""
import dataclasses
import json
import os
import re
import subprocess
import sys

import pytest

from dmlc.engine import plan as P

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

with open(os.path.join(HERE, "plan_table.json")) as f:
    TABLE = json.load(f)
BUFFER_FIELDS = {"has_w2f8": "fp8", "has_p1f8": "fp8_wgrad"}     # recorded buffer -> the plan field sizing it


def _rows():
    for over, bits, ints in TABLE["rows"]:
        inputs = dict(TABLE["base_inputs"], **over)
        want = {k: c == "1" for k, c in zip(TABLE["bool_fields"], bits)}
        want.update(zip(TABLE["int_fields"], ints))
        want["variant"] = dict(TABLE["variant_defaults"], **(inputs["variant"] or {}))
        yield inputs, want


ROWS = list(_rows())


def test_table_covers_the_plan():
    """The table names every StepPlan field (so a new field cannot go unpinned) and is not vacuous:
    every boolean is True somewhere and False somewhere, every listed choice takes two values."""
    fields = {f.name for f in dataclasses.fields(P.StepPlan)}
    recorded = set(TABLE["bool_fields"]) | set(TABLE["int_fields"]) | {"variant"}
    assert recorded - set(BUFFER_FIELDS) == fields
    assert TABLE["variant_defaults"] == P.VARIANT_DEFAULTS
    assert len(ROWS) >= 300
    for k in TABLE["bool_fields"]:
        assert {w[k] for _, w in ROWS} == {False, True}, k
    for k in ("conv_split", "dgrad_split", "conv1_split", "head_rows", "fc1_split", "_comm_blocks"):
        assert len({w[k] for _, w in ROWS}) >= 2, k
    # the grid the table was asked to span
    assert {i["batch_size"] for i, _ in ROWS} >= {1, 8, 16, 32, 64, 96, 112, 128, 130, 144, 160, 192, 224, 256, 272,
                                                  512, 1024}
    assert {i["dtype"] for i, _ in ROWS} == {"bf16", "fp8"} and {i["comm_dtype"] for i, _ in ROWS} == {"fp32", "bf16"}
    assert {(i["world_size"], i["ndev"]) for i, _ in ROWS} >= {(1, 8), (2, 8), (2, 1)}
    assert any(i["dp_force"] and i["have_xgmi"] and i["world_size"] == 1 for i, _ in ROWS)
    for sw in ("DMLC_FC_FUSED", "DMLC_WGRAD_SGD", "DMLC_FWD12_SPLIT"):
        assert any(i["env"].get(sw) == "0" for i, _ in ROWS), sw
    for key in P.VARIANT_DEFAULTS:
        for b in (128, 256):
            assert {i["variant"][key] for i, _ in ROWS
                    if i["batch_size"] == b and i["variant"] and key in i["variant"]} == {False, True}, (key, b)
    assert any(i["conv_split"] == 2 and i["conv1_split"] == 4 for i, _ in ROWS)


def test_plan_equals_the_recorded_constructor_decisions():
    for inputs, want in ROWS:
        got = dataclasses.asdict(P.plan_step(**inputs))
        for k, v in want.items():
            g = got[BUFFER_FIELDS.get(k, k)]
            assert g == v and type(g) is type(v), (inputs, k, g, v)


def test_plan_reads_only_the_env_it_is_given(monkeypatch):
    """The switches come from the ``env`` mapping, not from the process environment (and
    LOCAL_WORLD_SIZE is the caller's to read: ``local_world``)."""
    kw = dict(TABLE["base_inputs"])
    for k in ("DMLC_FC_FUSED", "DMLC_WGRAD_SGD", "DMLC_FWD12_SPLIT"):
        monkeypatch.setenv(k, "0")
    monkeypatch.setenv("LOCAL_WORLD_SIZE", "64")
    on = P.plan_step(**kw)
    assert on.fc_fused and on.wgrad_apply and on.bwd_fused and on._comm_blocks == 512
    kw.pop("env")
    off = P.plan_step(**kw)              # default: os.environ
    assert not off.fc_fused and not off.wgrad_apply and off._comm_blocks == 512


def test_invalid_configurations_raise():
    kw = dict(TABLE["base_inputs"])
    with pytest.raises(ValueError, match=r"unknown engine variant keys \['nope'\]"):
        P.plan_step(**dict(kw, variant={"nope": 1}))
    for bad in (dict(conv_split=3), dict(dgrad_split=4), dict(conv1_split=3), dict(conv_split=2, conv1_split=8)):
        with pytest.raises(ValueError, match="conv_split / dgrad_split must be 1 or 2 and conv1_split 2 or 4"):
            P.plan_step(**dict(kw, **bad))
    with pytest.raises(ValueError, match="fused engine dtype must be bf16 or fp8"):
        P.plan_step(**dict(kw, dtype="fp32"))
    with pytest.raises(ValueError, match="batch size must be >= 1"):
        P.plan_step(**dict(kw, batch_size=0))
    with pytest.raises(dataclasses.FrozenInstanceError):
        P.plan_step(**kw).bwd_fused = False


def test_plan_imports_without_a_gpu_or_the_extension():
    """plan.py needs neither torch.cuda nor the native extension: importing it and planning with it
    pulls in neither torch, the extension loader nor the engine."""
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import dmlc; from dmlc.engine import plan as P\n"
            "p = P.plan_step(batch_size=130, dtype='bf16', world_size=1, dp_force=False, local_world=1, ndev=1, "
            "cus=256, have_xgmi=False, comm_dtype='fp32', env={})\n"
            "assert p.B == 144 and p.bwd_fused\n"
            "bad = [m for m in sys.modules if m.endswith('ops._ext') or m.endswith('engine.fused') "
            "or m.split('.')[0] == 'torch']\n"
            "assert not bad, bad\n"
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code, REPO], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]


def test_word_constants_match_the_kernel_header():
    with open(os.path.join(REPO, "csrc", "kernels", "api.h")) as f:
        text = f.read()

    def macro(name):
        m = re.search(r"^#define %s \(([0-9* ]+)\)$" % name, text, re.M)
        assert m, name
        n = 1
        for x in m.group(1).split("*"):
            n *= int(x)
        return n

    from dmlc.engine import fused as F
    for name, attr in (("DMLC_TICKET_WORDS", "TICKET_WORDS"), ("DMLC_WBAR_WORDS", "WBAR_WORDS"),
                       ("DMLC_HAND_WORDS", "HAND_WORDS"), ("DMLC_WBAR_ERR", "ERR_WORD"),
                       ("DMLC_FC_SYNC_WORDS", "FC_SYNC_WORDS")):
        assert macro(name) == getattr(P, attr) == getattr(F, attr), name
    assert P.ERR_WORD < P.WBAR_WORDS
    # fused.py keeps exporting what the resnet engine, the tools and the tests import from it
    for name in ("VARIANT_DEFAULTS", "head_rows", "BUF_NAMES", "SEG_OFF"):
        assert hasattr(F, name), name
    assert F.VARIANT_DEFAULTS is P.VARIANT_DEFAULTS and F.head_rows is P.head_rows
