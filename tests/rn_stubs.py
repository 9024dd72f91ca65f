"""CPU stand-ins for building and stepping the fused ResNet-20 engine without a GPU or the native
extension (tests/test_rn_plan.py): a recording op namespace and fake ``torch.cuda`` streams / events.

``stubbed()`` patches ``torch.cuda.Stream``, ``torch.cuda.Event``, ``torch.cuda.current_stream`` and
the ``torch.cuda.stream`` context (a no-op without a device, so the launches could not be attributed
to a stream otherwise), records ``torch.distributed.all_reduce`` instead of running it (the eager
collective of a data-parallel step) and puts a ``RecordingOps`` in place of the engines' lazily loaded
``torch.ops.dmlc``.  Every op call and every stream edge is appended to ``RecordingOps.log``;
``launches`` names each tensor argument by the engine buffer it is.  Nothing here loads a library.
"""
import contextlib
import importlib

import torch
import torch.distributed as dist

_STATE = {"current": None, "n": 0, "log": None}


class FakeStream:
    def __init__(self, device=None, name=None):
        if name is None:
            _STATE["n"] += 1
            name = f"s{_STATE['n']}"
        self.name = name

    def wait_stream(self, other):
        _STATE["log"].append(("wait_stream", [], {}, f"{self.name}<-{other.name}"))

    def wait_event(self, ev):
        _STATE["log"].append(("wait_event", [], {}, f"{self.name}<-{ev.stream}"))


class FakeEvent:
    def __init__(self, *a, **k):
        self.stream = None

    def record(self, stream=None):
        self.stream = (stream or _STATE["current"]).name


@contextlib.contextmanager
def _stream_ctx(s):
    prev = _STATE["current"]
    _STATE["current"] = s
    try:
        yield
    finally:
        _STATE["current"] = prev


class RecordingOps:
    """``ops.<name>(*args, **kwargs)`` records (name, args, kwargs, current stream) and does nothing."""

    def __init__(self):
        self.log = []

    def __getattr__(self, name):
        def call(*args, **kwargs):
            self.log.append((name, list(args), kwargs, _STATE["current"].name))
        return call


@contextlib.contextmanager
def stubbed():
    """Yields the RecordingOps every engine built inside the block launches through."""
    ops = RecordingOps()
    saved = [(torch.cuda, n, getattr(torch.cuda, n)) for n in ("Stream", "Event", "current_stream", "stream")]
    for mod in ("base", "fused", "fused_resnet"):
        try:
            m = importlib.import_module(f"dmlc.engine.{mod}")
        except ImportError:
            continue
        if hasattr(m, "OPS"):
            saved.append((m, "OPS", m.OPS))
            m.OPS = ops
    _STATE.update(current=FakeStream(name="main"), n=0, log=ops.log)
    torch.cuda.Stream, torch.cuda.Event = FakeStream, FakeEvent
    torch.cuda.current_stream = lambda device=None: _STATE["current"]
    torch.cuda.stream = _stream_ctx
    saved.append((dist, "all_reduce", dist.all_reduce))     # the eager collective of a data-parallel step
    dist.all_reduce = lambda t, **k: ops.log.append(("all_reduce", [t], {}, _STATE["current"].name))
    try:
        yield ops
    finally:
        for obj, name, val in saved:
            setattr(obj, name, val)


def _buffer_names(eng):
    """(data_ptr, shape, dtype) -> name of every tensor the engine holds: ``z[3]``, ``stat[7]``, ``master``."""
    names = {}

    def add(t, name):
        if isinstance(t, torch.Tensor) and t.numel():
            names.setdefault((t.data_ptr(), tuple(t.shape), t.dtype), name)

    for k, v in vars(eng).items():
        if isinstance(v, (list, tuple)):
            for i, t in enumerate(v):
                add(t, f"{k}[{i}]")
        else:
            add(v, k)
    for k in ("stat", "red"):
        for i in range(getattr(eng, k).shape[0]):
            add(getattr(eng, k)[i], f"{k}[{i}]")
    return names


def launches(eng, log):
    """``log`` as JSON-able rows [op, [arguments], stream]: tensors by engine buffer name (``?dtype[shape]``
    for one the engine does not hold, e.g. an explicit index list), a list that is a whole engine list as
    ``part[0:19]``."""
    names = _buffer_names(eng)

    def enc(a):
        if isinstance(a, torch.Tensor):
            key = (a.data_ptr(), tuple(a.shape), a.dtype)
            return names.get(key, f"?{str(a.dtype)[6:]}{list(a.shape)}")
        if isinstance(a, (list, tuple)):
            got = [enc(t) for t in a]
            k = str(got[0]).split("[")[0] if got else ""
            return f"{k}[0:{len(got)}]" if got and got == [f"{k}[{i}]" for i in range(len(got))] else got
        return a

    return [[name, [enc(a) for a in args] + [f"{k}={enc(v)}" for k, v in sorted(kwargs.items())], stream]
            for name, args, kwargs, stream in log]
