"""`Stepper.capture` keeps Python's garbage collector out of a HIP graph capture (no device needed: torch's capture objects are replaced
by recorders).  A dead model that a reference cycle kept alive returns its C handles in `__del__`, and the library frees their device
memory with hipFree, which is not allowed while a stream is capturing; the collector runs at allocation counts nobody controls, so it
must stay off from the capture's beginning to its end.  (No collection is forced before it: a full one costs tens of milliseconds, a
quarter of a 50-step sampler call.)"""
import gc

import torch

from shapegen_amd.diffusion import Stepper


class _Handle:
    """Stands for a module with C handles: says when it is finalized."""

    def __init__(self, log):
        self.log, self.me = log, self          # a cycle: only the collector frees it

    def __del__(self):
        self.log.append("finalized")


def test_capture_keeps_the_collector_off(monkeypatch):
    log = []

    class FakeGraphContext:
        def __init__(self, graph):
            pass

        def __enter__(self):
            log.append("begin")

        def __exit__(self, *exc):
            log.append("end")
            return False

    monkeypatch.setattr(torch.cuda, "synchronize", lambda: None)
    monkeypatch.setattr(torch.cuda, "CUDAGraph", lambda: object())
    monkeypatch.setattr(torch.cuda, "graph", FakeGraphContext)

    class Dummy:
        graph = None

        def step(self, k, update):
            log.append(("step", gc.isenabled()))
            junk = [[] for _ in range(5000)]               # enough container allocations to trigger the collector if it were on
            del junk

    gc.collect()
    assert gc.isenabled()
    _Handle(log)                                           # dead at once, and unreachable only through its cycle
    assert log == []
    Stepper.capture(Dummy(), 3)
    assert log == ["begin", ("step", False), ("step", False), ("step", False), "end"]       # not finalized inside the capture
    assert gc.isenabled()
    gc.collect()
    assert log[-1] == "finalized"                          # and the steps above would have let the collector reach it

    # an exception inside the capture does not leave the collector off; a collector the caller had switched off stays off
    class Failing(Dummy):
        def step(self, k, update):
            raise RuntimeError("enqueue failed")

    try:
        Stepper.capture(Failing(), 1)
    except RuntimeError:
        pass
    assert gc.isenabled()
    gc.disable()
    try:
        Stepper.capture(Dummy(), 1)
        assert not gc.isenabled()
    finally:
        gc.enable()
