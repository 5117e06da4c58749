"""A harness for the tests of mlp.DEFER_WGRAD_SYNC (tests/test_gpu_mlp.py, tests/test_gpu_train.py): the merged
layer-0 weight gradient [dW_0 ; dW_s,x] -- the side-stream work whose wait the deferral moves to the end of the whole
backward -- made late on purpose.  mlp.wgrad is looked up as a module global, so a wrapper in its place sees the
merged call (n == 2 W), fills its outputs with NaN on the current (side) stream, spins the device for a bounded time
and only then runs the real kernel: a reader on the caller's stream that does not wait for the side stream is then
certain to run first and to read NaN, in one run, where the undelayed race would mostly go unseen.

The delay is a harness parameter, not a tolerance: three times the scenario's own measured time, at most 100 ms."""
import importlib

import torch

mlp = importlib.import_module("a-nerf_amd.mlp")

REAL_WGRAD = mlp.wgrad
REAL_DEFER_OK = mlp.defer_wgrad_sync_ok
MAX_DELAY_MS = 100.0
_CYCLES_PER_MS = []


def cycles_per_ms():
    """torch.cuda._sleep's cycles per millisecond on this device: one fixed spin between two events, measured once
    per process (the spin is linear in its argument)."""
    if not _CYCLES_PER_MS:
        n = 2_000_000
        torch.cuda._sleep(n)  # (the kernel's first launch loads its code object)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        torch.cuda._sleep(n)
        b.record()
        b.synchronize()
        _CYCLES_PER_MS.append(n / max(a.elapsed_time(b), 1e-3))
    return _CYCLES_PER_MS[0]


def delay_cycles(t_ms):
    """The spin for a scenario that takes t_ms undelayed: 3 t_ms, at most MAX_DELAY_MS."""
    return int(min(3.0 * t_ms, MAX_DELAY_MS) * cycles_per_ms())


def timed_ms(fn):
    """(fn(), the milliseconds its work took on the current stream)."""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b)


def record_decisions(monkeypatch):
    """The list that every call of mlp.defer_wgrad_sync_ok (one per _MLP backward with late gradients while
    DEFER_WGRAD_SYNC is on) appends its answer to."""
    seen = []

    def defer_wgrad_sync_ok(late, application):
        seen.append(REAL_DEFER_OK(late, application))
        return seen[-1]

    monkeypatch.setattr(mlp, "defer_wgrad_sync_ok", defer_wgrad_sync_ok)
    return seen


def patch_wgrad(monkeypatch, W, cycles):
    """mlp.wgrad replaced by the wrapper described above (cycles > 0: NaN fill + spin before the merged call; 0: the
    merged calls are only counted).  Returns the one-element list that counts the merged calls: a test asserts it
    equals the number of _MLP applications in its backward, so it cannot pass because the merged path was not taken."""
    calls = [0]

    def wgrad(m, n, k, dy, x, dw, db, ws, dev, prec=6):
        if n == 2 * W:
            calls[0] += 1
            if cycles:
                dw.fill_(float("nan"))
                db.fill_(float("nan"))
                torch.cuda._sleep(cycles)
        return REAL_WGRAD(m, n, k, dy, x, dw, db, ws, dev, prec)

    monkeypatch.setattr(mlp, "wgrad", wgrad)
    return calls
