"""A caller's own stream for the GPU tests, and the proof that a call was enqueued behind it (plain module).

The rest of the GPU suite runs on the legacy default stream, where the runtime orders everything.  A
scan owns its streams, and those do not synchronise with the default stream.  This module provides

`side_stream(i)`  a stream created with hipStreamCreateWithFlags(hipStreamNonBlocking) through ctypes
    and wrapped in torch.cuda.ExternalStream (streams 0 and 1 are made once per process and kept).
    torch's own pool streams are documented as non-blocking, but the torch build the suite runs with
    ships no C++ source to confirm it from (c10/cuda/CUDAStream.cpp is not in the wheel), so the
    stream is created here and its flag read back with hipStreamGetFlags.
`hold(stream, delay)`  enqueues a device-side delay (torch.cuda._sleep) on `stream` and returns an
    event recorded right after it.
`held(event)`  `not event.query()`: called directly after an engine call has returned on the host
    and before anything synchronises.  True means every launch of that call was enqueued while the
    stream was still blocked, so whatever the engine issued on another stream ran BEFORE its
    producers.  Without it a fast GPU drains the stream ahead of the host and the test degenerates
    into the default-stream test.
`calibrate(stream, ms)`  the `cycles` argument of torch.cuda._sleep that lasts `ms` on this device,
    from two events around trial sleeps (once per test module, from a module-scoped fixture).
`HeldContext(ctx, delay, table)`  stands in for a vortex_amd Context in the bindings and test
    helpers: every C entry point that takes a stream is called as hold -> call -> held, its host
    time is measured, and `check(kind, at)` then holds every call of an asynchronous row of `table`
    to `held`.  With delay=None nothing is held and only the host times are taken (`slowest()`):
    that is how the delay below was measured.

How long the delay is.  The longest host time of one asynchronous engine call over the selection of
tests/test_gpu_streams.py (every tree seed, batch seed and entry-point case; one warm pass on the
default stream, the maximum over the seeds) was measured on an MI355X as 0.505 ms
(MEASURED_ENQUEUE_MS: vxg_row_filter of tree seed 58; then vxg_plan_launch of eight trees 0.445 ms,
vxg_take_array_ex 0.277 ms, vxg_compare_scalar 0.274 ms, vxg_canonicalize 0.245 ms, every
per-encoding kernel under 0.24 ms).  The machines are shared and a command gets 16 CPUs, so host
jitter is large against a launch: MARGIN = 4, and DELAY_MS = 4 * 0.505 = 2.02, rounded up to 2.1 ms.
The assertion on `held` is the condition; the delay is only what makes it hold.

Figures so far: with tests/test_gpu_streams.py run alone every held call of an asynchronous row (about
10 000) returned inside the delay.  In one run of the whole GPU suite one of them did not: a
vxg_take_array_ex of tree seed 62 took 1.932 ms on the host (0.277 ms at most when measured) against
the 2.1 ms delay, and test_take[62] failed on `held`; its bytes were never in question.  The margin
is the stated 4 and was not widened for it.
"""
import ctypes as C
import time

MEASURED_ENQUEUE_MS = 0.505  # vxg_row_filter of tree seed 58, both bounds unpaired (next: vxg_plan_launch 0.445, eight trees)
MARGIN = 4
DELAY_MS = 2.1               # MARGIN * MEASURED_ENQUEUE_MS = 2.02, rounded up

HIP_STREAM_NON_BLOCKING = 0x01
_STREAMS: dict = {}
_HIP = None


def _hip():
    global _HIP
    if _HIP is None:
        import torch  # (loads the HIP runtime the process uses; the same library is opened again by name)
        torch.cuda.init()
        _HIP = C.CDLL("libamdhip64.so")
    return _HIP


def side_stream(i: int = 0, device: int = 0):
    """Stream `i` of this process that does not synchronise with the default stream."""
    import torch
    if (i, device) not in _STREAMS:
        hip = _hip()
        with torch.cuda.device(device):
            s = C.c_void_p()
            err = hip.hipStreamCreateWithFlags(C.byref(s), C.c_uint(HIP_STREAM_NON_BLOCKING))
            assert err == 0 and s.value, f"hipStreamCreateWithFlags: error {err}"
            flags = C.c_uint(0)
            err = hip.hipStreamGetFlags(s, C.byref(flags))
            assert err == 0 and flags.value & HIP_STREAM_NON_BLOCKING, (err, flags.value)
        _STREAMS[(i, device)] = torch.cuda.ExternalStream(s.value, device=device)
    return _STREAMS[(i, device)]


class Delay:
    """A device-side delay of `ms` milliseconds: `cycles` of torch.cuda._sleep on this device."""

    def __init__(self, cycles: int, ms: float):
        self.cycles, self.ms = int(cycles), float(ms)

    def __repr__(self):
        return f"Delay({self.ms:.3f} ms = {self.cycles} cycles)"


def calibrate(stream, ms: float) -> Delay:
    """The torch.cuda._sleep cycles that keep `stream` busy for `ms`, from two events around a trial
    sleep that is doubled until it lasts at least a millisecond (so the launch does not weigh)."""
    import torch
    assert ms > 0
    with torch.cuda.stream(stream):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1000)  # (the kernel is loaded)
        stream.synchronize()
        trial, took = 50_000, 0.0
        for _ in range(24):
            e0.record(stream)
            torch.cuda._sleep(trial)
            e1.record(stream)
            e1.synchronize()
            took = e0.elapsed_time(e1)
            if took >= 1.0:
                break
            trial *= 2
        assert took >= 1.0, f"torch.cuda._sleep({trial}) lasted {took} ms"
    return Delay(max(1, round(trial * ms / took)), ms)


def hold(stream, delay: Delay):
    """Block `stream` on the device for `delay`; -> the event recorded right after the delay."""
    import torch
    with torch.cuda.stream(stream):
        torch.cuda._sleep(delay.cycles)
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


def held(event) -> bool:
    """The delay has not run out yet: everything enqueued since `hold` is still behind it."""
    return not event.query()


class _HeldLib:
    """The engine library with every stream-taking entry point called as hold -> call -> held."""

    def __init__(self, lib, owner):
        self._lib, self._owner = lib, owner

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in self._owner.table:
            return fn
        owner = self._owner

        def call(*args):
            import torch
            stream = torch.cuda.current_stream(owner.device)
            ev = hold(stream, owner.delay) if owner.delay is not None else None
            t0 = time.perf_counter()
            status = fn(*args)
            ms = (time.perf_counter() - t0) * 1e3
            owner.calls.append((name, ev is None or held(ev), ms))
            return status

        return call


class HeldContext:
    """A vortex_amd Context whose stream-taking C calls are held (see the module's docstring).
    `table`: entry point -> {kind: asynchronous?}; an entry point that is not in it is called as it is."""

    def __init__(self, ctx, delay, table: dict):
        self._ctx, self.delay, self.table = ctx, delay, table
        self.lib = _HeldLib(ctx.lib, self)
        self.calls: list = []   # (entry point, held, host ms) since the last check()

    def __getattr__(self, name):  # handle, device, stream_ptr, sync, ...
        return getattr(self._ctx, name)

    def check(self, kind: str, at: str, expect=None) -> int:
        """Every call since the last check: one of an asynchronous row must have been held.  `expect`:
        entry points of which at least one call must have been seen.  -> the number of calls."""
        calls, self.calls = self.calls, []
        seen = {name for name, _, _ in calls}
        for name in expect or ():
            assert name in seen, f"{name} was not called, {at}"
        for name, was_held, ms in calls:
            if self.table[name][kind]:
                assert was_held, (f"{name} ({kind}) was not enqueued behind the delay: the call took {ms:.3f} ms on the "
                                  f"host against a delay of {self.delay.ms:.3f} ms, {at}")
        return len(calls)

    def slowest(self, kind: str) -> list:
        """(host ms, entry point) of the calls of asynchronous rows since the last check, slowest first."""
        calls, self.calls = self.calls, []
        return sorted(((ms, name) for name, _, ms in calls if self.table[name][kind]), reverse=True)
