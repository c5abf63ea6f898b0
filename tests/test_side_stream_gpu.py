"""Every wrapper of tests/side_stream.py's registry with a `stream` that is not
torch's current one (engine.py's stream contract).

(a) The ordering invariant, deterministic: under torch.cuda.stream(A) the entry
    is called with stream=B while a spy stands in for the product library in
    every lsbm_amd module.  Before each *_dev call it checks that the stream
    argument is B and that torch's current stream is B, and raises instead of
    calling through otherwise: a wrongly ordered launch is never made.
(b) Behaviour under a lagging current stream: A holds a long queue of ordinary
    work (engine.fill_splitmix64 over a private buffer), the entry is called
    under torch.cuda.stream(A) with stream=B, and B is synchronised.  A must
    still be busy then: a call given B neither waits for A nor enqueues behind
    it (and a ballast that is too short fails here instead of letting the case
    pass for nothing).  After a full synchronise, when anything wrongly queued
    on A has taken effect, the outputs equal the models' and the same call made
    beforehand on the default stream, to the byte.
(c) The harness on a function that mis-orders on purpose: (b) sees its late
    zero-fill and the spy of (a) rejects it.
"""
import ctypes
import importlib
import os
import pkgutil

import pytest

import side_stream as ss

pytestmark = pytest.mark.gpu

# The ballast on A: BALLAST_REPEATS fills of a private buffer of BALLAST_BYTES.
# Measured with HIP events on an MI355X: 136.5 ms from the first fill to the
# last (4.2 ms to enqueue).  The slowest entry, buffered.BufferedVersion.get,
# takes 9.7 ms warm on an idle device and 26.8 ms from its call to
# B.synchronize() while that ballast runs (sstable.compact 23.4 ms,
# db.Version.get 22.2 ms, every other entry under 8 ms): the ballast outlasts
# it five times over.
BALLAST_BYTES = 1 << 30
BALLAST_REPEATS = 600


class WrongStream(AssertionError):
    pass


def lsbm_modules():
    """The package and every Python module of it."""
    import lsbm_amd
    mods = [lsbm_amd]
    for info in pkgutil.iter_modules(lsbm_amd.__path__):
        if os.path.exists(os.path.join(lsbm_amd.__path__[0], info.name + ".py")):
            mods.append(importlib.import_module("lsbm_amd." + info.name))
    return mods


class Spy:
    """The product library with a check in front of every *_dev function."""

    def __init__(self, torch, real, stream):
        self._torch, self._real, self._want = torch, real, stream.cuda_stream
        self._at = ss.stream_positions()
        self.calls = []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in self._at:
            return fn

        def checked(*args):
            given = args[self._at[name]]
            given = given.value if isinstance(given, ctypes.c_void_p) else given
            current = self._torch.cuda.current_stream().cuda_stream
            if given != self._want or current != self._want:
                raise WrongStream(f"{name}: launch on stream {given} with torch's current stream {current}; "
                                  f"the call was given stream {self._want}")
            self.calls.append(name)
            return fn(*args)
        return checked


def install_spy(torch, monkeypatch, stream):
    """`lib` of every lsbm_amd module (each binds its own name) -> the spy."""
    from lsbm_amd import _lib
    spy = Spy(torch, _lib.lib(), stream)
    patched = 0
    for mod in lsbm_modules():
        if callable(getattr(mod, "lib", None)):
            monkeypatch.setattr(mod, "lib", lambda: spy)
            patched += 1
    assert patched >= 15
    return spy


@pytest.fixture(scope="module")
def ballast_buffer(torch_cuda):
    buf = torch_cuda.empty(BALLAST_BYTES, dtype=torch_cuda.uint8, device="cuda")
    yield buf
    del buf
    torch_cuda.cuda.empty_cache()


def ballast(torch, stream, buf, repeats=BALLAST_REPEATS):
    """A long queue of fills on `stream`; the event behind the last of them."""
    from lsbm_amd import engine
    with torch.cuda.stream(stream):
        for i in range(repeats):
            engine.fill_splitmix64(buf, i)
        done = torch.cuda.Event()
        done.record()
    return done


def two_streams(torch):
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    null = torch.cuda.default_stream().cuda_stream
    assert len({a.cuda_stream, b.cuda_stream, null}) == 3
    return a, b


@pytest.fixture(scope="module")
def side_by_side(torch_cuda, ballast_buffer):
    """(A, B) for the tests under ballast.  HIP spreads its streams over a few
    hardware queues (GPU_MAX_HW_QUEUES), and two streams that share one run
    one after the other whatever a wrapper does; which of torch's pooled
    streams share one depends on what ran before.  So: the first pair of
    torch.cuda.Stream()s on which one small fill on B overtakes the ballast
    on A.  Every test still asserts that its own call overtook it."""
    from lsbm_amd import engine
    torch = torch_cuda
    probe = torch.empty(4096, dtype=torch.uint8, device="cuda")
    for _ in range(8):
        a, b = two_streams(torch)
        busy = ballast(torch, a, ballast_buffer)
        engine.fill_splitmix64(probe, 1, stream=b)
        b.synchronize()
        overtook = not busy.query()
        torch.cuda.synchronize()
        if overtook:
            return a, b
    pytest.fail("no two of torch's streams ran side by side")


@pytest.mark.parametrize("name", sorted(ss.REGISTRY))
def test_every_launch_is_on_the_given_stream(torch_cuda, monkeypatch, name):
    torch = torch_cuda
    e = ss.REGISTRY[name]
    x = e.make(torch)
    torch.cuda.synchronize()
    a, b = two_streams(torch)
    spy = install_spy(torch, monkeypatch, b)
    with torch.cuda.stream(a):
        e.call(x, b)
    torch.cuda.synchronize()
    assert spy.calls, "the entry reached no *_dev function"


@pytest.mark.parametrize("name", sorted(ss.REGISTRY))
def test_given_stream_while_the_current_stream_lags(torch_cuda, ballast_buffer, side_by_side, name):
    torch = torch_cuda
    e = ss.REGISTRY[name]
    want = e.want()
    read = e.call(e.make(torch), None)  # on the default stream: the reference, and the allocator is warm
    torch.cuda.synchronize()
    reference = read()
    x = e.make(torch)
    torch.cuda.synchronize()
    a, b = side_by_side
    busy = ballast(torch, a, ballast_buffer)
    with torch.cuda.stream(a):
        read = e.call(x, b)
    b.synchronize()
    assert not busy.query(), "the call waited for the current stream, or the ballast is too short"
    torch.cuda.synchronize()
    got = read()
    ss.assert_same(got, want, "against the models")
    ss.assert_same(got, reference, "against the default stream")


def misordered_fill(torch, n, seed, stream):
    """What the wrappers did before engine.on_stream: the output zero-filled on
    torch's current stream, the kernel launched on `stream` (on_stream is
    stepped around on purpose).  Both write inside `buf` only."""
    from lsbm_amd import engine
    buf = torch.zeros(n, dtype=torch.uint8, device="cuda")
    return engine.fill_splitmix64.__wrapped__(buf, seed, stream=stream)


def test_the_harness_sees_a_late_fill_and_the_spy_rejects_it(torch_cuda, ballast_buffer, side_by_side, monkeypatch):
    torch = torch_cuda
    n, seed = 4096, 99
    want = ss.crc().fill_splitmix64(0, n, seed).tobytes()
    ordered = misordered_fill(torch, n, seed, None)
    torch.cuda.synchronize()
    assert ss.byts(ordered) == want and any(want)
    a, b = side_by_side
    busy = ballast(torch, a, ballast_buffer)
    with torch.cuda.stream(a):
        buf = misordered_fill(torch, n, seed, b)
    b.synchronize()
    assert not busy.query()
    torch.cuda.synchronize()
    assert ss.byts(buf) == bytes(n), "the zero-fill on the lagging stream landed after the kernel"
    spy = install_spy(torch, monkeypatch, b)
    with torch.cuda.stream(a):
        with pytest.raises(WrongStream, match="lsbm_fill_splitmix64_dev"):
            misordered_fill(torch, n, seed, b)
    torch.cuda.synchronize()
    assert not spy.calls
