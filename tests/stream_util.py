"""What tests/test_gpu_streams.py shares: HIP streams through the runtime that libslicer_amd.so links, and the delay job
that keeps one of them busy while the next call is made."""
import contextlib
import ctypes as C

import numpy as np

import slicer_amd
from slicer_amd import _lib, lensing

_L = _lib.load()  # (dlsym on the product library also finds the symbols of the HIP runtime it depends on)
HIP_STREAM_NON_BLOCKING = 1
HIP_ERROR_NOT_READY = 600

for _name, _args in (("hipStreamCreateWithFlags", [C.POINTER(C.c_void_p), C.c_uint]), ("hipStreamQuery", [C.c_void_p]),
                     ("hipStreamSynchronize", [C.c_void_p]), ("hipStreamDestroy", [C.c_void_p])):
    getattr(_L, _name).restype = C.c_int
    getattr(_L, _name).argtypes = _args


class Stream:
    """One hipStream_t: blocking (hipStreamCreate's kind) unless nonblocking; `ptr` is what Slicer.set_stream takes."""

    def __init__(self, nonblocking=False):
        p = C.c_void_p()
        rc = _L.hipStreamCreateWithFlags(C.byref(p), HIP_STREAM_NON_BLOCKING if nonblocking else 0)
        assert rc == 0 and p.value, f"hipStreamCreateWithFlags: {rc}"
        self.ptr = p.value

    def busy(self):
        """hipStreamQuery: True for "not ready", False for an idle stream; anything else is an error."""
        rc = _L.hipStreamQuery(C.c_void_p(self.ptr))
        assert rc in (0, HIP_ERROR_NOT_READY), f"hipStreamQuery: {rc}"
        return rc == HIP_ERROR_NOT_READY

    def synchronize(self):
        rc = _L.hipStreamSynchronize(C.c_void_p(self.ptr))
        assert rc == 0, f"hipStreamSynchronize: {rc}"

    def close(self):
        if self.ptr:
            self.synchronize()
            _L.hipStreamDestroy(C.c_void_p(self.ptr))
            self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


DELAY_NPIX = 2048
DELAY_RUNS = 200


class Delay:
    """The delay job: DELAY_RUNS runs of a Smooth of kind "map" at radius 128 (sigma 32, truncated at 4 sigma) on a
    DELAY_NPIX^2 map of its own, queued on whatever stream the handle S works on when queue() is called.  Everything it
    needs is allocated, uploaded and waited for here, so queue() itself only launches kernels.

    Measured on an MI355X: 81 ms on the device, under 1 ms of host time to queue; the consumers it has to outlast take
    the host 0.02-0.9 ms (figures in the docstring of tests/test_gpu_streams.py)."""

    def __init__(self, S, runs=DELAY_RUNS):
        self.S, self.runs = S, runs
        self.smooth = lensing.Smooth(S, DELAY_NPIX, "map", 32.0, 4.0)
        assert self.smooth.radius == 128
        rng = np.random.default_rng(5)
        self.d_map = S.to_device(rng.standard_normal((DELAY_NPIX, DELAY_NPIX)).astype(np.float32))
        self.smooth.run(self.d_map)  # (first launch: code objects loaded, the LDS limit raised)
        S.synchronize()

    def queue(self):
        for _ in range(self.runs):
            self.smooth.run(self.d_map)

    def close(self):
        if self.smooth is not None:
            self.S.synchronize()
            self.smooth.close()
            self.S.free(self.d_map)
            self.smooth = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def still_busy(stream, what):
    """The premise of an ordering test: the delayed stream has not drained when the consumer call has returned.  Without
    it the test would pass on any library, ordered or not."""
    assert stream.busy(), (f"the delay is too short: its stream was already idle after {what}, so this test proves "
                           "nothing about ordering -- raise stream_util.DELAY_RUNS")


class Scope(contextlib.ExitStack):
    """Streams, handles, sub-handles and device buffers of one test, released in reverse order whether it passes or
    fails: sub-handles before their Slicer, every Slicer while the streams it was set to still exist."""

    def __init__(self):
        super().__init__()
        self._streams = []

    def __exit__(self, *exc):
        for st in self._streams:  # nothing is released under work that is still queued, whatever the test found
            st.synchronize()
        return super().__exit__(*exc)

    def stream(self, nonblocking=False):
        self._streams.append(self.enter_context(Stream(nonblocking)))
        return self._streams[-1]

    def slicer(self, max_chunk=1 << 20):
        return self.enter_context(slicer_amd.Slicer(0, max_chunk=max_chunk))

    def sub(self, x):
        return self.enter_context(x)

    def device(self, S, arr):
        p = S.to_device(arr)
        self.callback(S.free, p)
        return p
