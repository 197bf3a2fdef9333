"""The peak catalogue under the stream contract that tests/test_gpu_streams.py pins for the other
sub-handles: a run queued on a user stream behind other work, a switch to a second stream, and only then the counts and
the read -- the bytes of the same calls on one stream."""
import numpy as np
import pytest

import catalogue_np as K
from slicer_amd import lensing
from stream_util import Delay, Scope, still_busy

pytestmark = pytest.mark.gpu

N = 65


def _map(seed):
    return np.random.default_rng(seed).standard_normal((N, N)).astype(np.float32)


def test_switch_keeps_order_catalogue_read_on_the_new_stream():
    x = _map(1)
    want = K.catalogue(x, 3, -0.5, 0.5)
    with Scope() as sc:
        A, B, S = sc.stream(nonblocking=True), sc.stream(nonblocking=True), sc.slicer()
        delay = sc.sub(Delay(S))
        d, d_other = sc.device(S, x), sc.device(S, _map(2))
        cat = sc.sub(lensing.PeakCatalogue(S, N, N * N // 2))
        cat.run(d_other, kinds=3)  # the result buffers hold the catalogue of another map
        assert cat.counts()["stored"] != len(want)
        S.set_stream(A.ptr)
        delay.queue()
        cat.run(d, kinds=3, min_peak=-0.5, max_minimum=0.5)
        S.set_stream(B.ptr)
        still_busy(A, "set_stream, before the read of the catalogue")
        c = cat.counts()
        got = cat.read()
        d_rec, d_cnt = cat.device_records()
        on_device = S.to_host(d_cnt, (3,), np.int64)
    assert (c["peaks"], c["minima"]) == K.totals(want) and c["stored"] == len(want)
    assert list(on_device) == [c["peaks"], c["minima"], c["stored"]]
    assert got.tobytes() == want.tobytes()
