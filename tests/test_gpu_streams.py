"""The stream contract of include/slicer_amd.h (slicer_set_stream): user streams, switches, sub-handles.

Every other GPU test works on the handle's own stream; a dependency missing between two streams cannot show there.
Here a stream is kept busy by the delay job (stream_util.Delay), the next call is made while it still runs, and whatever
that call could read too early holds known, different values beforehand (zeros, maps or tables of other inputs), so a
missing dependency shows as wrong numbers.  Each such test asserts its premise (stream_util.still_busy): the delayed
stream has not drained when the consumer call has returned.  A consumer that itself waits for the stream (a read) can
only have the premise checked directly before it: behind a correct wait the stream is idle by construction.

DELAY FIGURES, measured on an MI355X: the delay job (200 runs of Smooth "map", radius 128, on a 2048^2 map) keeps its
stream busy for 81 ms; queueing it takes the host under 1 ms.  The consumers it has to outlast, host time from the
delay being queued to the premise check: a whole pass enqueued (plane_begin ... file_end of 100000 device-resident
particles, with synth_positions) 0.9 ms; a sub-handle's create 0.01 ms, switch + run 0.02-0.1 ms; the reads return
81-82 ms after the delay was queued, i.e. behind it.  An earlier sizing (150 runs on 1024^2) gave 18 ms.

AGAINST A set_stream THAT ORDERS NOTHING (this library with the event record / wait taken out), on the same hardware,
every premise held and these failed on values: root handle kappa (blocking and non-blocking A) and plane_read
(non-blocking A); created-on-the-old-stream smooth_gauss, smooth_map, peaks, minkowski, betti, l1norm and kappa (kappa
came out at exactly twice the expected map: its add landed on what the decoy had left in the memory, before the queued
zero-fill; with a decoy that left zeros it had passed there, hence the decoy's add); read-on-the-new-stream all eight
modules.  These passed, for a reason: plane_read with a blocking A (its hipMemcpy runs on the legacy
default stream, which HIP orders behind every blocking stream); test 3 (one stream orders everything); created-on-the-
old-stream power (the control: its create waits).  So a pageable-host hipMemcpyAsync does NOT hold the host until the
stream drains here: the creates of Smooth, Peaks, Minkowski, L1Norm, Betti return at once with A still busy.
The staging events of deposit_host (stage_free, recorded on the caller's stream) showed nothing wrong: the same bits
on the own, a blocking and a non-blocking stream, and with two handles interleaved on two streams.

Every test makes its own Slicer, so a stream left set cannot reach another test; at most two handles and four streams
live at once.
"""
import numpy as np
import pytest

import slicer_amd
from slicer_amd import api, lensing, parallel, synth
from stream_util import Delay, Scope, still_busy
from test_gpu_parity import BOX, RND, one_type_file, run_gpu, run_oracle

pytestmark = pytest.mark.gpu
_L = api._L

NPIX, FOV, LD, LD2 = 128, 0.25, 3.0, 4.0
NPART = 100000
OTHER_SEED = 0xBEEF


@pytest.fixture(scope="module")
def particles():
    """The one file of the passes here and the oracle's maps of it, computed once and left unchanged."""
    f = one_type_file(NPART)
    ngp, _, nsel = run_oracle([f], NPIX, FOV, LD, LD2, ngp=True)
    ngp.setflags(write=False)
    return dict(file=f, ngp=ngp, nsel=nsel)


def enqueue_pass(S, d_pos, n, ngp=True, accum=slicer_amd.ACC_F32, first_type=1, m=0.0123):
    """plane_begin ... plane_finalize of one file of n device-resident particles: nothing here waits for the stream."""
    S.plane_begin(NPIX, FOV, [LD], [LD2], mas=slicer_amd.MAS_NGP if ngp else slicer_amd.MAS_TSC, accum=accum)
    npart, massarr = [0] * 6, [0.0] * 6
    npart[first_type], massarr[first_type] = n, m
    S.file_begin(npart, massarr, BOX, RND["sgn"], RND["face"], RND["center"], RND["rcase"])
    S.deposit_device(first_type, d_pos, n)
    S.file_end()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def same_bits(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a)
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return a.shape == b.shape and np.array_equal(bits(a), bits(b))
    return np.array_equal(a, b)


# ---- 1. the contract in words --------------------------------------------------------------------------------------
def test_contract_in_words():
    with Scope() as sc:
        U, S = sc.stream(), sc.slicer()
        own = S.get_stream()
        assert own and S.on_own_stream()
        S.set_stream(U.ptr)
        assert S.get_stream() == U.ptr and not S.on_own_stream()
        S.set_stream(None)
        assert S.get_stream() == own and S.on_own_stream()
        assert _L.slicer_set_stream(None, None) == 2  # SLICER_ERR_ARG

        def refused():
            with pytest.raises(slicer_amd.SlicerError) as e:
                S.set_stream(U.ptr)
            assert e.value.code == 3 and "plane pass" in str(e.value)  # SLICER_ERR_STATE
            assert S.get_stream() == own

        pos = synth.positions(0, 1000, BOX)
        S.plane_begin(16, FOV, [LD], [LD2], mas=slicer_amd.MAS_NGP)
        refused()  # in the pass, no file open
        S.file_begin([0, 1000, 0, 0, 0, 0], [0, 1.0, 0, 0, 0, 0], BOX, RND["sgn"], RND["face"], RND["center"], RND["rcase"])
        refused()  # ... with a file open
        S.deposit_host(1, pos)
        refused()
        S.file_end()
        refused()  # ... and between the last file and plane_finalize
        S.plane_finalize()
        S.set_stream(U.ptr)  # accepted from plane_finalize on
        assert S.get_stream() == U.ptr
        tot, _, cnt = S.plane_read(0)
        assert cnt[1] > 0 and tot.sum() > 0
        S.set_stream(None)  # accepted after plane_read
        assert S.get_stream() == own

        # a pass that ends in SLICER_ERR_NEGATIVE_COORD is over as well
        S.plane_begin(8, 1.0, [0.0], [1.0])
        S.file_begin([0, 2, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], BOX, (1, 1, 1), 1, (0, 0, 0), 0.0)
        S.deposit_host(1, np.array([[500, 500, 500], [-2600, 500, 500]], np.float32))
        S.file_end()
        with pytest.raises(slicer_amd.SlicerError) as e:
            S.plane_read(0)
        assert e.value.code == slicer_amd.api.ERR_NEGATIVE_COORD
        S.set_stream(U.ptr)
        assert S.get_stream() == U.ptr
        S.set_stream(None)


# ---- 2. same bits on any stream ------------------------------------------------------------------------------------
def _stream_kinds():
    return [("own", None), ("blocking", False), ("nonblocking", True)]


def test_same_bits_on_any_stream(particles):
    """The passes of test_gpu_parity.run_gpu on the handle's own stream, a blocking and a non-blocking user stream:
    NGP equals the oracle bit for bit and FIXED64 TSC is the same bits on all three, through deposit_host in 7 staging
    chunks of 16384 (both slots and their stage_free events reused on the caller's stream) and through deposit_device."""
    f = particles["file"]
    tsc = {}
    for kind, nonblocking in _stream_kinds():
        with Scope() as sc:
            U = None if nonblocking is None else sc.stream(nonblocking)
            S = sc.slicer(max_chunk=16384)
            if U:
                S.set_stream(U.ptr)
            for resident in (False, True):
                (tot, _, cnt), = run_gpu(S, [f], NPIX, FOV, [LD], [LD2], ngp=True, device_resident=resident)
                assert np.array_equal(cnt, particles["nsel"]), (kind, resident)
                assert np.array_equal(bits(tot), bits(particles["ngp"])), (kind, resident)
                (tot, _, _), = run_gpu(S, [f], NPIX, FOV, [LD], [LD2], accum=slicer_amd.ACC_FIXED64,
                                       device_resident=resident)
                tsc[kind, resident] = tot
    ref = tsc["own", False]
    assert ref.sum() > 0
    for key, tot in tsc.items():
        assert np.array_equal(bits(tot), bits(ref)), key


@pytest.mark.parametrize("nonblocking", [False, True], ids=["blocking", "nonblocking"])
def test_pending_lists_on_a_user_stream(nonblocking):
    """The case of test_up_to_32_chunks_wait_for_one_tile_launch (20 sub-files wait in the pending list for ONE tile
    launch, NGP with the in-tile per-file fold) on a user stream: bit for bit the oracle's map."""
    files, first = [], 0
    for ff in range(20):
        files.append(one_type_file(20000 + 7 * ff, first=first))
        first += 20000 + 7 * ff
    ref_tot, _, nsel = run_oracle(files, 256, FOV, LD, LD2, ngp=True)
    with Scope() as sc:
        U, S = sc.stream(nonblocking), sc.slicer()
        S.set_stream(U.ptr)
        S.set_option("k4_int", 2)
        S.set_option("pending", 32)
        (tot, _, cnt), = run_gpu(S, files, 256, FOV, [LD], [LD2], ngp=True, algo=slicer_amd.ALGO_BINNED)
        assert np.array_equal(cnt, nsel)
        assert np.array_equal(bits(tot), bits(ref_tot))


# ---- 3. ordered behind the caller's earlier work -------------------------------------------------------------------
def test_pass_is_ordered_behind_earlier_work_on_the_callers_stream(particles):
    """bench.py's pattern: a generator handle G and a pass handle S on ONE user stream U.  The delay, then
    G.synth_positions into d_pos (which holds particles of another seed), then S's pass over d_pos: the NGP map is the
    oracle's of the right seed.  (One stream orders all of it; this passes on an unordered set_stream too -- what it
    pins is that nothing in a pass leaves the caller's stream.)"""
    with Scope() as sc:
        U, G, S = sc.stream(), sc.slicer(), sc.slicer()
        delay = sc.sub(Delay(G))
        d_pos = sc.device(S, synth.positions(0, NPART, BOX, seed=OTHER_SEED))
        enqueue_pass(S, d_pos, NPART)  # (workspaces allocated; the map now holds the other seed's particles)
        S.plane_finalize()
        S.synchronize()
        G.set_stream(U.ptr)
        S.set_stream(U.ptr)
        delay.queue()
        G.synth_positions(d_pos, 0, NPART, BOX)
        enqueue_pass(S, d_pos, NPART)
        still_busy(U, "file_end")
        tot, _, cnt = S.plane_read(0)
        assert np.array_equal(cnt, particles["nsel"])
        assert np.array_equal(bits(tot), bits(particles["ngp"]))


# ---- 4. a switch keeps order: root handle --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kappa_unswitched(particles):
    """Kappa.add_device + Kappa.read of the finalized NGP map, all on one stream."""
    with Scope() as sc:
        S = sc.slicer()
        enqueue_pass(S, sc.device(S, particles["file"]["pos"]), NPART)
        S.plane_finalize()
        K = sc.sub(lensing.Kappa(S, NPIX, 1))
        K.add_device([S.plane_device_maps(0)[0]], [[2.5]])
        out = K.read(0)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("consumer", ["plane_read", "kappa"])
@pytest.mark.parametrize("nonblocking", [False, True], ids=["blocking", "nonblocking"])
def test_switch_keeps_order_root_handle(particles, kappa_unswitched, nonblocking, consumer):
    """A pass on stream A behind the delay, finalized there; set_stream(B); then plane_read gives the oracle's NGP map,
    and Kappa.add_device on plane_device_maps() + Kappa.read the bits of the same calls without a switch.  The maps hold
    another seed's particles beforehand.  Against a set_stream that orders nothing: kappa fails on values with either
    kind of A; plane_read fails with a non-blocking A and passes with a blocking one, because its copy is a hipMemcpy
    on the legacy default stream, which HIP orders behind every blocking stream."""
    with Scope() as sc:
        A, B, S = sc.stream(nonblocking), sc.stream(nonblocking), sc.slicer()
        delay = sc.sub(Delay(S))
        d_other = sc.device(S, synth.positions(0, NPART, BOX, seed=OTHER_SEED))
        d_pos = sc.device(S, particles["file"]["pos"])
        K = sc.sub(lensing.Kappa(S, NPIX, 1))
        enqueue_pass(S, d_other, NPART)
        S.plane_finalize()
        S.synchronize()
        S.set_stream(A.ptr)
        delay.queue()
        enqueue_pass(S, d_pos, NPART)
        S.plane_finalize()
        S.set_stream(B.ptr)
        if consumer == "kappa":
            K.add_device([S.plane_device_maps(0)[0]], [[2.5]])
            still_busy(A, "Kappa.add_device")
            assert np.array_equal(bits(K.read(0)), bits(kappa_unswitched))
        else:
            still_busy(A, "set_stream")
            tot, _, cnt = S.plane_read(0)
            assert np.array_equal(cnt, particles["nsel"])
            assert np.array_equal(bits(tot), bits(particles["ngp"]))


# ---- 5. a switch keeps order: sub-handles --------------------------------------------------------------------------
def _map(n, seed):
    return np.random.default_rng(seed).standard_normal((n, n)).astype(np.float32)


_T8 = np.linspace(-1.5, 1.5, 8)


class _Case:
    """One module: make(S, decoy) its sub-handle (decoy: other tables of the same sizes), run(x, d_map), read(x)."""

    def __init__(self, n, make, run=None, read=None, prepare=None, create_waits=False):
        self.n, self.make, self.create_waits = n, make, create_waits
        self.run = run or (lambda x, d, aux: x.run(d))
        self.read = read or (lambda x: x.read())
        self.prepare = prepare  # aux sub-handle made up front (the Starlet of the l1norm case)


def _l1_run(x, d, starlet):
    starlet.run(d)
    x.run_scale(starlet, 1)


CASES = {
    "smooth_gauss": _Case(64, lambda S, decoy: lensing.Smooth(S, 64, "gauss", 2.4 if decoy else 2.5)),
    "smooth_map": _Case(64, lambda S, decoy: lensing.Smooth(S, 64, "map", 2.4 if decoy else 2.5)),
    "peaks": _Case(65, lambda S, decoy: lensing.Peaks(S, 65, _T8 + (0.3 if decoy else 0.0))),
    "minkowski": _Case(65, lambda S, decoy: lensing.Minkowski(S, 65, _T8 + (0.3 if decoy else 0.0))),
    "betti": _Case(65, lambda S, decoy: lensing.Betti(S, 65, _T8 + (0.3 if decoy else 0.0))),
    "l1norm": _Case(65, lambda S, decoy: lensing.L1Norm(S, 65, 0.2 * (_T8 + 1.5) + (0.1 if decoy else 0.0)), run=_l1_run,
                    prepare=lambda S: lensing.Starlet(S, 65, 2)),
    # create leaves a zero-fill of the accumulators queued (hipMemsetAsync), no table
    "kappa": _Case(64, lambda S, decoy: lensing.Kappa(S, 64, 1), run=lambda x, d, aux: x.add_device([d], [[1.5]]),
                   read=lambda x: x.read(0)),
    # the control: slicer_power_create waits for its uploads
    "power": _Case(30, lambda S, decoy: lensing.Power(S, 30, 5.0, 1), run=lambda x, d, aux: x.run([d]),
                   read=lambda x: x.read()["cl"], create_waits=True),
}


_ONE_STREAM = {}


def _one_stream(name):
    """create, run, read of the module on one stream: computed once per module, shared by both tests."""
    if name not in _ONE_STREAM:
        _ONE_STREAM[name] = _run_one_stream(CASES[name])
    return _ONE_STREAM[name]


def _run_one_stream(case):
    with Scope() as sc:
        S = sc.slicer()
        d = sc.device(S, _map(case.n, 1))
        aux = sc.sub(case.prepare(S)) if case.prepare else None
        x = sc.sub(case.make(S, False))
        case.run(x, d, aux)
        return case.read(x)


@pytest.mark.parametrize("name", list(CASES))
def test_switch_keeps_order_sub_handle_created_on_the_old_stream(name):
    """The delay on A, the sub-handle created (its tables are uploaded on A), set_stream(B), the run on B, the read: the
    bits of the same calls on one stream.  Modules whose create returns with an upload or fill still queued, found by
    walking every *_create: Smooth (weights), Peaks, Minkowski, L1Norm and Betti (rank_upload's table) and Kappa (the
    zero-fill of its accumulators); Shear, Power, Pcl, Xi, Bispectrum and the FFT plan wait for theirs, Moments, Noise,
    Starlet and Rays upload nothing.  Power is the control: its create returns only when A has drained (asserted, in
    place of the premise, which cannot hold behind such a wait).  A sub-handle of the same sizes with other tables is made
    and destroyed first, so that memory a run could read too early holds other values."""
    case = CASES[name]
    want = _one_stream(name)
    with Scope() as sc:
        A, B, S = sc.stream(), sc.stream(), sc.slicer()
        delay = sc.sub(Delay(S))
        d = sc.device(S, _map(case.n, 1))
        aux = sc.sub(case.prepare(S)) if case.prepare else None
        with case.make(S, True) as decoy:
            if name == "kappa":  # (its queued fill writes zeros: the memory it takes over must hold something else)
                case.run(decoy, d, aux)
        S.set_stream(A.ptr)
        delay.queue()
        x = sc.sub(case.make(S, False))
        busy_after_create = A.busy()
        S.set_stream(B.ptr)
        case.run(x, d, aux)
        if case.create_waits:  # the control's create is the wait: the delay cannot outlast it
            assert not busy_after_create
        else:
            still_busy(A, f"the run of {name} on the new stream")
        got = case.read(x)
        assert same_bits(got, want)


@pytest.mark.parametrize("name", list(CASES))
def test_switch_keeps_order_sub_handle_read_on_the_new_stream(name):
    """The sub-handle runs on A behind the delay, set_stream(B), and only then read(): the bits of the same calls on
    one stream.  Its result buffers hold the result of another map beforehand."""
    case = CASES[name]
    want = _one_stream(name)
    with Scope() as sc:
        A, B, S = sc.stream(), sc.stream(), sc.slicer()
        delay = sc.sub(Delay(S))
        d, d_other = sc.device(S, _map(case.n, 1)), sc.device(S, _map(case.n, 2))
        aux = sc.sub(case.prepare(S)) if case.prepare else None
        x = sc.sub(case.make(S, False))
        if name != "kappa":  # (an accumulator: its other values are the zeros of create)
            case.run(x, d_other, aux)
        S.synchronize()
        S.set_stream(A.ptr)
        delay.queue()
        case.run(x, d, aux)
        S.set_stream(B.ptr)
        still_busy(A, f"set_stream, before the read of {name}")
        got = case.read(x)
        assert same_bits(got, want)


# ---- 6. two handles at once ----------------------------------------------------------------------------------------
def _two_files():
    return [one_type_file(60000, first=0), one_type_file(50003, first=60000)]


def _steps(S, f, ngp, sm):
    """One pass of file f and one Smooth of its map, as a generator: every yield is one call made."""
    S.plane_begin(NPIX, FOV, [LD], [LD2], mas=slicer_amd.MAS_NGP if ngp else slicer_amd.MAS_TSC,
                  accum=slicer_amd.ACC_F32 if ngp else slicer_amd.ACC_FIXED64)
    yield
    S.file_begin(f["npart"], f["massarr"], BOX, RND["sgn"], RND["face"], RND["center"], RND["rcase"])
    yield
    n = int(f["npart"][1])
    for lo in range(0, n, 20000):  # several deposit calls, each in staging chunks of 8192
        S.deposit_host(1, f["pos"][lo:min(lo + 20000, n)])
        yield
    S.file_end()
    yield
    S.plane_finalize()
    yield
    sm.run(S.plane_device_maps(0)[0])
    yield


def test_two_handles_at_once():
    """S1 on U1 and S2 on U2 with different files, their passes interleaved call by call, each followed by one Smooth of
    its plane map: every map (NGP; FIXED64 TSC) and every smoothed map is bit for bit what the same handle gives alone.
    deposit_host goes through the double-buffered staging, whose stage_free events are recorded on the caller's stream."""
    files = _two_files()
    with Scope() as sc:
        U1, U2, S1, S2 = sc.stream(), sc.stream(True), sc.slicer(max_chunk=8192), sc.slicer(max_chunk=8192)
        S1.set_stream(U1.ptr)
        S2.set_stream(U2.ptr)
        sm = [sc.sub(lensing.Smooth(S, NPIX, "gauss", 2.5)) for S in (S1, S2)]
        for ngp in (True, False):
            alone = []
            for S, f, m in zip((S1, S2), files, sm):
                for _ in _steps(S, f, ngp, m):
                    pass
                alone.append((S.plane_read(0)[0], m.read()))
            gens = [_steps(S, f, ngp, m) for S, f, m in zip((S1, S2), files, sm)]
            live = [True, True]
            while any(live):
                for k, g in enumerate(gens):
                    if live[k]:
                        live[k] = next(g, "end") != "end"
            for S, m, (tot0, sm0) in zip((S1, S2), sm, alone):
                sm1 = m.read()
                tot1 = S.plane_read(0)[0]
                assert tot0.sum() > 0
                assert np.array_equal(bits(tot1), bits(tot0)) and np.array_equal(bits(sm1), bits(sm0)), ngp


# ---- 7. the default stream -----------------------------------------------------------------------------------------
def test_pointer_zero_is_the_handles_own_blocking_stream():
    """torch.cuda.current_stream().cuda_stream is 0 under torch's default stream.  Slicer.set_stream(0) leaves (or puts)
    the handle on its own blocking stream, get_stream() says so, and parallel.works_with_stream -- the check of
    reduce_planes -- accepts exactly that pairing: HIP orders a blocking stream with the legacy default stream both
    ways.  (The route taken; the other, mapping 0 to hipStreamLegacy, would move bench.py's one-handle run onto the
    default stream.  tests/test_bench_cli.py runs the layouts that need it.)"""
    with Scope() as sc:
        U, V, S = sc.stream(), sc.stream(True), sc.slicer()
        own = S.get_stream()
        for ptr in (U.ptr, V.ptr):
            S.set_stream(ptr)
            assert parallel.works_with_stream(S, ptr) and not parallel.works_with_stream(S, 0)
            assert not parallel.works_with_stream(S, own)
            S.set_stream(0)
            assert S.get_stream() == own != 0 and S.on_own_stream()
            assert parallel.works_with_stream(S, 0) and parallel.works_with_stream(S, own)
            assert not parallel.works_with_stream(S, ptr)
