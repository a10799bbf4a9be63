"""GPU: the row-slab orchestration with halo rows still in flight.  The fabric of test_gpu_slab.py waits on the host for
the GPU before and after every copy, so the ordering between the compute streams and the exchange (FLUID_PARAM_XCHG_OVERLAP:
call_exchange's events, xchg_join, the split launches, the second stream's share of the debt, the velocity bound reduced on
the device) is never put to the test there.  AsyncFabric below moves the rows the way a real send / receive does: enqueued
on the stream the library hands the callback, ordered between ranks by events only, behind a delay, into landing rows
poisoned with NaN first -- so a consumer that does not wait reads NaN, and a producer that overwrites a row still being read
hands the peer the wrong value.  The bar stays the one of test_gpu_slab.py: slabs == one context, every field, every bit."""
import threading

import numpy as np
import pytest

from conftest import assert_bit_equal, rnd
from test_gpu_slab import DT, run_ranks, single, synthetic

pytestmark = pytest.mark.gpu
FIELDS = ("u", "v", "dens", "u_prev", "v_prev", "dens_prev")
DELAY_MS = 2.0      # 8 ranks share the GPU's queues and the host: 0.5 ms left most of their copies done at return
STATS = {"async_halo": 0, "pending_at_return": 0}


@pytest.fixture(scope="module")
def delay():
    """A callable that enqueues about DELAY_MS of GPU time on torch's current stream: torch.cuda._sleep, its cycle count
    measured here with two events (a cycle's length is not documented for this device); a chain of small ops on a scratch
    tensor if _sleep turns out not to wait."""
    import torch
    s = torch.cuda.Stream()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            a.record()
            fn()
            b.record()
        b.synchronize()
        return a.elapsed_time(b)

    probe = 1 << 20
    timed(lambda: torch.cuda._sleep(probe))
    ms = timed(lambda: torch.cuda._sleep(probe))
    if ms > 0.01:
        cycles = max(1, int(probe * DELAY_MS / ms))
        fn = lambda: torch.cuda._sleep(cycles)        # noqa: E731
        what = "torch.cuda._sleep(%d)" % cycles
    else:
        scratch = torch.zeros(1 << 16, device="cuda")
        timed(lambda: scratch.add_(1.0))
        per = max(timed(lambda: [scratch.add_(1.0) for _ in range(64)]) / 64, 1e-3)
        k = max(1, int(DELAY_MS / per))
        fn = lambda: [scratch.add_(1.0) for _ in range(k)]      # noqa: E731
        what = "%d chained adds" % k
    got = timed(fn)
    print("\nasync fabric delay: %s = %.3f ms" % (what, got))
    assert got > 0.25 * DELAY_MS, "the delay does not delay (%.3f ms)" % got
    yield fn
    if STATS["async_halo"]:
        print("\nasync fabric: %d of %d halo exchanges issued beside compute were still in flight at return"
              % (STATS["pending_at_return"], STATS["async_halo"]))


class AsyncFabric:
    """P ranks on one GPU whose callback never waits on the host for the GPU.  Per call, as a send / receive rendezvous:
    1. record `ready` on the exchange stream, publish this rank's field views, barrier;
    2. wait on the `ready` of the peers read from, poison the landing rows (NaN), delay, copy, record `copied`, barrier;
    3. wait on the `copied` of the peers that read this rank's rows (the source rows stay in use until the library's
       ev_xdone, as a real send's would), barrier.
    Every GPU-side wait is on a record enqueued before the last barrier: no wait cycle can form; a rank that diverges
    breaks the barrier (timeout / abort) instead of hanging.
    stream="exchange": enqueue on fluid_exchange_stream() asked inside the callback; "creation": on the solver's own stream.
    max="device": MAX_BEGIN reduces the device word in place (same three phases), END hands the value back; "host": END
    reduces on the host.  XCHG_MAX (synchronous) always reduces on the host."""

    def __init__(self, nranks, delay, stream="exchange", max="device", timeout=120):
        assert stream in ("exchange", "creation") and max in ("device", "host")
        self.nranks, self.delay, self.stream, self.max = nranks, delay, stream, max
        self.barrier = threading.Barrier(nranks, timeout=timeout)
        self.solvers = [None] * nranks
        self.log = [[] for _ in range(nranks)]
        self.maxima = [[] for _ in range(nranks)]
        self.scalars = [0.0] * nranks
        self.views = [None] * nranks             # fid -> [n+2, pitch] tensor, as placed at this call
        self.words = [None] * nranks             # the device reduction word, int32[1]
        self.stage = [None] * nranks
        self.ready = [None] * nranks
        self.copied = [None] * nranks
        self.async_halo = [0] * nranks           # halo exchanges issued on a stream other than the compute stream ...
        self.pending = [0] * nranks              # ... and those whose copy had not finished when the callback returned
        self._ext = [{} for _ in range(nranks)]

    def _stream_for(self, rank):
        """(stream to enqueue on, whether the library runs this exchange beside compute)"""
        import torch
        me = self.solvers[rank]
        ptr = me.exchange_stream()
        beside = ptr != me.torch_stream.cuda_stream
        if self.stream == "creation" or not beside:
            return me.torch_stream, beside
        st = self._ext[rank].get(ptr)
        if st is None:
            st = self._ext[rank][ptr] = torch.cuda.ExternalStream(ptr, device=me.torch_stream.device)
        return st, beside

    def _landing(self, rank, kind, depth):
        """(rows of this rank's copy, peer that owns them) for every range this rank receives."""
        from fluidsimulationcuda_amd import capi
        from fluidsimulationcuda_amd.slab import slab_rows
        me = self.solvers[rank]
        lo, hi = me.owned_rows
        if kind == capi.XCHG_HALO:
            out = []
            if rank > 0:
                out.append((slice(lo - depth, lo), rank - 1))
            if rank < self.nranks - 1:
                out.append((slice(hi, hi + depth), rank + 1))
            return out
        out = []
        for r in range(self.nranks):
            if r != rank:
                a, b = slab_rows(me.n, r, self.nranks)
                out.append((slice(a - (1 if r == 0 else 0), b + (1 if r == self.nranks - 1 else 0)), r))
        return out

    def _readers(self, rank, kind):
        from fluidsimulationcuda_amd import capi
        if kind == capi.XCHG_HALO:                 # the neighbours
            return [r for r in (rank - 1, rank + 1) if 0 <= r < self.nranks]
        return [r for r in range(self.nranks) if r != rank]

    def make_callback(self, rank):
        import torch
        from fluidsimulationcuda_amd import capi

        def host_max(scalar):
            self.scalars[rank] = scalar
            self.maxima[rank].append(scalar)
            self.barrier.wait()
            out = max(self.scalars)
            self.barrier.wait()
            return out

        def cb(kind, ids, depth, scalar):
            self.log[rank].append((kind, tuple(ids), depth))
            if kind == capi.XCHG_MAX:
                return host_max(scalar)
            if kind == capi.XCHG_MAX_END:
                if self.max == "host":
                    return host_max(scalar)
                self.maxima[rank].append(scalar)
                return scalar
            if kind == capi.XCHG_MAX_BEGIN and self.max == "host":
                return None
            stream, beside = self._stream_for(rank)
            with torch.cuda.stream(stream):
                if kind == capi.XCHG_MAX_BEGIN:
                    self._max_begin(rank, stream)
                    return None
                self._rows(rank, kind, ids, depth, stream)
                end = torch.cuda.Event()
                end.record(stream)
            if kind == capi.XCHG_HALO and beside:
                self.async_halo[rank] += 1
                self.pending[rank] += 0 if end.query() else 1
            return None

        return cb

    def _rows(self, rank, kind, ids, depth, stream):
        import torch
        me = self.solvers[rank]
        # phase 1: my rows are ready once the stream I was given reaches this point
        ev = torch.cuda.Event()
        ev.record(stream)
        self.ready[rank] = ev
        self.views[rank] = {fid: me.field_tensor(fid) for fid in ids}    # (buffers trade places inside solves)
        self.barrier.wait()
        # phase 2: behind the peers' rows, poison what is about to land, wait a while, then copy
        land = self._landing(rank, kind, depth)
        for peer in sorted({p for _, p in land}):
            stream.wait_event(self.ready[peer])
        for fid in ids:
            for rows, _ in land:
                self.views[rank][fid][rows].fill_(float("nan"))
        self.delay()
        for fid in ids:
            for rows, peer in land:
                self.views[rank][fid][rows].copy_(self.views[peer][fid][rows])
        ev = torch.cuda.Event()
        ev.record(stream)
        self.copied[rank] = ev
        self.barrier.wait()
        # phase 3: my rows stay untouched until every peer that reads them has copied them
        for peer in self._readers(rank, kind):
            stream.wait_event(self.copied[peer])
        self.barrier.wait()

    def _max_begin(self, rank, stream):
        import torch
        me = self.solvers[rank]
        if self.words[rank] is None:
            off = me.scalar_ptr() - me.arena.data_ptr()
            self.words[rank] = me.arena[off:off + 4].view(torch.int32)
            self.stage[rank] = torch.zeros(self.nranks, dtype=torch.int32, device=me.torch_stream.device)
        ev = torch.cuda.Event()
        ev.record(stream)
        self.ready[rank] = ev
        self.barrier.wait()
        peers = [r for r in range(self.nranks) if r != rank]
        for r in peers:
            stream.wait_event(self.ready[r])
        self.delay()
        for r in range(self.nranks):
            self.stage[rank][r:r + 1].copy_(self.words[r])
        ev = torch.cuda.Event()
        ev.record(stream)
        self.copied[rank] = ev
        self.barrier.wait()
        for r in peers:                                   # everyone has read my word: now it may change
            stream.wait_event(self.copied[r])
        # the word holds a non-negative float's bit pattern: MAX over the patterns is the float maximum
        self.words[rank].copy_(self.stage[rank].amax().reshape(1))
        self.barrier.wait()


def run_async(n, nranks, halo, fields, body, delay, stream="exchange", max="device", **kw):
    return run_ranks(n, nranks, halo, fields, body, fabric=lambda p: AsyncFabric(p, delay, stream=stream, max=max), **kw)


def check_fabric(fab, overlap, what):
    """Every rank issued the same exchange sequence; with the overlap on, most halo exchanges that ran beside compute
    returned while their rows were still on the way (else nothing here was in flight)."""
    for r in range(1, fab.nranks):
        assert fab.log[r] == fab.log[0], "rank %d issued a different exchange sequence -- %s" % (r, what)
    STATS["async_halo"] += sum(fab.async_halo)
    STATS["pending_at_return"] += sum(fab.pending)
    if overlap:
        calls, pending = sum(fab.async_halo), sum(fab.pending)
        assert calls > 0 and pending * 2 > calls, "only %d of %d halo exchanges were in flight at return -- %s" % (pending, calls, what)


def compare(got, want, what):
    for k in FIELDS:
        hint = {"v_prev": " (the last divergence)", "u_prev": " (the last pressure)"}.get(k, "")
        assert_bit_equal(got[k], want[k], "%s%s -- %s" % (k, hint, what))


# (XCHG_OVERLAP, SLAB_OVERLAP, stream, max, jacobi): every pair of values of any two switches appears in some row
DEFAULT = (1, 1, "exchange", "device", 3)
PAIRWISE = [(0, 0, "creation", "host", 0), (0, 0, "creation", "host", 3), (0, 1, "exchange", "device", 0),
            (1, 0, "exchange", "device", 0), (1, 1, "creation", "device", 3), (1, 1, "exchange", "host", 3)]
SHAPES = [(1022, 2, 42, 40, 0), (1022, 4, 0, 40, 0), (510, 3, 8, 40, 0), (257, 3, 5, 40, 0), (1022, 8, 20, 20, 0),
          (254, 2, 40, 20, 1)]
FULL_STEP_CASES = [s + DEFAULT for s in SHAPES] + [s + PAIRWISE[k] for s, k in zip(SHAPES, (0, 1, 2, 3, 5, 4))]


@pytest.mark.parametrize("n,nranks,halo,iters,storage,xo,so,stream,mx,jacobi", FULL_STEP_CASES)
def test_steps_with_rows_in_flight(delay, n, nranks, halo, iters, storage, xo, so, stream, mx, jacobi):
    """Three full steps (sources, then two more) on slabs whose rows arrive late: == one context, all six fields."""
    from fluidsimulationcuda_amd import capi
    fields = synthetic(n, seed=5)
    splits = {}

    def body(s):
        s.step(1, use_sources=True, iters=iters)
        s.step(2, iters=iters)
        splits[s.rank] = s.split_launches()

    what = "n=%d ranks=%d halo=%d iters=%d fp16=%d overlap=%d slab_overlap=%d stream=%s max=%s jacobi=%d" % (
        n, nranks, halo, iters, storage, xo, so, stream, mx, jacobi)
    want = single(n, fields, body, storage=storage)
    got, fab = run_async(n, nranks, halo, fields, body, delay, stream=stream, max=mx, jacobi=jacobi, storage=storage,
                         params={capi.PARAM_XCHG_OVERLAP: xo, capi.PARAM_SLAB_OVERLAP: so})
    compare(got, want, what)
    check_fabric(fab, xo == 1, what)
    if xo and jacobi == 3:
        assert all(splits[r] > 0 for r in range(nranks)), splits
    elif not xo:
        assert all(v == 0 for v in splits.values()), splits


@pytest.mark.parametrize("fill", [0, 1])
@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("n,nranks,halo", [(1022, 2, 42), (510, 3, 8)])
def test_fused_divergence_with_velocity_in_flight(delay, n, nranks, halo, fuse, fill):
    """FUSE_DIVERGENCE: the pressure solve's first launch forms and stores the divergence from u and v while their halo
    rows are on the way (project).  Its interior strips must store only rows whose stencil stays inside the slab, with the
    pipeline-fill triangle computed (TB_FILL 0) or skipped (1); the edge strips the rest."""
    from fluidsimulationcuda_amd import capi
    fields = synthetic(n, seed=21)
    params = {capi.PARAM_FUSE_DIVERGENCE: fuse, capi.PARAM_TB_FILL: fill}

    def body(s):
        for k, v in params.items():
            s.set_param(k, v)
        s.step(1, use_sources=True)
        s.step(2)

    want = single(n, fields, body)
    got, fab = run_async(n, nranks, halo, fields, body, delay, jacobi=3, params={capi.PARAM_XCHG_OVERLAP: 1})
    compare(got, want, "fuse_divergence=%d tb_fill=%d, n=%d ranks=%d halo=%d" % (fuse, fill, n, nranks, halo))
    check_fabric(fab, True, "fuse_divergence=%d tb_fill=%d" % (fuse, fill))


def test_gather_fallback_with_rows_in_flight(delay):
    """A back-trace longer than a neighbour's slab: whole fields gathered through the fabric, bound reduced on the device."""
    from fluidsimulationcuda_amd import capi
    n, nranks = 126, 4
    rng = np.random.default_rng(11)
    fields = dict(u=rnd(rng, n, -30, 30), v=rnd(rng, n, -30, 30), dens_prev=rnd(rng, n),
                  dens=np.zeros((n + 2, n + 2), np.float32))

    def body(s):
        s.advect(0, "dens", "dens_prev", "u", "v", DT)

    want = single(n, fields, body)
    got, fab = run_async(n, nranks, 4, fields, body, delay)
    assert_bit_equal(got["dens"], want["dens"], "advect with gather fallback")
    assert any(e[0] == capi.XCHG_GATHER for e in fab.log[0])
    check_fabric(fab, False, "gather")


@pytest.mark.parametrize("grow,expect", [(0.5, "kept"), (40.0, "repeated"), (4000.0, "gathered")])
def test_early_advection_on_a_bound_reduced_on_the_device(delay, grow, expect):
    """FLUID_PARAM_EARLY_ADVECT with the bound reduced in place on the device word behind a delay: advect_rows must wait
    for the copy of the reduced word before it trusts it, whether the early advection holds, is repeated, or gathers."""
    from fluidsimulationcuda_amd import capi
    n, nranks = 254, 3
    first = synthetic(n, seed=77)
    rng = np.random.default_rng(78)
    second = {k: (first[k] * np.float32(grow) + rnd(rng, n, -0.001, 0.001)).astype(np.float32)
              for k in ("u_prev", "v_prev", "dens_prev")}

    def body(s):
        s.step(1, use_sources=True)
        if s.nranks > 1:
            s.load_global(**second)
        else:
            s.upload(**second)
        s.step(1, use_sources=True)

    want = single(n, first, body)
    got, fab = run_async(n, nranks, 0, first, body, delay, max="device", jacobi=3, params={capi.PARAM_EARLY_ADVECT: 1})
    compare(got, want, "early advect, sources x %g" % grow)
    check_fabric(fab, True, "early advect x %g" % grow)
    gathers = [e[0] for e in fab.log[0]].count(capi.XCHG_GATHER)
    assert gathers == (2 if expect == "gathered" else 0), fab.log[0]
    # every rank brought the same (reduced) bound back from each MAX_END, and it is the bound of the whole grid
    assert all(fab.maxima[r] == fab.maxima[0] for r in range(nranks)), fab.maxima


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_operators_on_slabs_with_rows_in_flight(delay, variant):
    n, nranks = 126, 3
    rng = np.random.default_rng(13)
    fields = {k: rnd(rng, n) for k in FIELDS}

    def body(s):
        s.add_source("u", "u_prev", DT)
        s.diffuse(1, "u_prev", "u", 0.3, 2.2, 6)
        s.computeDivergenceAndPressure("u", "v", "dens", "dens_prev")
        s.diffuse(0, "dens", "dens_prev", 1.0, 4.0, 10)
        s.lastProject("u", "v", "dens")

    want = single(n, fields, body)
    got, fab = run_async(n, nranks, 4, fields, body, delay, jacobi=variant)
    compare(got, want, "operators, jacobi variant %d" % variant)
    check_fabric(fab, False, "operators")


@pytest.mark.parametrize("stream", ["exchange", "creation"])
@pytest.mark.parametrize("kind", ["halo", "gather"])
def test_exchange_now_delivers_the_peer_rows(delay, kind, stream):
    """fluid_exchange_now after a step, then synchronize(): the landing rows hold the peers' rows (== one context's),
    the poison is gone everywhere -- the fabric always overwrites what it poisons, and the library's synchronize covers
    an exchange it issued on the compute stream."""
    import ctypes as C
    from fluidsimulationcuda_amd import capi
    from fluidsimulationcuda_amd.slab import slab_rows
    n, nranks, depth = 257, 3, 7
    fields = synthetic(n, seed=3)
    ids = [capi.U, capi.V, capi.DENS, capi.U_PREV, capi.V_PREV, capi.DENS_PREV]
    seen = {}

    def body(s):
        s.step(1, use_sources=True)
        if s.nranks == 1:
            return
        arr = (C.c_int * len(ids))(*ids)
        k = capi.XCHG_HALO if kind == "halo" else capi.XCHG_GATHER
        capi.check(capi.lib().fluid_exchange_now(s._h, k, arr, len(ids), depth if kind == "halo" else 0))
        s.synchronize()
        lo, hi = s.owned_rows
        rows = (max(0, lo - depth), min(n + 2, hi + depth)) if kind == "halo" else (0, n + 2)
        out = {}
        for name in FIELDS:
            full = np.full((n + 2, n + 2), np.nan, np.float32)
            s.download_rows(name, full, *rows)
            out[name] = (rows, full)
        seen[s.rank] = out

    want = single(n, fields, body)
    _, fab = run_async(n, nranks, 0, fields, body, delay, stream=stream, jacobi=3)
    check_fabric(fab, False, "exchange_now")
    for r in range(nranks):
        for name in FIELDS:
            (a, b), full = seen[r][name]
            assert not np.isnan(full[a:b]).any(), "rank %d %s: poison left in rows [%d, %d)" % (r, name, a, b)
            assert_bit_equal(full[a:b], want[name][a:b], "rank %d %s rows [%d, %d) after exchange_now %s" % (r, name, a, b, kind))
            for peer in (r - 1, r + 1):             # ... which are the rows the neighbour owns
                if 0 <= peer < nranks:
                    pa, pb = slab_rows(n, peer, nranks)
                    rows = slice(max(pa, a), min(pb, b))
                    assert_bit_equal(full[rows], seen[peer][name][1][rows], "rank %d %s: rows landed from rank %d" % (r, name, peer))


@pytest.mark.parametrize("seed", range(24))
def test_random_slab_configuration_with_rows_in_flight(delay, seed):
    from test_gpu_random_configs import random_params
    from fluidsimulationcuda_amd import capi
    rng = np.random.default_rng(5000 + seed)
    nranks = int(rng.choice([2, 2, 3, 4, 5]))
    n = int(rng.choice([61, 100, 126, 200, 254, 257, 400, 510]))
    while n // nranks < 10:
        nranks -= 1
    storage = int(rng.choice([0, 0, 1]))
    halo = int(rng.choice([0, 1, 3, 8, 9, 16, 40, 41, 42, 60]))
    iters = int(rng.choice([2, 8, 12, 20, 28, 40, 40]))
    jacobi = int(rng.choice([3, 3, 3, 0]))
    params = random_params(rng, capi)
    params[capi.PARAM_SLAB_OVERLAP] = int(rng.choice([0, 1, 1]))
    params[capi.PARAM_XCHG_OVERLAP] = int(rng.choice([0, 1, 1]))
    params[capi.PARAM_TB_FILL] = int(rng.choice([0, 1]))
    params.pop(capi.PARAM_TB_MIN_CELLS)
    if storage == 1:
        jacobi = 3
        for k in (capi.PARAM_TB_MAX_SWEEPS, capi.PARAM_TB_T16_MIN_CELLS):
            params.pop(k)
    stream = str(rng.choice(["exchange", "exchange", "creation"]))
    mx = str(rng.choice(["device", "device", "host"]))
    fields = synthetic(n, seed=seed)
    what = "seed %d: n=%d ranks=%d halo=%d iters=%d storage=%d jacobi=%d stream=%s max=%s %r" % (
        seed, n, nranks, halo, iters, storage, jacobi, stream, mx, params)

    def body(s):
        if s.nranks == 1:
            s.set_param(capi.PARAM_TB_FILL, params[capi.PARAM_TB_FILL])
        s.step(1, use_sources=True, iters=iters)
        s.step(1, iters=iters)

    want = single(n, fields, body, storage=storage)
    got, fab = run_async(n, nranks, halo, fields, body, delay, stream=stream, max=mx, jacobi=jacobi, storage=storage,
                         params=params)
    compare(got, want, what)
    check_fabric(fab, False, what)
