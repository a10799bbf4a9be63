"""GPU: recombining ensembles -- fluid_transform_members / fluid_select_members (include/fluid_amd.h, "recombining
ensembles"): every new member of a field a linear combination of the old ones, per cell, in place.

Every expected value comes from `define` below, the header's definition in numpy: a loop over the old members k in
increasing order, in double, over the non-zero weights only, vectorised over the cells, one rounding to float -- applied
to what download_members (the pack) showed before the call -- then `narrow` (fp16 storage: one more rounding to nearest
even).  Everything is compared bit for bit; a NaN is a NaN, its sign and payload are not compared.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
F32 = np.float32
SIZES = [1, 6, 13, 30, 61]                  # W % 4 != 0, rows shorter and longer than a wave
MEMBERS = [1, 2, 3, 5, 8, 9, 17, 32, 33, 64]   # every padded count 1, 2, 4 .. 64, and the counts just past a power of two
MAIN = ("u", "v", "dens", "u_prev", "v_prev", "dens_prev")
DT = 0.016


def F():
    import fluidsimulationcuda_amd as f
    return f


def solver(n, members, storage=0, **kw):
    return F().FluidSolver(n, members=members, storage=storage, **kw)


# ---- the definition ------------------------------------------------------------------------------------------------------
def define(x, w):
    """x: (M, ...) float32, what the pack shows before the call; w: (M, M) float32, w[k, m] the weight of OLD member k in
    NEW member m.  The new members, float32."""
    x, w = np.asarray(x, F32), np.asarray(w, F32)
    xd = x.astype(np.float64)
    out = np.empty_like(x)
    with np.errstate(all="ignore"):
        for m in range(x.shape[0]):
            s = None
            for k in range(x.shape[0]):                   # member order
                if w[k, m] != 0:                          # a zero of either sign takes no part
                    p = xd[k] * np.float64(w[k, m])       # exact: 24 + 24 bits
                    s = p if s is None else s + p
            out[m] = F32(0) if s is None else s.astype(F32)
    return out


def narrow(y, storage):
    with np.errstate(all="ignore"):
        return y.astype(np.float16).astype(F32) if storage else y


def onehot(source):
    m = len(source)
    w = np.zeros((m, m), F32)
    w[np.asarray(source), np.arange(m)] = 1
    return w


def same(got, want, what):
    """bit for bit, except that a NaN is any NaN"""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, what
    ok = np.where(np.isnan(want), np.isnan(got), got.view(np.uint32) == want.view(np.uint32))
    if not ok.all():
        at = tuple(np.argwhere(~ok)[0])
        raise AssertionError("%s: %d of %d values differ; first at %s: got %r (%08x) want %r (%08x)" % (
            what, int((~ok).sum()), ok.size, at, got[at], got.view(np.uint32)[at], want[at], want.view(np.uint32)[at]))


# ---- data ------------------------------------------------------------------------------------------------------------------
def mixed_values(rng, shape, storage):
    """magnitudes over many binades, float (fp16 storage: half) denormals, +-0"""
    lo, hi = (-26, 10) if storage else (-149, 60)
    x = np.ldexp(rng.uniform(1.0, 2.0, shape), rng.integers(lo, hi, shape)) * rng.choice([-1.0, 1.0], shape)
    x = x.astype(F32)
    kind = rng.integers(0, 12, shape)
    x[kind == 0] = 0.0
    x[kind == 1] = -0.0
    x[kind == 2] = F32(2.0 ** -24 if storage else 1e-45) * rng.choice([-1, 1, 3, -5], shape)[kind == 2]       # denormals
    return x


def mixed_weights(rng, m, zeros=True):
    w = (np.ldexp(rng.uniform(1.0, 2.0, (m, m)), rng.integers(-10, 10, (m, m))) * rng.choice([-1.0, 1.0], (m, m))).astype(F32)
    if zeros:
        kind = rng.integers(0, 6, (m, m))
        w[kind == 0] = 0.0
        w[kind == 1] = -0.0
    return w


def shown(s, field):
    """what the pack shows: every member of a field, the lazy state settled"""
    return s.download_members(field)


# ---- 1. random weights and values -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("members", MEMBERS)
def test_random_weights_and_values(members, storage):
    rng = np.random.default_rng(1000 * storage + members)
    for n in SIZES:
        w = n + 2
        with solver(n, members, storage) as s:
            for zeros in (True, False):          # with zeros: the table with a mask; without: the table where every term is taken
                x = mixed_values(rng, (members, w, w), storage)
                s.upload_members(u=x)
                before = shown(s, "u")
                same(before, narrow(x, storage), "n=%d M=%d: the upload" % (n, members))
                t = mixed_weights(rng, members, zeros)
                s.transform(t, fields=("u",))
                same(shown(s, "u"), narrow(define(before, t), storage), "n=%d M=%d storage=%d zeros=%s" % (n, members, storage, zeros))


# ---- 2. the order is pinned ---------------------------------------------------------------------------------------------------
def order_data(rng, members, w, storage):
    """Members 0 and 2 hold +b and -b, the others values in (-1, 1); the weights are signed powers of two, row 2 equal to
    row 0.  The products of members 0 and 2 lie in 2^56 .. 2^90 and cancel exactly: in member order everything added
    between them is absorbed and everything after them survives, in any other order something else does.  fp32 storage: b
    itself is in 2^56 .. 2^90 and the weights in 2^-3 .. 2^3; fp16 storage cannot hold such a b, so b is in 2^8 .. 2^14 and
    rows 0 and 2 of the weights carry the other 2^50 .. 2^74."""
    x = narrow(rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32), storage)
    lo, hi = (8, 15) if storage else (56, 91)
    b = np.ldexp(1.0, rng.integers(lo, hi, (w, w))).astype(F32)
    x[0], x[2] = b, -b
    t = (np.ldexp(1.0, rng.integers(-3, 4, (members, members))) * rng.choice([-1.0, 1.0], (members, members))).astype(F32)
    if storage:
        t[0] = np.ldexp(t[0], rng.integers(50, 72, members)).astype(F32)
    t[2] = t[0]
    return x, t


@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("members", [m for m in MEMBERS if m >= 4])
def test_the_order_is_pinned(members, storage):
    rng = np.random.default_rng(2000 * storage + members)
    for n in SIZES:
        w = n + 2
        x, t = order_data(rng, members, w, storage)
        want = define(x, t)
        # on the CPU first: the data shows the order -- the reversed member order changes (nearly) every cell ...
        flip = define(x[::-1], t[::-1])
        differs = (flip.view(np.uint32) != want.view(np.uint32)).mean()
        assert differs >= 0.9, "n=%d M=%d: the reversed sum differs in only %.0f%% of the cells" % (n, members, 100 * differs)
        # ... and numpy's own in-order sum of the exact products agrees with the definition
        with np.errstate(all="ignore"):
            prod = x.astype(np.float64)[:, None] * t.astype(np.float64)[:, :, None, None]      # [k, m, i, j]
            acc = prod[0].copy()
            for k in range(1, members):
                acc += prod[k]
        same(acc.astype(F32), want, "n=%d M=%d: numpy's in-order sum" % (n, members))
        with solver(n, members, storage) as s:
            s.upload_members(dens=x)
            before = shown(s, "dens")
            same(before, x, "n=%d M=%d: the data is representable" % (n, members))
            s.transform(t, fields=("dens",))
            same(shown(s, "dens"), narrow(want, storage), "n=%d M=%d storage=%d: member order" % (n, members, storage))


# ---- 3. identity, and the pads ------------------------------------------------------------------------------------------------
def arena_ensemble(n, members, storage):
    import torch
    from fluidsimulationcuda_amd import capi
    nbytes = capi.lib().fluid_arena_bytes_ensemble(n, storage, members)
    arena = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return solver(n, members, storage, arena_ptr=arena.data_ptr(), arena_bytes=nbytes), arena


def arena_rows(s, arena):
    """the arena as (12 x members, N+2, pitch) stored elements, and the offset of column 0"""
    import torch
    from fluidsimulationcuda_amd import capi
    pitch, xoff, ff = C.c_int(), C.c_int(), C.c_size_t()
    assert capi.lib().fluid_layout(s.n, C.byref(pitch), C.byref(xoff), C.byref(ff)) == 0
    s.synchronize()
    torch.cuda.synchronize()
    dtype = np.uint16 if s.storage else np.uint32
    raw = arena.cpu().numpy()[:12 * s.members * ff.value * dtype().itemsize].view(dtype)
    return raw.reshape(12 * s.members, s.n + 2, pitch.value), xoff.value


@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("members", [1, 3, 9, 64])
def test_identity_and_the_pads(members, storage):
    from fluidsimulationcuda_amd import capi
    rng = np.random.default_rng(3000 * storage + members)
    for n in SIZES:
        w = n + 2
        s, arena = arena_ensemble(n, members, storage)
        with s:
            for name in capi.FIELD_NAMES:
                x = narrow(mixed_values(rng, (members, w, w), storage), storage)
                x[x == 0] = 1.5                  # no zero word anywhere: a pad written from a neighbour would show
                s.upload_members(**{name: x})
            stored, xoff = arena_rows(s, arena)
            stored = stored.copy()
            assert stored[:, :, xoff:xoff + w].all()
            s.transform(np.eye(members), fields=capi.FIELD_NAMES)
            after, _ = arena_rows(s, arena)
            assert np.array_equal(after[:, :, xoff:xoff + w], stored[:, :, xoff:xoff + w]), "n=%d M=%d: the identity changed a bit" % (n, members)
            assert not after[:, :, :xoff].any() and not after[:, :, xoff + w:].any(), "n=%d M=%d: pad columns were written" % (n, members)
            # a dense matrix and a selection leave the pads alone too
            s.transform(mixed_weights(rng, members, zeros=False), fields=capi.FIELD_NAMES)
            s.select(rng.integers(0, members, members), fields=capi.FIELD_NAMES)
            after, _ = arena_rows(s, arena)
            assert not after[:, :, :xoff].any() and not after[:, :, xoff + w:].any(), "n=%d M=%d: pad columns were written" % (n, members)


# ---- 4. select ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("members", MEMBERS)
def test_select_copies_members(members, storage):
    rng = np.random.default_rng(4000 * storage + members)
    ids = np.arange(members)
    swap = ids.copy()
    swap[:2] = swap[:2][::-1]                                         # a 2-cycle (M = 1: the identity)
    sources = [swap, np.roll(ids, 1), np.roll(ids, -1),               # ... the M-cycle both ways: the in-place hazard
               np.full(members, members // 2), rng.integers(0, members, members)]      # one member for all; resampling with repeats
    for n in SIZES:
        w = n + 2
        with solver(n, members, storage) as s:
            x = {f: narrow(mixed_values(rng, (members, w, w), storage), storage) for f in ("u", "v", "dens")}
            x["v"][0, 0, 0] = np.nan                                   # (a NaN is copied as a NaN)
            s.upload_members(**x)
            for src in sources:
                s.select(src)                                          # the default: u, v, dens
                for f in x:
                    want = x[f][src]                                   # exact copies of the old members ...
                    same(define(x[f], onehot(src)), want, "the definition with the one-hot matrix copies")      # ... as defined
                    same(shown(s, f), want, "n=%d M=%d storage=%d source=%s: %s" % (n, members, storage, list(src), f))
                    x[f] = want


# ---- 5. a member full of NaN, a member full of inf -------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("members", [3, 9, 64])
def test_nan_and_inf_members_poison_only_who_names_them(members, storage):
    rng = np.random.default_rng(5000 * storage + members)
    bad_nan, bad_inf = 1, members - 1
    for n in (6, 61):
        w = n + 2
        with solver(n, members, storage) as s:
            x = narrow(rng.uniform(0.5, 2.0, (members, w, w)).astype(F32), storage)
            x[bad_nan] = np.nan
            x[bad_inf] = np.inf
            for case in range(3):
                t = rng.uniform(0.25, 1.0, (members, members)).astype(F32)
                t[bad_nan] = rng.choice([0.0, -0.0], members)          # weight 0, either sign: they change nobody
                t[bad_inf] = rng.choice([0.0, -0.0], members)
                named_nan = named_inf = empty = ()
                if case >= 1:                                          # some columns name them
                    named_nan, named_inf = [0], [members - 2] if members > 3 else [2]
                    t[bad_nan, named_nan] = 0.5
                    t[bad_inf, named_inf] = -0.5
                if case == 2:                                          # a column of zeros
                    empty = [members // 2]
                    t[:, empty] = rng.choice([0.0, -0.0], (members, 1))
                s.upload_members(u=x)
                s.transform(t, fields=("u",))
                got = shown(s, "u")
                want = narrow(define(x, t), storage)
                same(got, want, "n=%d M=%d storage=%d case %d" % (n, members, storage, case))
                for m in range(members):
                    if m in empty:
                        assert not got[m].view(np.uint32).any(), "a column of zeros stores +0 (member %d)" % m
                    elif m in named_nan:
                        assert np.isnan(got[m]).all()
                    elif m in named_inf:
                        assert (got[m] == -np.inf).all()
                    else:
                        assert np.isfinite(got[m]).all(), "member %d was poisoned by a member of weight 0" % m


# ---- 6. lazy state ------------------------------------------------------------------------------------------------------------
def prepared(n, members, storage, fields, case):
    """a context in one of the lazy states, and the field the state is about"""
    s = solver(n, members, storage)
    s.upload_members(**fields)
    s.step(use_sources=(case == "scaled"))
    if case == "scaled":                   # fp16 storage: the pressure and the divergence of a step are held scaled
        return s, "u_prev"
    s.computeDivergenceAndPressure("u", "v", "dens_prev", "tmp0")       # its pressure is zero by definition: marked, not written
    if case == "zero":
        return s, "dens_prev"
    s.add_source("dens", "dens_prev", DT)  # ... and adding such a source is deferred: dens owes itself an increment
    return s, "dens"


@pytest.mark.parametrize("storage,case", [(0, "zero"), (0, "pending"), (1, "zero"), (1, "pending"), (1, "scaled")])
@pytest.mark.parametrize("members", [2, 5, 33])
def test_lazy_state_is_settled_first(members, storage, case):
    rng = np.random.default_rng(6000 * storage + members)
    for n in (13, 30):
        w = n + 2
        fields = {f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in MAIN}
        t = (rng.uniform(-1.0, 1.0, (members, members)) / np.sqrt(members)).astype(F32)
        t[rng.integers(0, members), rng.integers(0, members)] = 0
        what = "n=%d M=%d storage=%d %s" % (n, members, storage, case)
        a, f = prepared(n, members, storage, fields, case)
        b, _ = prepared(n, members, storage, fields, case)
        with a, b:
            names = (f, "v_prev") if case == "scaled" else (f,)
            a.transform(t, fields=names)
            for name in names:                                         # b: pack -> the definition -> unpack of all members
                b.upload_members(**{name: define(shown(b, name), t)})
            state = {name: shown(a, name) for name in MAIN}
            for name in MAIN:
                same(state[name], shown(b, name), "%s: %s against pack, define, unpack" % (what, name))
            if case == "zero":
                assert (state[f] == 0).all()
            with solver(n, members, storage) as fresh:                 # one more step: the record of the field is plain again
                fresh.upload_members(**state)
                for s in (a, b, fresh):
                    s.step(use_sources=True)
                for name in ("u", "v", "dens"):
                    want = shown(fresh, name)
                    same(shown(a, name), want, "%s: %s a step later, against a fresh context" % (what, name))
                    same(shown(b, name), want, "%s: %s a step later, pack / unpack against a fresh context" % (what, name))


# ---- 7. several fields, several calls ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("members", [2, 9, 64])
def test_fields_in_one_call_and_calls_back_to_back(members, storage):
    rng = np.random.default_rng(7000 * storage + members)
    n = 30
    w = n + 2
    x = {f: narrow(rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32), storage) for f in MAIN}
    t = mixed_weights(rng, members)
    with solver(n, members, storage) as a, solver(n, members, storage) as b:
        a.upload_members(**x)
        b.upload_members(**x)
        a.transform(t, fields=MAIN[:4])
        for f in MAIN[:4]:
            b.transform(t, fields=(f,))
        for f in MAIN:
            want = narrow(define(x[f], t), storage) if f in MAIN[:4] else x[f]
            same(shown(a, f), want, "M=%d storage=%d: %s, four fields in one call" % (members, storage, f))
            same(shown(b, f), want, "M=%d storage=%d: %s, one call per field" % (members, storage, f))
        # ten calls, ten matrices, no wait in between: more tables than the ring has slots
        ts = [(rng.uniform(-1.0, 1.0, (members, members)) * rng.integers(0, 4, (members, members)).clip(0, 1) / np.sqrt(members)).astype(F32)
              for _ in range(10)]
        a.upload_members(u=x["u"], v=x["v"])
        for k, tk in enumerate(ts):
            if k % 3 == 2:
                a.select(np.roll(np.arange(members), k), fields=("v", "u"))
            a.transform(tk, fields=("u", "v"))
        for f in ("u", "v"):
            y = x[f]
            for k, tk in enumerate(ts):
                if k % 3 == 2:
                    y = y[np.roll(np.arange(members), k)]
                y = narrow(define(y, tk), storage)
            same(shown(a, f), y, "M=%d storage=%d: %s after ten calls back to back" % (members, storage, f))


# ---- 8. refusals on a live context ----------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    from fluidsimulationcuda_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(8)
    n, members = 6, 5
    w = n + 2
    fields = {f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in MAIN}

    def ints(*v):
        return (C.c_int * len(v))(*v)

    def mat():
        return rng.uniform(-1.0, 1.0, (members, members)).astype(F32)

    def transform(hnd, ids, t, count=None):
        t = np.ascontiguousarray(t, F32)
        return lambda: L.fluid_transform_members(hnd, ids, len(ids) if count is None else count, t.ctypes.data_as(capi._MF))

    def select(hnd, ids, src, count=None):
        return lambda: L.fluid_select_members(hnd, ids, len(ids) if count is None else count, src)

    good_t, good_s, ids = mat(), ints(0, 1, 2, 3, 4), ints(0, 1, 2)
    with solver(n, members) as s, solver(n, members) as twin:
        for c in (s, twin):
            c.upload_members(**fields)
            c.step(use_sources=True)
            c.add_source("dens", "dens_prev", DT)                      # a lazy state that must survive the refusals
        hnd = s._h
        nan_t, inf_t = mat(), mat()
        nan_t[3, 1] = np.nan
        inf_t[0, 4] = -np.inf
        refused = [
            ("fluid_transform_members", lambda: L.fluid_transform_members(hnd, None, 1, good_t.ctypes.data_as(capi._MF)), (b"fields",)),
            ("fluid_transform_members", lambda: L.fluid_transform_members(hnd, ids, 3, None), (b"weights",)),
            ("fluid_transform_members", transform(hnd, ids, good_t, 0), (b"nfields 0",)),
            ("fluid_transform_members", transform(hnd, ids, good_t, 13), (b"nfields 13",)),
            ("fluid_transform_members", transform(hnd, ids, good_t, -1), (b"nfields -1",)),
            ("fluid_transform_members", transform(hnd, ints(0, 12), good_t), (b"bad field id 12", b"fields[1]")),
            ("fluid_transform_members", transform(hnd, ints(-1, 2), good_t), (b"bad field id -1", b"fields[0]")),
            ("fluid_transform_members", transform(hnd, ints(2, 1, 2), good_t), (b"field 2", b"twice", b"fields[0]", b"fields[2]")),
            ("fluid_transform_members", transform(hnd, ids, nan_t), (b"not finite", b"k = 3", b"m = 1")),
            ("fluid_transform_members", transform(hnd, ids, inf_t), (b"not finite", b"k = 0", b"m = 4")),
            ("fluid_select_members", lambda: L.fluid_select_members(hnd, None, 1, good_s), (b"fields",)),
            ("fluid_select_members", lambda: L.fluid_select_members(hnd, ids, 3, None), (b"source",)),
            ("fluid_select_members", select(hnd, ids, good_s, 0), (b"nfields 0",)),
            ("fluid_select_members", select(hnd, ids, good_s, 13), (b"nfields 13",)),
            ("fluid_select_members", select(hnd, ints(0, 99), good_s), (b"bad field id 99", b"fields[1]")),
            ("fluid_select_members", select(hnd, ints(5, 5), good_s), (b"field 5", b"twice")),
            ("fluid_select_members", select(hnd, ids, ints(0, 1, 5, 3, 4)), (b"source[2] = 5", b"[0, 5)")),
            ("fluid_select_members", select(hnd, ids, ints(0, 1, 2, 3, -1)), (b"source[4] = -1",)),
        ]
        for name, call, words in refused:
            L.fluid_synchronize(None)                   # (an unrelated message in between)
            assert call() == capi.E_INVALID, (name, words)
            msg = L.fluid_last_error()
            assert name.encode() in msg and all(word in msg for word in words), (name, words, msg)
        for f in capi.FIELD_NAMES:                      # every field of every member, and what they still owe themselves
            same(shown(s, f), shown(twin, f), "%s after the refusals" % f)
        for c in (s, twin):
            c.step(use_sources=True)
        for f in ("u", "v", "dens"):
            same(shown(s, f), shown(twin, f), "%s a step after the refusals" % f)
    # the cap: one member too many
    big = capi.TRANSFORM_MAX_MEMBERS + 1
    with solver(2, big) as s:
        x = rng.uniform(-1.0, 1.0, (big, 4, 4)).astype(F32)
        s.upload_members(u=x)
        t = np.eye(big, dtype=F32)
        for name, call in (("fluid_transform_members", transform(s._h, ints(0), t)),
                           ("fluid_select_members", select(s._h, ints(0), ints(*range(big))))):
            assert call() == capi.E_INVALID, name
            msg = L.fluid_last_error()
            assert name.encode() in msg and b"65" in msg and b"64" in msg, msg
        same(shown(s, "u"), x, "u after the refused transform of 65 members")
    with solver(2, capi.TRANSFORM_MAX_MEMBERS) as s:    # ... and the last count that works
        x = rng.uniform(-1.0, 1.0, (64, 4, 4)).astype(F32)
        s.upload_members(u=x)
        s.select(np.arange(64)[::-1], fields=("u",))
        same(shown(s, "u"), x[::-1], "64 members reversed")
    # row slabs
    with F().FluidSolver(n, rank=0, nranks=2) as s:
        one, zero = (C.c_float * 1)(1.0), ints(0)
        for name, call in (("fluid_transform_members", lambda: L.fluid_transform_members(s._h, ints(0), 1, one)),
                           ("fluid_select_members", lambda: L.fluid_select_members(s._h, ints(0), 1, zero))):
            assert call() == capi.E_INVALID, name
            msg = L.fluid_last_error()
            assert name.encode() in msg and b"slab" in msg, (name, msg)


# ---- 9. member 63 at least 2^32 bytes behind member 0 ------------------------------------------------------------------------------
def test_members_past_4_gib():
    """The kernel takes no index-width template: member and row bases are 64-bit scalar arithmetic, and this is the one
    place where they can go wrong -- the smallest N whose 64th fp32 member starts 2^32 bytes or more behind the first."""
    import torch
    from fluidsimulationcuda_amd import capi
    L = capi.lib()
    members = 64

    def field_floats(n):
        pitch, xoff, ff = C.c_int(), C.c_int(), C.c_size_t()
        assert L.fluid_layout(n, C.byref(pitch), C.byref(xoff), C.byref(ff)) == 0
        return ff.value

    n = next(n for n in range(3900, 4200) if (members - 1) * field_floats(n) * 4 >= 1 << 32)
    assert (members - 1) * field_floats(n - 1) * 4 < 1 << 32
    w = n + 2
    arena = L.fluid_arena_bytes_ensemble(n, 0, members)
    free, total = torch.cuda.mem_get_info()
    if free < arena + (1 << 30):
        pytest.skip("n=%d, M=64 needs an arena of %.1f GB, %.1f GB of %.1f GB are free" % (n, arena / 1e9, free / 1e9, total / 1e9))
    rng = np.random.default_rng(9)
    base = F32(0.75)
    marked = {0: None, 31: None, 63: None}
    rows = np.array([0, 1, w // 2, w - 2, w - 1])
    cols = np.array([0, 1, 2, 63, 64, 255, 256, w // 2, w - 3, w - 2, w - 1])
    with solver(n, members) as s:
        s.fill("u", float(base))
        for m in marked:
            a = np.full((w, w), base, F32)
            a[np.ix_(rows, cols)] = rng.uniform(-4.0, 4.0, (rows.size, cols.size)).astype(F32)
            marked[m] = a
            s.upload(member=m, u=a)

        def sampled(x):              # every member at the sampled cells, from what is known of them
            return np.stack([(x[m] if m in x else np.full((w, w), base, F32))[np.ix_(rows, cols)] for m in range(members)])

        x = sampled(marked)
        src = rng.integers(0, members, members)                        # a sparse call: a selection
        src[[0, 5, 40, 63]] = [63, 0, 31, 0]
        s.select(src, fields=("u",))
        x = define(x, onehot(src))
        for m in (0, 5, 31, 40, 63):
            same(s.download("u", member=m)[np.ix_(rows, cols)], x[m], "member %d after the selection" % m)
        t = rng.uniform(-1.0, 1.0, (members, members)).astype(F32)     # a dense one
        assert t.all()
        s.transform(t, fields=("u",))
        x = define(x, t)
        for m in (0, 31, 63):
            got = s.download("u", member=m)
            same(got[np.ix_(rows, cols)], x[m], "member %d after the dense transform" % m)
            # away from the marked cells every old member held `base`: whole rows between the sampled ones
            plain = define(np.full((members, 1), base, F32), t)[m, 0]
            for row in (7, w // 3, w - 9):
                same(got[row], np.full(w, plain, F32), "member %d row %d after the dense transform" % (m, row))
