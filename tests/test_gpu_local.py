"""GPU: localised updates -- fluid_transform_members_local / fluid_taper_gaspari_cohn (include/fluid_amd.h, "localised
updates"): the increment of a transform under a per-cell taper, over a box of cells, in place: X' = X + g o (X D).

Every expected value comes from `define_local` below, the header's definition in numpy: per new member a loop over the old
members k in increasing order, in double, over the non-zero increments only; p = g * s rounded once, y = x_m + p rounded
once, one rounding to float -- applied to what download_members (the pack) showed before the call -- then `narrow` (fp16
storage: one more rounding to nearest even).  Cells with g == 0, cells outside the box and members without a term keep
what they held.  Everything is compared bit for bit; a NaN is a NaN, its sign and payload are not compared.  The only
tolerance is the taper's own (part 8), derived there."""
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


def dev(a):
    """a host array as a float32 device tensor (None stays None)"""
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, F32)).cuda()


# ---- the definition ------------------------------------------------------------------------------------------------------
def define_local(x, d, g=None, box=None, order=None):
    """x: (M, W, W) float32, what the pack shows before the call; d: (M, M) float32, d[k, m] the weight of OLD member k in
    the INCREMENT of new member m; g: (W, W) float32 or None for 1; box: (row_lo, row_hi, col_lo, col_hi) or None for
    everything.  The new members, float32.  `order`: the order the old members are walked in (the contract: increasing)."""
    x, d = np.asarray(x, F32), np.asarray(d, F32)
    members, w = x.shape[0], x.shape[-1]
    xd = x.astype(np.float64)
    gd = np.ones((w, w), np.float64) if g is None else np.asarray(g, F32).astype(np.float64)
    stored = np.zeros((w, w), bool)
    r0, r1, c0, c1 = (0, w, 0, w) if box is None else box
    stored[r0:r1, c0:c1] = True
    if g is not None:
        stored &= np.asarray(g, F32) != 0                     # a zero of either sign: unchanged
    out = x.copy()
    with np.errstate(all="ignore"):
        for m in range(members):
            s = None
            for k in (range(members) if order is None else order):
                if d[k, m] != 0:                              # a zero of either sign takes no part
                    p = xd[k] * np.float64(d[k, m])           # exact: 24 + 24 bits
                    s = p if s is None else s + p
            if s is None:
                continue                                      # no term: member m is stored nowhere
            p = gd * s                                        # rounded once
            y = (xd[m] + p).astype(F32)                       # rounded once, then to float
            out[m] = np.where(stored, y, x[m])
    return out


def narrow(y, storage):
    with np.errstate(all="ignore"):
        return y.astype(np.float16).astype(F32) if storage else y


def same(got, want, what):
    """bit for bit, except that a NaN is any NaN"""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, what
    ok = np.where(np.isnan(want), np.isnan(got), got.view(np.uint32) == want.view(np.uint32))
    if not ok.all():
        at = tuple(np.argwhere(~ok)[0])
        raise AssertionError("%s: %d of %d values differ; first at %s: got %r (%08x) want %r (%08x)" % (
            what, int((~ok).sum()), ok.size, at, got[at], got.view(np.uint32)[at], want[at], want.view(np.uint32)[at]))


def same_bits(got, want, what):
    """every bit, NaN payloads included: for memory the call must not have stored"""
    got, want = np.ascontiguousarray(got, F32), np.ascontiguousarray(want, F32)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), "%s: %d of %d words changed; first at %s" % (what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))


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


def mixed_increments(rng, m, zeros=True):
    d = (np.ldexp(rng.uniform(1.0, 2.0, (m, m)), rng.integers(-10, 10, (m, m))) * rng.choice([-1.0, 1.0], (m, m))).astype(F32)
    if zeros:
        kind = rng.integers(0, 6, (m, m))
        d[kind == 0] = 0.0
        d[kind == 1] = -0.0
    return d


def random_taper(rng, w):
    """values in [0, 1], about a third of them exactly zero (of either sign), some exactly one"""
    g = rng.uniform(0.0, 1.0, (w, w)).astype(F32)
    kind = rng.integers(0, 12, (w, w))
    g[kind <= 2] = 0.0
    g[kind == 3] = -0.0
    g[kind == 4] = 1.0
    return g


def disc_taper(rng, w, radius):
    """non-zero inside a disc about the middle, exactly zero outside"""
    i, j = np.mgrid[0:w, 0:w]
    inside = (i - (w - 1) / 2.0) ** 2 + (j - (w - 1) / 2.0) ** 2 < radius ** 2
    return np.where(inside, rng.uniform(0.25, 1.0, (w, w)), 0.0).astype(F32), inside


def shown(s, field):
    """what the pack shows: every member of a field, the lazy state settled"""
    return s.download_members(field)


def apply_and_check(s, field, d, g, box, storage, what):
    """one call on one field against the definition applied to what the pack showed before; returns (before, after)"""
    before = shown(s, field)
    s.transform_local(d, taper=dev(g), box=box, fields=(field,))
    after = shown(s, field)
    same(after, narrow(define_local(before, d, g, box), storage), what)
    return before, after


# ---- 1. random increments, tapers and values ----------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("members", MEMBERS)
def test_random_increments_tapers_and_values(members, storage):
    rng = np.random.default_rng(1000 * storage + members)
    for n in SIZES:
        w = n + 2
        with solver(n, members, storage) as s:
            for zeros in (True, False):          # with zeros: the table with a mask; without: the table where every term is taken
                x = mixed_values(rng, (members, w, w), storage)
                s.upload_members(u=x)
                same(shown(s, "u"), narrow(x, storage), "n=%d M=%d: the upload" % (n, members))
                g = random_taper(rng, w)
                assert w < 20 or 0.2 < (g == 0).mean() < 0.5
                before, after = apply_and_check(s, "u", mixed_increments(rng, members, zeros), g, None, storage,
                                                "n=%d M=%d storage=%d zeros=%s" % (n, members, storage, zeros))
                same_bits(after[:, g == 0], before[:, g == 0], "n=%d M=%d: cells under a zero taper" % (n, members))


# ---- 2. boxes: a row of two blocks, every edge ----------------------------------------------------------------------------------
def test_boxes_across_two_blocks():
    rng = np.random.default_rng(2)
    n, members = 300, 5
    w = n + 2
    col_edges, row_edges = (0, 1, 255, 256, 257, w), (0, 1, w)
    boxes = [(r0, r1, c0, c1) for r0 in row_edges for r1 in row_edges if r0 < r1
             for c0 in col_edges for c1 in col_edges if c0 < c1]
    boxes += [(7, 7, 0, w), (0, w, 256, 256), (0, 0, 0, 0), (w, w, w, w)]          # empty ones
    boxes += [(0, 1, 0, 1), (w - 1, w, w - 1, w), (150, 151, 256, 257)]            # one cell
    assert len(boxes) == 3 * 15 + 7
    g = random_taper(rng, w)
    g_dev = dev(g)
    with solver(n, members) as s:
        x = rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32)
        s.upload_members(dens=x)
        for k, box in enumerate(boxes):
            d = (rng.uniform(-1.0, 1.0, (members, members)) / members).astype(F32)
            if k % 3:                                                              # (every third call takes the dense table)
                d[rng.integers(0, 3, (members, members)) == 0] = 0
            taper = None if k % 2 else g
            s.transform_local(d, taper=None if taper is None else g_dev, box=box, fields=("dens",))
            after = shown(s, "dens")
            same(after, define_local(x, d, taper, box), "n=%d M=%d box %s taper %s" % (n, members, box, taper is not None))
            outside = np.ones((w, w), bool)
            outside[box[0]:box[1], box[2]:box[3]] = False
            same_bits(after[:, outside], x[:, outside], "box %s: cells outside it" % (box,))
            if box[0] == box[1] or box[2] == box[3]:
                same_bits(after, x, "the empty box %s" % (box,))
            x = after


# ---- 3. untouched means untouched --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("members", [3, 9, 64])
def test_outside_the_taper_nothing_changes_with_nan_and_inf_members(members, storage):
    rng = np.random.default_rng(3000 * storage + members)
    bad_nan, bad_inf = 1, members - 1
    for n in (13, 61):
        w = n + 2
        g, inside = disc_taper(rng, w, 0.3 * w)
        assert inside.any() and not inside.all()
        with solver(n, members, storage) as s:
            x = narrow(rng.uniform(0.5, 2.0, (members, w, w)).astype(F32), storage)
            x[bad_nan] = np.nan
            x[bad_inf] = -np.inf
            s.upload_members(u=x)
            d = rng.uniform(0.25, 1.0, (members, members)).astype(F32)         # every member names the bad ones
            before, after = apply_and_check(s, "u", d, g, None, storage, "n=%d M=%d storage=%d" % (n, members, storage))
            same_bits(after[:, ~inside], before[:, ~inside], "n=%d M=%d storage=%d: outside the disc" % (n, members, storage))
            assert np.isnan(after[:, inside]).all(), "inf - inf and NaN reach every member inside the disc"
            assert np.isfinite(after[0][~inside]).all()


def scaled_case():
    """fp16 storage, N = 30, M = 5: after a step u_prev holds the pressure times a power of two (4 at this N)"""
    rng = np.random.default_rng(33)
    n, members = 30, 5
    w = n + 2
    g, inside = disc_taper(rng, w, 0.3 * w)
    fields = {f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in MAIN}
    d = (rng.uniform(-1.0, 1.0, (members, members)) / members).astype(F32)
    s = solver(n, members, storage=1)
    s.upload_members(**fields)
    s.step(use_sources=True)
    return s, d, g, inside


def test_outside_the_taper_a_scaled_fp16_field_shows_what_it_showed():
    """fp16 storage: after a step u_prev holds the pressure times a power of two, and some of what download_members shows
    of it (widen(h) / scale) is no half.  The call keeps the scale: outside the disc the values equal what download_members
    showed before the call, bit for bit; inside, the definition applied to what it showed, narrowed."""
    s, d, g, inside = scaled_case()
    with s:
        before = shown(s, "u_prev")
        assert before.any()
        print("scaled field: %d of %d values shown before the call are no halves" % (int((narrow(before, 1) != before).sum()), before.size))
        s.transform_local(d, taper=dev(g), fields=("u_prev",))
        after = shown(s, "u_prev")
        same_bits(after[:, ~inside], before[:, ~inside], "u_prev outside the disc")
        same(after[:, inside], narrow(define_local(before, d, g), 1)[:, inside], "u_prev inside the disc")
        # and the field goes on as the scaled field it was: a second call sees what the first one left
        s.transform_local(d, taper=dev(g), box=(3, 20, 5, 30), fields=("u_prev",))
        again = shown(s, "u_prev")
        stored = stored_cells(d, g, (3, 20, 5, 30), before.shape[-1])
        same(again, np.where(stored, narrow(define_local(after, d, g, (3, 20, 5, 30)), 1), after), "u_prev after a second call")


# ---- 4. null taper, zero taper, zero increments ---------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("members", [1, 5, 33])
def test_null_taper_is_ones_and_zeros_change_nothing(members, storage):
    rng = np.random.default_rng(4000 * storage + members)
    for n in (6, 61):
        w = n + 2
        x = narrow(mixed_values(rng, (members, w, w), storage), storage)
        x[members // 2, 1, 2] = np.nan
        d = mixed_increments(rng, members)
        with solver(n, members, storage) as a, solver(n, members, storage) as b:
            a.upload_members(v=x)
            b.upload_members(v=x)
            a.transform_local(d, fields=("v",))
            b.transform_local(d, taper=dev(np.ones((w, w), F32)), fields=("v",))
            got = shown(a, "v")
            same(got, narrow(define_local(x, d), storage), "n=%d M=%d storage=%d: the null taper" % (n, members, storage))
            finite = ~np.isnan(got)
            same_bits(shown(b, "v")[finite], got[finite], "n=%d M=%d storage=%d: all ones against the null taper" % (n, members, storage))
            assert np.isnan(shown(b, "v")[~finite]).all()
            # a taper of zeros of either sign; increments of zeros of either sign, with a member of NaN present
            a.upload_members(v=x)
            before = shown(a, "v")
            a.transform_local(d, taper=dev(rng.choice([0.0, -0.0], (w, w))), fields=("v",))
            same_bits(shown(a, "v"), before, "n=%d M=%d storage=%d: a taper of zeros" % (n, members, storage))
            x[0] = np.nan
            a.upload_members(v=x)
            before = shown(a, "v")
            assert np.isnan(before[0]).all()
            a.transform_local(rng.choice([0.0, -0.0], (members, members)), taper=dev(random_taper(rng, w)), fields=("v",))
            same_bits(shown(a, "v"), before, "n=%d M=%d storage=%d: increments of zeros" % (n, members, storage))


# ---- 5. the order is pinned ---------------------------------------------------------------------------------------------------
def order_data(rng, members, w, storage):
    """The construction of tests/test_gpu_transform.py, on the increments.  Members 0 and 2 hold +b and -b, the others
    values in (-1, 1); the increments are signed powers of two, row 2 equal to row 0.  The products of members 0 and 2 lie
    in 2^56 .. 2^90 and cancel exactly: in member order everything added between them is absorbed and everything after
    them survives, in any other order something else does.  fp32 storage: b itself is in 2^56 .. 2^90 and the increments
    in 2^-3 .. 2^3; fp16 storage cannot hold such a b, so b is in 2^8 .. 2^14 and rows 0 and 2 carry the other 2^50 .. 2^74."""
    x = narrow(rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32), storage)
    lo, hi = (8, 15) if storage else (56, 91)
    b = np.ldexp(1.0, rng.integers(lo, hi, (w, w))).astype(F32)
    x[0], x[2] = b, -b
    d = (np.ldexp(1.0, rng.integers(-3, 4, (members, members))) * rng.choice([-1.0, 1.0], (members, members))).astype(F32)
    if storage:
        d[0] = np.ldexp(d[0], rng.integers(50, 72, members)).astype(F32)
    d[2] = d[0]
    return x, d


@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("members", [m for m in MEMBERS if m >= 4])
def test_the_order_is_pinned(members, storage):
    rng = np.random.default_rng(5000 * storage + members)
    small = [m for m in range(members) if m not in (0, 2)]       # the members whose own value does not drown the increment
    for n in SIZES:
        w = n + 2
        x, d = order_data(rng, members, w, storage)
        want = define_local(x, d)
        # on the CPU first: the data shows the order -- the reversed member order changes (nearly) every cell
        flip = define_local(x, d, order=range(members - 1, -1, -1))
        differs = (flip[small].view(np.uint32) != want[small].view(np.uint32)).mean()
        assert differs >= 0.9, "n=%d M=%d: the reversed sum differs in only %.0f%% of the cells" % (n, members, 100 * differs)
        with solver(n, members, storage) as s:
            s.upload_members(dens=x)
            same(shown(s, "dens"), x, "n=%d M=%d: the data is representable" % (n, members))
            s.transform_local(d, fields=("dens",))
            same(shown(s, "dens"), narrow(want, storage), "n=%d M=%d storage=%d: member order" % (n, members, storage))


# ---- 6. in place ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("members", [2, 3, 9, 64])
def test_a_cyclic_shift_in_place(members, storage):
    """D = P - I with a cyclic shift P and taper 1: new member m = x_m + (x_{m-1} - x_m), what an out-of-place call gives --
    a kernel that stored member m before reading it for member m + 1 would hand the new value on."""
    rng = np.random.default_rng(6000 * storage + members)
    for shift in (1, -1):
        perm = np.zeros((members, members), F32)
        perm[np.roll(np.arange(members), shift), np.arange(members)] = 1          # new member m := old member (m + shift) % M
        d = perm - np.eye(members, dtype=F32)
        for n in (6, 61):
            w = n + 2
            x = narrow(rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32), storage)
            with solver(n, members, storage) as s:
                s.upload_members(u=x)
                s.transform_local(d, fields=("u",))
                got = shown(s, "u")
                same(got, narrow(define_local(x, d), storage), "n=%d M=%d storage=%d shift %d" % (n, members, storage, shift))
                with np.errstate(all="ignore"):                                      # the out-of-place model, written out
                    xd = x.astype(np.float64)
                    moved = xd[np.roll(np.arange(members), shift)]
                    same(got, narrow((xd + (moved - xd)).astype(F32), storage), "n=%d M=%d shift %d: out of place" % (n, members, shift))


# ---- 7. lazy state ------------------------------------------------------------------------------------------------------------
def prepared(n, members, storage, fields, case):
    """a context in one of the lazy states, and the fields the call is made on"""
    s = solver(n, members, storage)
    if case == "fill":
        s.upload_members(**fields)
        s.fill("dens", 0.375)
        s.fill("u_prev", 0.0)
        return s, ("dens", "u_prev")
    s.upload_members(**fields)
    s.step(use_sources=True)                  # fp16 storage: u_prev and v_prev now hold the pressure and the divergence scaled
    if case == "step":
        return s, MAIN
    s.computeDivergenceAndPressure("u", "v", "dens_prev", "tmp0")       # its pressure is zero by definition: marked, not written
    s.add_source("dens", "dens_prev", DT)     # ... and adding such a source is deferred: dens owes itself an increment
    return s, ("dens", "dens_prev")


def stored_cells(d, g, box, w):
    """(M, W, W) bool: the cells the definition stores -- inside the box, taper non-zero, the member has a term"""
    cells = np.zeros((w, w), bool)
    cells[box[0]:box[1], box[2]:box[3]] = True
    cells &= np.asarray(g, F32) != 0
    return (np.asarray(d, F32) != 0).any(axis=0)[:, None, None] & cells


@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("case", ["fill", "step", "pending"])
@pytest.mark.parametrize("members", [2, 5, 33])
def test_lazy_state_is_settled_first(members, storage, case):
    """The call against the definition applied to what a twin context shows (the pack settles what the field owes itself
    and divides a scale back): stored cells hold narrow(y), every other cell shows exactly what it showed -- in an fp16
    field held at a scale too, where that need not be a half."""
    rng = np.random.default_rng(7000 * storage + members)
    for n in (13, 30):
        w = n + 2
        fields = {f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in MAIN}
        d = (rng.uniform(-1.0, 1.0, (members, members)) / np.sqrt(members)).astype(F32)
        d[rng.integers(0, members), rng.integers(0, members)] = 0
        g = random_taper(rng, w)
        box = (1, w - 2, 2, w)
        what = "n=%d M=%d storage=%d %s" % (n, members, storage, case)
        a, names = prepared(n, members, storage, fields, case)
        b, _ = prepared(n, members, storage, fields, case)
        with a, b:
            a.transform_local(d, taper=dev(g), box=box, fields=names)
            state = {name: shown(a, name) for name in MAIN}
            for name in MAIN:
                before = shown(b, name)                                # the twin: the call never ran there
                want = before
                if name in names:
                    want = np.where(stored_cells(d, g, box, w), narrow(define_local(before, d, g, box), storage), before)
                same(state[name], want, "%s: %s against the definition on what the twin shows" % (what, name))
                if name not in names:
                    same_bits(state[name], before, "%s: %s was not listed" % (what, name))
            # one more step: the record of every field is right again.  fp16 storage: without sources, so that the step reads
            # no *_prev field -- a fresh context cannot be given the scaled ones bit for bit (an upload rounds to halves)
            with solver(n, members, storage) as fresh:
                fresh.upload_members(**state)
                for s in (a, fresh):
                    s.step(use_sources=not storage)
                for name in ("u", "v", "dens"):
                    same(shown(a, name), shown(fresh, name), "%s: %s a step later, against a fresh context" % (what, name))


# ---- 8. the taper --------------------------------------------------------------------------------------------------------------
def gaspari_cohn(w, col, row, c):
    """the formula as the header states it, in double: (g, r) over the (w, w) cells"""
    i, j = np.mgrid[0:w, 0:w].astype(np.float64)
    col, row, c = (np.float64(F32(v)) for v in (col, row, c))
    r = np.sqrt((j - col) ** 2 + (i - row) ** 2) / c
    with np.errstate(all="ignore"):
        near = 1 - 5 * r ** 2 / 3 + 5 * r ** 3 / 8 + r ** 4 / 2 - r ** 5 / 4
        far = 4 - 5 * r + 5 * r ** 2 / 3 + 5 * r ** 3 / 8 - r ** 4 / 2 + r ** 5 / 12 - 2 / (3 * r)
    g = np.where(r <= 1, near, np.where(r < 2, far, 0.0))
    return np.clip(g, 0.0, 1.0), r


def taper_cases(n):
    centres = [(n // 2 + 1, (n + 1) // 2), (n / 2 + 0.5, n / 3 + 0.75), (0.5, 0.5), (n + 0.5, n + 0.5), (0.5, n + 0.5), (n // 3 + 1, n + 0.5),
               (1, n)]
    return [(col, row, c) for col, row in centres for c in (0.3, 1, 2.5, n)]


@pytest.mark.parametrize("n", [1, 13, 30, 300])
def test_the_taper(n):
    w = n + 2
    with solver(n, 2) as s:
        for col, row, c in taper_cases(n):
            what = "n=%d centre (%g, %g) c=%g" % (n, col, row, c)
            t, box = s.taper_gaspari_cohn(col, row, c)
            got = t.cpu().numpy()
            assert got.dtype == F32 and got.shape == (w, w), what
            want, r = gaspari_cohn(w, col, row, c)
            # one rounding to float (2^-24 relative) on top of the double evaluation of a polynomial whose terms stay below 32
            err = np.abs(got.astype(np.float64) - want)
            bound = 2.0 ** -24 * np.abs(want) + 1e-13
            assert (err <= bound).all(), "%s: error %g over the bound at %s" % (what, (err - bound).max(), np.unravel_index((err - bound).argmax(), err.shape))
            assert (got[r >= 2] == 0).all(), "%s: non-zero at r >= 2" % what
            assert (got >= 0).all() and (got <= 1).all(), what
            if float(col).is_integer() and float(row).is_integer():
                assert got[int(row), int(col)] == 1, what
            # the box: every non-zero cell, and at most one cell more per side than the tight box of r < 2
            r0, r1, c0, c1 = box
            assert 0 <= r0 <= r1 <= w and 0 <= c0 <= c1 <= w, (what, box)
            outside = np.ones((w, w), bool)
            outside[r0:r1, c0:c1] = False
            assert not got[outside].any(), "%s: a non-zero cell outside the box %s" % (what, box)
            rows, cols = np.nonzero(r < 2)
            if rows.size:
                assert r0 >= rows.min() - 1 and r1 <= rows.max() + 2 and c0 >= cols.min() - 1 and c1 <= cols.max() + 2, (what, box)
            else:
                assert r0 == r1 or c0 == c1, (what, box)


# ---- 9. refusals on a live context ----------------------------------------------------------------------------------------------
def hip_runtime():
    """the HIP runtime this process already holds (the one libfluid_amd.so runs on)"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime is loaded")


def test_refusals_change_nothing():
    import torch
    from fluidsimulationcuda_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(9)
    n, members = 6, 5
    w = n + 2
    fields = {f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in MAIN}
    hip = hip_runtime()
    exact = C.c_void_p()
    size = 1 << 20
    assert hip.hipMalloc(C.byref(exact), C.c_size_t(size)) == 0
    short = exact.value + size - w * w * 4 + 4          # device memory whose allocation ends one float short of a taper
    fits = exact.value + size - w * w * 4               # ... and a taper that ends with its allocation
    host = np.ones((w, w), F32)
    taper = torch.full((w, w), 0.5, dtype=torch.float32, device="cuda")
    out = torch.full((w, w), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def ints(*v):
        return (C.c_int * len(v))(*v)

    def mat():
        return rng.uniform(-1.0, 1.0, (members, members)).astype(F32)

    def local(hnd, ids, d, count=None, taper_p=None, box=None):
        d = np.ascontiguousarray(d, F32)
        return lambda: L.fluid_transform_members_local(hnd, ids, len(ids) if count is None else count, d.ctypes.data_as(capi._MF), taper_p, box)

    def gc(hnd, col=3.0, row=3.0, c=1.0, out_p=None, box=None):
        return lambda: L.fluid_taper_gaspari_cohn(hnd, col, row, c, out.data_ptr() if out_p is None else out_p, box)

    good, ids = mat(), ints(0, 1, 2)
    try:
        with solver(n, members) as s, solver(n, members) as twin:
            for c in (s, twin):
                c.timing_enable(True)
                c.upload_members(**fields)
                c.step(use_sources=True)
                c.add_source("dens", "dens_prev", DT)                      # a lazy state that must survive the refusals
            hnd = s._h
            nan_d, inf_d = mat(), mat()
            nan_d[3, 1] = np.nan
            inf_d[0, 4] = -np.inf
            one, two = "fluid_transform_members_local", "fluid_taper_gaspari_cohn"
            refused = [
                (one, lambda: L.fluid_transform_members_local(hnd, None, 1, good.ctypes.data_as(capi._MF), None, None), (b"fields",)),
                (one, lambda: L.fluid_transform_members_local(hnd, ids, 3, None, None, None), (b"increments",)),
                (one, local(None, ids, good), (b"null context",)),
                (one, local(hnd, ids, good, 0), (b"nfields 0",)),
                (one, local(hnd, ids, good, 13), (b"nfields 13",)),
                (one, local(hnd, ids, good, -1), (b"nfields -1",)),
                (one, local(hnd, ints(0, 12), good), (b"bad field id 12", b"fields[1]")),
                (one, local(hnd, ints(-1, 2), good), (b"bad field id -1", b"fields[0]")),
                (one, local(hnd, ints(2, 1, 2), good), (b"field 2", b"twice", b"fields[0]", b"fields[2]")),
                (one, local(hnd, ids, nan_d), (b"not finite", b"k = 3", b"m = 1")),
                (one, local(hnd, ids, inf_d), (b"not finite", b"k = 0", b"m = 4")),
                (one, local(hnd, ids, good, box=ints(-1, 2, 0, 2)), (b"box[0] = -1", b"row_lo")),
                (one, local(hnd, ids, good, box=ints(0, w + 1, 0, 2)), (b"box[1] = %d" % (w + 1), b"row_hi")),
                (one, local(hnd, ids, good, box=ints(0, 2, -3, 2)), (b"box[2] = -3", b"col_lo")),
                (one, local(hnd, ids, good, box=ints(0, 2, 0, w + 5)), (b"box[3] = %d" % (w + 5), b"col_hi")),
                (one, local(hnd, ids, good, box=ints(3, 2, 0, 2)), (b"box[0] = 3", b"box[1] = 2")),
                (one, local(hnd, ids, good, box=ints(0, 2, 5, 4)), (b"box[2] = 5", b"box[3] = 4")),
                (one, local(hnd, ids, good, taper_p=host.ctypes.data), (b"taper_dev", b"not device memory")),
                (one, local(hnd, ids, good, taper_p=short), (b"taper_dev", b"allocation ends")),
                (one, local(hnd, ids, good, taper_p=fits + 2), (b"taper_dev",)),                  # (misaligned, and short)
                (two, gc(hnd, out_p=0), (b"out_dev",)),
                (two, gc(None), (b"null context",)),
                (two, gc(hnd, col=float("nan")), (b"col",)),
                (two, gc(hnd, col=0.25), (b"col",)),
                (two, gc(hnd, col=n + 0.75), (b"col",)),
                (two, gc(hnd, row=float("inf")), (b"row",)),
                (two, gc(hnd, row=0.0), (b"row",)),
                (two, gc(hnd, row=n + 1.0), (b"row",)),
                (two, gc(hnd, c=0.0), (b"c =",)),
                (two, gc(hnd, c=-1.0), (b"c =",)),
                (two, gc(hnd, c=float("nan")), (b"c =",)),
                (two, gc(hnd, c=float("inf")), (b"c =",)),
                (two, gc(hnd, out_p=host.ctypes.data), (b"out_dev", b"not device memory")),
                (two, gc(hnd, out_p=short), (b"out_dev", b"allocation ends")),
            ]
            for name, call, words in refused:
                L.fluid_synchronize(None)                   # (an unrelated message in between)
                assert call() == capi.E_INVALID, (name, words)
                msg = L.fluid_last_error()
                assert name.encode() in msg and all(word in msg for word in words), (name, words, msg)
            s.synchronize()
            assert (out.cpu().numpy() == 7.0).all() and (taper.cpu().numpy() == 0.5).all()
            ta, tb = s.timing_read(reset=False), twin.timing_read(reset=False)
            assert ta == {**tb, **{k: ta[k] for k in ta if k.endswith("_ms")}}             # every count; the times are times
            for f in capi.FIELD_NAMES:                      # every field of every member, and what they still owe themselves
                same(shown(s, f), shown(twin, f), "%s after the refusals" % f)
            for c in (s, twin):
                c.step(use_sources=True)
            for f in ("u", "v", "dens"):
                same(shown(s, f), shown(twin, f), "%s a step after the refusals" % f)
            # what is not refused: a taper that ends with its allocation, written and then read there
            box = ints(9, 9, 9, 9)
            assert L.fluid_taper_gaspari_cohn(hnd, 3.0, 4.0, 1.5, fits, box) == capi.OK
            assert L.fluid_transform_members_local(hnd, ids, 3, good.ctypes.data_as(capi._MF), fits, box) == capi.OK
            s.synchronize()
            assert list(box) != [9, 9, 9, 9]
        # the cap: one member too many
        big = capi.TRANSFORM_MAX_MEMBERS + 1
        with solver(2, big) as s:
            x = rng.uniform(-1.0, 1.0, (big, 4, 4)).astype(F32)
            s.upload_members(u=x)
            assert local(s._h, ints(0), np.eye(big, dtype=F32))() == capi.E_INVALID
            msg = L.fluid_last_error()
            assert b"fluid_transform_members_local" in msg and b"65" in msg and b"64" in msg, msg
            same(shown(s, "u"), x, "u after the refused call of 65 members")
        # row slabs
        with F().FluidSolver(n, rank=0, nranks=2) as s:
            one_f = (C.c_float * 1)(1.0)
            for name, call in (("fluid_transform_members_local", lambda: L.fluid_transform_members_local(s._h, ints(0), 1, one_f, None, None)),
                               ("fluid_taper_gaspari_cohn", lambda: L.fluid_taper_gaspari_cohn(s._h, 1.0, 1.0, 1.0, out.data_ptr(), None))):
                assert call() == capi.E_INVALID, name
                msg = L.fluid_last_error()
                assert name.encode() in msg and b"slab" in msg, (name, msg)
    finally:
        assert hip.hipFree(exact) == 0


# ---- 10. one localised analysis, end to end ---------------------------------------------------------------------------------------
def etkf_increments(gram, rhs, members):
    """D = T - I of the ensemble transform Kalman filter, from the observation-space Gram matrix C = A^T A of the scaled
    anomalies and rhs = A^T d: Pa = ((M - 1) I + C)^-1, mean weights Pa rhs, anomaly weights sqrt((M - 1) Pa)."""
    vals, vecs = np.linalg.eigh((members - 1) * np.eye(members) + gram)
    pa = (vecs / vals) @ vecs.T
    wa = (vecs * np.sqrt((members - 1) / vals)) @ vecs.T
    centre = np.eye(members) - np.full((members, members), 1.0 / members)
    t = np.full((members, members), 1.0 / members) + centre @ ((pa @ rhs)[:, None] + wa)
    return (t - np.eye(members)).astype(F32)


def test_one_localised_analysis():
    rng = np.random.default_rng(10)
    n, members = 30, 8
    w = n + 2
    i, j = np.mgrid[0:w, 0:w]
    truth = np.sin(0.2 * i) * np.cos(0.3 * j)
    x = (truth + 0.3 * rng.standard_normal((members, w, w))).astype(F32)
    cols = np.array([11.0, 12.5, 13.25, 14.0, 12.0], F32)
    rows = np.array([17.0, 18.5, 16.75, 18.0, 19.5], F32)
    with solver(n, members) as s:
        s.upload_members(dens=x)
        s.set_observation_points(cols, rows)
        obs = (np.sin(0.2 * rows) * np.cos(0.3 * cols) + 0.05 * rng.standard_normal(5)).astype(F32)
        gram, rhs, _ = s.observation_gram("dens", obs=obs, inv_sigma=np.full(5, 1 / 0.05, F32))
        d = etkf_increments(gram, rhs, members)
        assert np.isfinite(d).all() and np.abs(d).max() > 1e-3
        taper, box = s.taper_gaspari_cohn(float(cols.mean()), float(rows.mean()), 4.0)
        g = taper.cpu().numpy()
        assert 0 < (g != 0).sum() < w * w and (box[1] - box[0]) * (box[3] - box[2]) < w * w
        before = shown(s, "dens")
        s.transform_local(d, taper=taper, box=box, fields=("dens",))
        after = shown(s, "dens")
        same(after, define_local(before, d, g, box), "the localised analysis")
        same(define_local(before, d, g, box), define_local(before, d, g), "the box holds the taper's support")
        same_bits(after[:, g == 0], before[:, g == 0], "members outside the support")
        spread = lambda a: a.astype(np.float64).var(axis=0)
        assert np.array_equal(spread(after)[g == 0], spread(before)[g == 0]), "the spread outside the support"
        inside = g > 0.5
        assert spread(after)[inside].mean() < spread(before)[inside].mean(), "the analysis tightens the ensemble near the observations"
