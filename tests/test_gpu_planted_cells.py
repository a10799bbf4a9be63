"""GPU: the kernels that answer with ONE number or ONE decision -- k_absmax2, k_residual, k_subtract_gradient_max with
k_max_partials, the launch_absmax2 of a slab's stand-alone advection, division mode 5's sticky non-finite test -- must see
every cell.  On random or smooth fields a dropped cell does not change such an answer, so each test here starts from a
field on which the answer is known, plants ONE cell that alone changes it, moves that cell over every class of position
the kernel's indexing tells apart (tests/test_planted_positions.py: first / last row and column, each lane of the masked
last vector, both sides of the 256-column, 1024-column and 1024-row seams, window and strip seams of the fused kernel),
and compares with a numpy definition of the same number bit for bit.  Ghost cells hold values far larger than anything
planted and the pad floats of the layout are poisoned, so a kernel that counted one of them fails as well.

Failures of a sweep are collected and reported together: which cells fail names the class that was dropped."""
import numpy as np
import pytest

from conftest import assert_bit_equal, rnd, tb_schedule
from test_gpu_ensemble_reduce import solver, stored
from test_gpu_lazy_state import absmax32, arena_solver, residual32
from test_gpu_slab import run_ranks, single, synthetic
from test_planted_positions import COL_PERIODS, LARGE, ROW_PERIODS, SMALL, corners, lines, positions

pytestmark = pytest.mark.gpu
F32 = np.float32
DT = 0.016
GHOST = F32(1024)             # the ghost ring: +-1024, far larger than any value planted for a maximum over the interior
POISON = 3e4                  # the pad floats: finite (fmaxf drops a NaN), representable in fp32 and in fp16
PLANT = F32(64)               # |u|, |v| <= 1 elsewhere
RPLANT = F32(16384)           # a right-hand side (or ghost) cell no other residual term comes near: those stay below 4200
COEFFS = ((1.0, 4.0), (0.7, 3.3))
SIZES = list(SMALL) + sorted(LARGE)
STORAGE = pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])


def u32(a):
    return np.asarray(a, F32).view(np.uint32)


def same_word(got, want):
    return u32(got) == u32(want)


def report(bad, what):
    assert not bad, "%s: %d placements fail; the first: %s" % (what, len(bad), "; ".join(str(b) for b in bad[:12]))


def base_field(rng, n, storage):
    """interior: random multiples of 2^-8 in [-1, 1] (exact in fp16); ghost ring: +-1024"""
    f = (rng.integers(-256, 257, size=(n + 2, n + 2)).astype(F32) / F32(256)).astype(F32)
    ring = GHOST * rng.choice(np.array([-1, 1], F32), size=(n + 2, n + 2))
    inner = np.zeros((n + 2, n + 2), bool)
    inner[1:-1, 1:-1] = True
    f = np.where(inner, f, ring).astype(F32)
    assert np.array_equal(stored(f, storage), f)
    return f


def pad_views(s, name):
    """the floats of a field's rows that are no cell: left of column 0 and past column n + 1 up to the pitch, through
    fluid_field_ptr (the arena is a torch tensor: test_gpu_slab._init_fake)"""
    p = s.field_ptr(name)
    s.synchronize()
    slot, rem = divmod(p - s.arena.data_ptr(), s._fb)
    assert rem == 0
    rows = s._views[slot]
    return rows[:, :s.xoff], rows[:, s.xoff + s.n + 2:]


def poison_pads(s, names):
    import torch
    for name in names:
        for pad in pad_views(s, name):
            pad.fill_(POISON)
    torch.cuda.synchronize()


def pads_still_poisoned(s, names):
    for name in names:
        left, right = pad_views(s, name)
        assert left.numel() > 0 and right.numel() > 0
        assert bool((left == POISON).all()) and bool((right == POISON).all()), "the pads of %s were overwritten" % name


def planted_rows(s, name, field, cells, values):
    """for every cell and value: the field with that one cell replaced, on the device (one row upload per placement; a row
    is put back when the sweep leaves it) -- yields (cell, value) with the plant in place"""
    work = field.copy()
    for k, (i, j) in enumerate(cells):
        for value in values:
            work[i, j] = value
            s.upload_rows(name, work, i, i + 1)
            yield (i, j), value
        work[i, j] = field[i, j]
        if k + 1 == len(cells) or cells[k + 1][0] != i:
            s.upload_rows(name, work, i, i + 1)


# ---- 1. absmax_velocity and residual, one context --------------------------------------------------------------------------
def cells_of(n):
    return positions(n, COL_PERIODS, ROW_PERIODS)


@STORAGE
@pytest.mark.parametrize("n", SIZES)
def test_absmax_sees_every_cell_and_nothing_else(n, storage):
    rng = np.random.default_rng(1000 + n)
    u, v = base_field(rng, n, storage), base_field(rng, n, storage)
    s = arena_solver(n, storage=storage)
    try:
        s.upload(u=u, v=v)
        poison_pads(s, ("u", "v"))
        # no plant: the interior's maximum -- neither the ghost ring (1024) nor the pads (3e4) show
        assert same_word(s.absmax_velocity("u", "v"), absmax32(u, v)), (s.absmax_velocity("u", "v"), absmax32(u, v))
        assert absmax32(u, v) <= 1
        bad = []
        for name, f in (("u", u), ("v", v)):
            for cell, value in planted_rows(s, name, f, cells_of(n), (PLANT, -PLANT)):
                got = s.absmax_velocity("u", "v")
                if not same_word(got, PLANT):
                    bad.append((name, cell, float(value), got))
        report(bad, "absmax_velocity, n=%d: (field, (row, column), planted, returned)" % n)
        assert same_word(s.absmax_velocity("u", "v"), absmax32(u, v))
        assert_bit_equal(s.download("u"), u, "u put back")
        assert_bit_equal(s.download("v"), v, "v put back")
        pads_still_poisoned(s, ("u", "v"))
    finally:
        s.close()


class ResidualModel:
    """residual32 with one right-hand-side cell replaced, without a pass over the field per placement: only that cell's
    term changes, the maximum over all other terms is the base's largest term or, for the cell that holds it, the second
    largest.  The same float32 expressions as residual32, term by term."""

    def __init__(self, x, x0, alpha, beta):
        nb = ((x[1:-1, :-2] + x[1:-1, 2:]) + x[:-2, 1:-1]) + x[2:, 1:-1]
        self.lhs = F32(beta) * x[1:-1, 1:-1] - F32(alpha) * nb
        terms = np.abs(self.lhs - x0[1:-1, 1:-1])
        assert self.lhs.dtype == F32 and terms.dtype == F32
        self.top = np.unravel_index(np.argmax(terms), terms.shape)
        self.first = terms[self.top]
        terms[self.top] = 0
        self.second = terms.max() if terms.size > 1 else F32(0)

    def planted(self, i, j, value):
        others = self.second if (i - 1, j - 1) == self.top else self.first
        return F32(np.fmax(others, np.abs(self.lhs[i - 1, j - 1] - F32(value)))), others


def ghost_taps(n):
    """the ghost cells next to the interior corners, to columns 256 / 257 and to rows 1024 / 1025: one per tap and class"""
    taps = [(0, 1), (1, 0), (0, n), (1, n + 1), (n + 1, 1), (n, 0), (n + 1, n), (n, n + 1)]
    taps += [(i, j) for j in (256, 257) if j <= n for i in (0, n + 1)]
    taps += [(i, j) for i in (1024, 1025) if i <= n for j in (0, n + 1)]
    return sorted(set(taps))


@STORAGE
@pytest.mark.parametrize("n", SIZES)
def test_residual_sees_every_cell_and_every_tap(n, storage):
    rng = np.random.default_rng(2000 + n)
    x, x0 = base_field(rng, n, storage), base_field(rng, n, storage)
    cells = cells_of(n)
    s = arena_solver(n, storage=storage)
    try:
        s.upload(dens=x, dens_prev=x0)
        poison_pads(s, ("dens", "dens_prev"))
        models = [ResidualModel(x, x0, a, b) for a, b in COEFFS]
        for (a, b), m in zip(COEFFS, models):
            assert same_word(s.residual("dens", "dens_prev", a, b), residual32(x, x0, a, b))
            assert same_word(m.first, residual32(x, x0, a, b)) and m.first < 4200
        # one right-hand-side cell: only that cell's term changes, and it is the largest
        bad = []
        full = set(cells if n <= 9 else cells[:3] + cells[-3:])      # (the model itself against residual32, in passing)
        for cell, value in planted_rows(s, "dens_prev", x0, cells, (RPLANT,)):
            for (a, b), m in zip(COEFFS, models):
                want, others = m.planted(cell[0], cell[1], value)
                assert want > others
                if cell in full:
                    x0p = x0.copy()
                    x0p[cell] = value
                    assert same_word(want, residual32(x, x0p, a, b))
                got = s.residual("dens", "dens_prev", a, b)
                if not same_word(got, want):
                    bad.append((cell, (a, b), got, float(want)))
        report(bad, "residual, a cell of x0, n=%d: ((row, column), (alpha, beta), returned, the model)" % n)
        # one ghost cell of x: the one interior cell whose stencil holds it takes the maximum, through that tap
        for cell, value in planted_rows(s, "dens", x, ghost_taps(n), (RPLANT,)):
            xp = x.copy()
            xp[cell] = value
            for (a, b), m in zip(COEFFS, models):
                want = residual32(xp, x0, a, b)
                assert want > m.first
                got = s.residual("dens", "dens_prev", a, b)
                if not same_word(got, want):
                    bad.append((cell, (a, b), got, float(want)))
        report(bad, "residual, a ghost cell of x, n=%d: ((row, column), (alpha, beta), returned, the model)" % n)
        for a, b in COEFFS:
            assert same_word(s.residual("dens", "dens_prev", a, b), residual32(x, x0, a, b))
        assert_bit_equal(s.download("dens"), x, "x put back")
        assert_bit_equal(s.download("dens_prev"), x0, "x0 put back")
        pads_still_poisoned(s, ("dens", "dens_prev"))
    finally:
        s.close()


# ---- 2. one result per member ----------------------------------------------------------------------------------------------
@STORAGE
def test_a_cell_of_one_member_moves_that_members_word_only(storage):
    """3 members, n = 258 (a second pass of k_residual's column loop: columns 257 / 258): the plant goes into member 1.  The
    members' interiors are scaled by 1, 1/2, 1/4, so no two words are equal to begin with."""
    n, members = 258, 3
    rng = np.random.default_rng(258 + storage)
    cells = sorted({(i, j) for i in (1, n) for j in (1, 256, 257, 258)} | set(corners(n)))
    alpha, beta = np.array([1.0, 0.7, 0.5], F32), np.array([4.0, 3.3, 3.0], F32)

    def fields():
        out = []
        for m in range(members):
            f = base_field(rng, n, storage)
            f[1:-1, 1:-1] *= F32(0.5) ** m
            assert np.array_equal(stored(f, storage), f)
            out.append(f)
        return out

    u, v, x, x0 = fields(), fields(), fields(), fields()
    with solver(n, members, storage=storage) as s:
        for m in range(members):
            s.upload(member=m, u=u[m], v=v[m], dens=x[m], dens_prev=x0[m])
        amax0 = s.absmax_velocity_members("u", "v")
        res0 = s.residual_members("dens", "dens_prev", alpha, beta)
        for m in range(members):
            assert same_word(amax0[m], absmax32(u[m], v[m])) and same_word(res0[m], residual32(x[m], x0[m], alpha[m], beta[m]))
        assert len({int(w) for w in u32(amax0)}) == members
        assert same_word(s.absmax_velocity("u", "v"), amax0.max())
        assert same_word(s.residual("dens", "dens_prev", 0.7, 3.3), max(residual32(x[m], x0[m], 0.7, 3.3) for m in range(members)))
        bad = []
        for cell in cells:
            for name, f in (("u", u[1]), ("v", v[1])):
                for value in (PLANT, -PLANT):
                    g = f.copy()
                    g[cell] = value
                    s.upload(member=1, **{name: g})
                    got = s.absmax_velocity_members("u", "v")
                    if not (same_word(got[1], PLANT) and same_word(got[0], amax0[0]) and same_word(got[2], amax0[2])
                            and same_word(s.absmax_velocity("u", "v"), PLANT)):
                        bad.append((name, cell, float(value), got.tolist()))
                s.upload(member=1, **{name: f})
            g = x0[1].copy()
            g[cell] = RPLANT
            s.upload(member=1, dens_prev=g)
            got = s.residual_members("dens", "dens_prev", alpha, beta)
            want = residual32(x[1], g, alpha[1], beta[1])
            assert want > res0.max()
            scalar = max(residual32(x[m], g if m == 1 else x0[m], 0.7, 3.3) for m in range(members))
            if not (same_word(got[1], want) and same_word(got[0], res0[0]) and same_word(got[2], res0[2])
                    and same_word(s.residual("dens", "dens_prev", 0.7, 3.3), scalar)):
                bad.append(("dens_prev", cell, got.tolist(), float(want)))
            s.upload(member=1, dens_prev=x0[1])
        report(bad, "per-member maxima with a cell planted in member 1")
        assert np.array_equal(u32(s.absmax_velocity_members("u", "v")), u32(amax0))
        assert np.array_equal(u32(s.residual_members("dens", "dens_prev", alpha, beta)), u32(res0))


# ---- 3. the bounds of a slab's advections ----------------------------------------------------------------------------------
# (n, ranks, sweeps per solve).  2049 over 2 ranks is the smallest shape at which rows * ceil(n / 256) exceeds the 8192
# partial maxima of k_subtract_gradient_max, so that its `i += gridDim.y` loop repeats; its solves are cut to 4 sweeps.
SLABS = [(257, 3, 40), (1030, 2, 40), (2049, 2, 4)]
SLAB_COLS = (1, 256, 257)


def slab_cols(n):
    return sorted({j for j in SLAB_COLS + (n,) if j <= n})


def own_maximum(u, v, n, lo, hi):
    return F32(max(np.abs(u[lo:hi, 1:n + 1]).max(), np.abs(v[lo:hi, 1:n + 1]).max()))


def spike(n):
    """A velocity source at one cell that sizes the halo of the advection at about 10 rows.  visc = 0 makes the diffusion
    the identity (alpha = 0, beta = 1), so the advected velocity is dt * source, projected; the projection leaves a
    single-cell spike f = 0.71 .. 0.90 of its height (next to a wall, mid-field, 4 or 40 sweeps: every placement below,
    checked with the oracle when this test was written).  reach = ceil(dt * n * vmax) + 2 with vmax = f * dt * spike:
    spike = 9.5 / (dt^2 n) puts dt * n * vmax between 6.7 and 8.6, reach between 9 and 11, where the sources below 1
    alone reach 3 rows."""
    return F32(9.5 / (DT * DT * n))


@pytest.mark.parametrize("n,nranks,iters", SLABS)
def test_gradient_bound_sees_a_spike_on_every_edge_of_every_slab(n, nranks, iters):
    """fluid_vel_step on row slabs: the bound of its advection is reduced by k_subtract_gradient_max + k_max_partials over
    each slab's own rows.  A spike in the u_prev / v_prev source at the first and at the last row a rank owns, at columns 1,
    256, 257 and n (the seams of blockIdx.x * 256), puts the maximum on that cell: every value a rank brings to the MAX
    exchange is numpy's maximum over its rows of the velocity a one-context replay through the operators produces."""
    from fluidsimulationcuda_amd import capi
    from fluidsimulationcuda_amd.slab import slab_rows
    import fluidsimulationcuda_amd as F
    base = synthetic(n, seed=3 + n)
    rows = sorted({i for r in range(nranks) for i in (slab_rows(n, r, nranks)[0], slab_rows(n, r, nranks)[1] - 1)})
    placements = [(i, j) for i in rows for j in slab_cols(n)]
    bad = []
    with F.FluidSolver(n, params={capi.PARAM_TB_MIN_CELLS: 0}) as one:
        for k, (i, j) in enumerate(placements):
            name = ("u_prev", "v_prev")[k % 2]
            fields = dict(base)
            fields[name] = base[name].copy()
            fields[name][i, j] += spike(n)
            # one context, through the operators (FluidSequential.c:189-241 with visc = 0)
            one.upload(**fields)
            one.add_source("u", "u_prev")
            one.add_source("v", "v_prev")
            one.diffuse(1, "u_prev", "u", 0.0, 1.0, iters)
            one.diffuse(2, "v_prev", "v", 0.0, 1.0, iters)
            one.computeDivergenceAndPressure("u_prev", "v_prev", "u", "v")
            one.diffuse(0, "u", "v", 1.0, 4.0, iters)
            one.lastProject("u_prev", "v_prev", "u")
            wu, wv = one.download("u_prev"), one.download("v_prev")
            one.advect(1, "u", "u_prev", "u_prev", "v_prev")
            one.advect(2, "v", "v_prev", "u_prev", "v_prev")
            one.computeDivergenceAndPressure("u", "v", "u_prev", "v_prev")
            one.diffuse(0, "u_prev", "v_prev", 1.0, 4.0, iters)
            one.lastProject("u", "v", "u_prev")
            want = {f: one.download(f) for f in ("u", "v", "dens")}
            # the spike is where the maximum is, and it sizes the halo as stated
            speed = np.maximum(np.abs(wu[1:-1, 1:-1]), np.abs(wv[1:-1, 1:-1]))
            at = np.unravel_index(np.argmax(speed), speed.shape)
            assert (at[0] + 1, at[1] + 1) == (i, j), "the maximum of the replay is at %r, the spike at %r" % (at, (i, j))
            reach = int(np.ceil(DT * n * float(speed.max()))) + 2
            assert 8 <= reach <= 12, reach
            got, fab = run_ranks(n, nranks, 0, fields, lambda s: s.vel_step(visc=0.0, iters=iters), jacobi=3)
            for f in ("u", "v", "dens"):
                assert_bit_equal(got[f], want[f], "%s, a spike in %s at (%d, %d): %d slabs vs one context" % (f, name, i, j, nranks))
            for r in range(nranks):
                lo, hi = slab_rows(n, r, nranks)
                m = own_maximum(wu, wv, n, lo, hi)
                if len(fab.maxima[r]) != 1 or not same_word(fab.maxima[r][0], m):
                    bad.append(((i, j), name, "rank %d" % r, fab.maxima[r], float(m)))
    report(bad, "vel_step, n=%d on %d slabs: ((row, column), source, rank, the bounds it brought, numpy)" % (n, nranks))


@pytest.mark.parametrize("n,nranks,iters", SLABS)
def test_advect_bound_stops_at_the_slabs_own_rows(n, nranks, iters):
    """The stand-alone advect operator on slabs reduces its bound with launch_absmax2 over rows [own0, own1) (vmax_begin).
    A cell of u planted on the row just above and on the row just below the slab of the middle (first) rank must raise
    the neighbour's maximum and leave this rank's alone -- above the first rank lies the ghost row, which is nobody's."""
    from fluidsimulationcuda_amd.slab import slab_rows
    rng = np.random.default_rng(n)
    # dt * n * 0.25 / 4: a back-trace of about a cell; the plant: 8 cells, a halo of 10 rows
    amp = 1.0 / (DT * n)
    base = dict(u=rnd(rng, n, -amp, amp), v=rnd(rng, n, -amp, amp), dens_prev=rnd(rng, n), dens=np.zeros((n + 2, n + 2), F32))
    plant = F32(8.0 / (DT * n))
    me = 1 if nranks > 2 else 0
    own0, own1 = slab_rows(n, me, nranks)
    bad = []
    for i in (own0 - 1, own1):
        for j in slab_cols(n):
            fields = dict(base)
            fields["u"] = base["u"].copy()
            fields["u"][i, j] = plant if (i + j) % 2 else -plant

            def body(s):
                s.advect(0, "dens", "dens_prev", "u", "v", DT)

            want = single(n, fields, body)
            got, fab = run_ranks(n, nranks, 0, fields, body, jacobi=3)
            assert_bit_equal(got["dens"], want["dens"], "advect with u planted at (%d, %d), %d slabs vs one context" % (i, j, nranks))
            for r in range(nranks):
                lo, hi = slab_rows(n, r, nranks)
                m = own_maximum(fields["u"], fields["v"], n, lo, hi)
                unplanted = own_maximum(base["u"], base["v"], n, lo, hi)
                assert (m == abs(plant)) == (lo <= i < hi) and (m == unplanted) == (not lo <= i < hi)
                assert r != me or m == unplanted
                if len(fab.maxima[r]) != 1 or not same_word(fab.maxima[r][0], m):
                    bad.append(((i, j), "rank %d" % r, fab.maxima[r], float(m)))
    report(bad, "advect, n=%d on %d slabs: ((row, column), rank, the bounds it brought, numpy)" % (n, nranks))


# ---- 4. division mode 5: one non-finite result anywhere in a wave's strip reruns the strip ---------------------------------
TB_N = 225                                                     # three windows at every depth but 2: 2 x 96, 2 x 104, 2 x 112 < 225
OWNED = {16: 96, 12: 104, 8: 112, 4: 120, 2: 124}              # columns a window of 2-column lanes owns (test_gpu_ops.py)
PLANTS = {"x0=2^105": ("v", F32(2.0 ** 105)), "x=2^105": ("u", F32(2.0 ** 105)), "x0=inf": ("v", F32(np.inf)), "x=nan": ("u", F32(np.nan))}


def tb_cells(max_t, rows):
    """every column of rows {1, a strip seam, n} and every row of columns {1, a window seam, n}.  The window seam: the last
    column the first window owns in the solve's deepest launch (the row sweeps cross the first column of the next window
    and every other seam).  The strip seam: the first row of an odd strip near the middle -- strips are `rows` output rows
    from row 1; rows = 0 leaves the height to the library, whose closed form gives 2 at this size (the column sweeps
    cross every seam whatever the height)."""
    n = TB_N
    seam_col = OWNED[max(tb_schedule(16, max_t))]
    rb = rows if rows > 0 else 2
    seam_row = rb * ((n // (2 * rb)) | 1) + 1
    assert 1 < seam_col < n and 1 < seam_row < n
    return lines(n, (1, seam_row, n), (1, seam_col, n))


def oracle_near(oracle, base_want, xp, x0p, i, j, alpha, beta, sweeps):
    """oracle.diffuse(0, ..) of fields that differ from the base fields at cell (i, j) only, given the oracle's result on the
    base fields -- without a pass over the whole grid per placement.  A Jacobi sweep moves a difference by one cell, so
    after `sweeps` sweeps the two results differ within `sweeps` cells of (i, j) at most -- one more where that is a ghost
    cell, which copies its neighbour within the sweep; there the oracle runs on a box cut out of the fields.  A side of the box that is no wall of the grid gets the oracle's wall rule, which is wrong
    there, and the error travels one cell per sweep: the box reaches 2 * sweeps + 3 cells past the plant on such a side,
    so the error stops short of the cells that are taken from it.  (test below: a few placements against the whole grid.)"""
    w = base_want.shape[0]
    side, half = 4 * sweeps + 6, 2 * sweeps + 3
    assert side <= w
    a, b = min(max(i - half, 0), w - side), min(max(j - half, 0), w - side)
    xs, x0s = xp[a:a + side, b:b + side].copy(), x0p[a:a + side, b:b + side].copy()
    with np.errstate(all="ignore"):
        oracle.diffuse(0, xs, x0s, alpha, beta, sweeps)
    reach = sweeps + 1
    r0, r1, c0, c1 = max(0, i - reach), min(w, i + reach + 1), max(0, j - reach), min(w, j + reach + 1)
    for lo, hi, at in ((r0, r1, a), (c0, c1, b)):      # taken from the box: only what no wrong side has reached
        assert (at == 0 or lo - at > sweeps) and (at + side == w or at + side - hi > sweeps)
    want = base_want.copy()
    want[r0:r1, c0:c1] = xs[r0 - a:r1 - a, c0 - b:c1 - b]
    return want


@pytest.fixture(scope="module")
def tb_base(oracle):
    rng = np.random.default_rng(TB_N)
    x, x0 = rnd(rng, TB_N), rnd(rng, TB_N)
    want = x.copy()
    oracle.diffuse(0, want, x0, 0.7, 3.3, 16)
    return x, x0, want


@pytest.mark.parametrize("kind", list(PLANTS))
@pytest.mark.parametrize("rows", [0, 3])
@pytest.mark.parametrize("max_t", [16, 12, 8, 2])
def test_mode5_reruns_the_strip_wherever_the_offending_cell_is(oracle, tb_base, max_t, rows, kind):
    from fluidsimulationcuda_amd import capi
    import fluidsimulationcuda_amd as F
    n, (alpha, beta), sweeps = TB_N, (0.7, 3.3), 16
    x, x0, base_want = tb_base
    name, value = PLANTS[kind]
    cells = tb_cells(max_t, rows)
    whole = set(cells[:2] + cells[len(cells) // 2:len(cells) // 2 + 2] + cells[-2:])     # (oracle_near against the whole grid)
    params = {capi.PARAM_TB_MIN_CELLS: 0, capi.PARAM_TB_T16_MIN_CELLS: 0, capi.PARAM_TB_FAST_DIVISION: 2, capi.PARAM_TB_LANE_COLUMNS: 2,
              capi.PARAM_TB_MAX_SWEEPS: max_t, capi.PARAM_TB_ROWS: rows}
    bad = []
    with F.FluidSolver(n, jacobi=capi.JACOBI_TB, params=params) as s:
        assert s.division_mode(alpha, beta) == 5
        s.upload(u=x, v=x0)
        xp, x0p = x.copy(), x0.copy()
        planted = xp if name == "u" else x0p
        for i, j in cells:
            planted[i, j] = value
            s.upload(u=xp)                                     # (the solve overwrote it)
            s.upload_rows("v", x0p, i, i + 1)
            s.diffuse(0, "u", "v", alpha, beta, sweeps)
            got, rhs = s.download("u"), s.download("v")
            want = oracle_near(oracle, base_want, xp, x0p, i, j, alpha, beta, sweeps)
            if (i, j) in whole:
                full = xp.copy()
                with np.errstate(all="ignore"):
                    oracle.diffuse(0, full, x0p, alpha, beta, sweeps)
                assert np.array_equal(u32(full), u32(want)), "oracle_near differs from oracle.diffuse for a plant at %r" % ((i, j),)
            nan = np.isnan(want)
            if not np.array_equal(np.isnan(got), nan):
                bad.append(((i, j), "NaN in %d cells, the oracle in %d" % (np.isnan(got).sum(), nan.sum())))
            elif not np.array_equal(u32(got)[~nan], u32(want)[~nan]):
                k = np.argwhere((u32(got) != u32(want)) & ~nan)
                bad.append(((i, j), "%d cells differ, the first at %r: %r, the oracle %r" % (len(k), tuple(k[0]), got[tuple(k[0])], want[tuple(k[0])])))
            if not np.array_equal(u32(rhs)[~np.isnan(x0p)], u32(x0p)[~np.isnan(x0p)]):
                bad.append(((i, j), "x0 was touched"))
            planted[i, j] = (x if name == "u" else x0)[i, j]
            s.upload_rows("v", x0p, i, i + 1)
    report(bad, "mode 5, %s, %d sweeps per launch at most, strips of %d rows: ((row, column), what)" % (kind, max_t, rows))


# ---- 5. diffuse_tol stops on the residual of the one cell that has one ------------------------------------------------------
def test_diffuse_tol_stops_on_a_single_cell(oracle):
    """x = 0, x0 = 0 but for one cell of 64: the residual that ends the solve is that cell's neighbourhood's alone.  Sweeps
    done and the final residual are the model's: residual32 after oracle.diffuse of as many sweeps, checked every 4."""
    import fluidsimulationcuda_amd as F
    n, tol, every = 258, 1e-3, 4
    alpha, beta = F.coefficients(n, DT, 0.0025)
    cells = sorted(set(corners(n)) | {(1, 257), (n, 257), (130, 257), (n, 130)})
    z = np.zeros((n + 2, n + 2), F32)
    with F.FluidSolver(n) as s:
        for cell in cells:
            x0 = z.copy()
            x0[cell] = PLANT
            s.upload(u=z, v=x0)
            done, res = s.diffuse_tol(0, "u", "v", alpha, beta, tol, max_iters=400, check_every=every)
            x, sweeps = z.copy(), 0
            r = residual32(x, x0, alpha, beta)
            while r > F32(tol) and sweeps < 400:
                oracle.diffuse(0, x, x0, alpha, beta, every)
                sweeps += every
                r = residual32(x, x0, alpha, beta)
            assert every < sweeps < 400, sweeps
            assert done == sweeps, "x0 planted at %r: %d sweeps, the model %d" % (cell, done, sweeps)
            assert same_word(res, r), "x0 planted at %r: residual %r, the model %r" % (cell, res, r)
            assert_bit_equal(s.download("u"), x, "the solution, x0 planted at %r" % (cell,))
