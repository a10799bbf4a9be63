"""GPU: verifying ensembles -- fluid_verify_members (include/fluid_amd.h, "verifying ensembles"): per cell of a box the error
of the ensemble mean, the sample variance, the CRPS and the rank of a truth among the members; per field one row of sums
and the rank histogram.

Every expected value comes from tests/verify_model.py, the header's rules in numpy float64, applied to what download_members
(the pack) showed before the call.  The CRPS map, the counts and the bins are compared exactly (a NaN is any NaN); one-cell
boxes, planted cells and dyadic inputs make the four sums exact too; elsewhere each sum is within n * 2^-53 * sum |terms| of
the model's fsum, the bound for n doubles added in any order.  tests/test_verify_abi.py shows on the CPU what the model
itself has to have.

The kernel's own indexing (fluid_verify.hip): the cells of the box are numbered row by row, t = (row - row_lo) * cols + (col -
col_lo); lane t of block t / 256 takes cell t while t < 256 * 2048, beyond that lane t mod (256 * 2048) takes a second cell.
Its seams: the end of a box row (t = k * cols - 1 | k * cols: the last and the first column of the box), the end of a wave
(t = 63 | 64), the end of a block (t = 255 | 256) and the wrap of the grid (t = 524287 | 524288, reached from N = 723 on).  The
member count picks one of six kernels, padded to MP = 2, 4, 8, 16, 32, 64 members.

Shapes: N = 14 is one partial block, N = 30 four blocks with a tail, N = 61 has W = 63, odd and no multiple of 4; N = 766
with the whole 768 x 768 array as the box is past the wrap of the grid (any N from 723 on is), with 65536 lanes that take a
second cell."""
import ctypes as C
import math

import numpy as np
import pytest

from verify_model import F32, F64, ROW, SUMS, cell_scores, dyadic_inputs, in_box, interior, narrow, random_inputs, score_row, sum_bounds

pytestmark = pytest.mark.gpu
MEMBERS = [2, 3, 5, 8, 33, 64]
MAIN = ("u", "v", "dens", "u_prev", "v_prev", "dens_prev")
DT = 0.016
NAN32 = 0x7FC5A5A5                 # a NaN: memory the call must not write
NAN64 = 0x7FF8A5A5A5A5A5A5
NAME = b"fluid_verify_members"


def F():
    import fluidsimulationcuda_amd as f
    return f


def torch_():
    import torch
    return torch


def solver(n, members, storage=0, **kw):
    return F().FluidSolver(n, members=members, storage=storage, **kw)


def dev(a):
    return torch_().from_numpy(np.ascontiguousarray(a, F32)).cuda()


def ints(*v):
    return (C.c_int * len(v))(*v)


def shown(s, field):
    """what the pack shows: every member of a field, the lazy state settled"""
    return s.download_members(field)


def same(got, want, what):
    """bit for bit, except that a NaN is any NaN"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    u = np.uint32 if got.dtype == F32 else np.uint64
    ok = np.where(np.isnan(want), np.isnan(got), got.view(u) == want.view(u))
    if not ok.all():
        at = tuple(np.argwhere(~ok)[0])
        raise AssertionError("%s: %d of %d values differ; first at %s: got %r want %r" % (what, int((~ok).sum()), ok.size, at, got[at], want[at]))


def same_bits(got, want, what):
    """every bit, NaN payloads included: for memory the call must not have changed"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = got.view(np.uint8) != want.view(np.uint8)
    assert not bad.any(), "%s: %d of %d bytes changed; first at %s" % (what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))


def run(s, y, field="dens", box=None, fair=False):
    """one field through the solver: (row (ROW,) float64, map (W, W) float32 with NaN32 where nothing was written)"""
    torch = torch_()
    w = s.n + 2
    cm = torch.full((1, w, w), NAN32, dtype=torch.int32, device="cuda").view(torch.float32)
    out = s.verify(dev(np.asarray(y, F32)[None]), (field,), box=box, fair=fair, crps_map=cm)
    assert tuple(out.shape) == (1, ROW) and out.dtype == torch.float64
    return out.cpu().numpy()[0], cm.cpu().numpy()[0]


def check_map(cm, c, box, what):
    """the model's CRPS inside the box, the sentinel outside"""
    want = np.full(cm.shape, 0, np.uint32)
    want[:] = NAN32
    want = want.view(F32)
    in_box(want, box)[...] = in_box(c["crps"], box).astype(F32)
    inside = np.zeros(cm.shape, bool)
    in_box(inside, box)[...] = True
    same(cm[inside], want[inside], what + ": the CRPS map")
    same_bits(cm[~inside], want[~inside], what + ": the map outside the box")


def check_row(row, c, box, members, what, exact=()):
    """count and bins exact, zeros beyond the bins, each sum within its bound of fsum -- the sums named in `exact` bit for bit"""
    want = score_row(c, box, members)
    assert row[0] == want[0], what
    same_bits(row[SUMS:], want[SUMS:], what + ": the rank histogram and the zeros behind it")
    bounds = sum_bounds(c, box) if np.isfinite(want[1:SUMS]).all() else [0.0] * 4
    for k, name in enumerate(("e", "se", "var", "crps")):
        g, v = row[1 + k], want[1 + k]
        print("%s: sum %s = %r, model %r, off by %g, bound %g" % (what, name, g, v, abs(g - v) if np.isfinite(v) else 0.0, bounds[k]))
        if np.isnan(v):
            assert np.isnan(g), "%s: sum %s is %r, the model's is a NaN" % (what, name, g)
        elif np.isinf(v) or name in exact:
            assert g == v, "%s: sum %s is %r, the model's %r" % (what, name, g, v)
        else:
            assert abs(g - v) <= bounds[k], "%s: sum %s = %r is %g off the model's %r, bound %g" % (what, name, g, abs(g - v), v, bounds[k])


def check(s, x, y, box, fair, what, field="dens", exact=()):
    row, cm = run(s, y, field, box, fair)
    c = cell_scores(x, y, fair)
    b = interior(s.n) if box is None else box
    check_map(cm, c, b, what)
    check_row(row, c, b, s.members, what, exact)
    return row, cm


# ---- 1. the model --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fair", [False, True], ids=["plain", "fair"])
@pytest.mark.parametrize("members", MEMBERS)
def test_random_values_against_the_model(members, fair):
    for n in (14, 30, 61):
        x, y = random_inputs(n, members, 0, seed=100 * n + members)
        with solver(n, members) as s:
            s.upload_members(dens=x)
            same_bits(shown(s, "dens"), x, "the upload")
            check(s, x, y, None, fair, "n=%d M=%d fair=%d" % (n, members, fair))
            check(s, x, y, (0, n + 2, 0, n + 2), fair, "n=%d M=%d fair=%d, the whole array" % (n, members, fair))


@pytest.mark.parametrize("members", MEMBERS)
def test_fp16_fields_a_few_steps_have_left(members):
    """fp16 storage: u_prev holds the pressure (from N = 16 on at a scale), dens owes itself a deferred source.  What the
    pack shows comes from a twin context the call never ran on."""
    for n in (14, 66):
        w = n + 2
        x, y = random_inputs(n, members, 1, seed=100 * n + members + 7)
        rng = np.random.default_rng(members)
        fields = {f: narrow(rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32), 1) for f in MAIN}
        fields["dens"] = x

        def prepared():
            s = solver(n, members, 1)
            s.upload_members(**fields)
            s.step(use_sources=True)
            s.step(use_sources=True)
            s.add_source("dens", "dens_prev", DT)
            return s

        with prepared() as s, prepared() as twin:
            for k, f in enumerate(("dens", "u_prev")):
                before = shown(twin, f)
                truth = (before[0] + before.std(axis=0) * rng.normal(size=(w, w))).astype(F32)
                for fair in (False, True):
                    check(s, before, truth, None, fair, "fp16 n=%d M=%d %s fair=%d" % (n, members, f, fair), field=f)
                same_bits(shown(s, f), before, "fp16 n=%d M=%d: %s after the calls" % (n, members, f))


def test_past_the_wrap_of_the_grid():
    """768 x 768 cells are more than 2048 blocks of 256 lanes: the first 65536 lanes take a second cell"""
    n, members = 766, 2
    x, y = random_inputs(n, members, 0, seed=766)
    with solver(n, members) as s:
        s.upload_members(dens=x)
        check(s, x, y, (0, n + 2, 0, n + 2), False, "n=766 M=2, the whole array")


# ---- 2. every member count -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mp", [2, 4, 8, 16, 32, 64])
def test_every_member_count(mp):
    """every M of a padded class at N = 14, one call each: every pad count of every kernel"""
    n = 14
    for members in range(mp // 2 + 1, mp + 1):
        if members < 2:
            continue
        x, y = random_inputs(n, members, 0, seed=3000 + members)
        with solver(n, members) as s:
            s.upload_members(dens=x)
            check(s, x, y, None, bool(members & 1), "n=14 M=%d (MP=%d)" % (members, mp))


# ---- 3. one-cell boxes, 4. planted cells -----------------------------------------------------------------------------------------
def lines_and_seams(n):
    """the corners, every cell of rows and columns 0, 1, N, N+1 (with the interior as the box, columns 1 | N are the two sides
    of every row seam; with the whole array, columns 0 | N+1), and the cells on both sides of the wave seam t = 63 | 64 and of
    the block seam t = 255 | 256, in the numbering of the interior box and of the whole array"""
    w = n + 2
    cells = set()
    for k in (0, 1, n, n + 1):
        cells |= {(k, j) for j in range(w)} | {(i, k) for i in range(w)}
    for t in (63, 64, 255, 256):
        cells.add((1 + t // n, 1 + t % n))
        cells.add((t // w, t % w))
    return sorted(cells)


def raw_verify(s, ids, truth_ptr, stride, box, flags, map_ptr, out_ptr):
    from fluidsimulationcuda_amd import capi
    L = capi.lib()
    rc = L.fluid_verify_members(s._h, ids, len(ids), truth_ptr, stride, None if box is None else ints(*box), flags, map_ptr, out_ptr)
    assert rc == capi.OK, L.fluid_last_error()


@pytest.mark.parametrize("fair", [False, True], ids=["plain", "fair"])
def test_one_cell_boxes(fair):
    """the row of a 1 x 1 box is that cell's e, se, var and crps as doubles, bit for bit; count 1, one bin set.  A 1 x 1 box
    is cell t = 0 of lane 0 whatever the cell: what varies here is the cell's place in the field and in the dense arrays -- the
    ghost ring, the corners, the first and last columns.  The seams of the numbering t are crossed by the planted-cell tests,
    whose boxes have many cells."""
    torch = torch_()
    from fluidsimulationcuda_amd import capi
    n, members = 30, 5
    w = n + 2
    x, y = random_inputs(n, members, 0, seed=31)
    c = cell_scores(x, y, fair)
    cells = lines_and_seams(n)
    assert {(0, 0), (0, w - 1), (w - 1, 0), (w - 1, w - 1), (3, 4), (3, 5), (9, 16), (9, 17), (1, 31), (2, 0), (7, 31), (8, 0)} <= set(cells)
    with solver(n, members) as s:
        s.upload_members(dens=x)
        truth = dev(y)
        out = torch.full((len(cells), ROW), NAN64, dtype=torch.int64, device="cuda").view(torch.float64)
        cm = torch.full((w, w), NAN32, dtype=torch.int32, device="cuda").view(torch.float32)
        torch.cuda.synchronize()
        for k, (i, j) in enumerate(cells):
            raw_verify(s, ints(2), truth.data_ptr(), 0, (i, i + 1, j, j + 1), capi.VERIFY_FAIR if fair else 0, cm.data_ptr(),
                       out.data_ptr() + 8 * ROW * k)
        s.synchronize()
        out, cm = out.cpu().numpy(), cm.cpu().numpy()
    want = np.zeros((len(cells), ROW), F64)
    want_map = np.full((w, w), NAN32, np.uint32).view(F32)
    for k, (i, j) in enumerate(cells):
        want[k, :SUMS] = [1.0, c["e"][i, j], c["se"][i, j], c["var"][i, j], c["crps"][i, j]]
        want[k, SUMS + c["rank"][i, j]] = 1.0
        want_map[i, j] = c["crps"][i, j]
    same_bits(out, want, "the rows of %d one-cell boxes" % len(cells))
    same_bits(cm, want_map, "the map after %d one-cell boxes" % len(cells))


def planted_case(n, members, cells, seed, box=None):
    """the ensemble is constant and equal to the truth -- every term 0, every rank 0 -- except in one cell"""
    rng = np.random.default_rng(seed)
    w = n + 2
    const = F32(0.75)
    y = np.full((w, w), const, F32)
    given, box = box, interior(n) if box is None else box
    with solver(n, members) as s:
        for (i, j) in cells:
            x = np.full((members, w, w), const, F32)
            x[:, i, j] = const + rng.uniform(-2.0, 2.0, members).astype(F32)
            s.upload_members(dens=x)
            row, _ = run(s, y, box=given)
            c = cell_scores(x, y)
            want = score_row(c, box, members)
            inside = box[0] <= i < box[1] and box[2] <= j < box[3]
            if inside:                             # (the model's sums have one term that is not +0: fsum is that term)
                assert list(want[1:SUMS]) == [c["e"][i, j], c["se"][i, j], c["var"][i, j], c["crps"][i, j]] and want[2] > 0
                assert want[SUMS + c["rank"][i, j]] >= 1
            else:
                assert not want[1:SUMS].any() and want[SUMS] == (box[1] - box[0]) * (box[3] - box[2])
            same_bits(row, want, "n=%d M=%d: the row with cell (%d, %d) planted" % (n, members, i, j))


def test_planted_cells_every_interior_cell():
    n = 14
    planted_case(n, 3, [(i, j) for i in range(1, n + 1) for j in range(1, n + 1)], 41)


def test_planted_cells_lines_and_seams():
    """N = 61: rows and columns 0, 1, N, N+1 and the seams: a ghost cell is never counted, an interior cell exactly once"""
    planted_case(61, 3, lines_and_seams(61), 42)


def test_planted_cells_seams_of_other_boxes():
    """N = 61, boxes whose numbering t differs from the interior's: the whole array (63 columns) and a box of 7 columns off
    the edges; in each the cells t = 62 | 63 | 64 | 65, 254 .. 257 and the last, and the cells just outside the box"""
    n = 61
    w = n + 2
    for box in ((0, w, 0, w), (3, 50, 5, 12)):
        cols = box[3] - box[2]
        last = (box[1] - box[0]) * cols - 1
        cells = [(box[0] + t // cols, box[2] + t % cols) for t in (0, 62, 63, 64, 65, 254, 255, 256, 257, last)]
        if box[0] > 0:
            cells += [(box[0] - 1, box[2]), (box[1], box[3] - 1), (box[0], box[2] - 1), (box[1] - 1, box[3])]
        planted_case(n, 3, cells, 43, box=box)


# ---- 5. exact sums ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("members", [2, 8, 64])
def test_dyadic_inputs_sum_exactly(members):
    """every partial sum is representable (tests/test_verify_abi.py shows it on these inputs): the sums are fsum's, bit for bit"""
    for n in (14, 61):
        x, y = dyadic_inputs(n, members, seed=9000 + 10 * n + members)
        with solver(n, members) as s:
            s.upload_members(dens=x)
            for fair in ((False, True) if members == 2 else (False,)):
                exact = ("e", "se", "crps") + (("var",) if members == 2 else ())
                check(s, x, y, None, fair, "dyadic n=%d M=%d fair=%d" % (n, members, fair), exact=exact)


# ---- 6. hand-made cells ----------------------------------------------------------------------------------------------------------
def test_hand_made_cells_and_boxes():
    n, members = 14, 5
    w = n + 2
    x, y = random_inputs(n, members, 0, seed=61)
    x[:, 2, 2] = [1.5, 1.5, -2.0, 1.5, -2.0]                     # ties among the members
    x[:, 2, 3], y[2, 3] = [1.0, 2.0, 3.0, 4.0, 5.0], 3.0          # the truth equal to a member
    x[:, 2, 4], y[2, 4] = [7.0, 7.0, 7.0, 7.0, 7.0], 7.0          # ... to all of them
    zeros = [(3, 2), (3, 3), (3, 4), (0, 5)]
    x[:, 3, 2], y[3, 2] = [0.0, -0.0, 0.0, -0.0, 1.0], -0.0
    x[:, 3, 3], y[3, 3] = [-0.0, -0.0, -0.0, -0.0, -0.0], 0.0
    x[:, 3, 4], y[3, 4] = [-0.0, 0.0, -1.0, 0.0, 2.0], 0.0
    x[:, 0, 5], y[0, 5] = [0.0, 0.0, -0.0, 0.0, 0.0], -0.0
    whole = (0, w, 0, w)
    boxes = [None, whole, (3, 3, 0, w), (0, w, 7, 7), (0, 0, 0, 0), (w, w, w, w), (5, 6, 0, w), (0, w, w - 1, w), (2, 4, 2, 5)]
    with solver(n, members) as s:
        s.upload_members(dens=x)
        for box in boxes:
            for fair in (False, True):
                check(s, x, y, box, fair, "hand-made cells, box %s fair=%d" % (box, fair))
        row, base = run(s, y, box=whole)
        # +-0 mixtures: the map is the same bits whichever sign
        x2, y2 = x.copy(), y.copy()
        for (i, j) in zeros:
            z = x2[:, i, j] == 0
            x2[z, i, j] = -x2[z, i, j]
            y2[i, j] = -y2[i, j]
        s.upload_members(dens=x2)
        _, flipped = check(s, x2, y2, whole, False, "signs of zero flipped")
        same_bits(flipped, base, "the map with every zero's sign flipped")
        # non-finite values: that cell's map is a NaN, every other cell's is what it was
        bad = [(4, 4), (0, 0), (w - 1, 9), (9, 1)]
        x3, y3 = x.copy(), y.copy()
        x3[1, 4, 4] = np.nan
        x3[4, 0, 0] = np.inf
        x3[0, w - 1, 9] = -np.inf
        y3[9, 1] = np.nan
        s.upload_members(dens=x3)
        row3, cm3 = check(s, x3, y3, whole, False, "non-finite cells")
        assert all(np.isnan(cm3[i, j]) for (i, j) in bad) and np.isnan(row3[4])
        keep = np.ones((w, w), bool)
        for (i, j) in bad:
            keep[i, j] = False
        same_bits(cm3[keep], base[keep], "the map of the other cells")
        c3 = cell_scores(x3, y3)
        assert c3["rank"][9, 1] == 0 and c3["rank"][4, 4] == int((x[[0, 2, 3, 4], 4, 4] < y[4, 4]).sum())       # rule 4
        # ... and a box without them is not poisoned
        check(s, x3, y3, (5, 9, 2, w), False, "a box beside the non-finite cells")


# ---- 7. nothing else written -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("storage", [0, 1], ids=["f32", "f16"])
def test_nothing_else_is_written(storage):
    torch = torch_()
    from fluidsimulationcuda_amd import capi
    n, members = 30, 5
    w = n + 2
    cells, stride, lead = w * w, w * w + 7, 3
    rng = np.random.default_rng(70 + storage)
    fields = {f: narrow(rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32), storage) for f in MAIN}
    names = ("dens", "u", "v_prev")
    ids = ints(*[capi.FIELD_NAMES.index(f) for f in names])
    box = (2, 29, 0, 31)

    def prepared():
        s = solver(n, members, storage)
        s.upload_members(**fields)
        s.step(use_sources=True)
        s.add_source("dens", "dens_prev", DT)
        return s

    with prepared() as s, prepared() as twin:
        before = {f: shown(twin, f) for f in names}
        words = lead + 2 * stride + cells + 5
        truth_h = np.full(words, NAN32, np.uint32)
        ys = {}
        for k, f in enumerate(names):
            ys[f] = (before[f][0] + F32(0.1) * rng.normal(size=(w, w))).astype(F32)
            truth_h[lead + k * stride:lead + k * stride + cells] = ys[f].view(np.uint32).ravel()
        truth = torch.from_numpy(truth_h.view(np.int32)).cuda()
        cm = torch.full((words,), NAN32, dtype=torch.int32, device="cuda")
        out = torch.full((2 + 3 * ROW + 2,), NAN64, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        raw_verify(s, ids, truth.data_ptr() + 4 * lead, stride, box, capi.VERIFY_FAIR, cm.data_ptr() + 4 * lead, out.data_ptr() + 16)
        s.synchronize()
        same_bits(truth.cpu().numpy().view(np.uint32), truth_h, "the truth after the call")
        got_map, got = cm.cpu().numpy().view(np.uint32), out.cpu().numpy()
        assert (got[:2] == NAN64).all() and (got[-2:] == NAN64).all(), "the doubles around the rows"
        untouched = np.ones(words, bool)
        for k, f in enumerate(names):
            c = cell_scores(before[f], ys[f], True)
            at = lead + k * stride
            check_map(got_map[at:at + cells].view(F32).reshape(w, w), c, box, "%s (storage %d)" % (f, storage))
            row = got[2 + k * ROW:2 + (k + 1) * ROW].view(F64)
            check_row(row, c, box, members, "%s (storage %d)" % (f, storage))
            same_bits(row[SUMS + members + 1:], np.zeros(ROW - SUMS - members - 1, F64), "the entries beyond 5 + M are +0.0")
            untouched[at:at + cells] = False
        assert (got_map[untouched] == NAN32).all(), "the floats between and around the maps"
        for f in MAIN:
            same_bits(shown(s, f), shown(twin, f), "%s after the call" % f)
        for c in (s, twin):
            c.step(use_sources=True)
        for f in ("u", "v", "dens"):
            same_bits(shown(s, f), shown(twin, f), "%s a step after the call" % f)


# ---- 8. repeatability ------------------------------------------------------------------------------------------------------------
def test_the_same_bytes_call_after_call_and_context_after_context():
    n, members = 61, 8
    w = n + 2
    x, y = random_inputs(n, members, 0, seed=81)
    small, large = (5, 9, 5, 9), (0, w, 0, w)
    with solver(n, members) as a, solver(n, members) as b:
        a.upload_members(dens=x)
        b.upload_members(dens=x)
        first = run(b, y, box=large)                 # a fresh context's
        same_bits(run(b, y, box=large)[0], first[0], "two calls")
        one = run(a, y, box=small)
        grown = run(a, y, box=large)                 # the scratch has grown from one block's to 16 blocks'
        same_bits(grown[0], first[0], "after a small box, the rows")
        same_bits(grown[1], first[1], "after a small box, the maps")
        same_bits(run(a, y, box=small)[0], one[0], "the small box again")
        same_bits(run(a, y)[0], run(b, y)[0], "the interior")


def test_rows_of_unwaited_calls_on_a_shared_stream():
    """K calls with wait=False into the K rows of one tensor, read once: what K waited calls give"""
    torch = torch_()
    n, members, K = 30, 5, 6
    w = n + 2
    x, y = random_inputs(n, members, 0, seed=82)
    rng = np.random.default_rng(82)
    ys = [(y + F32(0.01 * k) * rng.normal(size=(w, w))).astype(F32) for k in range(K)]
    ts = torch.cuda.Stream()
    with solver(n, members, stream=ts.cuda_stream) as s:
        s.upload_members(dens=x)
        waited = np.stack([run(s, ys[k], fair=bool(k & 1))[0] for k in range(K)])
        with torch.cuda.stream(ts):
            truths = [dev(ys[k][None]) for k in range(K)]
            scores = torch.full((K, 1, ROW), NAN64, dtype=torch.int64, device="cuda").view(torch.float64)
            for k in range(K):
                assert s.verify(truths[k], out=scores[k], fair=bool(k & 1), wait=False).data_ptr() == scores[k].data_ptr()
            per = s.verify_scores(scores)
        same_bits(scores.cpu().numpy()[:, 0], waited, "the rows of the unwaited calls")
    assert len(per) == K and all(len(p) == 1 for p in per)
    for k in range(K):
        c = cell_scores(x, ys[k], bool(k & 1))
        d = per[k][0]
        assert d["count"] == n * n and d["rank_hist"].dtype == np.int64 and d["rank_hist"].shape == (members + 1,)
        assert np.array_equal(d["rank_hist"], np.bincount(in_box(c["rank"], interior(n)).ravel(), minlength=members + 1))
        t = {name: in_box(c[name], interior(n)).ravel() for name in ("e", "se", "var", "crps")}
        for key, v in (("bias", math.fsum(t["e"]) / n ** 2), ("rmse", math.sqrt(math.fsum(t["se"]) / n ** 2)),
                       ("spread", math.sqrt(math.fsum(t["var"]) / n ** 2)), ("crps", math.fsum(t["crps"]) / n ** 2)):
            assert abs(d[key] - v) <= 1e-12 * max(abs(v), np.abs(t["e"]).max()), (key, d[key], v)


# ---- 9. refusals on a live context -----------------------------------------------------------------------------------------------
def hip_runtime():
    """the HIP runtime this process already holds (the one libfluid_amd.so runs on)"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            lib = C.CDLL(line.split()[-1])
            lib.hipMalloc.argtypes, lib.hipMalloc.restype = [C.POINTER(C.c_void_p), C.c_size_t], C.c_int
            lib.hipFree.argtypes, lib.hipFree.restype = [C.c_void_p], C.c_int
            return lib
    raise RuntimeError("no HIP runtime is loaded")


def test_refusals_change_nothing():
    torch = torch_()
    from fluidsimulationcuda_amd import capi
    L = capi.lib()
    rng = np.random.default_rng(9)
    n, members = 6, 5
    w = n + 2
    cells = w * w
    fields = {f: rng.uniform(-1.0, 1.0, (members, w, w)).astype(F32) for f in MAIN}
    hip = hip_runtime()
    exact, exact2 = C.c_void_p(), C.c_void_p()
    size = 1 << 20
    assert hip.hipMalloc(C.byref(exact), size) == 0 and hip.hipMalloc(C.byref(exact2), size) == 0
    try:
        end = exact.value + size
        truth_fits, truth_short = end - 2 * cells * 4, end - 2 * cells * 4 + 4      # two dense arrays that end with the allocation
        end = exact2.value + size
        rows_fit, rows_short = end - 2 * ROW * 8, end - 2 * ROW * 8 + 8             # two rows that end with theirs
        truth = torch.full((2, w, w), 0.5, dtype=torch.float32, device="cuda")
        cm = torch.full((2, w, w), NAN32, dtype=torch.int32, device="cuda")
        out = torch.full((2 * ROW + 1,), NAN64, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

        def call(hnd, ids=ints(2, 0), count=None, t=None, stride=0, box=None, flags=0, m=None, o=None):
            return lambda: L.fluid_verify_members(hnd, ids, len(ids) if count is None else count, truth.data_ptr() if t is None else t, stride,
                                                  None if box is None else ints(*box), flags, cm.data_ptr() if m is None else m,
                                                  out.data_ptr() if o is None else o)

        with solver(n, members) as s, solver(n, members) as twin:
            for c in (s, twin):
                c.timing_enable(True)
                c.upload_members(**fields)
                c.step(use_sources=True)
                c.add_source("dens", "dens_prev", DT)                      # a lazy state that must survive the refusals
            hnd = s._h
            refused = [
                (lambda: L.fluid_verify_members(hnd, None, 2, truth.data_ptr(), 0, None, 0, None, out.data_ptr()), (b"fields",)),
                (call(hnd, t=0), (b"truth_dev",)),
                (lambda: L.fluid_verify_members(hnd, ints(2, 0), 2, truth.data_ptr(), 0, None, 0, None, None), (b"scores_dev",)),
                (call(None), (b"null context",)),
                (call(hnd, count=0), (b"nfields 0",)),
                (call(hnd, count=13), (b"nfields 13",)),
                (call(hnd, ints(0, 12)), (b"bad field id 12", b"fields[1]")),
                (call(hnd, ints(-1, 2)), (b"bad field id -1", b"fields[0]")),
                (call(hnd, ints(2, 2)), (b"field 2", b"twice")),
                (call(hnd, stride=cells - 1), (b"field_stride %d" % (cells - 1),)),
                (call(hnd, box=(0, w + 1, 0, w)), (b"box[1]", b"outside [0, %d]" % w)),
                (call(hnd, box=(-1, w, 0, w)), (b"box[0]", b"outside")),
                (call(hnd, box=(0, w, 0, w + 1)), (b"box[3]", b"outside")),
                (call(hnd, box=(5, 4, 0, w)), (b"box[0]", b"above")),
                (call(hnd, box=(0, w, 3, 2)), (b"box[2]", b"above")),
                (call(hnd, flags=2), (b"flag",)),
                (call(hnd, flags=capi.VERIFY_FAIR | 4), (b"flag",)),
                (call(hnd, flags=-1), (b"flag",)),
                (call(hnd, o=out.data_ptr() + 4), (b"scores_dev", b"8 bytes")),
                (call(hnd, o=rows_short), (b"scores_dev", b"allocation ends")),
                (call(hnd, t=truth_short), (b"truth_dev", b"allocation ends")),
                (call(hnd, m=truth_short), (b"crps_dev", b"allocation ends")),
                (call(hnd, t=fields["dens"].ctypes.data), (b"not device memory",)),
            ]
            for fn, words in refused:
                L.fluid_synchronize(None)                   # (an unrelated message in between)
                assert fn() == capi.E_INVALID, words
                msg = L.fluid_last_error()
                assert NAME in msg and all(word in msg for word in words), (words, msg)
            s.synchronize()
            assert (cm.cpu().numpy() == NAN32).all() and (out.cpu().numpy() == NAN64).all() and (truth.cpu().numpy() == 0.5).all()
            ta, tb = s.timing_read(reset=False), twin.timing_read(reset=False)
            assert ta == {**tb, **{k: ta[k] for k in ta if k.endswith("_ms")}}             # every count; the times are times
            for f in capi.FIELD_NAMES:
                same_bits(shown(s, f), shown(twin, f), "%s after the refusals" % f)
            # what is not refused: arrays and rows that end with their allocation, an empty box, no map
            assert call(hnd, t=truth_fits, m=truth_fits - 2 * cells * 4, o=rows_fit)() == capi.OK, L.fluid_last_error()
            assert L.fluid_verify_members(hnd, ints(2), 1, truth.data_ptr(), 0, ints(4, 4, 0, w), 0, None, out.data_ptr()) == capi.OK
            s.synchronize()
            got = out.cpu().numpy()
            assert got[0:SUMS].view(F64).tolist() == [0.0] * SUMS and not got[SUMS:ROW].any() and (got[ROW:] == NAN64).all()
            ta, tb = s.timing_read(reset=False), twin.timing_read(reset=False)
            assert ta == {**tb, **{k: ta[k] for k in ta if k.endswith("_ms")}}, "the launches belong to no timing category"
        for m_bad, word in ((1, b"1 member"), (65, b"65 members")):
            with solver(n, m_bad) as s:
                s.upload_members(dens=rng.uniform(-1.0, 1.0, (m_bad, w, w)).astype(F32))
                before = shown(s, "dens")
                assert call(s._h)() == capi.E_INVALID
                msg = L.fluid_last_error()
                assert NAME in msg and word in msg and (m_bad == 1 or b"64" in msg), msg
                same_bits(shown(s, "dens"), before, "dens after the refusal")
        with F().FluidSolver(n, rank=0, nranks=2) as s:
            assert call(s._h)() == capi.E_INVALID
            assert NAME in L.fluid_last_error() and b"slab" in L.fluid_last_error()
        torch.cuda.synchronize()
        assert (cm.cpu().numpy() == NAN32).all()
    finally:
        hip.hipFree(exact)
        hip.hipFree(exact2)


def test_the_solver_refuses_tensors_of_the_wrong_kind():
    torch = torch_()
    n, members = 6, 3
    w = n + 2
    with solver(n, members) as s:
        x = np.random.default_rng(2).uniform(-1, 1, (members, w, w)).astype(F32)
        s.upload_members(dens=x)
        good = torch.ones((1, w, w), dtype=torch.float32, device="cuda")
        for bad in (torch.ones((2, w, w), dtype=torch.float32, device="cuda"), torch.ones((1, w, w), dtype=torch.float64, device="cuda"),
                    torch.ones((1, w, 2 * w), dtype=torch.float32, device="cuda")[:, :, ::2], torch.ones((1, w, w), dtype=torch.float32)):
            with pytest.raises(ValueError):
                s.verify(bad)
            with pytest.raises(ValueError):
                s.verify(good, crps_map=bad)
        for bad in (torch.ones((1, ROW), dtype=torch.float32, device="cuda"), torch.ones((2, ROW), dtype=torch.float64, device="cuda"),
                    torch.ones((1, ROW - 1), dtype=torch.float64, device="cuda"), torch.ones((1, 2 * ROW), dtype=torch.float64, device="cuda")[:, ::2]):
            with pytest.raises(ValueError):
                s.verify(good, out=bad)
        with pytest.raises(TypeError):
            s.verify(np.ones((1, w, w), F32))
        big = torch.zeros((4, 1, ROW), dtype=torch.float64, device="cuda")
        assert s.verify(good, out=big[2]).data_ptr() == big[2].data_ptr()
        got = s.verify_scores(big[2])
        assert len(got) == 1 and got[0]["count"] == n * n and got[0]["rank_hist"].sum() == n * n
