"""Where the planted-cell tests (test_gpu_planted_cells.py) put their one offending cell, and the proof -- on the CPU, with
no device -- that those places cover every class of position the reductions' indexing tells apart.

k_absmax2 reads whole 4-float vectors (the last one masked), 256 vectors per pass of its column loop (columns 1024 / 1025
meet between two passes) and 1024 rows per pass of its row loop; k_residual walks 256 columns per pass and the same rows;
k_subtract_gradient_max cuts a row into blocks of 256 columns.  A cell is dropped, or a ghost / pad float counted, per
class of (row, column) -- first, last, on either side of such a seam, on a given lane of the last vector -- never per cell:
so the sets below hold every column of the edge rows, every row of the edge columns, and both sides of every seam, and
nothing else.  No placement is skipped at run time: the sets are what runs."""
import pytest

# what test_gpu_planted_cells.py sweeps with the reductions: (n, column periods, row periods) -> cells, stated so that the
# GPU time stays bounded (a placement is two row uploads and a handful of reductions)
COL_PERIODS, ROW_PERIODS = (4, 256, 1024), (1024,)
LARGE = {1028: 9232, 1030: 9250}
SMALL = range(1, 10)


def seams(n, periods):
    """the cells on both sides of every multiple of every period, within 1..n"""
    return sorted({c for p in periods for m in range(p, n + 1, p) for c in (m, m + 1) if 1 <= c <= n})


def positions(n, col_periods, row_periods, extra_cols=(), extra_rows=()):
    """A deterministic, row-major list of (row, column) interior cells: every cell if n <= 9; otherwise every column of rows
    {1, 2, n-1, n} and of `extra_rows`, every row of columns {1, 2, n-1, n} and of `extra_cols`, and, for each period, the
    cells on both sides of every multiple of it: the seam columns on every row named here (the seam rows included), the
    seam rows on every column named here."""
    span = range(1, n + 1)
    if n <= 9:
        return [(i, j) for i in span for j in span]
    inside = lambda s: {k for k in s if 1 <= k <= n}
    line_rows, line_cols = inside({1, 2, n - 1, n} | set(extra_rows)), inside({1, 2, n - 1, n} | set(extra_cols))
    rows, cols = line_rows | set(seams(n, row_periods)), line_cols | set(seams(n, col_periods))
    cells = {(i, j) for i in line_rows for j in span} | {(i, j) for i in span for j in line_cols}
    cells |= {(i, j) for i in rows for j in cols}
    return sorted(cells)


def lines(n, rows, cols):
    """every column of `rows` and every row of `cols`, row-major"""
    span = range(1, n + 1)
    return sorted({(i, j) for i in rows for j in span} | {(i, j) for i in span for j in cols})


def corners(n):
    return [(1, 1), (1, n), (n, 1), (n, n)]


def check_classes(n, cells, col_periods, row_periods):
    cols, rows = {j for _, j in cells}, {i for i, _ in cells}
    assert len(set(cells)) == len(cells) and cells == sorted(cells)
    assert all(1 <= i <= n and 1 <= j <= n for i, j in cells)
    assert n in cols and (n % 4 != 0 or n - 3 in cols)
    last = 4 * ((n - 1) // 4)                             # the last vector holds columns last + 1 .. n
    for row in (1, n):                                    # ... every lane of it that is a column, on the edge rows
        assert all((row, j) in cells for j in range(last + 1, n + 1))
    assert {j % 4 for j in range(last + 1, n + 1)} <= {j % 4 for j in cols if j > last}
    for p in col_periods:
        if p + 1 <= n:
            assert p in cols and p + 1 in cols, "columns %d / %d" % (p, p + 1)
            assert all((i, j) in cells for i in (1, n) for j in (p, p + 1))
    for p in row_periods:
        if p + 1 <= n:
            assert p in rows and p + 1 in rows, "rows %d / %d" % (p, p + 1)
            assert all((i, j) in cells for i in (p, p + 1) for j in (1, n))
            assert all((i, j) in cells for i in (p, p + 1) for q in col_periods if q + 1 <= n for j in (q, q + 1))
    assert set(corners(n)) <= set(cells)


@pytest.mark.parametrize("n", SMALL)
def test_small_grids_plant_every_cell(n):
    cells = positions(n, COL_PERIODS, ROW_PERIODS)
    assert len(cells) == n * n and set(cells) == {(i, j) for i in range(1, n + 1) for j in range(1, n + 1)}
    check_classes(n, cells, COL_PERIODS, ROW_PERIODS)


@pytest.mark.parametrize("n", sorted(LARGE))
def test_large_grids_plant_every_class(n):
    cells = positions(n, COL_PERIODS, ROW_PERIODS)
    check_classes(n, cells, COL_PERIODS, ROW_PERIODS)
    # every column of the edge rows and every row of the edge columns: the sweeps that carry the lane and stride classes
    for k in (1, 2, n - 1, n):
        assert all((k, j) in cells and (j, k) in cells for j in range(1, n + 1))
    # rows of the row loop's second pass (1025 ..) with every column: rows n - 1 and n are such rows
    assert n - 1 > 1024
    assert len(cells) == LARGE[n] and len(cells) < 10 * n, len(cells)


def test_positions_are_deterministic_and_take_extras():
    assert positions(1030, COL_PERIODS, ROW_PERIODS) == positions(1030, COL_PERIODS, ROW_PERIODS)
    cells = positions(40, (16,), (), extra_cols=(7,), extra_rows=(9, 99))
    assert all((i, 7) in cells for i in range(1, 41)) and all((9, j) in cells for j in range(1, 41))
    assert {16, 17, 32, 33} <= {j for i, j in cells if i == 9} and not any(i == 99 for i, _ in cells)
    assert (20, 16) not in cells and (20, 20) not in cells            # mid-field cells stay out


def test_lines():
    cells = lines(225, (1, 114, 225), (1, 96, 225))
    assert len(cells) == 6 * 225 - 9 and set(corners(225)) <= set(cells)
    assert all((114, j) in cells and (j, 96) in cells for j in range(1, 226))
