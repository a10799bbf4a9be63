"""GPU: FLUID_PARAM_TB_FILL.  The fused Jacobi kernel skips the stage evaluations of each strip's pipeline fill (and of
the surplus steps past its last row) that no stored row depends on.  Results must not depend on it: every launch shape
is run with the switch on and off and must agree bit for bit -- strip heights around the pipeline depth T, every depth,
division mode, lane width and storage type, the divergence- and source-fused first launches, edge windows, slabs whose
first launch is split around an exchange -- and with the oracle at a few sizes."""
import numpy as np
import pytest

from conftest import assert_bit_equal, rnd

pytestmark = pytest.mark.gpu

DT, VISC, DIFF = 0.016, 0.0025, 0.1


@pytest.fixture(scope="module")
def F():
    import fluidsimulationcuda_amd as F
    return F


def heights(T):
    return sorted({1, 2, max(1, T - 1), T, 2 * T - 1, 2 * T, 3 * T + 1, 97})


def diffuse_both(F, n, storage, params, fields, solves, rows_list):
    """Each solve (b, alpha, beta, iters) on each pair of fields at each strip height, with TB_FILL = 1 and 0 in two
    contexts; yields (what, result with fill, result without)."""
    from fluidsimulationcuda_amd import capi
    ctx = [F.FluidSolver(n, jacobi=capi.JACOBI_TB, storage=storage, params={**params, capi.PARAM_TB_FILL: f}) for f in (1, 0)]
    try:
        for rows in rows_list:
            for s in ctx:
                s.set_param(capi.PARAM_TB_ROWS, rows)
            for i, (x, x0) in enumerate(fields):
                for b, alpha, beta, iters in solves:
                    got = []
                    for s in ctx:
                        s.upload(u=x, v=x0)
                        s.diffuse(b, "u", "v", alpha, beta, iters)
                        got.append(s.download("u"))
                    yield "rows=%d fields=%d solve=%r" % (rows, i, (b, alpha, beta, iters)), got[0], got[1]
    finally:
        for s in ctx:
            s.close()


@pytest.mark.parametrize("storage", [0, 1])
@pytest.mark.parametrize("T,lane_cols", [(2, 2), (2, 4), (4, 2), (4, 4), (8, 2), (8, 4), (12, 2), (16, 2)])
@pytest.mark.parametrize("fast_div", [0, 1, 2, 3])
def test_fill_switch_is_bit_identical(F, T, lane_cols, fast_div, storage):
    """One launch of depth T per solve (iters = T), both forms: the pressure form divides by 4 (mode 4), the general form
    in mode 0 / 3 / 5 / 2 (fast_div 0 / 1 / 2 / 3).  n = 250 has edge windows and interior ones, and walls at both ends
    of the strips next to them; every strip height of heights(T)."""
    from fluidsimulationcuda_amd import capi
    n = 250
    rng = np.random.default_rng(1000 + 10 * T + fast_div)
    fields = [(rnd(rng, n), rnd(rng, n))]
    solves = [(0, 1.0, 4.0, T), (1, *F.coefficients(n, DT, VISC), T), (2, 0.7, 3.3, T)]
    params = {capi.PARAM_TB_MIN_CELLS: 0, capi.PARAM_TB_T16_MIN_CELLS: 0, capi.PARAM_TB_MAX_SWEEPS: T,
              capi.PARAM_TB_LANE_COLUMNS: lane_cols, capi.PARAM_TB_FAST_DIVISION: fast_div}
    for what, on, off in diffuse_both(F, n, storage, params, fields, solves, heights(T)):
        assert_bit_equal(on, off, "T=%d cols=%d div=%d st=%d %s" % (T, lane_cols, fast_div, storage, what))


@pytest.mark.parametrize("T", [2, 4, 8, 12, 16])
def test_fill_switch_special_values(F, T):
    """Signed zeros (dyadic fields: exact cancellations everywhere) and a field holding inf and NaN, which sends every
    mode-5 wave that meets it through its second pass: fill on == fill off."""
    from fluidsimulationcuda_amd import capi
    n = 126
    rng = np.random.default_rng(7 + T)
    vals = np.array([-1, -0.5, -0.25, 0.0, -0.0, 0.25, 0.5, 1], np.float32)
    dy = [(rng.choice(vals, size=(n + 2, n + 2)).astype(np.float32), rng.choice(vals, size=(n + 2, n + 2)).astype(np.float32))]
    bad = rnd(rng, n)
    bad[40, 50], bad[90, 7], bad[3, 120] = np.inf, np.nan, -np.inf
    special = [(rnd(rng, n), bad), (bad.copy(), rnd(rng, n))]
    solves = [(0, 1.0, 4.0, T), (1, *F.coefficients(n, DT, VISC), T), (0, 0.7, 3.3, T)]
    params = {capi.PARAM_TB_MIN_CELLS: 0, capi.PARAM_TB_T16_MIN_CELLS: 0, capi.PARAM_TB_MAX_SWEEPS: T}
    for what, on, off in diffuse_both(F, n, 0, params, dy + special, solves, (max(1, T - 1), 2 * T, 97)):
        assert_bit_equal(on, off, "T=%d %s" % (T, what))


@pytest.mark.parametrize("n", [61, 257, 1022])
def test_fill_matches_oracle(F, oracle, n):
    """Fill on (the default), 40 sweeps of each form at the deepest launches, default and short strips: the oracle's bits."""
    from fluidsimulationcuda_amd import capi
    rng = np.random.default_rng(n)
    for rows in (0, 3, 17, 33):
        with F.FluidSolver(n, jacobi=capi.JACOBI_TB, params={capi.PARAM_TB_MIN_CELLS: 0, capi.PARAM_TB_T16_MIN_CELLS: 0,
                                                             capi.PARAM_TB_ROWS: rows}) as s:
            for b, (alpha, beta) in ((0, (1.0, 4.0)), (2, F.coefficients(n, DT, DIFF))):
                x, x0 = rnd(rng, n), rnd(rng, n)
                s.upload(u=x, v=x0)
                s.diffuse(b, "u", "v", alpha, beta, 40)
                want = x.copy()
                oracle.diffuse(b, want, x0, alpha, beta, 40)
                assert_bit_equal(s.download("u"), want, "n=%d rows=%d b=%d" % (n, rows, b))


@pytest.mark.parametrize("storage", [0, 1])
@pytest.mark.parametrize("n,rows,max_t", [(254, 0, 16), (254, 15, 16), (254, 33, 12), (510, 97, 16), (126, 7, 8)])
def test_fill_switch_whole_steps(F, n, rows, max_t, storage):
    """Whole steps: the first launch of each diffusion adds the sources (ADDSRC), the first launch of each pressure solve
    forms the divergence (DIVSRC); fill on == fill off on every field."""
    from fluidsimulationcuda_amd import capi
    from fluidsimulationcuda_amd.harness import initialize_parameters
    fields = initialize_parameters(n, seed=3)
    got = []
    for fill in (1, 0):
        with F.FluidSolver(n, storage=storage, params={capi.PARAM_TB_MIN_CELLS: 0, capi.PARAM_TB_T16_MIN_CELLS: 0,
                                                       capi.PARAM_TB_ROWS: rows, capi.PARAM_TB_MAX_SWEEPS: max_t,
                                                       capi.PARAM_TB_FILL: fill}) as s:
            s.upload(**fields)
            s.step(1, use_sources=True)
            s.step(2)
            got.append({k: s.download(k) for k in ("u", "v", "dens", "u_prev", "v_prev", "dens_prev")})
    for k in got[0]:
        assert_bit_equal(got[0][k], got[1][k], "%s n=%d rows=%d max_t=%d st=%d" % (k, n, rows, max_t, storage))


@pytest.mark.parametrize("n,nranks,halo,rows", [(1022, 2, 42, 0), (1022, 4, 0, 13), (510, 3, 8, 0)])
def test_fill_switch_on_slabs_split_around_the_exchange(n, nranks, halo, rows):
    """Row slabs with the exchange beside the compute: the first launch of a solve runs as an interior part and the edge
    part around its hole (strips begin at the hole's end).  Fill on == fill off == one context, and the split happened."""
    from fluidsimulationcuda_amd import capi
    from test_gpu_slab import run_ranks, single, synthetic
    fields = synthetic(n, seed=11)
    splits = {}

    def body(s):
        s.step(1, use_sources=True)
        s.step(2)
        splits[s.rank] = s.split_launches()

    want = single(n, fields, body)
    for fill in (1, 0):
        splits.clear()
        got, _ = run_ranks(n, nranks, halo, fields, body, jacobi=3,
                           params={capi.PARAM_XCHG_OVERLAP: 1, capi.PARAM_TB_FILL: fill, capi.PARAM_TB_ROWS: rows})
        assert all(v > 0 for v in splits.values()), splits
        for k in ("u", "v", "dens"):
            assert_bit_equal(got[k], want[k], "%s fill=%d, %d slabs halo %d rows %d" % (k, fill, nranks, halo, rows))
