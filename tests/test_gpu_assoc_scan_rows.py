"""The decade scan on its packed rows — run with -m gpu on an MI355X.

The scan of assoc_kernel reads one SNP-independent row per element (w, y and h at the 11 decade lambdas, a copy of what the fixed rows
and the h table hold) through a two-slot register ring whose loads are issued a whole element ahead.  Only where the operands come
from and when they are loaded differs from the scan on the two tables: every case here is bit-exact against the oracle in the
kernels' summation order, NaN patterns included (the comparison of test_gpu_assoc_decade.py).

Decade lambdas per scan pass (Shape<C>::G = assoc_scan_lams(c)): 64 accumulators up to c = 2 and at c = 14, 96 elsewhere, over
2 (c + 2) entries per lambda.  c = 0: one pass of 11; 1: 10 + 1; 2: 8 + 3; 3: 9 + 2; 5: 6 + 5; 8 and 10: 4 + 4 + 3; 11: 3 + 3 + 3 + 2;
14, 15 and 18 to 22: five passes of 2 and one of 1; 23 and 30: 11 passes of 1.  c = 19 to 22 do not read the packed rows: their scan
stays on the fixed rows and the h table (assoc_scan_packed), so 18 and 23 are the last and the first c on either side of that switch.
"""
import numpy as np
import pytest

from test_gpu_assoc_decade import check
from test_gpu_assoc_powers import COLS, bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pygemma_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


_PANELS = {}


def panel(n, p, c):     # one panel per shape, shared by the search modes and never modified
    from pygemma_amd import synth
    if (n, p, c) not in _PANELS:
        _PANELS[(n, p, c)] = synth.rotated_panel(n, p, c, seed=7)
    return _PANELS[(n, p, c)]


# one, two or three element-iterations of the ring (64 elements each), odd and even counts, a last iteration of 1, 63 or 64 live
# rows; p = 7: the last workgroup holds one wave.  The grid search returns decade values directly and exposes every scan entry.
@pytest.mark.parametrize("grid", [False, True])
@pytest.mark.parametrize("c", [1, 5, 14])
@pytest.mark.parametrize("n", [64, 65, 127, 128, 129, 191, 193])
def test_ring_edges(n, c, grid, ctx):
    check(panel(n, 7, c), grid, ctx)


@pytest.mark.parametrize("grid", [False, True])
@pytest.mark.parametrize("c", [1, 2, 3, 5, 8, 10, 11, 14, 15, 18, 19, 20, 21, 22, 23, 30])
def test_every_pass_shape(c, grid, ctx):
    got = check(panel(130, 24, c), grid, ctx)
    if grid:
        decades = (10.0 ** np.arange(-5, 6)).astype(np.float32).astype(np.float64)
        assert np.isin(got["lambda"], decades).all()


def lrt_against_oracle(n, p, c, seed):
    """The LRT entry point as test_gpu_assoc_decade.py::test_lrt_reads_the_decade_values compares it: the ML candidates read yPy,
    yPPy and sh of every decade evaluation; the null model runs the kernel of c - 1 covariates."""
    from oracle import oracle as O
    from pygemma_amd import lmm, synth
    rp = synth.rotated_panel(n, p, c, seed=seed, h2=0.4)
    df = lmm.pygemma(rp["Y"], rp["X"], rp["W"], rp["d"], eigen=False, lrt=True)
    orc = O.calculate_lrt(rp["d"], rp["Y"], rp["W"], rp["X"], order=1, nthreads=8)
    ulp = np.spacing(np.float32(abs(orc["l_null"])))
    assert abs(df["l_null"].to_numpy()[0] - orc["l_null"]) <= ulp
    assert np.abs(df["l_alt"].to_numpy() - orc["l_alt"]).max() <= ulp
    assert (bits(df["l_alt"].to_numpy().astype(np.float32)) == bits(orc["l_alt"])).mean() >= 0.9
    np.testing.assert_allclose(df["p_lrt"].to_numpy(), orc["p_lrt"], rtol=5e-3)
    wald = O.calculate(rp["d"], rp["Y"], rp["W"], rp["X"], grid=False, order=1, nthreads=8)
    for col in COLS:
        a = df[col].to_numpy()
        assert (bits(a) == bits(wald[col].astype(a.dtype))).all(), col


def test_lrt_entry_point():
    """n = 413: seven element-iterations, the last with 29 live rows."""
    lrt_against_oracle(413, 33, 5, seed=311)


def test_lrt_null_model_without_covariates():
    """c = 1: the null model is the kernel of c = 0, all 11 decade lambdas in one scan pass."""
    lrt_against_oracle(130, 24, 1, seed=306)


def test_second_call_rebuilds_the_rows(ctx):
    """Two calls on one context with different n and c, then the first again: each call's rows are its own."""
    check(panel(193, 7, 14), False, ctx)
    check(panel(130, 24, 5), True, ctx)
    check(panel(193, 7, 14), True, ctx)


def test_strided_block(ctx):
    """pg_assoc_dev on a SNP-major block whose row pitch is wider than n rounded up to 64, the pad filled with NaN: the scan reads x
    at min(i, n - 1) and nothing behind it."""
    from oracle import oracle as O
    from pygemma_amd import _lib
    L = _lib.load()
    n, p, c = 129, 7, 5
    z = panel(n, p, c)
    ldx = 192 + 64
    Xr = np.full((p, ldx), np.nan, np.float32)
    Xr[:, :n] = z["X"].T
    dd, dW, dy, dX = (ctx.to_device(np.ascontiguousarray(a, dtype=np.float32)) for a in (z["d"], z["W"], z["Y"].reshape(-1), Xr))
    out = [ctx.alloc(p * 4) for _ in range(4)] + [ctx.alloc(p * 8)]
    for grid in (0, 1):
        _lib.check(L.pg_assoc_dev(ctx.handle, n, c, p, dd.ptr, dW.ptr, dy.ptr, dX.ptr, ldx, grid, *[b.ptr for b in out], None, None),
                   "pg_assoc_dev")
        ctx.sync()
        orc = O.calculate(z["d"], z["Y"], z["W"], z["X"], grid=bool(grid), order=1, nthreads=8)
        for k, col in enumerate(COLS):
            got = out[k].download((p,), np.float32 if k < 4 else np.float64)
            want = orc[col].astype(got.dtype)
            assert (np.isnan(got) == np.isnan(want)).all(), (col, grid, "the NaN pattern differs")
            ne = (bits(got) != bits(want)) & ~np.isnan(want)
            assert not ne.any(), (col, grid, int(ne.sum()))
