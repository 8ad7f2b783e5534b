"""The decade sweeps of the association scan with the shared covariate block eliminated once per call — run with -m gpu on an MI355X.

At the 11 decade lambdas the block [W | y] of P and Q is the same for every SNP: setup_tabs_kernel runs the c covariate pivots on it
once (the decade table) and assoc_kernel updates only a SNP's x row, several lambdas side by side on the lanes.  Every value is
formed by the expression of the full sweeps from operands of the same bits, so every case here is bit-exact against the oracle in the
kernels' summation order, NaN patterns included.
"""
import numpy as np
import pytest

from test_gpu_assoc_powers import COLS, bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pygemma_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


_PANELS = {}


def panel(c):     # one panel per c, shared by the two search modes and never modified
    from pygemma_amd import synth
    if c not in _PANELS:
        _PANELS[c] = synth.rotated_panel(130, 24, c, seed=7)
    return _PANELS[c]


def check(z, grid, ctx):
    from oracle import oracle as O
    from pygemma_amd import ops
    got = ops.assoc(z["d"], z["W"], z["Y"], z["X"], grid=grid, ctx=ctx)
    orc = O.calculate(z["d"], z["Y"], z["W"], z["X"], grid=grid, order=1, nthreads=8)
    for col in COLS:
        want = orc[col].astype(got[col].dtype)
        assert (np.isnan(got[col]) == np.isnan(want)).all(), (col, "the NaN pattern differs")
        ne = (bits(got[col]) != bits(want)) & ~np.isnan(want)      # as test_gpu_edge.py: a NaN's payload is not compared
        assert not ne.any(), (col, int(ne.sum()), np.nonzero(ne)[0][:5], got[col][ne][:3], want[ne][:3])
    return got


# lambdas per round = 64 // (c + 2): c = 1 one covariate step, all 11 lambdas in one round; 2 one round, 16 lane groups of which 11
# work; 5 (the flagship shape) 9 + 2; 8 rounds of 6 and 5; 11 (slot-chunked Gram passes) 4 + 4 + 3; 14 (pivot column through LDS in the
# full sweeps) 4 + 4 + 3 with all 64 lanes in use.  The grid search returns decade values directly: it exposes every field of every
# decade evaluation, which the Brent path reads for signs and brackets only.
@pytest.mark.parametrize("grid", [False, True])
@pytest.mark.parametrize("c", [1, 2, 5, 8, 11, 14])
def test_decade_values_every_round_shape(c, grid, ctx):
    got = check(panel(c), grid, ctx)
    if grid:
        decades = (10.0 ** np.arange(-5, 6)).astype(np.float32).astype(np.float64)
        assert np.isin(got["lambda"], decades).all()


@pytest.mark.parametrize("grid", [False, True])
def test_degenerate_x_rows_drive_the_clamps(grid, ctx):
    """c = 5, n = 130: an all-zero rotated x ((x, x) clamps to PG_MINV at the last covariate step), x equal to a covariate column
    ((x, x) after the covariate steps is rounding noise or clamped), x equal to y — among ordinary SNPs, so that a lane group
    working on a degenerate row sits beside groups that do not."""
    z = dict(panel(5))
    X = z["X"].copy()
    X[:, 3] = 0.0
    X[:, 7] = z["W"][:, 0]
    X[:, 11] = z["W"][:, 4]
    X[:, 15] = z["Y"].reshape(-1)
    z["X"] = X
    check(z, grid, ctx)


def test_lrt_reads_the_decade_values():
    """The ML candidates of the LRT read yPy, yPPy and sh of every decade evaluation: the LRT columns against the oracle as
    test_gpu_lrt.py compares them, the Wald columns bit-exact."""
    from oracle import oracle as O
    from pygemma_amd import lmm, synth
    rp = synth.rotated_panel(300, 40, 5, seed=305, h2=0.4)
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
