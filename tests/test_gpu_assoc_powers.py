"""Which Gram powers the association scan's SNP-specific evaluations compute — run with -m gpu on an MI355X.

The evaluation at a root makes P alone, and Newton's first evaluation takes P and Q from Brent when it starts at one of the last
two lambdas Brent evaluated.  Neither may change a result bit (every Gram entry is its own fma chain; only the grouping of entries
into passes differs), so every case is bit-exact against the oracle in the kernels' summation order, and the pass counters of
pg_assoc_set_pass_stats say which path ran.

Roots are counted from the oracle's evaluation count, independently of the pass counters: per SNP the oracle makes 13 two-power
evaluations at the shared lambdas, and per root Brent's two endpoint re-evaluations, Brent's own points and the one at the root;
the GPU counts the last two only.  Hence roots = (oracle fast - 13 p - GPU fast) / 2.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(__file__), "golden")
COLS = ["beta", "se_beta", "tau", "lambda", "F_wald"]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64)


@pytest.fixture(scope="module")
def ctx():
    from pygemma_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def run_and_check(z, ctx):
    """ops.assoc on the Brent path against oracle.calculate(order=1): bit-equal columns, equal Newton count, and the pass
    accounting.  Returns (roots, reuse)."""
    from oracle import oracle as O
    from pygemma_amd import ops
    got = ops.assoc(z["d"], z["W"], z["Y"], z["X"], grid=False, ctx=ctx, return_stats=True)
    orc = O.calculate(z["d"], z["Y"], z["W"], z["X"], grid=False, order=1, nthreads=8)
    p = len(got["beta"])
    for col in COLS:
        ne = bits(got[col]) != bits(orc[col].astype(got[col].dtype))
        assert not ne.any(), (col, int(ne.sum()), np.nonzero(ne)[0][:5], got[col][ne][:3], orc[col][ne][:3])
    n_fast, n_full = (int(v) for v in got["n_evals"])
    assert n_full == int(orc["n_evals"][1])
    twice_roots = int(orc["n_evals"][0]) - 13 * p - n_fast
    assert twice_roots >= 0 and twice_roots % 2 == 0, (orc["n_evals"], got["n_evals"])
    roots = twice_roots // 2
    P, Q, R, reuse = (int(v) for v in got["passes"])
    print(f"p={p} roots={roots} n_fast={n_fast} n_full={n_full} passes P={P} Q={Q} R={R} reuse={reuse}")
    assert P == n_fast + n_full - reuse
    assert R == n_full
    assert P - Q == roots                      # the evaluations at the roots, P alone
    assert Q == n_fast + n_full - reuse - roots
    return roots, reuse


# every Shape branch at the smallest n that exercises the element loop: c = 1 the smallest, 5 P, Q, R fused, 6 P, Q fused and R
# separate, 7 nothing fused, 11 chunked with two slots, 14 three slots and the pivot exchange through LDS; n = 130 is three element
# iterations, the last one mostly pad rows, and the depth-2 prefetch ring wraps
@pytest.mark.parametrize("c", [1, 5, 6, 7, 11, 14])
def test_every_shape_branch(c, ctx):
    from pygemma_amd import synth
    rp = synth.rotated_panel(130, 24, c, seed=7)
    roots, reuse = run_and_check(rp, ctx)
    assert roots >= 1
    assert 1 <= reuse <= roots


def test_fallback_and_reuse_both_run_on_the_weak_panel(ctx):
    # 142 of 172 Newton starts are among Brent's last two lambdas on the CPU oracle; the rest take all three powers
    z = np.load(os.path.join(G, "panel_weak_n300_c3.npz"))
    roots, reuse = run_and_check(z, ctx)
    assert 0 < reuse < roots


def test_reuse_is_the_rule_on_the_signal_panel(ctx):
    z = np.load(os.path.join(G, "panel_signal_n400_c5.npz"))   # 300 of 300 on the CPU oracle
    roots, reuse = run_and_check(z, ctx)
    assert reuse >= 0.95 * roots


def test_grid_counts_nothing_and_null_writes_nothing(ctx):
    from pygemma_amd import _lib, ops
    L = _lib.load()
    z = np.load(os.path.join(G, "panel_signal_n257_c1.npz"))
    CANARY = np.uint64(0xA5A5A5A55A5A5A5A)
    buf = ctx.to_device(np.array([0, 0, 0, 0, CANARY], np.uint64))   # the four counters and a canary word after them
    try:
        _lib.check(L.pg_assoc_set_pass_stats(ctx.handle, buf.ptr), "pg_assoc_set_pass_stats")
        try:
            ops.assoc(z["d"], z["W"], z["Y"], z["X"], grid=True, ctx=ctx)
            assert buf.download((5,), np.uint64).tolist() == [0, 0, 0, 0, int(CANARY)]
            ops.assoc(z["d"], z["W"], z["Y"], z["X"], grid=False, ctx=ctx)
            counted = buf.download((5,), np.uint64)
            assert counted[0] > 0 and counted[4] == CANARY
        finally:
            _lib.check(L.pg_assoc_set_pass_stats(ctx.handle, None), "pg_assoc_set_pass_stats")
        ops.assoc(z["d"], z["W"], z["Y"], z["X"], grid=False, ctx=ctx)
        assert (buf.download((5,), np.uint64) == counted).all()
    finally:
        buf.free()
