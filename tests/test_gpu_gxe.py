"""GPU tests of the SNP-by-environment interaction scan (pg_assoc_gxe_dev, ops.gxe, lmm.pygemma_gxe) — run with -m gpu on an MI355X.

Row j is by definition calculate(d, yr, [W', xr_j], xer_j) with W' = [U'W, U'e], xr_j = U'x_j, xer_j = U'(x_j o e):
  * vs the oracle in the kernels' summation order (order=1): bit-exact;
  * vs the oracle in the reference's order (order=0): SURVEY 8c Tier A (>= 99 % of rows bit-identical, the rest within 2e-5 in
    lambda and 1e-4 in beta, se, p);
  * end to end against an fp64 truth (host eigh, fp64 rotations, fp64 REML with the same lambda-selection rule).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COLS5 = ("beta", "se_beta", "tau", "lambda", "F_wald")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64)


@pytest.fixture(scope="module")
def ctx():
    from pygemma_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _raw(n, p, c, e_kind, null, seed, planted=(3, 17, 40), effect=0.6):
    """Raw inputs (Y, X, W, K, e) from synth.panel, with an interaction of size `effect` planted in the SNPs `planted` unless null."""
    from pygemma_amd import synth
    raw = synth.panel(n, p, c, seed=seed, null=null)
    rng = np.random.default_rng(seed + 1)
    e = (rng.integers(0, 2, n) if e_kind == "binary" else rng.standard_normal(n)).astype(np.float32)
    y = raw["Y"].reshape(-1).astype(np.float64) + 0.3 * e
    if not null:
        for j in planted:
            if j < p:
                y += effect * raw["X"][:, j] * e
    return y.astype(np.float32).reshape(-1, 1), raw["X"], raw["W"], raw["K"], e


def _rotated(Y, X, W, K, e):
    """Eigen-basis inputs rotated in fp64 on the host: d, W' = U'[W, e], yr, U'X, U'(X o e) (float32)."""
    d, U = np.linalg.eigh(K.astype(np.float64))
    d = np.maximum(d, 0.0).astype(np.float32)
    rot = lambda A: (U.T @ np.asarray(A, np.float64)).astype(np.float32)
    X64 = X.astype(np.float64)
    return d, rot(np.c_[W, e]), rot(Y).reshape(-1), rot(X64), rot(X64 * e.astype(np.float64)[:, None])


def _oracle(d, Wp, yr, Xr, XEr, order):
    from oracle import oracle as O
    p = Xr.shape[1]
    out = {k: np.empty(p, np.float32) for k in ("beta", "se_beta", "tau")}
    out.update({k: np.empty(p, np.float64) for k in ("lambda", "F_wald", "p_wald")})
    for j in range(p):
        r = O.calculate(d, yr, np.c_[Wp, Xr[:, j]], XEr[:, j:j + 1], order=order)
        for k in out:
            out[k][j] = r[k][0]
    return out


# n in {257, 400, 2000}, W columns in {1, 5, 10, 28}, binary and continuous e, null and planted-signal phenotypes
TIER_A = [(257, 1, "binary", False), (257, 28, "continuous", True), (400, 5, "continuous", False), (400, 10, "binary", True),
          (400, 28, "binary", False), (2000, 1, "continuous", True), (2000, 5, "binary", False), (2000, 10, "continuous", False)]


@pytest.mark.parametrize("n,c,e_kind,null", TIER_A)
def test_kernel_vs_oracle(n, c, e_kind, null, ctx):
    from pygemma_amd import ops
    p = 120 if n <= 400 else 60
    d, Wp, yr, Xr, XEr = _rotated(*_raw(n, p, c, e_kind, null, seed=n + 7 * c))
    got = ops.gxe(d, Wp, yr, Xr, XEr, ctx=ctx)
    # 1) bit-exact vs the oracle in the kernels' order
    o1 = _oracle(d, Wp, yr, Xr, XEr, order=1)
    for col in COLS5:
        ne = bits(got[col]) != bits(o1[col].astype(got[col].dtype))
        assert not ne.any(), (col, int(ne.sum()), np.nonzero(ne)[0][:5])
    np.testing.assert_allclose(got["p_wald"], o1["p_wald"], rtol=1e-9)
    # 2) Tier A vs the oracle in the reference's order
    o0 = _oracle(d, Wp, yr, Xr, XEr, order=0)
    rowbad = np.zeros(p, bool)
    for col in COLS5:
        rowbad |= bits(got[col]) != bits(o0[col].astype(got[col].dtype))
    assert rowbad.mean() <= 0.01, int(rowbad.sum())
    np.testing.assert_allclose(got["p_wald"][~rowbad], o0["p_wald"][~rowbad], rtol=1e-9)
    for col, tol in (("beta", 1e-4), ("se_beta", 1e-4), ("lambda", 2e-5), ("p_wald", 1e-4)):
        np.testing.assert_allclose(np.asarray(got[col], np.float64)[rowbad], np.asarray(o0[col], np.float64)[rowbad], rtol=tol,
                                   err_msg=col)
    assert np.isfinite(got["F_wald"]).all()


def test_degenerate_snps_give_the_oracles_nan_rows(ctx):
    """A constant SNP, a zero SNP, x o e in span([W', x]) (binary e, x non-zero only where e = 1; x = e), non-finite SNPs, and a
    rank-deficient W': the NaN pattern of the oracle, bit-identical values elsewhere, nothing raises."""
    from pygemma_amd import ops
    rng = np.random.default_rng(5)
    n, c = 203, 3
    d = np.sort(rng.gamma(0.5, 2.0, n)).astype(np.float32)
    W = np.c_[np.ones(n), rng.standard_normal((n, c - 1))].astype(np.float32)
    e = rng.integers(0, 2, n).astype(np.float32)
    X = (rng.binomial(2, 0.3, size=(n, 12)) - 0.6).astype(np.float32)
    X[:, 0] = 3.0
    X[:, 1] = 0.0
    X[:, 2] = np.where(e == 1, X[:, 2], 0.0)          # x o e = x
    X[:, 3] = e
    X[3, 4] = np.nan
    X[5, 5] = np.inf
    X[7, 6] = -np.inf
    y = (W @ rng.standard_normal(c) + 0.5 * X[:, 7] * e + rng.standard_normal(n)).astype(np.float32)
    XE = X * e[:, None]
    for Wp in (np.c_[W, e], np.c_[W, W[:, 1:2], e]):
        Wp = np.ascontiguousarray(Wp, np.float32)
        got = ops.gxe(d, Wp, y, X, XE, ctx=ctx)
        o1 = _oracle(d, Wp, y, X, XE, order=1)
        for col in COLS5 + ("p_wald",):
            g, o = np.asarray(got[col]), np.asarray(o1[col], got[col].dtype)
            assert (np.isnan(g) == np.isnan(o)).all(), col
            fin = ~np.isnan(o)
            if col != "p_wald":
                assert (bits(g[fin]) == bits(o[fin])).all(), col
        assert np.isnan(got["beta"][4:7]).all()


def _call_dev(ctx, d, Wp, yr, Xsm, XEsm, ldx, ldxe):
    """pg_assoc_gxe_dev on SNP-major rows laid out at row strides ldx / ldxe (pads filled with NaN: never read)."""
    from pygemma_amd import _lib
    L = _lib.load()
    n, c = Wp.shape
    p = Xsm.shape[0]
    A = np.full((p, ldx), np.nan, np.float32); A[:, :n] = Xsm
    B = np.full((p, ldxe), np.nan, np.float32); B[:, :n] = XEsm
    bufs = [ctx.to_device(np.ascontiguousarray(v, np.float32)) for v in (d, Wp, yr, A, B)]
    out = [ctx.alloc(p * 4) for _ in range(4)] + [ctx.alloc(p * 8) for _ in range(2)]
    _lib.check(L.pg_assoc_gxe_dev(ctx.handle, n, c, p, *[b.ptr for b in bufs[:4]], ldx, bufs[4].ptr, ldxe, *[b.ptr for b in out], None),
               "pg_assoc_gxe_dev")
    ctx.sync()
    res = [b.download((p,), np.float32 if k < 4 else np.float64) for k, b in enumerate(out)]
    for b in bufs + out:
        b.free()
    return res


def test_rows_depend_only_on_their_snp(ctx):
    from pygemma_amd import ops
    d, Wp, yr, Xr, XEr = _rotated(*_raw(384, 301, 4, "continuous", False, seed=9))
    ref = ops.gxe(d, Wp, yr, Xr, XEr, ctx=ctx)
    perm = np.random.default_rng(1).permutation(301)
    got = ops.gxe(d, Wp, yr, Xr[:, perm], XEr[:, perm], ctx=ctx)
    for col in COLS5 + ("p_wald",):
        assert (bits(got[col]) == bits(ref[col][perm])).all(), col
    base = _call_dev(ctx, d, Wp, yr, Xr.T, XEr.T, 384, 384)
    for ldx, ldxe in ((448, 384), (384 + 37, 512), (1000, 401)):
        other = _call_dev(ctx, d, Wp, yr, Xr.T, XEr.T, ldx, ldxe)
        for a, b in zip(base, other):
            assert (bits(a) == bits(b)).all(), (ldx, ldxe)
    for a, col in zip(base, COLS5 + ("p_wald",)):
        assert (bits(a) == bits(np.asarray(ref[col], a.dtype))).all(), col


def test_abi_misuse_launches_nothing(ctx):
    """Every refused call returns its code and writes nothing: the output and stats buffers keep their sentinel bytes.  A valid call
    with the same buffers then does write them (the check can see a launch)."""
    from pygemma_amd import _lib
    L = _lib.load()
    rng = np.random.default_rng(8)
    n, c, p = 64, 3, 8
    d = np.sort(rng.gamma(0.5, 2.0, n)).astype(np.float32)
    Wp = np.c_[np.ones(n), rng.standard_normal((n, c - 1))].astype(np.float32)
    y, X, XE = (rng.standard_normal(s).astype(np.float32) for s in (n, (p, n), (p, n)))
    dd, dW, dy, dX, dXE = (ctx.to_device(v) for v in (d, Wp, y, X, XE))
    nb = 1 << 16
    sent = ctx.alloc(nb)
    _lib.check(L.pg_memset(ctx.handle, sent.ptr, 0xA5, nb), "pg_memset")
    o = sent.ptr
    outs = (o, o + 4 * p, o + 8 * p, o + 12 * p, o + 16 * p, o + 32 * p, o + 48 * p)   # beta se tau lambda F p stats

    def call(n=n, c=c, ldx=n, ldxe=n, xr=dX.ptr):
        return L.pg_assoc_gxe_dev(ctx.handle, n, c, p, dd.ptr, dW.ptr, dy.ptr, xr, ldx, dXE.ptr, ldxe, *outs)
    assert call(c=0) == -95
    assert call(c=30) == -95
    assert call(n=10, c=8, ldx=10, ldxe=10) == -22       # n - c - 2 = 0
    assert call(ldx=n - 1) == -22
    assert call(ldxe=10) == -22
    assert call(xr=None) == -22
    assert L.pg_assoc_gxe_dev(None, n, c, p, dd.ptr, dW.ptr, dy.ptr, dX.ptr, n, dXE.ptr, n, *outs) == -22
    assert L.pg_assoc_gxe_warm(ctx.handle, n, 30) == -95
    assert L.pg_gxe_scale_u_dev(ctx.handle, n, dX.ptr, n - 1, dd.ptr, o) == -22
    assert L.pg_gxe_scale_u_dev(ctx.handle, n, dX.ptr, n, None, o) == -22
    ctx.sync()
    assert (sent.download((nb,), np.uint8) == 0xA5).all()
    _lib.check(L.pg_memset(ctx.handle, o + 48 * p, 0, 16), "pg_memset")
    _lib.check(call(), "pg_assoc_gxe_dev")
    ctx.sync()
    after = sent.download((nb,), np.uint8)
    assert (after[:56 * p] != 0xA5).any() and (after[64 * p:] == 0xA5).all()
    for b_ in (dd, dW, dy, dX, dXE, sent):
        b_.free()


def _frames_equal(a, b):
    assert list(a.columns) == list(b.columns)
    for col in a.columns:
        if col == "SNPs":
            assert list(a[col]) == list(b[col])
            continue
        assert a[col].dtype == b[col].dtype, col
        assert (bits(a[col].to_numpy()) == bits(b[col].to_numpy())).all(), col


def test_pipeline_batch_size_and_gpus(monkeypatch):
    from pygemma import lmm
    import pygemma_amd.lmm as impl
    from pygemma_amd import _lib
    Y, X, W, K, e = _raw(512, 3001, 3, "binary", False, seed=4)
    snps = [f"rs{i}" for i in range(3001)]
    a = lmm.pygemma_gxe(Y, X, W, K, e, snps=snps)
    assert list(a.columns) == ["beta", "se_beta", "tau", "lambda", "F_wald", "p_wald", "SNPs"]
    assert np.isfinite(a["p_wald"]).all()
    monkeypatch.setattr(impl, "_BATCH_SNPS", 512)
    b = lmm.pygemma_gxe(Y, X, W, K, e, snps=snps)
    _frames_equal(a, b)
    if _lib.device_count() >= 2:
        _frames_equal(a, lmm.pygemma_gxe(Y, X, W, K, e, snps=snps, nproc=2))


def test_nproc2_equals_nproc1():
    from pygemma import lmm
    from pygemma_amd import _lib
    if _lib.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    Y, X, W, K, e = _raw(400, 2001, 2, "continuous", False, seed=6)
    _frames_equal(lmm.pygemma_gxe(Y, X, W, K, e, nproc=1), lmm.pygemma_gxe(Y, X, W, K, e, nproc=2))


def test_checkpoint_restart(tmp_path, monkeypatch):
    """Finished batches land under `checkpoint`; a rerun restores them and recomputes only what is missing; a Wald run's directory
    is refused for an interaction run and the other way round."""
    import os
    from pygemma_amd import lmm
    monkeypatch.setattr(lmm, "_BATCH_SNPS", 512)
    Y, X, W, K, e = _raw(200, 1500, 2, "binary", False, seed=4)
    ck = str(tmp_path / "ck")
    ref = lmm.pygemma_gxe(Y, X, W, K, e)
    a = lmm.pygemma_gxe(Y, X, W, K, e, checkpoint=ck)
    parts = sorted(f for f in os.listdir(ck) if f.startswith("part_"))
    assert len(parts) == 3
    os.remove(os.path.join(ck, parts[1]))
    z = dict(np.load(os.path.join(ck, parts[0])))
    z["beta"] = z["beta"] + 1.0
    np.savez(os.path.join(ck, parts[0]), **z)
    b = lmm.pygemma_gxe(Y, X, W, K, e, checkpoint=ck)
    for col in ("se_beta", "tau", "lambda", "F_wald", "p_wald"):
        assert (a[col].to_numpy() == ref[col].to_numpy()).all() and (b[col].to_numpy() == ref[col].to_numpy()).all()
    assert (a["beta"].to_numpy() == ref["beta"].to_numpy()).all()
    assert (b["beta"].to_numpy()[:512] == ref["beta"].to_numpy()[:512] + 1.0).all()
    assert (b["beta"].to_numpy()[512:] == ref["beta"].to_numpy()[512:]).all()
    with pytest.raises(ValueError, match="manifest"):                  # another environment
        lmm.pygemma_gxe(Y, X, W, K, e[::-1].copy(), checkpoint=ck)
    with pytest.raises(ValueError, match="manifest"):                  # a Wald run in an interaction run's directory
        lmm.pygemma(Y, X, np.c_[W, e], K, checkpoint=ck)
    ckw = str(tmp_path / "ckw")
    lmm.pygemma(Y, X, np.c_[W, e], K, checkpoint=ckw)
    with pytest.raises(ValueError, match="manifest"):                  # ... and the other way round
        lmm.pygemma_gxe(Y, X, W, K, e, checkpoint=ckw)


# ---- end to end against fp64 truth --------------------------------------------------------------------------------------------
def _reml_fp64(d, Wp, yr, Xr, XEr):
    """fp64 REML Wald test of XEr[:, j] in y ~ [Wp, Xr[:, j], XEr[:, j]] for every SNP, with the kernels' lambda-selection rule:
    the boundaries 1e-5, 1e5 and, in every decade whose end points' dlogL/dlambda differ in sign, the root (bisection in log lambda
    to full precision), the candidate with the largest restricted log-likelihood winning.  Returns beta, p."""
    from scipy import special
    n, cw = Wp.shape
    p = Xr.shape[1]
    m = cw + 2
    nu = n - m
    Xt, XEt = Xr.T, XEr.T                                   # (p, n)
    WW = (Wp[:, :, None] * Wp[:, None, :]).reshape(n, cw * cw)
    Wy, yy = Wp * yr[:, None], yr * yr

    def grams(h):
        """V'HV (p, m, m), V'Hy (p, m), y'Hy (p,) with V = [Wp, x, xe] and H = diag(h), h (p, n)."""
        A = np.empty((p, m, m))
        A[:, :cw, :cw] = (h @ WW).reshape(p, cw, cw)
        hx, hxe = h * Xt, h * XEt
        A[:, cw, :cw] = A[:, :cw, cw] = hx @ Wp
        A[:, cw + 1, :cw] = A[:, :cw, cw + 1] = hxe @ Wp
        A[:, cw, cw] = (hx * Xt).sum(1)
        A[:, cw, cw + 1] = A[:, cw + 1, cw] = (hx * XEt).sum(1)
        A[:, cw + 1, cw + 1] = (hxe * XEt).sum(1)
        b = np.concatenate([h @ Wy, (hx @ yr)[:, None], (hxe @ yr)[:, None]], axis=1)
        return A, b, h @ yy

    def forms(lam):
        """lam (p,) -> logL (up to a constant), dlogL/dlambda, beta, se per SNP."""
        h = 1.0 / (lam[:, None] * d[None, :] + 1.0)
        A, b, yHy = grams(h)
        A2, b2, yH2y = grams(h * h)
        coef = np.linalg.solve(A, b[:, :, None])[:, :, 0]
        yPy = yHy - (b * coef).sum(1)
        yPPy = yH2y - 2.0 * (coef * b2).sum(1) + np.einsum("pk,pkl,pl->p", coef, A2, coef)
        Ainv = np.linalg.inv(A)
        trP = h.sum(1) - np.einsum("pkl,plk->p", Ainv, A2)
        ldA = np.linalg.slogdet(A)[1]
        logL = -0.5 * np.log(lam[:, None] * d[None, :] + 1.0).sum(1) - 0.5 * ldA - 0.5 * nu * np.log(yPy)
        d1 = -0.5 * (nu - trP) / lam + 0.5 * nu * (yPy - yPPy) / lam / yPy
        return logL, d1, coef[:, -1], np.sqrt(yPy / nu * Ainv[:, -1, -1])

    lams = 10.0 ** np.arange(-5, 6)
    scan = [forms(np.full(p, l)) for l in lams]
    best_l, best_b, best_se = scan[0][0].copy(), scan[0][2].copy(), scan[0][3].copy()
    hi = scan[-1][0] > best_l
    best_l[hi], best_b[hi], best_se[hi] = scan[-1][0][hi], scan[-1][2][hi], scan[-1][3][hi]
    for k in range(10):
        f0, f1 = scan[k][1], scan[k + 1][1]
        br = np.signbit(f0) != np.signbit(f1)
        if not br.any():
            continue
        lo, up = np.full(p, np.log(lams[k])), np.full(p, np.log(lams[k + 1]))
        for _ in range(40):
            mid = 0.5 * (lo + up)
            same = np.signbit(forms(np.exp(mid))[1]) == np.signbit(f0)
            lo, up = np.where(same, mid, lo), np.where(same, up, mid)
        lg, _, b, se = forms(np.exp(0.5 * (lo + up)))
        take = br & (lg > best_l)
        best_l[take], best_b[take], best_se[take] = lg[take], b[take], se[take]
    F = (best_b / best_se) ** 2
    return best_b, special.betainc(0.5 * nu, 0.5, nu / (nu + F))


def _within(a, b, tol, frac=0.99):
    rel = np.abs(np.asarray(a, np.float64) - b) / np.abs(b)
    return np.mean(rel <= tol) >= frac, float(np.quantile(rel, frac))


@pytest.mark.parametrize("c,e_kind", [(1, "binary"), (5, "continuous")])
def test_pipeline_against_fp64_truth(c, e_kind):
    from pygemma import lmm
    n, p = 2000, 2000
    Y, X, W, K, e = _raw(n, p, c, e_kind, False, seed=30 + c)
    dK, U = np.linalg.eigh(K.astype(np.float64))
    dK = np.maximum(dK, 0.0)
    R = lambda A: U.T @ np.asarray(A, np.float64)
    X64 = X.astype(np.float64)
    b_t, p_t = _reml_fp64(dK, R(np.c_[W, e]), R(Y).reshape(-1), R(X64), R(X64 * e.astype(np.float64)[:, None]))
    runs = {"K": lmm.pygemma_gxe(Y, X, W, K, e)}
    if c == 1 and e_kind == "binary":
        runs["eigenpairs"] = lmm.pygemma_gxe(Y, X, W, None, e, eigenpairs=(dK, U))
    if c == 5 and e_kind == "continuous":
        runs["Z"] = lmm.pygemma_gxe(Y, X, W, K, e, Z=np.eye(n, dtype=np.float32))
        _frames_equal(runs["K"], runs["Z"])
    for tag, df in runs.items():
        okp, qp = _within(df["p_wald"].to_numpy(), p_t, 1e-3)
        okb, qb = _within(df["beta"].to_numpy(), b_t, 1e-3)
        print(f"fp64 truth c={c} {e_kind} {tag}: 99th percentile rel err p {qp:.2e}, beta {qb:.2e}")
        assert okp and okb, (tag, qp, qb)


def test_calibration_null_and_planted():
    from pygemma import lmm
    n, p = 2000, 20000
    Y, X, W, K, e = _raw(n, p, 3, "continuous", True, seed=77)
    df = lmm.pygemma_gxe(Y, X, W, K, e)
    lam_gc = float(np.median(df["F_wald"].to_numpy()) / 0.4549364231195724)
    print(f"lambda_GC under no interaction: {lam_gc:.3f}")
    assert 0.9 <= lam_gc <= 1.1
    planted = (11, 5000, 17000)
    y = Y.reshape(-1).astype(np.float64)
    for j in planted:
        y += 0.35 * X[:, j] * e
    df = lmm.pygemma_gxe(y.astype(np.float32).reshape(-1, 1), X, W, K, e)
    rank = np.argsort(np.argsort(df["p_wald"].to_numpy()))
    assert (rank[list(planted)] < p // 100).all(), rank[list(planted)]


def test_pipeline_x_kinds_agree_where_wald_does(tmp_path):
    from pygemma import lmm
    from pygemma_amd import synth
    from pygemma_amd.bed import PackedBed, write_bed
    n, p, c = 384, 600, 3
    raw = synth.exact_panel(n, p, c, seed=3)
    rng = np.random.default_rng(3)
    W = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, c - 1))], axis=1).astype(np.float32)
    G = raw["X"]
    e = rng.standard_normal(n).astype(np.float32)
    y = (G[:, :20] @ rng.standard_normal(20) + 0.5 * G[:, 3] * e + rng.standard_normal(n)).reshape(-1, 1)
    Gm = G.astype(np.float64).copy()
    Gm[rng.random(Gm.shape) < 0.01] = np.nan                           # missing calls in the .bed image
    write_bed(str(tmp_path / "toy"), G.astype(np.float64))
    write_bed(str(tmp_path / "miss"), Gm)
    K = raw["K"]
    kinds = {"f32": G, "f32_snp_major": np.asfortranarray(G), "f64": G.astype(np.float64), "i8": G.astype(np.int8),
             "u8": G.astype(np.uint8), "bed": PackedBed.open(str(tmp_path / "toy"))}
    We = np.c_[W, e]
    wald = {k: lmm.pygemma(y, X, We, K) for k, X in kinds.items()}
    gxe = {k: lmm.pygemma_gxe(y, X, W, K, e) for k, X in kinds.items()}
    names = list(kinds)
    pairs = 0
    for i, a in enumerate(names):
        assert np.isfinite(gxe[a]["F_wald"]).all(), a
        for b in names[i + 1:]:
            if all((bits(wald[a][col].to_numpy()) == bits(wald[b][col].to_numpy())).all() for col in wald[a].columns):
                _frames_equal(gxe[a], gxe[b])
                pairs += 1
            else:         # otherwise within the rotation's error class
                np.testing.assert_allclose(gxe[a]["F_wald"].to_numpy(), gxe[b]["F_wald"].to_numpy(), rtol=1e-3, atol=1e-4)
    assert pairs >= 1
    # missing calls: imputed before e is applied, as in host X o e of the imputed matrix
    bed = PackedBed.open(str(tmp_path / "miss"))
    Gi = bed.to_float(impute=True)
    a = lmm.pygemma_gxe(y, bed, W, K, e)
    b = lmm.pygemma_gxe(y, np.ascontiguousarray(Gi, np.float32), W, K, e)
    np.testing.assert_allclose(a["F_wald"].to_numpy(), b["F_wald"].to_numpy(), rtol=1e-3, atol=1e-4)


def test_float64_block_off_the_genotype_path_matches_float32():
    """A float64 block that fails the genotype check is cast to float32 once and both rotations (U and diag(e) U) read that image:
    the frame equals the one of the float32 matrix, NaN rows included."""
    from pygemma import lmm
    rng = np.random.default_rng(21)
    n, p = 257, 600
    Y, _X, W, K, e = _raw(n, p, 2, "continuous", False, seed=12)
    G2 = rng.integers(0, 6, size=(n, p)) + rng.uniform(-0.3, 0.3, (n, p))    # dosages with more digits than float32 holds
    G2[7, 3] = np.nan
    a = lmm.pygemma_gxe(Y, G2, W, K, e)
    b = lmm.pygemma_gxe(Y, G2.astype(np.float32), W, K, e)
    for col in ("beta", "se_beta", "tau", "lambda", "F_wald", "p_wald"):
        x, z = a[col].to_numpy(), b[col].to_numpy()
        assert ((x == z) | (np.isnan(x) & np.isnan(z))).all(), col
    assert np.isnan(a["beta"].to_numpy()).sum() >= 1 and np.isfinite(a["beta"].to_numpy()).mean() > 0.9
