"""GPU checks of the variance-component kernels and of lmm.reml / lmm.vc_kinship (csrc/vc.hip) — run with -m gpu on an MI355X.

The truth is tests/_vc_truth.py.  U = 2^-53.  Every matrix the device writes is the LOWER triangle of a window of pitch n + 5, three
elements into a buffer of 0x7f bytes (so the window is 8-byte, not 16-byte aligned); every byte outside the triangle — the strict upper
triangle, the pad of every row, the head and the tail — must come back as it was.  Panels and scalars lie in windows of the same kind.
Matrices: K_i = Z_i Z_i' / p_i from synth genotypes scaled to trace n, float32 and float64 mixed within a call; V = sum s_i K_i + s_e I
with s_e at least a quarter of the sum, kappa_2 by eigvalsh.  n covers both sides of the 64 and 128 block edges, more than two panels
and one size off every alignment.
  potrf    max |A - L L'| <= (n + 8) U kappa_2(A) max |A|   (kappa_2: panels are formed with the inverted diagonal block)
           info: LAPACK's on an indefinite A whose first bad pivot is at 0, in the middle of a panel, in the last partial block
  log det  within (n + 8) U sum |log L_jj| of 2 sum log L_jj (fsum over the device's own factor)
  potri    max |A A^-1 - I| <= 8 (n + 8) U kappa_2(A)
  trdot    |t - truth| <= (n^2 + 8) U sum |a||b|;   symv  |y_i - truth| <= (n + 8) U sum_j |a_ij||x_j|  — fp64 sums in any order;
           integer entries below 2^10: NumPy's bits; two runs: the same bits
  combine  NumPy's bits (the same products and additions in the same order, no fused multiply-add)
  eval     logL, score_i, AI_ij within 64 n U kappa_2(V) mag of the truth (mag: the sum of the magnitudes of the terms); beta within
           d beta (below) and P y within 64 n U kappa (|V^-1||y| + |V^-1||W||beta|) + |V^-1||W| d beta
  reml     converged; the TRUTH's AI step at the device's estimate <= 2 tol sum sigma per component; se, h2, h2_se and beta against the
           truth at that estimate within the eval bound propagated:  d cov <= |cov| E |cov| with E_ij = 64 n U kappa mag_ai_ij,
           d se_i = d cov_ii / (2 se_i), d h2_se_i = |g|' d cov |g| / (2 h2_se_i), h2 to 4 U (the same sigma, another order), and
           d beta <= |H| (|W|'|V^-1||y| + |W|'|V^-1||W||beta|) 64 n U kappa
With PG_VC_FRACTIONS=<path> the largest fraction of each bound that was used is written there as JSON (tools/bench_vc.py reads it)."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import _vc_truth as T

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 257, 600]
FRACTIONS = {}


def within(name, err, bound):
    err, bound = np.abs(np.asarray(err, np.float64)), np.asarray(bound, np.float64)
    assert np.isfinite(err).all(), f"{name}: not finite"
    frac = float(np.max(np.where(err > 0, err / np.where(bound > 0, bound, 1e-300), 0.0)))
    FRACTIONS[name] = max(FRACTIONS.get(name, 0.0), frac)
    print(f"{name}: {frac:.3g} of the bound")
    assert frac <= 1.0, f"{name}: error is {frac:.3g} of the bound"


@pytest.fixture(scope="module")
def ctx():
    from pygemma_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()
    path = os.environ.get("PG_VC_FRACTIONS")
    if path:
        with open(path, "w") as f:
            json.dump(FRACTIONS, f, indent=1, sort_keys=True)


class Both:
    """The functions of the variance-component library, then those of the main one (pg_memset)."""

    def __getattr__(self, name):
        from pygemma_amd import _lib
        V = _lib.load_vc()
        return getattr(V, name) if name in _lib.VC_SYMBOLS else getattr(_lib.load(), name)


def lib():
    from pygemma_amd import _lib
    return _lib, Both()


class Tri:
    """The lower triangle of an n x n matrix of `dtype` in a window of pitch n + 5, three elements into a buffer of 0x7f bytes; `lower`
    (n, n): its starting values (None: 0x7f as well — the call has to write all of it)."""

    def __init__(self, ctx, n, lower=None, dtype=np.float64):
        self.n, self.ld, self.dtype = n, n + 5, np.dtype(dtype)
        size = 3 + n * self.ld + 4
        self.mask = np.zeros(size, bool)
        for i in range(n):
            self.mask[3 + i * self.ld:3 + i * self.ld + i + 1] = True
        host = np.full(size * self.dtype.itemsize, 0x7f, np.uint8)
        if lower is not None:
            host.view(self.dtype)[self.mask] = np.asarray(lower)[np.tril_indices(n)]
        self.before = host.reshape(size, self.dtype.itemsize).copy()
        self.buf = ctx.to_device(host)
        self.ptr = self.buf.ptr + 3 * self.dtype.itemsize

    def take(self):
        """The lower triangle as an (n, n) float64 matrix with zeros above it; asserts every byte outside it and frees the buffer."""
        full = self.buf.download((self.mask.size, self.dtype.itemsize), np.uint8)
        self.buf.free()
        assert (full[~self.mask] == self.before[~self.mask]).all(), "bytes outside the lower triangle were written"
        M = np.zeros((self.n, self.n))
        M[np.tril_indices(self.n)] = full.reshape(-1).view(self.dtype)[self.mask]
        return M


class Panel:
    """`rows` windows of `width` doubles at pitch width + 5, three doubles into a buffer of 0x7f bytes, holding `fill` (None: 0x7f)."""

    def __init__(self, ctx, rows, width, fill=None):
        self.rows, self.width, self.ld = rows, width, width + 5
        size = 3 + rows * self.ld + 4
        self.inside = np.zeros(size, bool)
        for k in range(rows):
            self.inside[3 + k * self.ld:3 + k * self.ld + width] = True
        host = np.full(size * 8, 0x7f, np.uint8)
        if fill is not None:
            host.view(np.float64)[self.inside] = np.asarray(fill, np.float64).reshape(-1)
        self.buf = ctx.to_device(host)
        self.ptr = self.buf.ptr + 24

    def take(self):
        full = self.buf.download((self.inside.size,), np.uint64)
        self.buf.free()
        assert (full[~self.inside].view(np.uint8) == 0x7f).all(), "bytes outside the windows were written"
        return full[self.inside].view(np.float64).reshape(self.rows, self.width)


def spd(n, seed=0, k=2):
    """(A, kappa_2): V = sum s_i K_i + s_e I with s_e a quarter of the sum."""
    Ks = T.kin_matrices(n, k, seed)
    A = T.v_of(Ks, np.r_[np.full(k, 0.75 / k), 0.25] * 1.7)
    w = np.linalg.eigvalsh(A)
    return A, w[-1] / w[0]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def mats_args(ctx, Ks):
    """The K's in Tri windows and the host arrays the entry points take -> (windows, (ptrs, f64, ldk))."""
    wins = [Tri(ctx, K.shape[0], K, K.dtype) for K in Ks]
    k = len(Ks)
    return wins, ((C.c_void_p * k)(*[w.ptr for w in wins]), (C.c_int * k)(*[int(K.dtype == np.float64) for K in Ks]), (C.c_int64 * k)(*[w.ld for w in wins]))


# ---- potrf, log det, potri ----------------------------------------------------------------------------------------------------------------

def run_potrf(ctx, A):
    _lib, L = lib()
    n = A.shape[0]
    win, info = Tri(ctx, n, A), ctx.to_device(np.full(2, 0x7f7f7f7f, np.int32))
    _lib.check(L.pg_potrf_dev(ctx.handle, n, win.ptr, win.ld, info.ptr), "pg_potrf_dev")
    ctx.sync()
    iv = info.download((2,), np.int32)
    info.free()
    assert iv[1] == 0x7f7f7f7f
    return win, int(iv[0])


@pytest.mark.parametrize("n", SIZES)
def test_potrf_and_logdet(ctx, n):
    _lib, L = lib()
    A, kap = spd(n, seed=n)
    win, info = run_potrf(ctx, A)
    out = Panel(ctx, 1, 1)
    _lib.check(L.pg_potrf_logdet_dev(ctx.handle, n, win.ptr, win.ld, out.ptr), "pg_potrf_logdet_dev")
    ctx.sync()
    ld = out.take()[0, 0]
    Lf = win.take()
    assert info == 0
    within("potrf", np.max(np.abs(A - Lf @ Lf.T)), (n + 8) * U * kap * np.max(np.abs(A)))
    logs = np.log(np.diagonal(Lf))
    within("logdet", ld - 2 * math.fsum(logs), (n + 8) * U * np.sum(np.abs(logs)))


@pytest.mark.parametrize("bad", [0, 100, 197])
def test_potrf_info_agrees_with_lapack(ctx, bad):
    """n = 200: panels at 0, 64, 128 and a last block of 8.  A = M D M' with M unit lower triangular and D positive but for D[bad] < 0:
    the leading minors are positive up to `bad`.  The call returns normally and writes nothing outside the triangle."""
    from scipy.linalg import lapack
    n = 200
    rng = np.random.default_rng(bad)
    M = np.tril(rng.standard_normal((n, n)) * 0.05, -1) + np.eye(n)
    d = rng.uniform(0.5, 2.0, n)
    d[bad] = -1.0
    A = M @ np.diag(d) @ M.T
    A = (A + A.T) / 2
    _, want = lapack.dpotrf(A, lower=1)
    assert want == bad + 1
    win, info = run_potrf(ctx, A)
    win.take()
    assert info == want


def test_potrf_refuses_a_nan_pivot(ctx):
    A, _ = spd(129, seed=4)
    A[70, 70] = np.nan
    win, info = run_potrf(ctx, A)
    win.take()
    assert info == 71


@pytest.mark.parametrize("n", SIZES)
def test_potri(ctx, n):
    _lib, L = lib()
    A, kap = spd(n, seed=100 + n)
    Lf = np.linalg.cholesky(A)
    lwin, owin = Tri(ctx, n, Lf), Tri(ctx, n)
    work = ctx.alloc(max(int(L.pg_potri_work_bytes(n)), 256))
    _lib.check(L.pg_memset(ctx.handle, work.ptr, 0xff, work.nbytes), "pg_memset")
    _lib.check(L.pg_potri_dev(ctx.handle, n, lwin.ptr, lwin.ld, owin.ptr, owin.ld, work.ptr), "pg_potri_dev")
    ctx.sync()
    work.free()
    assert np.array_equal(lwin.take(), np.tril(Lf))
    Ai = T.sym(owin.take())
    within("potri", np.max(np.abs(A @ Ai - np.eye(n))), 8 * (n + 8) * U * kap)


# ---- trdot, symv, combine -------------------------------------------------------------------------------------------------------------------

def run_trdot(ctx, A, B):
    _lib, L = lib()
    n = A.shape[0]
    a, b, out = Tri(ctx, n, A), Tri(ctx, n, B, B.dtype), Panel(ctx, 1, 1)
    _lib.check(L.pg_sym_trdot_dev(ctx.handle, n, a.ptr, a.ld, b.ptr, int(B.dtype == np.float64), b.ld, out.ptr), "pg_sym_trdot_dev")
    ctx.sync()
    a.take(), b.take()
    return out.take()[0, 0]


@pytest.mark.parametrize("n", SIZES)
def test_trdot(ctx, n):
    rng = np.random.default_rng(n)
    A = T.sym(rng.standard_normal((n, n)))
    for dt in (np.float32, np.float64):
        B = T.sym(rng.standard_normal((n, n)).astype(dt)).astype(dt)
        B64 = B.astype(np.float64)
        terms = A * B64
        got = run_trdot(ctx, A, B)
        within("trdot", got - math.fsum(terms.reshape(-1)), (n * n + 8) * U * np.sum(np.abs(terms)))
        assert bits(run_trdot(ctx, A, B)) == bits(got), "two runs differ"
        # exact leg: integers below 2^10, every partial sum an integer below 2^53
        Ai = T.sym(rng.integers(-1023, 1024, (n, n)).astype(np.float64))
        Bi = T.sym(rng.integers(-1023, 1024, (n, n)).astype(dt)).astype(dt)
        assert bits(run_trdot(ctx, Ai, Bi)) == bits(np.sum(Ai * Bi.astype(np.float64)))


def run_symv(ctx, A, X):
    _lib, L = lib()
    n, m = X.shape
    a, x, y = Tri(ctx, n, A, A.dtype), Panel(ctx, n, m, X), Panel(ctx, n, m)
    _lib.check(L.pg_symv_dev(ctx.handle, n, a.ptr, int(A.dtype == np.float64), a.ld, m, x.ptr, x.ld, y.ptr, y.ld), "pg_symv_dev")
    ctx.sync()
    a.take()
    assert np.array_equal(bits(x.take()), bits(X))
    return y.take()


@pytest.mark.parametrize("n,m", list(zip(SIZES, [1, 5, 31, 32, 8, 9, 32, 1, 17, 31])))
def test_symv(ctx, n, m):
    rng = np.random.default_rng(1000 + n)
    X = rng.standard_normal((n, m))
    for dt in (np.float32, np.float64):
        A = T.sym(rng.standard_normal((n, n)).astype(dt)).astype(dt)
        A64 = A.astype(np.float64)
        got = run_symv(ctx, A, X)
        within("symv", got - A64 @ X, (n + 8) * U * (np.abs(A64) @ np.abs(X)))
        assert np.array_equal(bits(run_symv(ctx, A, X)), bits(got)), "two runs differ"
        Ai = T.sym(rng.integers(-1023, 1024, (n, n)).astype(dt)).astype(dt)
        Xi = rng.integers(-1023, 1024, (n, m)).astype(np.float64)
        assert np.array_equal(bits(run_symv(ctx, Ai, Xi)), bits(Ai.astype(np.float64) @ Xi))


@pytest.mark.parametrize("n", SIZES)
def test_combine_carries_numpys_bits(ctx, n):
    _lib, L = lib()
    Ks = T.kin_matrices(n, 3, seed=n, dtypes=[np.float32, np.float64, np.float32])
    s = np.array([0.3, 1.7, 0.01, 0.45])
    wins, args = mats_args(ctx, Ks)
    out = Tri(ctx, n)
    _lib.check(L.pg_vc_combine_dev(ctx.handle, n, 3, *args, (C.c_double * 4)(*s), out.ptr, out.ld), "pg_vc_combine_dev")
    ctx.sync()
    for w in wins:
        w.take()
    want = np.zeros((n, n))
    for si, K in zip(s, Ks):
        want = want + si * K.astype(np.float64)
    want = want + np.diag(np.full(n, s[3]))
    assert np.array_equal(bits(out.take()), bits(np.tril(want)))


# ---- one evaluation -------------------------------------------------------------------------------------------------------------------------

def run_eval(ctx, Ks, y, W, sigma, want_py=False):
    _lib, L = lib()
    n, c, k = len(y), W.shape[1], len(Ks)
    wins, args = mats_args(ctx, Ks)
    dWy = ctx.to_device(np.ascontiguousarray(np.c_[W, y]))
    work = ctx.alloc(int(L.pg_vc_work_bytes(n, k)))
    _lib.check(L.pg_memset(ctx.handle, work.ptr, 0xff, work.nbytes), "pg_memset")
    out, info = np.full(int(L.pg_vc_out_len(k, c)) + 1, 7.5), C.c_int(-1)
    py = Panel(ctx, 1, n)
    _lib.check(L.pg_vc_eval_dev(ctx.handle, n, k, c, *args, (C.c_double * (k + 1))(*sigma), dWy.ptr, work.ptr, out.ctypes.data, py.ptr, C.byref(info)),
               "pg_vc_eval_dev")
    for w in wins:
        w.take()
    work.free(), dWy.free()
    assert out[-1] == 7.5
    from pygemma_amd import vc
    pyv = py.take()[0] if info.value == 0 else (py.buf.free(), None)[1]
    return (vc._unpack(out, k, c) if info.value == 0 else None), info.value, pyv, out[:-1]


EVAL_CASES = [(2, 1, 1), (63, 2, 5), (64, 5, 30), (65, 1, 30), (127, 2, 1), (128, 5, 5), (129, 1, 5), (257, 5, 1), (600, 2, 30)]


@pytest.mark.parametrize("n,k,c", EVAL_CASES)
def test_eval(ctx, n, k, c):
    Ks = T.kin_matrices(n, k, seed=7 * n + k)
    sigma = np.r_[np.linspace(0.5, 1.0, k) * (0.7 / k), 0.3]
    y, W = T.phenotype(Ks, c, sigma, seed=n + c)
    sigma = sigma * np.linspace(1.2, 0.9, k + 1)            # not the generating values; s_e stays above a quarter of the sum
    assert sigma[-1] >= 0.25 * sigma.sum()
    want = T.evaluate(y, W, Ks, sigma)
    w = np.linalg.eigvalsh(T.v_of(Ks, sigma))
    unit = 64 * n * U * (w[-1] / w[0])
    ev, info, py, _ = run_eval(ctx, Ks, y, W, sigma)
    assert info == 0
    within("eval logL", ev["logl"] - want["logl"], unit * want["mag_logl"])
    within("eval score", ev["score"] - want["score"], unit * want["mag_score"])
    within("eval AI", ev["ai"] - want["ai"], unit * want["mag_ai"])
    assert np.array_equal(ev["ai"], ev["ai"].T)
    # beta and P y through the same perturbation of V^-1 (relative error 64 n U kappa, entry by entry): the bounds of the docstring
    Vi, H = np.abs(np.linalg.inv(T.v_of(Ks, sigma))), np.abs(want["xvx_inv"])
    dbeta = unit * (H @ (np.abs(W).T @ Vi @ np.abs(y) + np.abs(W).T @ Vi @ np.abs(W) @ np.abs(want["beta"])))
    within("eval beta", ev["beta"] - want["beta"], dbeta)
    within("eval Py", py - want["py"], unit * (Vi @ np.abs(y) + Vi @ np.abs(W) @ np.abs(want["beta"])) + Vi @ np.abs(W) @ dbeta)
    np.testing.assert_allclose(ev["score"], -0.5 * (ev["tr_pk"] - ev["ypkpy"]), rtol=1e-13, atol=0)


def test_eval_reports_an_indefinite_v(ctx):
    Ks = T.kin_matrices(129, 2, seed=5)
    y, W = T.phenotype(Ks, 3, np.array([0.3, 0.3, 0.4]), seed=6)
    ev, info, py, out = run_eval(ctx, Ks, y, W, np.array([0.5, -2.0, 0.1]))
    assert ev is None and 1 <= info <= 129 and np.isnan(out).all()
    V = T.v_of(Ks, np.array([0.5, -2.0, 0.1]))
    from scipy.linalg import lapack
    assert info == lapack.dpotrf(V, lower=1)[1]


# ---- lmm.reml, lmm.vc_kinship --------------------------------------------------------------------------------------------------------------------

# seeds at which the truth's own estimate lies inside the parameter space (five components of 0.13 each are two standard errors from 0)
@pytest.mark.parametrize("n,k,seed", [(257, 1, 258), (257, 2, 259), (257, 5, 2), (600, 1, 601), (600, 2, 602), (600, 5, 1)])
def test_reml_end_to_end(n, k, seed):
    from pygemma import lmm
    c, tol = 3, 1e-8
    Ks = T.kin_matrices(n, k, seed=seed)
    y, W = T.phenotype(Ks, c, np.r_[np.full(k, 0.65 / k), 0.35], seed=seed + 1)
    tsig, _, _, tconv, tcons = T.iterate(y, W, Ks, tol=tol)
    assert tconv and not tcons.any() and tsig.min() > 0.03, "the fixture must have an interior optimum"
    stats = {}
    res = lmm.reml(y, W, Ks if k > 1 else Ks[0], tol=tol, stats=stats)
    assert res.converged and not res.constrained.any() and res.iters >= 2 and stats["evaluations"] >= res.iters + 1
    s = res.sigma2
    want = T.evaluate(y, W, Ks, s)
    step = T.ai_step(want)
    print(f"n={n} k={k}: sigma2 {s}, {res.iters} iterations, the truth's next step {step}")
    np.testing.assert_allclose(s, tsig, rtol=0, atol=4 * tol * s.sum())
    within("reml stationary", step, np.full(k + 1, 2 * tol * s.sum()))
    # the summary against the truth at the same sigma
    V = T.v_of(Ks, s)
    w = np.linalg.eigvalsh(V)
    unit = 64 * n * U * (w[-1] / w[0])
    ts = T.summarize(s, want)
    dcov = np.abs(ts["cov"]) @ (unit * want["mag_ai"]) @ np.abs(ts["cov"])
    within("reml se", res.se - ts["se"], np.diagonal(dcov) / (2 * ts["se"]) + 4 * U * ts["se"])
    within("reml h2", res.h2 - ts["h2"], 4 * U * ts["h2"])
    S = s.sum()
    G = (np.eye(k + 1)[:k] * S - s[:k, None]) / S ** 2
    within("reml h2_se", res.h2_se - ts["h2_se"], np.einsum("ij,jl,il->i", np.abs(G), dcov, np.abs(G)) / (2 * ts["h2_se"]) + 4 * U * ts["h2_se"])
    Vi, H = np.abs(np.linalg.inv(V)), np.abs(want["xvx_inv"])
    within("reml beta", res.beta - want["beta"], unit * (H @ (np.abs(W).T @ Vi @ np.abs(y) + np.abs(W).T @ Vi @ np.abs(W) @ np.abs(want["beta"]))))
    within("reml logL", res.logl - want["logl"], unit * want["mag_logl"])
    assert abs(res.h2_total - s[:k].sum() / S) <= 4 * U and res.lrt == 2 * (res.logl - res.logl0) and res.lrt > 0
    assert len(res.frame()) == 2 * k + 8 + (k > 1)


def test_reml_with_a_collinear_component_says_so():
    from pygemma import lmm
    from pygemma_amd import _lib
    Ks = T.kin_matrices(257, 1, seed=3)
    y, W = T.phenotype(Ks, 2, np.array([0.6, 0.4]), seed=4)
    try:
        res = lmm.reml(y, W, [Ks[0], Ks[0].copy()], max_iter=20)
    except _lib.PgError:
        return
    assert not res.converged and np.isfinite(res.sigma2).all()


def test_reml_flags_a_zero_variance_component():
    """The fixture of tests/test_host_vc.py: y drawn without the second component, at a seed where the truth holds it at the floor."""
    from pygemma import lmm
    Ks = T.kin_matrices(200, 2, 52)
    y, W = T.phenotype(Ks, 2, np.array([0.6, 0.0, 0.4]), 53)
    ts, _, _, tconv, tcons = T.iterate(y, W, Ks)
    assert tconv and tcons[1] and not tcons[0] and not tcons[2]
    res = lmm.reml(y, W, Ks)
    assert res.converged and list(res.constrained) == [False, True, False]
    assert res.sigma2[1] == 1e-6 * np.var(y, ddof=1)
    np.testing.assert_allclose(res.sigma2, ts, rtol=0, atol=4e-8 * ts.sum())      # each within tol sum sigma of the optimum, and slack


@pytest.mark.parametrize("n", [1, 65, 257])
def test_vc_kinship_carries_numpys_bits(n):
    from pygemma import lmm
    rng = np.random.default_rng(n)
    Ks = [T.sym(rng.integers(-8, 9, (n, n)).astype(dt)).astype(dt) for dt in (np.float32, np.float64, np.float32)]
    res = lmm.RemlResult(sigma2=np.array([1.0, 2.0, 5.0, 123.0]))
    got = lmm.vc_kinship(Ks, res)
    want = (0.125 * Ks[0].astype(np.float64) + 0.25 * Ks[1] + 0.625 * Ks[2].astype(np.float64)).astype(np.float32)
    assert got.dtype == np.float32 and got.shape == (n, n)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
