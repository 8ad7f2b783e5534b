"""The detect pass in front of the genotype rotation: one read of X (detect_encode_kernel: extremes, codes and flags from 2-bit tags held in
LDS) against the two passes it replaces (PG_GENO_ONEPASS=0: minmax_geno_kernel + encode_geno_kernel).  Every public rotation entry point
must give the same bits and the same path code either way, on the value patterns that steer the detect pass: one / two / three values, raw
and standardised, -0.0 beside +0.0, a midpoint in two bit patterns (a fifth pattern: the dictionary overflows and encode_geno_kernel runs,
predicated), one imputed value, two of them, dosages, NaN / Inf — for float32, int8 / uint8 and float64 X, at n that is no multiple of 4, 64
or 128 and p = 70 (two whole 32-column strips and a ragged one), and at the first n that no longer fits the LDS."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 70
SHAPES = [257, 130]


@pytest.fixture(scope="module")
def ctx():
    from pygemma_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


_prepared = {}


def _basis(ctx, n):
    """(U float32 orthogonal, device U, prepared planes) of size n: made once and left unchanged"""
    from pygemma_amd import _lib
    if n not in _prepared:
        L = _lib.load()
        U = np.linalg.qr(np.random.default_rng(n).standard_normal((n, n)))[0].astype(np.float32)
        dU, dprep = ctx.to_device(U), ctx.alloc(L.pg_geno_prep_bytes(n))
        _lib.check(L.pg_geno_prep_dev(ctx.handle, n, dU.ptr, n, dprep.ptr), "pg_geno_prep_dev")
        _prepared[n] = (U, dU, dprep)
    return _prepared[n]


def _rotate(ctx, n, X, entry, dU, dprep):
    """one public entry point on X (n, p) of dtype float32 / float64 / int8 / uint8 -> (Xr (p, ldx) or None, path code)"""
    from pygemma_amd import _lib
    L = _lib.load()
    p = X.shape[1]
    ldx = (n + 127) // 128 * 128
    X = np.ascontiguousarray(X)
    dX, dwork = ctx.to_device(X), ctx.alloc(L.pg_geno_work_bytes(n, p))
    dXr, dpath = ctx.alloc(p * ldx * 4), ctx.alloc(4)
    dXr.upload(np.full((p, ldx), -77.0, np.float32))
    ok, h = C.c_int(-1), ctx.handle
    small = X.dtype in (np.int8, np.uint8)
    if entry == "auto" and X.dtype == np.float32:
        _lib.check(L.pg_rotate_auto_dev(h, n, p, dU.ptr, n, dprep.ptr, dX.ptr, p, dXr.ptr, ldx, dwork.ptr, dpath.ptr), entry)
    elif entry == "auto" and small:
        _lib.check(L.pg_rotate_auto_i8_dev(h, n, p, dprep.ptr, dX.ptr, int(X.dtype == np.uint8), p, dXr.ptr, ldx, dwork.ptr, dpath.ptr), entry)
    elif entry == "geno" and X.dtype == np.float32:
        _lib.check(L.pg_rotate_geno_dev(h, n, p, dprep.ptr, dX.ptr, p, dXr.ptr, ldx, dwork.ptr, C.byref(ok)), entry)
    elif entry == "geno" and small:
        _lib.check(L.pg_rotate_geno_i8_dev(h, n, p, dprep.ptr, dX.ptr, int(X.dtype == np.uint8), p, dXr.ptr, ldx, dwork.ptr, C.byref(ok)), entry)
    elif entry == "geno" and X.dtype == np.float64:
        _lib.check(L.pg_rotate_geno_f64_dev(h, n, p, dprep.ptr, dX.ptr, p, dXr.ptr, ldx, dwork.ptr, C.byref(ok)), entry)
    else:
        raise AssertionError((entry, X.dtype))
    ctx.sync()
    path = int(dpath.download((1,), np.int32)[0]) if entry == "auto" else int(ok.value)
    out = dXr.download((p, ldx), np.float32) if (entry == "auto" or path) else None
    for b in (dX, dwork, dXr, dpath):
        b.free()
    return out, path


def _both(ctx, monkeypatch, n, X, entry, basis=None):
    """the entry point with the default detect pass and with PG_GENO_ONEPASS=0: bit-equal Xr (NaN where NaN), equal path code"""
    U, dU, dprep = basis or _basis(ctx, n)
    monkeypatch.delenv("PG_GENO_ONEPASS", raising=False)
    one, path1 = _rotate(ctx, n, X, entry, dU, dprep)
    monkeypatch.setenv("PG_GENO_ONEPASS", "0")
    two, path2 = _rotate(ctx, n, X, entry, dU, dprep)
    monkeypatch.delenv("PG_GENO_ONEPASS", raising=False)
    assert path1 == path2
    assert (one is None) == (two is None)
    if one is not None:
        assert (one.view(np.uint32) == two.view(np.uint32)).all(), np.nanmax(np.abs(one - two))
    return one, path1


def _within_fp64(n, U, X, got):
    """the bound tests/test_gpu_rotate.py holds the int8 genotype kernel to: 4 * 2^-24 sqrt(n) sum_i |x_i||u_ik| against the fp64 rotation"""
    X64, U64 = X.astype(np.float32).astype(np.float64), U.astype(np.float64)
    exact, bound = (U64.T @ X64).T, np.abs(X64).T @ np.abs(U64)
    err = np.abs(got[:, :n] - exact)
    print("max error / bound:", float((err / np.maximum(bound, 1e-300)).max()), "allowed", 4 * 2.0 ** -24 * np.sqrt(n))
    assert (err <= 4 * 2.0 ** -24 * np.sqrt(n) * bound).all()
    assert (got[:, n:] == 0).all()


KINDS = ["one", "two", "raw", "std", "zeros", "mid2", "imputed"]


def _column(rng, n, kind):
    g = rng.binomial(2, rng.uniform(0.2, 0.5), size=n).astype(np.float32)
    g[:3] = [0, 1, 2]                                     # every column really holds its three values
    if kind == "one":
        return np.full(n, np.float32(1.25))
    if kind == "two":
        return np.where(g == 1, np.float32(2), g)
    if kind == "raw":
        return g
    if kind == "std":
        return ((g - g.mean(dtype=np.float64)) / g.std(dtype=np.float64)).astype(np.float32)
    if kind == "zeros":                                    # lowest value 0 in both signs: equal by value, two bit patterns
        z = g.copy(); z[(g == 0) & (rng.random(n) < 0.5)] = np.float32(-0.0); z[0] = np.float32(-0.0); z[3] = 0.0
        return z
    if kind == "mid2":                                     # the midpoint 1 ulp apart, lo, hi and an imputed value: five patterns
        m = g.copy(); m[(g == 1) & (rng.random(n) < 0.5)] = np.nextafter(np.float32(1), np.float32(2)); m[1] = 1.0
        m[4] = np.nextafter(np.float32(1), np.float32(2)); m[5] = m[9] = np.float32(0.8125)
        return m
    assert kind == "imputed"
    m = g.copy(); m[rng.random(n) < 0.05] = np.float32(0.7310585); m[6] = np.float32(0.7310585)
    return m


def _block(n, kinds, seed=0):
    rng = np.random.default_rng(1000 * n + seed)
    return np.stack([_column(rng, n, kinds[j % len(kinds)]) for j in range(P)], axis=1).astype(np.float32)


@pytest.fixture(scope="module")
def mixed():
    return {n: _block(n, KINDS) for n in SHAPES}


@pytest.mark.parametrize("codes", ["i8", "f16"])
@pytest.mark.parametrize("entry", ["auto", "geno"])
@pytest.mark.parametrize("n", SHAPES)
def test_mixed_genotype_block_float32(n, entry, codes, mixed, ctx, monkeypatch):
    """every kind of genotype column in one block, some with an imputed value: flag[1] set, the indicator pass runs; with the codes
    written as int8 (the int8 GEMM's operand) and as fp16 (PG_GENO_I8=0)"""
    monkeypatch.setenv("PG_GENO_I8", "1" if codes == "i8" else "0")
    X = mixed[n]
    assert np.signbit(X[:, 4]).any() and (X[:, 4] == 0).sum() > np.signbit(X[:, 4]).sum()
    assert len(np.unique(X[:, 5].view(np.uint32))) == 5
    got, path = _both(ctx, monkeypatch, n, X, entry)
    assert path == 1
    _within_fp64(n, _basis(ctx, n)[0], X, got)


@pytest.mark.parametrize("entry", ["auto", "geno"])
@pytest.mark.parametrize("n", SHAPES)
def test_plain_genotype_block_float32(n, entry, ctx, monkeypatch):
    """no imputed value anywhere: flag[1] stays clear, the indicator pass is predicated off"""
    X = _block(n, ["one", "two", "raw", "std", "zeros"], seed=1)
    got, path = _both(ctx, monkeypatch, n, X, entry)
    assert path == 1
    _within_fp64(n, _basis(ctx, n)[0], X, got)


@pytest.mark.parametrize("n", SHAPES)
def test_mixed_genotype_block_float64(n, mixed, ctx, monkeypatch):
    """float64 X: the kernels round each element to float32 as they read it; a column standardised in float64 is no float32 value"""
    X = mixed[n].astype(np.float64)
    g = X[:, 2]
    X[:, 3] = (g - g.mean()) / g.std()
    assert (X[:, 3] != X[:, 3].astype(np.float32)).any()
    got, path = _both(ctx, monkeypatch, n, X, "geno")
    assert path == 1
    _within_fp64(n, _basis(ctx, n)[0], X, got)


def _int_block(n, dtype, seed):
    rng = np.random.default_rng(n + seed)
    cols = []
    for j in range(P):
        g = rng.binomial(2, 0.4, size=n); g[:3] = [0, 1, 2]
        k = j % 4
        if k == 0:
            g[:] = 2
        elif k == 1:
            g[g == 1] = 0
        elif k == 3:                                       # codes two apart (-2/0/2 or 0/2/4) and one other value between them
            g = 2 * g - (2 if dtype == np.int8 else 0)
            g[rng.random(n) < 0.05] = 1
            g[7] = 1
        cols.append(g)
    return np.stack(cols, axis=1).astype(dtype)


@pytest.mark.parametrize("entry", ["auto", "geno"])
@pytest.mark.parametrize("dtype", [np.int8, np.uint8])
@pytest.mark.parametrize("n", SHAPES)
def test_genotype_block_int8(n, dtype, entry, ctx, monkeypatch):
    X = _int_block(n, dtype, 3)
    got, path = _both(ctx, monkeypatch, n, X, entry)
    assert path == 1
    _within_fp64(n, _basis(ctx, n)[0], X, got)
    Y = X.copy(); Y[11, 3] = 5; Y[12, 3] = 7                # two other values in one column: no genotype block
    _, path = _both(ctx, monkeypatch, n, Y, entry)
    assert path == 2
    D = np.random.default_rng(n).integers(0, 100, (n, P)).astype(dtype)      # dosages in percent
    _, path = _both(ctx, monkeypatch, n, D, entry)
    assert path == 2


@pytest.mark.parametrize("entry", ["auto", "geno"])
@pytest.mark.parametrize("n", SHAPES)
def test_blocks_that_leave_the_genotype_path_float32(n, entry, mixed, ctx, monkeypatch):
    X = mixed[n].copy(); X[20, 6] = np.float32(0.25)        # a second other value in an imputed column
    _, path = _both(ctx, monkeypatch, n, X, entry)
    assert path == 2
    D = np.random.default_rng(n).uniform(0, 2, (n, P)).astype(np.float32)
    D[:, 1] = mixed[n][:, 2]                                # dosages, one hard-call column among them
    _, path = _both(ctx, monkeypatch, n, D, entry)
    assert path == 2
    for v in (np.nan, np.inf, -np.inf):
        X = mixed[n].copy(); X[n - 1, 69] = v
        got, path = _both(ctx, monkeypatch, n, X, entry)
        assert path == 0
        if entry == "auto":                                 # the fp32 kernel's propagation: SNP 69 non-finite, its neighbour untouched
            assert not np.isfinite(got[69, :n]).any() and np.isfinite(got[68, :n]).all()


def test_first_n_past_the_lds_limit_takes_two_passes(ctx, monkeypatch):
    """n one above what the device's LDS holds (from its reported per-workgroup size), p = 40: the host must choose the two-pass detect,
    and the result is the forced two-pass one.  U is a random row block repeated down the matrix: the comparison needs no orthogonality."""
    from pygemma_amd import _lib
    L = _lib.load()
    limit = int(L.pg_geno_onepass_limit(ctx.handle))
    assert limit >= 512 and limit % 512 == 0
    n, p = limit + 1, 40
    assert int(L.pg_geno_onepass_max_n(4 * ((n + 511) // 512 * 1056 + 256))) >= n > limit      # n needs one more layer than the device has
    rows = 256
    blk = np.random.default_rng(5).standard_normal((rows, n)).astype(np.float32) / np.float32(np.sqrt(n))
    dU, dprep = ctx.alloc(n * n * 4), ctx.alloc(L.pg_geno_prep_bytes(n))
    for r0 in range(0, n, rows):
        r = min(rows, n - r0)
        _lib.check(L.pg_memcpy_h2d(ctx.handle, dU.ptr + r0 * n * 4, blk.ctypes.data, r * n * 4), "pg_memcpy_h2d")
    _lib.check(L.pg_geno_prep_dev(ctx.handle, n, dU.ptr, n, dprep.ptr), "pg_geno_prep_dev")
    rng = np.random.default_rng(6)
    X = np.stack([_column(rng, n, KINDS[j % len(KINDS)]) for j in range(p)], axis=1).astype(np.float32)
    got, path = _both(ctx, monkeypatch, n, X, "auto", basis=(None, dU, dprep))
    assert path == 1 and np.isfinite(got[:, :n]).all() and (got[:, n:] == 0).all()
    # and the largest n that does fit (the leading n - 1 rows and columns of the same U): the one-pass kernel at the whole of the LDS
    dprep1 = ctx.alloc(L.pg_geno_prep_bytes(limit))
    _lib.check(L.pg_geno_prep_dev(ctx.handle, limit, dU.ptr, n, dprep1.ptr), "pg_geno_prep_dev")
    got1, path1 = _both(ctx, monkeypatch, limit, X[:limit], "geno", basis=(None, dU, dprep1))
    assert path1 == 1 and np.isfinite(got1[:, :limit]).all()
    for b in (dU, dprep, dprep1):
        b.free()


def test_dictionary_order_is_a_race_the_outputs_are_not(mixed, ctx, monkeypatch):
    """slots of a column's dictionary fill in first-come order; ten runs of the mixed block must give the same bits"""
    n = 257
    U, dU, dprep = _basis(ctx, n)
    monkeypatch.delenv("PG_GENO_ONEPASS", raising=False)
    first, path = _rotate(ctx, n, mixed[n], "auto", dU, dprep)
    assert path == 1
    for _ in range(9):
        again, path = _rotate(ctx, n, mixed[n], "auto", dU, dprep)
        assert path == 1 and (again.view(np.uint32) == first.view(np.uint32)).all()
