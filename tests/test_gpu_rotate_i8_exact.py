"""The int8 digit-plane genotype rotation against its host model (tests/_rotate_i8_truth.py), BIT FOR BIT: rotate_geno_i8_kernel behind
pg_rotate_bed_dev, pg_rotate_geno{,_i8,_f64}_dev and pg_rotate_auto{,_i8}_dev, with the prepare step (pg_geno_prep_dev) and the detect /
decode passes in front of it.  The path is exact integer arithmetic, one fp64 fma and one rounding per pass, so this is an identity and
has no tolerance: every entry of Xr[:, :n] carries the model's float32 bit pattern (zeros compare by value: the model's exact sum has no
signed zero; NaN where the model is NaN), and the pad columns [n, ldx) are +0.0.  Shapes cross every seam of the kernel: the 128-sample
K-tile, the 85-eigen-index plane tile with its pad row, the 256-SNP tile and its two epilogue halves, one n-tile chunk and several.
PG_GENO_I8 stays unset throughout (the shipped path: the indicator pass runs on the int8 kernel too)."""
import ctypes as C

import numpy as np
import pytest

import _rotate_i8_truth as T

pytestmark = pytest.mark.gpu

NS = [1, 3, 63, 64, 65, 85, 86, 127, 128, 129, 170, 171, 255, 256, 257]
PS = [1, 2, 127, 128, 129, 255, 256, 257]
DIAG = [(1, 2), (3, 1), (63, 129), (64, 257), (65, 127), (85, 256), (86, 128), (127, 255), (128, 129), (129, 257), (170, 128), (171, 256),
        (255, 127), (256, 257), (257, 256)]
BIG = (1030, 600)       # 13 plane tiles (2 chunks of 7 + 6 at PG_GENO_CHUNK_MB=1), 9 K-tiles, 3 SNP tiles

compared = [0]          # entries that went through the bit comparison (printed per test: none is left out)


@pytest.fixture(scope="module")
def ctx():
    from pygemma_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _shipped_path(monkeypatch):
    for v in ("PG_GENO_I8", "PG_GENO_ONEPASS", "PG_GENO_CHUNK_MB"):
        monkeypatch.delenv(v, raising=False)


class Prepared:
    """U on the device (row stride ldU, `lead` columns of something else in front of it), its prepared planes, and the model's Prep"""

    def __init__(self, ctx, U, wide=None, lead=0):
        from pygemma_amd import _lib
        L = _lib.load()
        self.U, self.n = U, U.shape[0]
        self.model = T.prep(U)
        host = U if wide is None else wide
        self.ldU = host.shape[1]
        self.dU = ctx.to_device(host)
        self.u_ptr = self.dU.ptr + 4 * lead
        self.dprep = ctx.alloc(L.pg_geno_prep_bytes(self.n))
        _lib.check(L.pg_geno_prep_dev(ctx.handle, self.n, self.u_ptr, self.ldU, self.dprep.ptr), "pg_geno_prep_dev")


_bases = {}


def _basis(ctx, key):
    """the prepared basis of size n (key = n), or a named one: made once and left unchanged"""
    if key not in _bases:
        if key == "adversarial":
            U = T.adversarial_basis()[0]
        elif key == "cancelling":
            U = T.cancelling_basis()
        elif key == "identity":
            U = np.eye(86, dtype=np.float32)
        else:
            U = T.basis(key)
        _bases[key] = Prepared(ctx, U)
    return _bases[key]


def _ldxs(n):
    return sorted({n, (n + 127) // 128 * 128})


ENTRIES = {np.dtype(np.float32): ["geno", "auto"], np.dtype(np.float64): ["geno_f64"], np.dtype(np.int8): ["geno_i8", "auto_i8"],
           np.dtype(np.uint8): ["geno_i8", "auto_i8"]}


def _rotate(ctx, B, entry, src, ldx, count_a1=0, lead=0):
    """one entry point on src -> Xr (p, ldx) as the device left it (every entry preset to -77) and the path code (bed: 1).  src: packed
    records (p, ldb) for "bed", else X (n, ldX) of which the columns [lead, lead + p) are the block (ldX = its row length)."""
    from pygemma_amd import _lib
    L = _lib.load()
    n, h = B.n, ctx.handle
    src = np.ascontiguousarray(src)
    p = src.shape[0] if entry == "bed" else src.shape[1] - 2 * lead
    dS, dwork = ctx.to_device(src), ctx.alloc(L.pg_geno_work_bytes(n, p))
    dXr, dpath = ctx.alloc(p * ldx * 4), ctx.alloc(4)
    dXr.upload(np.full((p, ldx), -77.0, np.float32))
    dpath.upload(np.full(1, -1, np.int32))
    ok = C.c_int(-1)
    x_ptr, ldX = dS.ptr + lead * src.dtype.itemsize, src.shape[1]
    uns = int(src.dtype == np.uint8)
    if entry == "bed":
        assert src.dtype == np.uint8
        _lib.check(L.pg_rotate_bed_dev(h, n, p, B.dprep.ptr, dS.ptr, src.shape[1], int(count_a1), dXr.ptr, ldx, dwork.ptr), entry)
        ok.value = 1
    elif entry == "geno":
        assert src.dtype == np.float32
        _lib.check(L.pg_rotate_geno_dev(h, n, p, B.dprep.ptr, x_ptr, ldX, dXr.ptr, ldx, dwork.ptr, C.byref(ok)), entry)
    elif entry == "auto":
        assert src.dtype == np.float32
        _lib.check(L.pg_rotate_auto_dev(h, n, p, B.u_ptr, B.ldU, B.dprep.ptr, x_ptr, ldX, dXr.ptr, ldx, dwork.ptr, dpath.ptr), entry)
    elif entry == "geno_i8":
        assert src.dtype in (np.int8, np.uint8)
        _lib.check(L.pg_rotate_geno_i8_dev(h, n, p, B.dprep.ptr, x_ptr, uns, ldX, dXr.ptr, ldx, dwork.ptr, C.byref(ok)), entry)
    elif entry == "auto_i8":
        assert src.dtype in (np.int8, np.uint8)
        _lib.check(L.pg_rotate_auto_i8_dev(h, n, p, B.dprep.ptr, x_ptr, uns, ldX, dXr.ptr, ldx, dwork.ptr, dpath.ptr), entry)
    elif entry == "geno_f64":
        assert src.dtype == np.float64
        _lib.check(L.pg_rotate_geno_f64_dev(h, n, p, B.dprep.ptr, x_ptr, ldX, dXr.ptr, ldx, dwork.ptr, C.byref(ok)), entry)
    else:
        raise AssertionError(entry)
    ctx.sync()
    path = int(dpath.download((1,), np.int32)[0]) if entry.startswith("auto") else int(ok.value)
    out = dXr.download((p, ldx), np.float32)
    for b in (dS, dwork, dXr, dpath):
        b.free()
    return out, path


def _assert_bits(got, want, what):
    """got (p, ldx) from the device, want (p, n) from the model: the identity of the module docstring, over every entry"""
    p, n = want.shape
    assert got.shape[0] == p and got.shape[1] >= n
    g = np.ascontiguousarray(got[:, :n])
    nan = np.isnan(want)
    same = (g.view(np.uint32) == want.view(np.uint32)) | ((g == 0) & (want == 0))
    same = np.where(nan, np.isnan(g), same)
    if not same.all():
        r, k = np.argwhere(~same)[0]
        raise AssertionError(f"{what}: {int((~same).sum())} of {same.size} entries differ, first at SNP {r}, eigen index {k}: device "
                             f"{g[r, k]!r} ({g.view(np.uint32)[r, k]:#010x}), model {want[r, k]!r} ({want.view(np.uint32)[r, k]:#010x}); "
                             f"SNP rows {sorted(set(np.argwhere(~same)[:, 0]))[:8]}, eigen indices {sorted(set(np.argwhere(~same)[:, 1]))[:8]}")
    pad = np.ascontiguousarray(got[:, n:])
    assert (pad.view(np.uint32) == 0).all(), f"{what}: pad columns [n, ldx) are not +0.0"
    compared[0] += same.size


def _bed_case(ctx, B, G, what, count_a1s=(0, 1), extras=(0, 3), ldxs=None):
    """every (count_a1, ldb, ldx) of one panel of hard calls against the model"""
    n = B.n
    for count_a1 in count_a1s:
        want = None
        for extra in extras:
            data = T.pack_bed(G, count_a1, extra=extra, seed=extra)
            model = T.rotate(B.model, *T.encode_bed(data, n, count_a1))
            if want is not None:                         # the bytes past ceil(n/4) and other pad bits change nothing
                assert (model.view(np.uint32) == want.view(np.uint32)).all()
            want = model
            for ldx in (ldxs or _ldxs(n)):
                got, _ = _rotate(ctx, B, "bed", data, ldx, count_a1)
                _assert_bits(got, want, f"{what} bed count_a1={count_a1} ldb=+{extra} ldx={ldx}")
    return want


@pytest.mark.parametrize("n", NS)
def test_bed_without_missing_calls_full_grid(n, ctx):
    """every p of the grid at this n; the random calls have no missing one, the special SNPs of every block do (T.hard_calls)"""
    B = _basis(ctx, n)
    for p in PS:
        _bed_case(ctx, B, T.hard_calls(n, p, seed=1), f"n={n} p={p}")
    print("entries compared so far:", compared[0])


@pytest.mark.parametrize("n,p", DIAG)
def test_bed_with_missing_calls(n, p, ctx):
    B = _basis(ctx, n)
    G = T.hard_calls(n, p, seed=2, miss=0.02)
    _bed_case(ctx, B, G, f"n={n} p={p} 2% missing")
    print("entries compared so far:", compared[0])


def _array_case(ctx, B, X, what, ldxs=None, entries=None):
    want = T.rotate(B.model, *T.encode_x(X))
    for entry in (entries or ENTRIES[X.dtype]):
        for ldx in (ldxs or _ldxs(B.n)):
            got, path = _rotate(ctx, B, entry, X, ldx)
            assert path == 1, (what, entry, path)
            _assert_bits(got, want, f"{what} {X.dtype} {entry} ldx={ldx}")
    return want


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int8, np.uint8], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("n,p", DIAG)
def test_arrays_every_entry_point(n, p, dtype, ctx):
    """raw calls, two-valued and one-valued columns, centred and standardised ones, with one other value (the indicator pass runs for the
    whole block) and without (it does not)"""
    B = _basis(ctx, n)
    for imputed in (True, False):
        X = T.array_block(n, p, dtype, seed=3, imputed=imputed)
        has_other = bool(T.encode_x(X)[3].any())
        assert not has_other if not imputed else (has_other or p < 8 or n < 16)
        _array_case(ctx, B, X, f"n={n} p={p} imputed={imputed}")
    print("entries compared so far:", compared[0])


@pytest.fixture(scope="module")
def big(ctx):
    """the multi-tile case: basis, sources and their models, made once"""
    n, p = BIG
    B = _basis(ctx, n)
    G = T.hard_calls(n, p, seed=4, miss=0.02)
    bed = T.pack_bed(G, 0, extra=3)
    Xf, Xi = T.array_block(n, p, np.float32, seed=4), T.array_block(n, p, np.int8, seed=4)
    return B, {"bed": (bed, T.rotate(B.model, *T.encode_bed(bed, n, 0))), "auto": (Xf, T.rotate(B.model, *T.encode_x(Xf))),
               "geno_i8": (Xi, T.rotate(B.model, *T.encode_x(Xi)))}


@pytest.mark.parametrize("chunk_mb", [None, "1"])
def test_multi_tile_and_chunked_tile_order(chunk_mb, big, ctx, monkeypatch):
    """n = 1030, p = 600 in one chunk of plane tiles (default) and, at PG_GENO_CHUNK_MB=1, in two chunks of 7 and 6: the tile order of
    launch_geno_i8 must reach every output tile exactly as before"""
    if chunk_mb is not None:
        monkeypatch.setenv("PG_GENO_CHUNK_MB", chunk_mb)
        n = BIG[0]
        ldk8, tiles8 = (n + 127) // 128 * 128, (n + 84) // 85
        ncmax = max(8, (1 << 20) // (256 * ldk8))
        assert tiles8 == 13 and -(-tiles8 // ncmax) == 2 and tiles8 % 2 == 1      # what the launch derives from the variable
    B, cases = big
    for entry, (src, want) in cases.items():
        for ldx in _ldxs(B.n):
            got, path = _rotate(ctx, B, entry, src, ldx)
            assert path == 1
            _assert_bits(got, want, f"n=1030 p=600 chunk_mb={chunk_mb} {entry} ldx={ldx}")
    print("entries compared so far:", compared[0])


def test_two_pass_detect(ctx, monkeypatch):
    monkeypatch.setenv("PG_GENO_ONEPASS", "0")
    B = _basis(ctx, 257)
    for dtype in (np.float32, np.uint8):
        _array_case(ctx, B, T.array_block(257, 129, dtype, seed=5), "two-pass detect")


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int8], ids=lambda d: np.dtype(d).name)
def test_column_window_of_a_wider_matrix(dtype, ctx):
    """ldX > p: the block is columns [2, 2 + p) of rows of p + 4; the columns beside it hold NaN (floats) or dosages (8-bit), either of
    which would take the block off the genotype path if it were read"""
    n, p, lead = 171, 129, 2
    B = _basis(ctx, n)
    X = T.array_block(n, p, dtype, seed=6)
    wide = np.full((n, p + 2 * lead), np.nan if np.dtype(dtype).kind == "f" else 0, dtype)
    if np.dtype(dtype).kind != "f":
        wide[:] = np.random.default_rng(6).integers(0, 100, wide.shape)
    wide[:, lead:lead + p] = X
    want = T.rotate(B.model, *T.encode_x(X))
    for entry in ENTRIES[np.dtype(dtype)]:
        got, path = _rotate(ctx, B, entry, wide, 256, lead=lead)
        assert path == 1
        _assert_bits(got, want, f"window {np.dtype(dtype).name} {entry}")


def test_prepare_from_a_window_of_a_wider_matrix(ctx):
    """pg_geno_prep_dev with ldU = n + 5: U is columns [2, 2 + n) of a matrix whose other columns hold NaN"""
    n, lead = 129, 2
    U = T.basis(n, seed=1)
    wide = np.full((n, n + 5), np.nan, np.float32)
    wide[:, lead:lead + n] = U
    B = Prepared(ctx, U, wide=wide, lead=lead)
    assert B.ldU == n + 5
    _bed_case(ctx, B, T.hard_calls(n, 130, seed=7, miss=0.02), "ldU = n + 5")
    _array_case(ctx, B, T.array_block(n, 130, np.float32, seed=7), "ldU = n + 5")     # "auto" hands the same window to the fp32 fallback
    for b in (B.dU, B.dprep):
        b.free()


@pytest.mark.parametrize("n,p", [(130, 257), (257, 300)])
def test_one_bit_pattern_across_storages(n, p, ctx):
    """the same hard calls without a missing one, every column holding a 0 and a 2 (so that v0 = 0 and dx = 1 from every storage),
    through .bed, int8, uint8, float32 and float64"""
    B = _basis(ctx, n)
    G = T.hard_calls(n, p, seed=8, specials=False)
    G[0], G[n - 1], G[n // 2] = 0, 2, 1
    want = T.rotate(B.model, *T.encode_bed(T.pack_bed(G, 0), n, 0))
    ldx = (n + 127) // 128 * 128
    outs = {"bed": _rotate(ctx, B, "bed", T.pack_bed(G, 0), ldx)[0]}
    for dtype, entries in ENTRIES.items():
        for entry in entries:
            outs[f"{dtype.name} {entry}"], path = _rotate(ctx, B, entry, G.astype(dtype), ldx)
            assert path == 1
    for name, got in outs.items():
        assert (got.view(np.uint32) == outs["bed"].view(np.uint32)).all(), name
        _assert_bits(got, want, f"storages {name}")
    assert len(outs) == 8


def test_adversarial_eigenvectors(ctx):
    """the columns of T.adversarial_basis (T.ADVERSARIAL names them): only the two with a NaN / Inf may give NaN"""
    B = _basis(ctx, "adversarial")
    n = B.n
    bad = T.adversarial_basis()[1]
    want = _bed_case(ctx, B, T.hard_calls(n, 130, seed=9, miss=0.02), "adversarial", extras=(0,))
    assert np.isnan(want[:, bad]).all() and np.isfinite(want[:, ~bad]).all()
    for dtype in ENTRIES:
        for imputed in (True, False):
            want = _array_case(ctx, B, T.array_block(n, 130, dtype, seed=9, imputed=imputed), f"adversarial imputed={imputed}")
            assert np.isnan(want[:, bad]).all() and np.isfinite(want[:, ~bad]).all()
    print("entries compared so far:", compared[0])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_cancelling_basis_shows_the_fp64_steps(dtype, ctx):
    """T.cancelling_basis: the order of the fp64 column sums (tiles of 64 in sequence, then the partials) and the single rounding of the
    fma decide thousands of these float32 outputs (tests/test_host_rotate_i8_truth.py counts them)"""
    B = _basis(ctx, "cancelling")
    _array_case(ctx, B, T.cancelling_block(B.n, 130, dtype), "cancelling")


def test_identity_basis(ctx):
    B = _basis(ctx, "identity")
    G = T.hard_calls(B.n, 129, seed=10, miss=0.02)
    _bed_case(ctx, B, G, "U = I")
    for dtype in ENTRIES:
        _array_case(ctx, B, T.array_block(B.n, 129, dtype, seed=10), "U = I")
