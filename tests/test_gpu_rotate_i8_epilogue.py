"""The epilogue of rotate_geno_i8_kernel — the staged halves of 128 SNP rows, the 85 eigen columns of a plane tile, the row groups of six
and the steps of four rows a thread walks — against the host model (tests/_rotate_i8_truth.py), BIT FOR BIT, inside guard bands.

Shapes (n, p): (1, 1) the smallest; (85, 128) one tile column and one half, exactly full; (86, 129) a second n-tile with one valid
column and a second half with one valid row; (170, 256) two exact n-tiles and one exact m-tile; (341, 513) five n-tiles, the last with
one column, and three m-tiles, the last with one row.  Each through pg_rotate_bed_dev (packed .bed) and pg_rotate_geno_dev (float32).

Every call writes into a buffer preset to a signalling-NaN pattern no result can equal, with guard floats in front of row 0 and behind
row p - 1.  Asserted: Xr[:, :n] carries the model's bits (so no sentinel is left), the pad columns [n, ldx) are +0.0, the guards are
untouched, and a second call into the same buffer leaves the same bits.  Leading dimensions: the smallest multiple of 64 that holds n
and a second one — the wider roundup(n, 128) where that differs (n = 1, 170); for n = 85, 86 and 341 the two coincide and the entry
points refuse anything wider (n <= ldx <= roundup(n, 128)), so the second one there is ldx = n, the unaligned rows.

The accumulating pass (Xr += dlt * U'ind, run for the whole block as soon as one column holds an imputed value / a missing call) is
driven by columns with exactly one such entry, placed in the SNP rows 0, 127, 128, 255, 256 and p - 1 (where p has them); the model's
own indicator products are asserted non-zero in the eigen columns 0, 84, 85 and n - 1 of those rows, so the pass changes those outputs.
The same sources without those entries run the write pass alone."""
import ctypes as C

import numpy as np
import pytest

import _rotate_i8_truth as T

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (85, 128), (86, 129), (170, 256), (341, 513)]
GUARD = 64                                   # floats in front of and behind Xr (256 bytes: the alignment of Xr is the allocation's)
SENTINEL = np.uint32(0x7FA5A5A5)             # a signalling NaN: the kernel's NaNs are quiet, and these bases give none
GUARD_BITS = np.uint32(0x7FB6B6B6)
EDGE_ROWS = (0, 127, 128, 255, 256)
EDGE_COLS = (0, 84, 85)


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


def _ldxs(n):
    r64, r128 = (n + 63) // 64 * 64, (n + 127) // 128 * 128
    return [r64, r128 if r128 > r64 else n]


def _edge_rows(p):
    return sorted({r for r in EDGE_ROWS + (p - 1,) if r < p})


def _sources(n, p, imputed):
    """(.bed records, float32 array) of one shape; with `imputed`, SNP g of _edge_rows(p) has one missing call / one other value in
    sample g % n"""
    G = T.hard_calls(n, p, seed=21, specials=False)
    X = T.array_block(n, p, np.float32, seed=21, imputed=False)
    if imputed:
        rng = np.random.default_rng(77 * n + p)
        for g in _edge_rows(p):
            G[g % n, g] = np.nan
            if n >= 3:                       # a column needs its two extremes beside the other value
                col = rng.integers(0, 3, n).astype(np.float32)
                i = g % n
                col[(i + 1) % n], col[(i + 2) % n], col[i] = 0.0, 2.0, 0.3125
                X[:, g] = col
    return T.pack_bed(G, 0), X


_cases = {}


def _case(ctx, n, p, imputed):
    """prepared basis, sources and their models of one shape: made once, left unchanged"""
    key = (n, p, imputed)
    if key not in _cases:
        from pygemma_amd import _lib
        L = _lib.load()
        if n not in _cases:
            U = T.basis(n, seed=2)
            dU, dprep = ctx.to_device(U), ctx.alloc(L.pg_geno_prep_bytes(n))
            _lib.check(L.pg_geno_prep_dev(ctx.handle, n, dU.ptr, n, dprep.ptr), "pg_geno_prep_dev")
            _cases[n] = (T.prep(U), dprep, dU)
        model, dprep, _ = _cases[n]
        bed, X = _sources(n, p, imputed)
        enc = {"bed": T.encode_bed(bed, n, 0), "geno": T.encode_x(X)}
        for name, e in enc.items():
            ind = e[3]
            runs_pass2 = bool(ind.any())
            assert runs_pass2 == (imputed and (name == "bed" or n >= 3)), (name, n, p)
            if runs_pass2:                   # the accumulating pass reaches the rows and eigen columns at the seams of the epilogue
                rows = _edge_rows(p)
                assert all(ind[:, g].sum() == 1 for g in rows)
                Pind = T._dot(ind, model.q)
                cols = sorted({k for k in EDGE_COLS + (n - 1,) if k < n})
                assert (Pind[np.ix_(rows, cols)] != 0).all(), (name, n, p)
        want = {name: T.rotate(model, *e) for name, e in enc.items()}
        _cases[key] = (dprep, {"bed": bed, "geno": X}, want)
    return _cases[key]


def _call(ctx, L, entry, n, p, dprep, dS, src, xr_ptr, ldx, dwork):
    from pygemma_amd import _lib
    if entry == "bed":
        _lib.check(L.pg_rotate_bed_dev(ctx.handle, n, p, dprep.ptr, dS.ptr, src.shape[1], 0, xr_ptr, ldx, dwork.ptr), entry)
    else:
        ok = C.c_int(-1)
        _lib.check(L.pg_rotate_geno_dev(ctx.handle, n, p, dprep.ptr, dS.ptr, src.shape[1], xr_ptr, ldx, dwork.ptr, C.byref(ok)), entry)
        assert ok.value == 1, "the block left the genotype path"
    ctx.sync()


def _check(buf, want, n, p, ldx, what):
    bits = buf.view(np.uint32)
    assert (bits[:GUARD] == GUARD_BITS).all(), f"{what}: the guard in front of row 0 was written"
    assert (bits[GUARD + p * ldx:] == GUARD_BITS).all(), f"{what}: the guard behind row p - 1 was written"
    got = bits[GUARD:GUARD + p * ldx].reshape(p, ldx)
    left = got[:, :n] == SENTINEL
    assert not left.any(), f"{what}: {int(left.sum())} outputs never written, first at {tuple(np.argwhere(left)[0])}"
    assert (got[:, n:] == 0).all(), f"{what}: pad columns [n, ldx) are not +0.0"
    w = want.view(np.uint32)
    same = (got[:, :n] == w) | ((got[:, :n].view(np.float32) == 0) & (want == 0))
    if not same.all():
        r, k = np.argwhere(~same)[0]
        raise AssertionError(f"{what}: {int((~same).sum())} of {same.size} entries differ, first at SNP {r}, eigen index {k}: device "
                             f"{got[r, k]:#010x}, model {w[r, k]:#010x}; SNP rows {sorted(set(np.argwhere(~same)[:, 0]))[:8]}, "
                             f"eigen indices {sorted(set(np.argwhere(~same)[:, 1]))[:8]}")


@pytest.mark.parametrize("imputed", [False, True], ids=["write-pass", "accumulating-pass"])
@pytest.mark.parametrize("entry", ["bed", "geno"])
@pytest.mark.parametrize("n,p", SHAPES)
def test_epilogue_bits_guards_and_stability(n, p, entry, imputed, ctx):
    from pygemma_amd import _lib
    L = _lib.load()
    dprep, srcs, wants = _case(ctx, n, p, imputed)
    src, want = np.ascontiguousarray(srcs[entry]), wants[entry]
    assert np.isfinite(want).all()
    dS, dwork = ctx.to_device(src), ctx.alloc(L.pg_geno_work_bytes(n, p))
    for ldx in _ldxs(n):
        what = f"n={n} p={p} {entry} imputed={imputed} ldx={ldx}"
        total = 2 * GUARD + p * ldx
        host = np.full(total, SENTINEL, np.uint32)
        host[:GUARD] = GUARD_BITS
        host[GUARD + p * ldx:] = GUARD_BITS
        dXr = ctx.alloc(total * 4)
        dXr.upload(host.view(np.float32))
        _call(ctx, L, entry, n, p, dprep, dS, src, dXr.ptr + 4 * GUARD, ldx, dwork)
        first = dXr.download((total,), np.float32)
        _check(first, want, n, p, ldx, what)
        _call(ctx, L, entry, n, p, dprep, dS, src, dXr.ptr + 4 * GUARD, ldx, dwork)
        second = dXr.download((total,), np.float32)
        assert (first.view(np.uint32) == second.view(np.uint32)).all(), f"{what}: a second call into the same Xr changed bits"
        dXr.free()
    for b in (dS, dwork):
        b.free()
