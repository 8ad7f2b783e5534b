"""CPU checks of the LD feature: the truth helper against np.corrcoef, the pure-NumPy decisions (_prune_band, _clump_band) against plain
loops over dense truth matrices, the public surface, every refusal before the device, and the C ABI's argument checks."""
import inspect

import numpy as np
import pandas as pd
import pytest

import _ld_truth as T


def _lib_loaded():
    from pygemma_amd import _lib
    return _lib.load()


def test_truth_r_is_corrcoef_on_the_jointly_called_samples():
    G = T.ld_panel(203, 40, seed=1)
    S = T.sums(G)
    R = T.r64_of(S)
    checked = 0
    for a in range(40):
        for b in range(40):
            both = np.isfinite(G[:, a]) & np.isfinite(G[:, b])
            xa, xb = G[both, a], G[both, b]
            hard = all(np.isin(G[np.isfinite(G[:, c]), c], (0, 1, 2)).all() for c in (a, b))
            if not hard or both.sum() == 0 or xa.std() == 0 or xb.std() == 0:
                assert np.isnan(R[a, b]), (a, b)
                continue
            assert abs(R[a, b] - np.corrcoef(xa, xb)[0, 1]) <= 1e-12, (a, b)
            checked += 1
    assert checked > 1000
    assert np.array_equal(T.r_of(S), R.astype(np.float32), equal_nan=True)


@pytest.mark.parametrize("n", [5, 64, 1001, 10000])
def test_truth_copies_and_flips_are_exactly_one(n):
    rng = np.random.default_rng(n)
    x = rng.binomial(2, 0.3, n).astype(np.float64)
    x[:3] = [0, 1, 2]
    x[rng.random(n) < 0.05] = np.nan
    x[:3] = [0, 1, 2]
    R = T.r_of(T.sums(np.stack([x, x.copy(), 2 - x], axis=1)))
    assert R[0, 1] == 1.0 and R[0, 2] == -1.0 and R[1, 2] == -1.0 and R[0, 0] == 1.0


def test_truth_not_hard_call_is_all_missing():
    G = T.ld_panel(80, 30, seed=3)
    S = T.sums(G)
    for col in (30 - 3, 30 - 8):                 # all missing, dosage
        assert (S[col] == 0).all() and (S[:, col] == 0).all()
    assert np.isnan(T.r_of(S)[30 - 2]).all()     # monomorphic


@pytest.mark.parametrize("seed,w,r2", [(0, 1, 0.5), (1, 7, 0.2), (2, 50, 0.5), (3, 200, 0.8), (4, 7, 0.0), (5, 7, 1.0)])
def test_prune_band_is_the_truth_loop(seed, w, r2):
    from pygemma_amd import lmm
    R = T.r_of(T.sums(T.ld_panel(90, 120, seed)))          # holds NaN rows (monomorphic, all-missing, dosage) and exact +-1
    assert np.isnan(R).any() and (np.abs(R[~np.isnan(R)]) == 1).any()
    keep = lmm._prune_band(T.band_of(R, w), r2)
    assert keep.dtype == np.bool_ and (keep == T.prune(R, w, r2)).all()
    assert keep[120 - 2] and keep[120 - 3]                 # no r: kept


def _clump_case(seed, p=150, with_chrom=False, with_pos=False, ties=False):
    rng = np.random.default_rng(seed)
    R = T.r_of(T.sums(T.ld_panel(90, p, seed)))
    pv = rng.uniform(0, 0.03, p)
    small = rng.random(p) < 0.25
    pv[small] = rng.uniform(0, 2e-4, int(small.sum()))
    if ties:
        pv[small] = np.round(pv[small], 4)                 # many equal p-values, zeros among them
    pv[rng.random(p) < 0.1] = np.nan
    chrom = np.repeat([1, 2, 7], [p // 3, p // 3, p - 2 * (p // 3)]) if with_chrom else None
    pos = None
    if with_pos:
        pos = np.cumsum(rng.integers(0, 40, p))
        if with_chrom:
            for c in np.unique(chrom):
                pos[chrom == c] -= pos[chrom == c][0]      # positions restart on every chromosome
    return R, pv, chrom, pos


@pytest.mark.parametrize("seed,with_chrom,with_pos,ties,window", [(0, False, False, False, 10), (1, True, False, False, 25), (2, False, True, False, 300),
                                                                  (3, True, True, True, 200), (4, False, False, True, 149), (5, True, True, False, 1)])
def test_clump_band_is_the_truth_loop(seed, with_chrom, with_pos, ties, window):
    from pygemma_amd import lmm
    R, pv, chrom, pos = _clump_case(seed, with_chrom=with_chrom, with_pos=with_pos, ties=ties)
    p, p1, p2, r2 = len(pv), 1e-4, 1e-2, 0.3
    want = T.clump(R, pv, p1, p2, r2, window, chrom, pos)
    assert len(want) >= 3
    with np.errstate(invalid="ignore"):
        cand = np.flatnonzero(pv < p2)
    run = np.zeros(p, np.int64) if chrom is None else np.concatenate([[0], np.cumsum(chrom[1:] != chrom[:-1])])
    coord = np.arange(p) if pos is None else pos
    width = int(lmm._clump_reach(coord[cand], run[cand], window).max())
    # the reach is exact: no in-range candidate pair lies further apart than `width` candidates, and one pair lies that far
    far = [b - a for a in range(len(cand)) for b in range(a + 1, len(cand))
           if run[cand[a]] == run[cand[b]] and abs(coord[cand[b]] - coord[cand[a]]) <= window]
    assert width == (max(far) if far else 0)
    band = T.band_of(R[np.ix_(cand, cand)], width)
    got = lmm._clump_band(band, pv[cand], coord[cand], run[cand], p1, r2, window)
    got = sorted(((pv[cand[c]], cand[c], sorted(cand[m])) for c, m in got))
    assert [(j, mem) for _, j, mem in got] == [(j, mem) for j, mem in want]


@pytest.mark.parametrize("dtype", [np.uint32, np.uint64, np.uint8, np.int32, np.float32])
def test_unsigned_positions_clump_like_signed_ones(dtype, monkeypatch):
    """An index SNP takes the candidates to its LEFT as well: the distance is a signed difference whatever the dtype of pos."""
    from pygemma_amd import lmm
    pos = np.array([0, 10, 20, 30, 40])
    pv = np.array([1e-3, 1e-3, 1e-9, 1e-3, 1e-3])
    band = np.ones((5, 4), np.float32)
    run = np.zeros(5, np.int64)
    want = lmm._clump_band(band, pv, pos.astype(np.int64), run, 1e-4, 0.5, 100)
    assert [(c, m.tolist()) for c, m in want] == [(2, [0, 1, 3, 4])]
    got = lmm._clump_band(band, pv, pos.astype(dtype), run, 1e-4, 0.5, 100)
    assert [(c, m.tolist()) for c, m in got] == [(2, [0, 1, 3, 4])]
    assert (lmm._clump_reach(pos.astype(dtype), run, 100) == [4, 3, 2, 1, 0]).all()
    # the public entry, its band from the truth instead of the device
    G = np.repeat(np.random.default_rng(0).integers(0, 3, (30, 1)), 5, axis=1).astype(np.float32)      # five copies of one SNP: r = 1
    monkeypatch.setattr(lmm, "ld_window", lambda X, w, **kw: T.band_of(T.r_of(T.sums(np.asarray(X, np.float64))), w))
    df = pd.DataFrame({"p_wald": pv})
    for kind in (np.int64, dtype):
        out = lmm.clump(df, G, p1=1e-4, p2=1e-2, r2=0.5, window=100, pos=pos.astype(kind))
        assert out["index"].tolist() == [2] and out["members"][0].tolist() == [0, 1, 3, 4] and out["n_members"].tolist() == [4]
    truth = T.clump(T.r_of(T.sums(G.astype(np.float64))), pv, 1e-4, 1e-2, 0.5, 100, pos=pos.astype(dtype))
    assert truth == [(2, [0, 1, 3, 4])]
    with pytest.raises(ValueError):
        lmm.clump(df, G, pos=np.array([0, 1, 2, 3, 2 ** 63], np.uint64))


def test_public_names_signatures_and_defaults():
    import pygemma.lmm as ref_style
    from pygemma_amd import lmm
    for name in ("ld", "ld_window", "ld_prune", "clump"):
        assert name in lmm.__all__ and getattr(ref_style, name) is getattr(lmm, name)
    sig = {k: str(inspect.signature(getattr(lmm, k))) for k in ("ld", "ld_window", "ld_prune", "clump")}
    assert sig["ld"] == "(X, a=None, b=None, *, counts=False, device=0, stats=None)"
    assert sig["ld_window"] == "(X, window, *, snp_batch=None, device=0, verbose=0, stats=None)"
    assert sig["ld_prune"] == "(X, window=50, r2=0.5, **stream_kw)"
    assert sig["clump"] == "(df, X, p1=0.0001, p2=0.01, r2=0.5, window=250, col='p_wald', chrom=None, pos=None, **stream_kw)"
    for name in ("_prune_band", "_clump_band"):
        assert callable(getattr(lmm, name))


def _no_device(monkeypatch):
    from pygemma_amd import _lib
    monkeypatch.setattr(_lib, "device_count", lambda: pytest.fail("reached the device"))
    monkeypatch.setattr(_lib, "Context", lambda *a, **k: pytest.fail("reached the device"))


X0 = np.random.default_rng(0).integers(0, 3, (20, 6)).astype(np.float32)
BAD_X = {"X 1-D": X0[:, 0], "X 3-D": X0[:, :, None], "X int32": X0.astype(np.int32), "X float16": X0.astype(np.float16), "no SNPs": X0[:, :0],
         "no samples": X0[:0]}


@pytest.mark.parametrize("bad", sorted(BAD_X))
def test_bad_genotypes_are_refused_before_the_device(bad, monkeypatch):
    from pygemma_amd import lmm
    _no_device(monkeypatch)
    X = BAD_X[bad]
    df = pd.DataFrame({"p_wald": np.full(X.shape[1] if X.ndim > 1 else 1, 0.5)})
    for call in (lambda: lmm.ld(X), lambda: lmm.ld_window(X, 3), lambda: lmm.ld_prune(X), lambda: lmm.clump(df, X)):
        with pytest.raises(ValueError):
            call()


@pytest.mark.parametrize("bad", ["window 0", "window float", "window bool", "window negative", "snp_batch 0", "snp_batch float", "snp_batch bool"])
def test_bad_window_and_batch_are_refused_before_the_device(bad, monkeypatch):
    from pygemma_amd import lmm
    _no_device(monkeypatch)
    df = pd.DataFrame({"p_wald": np.full(6, 1e-6)})
    if bad.startswith("window"):
        w = {"window 0": 0, "window float": 3.0, "window bool": True, "window negative": -2}[bad]
        calls = [lambda: lmm.ld_window(X0, w), lambda: lmm.ld_prune(X0, w), lambda: lmm.clump(df, X0, window=w)]
    else:
        sb = {"snp_batch 0": 0, "snp_batch float": 64.0, "snp_batch bool": True}[bad]
        calls = [lambda: lmm.ld_window(X0, 3, snp_batch=sb), lambda: lmm.ld_prune(X0, snp_batch=sb), lambda: lmm.clump(df, X0, snp_batch=sb)]
    for call in calls:
        with pytest.raises(ValueError):
            call()


def test_clump_with_pos_takes_a_real_window_but_not_less_than_one(monkeypatch):
    from pygemma_amd import lmm
    _no_device(monkeypatch)
    df = pd.DataFrame({"p_wald": np.full(6, 0.5)})
    out = lmm.clump(df, X0, window=2.5e5, pos=np.arange(6) * 1000.0)          # no candidate: no device work at all
    assert list(out.columns) == ["index", "p", "n_members", "members"] and len(out) == 0
    with pytest.raises(ValueError):
        lmm.clump(df, X0, window=0.5, pos=np.arange(6))


@pytest.mark.parametrize("name,value", [("r2", -0.1), ("r2", 1.5), ("r2", float("nan")), ("r2", "x"), ("p1", -1e-3), ("p1", 2), ("p2", 1.01), ("p2", None)])
def test_thresholds_outside_the_unit_interval_are_refused(name, value, monkeypatch):
    from pygemma_amd import lmm
    _no_device(monkeypatch)
    df = pd.DataFrame({"p_wald": np.full(6, 1e-6)})
    with pytest.raises(ValueError):
        lmm.clump(df, X0, **{name: value})
    if name == "r2":
        with pytest.raises(ValueError):
            lmm.ld_prune(X0, r2=value)


@pytest.mark.parametrize("bad", [np.ones(7, bool), np.ones((6, 1), bool), [6], [-7], np.array([0.0, 1.0]), np.zeros((2, 2), np.int64), np.zeros(6, bool),
                                 np.zeros(0, np.int64)])
def test_index_and_mask_errors_are_those_of_take(bad, monkeypatch):
    from pygemma_amd import lmm
    from pygemma_amd.bed import PackedBed
    _no_device(monkeypatch)
    bed = PackedBed(T.pack(X0.astype(np.float64)), 20)
    for X in (X0, bed):
        with pytest.raises(ValueError):
            lmm.ld(X, bad)
        with pytest.raises(ValueError):
            lmm.ld(X, [0, 1], bad)


@pytest.mark.parametrize("bad", ["df short", "df long", "no column", "chrom short", "chrom 2-D", "pos long", "pos decreasing", "pos strings", "pos nan"])
def test_clump_length_mismatches_are_refused(bad, monkeypatch):
    from pygemma_amd import lmm
    _no_device(monkeypatch)
    kw, rows, col = {}, 6, "p_wald"
    if bad == "df short":
        rows = 5
    elif bad == "df long":
        rows = 7
    elif bad == "no column":
        col = "p_lrt"
    elif bad == "chrom short":
        kw["chrom"] = [1] * 5
    elif bad == "chrom 2-D":
        kw["chrom"] = np.ones((6, 1))
    elif bad == "pos long":
        kw["pos"] = np.arange(7)
    elif bad == "pos decreasing":
        kw["pos"] = [0, 10, 20, 15, 30, 40]
    elif bad == "pos strings":
        kw["pos"] = list("abcdef")
    elif bad == "pos nan":
        kw["pos"] = [0, 1, 2, np.nan, 4, 5]
    df = pd.DataFrame({col: np.full(rows, 1e-6)})
    with pytest.raises(ValueError):
        lmm.clump(df, X0, **kw)


def test_pos_may_restart_on_a_new_chromosome(monkeypatch):
    from pygemma_amd import lmm
    _no_device(monkeypatch)
    df = pd.DataFrame({"p_wald": np.full(6, 0.5)})
    assert len(lmm.clump(df, X0, chrom=[1, 1, 1, 2, 2, 2], pos=[5, 6, 7, 1, 2, 3])) == 0
    with pytest.raises(ValueError):
        lmm.clump(df, X0, chrom=[1, 1, 1, 1, 2, 2], pos=[5, 6, 7, 1, 2, 3])


ENTRY = {
    "pg_ld_encode_bed_dev": lambda L, p: L.pg_ld_encode_bed_dev(None, 8, 1, p, 2, 0, p, 1, 0),
    "pg_ld_encode_x_dev": lambda L, p: L.pg_ld_encode_x_dev(None, 8, 1, p, 2, 8, 1, p, 1, 0),
    "pg_ld_shift_dev": lambda L, p: L.pg_ld_shift_dev(None, 8, p, 4, 1, 2),
    "pg_ld_block_dev": lambda L, p: L.pg_ld_block_dev(None, 8, p, 1, 0, 1, p, 1, 0, 1, p, 1, None),
    "pg_ld_band_dev": lambda L, p: L.pg_ld_band_dev(None, 8, p, 4, 0, 2, 4, 3, p, 3, None),
}


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_device_entry_points_refuse_a_null_context_by_name(name):
    L = _lib_loaded()
    buf = np.zeros(4096, np.uint8)
    assert ENTRY[name](L, buf.ctypes.data) == -22          # PG_EINVAL
    assert name in L.pg_last_error().decode()
    assert not buf.any()


def test_image_bytes():
    L = _lib_loaded()
    for n, pe in ((0, 4), (-1, 4), (1 << 28, 4), (100, 0), (100, -3), (100, 1 << 31)):
        assert L.pg_ld_image_bytes(n, pe) == 0
    sizes = [L.pg_ld_image_bytes(1000, pe) for pe in (1, 2, 85, 256, 10000)]
    assert all(b > a > 0 for a, b in zip(sizes, sizes[1:]))
    assert L.pg_ld_image_bytes((1 << 28) - 1, 1) >= 3 * ((1 << 28) - 1)
    assert L.pg_ld_image_bytes(1000, 256) >= 3 * 256 * 1000 + 16 * 256     # three int8 planes and the totals


def test_no_gpu_means_loud_failure_not_fallback():
    from pygemma_amd import _lib, lmm
    from pygemma_amd.bed import PackedBed
    _lib_loaded()
    if _lib.device_count() > 0:
        pytest.skip("a GPU is visible here")
    G = np.random.default_rng(0).integers(0, 3, (20, 6)).astype(np.float64)
    df = pd.DataFrame({"p_wald": np.full(6, 1e-6)})
    for X in (G.astype(np.float32), G.astype(np.int8), PackedBed(T.pack(G), 20)):
        for call in (lambda: lmm.ld(X), lambda: lmm.ld_window(X, 3), lambda: lmm.ld_prune(X), lambda: lmm.clump(df, X)):
            with pytest.raises(_lib.PgError):
                call()
