"""The two-slot host -> device feed of the streamed entry points (pygemma_amd/_feed.py) at the smallest shapes that reach every
branch of it: n no multiple of 4 or 64, a ragged last batch, one / two / three / six batches, every source kind from ordinary
memory (staged through pinned buffers) and from pinned memory (the DMA reads the source), eigenvectors from pageable memory in
several panels, and the clean-up after a consumer that raises.  The same bytes reach the same slot at the same pitch before the
same kernels whichever way they travel, so the comparisons between the two are equalities of bit patterns."""
import functools

import numpy as np
import pytest

from pygemma_amd.bed import PackedBed
from test_gpu_kinship_stream import _pack, check_gate, make_dosages, truth

pytestmark = pytest.mark.gpu

LM_COLS = ("beta", "se_beta", "tau", "F_wald", "p_wald")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def pinned_copy(G):
    """The same values in the same memory order in lmm.pinned_empty memory (F order: the transpose of a pinned (p, n) array)."""
    from pygemma_amd import lmm
    if isinstance(G, PackedBed):
        return PackedBed(pinned_copy(G.data), G.n, count_A1=G.count_A1)
    snp_major = G.flags.f_contiguous and not G.flags.c_contiguous
    P = lmm.pinned_empty(G.shape[::-1] if snp_major else G.shape, G.dtype)
    P[:] = G.T if snp_major else G
    return P.T if snp_major else P


def strided_pinned(bed):
    """The bed's records as a column slice of a wider pinned array."""
    from pygemma_amd import lmm
    wide = lmm.pinned_empty((bed.p, bed.data.shape[1] + 5), np.uint8)
    wide[:] = 0xff
    wide[:, :bed.data.shape[1]] = bed.data
    return PackedBed(wide[:, :bed.data.shape[1]], bed.n, count_A1=bed.count_A1)


@functools.lru_cache(maxsize=None)
def source(kind, n, p):
    """(genotype source in ordinary memory, fp64 dosages with NaN for a missing call) of one kind."""
    if kind == "bed":
        D = make_dosages(n, p, 0.02, seed=n + p)
        return PackedBed(np.ascontiguousarray(_pack(D)), n), D         # (_pack's records come out strided at some n)
    rng = np.random.default_rng(n + p)
    D = rng.binomial(2, rng.uniform(0.05, 0.5, p), size=(n, p)).astype(np.float64)
    if kind.startswith("float32"):
        D += 0.25 * rng.standard_normal((n, p))                    # imputed dosages: a general float32 matrix
    G = D.astype(kind.split()[0])
    return (np.asfortranarray(G) if kind.endswith("F") else G), G.astype(np.float64)


@functools.lru_cache(maxsize=None)
def kinship_truth(kind, n, p):
    return truth(source(kind, n, p)[1])


@pytest.fixture
def puts(monkeypatch):
    """Records, for every window that travels, whether it was staged."""
    from pygemma_amd import _feed
    staged, put = [], _feed._put_window

    def spy(ctx, src, s, e, dst, dpitch=None, staging=None, **kw):
        staged.append(staging is not None)
        return put(ctx, src, s, e, dst, dpitch, staging, **kw)

    monkeypatch.setattr(_feed, "_put_window", spy)
    return staged


@pytest.mark.parametrize("kind", ["bed", "int8 C", "int8 F", "float32 C", "float32 F"])
def test_kinship_staged_and_direct_are_the_same_bits(kind, puts):
    from pygemma_amd import _feed, lmm
    n, p, pb = 257, 333, 64                                          # six batches, the last of 13 SNPs
    G, _ = source(kind, n, p)
    Gp = pinned_copy(G)
    assert _feed._describe(G).direct is False and _feed._describe(Gp).direct is True
    Ka = lmm.kinship(G, snp_batch=pb)
    assert puts == [True] * 6
    check_gate(Ka, kinship_truth(kind, n, p), p)
    del puts[:]
    Kb = lmm.kinship(Gp, snp_batch=pb)
    assert puts == [False] * 6
    assert same_bits(Ka, Kb)
    if kind == "bed":                                                # strided records are staged even from pinned memory
        Gs = strided_pinned(G)
        assert _feed._describe(Gs).direct is False and not Gs.data.flags.c_contiguous and lmm._lib.is_pinned(Gs.data)
        del puts[:]
        Ks = lmm.kinship(Gs, snp_batch=pb)
        assert puts == [True] * 6
        assert same_bits(Ka, Ks)


@pytest.mark.parametrize("pb,nbat", [(130, 1), (65, 2), (64, 3)])
@pytest.mark.parametrize("kind", ["bed", "int8 C"])
def test_kinship_batch_counts(kind, pb, nbat, puts):
    from pygemma_amd import lmm
    n, p = 257, 130
    G, _ = source(kind, n, p)
    for X in (G, pinned_copy(G)):
        del puts[:]
        K = lmm.kinship(X, snp_batch=pb)
        assert len(puts) == nbat
        check_gate(K, kinship_truth(kind, n, p), p)


@pytest.mark.parametrize("kind", ["float32 C", "float32 F", "int8 C", "bed"])
def test_linear_model_is_the_same_bits_however_the_batches_travel(kind, puts):
    from pygemma_amd import _feed, lmm
    n, c, t, p = 203, 3, 2, 333
    rng = np.random.default_rng(7)
    X, D = source(kind, n, p)
    W = np.concatenate([np.ones((n, 1)), rng.standard_normal((n, c - 1))], axis=1).astype(np.float32)
    Y = (rng.standard_normal((n, t)) + 0.2 * np.nan_to_num(D[:, 5:8], nan=1.0) @ rng.standard_normal((3, t))).astype(np.float32)
    row_bytes = (n + 3) // 4 if kind == "bed" else n * X.itemsize
    ref = None
    for Xk, direct in ((X, False), (pinned_copy(X), True)):
        assert _feed._describe(Xk).direct is direct
        for sb, nbat in ((64, 6), (None, 1)):
            st = {}
            del puts[:]
            fr = lmm.pygemma_lm(Y, Xk, W, snp_batch=sb, stats=st)
            assert puts == [not direct] * nbat
            assert st["batches"] == nbat and st["bytes_in"] == p * row_bytes
            assert list(fr) == [0, 1]
            ref = ref or fr
            for k in range(t):
                assert np.isfinite(fr[k]["F_wald"].to_numpy()[8:]).all()
                for col in LM_COLS:
                    assert same_bits(fr[k][col].to_numpy(), ref[k][col].to_numpy()), (direct, sb, k, col)


def test_pageable_eigenvectors_travel_in_panels(monkeypatch, puts):
    import scipy.linalg
    from pygemma_amd import lmm, synth
    n, p, c = 300, 64, 2
    raw = synth.panel(n, p, c, seed=3)
    d, U = scipy.linalg.eigh(raw["K"].astype(np.float64))
    U = np.ascontiguousarray(U, np.float32)
    Up = lmm.pinned_empty((n, n), np.float32)
    Up[:] = U
    monkeypatch.setattr(lmm, "_U_PANEL_BYTES", 128 * n * 4)          # panels of 128, 128 and 44 rows
    a = lmm.pygemma(raw["Y"], raw["X"], raw["W"], None, eigenpairs=(d, U))
    assert puts == [True] * 3                                        # (the scan's batches do not go through the ring)
    del puts[:]
    b = lmm.pygemma(raw["Y"], raw["X"], raw["W"], None, eigenpairs=(d, Up))      # one DMA out of the pinned array
    assert puts == []
    assert np.isfinite(a["F_wald"].to_numpy()).all()
    for col in a.columns:
        assert same_bits(a[col].to_numpy(), b[col].to_numpy()), col


def test_a_consumer_that_raises_leaves_the_device_usable():
    import contextlib
    from pygemma_amd import _feed, _lib, lmm
    n, p, pb = 257, 250, 64                                          # four batches
    G, _ = source("int8 C", n, p)
    K0 = lmm.kinship(G, snp_batch=pb)
    seen = []
    with _lib.Context(0) as ctx:
        with pytest.raises(RuntimeError, match="consumer failed"):
            with contextlib.closing(_feed._Feed(ctx, _feed._describe(G))) as feed:
                for s, e, slot in feed.batches(pb):
                    seen.append((s, e))
                    if len(seen) == 3:                               # a Python exception only: nothing is launched
                        raise RuntimeError("consumer failed")
        assert seen == [(0, 64), (64, 128), (128, 192)]
        assert ctx._bufs == []                                       # the slots went with the feed
    K1 = lmm.kinship(G, snp_batch=pb)
    assert same_bits(K0, K1)
