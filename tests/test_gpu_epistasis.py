"""GPU checks of the epistasis kernels (pg_epi_split_dev, pg_epi_block_dev) and of lmm.epistasis — run with -m gpu on an MI355X.

The truth is tests/_epi_truth.py.  The eight sums of a pair are integers and are compared for EQUALITY, and so are the hit count, n_tot,
n_sig and best.  z goes through two fp64 logarithms, which the device's math library and NumPy round differently: the bound is
|z - z_truth| <= 1e-11 + 1e-14 |z|.  At n <= 1030 the cell products are exact in fp64 and their ratio is one rounding, log is within
1 ulp on both sides (the device library's documented bound), L of a group is at most log(4 n^2) < 16 so an ulp of it is 1.8e-15, and
1 / sqrt(v) <= sqrt(n / 2) = 23: a few 1e-13 in all, and the bound is that with a margin of 20.  No truth pair may lie within 1e-9 of
the chi2 cut, so that the hit SETS are equal, not just close.

Shapes: n in {1, 3, 63, 65, 129, 1030}, p in {19, 65, 129, 257, 300, 515} (across the 32-, 64-, 128- and 256-SNP edges of the two tile
geometries), missing rates 0 and 0.07, both paths (PG_EPI_PLANES), .bed, int8 and float64 sources.  For n >= 63 fewer than 20 % of the
visited pairs may be undefined and the hits are between 1 % and 20 % of the defined pairs, so that a kernel that reports nothing cannot
pass; n = 1 and n = 3 rest on equality alone."""
import functools
import os

import numpy as np
import pytest

import _epi_truth as E
import _ld_truth as T

pytestmark = pytest.mark.gpu

GUARD = 4          # 32-bit words (hit records, 64-bit words) before and after every output
EINVAL, ENOTSUP = -22, -95
CUT = 3.84
HIT = np.dtype([("a", "<i4"), ("b", "<i4"), ("z", "<f8")])


def z_close(z, want):
    return np.abs(z - want) <= 1e-11 + 1e-14 * np.abs(want)


@pytest.fixture(scope="module")
def ctx():
    from pygemma_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def panel(n, p, seed, miss, specials):
    G = T.ld_panel(n, p, seed, miss=miss, specials=specials)
    G.setflags(write=False)
    return G


@functools.lru_cache(maxsize=None)
def groups(n, seed):
    g = E.group_vector(n, seed)
    if n >= 3:
        g[0], g[1], g[2] = 1, 0, -1
    g.setflags(write=False)
    return g


def new_image(ctx, G, pe, group, kind="f64"):
    """The epistasis image for pe SNPs of a panel encoded from a source of `kind` at positions [0, p); every byte of both images is
    garbage before, so the positions [p, pe) still are."""
    from pygemma_amd import _lib
    L = _lib.load()
    n, p = G.shape
    ld_bytes, epi_bytes = int(L.pg_ld_image_bytes(n, pe)), int(L.pg_epi_image_bytes(n, pe))
    assert ld_bytes > 0 and epi_bytes > 0
    ldim, image = ctx.alloc(ld_bytes), ctx.alloc(epi_bytes)
    _lib.check(L.pg_memset(ctx.handle, ldim.ptr, 0x7f, ld_bytes), "pg_memset")
    _lib.check(L.pg_memset(ctx.handle, image.ptr, 0x7f, epi_bytes), "pg_memset")
    if kind == "bed":
        dX = ctx.to_device(T.pack(T.bed_view(G)))
        _lib.check(L.pg_ld_encode_bed_dev(ctx.handle, n, p, dX.ptr, (n + 3) // 4, 0, ldim.ptr, pe, 0), "pg_ld_encode_bed_dev")
    elif kind == "int8":
        assert np.isfinite(G).all() and (G == np.round(G)).all()
        dX = ctx.to_device(np.ascontiguousarray(G.astype(np.int8)))
        _lib.check(L.pg_ld_encode_x_dev(ctx.handle, n, p, dX.ptr, 0, p, 0, ldim.ptr, pe, 0), "pg_ld_encode_x_dev")
    else:
        dX = ctx.to_device(np.ascontiguousarray(G, np.float64))
        _lib.check(L.pg_ld_encode_x_dev(ctx.handle, n, p, dX.ptr, 3, p, 0, ldim.ptr, pe, 0), "pg_ld_encode_x_dev")
    dg = ctx.to_device(np.asarray(group, np.int8))
    split = p // 3                   # in two calls: the totals and the header do not depend on how the SNPs are cut
    _lib.check(L.pg_epi_split_dev(ctx.handle, n, ldim.ptr, pe, split, p - split, dg.ptr, image.ptr), "pg_epi_split_dev")
    _lib.check(L.pg_epi_split_dev(ctx.handle, n, ldim.ptr, pe, 0, split, dg.ptr, image.ptr), "pg_epi_split_dev")
    ctx.sync()
    for buf in (dX, dg, ldim):
        buf.free()
    return image


def test_dtype_codes():
    """new_image passes dtype codes 0 (int8) and 3 (float64): what lmm's own description of such arrays says."""
    from pygemma_amd._feed import _describe
    assert _describe(np.zeros((4, 3), np.int8)).dtype_code == 0 and _describe(np.zeros((4, 3), np.float64)).dtype_code == 3


class Outputs:
    """Every output of pg_epi_block_dev on the device, preset to a pattern, between guard words."""

    def __init__(self, ctx, size, cap, na, nb):
        i = np.arange(size + 2 * GUARD, dtype=np.int64)
        self.ctx, self.size, self.cap = ctx, size, cap
        best = np.zeros(size + 2 * GUARD, np.uint64)
        best[:GUARD] = best[-GUARD:] = 0xfeedfeedfeedfeed
        hits = np.zeros(cap + 2 * GUARD, HIT)
        hits["a"], hits["b"], hits["z"] = -7, -9, 1e300
        count = np.array([77] * GUARD + [0] + [77] * GUARD, np.uint64)
        sums = -1000 - np.arange(na * nb * 8 + 2 * GUARD, dtype=np.int32)
        self.host = dict(count=count, hits=hits, n_tot=(3 + i).astype(np.int32), n_sig=(-5 - i).astype(np.int32), best=best, sums=sums)
        self.dev = {k: ctx.to_device(h) for k, h in self.host.items()}

    def ptr(self, k):
        return self.dev[k].ptr + GUARD * self.host[k].itemsize

    def read(self):
        """The outputs as they are now, the guard words checked: count, the hit records, what was added to n_tot and n_sig, best, sums."""
        now = {k: d.download(self.host[k].shape, self.host[k].dtype) for k, d in self.dev.items()}
        for k, a in now.items():
            h = self.host[k]
            assert (a[:GUARD] == h[:GUARD]).all() and (a[-GUARD:] == h[-GUARD:]).all(), f"a guard word of {k} was written"
        inner = lambda k: now[k][GUARD:len(now[k]) - GUARD]
        was = lambda k: self.host[k][GUARD:len(self.host[k]) - GUARD]
        return SimpleOutputs(int(inner("count")[0]), inner("hits"), inner("n_tot").astype(np.int64) - was("n_tot"),
                             inner("n_sig").astype(np.int64) - was("n_sig"), inner("best"), inner("sums"), was("sums"), was("hits"))

    def untouched(self):
        return all((d.download(self.host[k].shape, self.host[k].dtype) == self.host[k]).all() for k, d in self.dev.items())

    def free(self):
        for d in self.dev.values():
            d.free()


class SimpleOutputs:
    def __init__(self, count, hits, n_tot, n_sig, best, sums, sums_before, hits_before):
        self.count, self.hits, self.n_tot, self.n_sig, self.best = count, hits, n_tot, n_sig, best
        self.sums, self.sums_before, self.hits_before = sums, sums_before, hits_before


def run_block(ctx, n, imA, pea, a0, na, ga0, imB, peb, b0, nb, gb0, mode, upper, cut, out, planes="", cap=None, with_sums=True):
    from pygemma_amd import _lib
    L = _lib.load()
    old = os.environ.get("PG_EPI_PLANES")
    os.environ["PG_EPI_PLANES"] = planes
    try:
        _lib.check(L.pg_epi_block_dev(ctx.handle, n, imA.ptr, pea, a0, na, ga0, imB.ptr, peb, b0, nb, gb0, mode, upper, cut, out.ptr("count"),
                                      out.ptr("hits"), out.cap if cap is None else cap, out.ptr("n_tot"), out.ptr("n_sig"), out.ptr("best"),
                                      out.ptr("sums") if with_sums else None), "pg_epi_block_dev")
        ctx.sync()
    finally:
        if old is None:
            del os.environ["PG_EPI_PLANES"]
        else:
            os.environ["PG_EPI_PLANES"] = old


def geometry(p, window):
    """(pB or None for the same image, pea, a0, na, ga0, peb, b0, nb, gb0, upper) of a window kind."""
    if window == "full":                 # one image against itself, every ordered pair (self pairs too)
        return None, p + 4, 0, p, 0, p + 4, 0, p, 0, 0
    if window == "upper":                # one image, two windows that straddle the diagonal, pairs a < b only
        return None, p + 4, 2, p - 5, 2, p + 4, 1, p - 1, 1, 1
    pB = p // 2 + 7                      # interior windows of two images, global indices that are not image positions
    return pB, p + 3, 3, p - 7, 10, pB + 2, 2, pB - 5, 10 + p, 0


def truth_block(n, p, miss, specials, window, mode, cut=CUT):
    """What pg_epi_block_dev must produce for a case: the panels, the group, the geometry and the truth of its window."""
    GA, g = panel(n, p, n + p, miss, specials), groups(n, n + 3 * p)
    pB, pea, a0, na, ga0, peb, b0, nb, gb0, upper = geometry(p, window)
    GB = GA if pB is None else panel(n, pB, n + p + 1, miss, False)
    S = E.sums(GA, g, None if pB is None else GB)[a0:a0 + na, b0:b0 + nb]
    ga, gb = ga0 + np.arange(na), gb0 + np.arange(nb)
    visit = (ga[:, None] < gb[None, :]) if upper else np.ones((na, nb), bool)
    ok, z = E.z_of(S, case_only=mode == 1)
    size = int(max(ga.max(), gb.max())) + 1
    hits, n_tot, n_sig, best = E.summary(ok, z, visit, cut, ga, gb, size)
    return dict(GA=GA, GB=GB, g=g, geom=(pea, a0, na, ga0, peb, b0, nb, gb0, upper), same=pB is None, S=S, visit=visit, ok=ok, z=z, size=size,
                hits=hits, n_tot=n_tot, n_sig=n_sig, best=best, near=E.near_cut(ok, z, visit, cut))


def conditions(n, t):
    """The panel can tell a kernel that reports nothing."""
    visited, defined = int(t["visit"].sum()), int((t["ok"] & t["visit"]).sum())
    assert visited > 0 and t["near"] == 0, "a truth pair lies within 1e-9 of the cut: move the cut"
    if n >= 63:
        assert 1 - defined / visited < 0.2, f"{1 - defined / visited:.0%} of the visited pairs are undefined"
        assert 0.01 <= len(t["hits"]) / defined <= 0.2, f"{len(t['hits']) / defined:.1%} of the defined pairs are hits"


def check_hits(records, want):
    """The records, sorted, are the truth's pairs with z inside the bound.  Returns the largest |z - z_truth|."""
    got = sorted(zip(records["a"].tolist(), records["b"].tolist(), records["z"].tolist()))
    assert [h[:2] for h in got] == [h[:2] for h in want], "the hit pairs differ from the truth's"
    if not got:
        return 0.0
    zg, zw = np.array([h[2] for h in got]), np.array([h[2] for h in want])
    assert z_close(zg, zw).all(), f"z differs from the truth by up to {np.abs(zg - zw).max():.3e}"
    return float(np.abs(zg - zw).max())


# n, p, missing calls, the special columns, PG_EPI_PLANES, source, window, mode
CASES = [(1030, 257, 0.07, True, "", "bed", "full", 0), (1030, 257, 0.0, False, "", "int8", "upper", 0), (1030, 300, 0.0, False, "1", "f64", "interior", 0),
         (129, 515, 0.07, True, "", "f64", "upper", 0), (129, 515, 0.0, False, "", "bed", "full", 1), (129, 515, 0.0, False, "1", "int8", "upper", 0),
         (129, 515, 0.0, True, "", "f64", "full", 0), (129, 300, 0.07, True, "", "bed", "interior", 1), (65, 300, 0.07, True, "1", "f64", "full", 0),
         (65, 257, 0.0, False, "", "int8", "interior", 0), (65, 129, 0.07, True, "", "bed", "upper", 0), (63, 129, 0.0, False, "", "f64", "full", 0),
         (63, 65, 0.07, False, "", "bed", "full", 1), (63, 65, 0.0, False, "1", "int8", "upper", 0), (63, 19, 0.07, False, "", "f64", "full", 0),
         (3, 19, 0.07, False, "", "bed", "full", 0), (3, 65, 0.0, False, "", "int8", "upper", 1), (1, 19, 0.0, False, "", "f64", "full", 1),
         (1, 19, 0.07, False, "1", "bed", "upper", 0)]


@pytest.mark.parametrize("n,p,miss,specials,planes,kind,window,mode", CASES,
                         ids=[f"n{c[0]}-p{c[1]}-miss{c[2]}-sp{int(c[3])}-planes{c[4]}-{c[5]}-{c[6]}-mode{c[7]}" for c in CASES])
def test_block_is_the_host_model(ctx, n, p, miss, specials, planes, kind, window, mode):
    t = truth_block(n, p, miss, specials, window, mode)
    conditions(n, t)
    pea, a0, na, ga0, peb, b0, nb, gb0, upper = t["geom"]
    imA = new_image(ctx, t["GA"], pea, t["g"], kind)
    imB = imA if t["same"] else new_image(ctx, t["GB"], peb, t["g"], "f64" if kind == "int8" and miss > 0 else kind)
    out = Outputs(ctx, t["size"], len(t["hits"]) + 3, na, nb)
    run_block(ctx, n, imA, pea, a0, na, ga0, imB, peb, b0, nb, gb0, mode, upper, CUT, out, planes)
    r = out.read()
    sums = r.sums.reshape(na, nb, 8)
    assert (sums[t["visit"]] == t["S"][t["visit"]]).all(), "the sums differ from the integer truth"
    assert (sums[~t["visit"]] == r.sums_before.reshape(na, nb, 8)[~t["visit"]]).all(), "sums of a pair that is not visited were written"
    assert r.count == len(t["hits"]), "the hit count differs from the truth's"
    worst = check_hits(r.hits[:r.count], t["hits"])
    print(f"n={n} p={p} {window}: {len(t['hits'])} hits of {int((t['ok'] & t['visit']).sum())} defined pairs, max |z - z_truth| = {worst:.3e}")
    assert (r.hits[r.count:] == r.hits_before[r.count:]).all(), "a record past the counter was written"
    assert (r.n_tot == t["n_tot"]).all() and (r.n_sig == t["n_sig"]).all(), "n_tot or n_sig differs from the truth"
    assert (r.best == t["best"]).all(), "best differs from the truth"
    out.free(); imA.free()
    if not t["same"]:
        imB.free()


@pytest.mark.parametrize("planes", ["", "1"])
def test_one_group_only(ctx, planes):
    """Every sample a case: no pair is defined for the case/control test, the case-only test sees them all."""
    n, p = 65, 129
    G = panel(n, p, 5, 0.07 if planes else 0.0, False)
    g = np.ones(n, np.int8)
    S = E.sums(G, g)
    image = new_image(ctx, G, p, g)
    out = Outputs(ctx, p, 16, p, p)
    run_block(ctx, n, image, p, 0, p, 0, image, p, 0, p, 0, 0, 1, CUT, out, planes)
    r = out.read()
    assert r.count == 0 and (r.n_tot == 0).all() and (r.n_sig == 0).all() and (r.best == 0).all() and (r.hits == r.hits_before).all()
    upper = np.triu(np.ones((p, p), bool), 1)
    assert (r.sums.reshape(p, p, 8)[upper] == S[upper]).all() and (S[..., 4:] == 0).all()
    out.free()
    ok, z = E.z_of(S, case_only=True)
    hits, n_tot, n_sig, best = E.summary(ok, z, upper, CUT, np.arange(p), np.arange(p), p)
    assert (ok & upper).sum() > 0.8 * upper.sum() and len(hits) > 10 and E.near_cut(ok, z, upper, CUT) == 0
    out = Outputs(ctx, p, len(hits), p, p)
    run_block(ctx, n, image, p, 0, p, 0, image, p, 0, p, 0, 1, 1, CUT, out, planes, with_sums=False)
    r = out.read()
    assert r.count == len(hits) and (r.n_tot == n_tot).all() and (r.n_sig == n_sig).all() and (r.best == best).all()
    check_hits(r.hits[:r.count], hits)
    assert (r.sums == r.sums_before).all()
    out.free(); image.free()


def test_cap_smaller_than_the_hit_count(ctx):
    """The counter counts every hit; records are written below cap only, each of them a true hit, no pair twice."""
    n, p = 129, 300
    t = truth_block(n, p, 0.07, True, "upper", 0)
    pea, a0, na, ga0, peb, b0, nb, gb0, upper = t["geom"]
    image = new_image(ctx, t["GA"], pea, t["g"])
    cap = len(t["hits"]) // 3
    assert cap > 10
    out = Outputs(ctx, t["size"], cap + 50, na, nb)              # the buffer is larger than the cap the kernel is told
    run_block(ctx, n, image, pea, a0, na, ga0, image, peb, b0, nb, gb0, 0, upper, CUT, out, cap=cap, with_sums=False)
    r = out.read()
    assert r.count == len(t["hits"]) and (r.n_tot == t["n_tot"]).all() and (r.n_sig == t["n_sig"]).all() and (r.best == t["best"]).all()
    assert (r.hits[cap:] == r.hits_before[cap:]).all(), "a record at or past cap was written"
    want = {h[:2]: h[2] for h in t["hits"]}
    got = [(int(h["a"]), int(h["b"])) for h in r.hits[:cap]]
    assert len(set(got)) == cap and all(k in want for k in got)
    assert z_close(r.hits[:cap]["z"], np.array([want[k] for k in got])).all()
    out.free()
    out = Outputs(ctx, t["size"], 4, na, nb)                       # cap = 0 and no buffer at all: the count alone
    from pygemma_amd import _lib
    L = _lib.load()
    _lib.check(L.pg_epi_block_dev(ctx.handle, n, image.ptr, pea, a0, na, ga0, image.ptr, peb, b0, nb, gb0, 0, upper, CUT, out.ptr("count"), None, 0,
                                  None, None, None, None), "pg_epi_block_dev")
    ctx.sync()
    r = out.read()
    assert r.count == len(t["hits"]) and (r.hits == r.hits_before).all() and (r.n_tot == 0).all() and (r.best == 0).all()
    out.free(); image.free()


def test_upper_reports_each_pair_once(ctx):
    """Windows cut anywhere: the upper-triangle calls over a 3 x 3 grid of windows of one image report every pair a < b exactly once and
    none with a >= b, also from the windows below the diagonal (which hold none) and those that straddle it."""
    n, p = 129, 300
    G, g = panel(n, p, n + p, 0.07, True), groups(n, n + 3 * p)
    S = E.sums(G, g)
    ok, z = E.z_of(S)
    upper = np.triu(np.ones((p, p), bool), 1)
    hits, n_tot, n_sig, best = E.summary(ok, z, upper, CUT, np.arange(p), np.arange(p), p)
    image = new_image(ctx, G, p, g)
    out = Outputs(ctx, p, len(hits) + 1, 1, 1)
    edges_a, edges_b = [0, 70, 200, p], [0, 130, 131, p]
    from pygemma_amd import _lib
    L = _lib.load()
    found, total = [], 0
    for a0, a1 in zip(edges_a, edges_a[1:]):
        for b0, b1 in zip(edges_b, edges_b[1:]):
            _lib.check(L.pg_memset(ctx.handle, out.ptr("count"), 0, 8), "pg_memset")
            run_block(ctx, n, image, p, a0, a1 - a0, a0, image, p, b0, b1 - b0, b0, 0, 1, CUT, out, with_sums=False)
            count = int(out.dev["count"].download((2 * GUARD + 1,), np.uint64)[GUARD])
            found.append(out.dev["hits"].download((out.cap + 2 * GUARD,), HIT)[GUARD:GUARD + count])
            total += count
    rec = np.concatenate(found)
    assert total == len(hits) and (rec["a"] < rec["b"]).all()
    check_hits(rec, hits)
    r = out.read()
    assert (r.n_tot == n_tot).all() and (r.n_sig == n_sig).all() and (r.best == best).all()
    out.free(); image.free()


def test_refused_calls_enqueue_nothing(ctx):
    from pygemma_amd import _lib
    L = _lib.load()
    n, p = 65, 65
    G, g = panel(n, p, 1, 0.07, False), groups(n, 2)
    image = new_image(ctx, G, p, g)
    out = Outputs(ctx, p, 8, p, p)
    good = dict(n=n, A=image.ptr, pea=p, a0=0, na=p, ga0=0, B=image.ptr, peb=p, b0=0, nb=p, gb0=0, mode=0, upper=1, cut=CUT, count=out.ptr("count"),
                hits=out.ptr("hits"), cap=8, n_tot=out.ptr("n_tot"), n_sig=out.ptr("n_sig"), best=out.ptr("best"), sums=out.ptr("sums"))
    order = list(good)
    bad = {"NULL A": dict(A=None), "NULL B": dict(B=None), "NULL count": dict(count=None), "NULL hits": dict(hits=None), "cap < 0": dict(cap=-1),
           "chi2_min < 0": dict(cut=-0.5), "chi2_min NaN": dict(cut=float("nan")), "chi2_min inf": dict(cut=float("inf")),
           "A off 16 bytes": dict(A=image.ptr + 8), "hits off 16 bytes": dict(hits=out.ptr("hits") + 8), "count off 8": dict(count=out.ptr("count") + 4),
           "best off 8": dict(best=out.ptr("best") + 4), "window beyond A": dict(a0=1), "window beyond B": dict(nb=p + 1), "a0 < 0": dict(a0=-1, na=1),
           "na < 0": dict(na=-1), "ga0 < 0": dict(ga0=-1), "gb0 at 2^31": dict(gb0=2 ** 31 - 1), "n = 0": dict(n=0), "n = 2^28": dict(n=1 << 28),
           "pea = 0": dict(pea=0, na=0)}
    for name, change in bad.items():
        a = dict(good, **change)
        assert L.pg_epi_block_dev(ctx.handle, *[a[k] for k in order]) == EINVAL and "pg_epi_block_dev" in L.pg_last_error().decode(), name
    for mode in (2, -1):
        assert L.pg_epi_block_dev(ctx.handle, *[dict(good, mode=mode)[k] for k in order]) == ENOTSUP and "mode" in L.pg_last_error().decode()
    assert L.pg_epi_block_dev(None, *[good[k] for k in order]) == EINVAL
    ctx.sync()
    assert out.untouched()
    # the split: refused calls leave the image as it is
    ld_bytes, epi_bytes = int(L.pg_ld_image_bytes(n, p)), int(L.pg_epi_image_bytes(n, p))
    ldim = ctx.alloc(ld_bytes)
    _lib.check(L.pg_memset(ctx.handle, ldim.ptr, 0, ld_bytes), "pg_memset")
    dg = ctx.to_device(g)
    before = image.download((epi_bytes,), np.uint8)
    sgood = dict(n=n, ld=ldim.ptr, pe=p, frm=0, count=p, group=dg.ptr, epi=image.ptr)
    sbad = {"NULL ld": dict(ld=None), "NULL group": dict(group=None), "NULL image": dict(epi=None), "off 16 bytes": dict(epi=image.ptr + 4),
            "beyond pe": dict(frm=1), "from < 0": dict(frm=-1), "count < 0": dict(count=-1), "n = 0": dict(n=0), "n = 2^28": dict(n=1 << 28)}
    for name, change in sbad.items():
        a = dict(sgood, **change)
        assert L.pg_epi_split_dev(ctx.handle, *[a[k] for k in sgood]) == EINVAL and "pg_epi_split_dev" in L.pg_last_error().decode(), name
    assert L.pg_epi_split_dev(ctx.handle, n, ldim.ptr, p, 3, 0, dg.ptr, image.ptr) == 0          # no SNPs: nothing to do
    ctx.sync()
    assert (image.download((epi_bytes,), np.uint8) == before).all()
    assert L.pg_epi_block_dev(ctx.handle, *[dict(good, na=0)[k] for k in order]) == 0                # an empty window: nothing to do
    ctx.sync()
    assert out.untouched()
    out.free(); image.free(); ldim.free(); dg.free()


# ---- lmm.epistasis ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scan_case(miss):
    """(n, p, panel, y, hits, n_tot, n_sig, best) of an all-pairs scan at the cut.  Without missing calls the panel is one every source
    kind can hold."""
    n, p = 129, 300
    G = np.array(T.ld_panel(n, p, 41, miss=miss, specials=miss > 0))
    if miss == 0:
        G[:, 100] = 2.0                                  # a monomorphic column
    G.setflags(write=False)
    g = groups(n, 17)
    y = np.where(g == 1, 1.0, np.where(g == 0, 0.0, np.nan))
    ok, z = E.z_of(E.sums(G, g))
    upper = np.triu(np.ones((p, p), bool), 1)
    assert E.near_cut(ok, z, upper, CUT) == 0
    return (n, p, G, y) + E.summary(ok, z, upper, CUT, np.arange(p), np.arange(p), p)


def same_result(r, s):
    cols = lambda df: all((df[0][c].to_numpy() == df[1][c].to_numpy()).all() for c in df[0].columns if c != "best_chi2")
    return (len(r.pairs) == len(s.pairs) and cols((r.pairs, s.pairs)) and cols((r.summary, s.summary)) and r.chi2_min == s.chi2_min
            and np.array_equal(r.summary["best_chi2"].to_numpy(), s.summary["best_chi2"].to_numpy(), equal_nan=True))


def check_result(res, p, hits, n_tot, n_sig, best):
    df, sm = res.pairs, res.summary
    assert list(df.columns) == ["i", "j", "z", "chi2", "p"] and list(sm.columns) == ["snp", "n_tot", "n_sig", "best_chi2", "best_partner"]
    assert list(zip(df["i"].tolist(), df["j"].tolist())) == [h[:2] for h in hits] and len(hits) > 100
    want = np.array([h[2] for h in hits])
    assert z_close(df["z"].to_numpy(), want).all()
    assert (df["chi2"].to_numpy() == df["z"].to_numpy() ** 2).all() and np.allclose(df["p"].to_numpy(), E.p_of(want), rtol=1e-9, atol=0)
    assert (sm["snp"] == np.arange(p)).all() and (sm["n_tot"] == n_tot).all() and (sm["n_sig"] == n_sig).all()
    some = n_tot > 0
    assert some.sum() >= p - 3 and (sm["best_partner"].to_numpy()[~some] == -1).all() and np.isnan(sm["best_chi2"].to_numpy()[~some]).all()
    assert (sm["best_chi2"].to_numpy()[some].view(np.uint32) == (best[some] >> np.uint64(32)).astype(np.uint32)).all()
    assert (sm["best_partner"].to_numpy()[some] == (~best[some] & np.uint64(0xffffffff)).astype(np.int64)).all()


def test_epistasis_is_the_host_model_whatever_the_batches():
    from pygemma_amd import lmm
    n, p, G, y, hits, n_tot, n_sig, best = scan_case(0.07)
    X = G.astype(np.float32)
    stats = {}
    results = [lmm.epistasis(X, y, chi2=CUT, snp_batch=sb, stats=stats) for sb in (64, 100, p)]
    assert stats["blocks"] == 1 and stats["reruns"] == 0 and stats["bytes_in"] == X.nbytes and stats["pairs_defined"] == n_tot.sum() // 2
    check_result(results[0], p, hits, n_tot, n_sig, best)
    for other in results[1:]:
        assert same_result(results[0], other), "the result depends on the block boundaries"
    assert results[0].chi2_min == CUT and lmm.epistasis(X, y, p=0.05, snp_batch=128).chi2_min == lmm._epi_chi2_min(0.05, None)


def test_epistasis_does_not_depend_on_the_storage():
    from pygemma_amd import lmm
    from pygemma_amd.bed import PackedBed
    n, p, G, y, hits, n_tot, n_sig, best = scan_case(0.0)
    base = lmm.epistasis(G, y, chi2=CUT)
    check_result(base, p, hits, n_tot, n_sig, best)
    for Xs in (PackedBed(T.pack(G), n), G.astype(np.int8), np.asfortranarray(G.astype(np.uint8)), G.astype(np.float32), np.asfortranarray(G)):
        assert same_result(base, lmm.epistasis(Xs, y, chi2=CUT, snp_batch=130))
    n, p, G, y, hits, n_tot, n_sig, best = scan_case(0.07)                    # missing calls: packed records and floats
    base = lmm.epistasis(G, y, chi2=CUT)
    assert same_result(base, lmm.epistasis(PackedBed(T.pack(T.bed_view(G)), n), y, chi2=CUT, snp_batch=77))
    assert same_result(base, lmm.epistasis(np.asfortranarray(G.astype(np.float32)), y, chi2=CUT))


def test_set_by_set_is_the_matching_rows_of_all_pairs():
    from pygemma_amd import lmm
    n, p, G, y, hits, _, _, _ = scan_case(0.07)
    X = G.astype(np.float32)
    full = lmm.epistasis(X, y, chi2=CUT).pairs
    a, b = np.arange(5, 140), np.array([3, 150, 151, 299, 200, 288])
    amask = np.zeros(p, bool)
    amask[a] = True
    for snp_batch in (None, 64):
        res = lmm.epistasis(X, y, a=amask, b=b, chi2=CUT, snp_batch=snp_batch)
        got = {(min(i, j), max(i, j)): z for i, j, z in zip(res.pairs["i"].tolist(), res.pairs["j"].tolist(), res.pairs["z"].tolist())}
        assert len(got) == len(res.pairs) and all(i in a and j in b for i, j in zip(res.pairs["i"], res.pairs["j"]))
        want = {(i, j): z for i, j, z in zip(full["i"].tolist(), full["j"].tolist(), full["z"].tolist())
                if (i in a and j in b) or (j in a and i in b)}
        assert got == want and len(want) > 20, "set-by-set differs from the all-pairs rows, bit for bit"
        assert list(res.summary["snp"]) == list(a) + list(b) and res.summary["n_sig"].sum() == 2 * len(want)
    within = lmm.epistasis(X, y, a=a, chi2=CUT).pairs                          # `a` alone: the pairs within the selection
    want = [(i, j) for i, j in zip(full["i"].tolist(), full["j"].tolist()) if i in a and j in a]
    assert list(zip(within["i"].tolist(), within["j"].tolist())) == want


def test_an_overflowing_block_is_rerun(monkeypatch):
    from pygemma_amd import lmm
    n, p, G, y, hits, n_tot, n_sig, best = scan_case(0.07)
    X = G.astype(np.float32)
    base = lmm.epistasis(X, y, chi2=CUT, snp_batch=100)
    monkeypatch.setenv("PYGEMMA_EPI_CAP", "7")
    stats = {}
    small = lmm.epistasis(X, y, chi2=CUT, snp_batch=100, stats=stats)
    assert stats["reruns"] >= 3 and stats["blocks"] == 6
    assert same_result(base, small)
    check_result(small, p, hits, n_tot, n_sig, best)


def test_a_planted_interaction_is_the_top_pair():
    """Case probability 0.95 when x_3 + x_40 >= 3, else 0.35.  With 0.8 against 0.45 the truth ranks an LD neighbour of SNP 40 first for
    two of three phenotype seeds (chi2 10.9 against 10.9: columns 41 - 43 of the panel are nine-tenths copies of 40); with this effect the
    planted pair leads for every seed tried (chi2 34 - 36 against 28 at most)."""
    from pygemma_amd import lmm
    n, p = 1030, 65
    G = T.ld_panel(n, p, 2024, miss=0.02, specials=False)
    rng = np.random.default_rng(9)
    load = np.nan_to_num(G[:, 3]) + np.nan_to_num(G[:, 40])
    y = (rng.random(n) < np.where(load >= 3, 0.95, 0.35)).astype(np.float64)
    ok, z = E.z_of(E.sums(G, y.astype(np.int8)))
    chi2 = np.where(ok & np.triu(np.ones((p, p), bool), 1), z * z, 0.0)
    assert np.unravel_index(chi2.argmax(), chi2.shape) == (3, 40) and chi2[3, 40] > 15
    res = lmm.epistasis(G, y, p=1e-3)
    top = res.pairs.sort_values("chi2", ascending=False).iloc[0]
    assert (int(top["i"]), int(top["j"])) == (3, 40) and z_close(top["z"], z[3, 40])
    assert int(res.summary["best_partner"][3]) == 40 and int(res.summary["best_partner"][40]) == 3
