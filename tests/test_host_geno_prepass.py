"""CPU-only: the host's choice between the one-pass and the two-pass detect in front of the genotype rotation is a plain function of
the LDS a workgroup may use (pg_geno_onepass_max_n): 512 rows per layer of 32 x 33 tag words, next to 256 fixed words."""
import os


def _L():
    from pygemma_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return _lib.load()


def _need(n):
    return 4 * ((n + 511) // 512 * 1056 + 256)


def test_onepass_limit_follows_the_lds_size():
    L = _L()
    assert L.pg_geno_onepass_max_n(160 * 1024) == 38 * 512       # gfx950: n = 10 000 (20 layers, 85 504 bytes) fits
    assert L.pg_geno_onepass_max_n(64 * 1024) == 15 * 512
    assert _need(10000) == 85504 and L.pg_geno_onepass_max_n(85504) == 10240 and L.pg_geno_onepass_max_n(85503) == 9728
    for lds in (0, 1023, 1024, 5247):                            # not even one layer
        assert L.pg_geno_onepass_max_n(lds) == 0
    assert L.pg_geno_onepass_max_n(5248) == 512
    prev = 0
    for lds in range(0, 200 * 1024, 1000):
        n = L.pg_geno_onepass_max_n(lds)
        assert n >= prev and n % 512 == 0
        assert n == 0 or (_need(n) <= lds < _need(n + 1))
        prev = n


def test_onepass_limit_without_a_context_is_zero():
    assert _L().pg_geno_onepass_limit(None) == 0
