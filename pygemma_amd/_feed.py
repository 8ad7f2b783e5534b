"""Host -> device transport of genotype windows: pinned staging buffers (_Pinned), one window in one DMA (_put_window), what a
streamed consumer needs to know of its source (_describe) and how it calls its kernels on a batch of it (_call_dev), and the two-slot
feed every streamed entry point of lmm.py reads its SNP batches from (_Feed; its staging half, _Ring, also carries a pageable U)."""
import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib
from .bed import PackedBed

_STAGE_THREADS = 8       # host copy threads per worker for the pageable -> pinned leg
_KIN_DTYPES = {np.dtype(np.int8): 0, np.dtype(np.uint8): 1, np.dtype(np.float32): 2, np.dtype(np.float64): 3}   # PG_DTYPE_*


class _Pinned:
    """Pinned host buffers (hipHostMalloc through ctx), one per size in `sizes` (`.bufs`), freed together by close()."""

    def __init__(self, ctx, *sizes):
        self.ctx, self.bufs = ctx, []
        try:
            for nbytes in sizes:
                p = C.c_void_p()
                _lib.check(_lib.load().pg_host_alloc(ctx.handle, int(nbytes), C.byref(p)), "pg_host_alloc")
                self.bufs.append(p.value)
        except BaseException:
            self.close()
            raise

    def close(self):
        for q in self.bufs:
            _lib.load().pg_host_free(self.ctx.handle, q)
        self.bufs = []


def _put_window(ctx, src, s, e, dst, dpitch=None, staging=None, threads=_STAGE_THREADS):
    """SNPs [s, e) of a host source -> device address `dst`, in ONE DMA on ctx's stream.
    `src` is an (n, p) array in C order (sample-major: n rows of the window's e - s values, landing `dpitch` bytes apart), or one
    in F order or a PackedBed (SNP-major: e - s contiguous rows, one per SNP, landing back to back, or `dpitch` apart through a
    2-D DMA when it is given).  Without `staging` src is pinned and the DMA reads it.  Otherwise `threads` copy threads first
    gather the window into the pinned buffer `staging`: sample-major rows at `dpitch` (then the DMA is flat), SNP-major rows back
    to back.  Waiting until `staging` or `dst` is free again is the caller's business."""
    L = _lib.load()
    if isinstance(src, PackedBed):
        rec = np.ascontiguousarray(src.data[s:e])      # a view of the records, unless they are strided
        snp_major, ptr, spitch, width, rows = True, rec.ctypes.data, rec.shape[1], rec.shape[1], e - s
    elif src.flags.f_contiguous and not src.flags.c_contiguous:
        width = src.shape[0] * src.itemsize
        snp_major, ptr, spitch, rows = True, src.ctypes.data + s * width, width, e - s
    else:
        snp_major, ptr, spitch, width, rows = False, src.ctypes.data + s * src.itemsize, src.strides[0], (e - s) * src.itemsize, src.shape[0]
    if staging is not None:
        sp = width if snp_major else (dpitch or width)
        _lib.check(L.pg_stage_rows(staging, sp, ptr, spitch, width, rows, threads), "pg_stage_rows")
        ptr, spitch = staging, sp
    if dpitch is None or (staging is not None and not snp_major):     # the rows lie as they will on the device
        _lib.check(L.pg_memcpy_h2d_async(ctx.handle, dst, ptr, rows * (dpitch or width)), "pg_memcpy_h2d_async")
    else:
        _lib.check(L.pg_memcpy2d_h2d_async(ctx.handle, dst, dpitch, ptr, spitch, width, rows), "pg_memcpy2d_h2d_async")


def _genotypes(X, who, name="X", cast=False):
    """A raw genotype argument as the streamed paths read it: a PackedBed as it is; an array 2-D, int8, uint8, float32 or float64
    (another dtype is cast to float32 with `cast`, otherwise refused in the name of the entry point `who`) and C- or F-contiguous
    (anything else is copied to C order)."""
    if isinstance(X, PackedBed):
        return X
    X = np.asarray(X)
    if X.ndim != 2:
        raise ValueError(f"{name} must be a 2-D (n, p) array, not {X.ndim}-D")
    if X.dtype not in _KIN_DTYPES:
        if not cast:
            raise ValueError(f"{who} takes int8, uint8, float32 or float64 genotypes (or a PackedBed), not {X.dtype}")
        X = X.astype(np.float32)
    if not (X.flags.c_contiguous or X.flags.f_contiguous):
        X = np.ascontiguousarray(X)
    return X


# A genotype source as _genotypes leaves it (`src`), and what a streamed consumer reads off it: packed .bed records or an array;
# SNP-major (records, or Fortran order) or sample-major; bytes per element and per SNP (its record, or its column of n values);
# n, p; the PG_DTYPE_* code (None for packed); count_A1 (None for an array); and `direct`: the DMA may read the source itself
# (pinned memory, and records that are not strided), no staging copy
_Source = namedtuple("_Source", "src packed snp_major esz row_bytes n p dtype_code count_a1 direct")


def _describe(X):
    if isinstance(X, PackedBed):
        rec = X.data
        return _Source(X, True, True, 1, rec.shape[1], X.n, X.p, None, int(X.count_A1), bool(_lib.is_pinned(rec) and rec.flags.c_contiguous))
    n, p = X.shape
    snp_major = bool(X.flags.f_contiguous and not X.flags.c_contiguous)
    return _Source(X, False, snp_major, X.itemsize, n * X.itemsize, n, p, _KIN_DTYPES[X.dtype], None, _lib.is_pinned(X))


def _call_dev(L, stem, src, head, slot, pb, tail):
    """A streamed consumer's kernels on the `pb` SNPs of `src` at the device address `slot`: the entry point stem.format("bed") with
    (*head, slot, bytes per record, count_A1, *tail) for packed records, stem.format("x") with (*head, slot, PG_DTYPE_*, ld, snp_major,
    *tail) for an array, ld = n for SNP-major columns and pb for the column window of a sample-major block."""
    if src.packed:
        name, source = stem.format("bed"), (slot, src.row_bytes, src.count_a1)
    else:
        name, source = stem.format("x"), (slot, src.dtype_code, src.n if src.snp_major else pb, int(src.snp_major))
    _lib.check(getattr(L, name)(*head, *source, *tail), name)


def _event(ctx):
    ev = C.c_void_p()
    _lib.check(_lib.load().pg_event_create(ctx.handle, C.byref(ev)), "pg_event_create")
    return ev


class _Ring:
    """Uploads on ctx's stream that take turns through two pinned staging buffers of `nbytes` (`staged`; without, the source is
    pinned and the DMAs read it), each with the event of its last DMA (`.events`): put(j, ...) is _put_window for upload j, once
    the DMA of upload j - 2 has left its buffer.  close() destroys the events and frees the buffers; syncing ctx before is the
    caller's business."""

    def __init__(self, ctx, nbytes, staged=True):
        self.ctx, self.events = ctx, []
        self.stg = _Pinned(ctx, *[nbytes] * (2 if staged else 0))
        try:
            for _ in range(2):
                self.events.append(_event(ctx))
        except BaseException:
            self.close()
            raise

    def put(self, j, src, s, e, dst, dpitch=None):
        L, k = _lib.load(), j % 2
        if j >= 2 and self.stg.bufs:
            _lib.check(L.pg_event_sync(self.ctx.handle, self.events[k]), "pg_event_sync")
        _put_window(self.ctx, src, s, e, dst, dpitch, self.stg.bufs[k] if self.stg.bufs else None)
        _lib.check(L.pg_event_record(self.ctx.handle, self.events[k]), "pg_event_record")

    def close(self):
        for ev in self.events:
            _lib.load().pg_event_destroy(self.ctx.handle, ev)
        self.events = []
        self.stg.close()


class _Feed:
    """The feed of a streamed consumer: the SNPs of the _Source `src` in batches, uploaded on a second stream of ctx's device into
    two device slots, one batch ahead of the consumer, ordered by events.  The second stream is made with the feed; batches(pb)
    makes the slots, the staging buffers (for a source the DMA cannot read itself) and the events, and returns an iterator of
    (s, e, slot address): when it hands out a batch, ctx's stream already waits for that batch's upload, and the consumer
    enqueues its kernels for SNPs [s, e) on ctx before it takes the next one (which marks the slot as read and starts the upload
    after the next).  close() — however the consumer ended — drains both streams and releases all of it."""

    def __init__(self, ctx, src):
        self.ctx, self.src, self.up = ctx, src, _lib.Context(ctx.device)
        self.slots, self.ring, self.ev_done = [], None, []

    def batches(self, pb):
        for _ in range(2):
            self.slots.append(self.ctx.alloc(pb * self.src.row_bytes))
        self.ring = _Ring(self.up, pb * self.src.row_bytes, staged=not self.src.direct)
        for _ in range(2):
            self.ev_done.append(_event(self.ctx))
        return self._run([(s, min(s + pb, self.src.p)) for s in range(0, self.src.p, pb)])

    def _upload(self, b, s, e):
        if b >= 2:       # batch b-2 is done with the slot
            _lib.check(_lib.load().pg_stream_wait_event(self.up.handle, self.ev_done[b % 2]), "pg_stream_wait_event")
        # SNP-major: the records / columns [s, e) back to back; sample-major: the column window of every row at row stride e - s
        self.ring.put(b, self.src.src, s, e, self.slots[b % 2].ptr, None if self.src.snp_major else (e - s) * self.src.esz)

    def _run(self, batches):
        L, ctx = _lib.load(), self.ctx
        if batches:
            self._upload(0, *batches[0])
        for b, (s, e) in enumerate(batches):
            _lib.check(L.pg_stream_wait_event(ctx.handle, self.ring.events[b % 2]), "pg_stream_wait_event")
            yield s, e, self.slots[b % 2].ptr
            _lib.check(L.pg_event_record(ctx.handle, self.ev_done[b % 2]), "pg_event_record")
            if b + 1 < len(batches):
                self._upload(b + 1, *batches[b + 1])      # overlaps the kernels of batch b

    def close(self):
        self.up.sync()
        self.ctx.sync()
        for ev in self.ev_done:
            _lib.load().pg_event_destroy(self.ctx.handle, ev)
        if self.ring is not None:
            self.ring.close()
        self.up.close()
        for slot in self.slots:
            slot.free()
        self.slots, self.ring, self.ev_done = [], None, []
