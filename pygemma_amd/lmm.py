"""lmm.pygemma(Y, X, W, K, snps=...) — drop-in for the reference's entry point (lmm/lmm.py:87-411) with
everything under it running on MI355X through the C ABI (include/pygemma_hip.h):

    eigh(K)                     -> pg_syevd_dev   (fp64 Householder + divide & conquer, lmm.py:152/197)
    U.T @ X, U.T @ Y, U.T @ W   -> pg_rotate_geno_dev for genotype-valued SNP blocks (f16x2 MFMA), else
                                   pg_rotate_dev  (fp32 MFMA GEMM)                      (lmm.py:243-246)
    Pool(nproc).imap(calculate) -> pg_assoc_dev   (wave-per-SNP fused lambda search + Wald test, lmm.py:378-403,461-495)
    stats.f.sf                  -> on device      (lmm.py:482)

Same signature, same casts to float32 (lmm.py:115-128), same output DataFrame schema (columns beta, se_beta,
tau as float32; lambda, F_wald, p_wald as float64; SNPs as object when `snps` is given; lmm.py:403-409).
`nproc` = number of GPUs to spread contiguous SNP blocks over, exactly like SampleIter's ceil(p/nproc)
column blocks (lmm.py:427-434); results come back in block order = SNP order.

Streaming (BASELINE configs 4-5): X never has to fit on a GPU.  Every GPU takes its block in batches; a batch is DMA'd from
PINNED host memory (directly out of X: the caller's own pinned array — `pinned_empty`/`pin` — or X page-locked in place for
the duration of the call; a pinned staging buffer filled by copy threads only where that fails) on one stream while the
previous batch computes on another, and its 32-byte result rows come back through a pinned buffer.  With several GPUs the
eigenvectors travel once, GPU 0 -> all, as one RCCL broadcast over xGMI (pg_comm_*; no PyTorch).
There is no CPU fallback: without the HIP library or a GPU this raises.
"""
import contextlib
import ctypes as C
import json
import math
import os
import threading
import time
import zlib
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import pandas as pd

from . import _lib, dist
from ._feed import _KIN_DTYPES, _Feed, _Pinned, _Ring, _call_dev, _describe, _genotypes, _put_window     # noqa: F401  (_KIN_DTYPES: re-exported)
from ._lib import pin, pinned_empty     # noqa: F401  (re-exported: how a caller hands over pinned inputs)
from .bed import PackedBed
from .ops import LM_COLS as _LM_COLS, _ldx
from .model import *          # noqa: F401,F403  (precompute_mat, calc_lambda_restricted, newton, the *_overload scalars)
from . import model as _model
from .vc import RemlResult, reml, vc_kinship     # noqa: F401  (re-exported: variance components for several kinship matrices)

__all__ = ["pygemma", "pygemma_multi", "pygemma_score", "pygemma_gxe", "pygemma_lm", "snp_stats", "snp_filter", "SampleIter", "pinned_empty", "pin",
           "kinship", "ld", "ld_window", "ld_prune", "clump", "ld_scores", "ldsc", "LdscResult", "epistasis", "EpistasisResult", "case_control", "case_control_perm", "PermResult", "prs", "prs_weights", "king", "ibs",
           "sample_stats", "related_pairs", "unrelated", "pca", "pca_project", "PcaResult", "reml", "vc_kinship", "RemlResult"] + _model.__all__

_BATCH_BYTES = 6 << 30   # device bytes for one SNP batch of one worker (raw block, rotated block, fp16 planes)
_BATCH_SNPS = 32768      # SNPs per batch at most: the unit of copy/compute overlap and of checkpointing
_WORKERS = 2             # host threads (each with its own stream and buffers) per GPU
_BATCH_MIN = 8192        # ... and at least, while the block is cut into up to _BATCH_COUNT batches: the first batch's DMA and the
_BATCH_COUNT = 12        # last batch's kernels are the part of the loop that does not overlap (measured at p = 100 000: 4 batches
                         # 0.149-0.172 s, 8: 0.116, 12: 0.112, 16: 0.112 — tools/ab_stream_batch.py)
# Device bytes of X per GPU that may be copied in while the eigensolver runs.  OFF by default (0): with the caller's X in
# hipHostMalloc'ed memory (pinned_empty) it takes the copy time out of the loop (p = 400 000 float32: 0.96 -> 0.90 s end to end), but
# inside a long-lived process the first allocations after the eigensolver were seen to stall for ~0.15 s in one run out of four, and
# from memory page-locked in place (hipHostRegister) the run was 0.25 s SLOWER every time (tools/ab_stream_batch.py, bench.py e2e leg
# with PYGEMMA_PREFETCH_MAX=1e11).  Opt-in: PYGEMMA_PREFETCH_MAX=<bytes>; only an X the caller pinned himself is prefetched.
_PREFETCH_MAX = int(float(os.environ.get("PYGEMMA_PREFETCH_MAX", 0)))
_PREFETCH_MARGIN = 8 << 30  # ... and what is left untouched beside the eigensolver's and the workers' buffers
_U_PANEL_BYTES = 256 << 20  # eigenvectors given in pageable memory travel in row panels of this size through two pinned buffers


class SampleIter:
    """Contiguous column blocks of ceil(p/nproc) SNPs (lmm/lmm.py:413-436) — here: one block per GPU."""

    def __init__(self, p, nproc):
        self.p, self.nproc = int(p), int(nproc)

    def __iter__(self):
        cols = int(np.ceil(self.p / self.nproc))
        for r in range(self.nproc):
            a, b = r * cols, min((r + 1) * cols, self.p)
            if a < b:
                yield a, b


_T_LOG = [time.time()]


def _log(verbose, msg):
    if verbose > 0:
        now = time.time()
        print(f"[pygemma_amd +{now - _T_LOG[0]:7.3f} s] {msg}", flush=True)
        _T_LOG[0] = now


def _rotate_small(ctx, L, n, dU, A):
    """U.T @ A for a narrow host matrix A (n,q) (Y and W): same MFMA kernel, SNP-major result transposed back."""
    q = A.shape[1]
    ldx = _ldx(n)
    with _lib.scope(ctx):
        dA = ctx.to_device(np.ascontiguousarray(A, np.float32))
        dO = ctx.alloc(q * ldx * 4)
        _lib.check(L.pg_rotate_dev(ctx.handle, n, q, dU.ptr, n, dA.ptr, q, dO.ptr, ldx), "pg_rotate_dev")
        ctx.sync()
        return dO.download((q, ldx), np.float32)[:, :n].T.copy()


_COLS = ("beta", "se_beta", "tau", "lambda", "F_wald", "p_wald")
_LRT_COLS = ("l_alt", "l_null", "D_lrt", "p_lrt")


def _part_path(ckpt, s, e):
    return os.path.join(ckpt, f"part_{s:012d}_{e:012d}.npz")


def _crc(a):
    return int(zlib.crc32(np.ascontiguousarray(a).view(np.uint8).reshape(-1)))


def _block_fingerprint(src, s, e):
    """Cheap identity of the raw SNP block [s, e): CRC-32 of 64 evenly spaced sample rows (of byte columns for packed
    records).  Stored in every checkpoint part and compared before a part is restored, so that parts of a run on another
    genotype matrix of the same shape are refused instead of being mixed into the result."""
    if src.packed:
        rec = src.src.data[s:e]
        return _crc(rec[:, ::max(1, src.row_bytes // 64)])
    rows = np.unique(np.linspace(0, src.n - 1, min(src.n, 64)).astype(np.int64))
    return _crc(src.src[rows, s:e])


def _batch_geometry(n, a, b, gxe=False):
    """(SNPs per batch, row pitch in elements of a raw sample-major batch) for the block [a, b) of one GPU (`gxe`: the interaction
    scan, whose batches also hold the rotated x o e block)."""
    ldx = _ldx(n)
    per_snp = (16 if gxe else 12) * ldx                               # raw block + rotated block + two fp16 planes [+ rotated x o e]
    pb_max = max(256, int(_BATCH_BYTES // per_snp) // 256 * 256)
    pb_max = min(pb_max, _BATCH_SNPS, b - a)
    nbat = max(-(-(b - a) // pb_max), min(_BATCH_COUNT, -(-(b - a) // _BATCH_MIN)))
    pb_max = min(pb_max, (-(-(b - a) // nbat) + 255) // 256 * 256)
    return pb_max, (pb_max + 15) // 16 * 16


_View = namedtuple("_View", "ptr")      # a range of a device buffer (what a worker needs of a batch: its address)


class _Prefetch:
    """X on its way to the devices WHILE the eigensolver runs (eigen=True from K; X a C-contiguous, page-locked host matrix): one
    host thread per GPU DMAs the leading batches of that GPU's block into ONE device buffer (allocated here, before the eigensolver
    starts: no allocation competes with its launches) on a stream of its own — PCIe and the HBM-bound tridiagonalisation do not
    compete — within what hipMemGetInfo leaves after the eigensolver's workspace (~60 n^2 bytes on GPU 0) and the workers' own
    buffers.  The SNP loop then takes those batches instead of issuing the copies: the loop runs at the kernels' rate, and at
    288 GB of HBM a 40 GB float32 X is resident before U is."""

    def __init__(self, L, src, blocks, verbose, gxe=False):
        self.L, self.X, self.n, self.esz, self.verbose = L, src.src, src.n, src.esz, verbose
        self.lock = threading.Lock()
        self.ready = [dict() for _ in blocks]
        self.ctxs, self.plans = [], []
        self.bytes = 0
        self.stop = False                        # set when the eigensolver is done: the batch in flight is the last one
        self.threads = []
        try:
            self._plan(blocks, gxe)
        except BaseException:                    # a context or buffer of GPU g failed: release those of the GPUs before it
            for ctx in self.ctxs:
                ctx.close()
            self.ctxs = []
            raise
        self.threads = [threading.Thread(target=self._run, args=(g,)) for g in range(len(blocks))]
        for th in self.threads:
            th.start()

    def _plan(self, blocks, gxe):
        n, esz = self.n, self.esz
        for g, (a, b) in enumerate(blocks):
            ctx = _lib.Context(g)
            self.ctxs.append(ctx)
            free, _total = ctx.mem_info()
            reserve = (96 * n * n if g == 0 else 12 * n * n) + 2 * _BATCH_BYTES + _PREFETCH_MARGIN      # GPU 0: the eigensolver's 10 n^2 doubles + its outputs
            if gxe:                                  # diag(e) U and its genotype prep beside U's (the x o e slices are in _BATCH_BYTES)
                reserve += 4 * n * n + int(self.L.pg_geno_prep_bytes(n))
            budget = min(free - reserve, _PREFETCH_MAX)
            pb_max, ldX = _batch_geometry(n, a, b, gxe)
            per = n * ldX * esz
            batches = [(s, min(s + pb_max, b)) for s in range(a, b, pb_max)]
            batches = batches[: max(0, int(budget // per))]
            big = ctx.alloc(per * len(batches)) if batches else None
            self.plans.append((batches, big, per, ldX))

    def _run(self, g):
        try:
            n, esz = self.n, self.esz
            ctx = self.ctxs[g]
            batches, big, per, ldX = self.plans[g]
            done = 0
            for k, (s, e) in enumerate(batches):
                if self.stop:
                    break
                dst = big.ptr + k * per
                _put_window(ctx, self.X, s, e, dst, ldX * esz)
                ctx.sync()                       # a batch is offered only once it has landed
                with self.lock:
                    self.ready[g][(s, e)] = _View(dst)
                    self.bytes += n * (e - s) * esz
                done += n * (e - s) * esz
                _log(self.verbose - 1, f"GPU {g}: SNPs [{s},{e}) prefetched")
            _log(self.verbose, f"GPU {g}: {done / 1e9:.2f} GB of X prefetched during the eigendecomposition")
        except Exception as ex:                  # prefetching is an optimisation: on any failure the loop copies as usual
            _log(self.verbose, f"GPU {g}: prefetch stopped ({ex!r})")

    def join(self):
        self.stop = True
        for th in self.threads:
            th.join()

    def take(self, g, s, e):
        with self.lock:
            return self.ready[g].pop((s, e), None)

    def close(self):
        self.join()
        for ctx in self.ctxs:
            ctx.close()                          # frees the buffers (after the loop: hipFree inside it would drain the device)
        self.ctxs = []


# What one kind of scan does with a batch of rotated SNPs (_scan_mode builds it once per call): its result columns in output order
# (also those of a checkpoint part), result bytes per SNP, warm(ctx, pb_max) before a worker's first batch (or None),
# launch(ctx, dev, pb, dXr, r0) of a batch's kernels (dev = (d, W, y) on that GPU, result rows at r0) and decode(host bytes, out,
# s, e) of a batch's result rows into out[col][..., s:e]
_Mode = namedtuple("_Mode", "cols nout warm launch decode")


def _scan_mode(L, n, c, grid, lrt, npheno, lam0, gxe=False):
    """The Wald scan (with `lrt` plus the likelihood-ratio columns), the scan of `npheno` > 0 phenotypes, the score scan at the
    null model's float32 ML lambda `lam0` (the same for every GPU), or with `gxe` the interaction scan (c shared covariates, the
    last of them e; its launch takes the rotated x o e block as a sixth argument).  Each writes the 32-byte rows
    [F | p | beta | se | tau | lambda] of dist.result_columns, for npheno phenotype-major rows of pb SNPs with npheno; lrt appends
    [l_alt | l_null | D_lrt | p_lrt] in float64."""
    ldx = _ldx(n)
    t = npheno or 1

    def rows(r0, m):      # the fields of m result rows at r0 in the kernels' argument order: beta, se, tau, lambda, F, p
        return r0 + 16 * m, r0 + 20 * m, r0 + 24 * m, r0 + 28 * m, r0, r0 + 8 * m

    warm = None
    if npheno:
        def warm(ctx, pb_max):
            _lib.check(L.pg_assoc_pheno_warm(ctx.handle, n, c, npheno, pb_max), "pg_assoc_pheno_warm")

        def launch(ctx, dev, pb, dXr, r0):
            _lib.check(L.pg_assoc_pheno_dev(ctx.handle, n, c, pb, npheno, *dev, n, dXr, ldx, int(grid), *rows(r0, npheno * pb), None),
                       "pg_assoc_pheno_dev")
    elif gxe:
        def warm(ctx, pb_max):
            _lib.check(L.pg_assoc_gxe_warm(ctx.handle, n, c), "pg_assoc_gxe_warm")

        def launch(ctx, dev, pb, dXr, r0, dXEr):
            _lib.check(L.pg_assoc_gxe_dev(ctx.handle, n, c, pb, *dev, dXr, ldx, dXEr, ldx, *rows(r0, pb), None), "pg_assoc_gxe_dev")
    elif lam0 is not None:
        def launch(ctx, dev, pb, dXr, r0):
            _lib.check(L.pg_score_dev(ctx.handle, n, c, pb, *dev, float(lam0), dXr, ldx, *rows(r0, pb)), "pg_score_dev")
    else:
        def warm(ctx, pb_max):      # the first batch's kernels then queue without a host stall
            _lib.check(L.pg_assoc_warm(ctx.handle, n, c), "pg_assoc_warm")

        def launch(ctx, dev, pb, dXr, r0):
            if lrt:
                _lib.check(L.pg_assoc_lrt_dev(ctx.handle, n, c, pb, *dev, dXr, ldx, int(grid), *rows(r0, pb),
                                              r0 + 32 * pb, r0 + 40 * pb, r0 + 48 * pb, r0 + 56 * pb), "pg_assoc_lrt_dev")
            else:
                _lib.check(L.pg_assoc_dev(ctx.handle, n, c, pb, *dev, dXr, ldx, int(grid), *rows(r0, pb), None), "pg_assoc_dev")

    def decode(hb, out, s, e):
        pb = e - s
        for col, v in dist.result_columns(hb, t * pb).items():
            out[col][..., s:e] = v.reshape(npheno, pb) if npheno else v
        if lrt:
            LR = np.frombuffer(hb, np.float64, 4 * pb, 32 * pb).reshape(4, pb)
            for k, col in enumerate(_LRT_COLS):
                out[col][s:e] = LR[k]

    return _Mode(_COLS + (_LRT_COLS if lrt else ()), 32 * t + (32 if lrt else 0), warm, launch, decode)


# The per-call invariants every GPU's block of a scan reads: eigenvalues d, rotated covariates Wr (n, c), rotated phenotype yr ((n,),
# or (npheno, n) phenotype-major rows), the _Source of X as _scan leaves it, the _Mode, the checkpoint directory, the stats dict, the
# _Prefetch (each or None), the result columns `out` (filled in place) and `errs`, where the block and worker threads leave their
# exceptions, and for the interaction scan the float32 environment `e` (n,) (None otherwise)
_Job = namedtuple("_Job", "n c d Wr yr src grid eigen mode ckpt stats pre verbose out errs e", defaults=(None,))


def _restore(job, device, a, b, pb_max):
    """The batches of [a, b) still to do; those with a checkpoint part are read back into job.out instead."""
    todo = []
    for s in range(a, b, pb_max):
        e = min(s + pb_max, b)
        part = _part_path(job.ckpt, s, e) if job.ckpt else None
        if part is None or not os.path.exists(part):
            todo.append((s, e))
            continue
        with np.load(part) as z:
            if "fingerprint" not in z.files or int(z["fingerprint"]) != _block_fingerprint(job.src, s, e):
                raise ValueError(f"checkpoint part {part} was computed from different genotypes "
                                 f"(fingerprint of SNPs [{s},{e}) differs): refusing to mix runs")
            for col in job.mode.cols:
                job.out[col][s:e] = z[col]
        _log(job.verbose, f"GPU {device}: SNPs [{s},{e}) restored from {job.ckpt}")
    return todo


def _save_part(job, s, e):
    tmp = _part_path(job.ckpt, s, e) + ".tmp.npz"
    np.savez(tmp, fingerprint=np.int64(_block_fingerprint(job.src, s, e)), **{col: job.out[col][s:e] for col in job.mode.cols})
    os.replace(tmp, _part_path(job.ckpt, s, e))


def _run_threads(target, argsets):      # one thread per argument tuple: all started, then all joined
    threads = [threading.Thread(target=target, args=args) for args in argsets]
    for th in threads:
        th.start()
    for th in threads:
        th.join()


def _stat_max(stats, key, since, lock=contextlib.nullcontext()):
    if stats is not None:
        with lock:
            stats[key] = max(stats.get(key, 0.0), time.time() - since)


def _rotation(L, src, eigen, n, ldx, ldX):
    """The rotation of a block's batches, picked once (it depends on X's kind, `eigen` and PYGEMMA_ROTATE, not on the batch):
    rot(ctx, w, pb, dXc, dU, dprep, dXr, xf) sends the pb SNPs whose raw block lies at dXc (pitch ldX), rotated by dU with its genotype
    prep, to dXr (pitch ldx).  `xf`: a list the interaction scan's two rotations of a batch (U, then diag(e) U) share, empty at first."""
    if src.packed:       # decode + impute + rotate for .bed records
        def rot(ctx, w, pb, dXc, dU, dprep, dXr, xf):
            _lib.check(L.pg_rotate_bed_dev(ctx.handle, n, pb, dprep.ptr, w.X.ptr, src.row_bytes, src.count_a1, dXr, ldx, w.work.ptr), "pg_rotate_bed_dev")
    elif src.src.dtype == np.float64:
        def rot(ctx, w, pb, dXc, dU, dprep, dXr, xf):
            if not xf:       # the genotype check depends on X only: a block that failed it for U fails it for Ue
                is_geno = C.c_int(0)
                _lib.check(L.pg_rotate_geno_f64_dev(ctx.handle, n, pb, dprep.ptr, dXc.ptr, ldX, dXr, ldx, w.work.ptr, C.byref(is_geno)), "pg_rotate_geno_f64_dev")
                if is_geno.value:
                    return
                # off the genotype path: the block's float32 image in w.Xf (allocated with the first such block), cast once for both rotations
                w.Xf = w.Xf or ctx.alloc(n * ldX * 4)
                _lib.check(L.pg_cast_f64_f32_dev(ctx.handle, n, pb, dXc.ptr, ldX, w.Xf.ptr, ldX), "pg_cast_f64_f32_dev")
                xf.append(True)
            _lib.check(L.pg_rotate_dev(ctx.handle, n, pb, dU.ptr, n, w.Xf.ptr, ldX, dXr, ldx), "pg_rotate_dev")
    elif src.src.dtype in (np.int8, np.uint8):      # 8-bit block (always finite): genotype codes or split planes, chosen on the device
        def rot(ctx, w, pb, dXc, dU, dprep, dXr, xf):
            _lib.check(L.pg_rotate_auto_i8_dev(ctx.handle, n, pb, dprep.ptr, dXc.ptr, int(src.src.dtype == np.uint8), ldX, dXr, ldx, w.work.ptr, None),
                       "pg_rotate_auto_i8_dev")
    elif eigen and os.environ.get("PYGEMMA_ROTATE", "") == "fp32":      # the reference-arithmetic kernel for every block (tests, A/B)
        def rot(ctx, w, pb, dXc, dU, dprep, dXr, xf):
            _lib.check(L.pg_rotate_dev(ctx.handle, n, pb, dU.ptr, n, dXc.ptr, ldX, dXr, ldx), "pg_rotate_dev")
    elif eigen:          # float32 block: path (genotype fp16x2 / split planes / fp32 MFMA) chosen on the device, no host wait
        def rot(ctx, w, pb, dXc, dU, dprep, dXr, xf):
            _lib.check(L.pg_rotate_auto_dev(ctx.handle, n, pb, dU.ptr, n, dprep.ptr, dXc.ptr, ldX, dXr, ldx, w.work.ptr, None), "pg_rotate_auto_dev")
    elif not src.snp_major:      # eigen=False: rotated by the caller, only turned SNP-major
        def rot(ctx, w, pb, dXc, dU, dprep, dXr, xf):
            _lib.check(L.pg_transpose_dev(ctx.handle, n, pb, dXc.ptr, ldX, dXr, ldx), "pg_transpose_dev")
    else:                # ... and SNP-major: the copy-in landed it in the layout the scan reads
        def rot(ctx, w, pb, dXc, dU, dprep, dXr, xf):
            pass
    return rot


def _block_setup(job, device, a, b, dU, comm, ctx0):
    """What a GPU's workers share: U (broadcast first), the scan's invariants and the rotation's preps on the device, geometry, rotation."""
    L, n, src = _lib.load(), job.n, job.src
    if job.eigen and comm is not None:
        # U: resident on GPU 0 (the eigensolver's output); the other GPUs get it over xGMI.  The collective comes before
        # anything else of this thread that can fail (its receive buffer was allocated by the caller), so that no GPU is
        # left waiting in the broadcast for a peer that has already given up.
        t0 = time.time()
        _lib.check(L.pg_comm_broadcast_dev(comm.handle, dU.ptr, n * n * 4, 0), "pg_comm_broadcast_dev")
        ctx0.sync()
        _log(job.verbose, f"GPU {device}: U ({n * n * 4 / 1e9:.2f} GB) broadcast over RCCL in {time.time() - t0:.3f} s")
    g = SimpleNamespace(L=L, device=device, n=n, src=src, ldx=_ldx(n), gxe=job.e is not None, dU=dU, dprep=None, dUe=None, dprepe=None)
    g.dev = tuple(ctx0.to_device(v).ptr for v in (job.d, job.Wr, job.yr))
    if job.eigen:
        # genotype fast path of the rotation (<= 3 equally spaced values per column), fp32 MFMA otherwise
        g.dprep = ctx0.alloc(L.pg_geno_prep_bytes(n))
        _lib.check(L.pg_geno_prep_dev(ctx0.handle, n, dU.ptr, n, g.dprep.ptr), "pg_geno_prep_dev")
    if g.gxe:
        # U'(x o e) = (diag(e) U)' x: Ue and its genotype prep, made on this GPU (after the broadcast of U), and every batch
        # rotated twice, with (U, prep) into Xr and with (Ue, prep_e) into XEr
        dE = ctx0.to_device(job.e)
        g.dUe, g.dprepe = ctx0.alloc(n * n * 4), ctx0.alloc(L.pg_geno_prep_bytes(n))
        _lib.check(L.pg_gxe_scale_u_dev(ctx0.handle, n, dU.ptr, n, dE.ptr, g.dUe.ptr), "pg_gxe_scale_u_dev")
        _lib.check(L.pg_geno_prep_dev(ctx0.handle, n, g.dUe.ptr, n, g.dprepe.ptr), "pg_geno_prep_dev")
    ctx0.sync()
    g.pb_max, g.ldX = _batch_geometry(n, a, b, g.gxe)
    # X itself is page-locked: DMA straight out of it.  Packed records are always staged here (_copy_in), even when pinned: whether the
    # DMA could read them directly, as the feed does, is a change of its own with its own measurement.
    g.direct = src.direct and not src.packed
    g.rotate = _rotation(L, src, job.eigen, n, g.ldx, g.ldX)
    return g


def _copy_in(job, g, ctx, w, s, e):
    """The raw block of SNPs [s, e) travels to the device, or landed there while the eigensolver ran: returns (where it is, prefetched)."""
    dXc = job.pre.take(g.device, s, e) if job.pre is not None else None
    if dXc is not None:
        return dXc, True     # (a prefetched buffer is freed with the prefetcher: hipFree would drain the device here)
    src, n = g.src, g.n
    if src.packed:       # SNP records [s, e) of the .bed image, staged by one thread
        _put_window(ctx, src.src, s, e, w.X.ptr, staging=w.inp, threads=1)
    elif src.snp_major:  # SNPs [s, e) are pb contiguous rows of n floats (float32 only: _inputs sees to it)
        dst, dpitch = (w.T.ptr, 4 * n) if job.eigen else (w.Xr.ptr, 4 * g.ldx)     # eigen=False: already the layout the scan reads
        _put_window(ctx, src.src, s, e, dst, dpitch, w.inp)
        if job.eigen:    # (pb x n) -> (n x ldX): the transposition kernel with the roles of n and p exchanged
            _lib.check(g.L.pg_transpose_dev(ctx.handle, e - s, n, w.T.ptr, n, w.X.ptr, g.ldX), "pg_transpose_dev")
    else:                # the column window [s, e) of every sample row, at row pitch ldX
        _put_window(ctx, src.src, s, e, w.X.ptr, g.ldX * src.esz, w.inp)
    return w.X, False


def _batch(job, g, ctx, w, s, e):
    """SNPs [s, e) on this worker's stream up to their result rows in w.out; returns (t_dma, prefetched)."""
    pb = e - s
    dXc, prefetched = _copy_in(job, g, ctx, w, s, e)
    t_dma = time.time()
    xf = []
    g.rotate(ctx, w, pb, dXc, g.dU, g.dprep, w.Xr.ptr, xf)
    if g.gxe:            # x o e: the same path on the same raw block, with Ue in U's place
        g.rotate(ctx, w, pb, dXc, g.dUe, g.dprepe, w.XEr.ptr, xf)
    job.mode.launch(ctx, g.dev, pb, w.Xr.ptr, w.res.ptr, *((w.XEr.ptr,) if g.gxe else ()))      # the mode's kernels, and the result rows back
    _lib.check(g.L.pg_memcpy_d2h_async(ctx.handle, w.out, w.res.ptr, pb * job.mode.nout), "pg_memcpy_d2h_async")
    ctx.sync()
    return t_dma, prefetched


def _worker_buffers(job, g, ctx, w):
    """A worker's device buffers (w.X, T, Xr, res, work, XEr) and pinned ones (w.stg: staging w.inp unless the DMA reads X itself, result rows w.out)."""
    n, src, pb_max, ldx, nout = g.n, g.src, g.pb_max, g.ldx, job.mode.nout
    raw_bytes = pb_max * src.row_bytes if src.packed else n * g.ldX * src.esz
    # one device allocation per worker, cut into its buffers: every hipMalloc / hipFree of a few hundred MB costs
    # 1 - 2 ms of host time that nothing overlaps (r4: worker set-up 3.8 ms, teardown 9.2 ms with five allocations)
    sizes = [raw_bytes, pb_max * n * 4 if (src.snp_major and not src.packed and job.eigen) else 0, pb_max * ldx * 4, pb_max * nout,
             g.L.pg_geno_work_bytes(n, pb_max) if job.eigen else 0, pb_max * ldx * 4 if g.gxe else 0]
    offs = np.concatenate([[0], np.cumsum([(int(z) + 255) // 256 * 256 for z in sizes])])
    arena = ctx.alloc(int(offs[-1]))
    for k, o, z in zip(("X", "T", "Xr", "res", "work", "XEr"), offs[:-1], sizes):
        setattr(w, k, _View(arena.ptr + int(o)) if z else None)
    w.stg = _Pinned(ctx, pb_max * nout) if g.direct else _Pinned(ctx, raw_bytes, pb_max * nout)
    w.inp, w.out = (None, *w.stg.bufs) if g.direct else w.stg.bufs
    w.hres = (C.c_char * (pb_max * nout)).from_address(w.out)


def _worker(job, g):
    """One of a GPU's host threads, with its own stream, device buffers and pinned staging, so that the host->device DMA of its batch
    overlaps the kernels of the other's: batches off g.todo until it is empty or a thread has failed."""
    try:
        ctx, stats = _lib.Context(g.device), job.stats
        w = SimpleNamespace(stg=None, Xf=None)
        t_w = time.time()
        try:
            _worker_buffers(job, g, ctx, w)
            if job.mode.warm is not None:
                job.mode.warm(ctx, g.pb_max)
            _stat_max(job.stats, "worker_alloc_s", t_w, g.lock)
            while True:
                with g.lock:
                    if not g.todo or job.errs:
                        return
                    s, e = g.todo.pop(0)
                t_in = time.time()
                t_dma, prefetched = _batch(job, g, ctx, w, s, e)
                t_ker = time.time()
                job.mode.decode(w.hres, job.out, s, e)
                if stats is not None:
                    with g.lock:
                        if prefetched:
                            stats["prefetched_batches"] = stats.get("prefetched_batches", 0) + 1
                        stats["batches"] += 1
                        stats["bytes_in"] += (e - s) * g.src.row_bytes
                        stats["batch_s"] += time.time() - t_in
                        stats["dma_s"] = stats.get("dma_s", 0.0) + (t_dma - t_in)       # copy-in: staging + DMA issue
                        stats["kernel_s"] = stats.get("kernel_s", 0.0) + (t_ker - t_dma)
                if job.ckpt:
                    _save_part(job, s, e)
                _log(job.verbose, f"GPU {g.device}: SNPs [{s},{e}) done")
        finally:
            t_td = time.time()
            if w.stg is not None:
                ctx.sync()
                w.stg.close()
            ctx.close()
            _stat_max(job.stats, "worker_teardown_s", t_td, g.lock)
    except Exception as ex:  # surfaced by the caller; never swallowed
        job.errs.append(ex)


def _run_block(job, device, a, b, dU, comm):
    """One GPU: SNP columns [a,b) of X through (rotate | transpose) -> the kernels of job.mode, in batches that _WORKERS host threads
    take from a shared list.  `dU`: GPU 0's resident eigenvectors (device 0) or None; with a communicator the other GPUs receive them
    by RCCL broadcast.  With job.ckpt every finished batch is written to disk (and batches found there, with a matching fingerprint
    of the raw block, are not redone)."""
    try:
        ctx0 = comm.ctx if comm is not None else _lib.Context(device)
        t_blk = time.time()
        try:
            g = _block_setup(job, device, a, b, dU, comm, ctx0)
            g.todo, g.lock = _restore(job, device, a, b, g.pb_max), threading.Lock()
            _stat_max(job.stats, "setup_s", t_blk)
            _run_threads(_worker, [(job, g)] * min(_WORKERS, len(g.todo)))
        finally:
            t_td = time.time()
            if comm is None:
                ctx0.close()
            _stat_max(job.stats, "block_teardown_s", t_td)
    except Exception as ex:  # surfaced by the caller; never swallowed
        job.errs.append(ex)


_Comm = namedtuple("_Comm", "handle ctx")     # one communicator of a pg_comm_init_all group + the context it is bound to


def _make_comms(L, ndev):
    ctxs = [_lib.Context(g) for g in range(ndev)]
    hs = (C.c_void_p * ndev)(*[c.handle for c in ctxs])
    outs = (C.c_void_p * ndev)()
    rc = L.pg_comm_init_all(ndev, hs, outs)
    if rc:
        msg = L.pg_last_error().decode()
        for h in outs:
            if h:
                L.pg_comm_destroy(h)
        for c in ctxs:
            c.close()
        raise _lib.PgError(f"pg_comm_init_all({ndev}) failed (code {rc}): {msg}")
    return [_Comm(C.c_void_p(outs[g]), ctxs[g]) for g in range(ndev)]


def kinship(G, standardize=True, device=0, *, snp_batch=None):
    """K = Z Z' / p from the (n, p) genotype matrix G on the GPU (the step before the path in the reference's callers:
    experiments/animal_gwas/run_gwas.py:46-56, tests/test_pygemma.py:184-192): columns centred and divided by their
    standard deviation (population, ddof=0; sd == 0 -> 1) when `standardize`, then a lower-triangle syrk on the MFMA pipe.
    Returns the (n, n) float32 matrix (both triangles, bit-symmetric), ready for `pygemma`.

    G may also be a `PackedBed`, and an array may be streamed with `snp_batch`: then SNP batches of that many columns travel to
    the device one after the other (host and device memory bounded at any p) and K is accumulated there in fp64
    (DESIGN §4.7).  The streamed path takes a PackedBed (always; `snp_batch` None picks the batch from n and the free device
    memory) and int8, uint8, float32 or float64 arrays, sample-major (C order) or SNP-major (Fortran order), pinned or
    pageable, without a host copy or cast of the whole matrix.  .bed codes and 8-bit values go through the fp16 matrix pipe,
    float blocks through the fp32 syrk (PG_KINSHIP_FP32=1 sends every block there).  A missing .bed call takes the mean of the
    called genotypes of its SNP, so K equals kinship(G.to_float(impute=True)) up to rounding; an all-missing SNP, where
    to_float gives NaN, is treated like a monomorphic one: it contributes zeros and still counts in p.
    With an array and `snp_batch` None, the whole float32 matrix is uploaded and handled at once (the original path)."""
    _check_snp_batch(snp_batch)
    if isinstance(G, PackedBed) or snp_batch is not None:
        G = _genotypes(G, "streamed kinship", "G")
        if G.shape[0] < 1 or G.shape[1] < 1:
            raise ValueError(f"kinship needs at least one sample and one SNP: G holds n={G.shape[0]}, p={G.shape[1]}")
        return _kinship_stream(G, bool(standardize), device, snp_batch)
    L = _lib.load()
    G = np.ascontiguousarray(G, np.float32)
    n, p = G.shape
    with _lib.scope(device=device) as ctx:
        dG = ctx.to_device(G)
        dK = ctx.alloc(n * n * 4)
        _lib.check(L.pg_kinship_geno_dev(ctx.handle, n, p, dG.ptr, p, int(bool(standardize)), dK.ptr), "pg_kinship_geno_dev")
        ctx.sync()
        return dK.download((n, n), np.float32)


# SNPs per batch by default: the fp64 read-modify-write of the accumulator (8 n^2 bytes per batch) against the batch's syrk
# (2 n^2 pb fp16 flops on and below the diagonal) costs ~1 000 / pb of the batch at 5 TB/s and 1.2 PF: 6 % at 16 384
_KIN_BATCH = 16384


def _check_snp_batch(snp_batch):
    if snp_batch is not None and (isinstance(snp_batch, bool) or not isinstance(snp_batch, (int, np.integer)) or snp_batch < 1):
        raise ValueError(f"snp_batch must be a positive integer, not {snp_batch!r}")


def _fit_batch(ctx, snp_batch, default, p, floor, need, who, what):
    """SNPs per batch of a streamed scan over p SNPs: the caller's `snp_batch`, or `default` halved down to `floor` until the need(pb)
    device bytes fit into 0.9 of what is free on ctx's GPU; a batch that does not fit is refused."""
    pb, auto = min(p, int(snp_batch or default)), snp_batch is None
    free, _total = ctx.mem_info()
    while auto and pb > floor and need(pb) > 0.9 * free:
        pb = max(floor, pb // 2)
    if need(pb) > free:
        raise _lib.PgError(f"{who}, snp_batch={pb} needs {need(pb) / 2**30:.2f} GiB of device memory ({what}), "
                           f"{free / 2**30:.2f} GiB free on GPU {ctx.device}")
    return pb


def _kinship_stream(G, standardize, device, snp_batch):
    """The streamed kinship: SNP batches from the feed (_feed._Feed) through pg_kinship_{bed,x}_acc_dev into one fp64
    accumulator, then pg_kinship_finish_dev."""
    L = _lib.load()
    src = _describe(G)
    n, p = src.n, src.p
    with _lib.Context(device) as ctx, contextlib.closing(_Feed(ctx, src)) as feed:
        pb = _fit_batch(ctx, snp_batch, _KIN_BATCH, p, 64,
                        lambda pb: int(L.pg_kinship_acc_bytes(n, pb)) + 4 * n * n + 2 * pb * src.row_bytes,
                        f"kinship: n={n}", "fp64 accumulator 8 n^2, K 4 n^2, batch buffers")
        dacc = ctx.alloc(L.pg_kinship_acc_bytes(n, pb))
        dK = ctx.alloc(4 * n * n)
        batches = feed.batches(pb)
        _lib.check(L.pg_memset(ctx.handle, dacc.ptr, 0, 8 * n * n), "pg_memset")
        for s, e, slot in batches:
            _call_dev(L, "pg_kinship_{}_acc_dev", src, (ctx.handle, n, e - s), slot, e - s, (int(standardize), dacc.ptr))
        _lib.check(L.pg_kinship_finish_dev(ctx.handle, n, p, dacc.ptr, dK.ptr), "pg_kinship_finish_dev")
        ctx.sync()
        return dK.download((n, n), np.float32)


_LM_SLOT_BYTES = 256 << 20     # device bytes of one upload slot by default, and SNPs per batch at most: many batches, so that only the
_LM_BATCH = 16384              # first upload (and, from pageable memory, the first staging copy) is exposed
_CHI2_MEDIAN = 0.4549364       # chi2.ppf(0.5, 1)


def _gpus():     # how many are in sight; none is an error
    ngpu = _lib.device_count()
    if ngpu < 1:
        raise _lib.PgError("no MI355X visible: pygemma_amd has no CPU path")
    return ngpu


def _lm_batch(src):     # SNPs per batch of the linear-model and QC streams by default: one upload slot's worth
    return min(_LM_BATCH, max(128, _LM_SLOT_BYTES // src.row_bytes // 128 * 128))


def _stream_stats(stats, src, pb, t0):
    if stats is not None:
        stats.update({"batches": -(-src.p // pb), "bytes_in": src.p * src.row_bytes, "seconds": time.time() - t0})


def _pheno_columns(Y):
    """(labels, float32 columns) of a phenotype argument: (n,), (n, 1), (n, t) or a DataFrame (labelled by its columns, an array by
    0..t-1), every column cast on its own as lmm.pygemma casts its Y (lmm.py:115-116)."""
    if isinstance(Y, pd.DataFrame):
        labels = list(Y.columns)
        cols = [np.asarray(Y.iloc[:, k]) for k in range(Y.shape[1])]
    else:
        Ya = np.asarray(Y)
        if Ya.ndim == 1:
            Ya = Ya.reshape(-1, 1)
        if Ya.ndim != 2:
            raise ValueError(f"Y must be (n,), (n, 1) or (n, t), got shape {Ya.shape}")
        labels = list(range(Ya.shape[1]))
        cols = [Ya[:, k] for k in range(Ya.shape[1])]
    if not cols:
        raise ValueError("Y has no phenotype columns")
    return labels, [col.astype(np.float32) for col in cols]


def _frame(out, cols, snps, k=None):
    """The result columns `cols` of `out` (with k: of phenotype k) as the DataFrame the reference returns (lmm.py:403-409)."""
    df = pd.DataFrame({col: out[col] if k is None else out[col][k] for col in cols}, columns=list(cols))
    if snps is not None:
        df["SNPs"] = snps
    return df


def pygemma_lm(Y, X, W, snps=None, verbose=0, device=0, snp_batch=None, stats=None):
    """The plain linear model per SNP (GEMMA's -lm 1; the OLS loop of experiments/1000G/run_lin_reg.py): y_k = W alpha + x_g beta + eps,
    the K-free baseline a mixed-model scan is read against (how much inflation does K remove?).  Neither eigensolver nor rotation:
    the scan reads the raw genotypes once, so a whole-genome pass costs little more than moving X.

    Y: (n,), (n, 1), (n, t) or a DataFrame, cast per column to float32 like pygemma_multi's; W (n, c), c = 1..30 (bring your own
    intercept), c + t <= 64; X (n, p): whatever lmm.kinship's streamed path takes — a PackedBed, or an int8, uint8, float32 or float64
    array in C or Fortran order, pinned or pageable — read where it lies, without a host copy or cast of the whole matrix.  Values
    are the reference's X.astype(np.float32); a missing .bed call takes the mean of the called genotypes of its SNP
    (PackedBed.to_float(impute=True)).
    In fp64 (csrc/lm.hip), with Q an orthonormal basis of span(W), y~ = y - Q Q'y and df = n - c - 1:
      sxx = x'x - |Q'x|^2, sxy = x'y~, rss = y~'y~ - sxy^2/sxx
      beta = sxy/sxx, se_beta = sqrt(rss/(df sxx)), tau = df/rss     (float32)
      F_wald = df sxy^2/(sxx rss), p_wald = F(1, df).sf(F_wald)      (float64)
    One phenotype returns the DataFrame beta, se_beta, tau, F_wald, p_wald[, SNPs] (no lambda column); several return a dict in
    column order {label: frame}, keyed like pygemma_multi's, each frame bit-identical to the one-column call.  A SNP that is constant
    or in span(W) (sxx <= 1e-10 x'x), holds a NaN/Inf or is an all-missing .bed record gets NaN rows for every phenotype; a
    rank-deficient or non-finite W gives NaN everywhere; a non-finite phenotype NaN in its own frame only.
    SNP batches of `snp_batch` columns (default: from n and the free device memory) are uploaded on a second stream into two device
    slots, one batch ahead of the kernels; the results stay on the device until one download at the end, and do not depend on the
    batch boundaries.  `stats` receives batches, bytes_in, seconds and lambda_gc — per phenotype, median(chi2.isf(p_wald, 1)) /
    chi2.ppf(0.5, 1) over the non-NaN rows, as run_lin_reg.py computes it.  Refused with ValueError before any device work: shape
    mismatches, X not 2-D or of another dtype, W with other than 1..30 columns, c + t > 64, n - c - 1 <= 0, a bad snp_batch."""
    _check_snp_batch(snp_batch)
    X = _genotypes(X, "pygemma_lm")
    n, p = X.shape
    W = np.asarray(W)
    if W.ndim != 2 or not 1 <= W.shape[1] <= 30:
        raise ValueError(f"the linear model takes W with 1 to 30 columns, got W {W.shape}")
    labels, cols = _pheno_columns(Y)
    Yt = np.stack(cols)                                      # (t, n): phenotype-major rows
    t, c = len(labels), W.shape[1]
    if W.shape[0] != n or Yt.shape[1] != n:
        raise ValueError(f"shape mismatch: Y has {Yt.shape[1]} rows, X {n}, W {W.shape[0]}")
    if c + t > 64:
        raise ValueError(f"the linear model takes c + t <= 64 panel columns, got c = {c}, t = {t}")
    if n - c - 1 <= 0:
        raise ValueError(f"the linear model needs n - c - 1 > 0 (n = {n}, c = {c})")
    if snps is not None and len(snps) != p:
        raise ValueError(f"shape mismatch: {len(snps)} SNP names for {p} SNPs")
    W = np.ascontiguousarray(W.astype(np.float32))           # lmm.py:118-119
    out = _lm_stream(X, W, Yt, device, snp_batch, verbose, stats)
    frames = {lab: _frame(out, _LM_COLS, snps, k) for k, lab in enumerate(labels)}
    if stats is not None:
        from scipy import stats as _sps      # lazily, as model.py does
        lam = []
        for k in range(t):
            pv = out["p_wald"][k]
            pv = pv[~np.isnan(pv)]
            lam.append(float(np.median(_sps.chi2.isf(pv, 1)) / _CHI2_MEDIAN) if pv.size else float("nan"))
        stats["lambda_gc"] = lam
    return frames[labels[0]] if t == 1 else frames


def _lm_stream(X, W, Yt, device, snp_batch, verbose, stats):
    """The streamed linear-model scan: pg_lm_setup_dev once, then SNP batches from the feed (_feed._Feed) through
    pg_lm_{bed,x}_dev into windows of the (t, p) result arrays on the device.  Returns the five (t, p) host arrays."""
    L, t0 = _lib.load(), time.time()
    src = _describe(X)
    (t, n), c, p = Yt.shape, W.shape[1], src.p
    _gpus()
    with _lib.Context(device) as ctx, contextlib.closing(_Feed(ctx, src)) as feed:
        fixed = int(L.pg_lm_work_bytes(n, c, t)) + 28 * t * max(p, 1) + 4 * n * (c + t)
        pb = _fit_batch(ctx, snp_batch, _lm_batch(src), max(p, 1), 128, lambda pb: fixed + 2 * pb * src.row_bytes,
                        f"pygemma_lm: n={n}, p={p}, t={t}", f"panel, {t} x {p} result rows, two batch slots")
        dW, dY = ctx.to_device(W), ctx.to_device(Yt)
        work = ctx.alloc(L.pg_lm_work_bytes(n, c, t))
        _lib.check(L.pg_lm_setup_dev(ctx.handle, n, c, t, dW.ptr, dY.ptr, n, work.ptr), "pg_lm_setup_dev")
        res = [ctx.alloc(max(t * p, 1) * (4 if k < 3 else 8)) for k in range(5)]
        for s, e, slot in feed.batches(pb):
            win = [r.ptr + s * (4 if j < 3 else 8) for j, r in enumerate(res)]      # SNPs [s, e) of every phenotype's row: ldo = p
            _call_dev(L, "pg_lm_{}_dev", src, (ctx.handle, n, c, t, e - s), slot, e - s, (work.ptr, *win, p))
            _log(verbose - 1, f"linear model: SNPs [{s},{e}) queued")
        ctx.sync()
        out = {col: r.download((t, p), np.float32 if j < 3 else np.float64) for j, (col, r) in enumerate(zip(_LM_COLS, res))}
    _stream_stats(stats, src, pb, t0)
    _log(verbose, f"Linear model: {p} SNPs x {t} phenotype(s) with {n} individuals in {time.time() - t0:.3f} s")
    return out


_STAT_COLS = ("n_obs", "n_miss", "n0", "n1", "n2", "miss", "mean", "var", "min", "max", "af", "maf", "hwe_p")


def snp_stats(X, snps=None, hwe=True, device=0, snp_batch=None, verbose=0, stats=None):
    """Per-SNP quality control from the raw genotypes, read once where they lie: what GEMMA prints as n_miss and af and filters on with
    -miss, -maf and -hwe (calculate_allele_frequency_matrix and the MAF mask of the reference's callers, without a host pass).

    X (n, p): whatever pygemma_lm takes — a PackedBed, or an int8, uint8, float32 or float64 array in C or Fortran order, pinned or
    pageable — streamed in SNP batches of `snp_batch` columns through the two-slot feed; the results stay on the device until one
    download at the end and do not depend on the batch boundaries.  Values are the scans' (float64 rounded to float32 per element); a
    .bed code 01 and a NaN or +-Inf are missing, an 8-bit array has no missing code.  Returns a DataFrame of p rows (csrc/snp_stats.hip):
      n_obs, n_miss, n0, n1, n2 (int64)  observed and missing calls; observed values that are exactly 0, 1, 2
      miss                               n_miss / n
      mean, var, min, max                of the observed values, var with ddof = 0; NaN with n_obs = 0.  A hard-call SNP
                                         (n0 + n1 + n2 == n_obs) takes mean and var from the integer counts, one exact division each
      af                                 mean / 2 where 0 <= min and max <= 2, else NaN (centred or standardised input has no allele
                                         frequency): the frequency of the allele the input counts, A2 for a PackedBed unless count_A1
      maf                                min(af, 1 - af)
      hwe_p                              the exact Hardy-Weinberg test (Wigginton et al. 2005, two-sided) on n0, n1, n2; NaN for a SNP
                                         that is not hard-call or has no observed call; the column is absent with hwe=False
      SNPs                               `snps`, when given
    `stats` receives batches, bytes_in, seconds.  Refused with ValueError before any device work: X not 2-D or of another dtype, an
    empty X, `snps` of another length, a bad snp_batch.  snp_filter(st) turns the frame into GEMMA's default mask."""
    _check_snp_batch(snp_batch)
    X = _genotypes(X, "snp_stats")
    n, p = X.shape
    if n < 1 or p < 1:
        raise ValueError(f"snp_stats needs at least one sample and one SNP: X holds n={n}, p={p}")
    if snps is not None and len(snps) != p:
        raise ValueError(f"shape mismatch: {len(snps)} SNP names for {p} SNPs")
    cnt, mom, pv = _snp_stats_stream(X, bool(hwe), device, snp_batch, verbose, stats)
    out = {"n_obs": n - cnt[:, 0], "n_miss": cnt[:, 0], "n0": cnt[:, 1], "n1": cnt[:, 2], "n2": cnt[:, 3], "miss": cnt[:, 0] / float(n),
           "mean": mom[:, 0], "var": mom[:, 1], "min": mom[:, 2], "max": mom[:, 3]}
    out["af"] = np.where((out["min"] >= 0) & (out["max"] <= 2), out["mean"] / 2, np.nan)
    out["maf"] = np.minimum(out["af"], 1 - out["af"])
    out["hwe_p"] = pv
    return _frame(out, _STAT_COLS if hwe else _STAT_COLS[:-1], snps)


def _snp_stats_stream(X, hwe, device, snp_batch, verbose, stats):
    """The streamed QC pass: SNP batches from the feed (_feed._Feed) through pg_snp_stats_{bed,x}_dev into windows of the (p, 4) count
    and moment arrays on the device, then pg_hwe_exact_dev on all p rows.  Returns the host arrays (counts, moments, hwe_p or None)."""
    L, t0 = _lib.load(), time.time()
    src = _describe(X)
    n, p = src.n, src.p
    _gpus()
    with _lib.Context(device) as ctx, contextlib.closing(_Feed(ctx, src)) as feed:
        # only a sample-major block has chunk partials: records and SNP-major columns leave the work area untouched
        work_bytes = (lambda pb: 256) if src.snp_major else (lambda pb: int(L.pg_snp_stats_work_bytes(n, pb)))
        pb = _fit_batch(ctx, snp_batch, _lm_batch(src), p, 128, lambda pb: 72 * p + 2 * pb * src.row_bytes + work_bytes(pb),
                        f"snp_stats: n={n}, p={p}", "72 p bytes of results, two batch slots, chunk partials of a sample-major source")
        work = ctx.alloc(work_bytes(pb))
        dc, dm = ctx.alloc(32 * p), ctx.alloc(32 * p)
        for s, e, slot in feed.batches(pb):
            _call_dev(L, "pg_snp_stats_{}_dev", src, (ctx.handle, n, e - s), slot, e - s, (work.ptr, dc.ptr + 32 * s, dm.ptr + 32 * s))
            _log(verbose - 1, f"snp_stats: SNPs [{s},{e}) queued")
        if hwe:
            dp = ctx.alloc(8 * p)
            _lib.check(L.pg_hwe_exact_dev(ctx.handle, n, p, dc.ptr, dp.ptr), "pg_hwe_exact_dev")
        ctx.sync()
        out = dc.download((p, 4), np.int64), dm.download((p, 4), np.float64), dp.download((p,), np.float64) if hwe else None
    _stream_stats(stats, src, pb, t0)
    _log(verbose, f"SNP statistics: {p} SNPs with {n} individuals in {time.time() - t0:.3f} s")
    return out


def snp_filter(st, maf=0.01, miss=0.05, hwe=0.0):
    """The boolean keep-mask GEMMA's filters give (defaults: -maf 0.01, -miss 0.05, no -hwe) on a frame of snp_stats; pure NumPy.  A SNP
    stays with miss <= `miss`, var > 0 (polymorphic, at least one observed call), maf >= `maf` (a NaN maf fails unless `maf` is 0) and,
    when `hwe` > 0, hwe_p >= `hwe` or hwe_p NaN (no test: not hard-call).  Equality keeps the SNP.  Hand the mask to PackedBed.take or
    index the columns of X with it."""
    keep = (st["miss"].to_numpy() <= miss) & (st["var"].to_numpy() > 0)
    if maf != 0:
        keep &= st["maf"].to_numpy() >= maf
    if hwe > 0:
        if "hwe_p" not in st:
            raise ValueError("snp_filter(hwe > 0) needs the hwe_p column: call snp_stats with hwe=True")
        pv = st["hwe_p"].to_numpy()
        keep &= (pv >= hwe) | np.isnan(pv)
    return keep


# ---- linkage disequilibrium (csrc/ld.hip) ------------------------------------------------------------------------------------
_LD_BATCH = 8192     # SNPs per batch of the LD streams by default: with the carry of `window` SNPs the image holds 3 n bytes per SNP


def _ld_source(X, who):
    X = _genotypes(X, who)
    if X.shape[0] < 1 or X.shape[1] < 1:
        raise ValueError(f"{who} needs at least one sample and one SNP: X holds n={X.shape[0]}, p={X.shape[1]}")
    return X


def _ld_take(X, index):
    """The SNPs `index` of a genotype source (a mask or integer indices, checked as PackedBed.take checks them; None: all of them) and
    their columns in X: a PackedBed over the selected records, or the selected columns of an array."""
    p = X.shape[1]
    if index is None:
        return X, np.arange(p, dtype=np.int64)
    idx = np.asarray(index)
    if idx.dtype == np.bool_:
        if idx.shape != (p,):
            raise ValueError(f"a mask over {p} SNPs has shape ({p},), not {idx.shape}")
        idx = np.flatnonzero(idx)
    else:
        if idx.ndim != 1 or (idx.size and idx.dtype.kind not in "iu"):
            raise ValueError("index must be a boolean mask of length p or a 1-D array of integer SNP indices")
        idx = idx.astype(np.int64)
        if idx.size and (idx.min() < -p or idx.max() >= p):
            raise ValueError(f"SNP index out of range for {p} SNPs")
        idx = np.where(idx < 0, idx + p, idx)
    if idx.size < 1:
        raise ValueError("the selection holds no SNP")
    return (X.take(idx) if isinstance(X, PackedBed) else np.ascontiguousarray(X[:, idx])), idx


def _check_unit(**kw):
    for name, v in kw.items():
        if not (isinstance(v, (int, float, np.integer, np.floating)) and 0 <= v <= 1):
            raise ValueError(f"{name} must lie in [0, 1], not {v!r}")


def _check_window(window):
    if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or window < 1:
        raise ValueError(f"window must be a positive integer, not {window!r}")


def _ld_encode(L, ctx, src, pb, image, pe):
    """All SNPs of `src` through the feed into positions [0, src.p) of an LD image for pe SNPs."""
    with contextlib.closing(_Feed(ctx, src)) as feed:
        for s, e, slot in feed.batches(pb):
            _call_dev(L, "pg_ld_encode_{}_dev", src, (ctx.handle, src.n, e - s), slot, e - s, (image.ptr, pe, s))


def ld(X, a=None, b=None, *, counts=False, device=0, stats=None):
    """The LD matrix of a region: the float32 matrix r of shape (len(a), len(b)) of genotype correlations between the SNPs `a` and `b` of
    X, each over the samples where both are called (the pairwise-complete Pearson r, PLINK's --r), for fine-mapping or a regional plot.

    X (n, p): whatever snp_stats takes — a PackedBed, or an int8, uint8, float32 or float64 array in C or Fortran order, pinned or
    pageable.  `a` and `b` are boolean masks of length p or integer indices, as for PackedBed.take; None is every SNP, and b=None is
    b = a.  Only the selected SNPs are uploaded (through the two-slot feed), encoded into int8 planes on the device and multiplied on
    the int8 matrix pipe (csrc/ld.hip).  Hard calls only: a SNP with an observed value other than 0, 1, 2 (a dosage, a centred column,
    an int8 -1) counts as all missing; missing is .bed code 01, NaN or +-Inf.  From the six int32 sums of a pair
      N = sum m_a m_b, Sa = sum x_a m_b, Sb = sum m_a x_b, Saa = sum x_a^2 m_b, Sbb = sum m_a x_b^2, Sab = sum x_a x_b
      r = (N Sab - Sa Sb) / sqrt((N Saa - Sa^2)(N Sbb - Sb^2)), the products exact in int64, clamped to [-1, 1], one rounding to float32;
    NaN when either variance is not positive (no jointly called sample, or a SNP monomorphic among them).  A copy of a SNP gives
    exactly 1.0, its flip 2 - x exactly -1.0.  `counts=True` returns (r, sums) with the (len(a), len(b), 6) int32 sums in that order.
    `stats` receives bytes_in and seconds.  Images and output that do not fit the device raise PgError.  Refused with ValueError before
    any device work: X not 2-D or of another dtype, an empty X, a mask of another length, an index out of range, an empty selection."""
    t0 = time.time()
    X = _ld_source(X, "ld")
    XA, ia = _ld_take(X, a)
    XB, ib = (XA, ia) if b is None else _ld_take(X, b)
    L = _lib.load()
    _gpus()
    sa, sb = _describe(XA), _describe(XB)
    n, na, nb = sa.n, sa.p, sb.p
    with _lib.Context(device) as ctx:
        fixed = int(L.pg_ld_image_bytes(n, na)) + (0 if XB is XA else int(L.pg_ld_image_bytes(n, nb))) + na * nb * (28 if counts else 4)
        pbs = [_fit_batch(ctx, None, _lm_batch(s), s.p, 128, lambda pb: fixed + 2 * pb * s.row_bytes, f"ld: n={n}, {na} x {nb} SNPs",
                          "int8 images 3 n bytes per SNP, the r matrix, two batch slots") for s in (sa, sb)]
        imA = ctx.alloc(L.pg_ld_image_bytes(n, na))
        _ld_encode(L, ctx, sa, pbs[0], imA, na)
        imB = imA
        if XB is not XA:
            imB = ctx.alloc(L.pg_ld_image_bytes(n, nb))
            _ld_encode(L, ctx, sb, pbs[1], imB, nb)
        dr = ctx.alloc(4 * na * nb)
        ds = ctx.alloc(24 * na * nb) if counts else None
        _lib.check(L.pg_ld_block_dev(ctx.handle, n, imA.ptr, na, 0, na, imB.ptr, nb, 0, nb, dr.ptr, nb, ds.ptr if counts else None), "pg_ld_block_dev")
        ctx.sync()
        r = dr.download((na, nb), np.float32)
        sums = ds.download((na, nb, 6), np.int32) if counts else None
    if stats is not None:
        stats.update({"bytes_in": na * sa.row_bytes + (0 if XB is XA else nb * sb.row_bytes), "seconds": time.time() - t0})
    return (r, sums) if counts else r


def ld_window(X, window, *, snp_batch=None, device=0, verbose=0, stats=None):
    """The LD band of X: the (p, window) float32 matrix band[j, k] = r(j, j + 1 + k), the correlation (as `ld` defines it) of every SNP
    with its next `window` SNPs; NaN where j + 1 + k >= p.  What ld_prune and clump read.

    X as for `ld`.  Streamed in SNP batches of `snp_batch` columns through the two-slot feed into ONE device image of snp_batch + window
    SNPs: a batch is encoded behind the carry of the previous ones, the band rows whose whole window is present are computed (the last
    batch computes the rest), and the last `window` SNPs move to the front; `window` may exceed `snp_batch`.  The band stays on the
    device until one download at the end when it fits there, else it comes back batch by batch.  The result does not depend on the
    batch boundaries, bit for bit (the sums are integers).  `stats` receives batches, bytes_in, seconds.  Refused with ValueError
    before any device work: X not 2-D or of another dtype, an empty X, window < 1, a bad snp_batch."""
    _check_snp_batch(snp_batch)
    _check_window(window)
    X = _ld_source(X, "ld_window")
    L, t0 = _lib.load(), time.time()
    src = _describe(X)
    n, p, w = src.n, src.p, int(window)
    _gpus()
    out = None
    with _lib.Context(device) as ctx, contextlib.closing(_Feed(ctx, src)) as feed:
        free, _total = ctx.mem_info()
        image_bytes = lambda pb: int(L.pg_ld_image_bytes(n, pb + w))
        resident = 4 * p * w + image_bytes(128) + 2 * 128 * src.row_bytes <= 0.9 * free
        out_bytes = (lambda pb: 4 * p * w) if resident else (lambda pb: 4 * (pb + w) * w)
        pb = _fit_batch(ctx, snp_batch, min(_LD_BATCH, _lm_batch(src)), p, 128, lambda pb: out_bytes(pb) + image_bytes(pb) + 2 * pb * src.row_bytes,
                        f"ld_window: n={n}, p={p}, window={w}", "the band or a batch of it, an int8 image of snp_batch + window SNPs, two batch slots")
        pe = pb + w
        image = ctx.alloc(image_bytes(pb))
        dband = ctx.alloc(out_bytes(pb))
        if not resident:
            out = np.empty((p, w), np.float32)
        base = have = emitted = 0          # the image holds SNPs [base, base + have); band rows [0, emitted) are computed
        for s, e, slot in feed.batches(pb):
            _call_dev(L, "pg_ld_encode_{}_dev", src, (ctx.handle, n, e - s), slot, e - s, (image.ptr, pe, have))
            have += e - s
            rows = (p if e == p else max(emitted, base + have - w)) - emitted
            if rows > 0:
                dst = dband.ptr + (4 * emitted * w if resident else 0)
                _lib.check(L.pg_ld_band_dev(ctx.handle, n, image.ptr, pe, emitted - base, rows, have, w, dst, w, None), "pg_ld_band_dev")
                if not resident:
                    ctx.sync()
                    out[emitted:emitted + rows] = dband.download((rows, w), np.float32)
                emitted += rows
            keep = base + have - emitted       # the SNPs whose rows are still to come: at most `window`
            if e < p and have > keep:
                _lib.check(L.pg_ld_shift_dev(ctx.handle, n, image.ptr, pe, have - keep, keep), "pg_ld_shift_dev")
                base, have = base + have - keep, keep
            _log(verbose - 1, f"ld_window: SNPs [{s},{e}) queued")
        ctx.sync()
        if resident:
            out = dband.download((p, w), np.float32)
    _stream_stats(stats, src, pb, t0)
    _log(verbose, f"LD band: {p} SNPs x window {w} with {n} individuals in {time.time() - t0:.3f} s")
    return out


def _in_ld(r, r2):
    """float64(r)^2 >= r2; a NaN pair is not in LD."""
    with np.errstate(invalid="ignore"):
        return np.asarray(r, np.float64) ** 2 >= r2


def _prune_band(band, r2):
    """The greedy forward pruning on a (p, window) band: SNP j stays unless a KEPT SNP i in [j - window, j) is in LD with it
    (band[i, j - i - 1]^2 >= r2).  Pure NumPy; returns the boolean keep-mask."""
    band = np.asarray(band)
    p, w = band.shape
    hit = _in_ld(band, r2)
    keep = np.ones(p, bool)
    for j in range(1, p):
        i = np.arange(max(0, j - w), j)
        keep[j] = not (keep[i] & hit[i, j - i - 1]).any()
    return keep


def ld_prune(X, window=50, r2=0.5, **stream_kw):
    """LD pruning before lmm.kinship: a boolean keep-mask over the SNPs of X for PackedBed.take, X[:, keep] or kinship, so that no two
    kept SNPs within `window` SNPs of each other have r^2 >= `r2`.  Greedy, front to back: SNP j is kept unless some KEPT SNP i in
    [j - window, j) is in LD with it, r as `ld` defines it, float64(r)^2 >= r2, a NaN r never in LD.  The band comes from
    ld_window(X, window, **stream_kw) (snp_batch, device, verbose, stats); the decision is the pure-NumPy _prune_band.
    Against PLINK's --indep-pairwise window step r2: no minor-allele-frequency choice of which SNP of a pair goes (always the later
    one), no step parameter (the window slides by one SNP), and every pair within the window is looked at once.  Monomorphic and
    all-missing SNPs have no r and are KEPT: removing them is snp_filter's job.  Refused with ValueError before any device work: what
    ld_window refuses, r2 outside [0, 1]."""
    _check_unit(r2=r2)
    return _prune_band(ld_window(X, window, **stream_kw), r2)


def _signed(coord):
    """Coordinates in a type whose differences have a sign: int64 for integers (an unsigned difference would wrap), float64 else."""
    coord = np.asarray(coord)
    return coord.astype(np.int64 if coord.dtype.kind in "iub" else np.float64)


def _check_span(window, pos):
    """A window in columns is a positive integer; one in the units of `pos` any number of at least 1."""
    if pos is None:
        _check_window(window)
    elif not (isinstance(window, (int, float, np.integer, np.floating)) and window >= 1):
        raise ValueError(f"window must be at least 1, not {window!r}")


def _coords(p, chrom, pos):
    """(coord, run) of p SNPs: the coordinate a window is measured in (`pos`, checked; the column without it) and the number of the
    chromosome run a SNP lies in (a window never crosses a change of `chrom`)."""
    run = np.zeros(p, np.int64)
    if chrom is not None:
        chrom = np.asarray(chrom)
        if chrom.shape != (p,):
            raise ValueError(f"shape mismatch: chrom has shape {chrom.shape} for {p} SNPs")
        run[1:] = np.cumsum(chrom[1:] != chrom[:-1])
    coord = np.arange(p, dtype=np.int64)
    if pos is not None:
        coord = np.asarray(pos)
        if coord.shape != (p,) or coord.dtype.kind not in "iuf":
            raise ValueError(f"shape mismatch: pos must be {p} numbers, got shape {coord.shape} of {coord.dtype}")
        if coord.dtype.kind == "u" and coord.size and coord.max() > np.iinfo(np.int64).max:
            raise ValueError("pos does not fit int64")
        coord = _signed(coord)
        if ((np.diff(coord) < 0) & (run[1:] == run[:-1])).any() or not np.isfinite(coord).all():
            raise ValueError("pos must be finite and nondecreasing within a chromosome")
    return coord, run


def _clump_reach(coord, run, window):
    """For candidate c, in column order, the number of later candidates of its chromosome run within `window` of it; the largest is
    the band width clumping (or an LD score) needs.  Integer coordinates (columns, base pairs; nondecreasing within a run, as the
    callers check) are bisected run by run; any other (centimorgans) walk two pointers in a Python loop, O(p) interpreted steps."""
    coord, run, m = _signed(coord), np.asarray(run), len(coord)
    reach = np.zeros(m, np.int64)
    if coord.dtype.kind == "i" and m:
        top = np.iinfo(np.int64).max
        span = int(min(np.floor(window), top))
        starts = np.flatnonzero(np.concatenate([[True], run[1:] != run[:-1]]))
        for s, e in zip(starts, np.concatenate([starts[1:], [m]])):
            seg = coord[s:e]
            last = seg + np.minimum(span, top - np.maximum(seg, 0))      # the furthest coordinate in reach, without wrapping int64
            reach[s:e] = np.searchsorted(seg, last, side="right") - 1 - np.arange(e - s)
        return reach
    hi = 0
    for c in range(m):
        hi = max(hi, c)
        while hi + 1 < m and run[hi + 1] == run[c] and coord[hi + 1] - coord[c] <= window:
            hi += 1
        reach[c] = hi - c
    return reach


def _clump_band(band, pv, coord, run, p1, r2, window):
    """The greedy clumping of m candidates (in column order) on their (m, w) band: by ascending p, ties by position, an unclumped
    candidate with p <= p1 becomes an index SNP and takes every unclumped candidate of its chromosome run within `window` (in `coord`)
    that is in LD with it.  Pure NumPy; returns [(index candidate, array of member candidates)] in the order the clumps were made."""
    band, pv, coord, run = np.asarray(band), np.asarray(pv, np.float64), _signed(coord), np.asarray(run)
    m, w = len(pv), band.shape[1] if band.ndim == 2 else 0
    hit = _in_ld(band, r2) if w else np.zeros((m, 0), bool)
    taken = np.zeros(m, bool)
    out = []
    for c in np.lexsort((np.arange(m), pv)):
        if taken[c] or not pv[c] <= p1:
            continue
        taken[c] = True
        lo = np.arange(max(0, c - w), c)
        up = np.arange(c + 1, min(m, c + 1 + w))
        near = np.concatenate([lo, up])
        linked = np.concatenate([hit[lo, c - lo - 1], hit[c, up - c - 1]]) if w else np.zeros(0, bool)
        ok = linked & ~taken[near] & (run[near] == run[c]) & (np.abs(coord[near] - coord[c]) <= window)
        members = near[ok]
        taken[members] = True
        out.append((int(c), members.astype(np.int64)))
    return out


def clump(df, X, p1=1e-4, p2=1e-2, r2=0.5, window=250, col="p_wald", chrom=None, pos=None, **stream_kw):
    """PLINK-style clumping of a scan frame into independent loci: df is the frame of a scan over the p SNPs of X (pygemma, pygemma_lm,
    ...), `col` its p-value column.  Candidates are the rows with p < p2 (a NaN p is never one); only their SNPs are uploaded.  By
    ascending p, ties by column, an unclumped candidate with p <= p1 becomes an index SNP and takes every unclumped candidate within
    `window` that is in LD with it (r as `ld` defines it, float64(r)^2 >= r2, NaN never in LD).  Distance is |i - j| in columns of X,
    or |pos_i - pos_j| when `pos` (length p, nondecreasing within a chromosome) is given; with `chrom` (length p, the SNPs of one
    chromosome adjacent) a clump never crosses a change of chromosome.  The band width over the candidates is found on the host and
    ld_window(candidates, width, **stream_kw) gives their r.
    Returns a frame sorted by p, one row per clump: index (column of X), SNPs (when df has it), p, n_members, members (int64 array of
    the columns of X the index SNP took, without itself).  The greedy is the pure-NumPy _clump_band.  Refused with ValueError before any
    device work: what ld_window refuses, thresholds outside [0, 1], window < 1, `col` missing, lengths of df, chrom, pos that are not
    p, pos decreasing within a chromosome."""
    _check_unit(p1=p1, p2=p2, r2=r2)
    _check_span(window, pos)
    _check_snp_batch(stream_kw.get("snp_batch"))
    X = _ld_source(X, "clump")
    p = X.shape[1]
    if col not in df:
        raise ValueError(f"the frame has no column {col!r}")
    pv = np.asarray(df[col], np.float64)
    if pv.shape != (p,):
        raise ValueError(f"shape mismatch: {len(pv)} rows of p-values for {p} SNPs")
    coord, run = _coords(p, chrom, pos)
    with np.errstate(invalid="ignore"):
        cand = np.flatnonzero(pv < p2)
    width = int(_clump_reach(coord[cand], run[cand], window).max()) if cand.size else 0
    if width > 0:
        band = ld_window(_ld_take(X, cand)[0], width, **stream_kw)
    else:
        band = np.zeros((cand.size, 0), np.float32)
    clumps = _clump_band(band, pv[cand], coord[cand], run[cand], p1, r2, window)
    clumps.sort(key=lambda cm: (pv[cand[cm[0]]], cm[0]))
    out = {"index": np.array([cand[c] for c, _ in clumps], np.int64)}
    if "SNPs" in df:
        out["SNPs"] = np.asarray(df["SNPs"], object)[out["index"]]
    out["p"] = pv[out["index"]]
    out["n_members"] = np.array([len(mem) for _, mem in clumps], np.int64)
    res = pd.DataFrame(out, columns=list(out))
    res["members"] = pd.Series([cand[mem] for _, mem in clumps], dtype=object, index=res.index)
    return res


# ---- LD scores and LD score regression (csrc/ld.hip) ----------------------------------------------------------------------
_LDS_COLS = ("l2", "n_pairs", "n_obs", "reach_fwd")
_LDS_MAX_W = 1 << 28     # pg_ld_score_dev: a SNP's 2 w pairs of at most 2^32 each stay inside int64
_CHI2_1DF_MEDIAN = 0.454936423119572     # the median of a chi-square with one degree of freedom


def ld_scores(X, window, *, pos=None, chrom=None, adjust=True, snps=None, snp_batch=None, device=0, verbose=0, stats=None):
    """The LD score of every SNP of X, l2_j = 1 + sum of r^2(j, k) over the other SNPs k of its window: the regressor of LD score
    regression (`ldsc`), which tells confounding (intercept) from polygenicity (slope) in an inflated lambda_GC.

    X as for `ld_window`.  The window is `clump`'s: the partners of SNP j are the SNPs with |i - j| <= window in columns of X, or
    |pos_i - pos_j| <= window when `pos` (length p, nondecreasing within a chromosome; base pairs or centimorgans) is given, and never
    beyond a change of `chrom` (length p, the SNPs of one chromosome adjacent).  r is the pairwise-complete correlation `ld` defines; a
    pair counts when both variances over its jointly called samples are positive and, with `adjust`, N > 2 of them are called.  In
    fp64, r2 = min(cab^2 / (ca cb), 1), with `adjust` (the default, as ldsc estimates LD scores) less the bias (1 - r2) / (N - 2) with
    the pair's own N, then rounded to fixed point at 2^-32 and summed in int64 on the device: the result is the same bits whatever the
    batches, the storage of X or the order of the tiles.  The SNP's own r^2 = 1 is the leading 1, not adjusted.
    Streamed like ld_window (one image of snp_batch + w SNPs, w the largest forward reach found on the host by _clump_reach), but every
    tile's pairs are reduced in the kernel (pg_ld_score_dev): 16 bytes per SNP stay on the device until one download at the end, where
    the band would be 4 w.  Returns a DataFrame of p rows:
      l2         float64; NaN for a SNP without variance of its own (monomorphic, all missing, not hard-call: n_obs = 0)
      n_pairs    int64, the pairs that counted, on both sides of the SNP
      n_obs      int64, the SNP's called samples, 0 as above
      reach_fwd  int64, the later SNPs inside the SNP's window
      SNPs       `snps`, when given
    `stats` receives batches, bytes_in, seconds and w.  Refused with ValueError before any device work: what ld_window and clump
    refuse for these arguments (X, snp_batch, chrom, pos), `snps` of another length, a window that is not at least 1 or, without
    `pos`, not an integer, a reach of 2^28 SNPs or more."""
    _check_snp_batch(snp_batch)
    _check_span(window, pos)
    X = _ld_source(X, "ld_scores")
    p = X.shape[1]
    if snps is not None and len(snps) != p:
        raise ValueError(f"shape mismatch: {len(snps)} SNP names for {p} SNPs")
    coord, run = _coords(p, chrom, pos)
    reach = _clump_reach(coord, run, window)
    w = int(reach.max())
    if w >= _LDS_MAX_W:
        raise ValueError(f"a window of {w} SNPs is more than the int64 sums hold (2^28 at most)")
    L, t0 = _lib.load(), time.time()
    src = _describe(X)
    n, wk = src.n, max(w, 1)          # w = 0 (one SNP, or every reach 0): the kernel still writes n_obs
    _gpus()
    with _lib.Context(device) as ctx, contextlib.closing(_Feed(ctx, src)) as feed:
        image_bytes = lambda pb: int(L.pg_ld_image_bytes(n, pb + wk))
        pb = _fit_batch(ctx, snp_batch, min(_LD_BATCH, _lm_batch(src)), p, 128, lambda pb: 20 * p + image_bytes(pb) + 2 * pb * src.row_bytes,
                        f"ld_scores: n={n}, p={p}, window of {w} SNPs", "20 p bytes of sums and reach, an int8 image of snp_batch + window SNPs, two batch slots")
        pe = pb + wk
        image = ctx.alloc(image_bytes(pb))
        dsum, dnp, dno = ctx.alloc(8 * p), ctx.alloc(4 * p), ctx.alloc(4 * p)
        dreach = ctx.to_device(reach.astype(np.int32))
        for buf in (dsum, dnp, dno):
            _lib.check(L.pg_memset(ctx.handle, buf.ptr, 0, buf.nbytes), "pg_memset")
        base = have = emitted = 0          # the image holds SNPs [base, base + have); rows [0, emitted) have met their forward partners
        for s, e, slot in feed.batches(pb):
            _call_dev(L, "pg_ld_encode_{}_dev", src, (ctx.handle, n, e - s), slot, e - s, (image.ptr, pe, have))
            have += e - s
            rows = (p if e == p else max(emitted, base + have - wk)) - emitted
            if rows > 0:
                _lib.check(L.pg_ld_score_dev(ctx.handle, n, image.ptr, pe, emitted - base, rows, have, wk, dreach.ptr + 4 * base, int(bool(adjust)),
                                             dsum.ptr + 8 * base, dnp.ptr + 4 * base, dno.ptr + 4 * base), "pg_ld_score_dev")
                emitted += rows
            keep = base + have - emitted       # the SNPs whose rows are still to come: at most the largest reach
            if e < p and have > keep:
                _lib.check(L.pg_ld_shift_dev(ctx.handle, n, image.ptr, pe, have - keep, keep), "pg_ld_shift_dev")
                base, have = base + have - keep, keep
            _log(verbose - 1, f"ld_scores: SNPs [{s},{e}) queued")
        ctx.sync()
        tot, npairs, nobs = dsum.download((p,), np.int64), dnp.download((p,), np.int32), dno.download((p,), np.int32)
    _stream_stats(stats, src, pb, t0)
    if stats is not None:
        stats["w"] = w
    _log(verbose, f"LD scores: {p} SNPs, window of {w} SNPs, with {n} individuals in {time.time() - t0:.3f} s")
    out = {"l2": np.where(nobs > 0, 1.0 + tot / 2.0 ** 32, np.nan), "n_pairs": npairs.astype(np.int64), "n_obs": nobs.astype(np.int64),
           "reach_fwd": reach}
    return _frame(out, _LDS_COLS, snps)


LdscResult = namedtuple("LdscResult", "h2 h2_se intercept intercept_se mean_chi2 lambda_gc ratio m n_used")


def _ldsc_sums(x, y, wt, edges):
    """Per block [edges[b], edges[b + 1]) the weighted sums a line fit needs: columns w, w x, w x^2, w y, w x y."""
    terms = np.stack([wt, wt * x, wt * x * x, wt * y, wt * x * y], axis=1)
    return np.add.reduceat(terms, edges[:-1], axis=0)


def _ldsc_solve(S, a):
    """(slope, intercept) of the weighted line from rows of sums (_ldsc_sums); with a fixed intercept `a` the slope of y - a through 0."""
    sw, sx, sxx, sy, sxy = (S[..., t] for t in range(5))
    if a is not None:
        return (sxy - a * sx) / sxx, np.full_like(sxx, a)
    slope = (sw * sxy - sx * sy) / (sw * sxx - sx * sx)
    return slope, (sy - slope * sx) / sw


def ldsc(chi2, l2, n, *, m=None, blocks=200, intercept=None):
    """LD score regression (Bulik-Sullivan et al. 2015): E[chi2_j] = a + N_j h2 l2_j / M over the SNPs of a scan.  The intercept a
    measures confounding (population structure, cryptic relatedness: 1 without), the slope gives the SNP heritability h2; lambda_GC
    alone cannot tell the two apart.

    chi2: the 1-df association statistics of a scan frame, df["F_wald"] or (df["beta"] / df["se_beta"]) ** 2; l2: lmm.ld_scores(X,
    ...)["l2"] of the same SNPs in the same order; n: the sample size, one number or one per SNP.  The SNPs where chi2, l2 and n are
    all finite are used (n_used of them); M = `m`, or their count.  Host-only NumPy:
      start      a = 1, h2 = clip(M (mean chi2 - 1) / mean(N l2), 0, 1); with `intercept` given a is that value here too (mean chi2 - a:
                 the one place this goes beyond the written model, as ldsc does for a constrained intercept)
      weights    w_j = 1 / (max(l2_j, 1) 2 (a + N_j h2 max(l2_j, 1) / M)^2) with the current (a, h2), h2 not clipped after the
                 start: one over the LD score (correlated SNPs are counted l2 times) times the variance of a chi-square with that mean
      updates    exactly two weighted least-squares fits of (h2, a), the weights recomputed before each; with `intercept` given it
                 stays fixed and chi2 - a is regressed on N l2 / M without a constant
      errors     a delete-one block jackknife over `blocks` contiguous blocks of the used SNPs (np.array_split's sizes), the weights
                 of the last update held fixed
    Returns an LdscResult: h2, h2_se, intercept, intercept_se (NaN when fixed), mean_chi2, lambda_gc = median chi2 / 0.4549...,
    ratio = (a - 1) / (mean chi2 - 1) (the share of the inflation that is confounding; NaN at mean chi2 = 1), m, n_used.
    Refused with ValueError: inputs that are not 1-D of one length, blocks < 2 or more blocks than used SNPs, m <= 0."""
    y, ell = np.asarray(chi2, np.float64), np.asarray(l2, np.float64)
    if y.ndim != 1 or ell.shape != y.shape:
        raise ValueError(f"shape mismatch: chi2 has shape {y.shape}, l2 {ell.shape}")
    nn = np.asarray(n, np.float64)
    if nn.ndim == 0:
        nn = np.full(y.shape, float(nn))
    if nn.shape != y.shape:
        raise ValueError(f"shape mismatch: n has shape {nn.shape} for {len(y)} SNPs")
    if isinstance(blocks, bool) or not isinstance(blocks, (int, np.integer)):
        raise ValueError(f"blocks must be an integer, not {blocks!r}")
    use = np.isfinite(y) & np.isfinite(ell) & np.isfinite(nn)
    y, ell, nn = y[use], ell[use], nn[use]
    used = len(y)
    if blocks < 2 or blocks > used:
        raise ValueError(f"blocks must lie in [2, {used}] for {used} usable SNPs, not {blocks}")
    M = float(used if m is None else m)
    if not M > 0:
        raise ValueError(f"m must be positive, not {m!r}")
    fixed = None if intercept is None else float(intercept)
    x, lw = nn * ell / M, np.maximum(ell, 1.0)
    edges = np.concatenate([[0], np.cumsum([len(part) for part in np.array_split(np.arange(used), blocks)])])
    whole = np.array([0, used])
    a = 1.0 if fixed is None else fixed
    h2 = float(np.clip(M * (y.mean() - a) / (nn * ell).mean(), 0.0, 1.0))
    for _ in range(2):
        wt = 1.0 / (lw * 2.0 * (a + nn * h2 * lw / M) ** 2)
        slope, const = _ldsc_solve(_ldsc_sums(x, y, wt, whole)[0], fixed)
        h2, a = float(slope), float(const)
    S = _ldsc_sums(x, y, wt, edges)
    dh, da = _ldsc_solve(S.sum(axis=0) - S, fixed)          # the fits without block b
    se = lambda d: float(np.sqrt((blocks - 1) / blocks * ((d - d.mean()) ** 2).sum()))
    mean = float(y.mean())
    return LdscResult(h2, se(dh), a, float("nan") if fixed is not None else se(da), mean, float(np.median(y)) / _CHI2_1DF_MEDIAN,
                      (a - 1.0) / (mean - 1.0) if mean != 1.0 else float("nan"), M, used)


# ---- pairwise SNP x SNP interaction (csrc/epistasis.hip) ------------------------------------------------------------------------
EpistasisResult = namedtuple("EpistasisResult", "pairs summary chi2_min")
_EPI_P = 1e-4                  # the default cut, as the object the signature holds: `p` left alone is told from p=1e-4 given beside `chi2`
_EPI_CAP = 1 << 22             # hit records (16 bytes each) a block pair's buffer holds before the pair is rerun with the counted size
_EPI_HIT = np.dtype([("a", "<i4"), ("b", "<i4"), ("z", "<f8")])
_EPI_MAX_SNPS = 2 ** 31 - 1


def _epi_chi2_min(p, chi2):
    """The chi2 cut of an epistasis scan: `chi2` when given, else the 1-df chi2 whose upper tail is p, by bisection on erfc(z / sqrt 2) = p
    (z in [0, 40]; erfc underflows beyond) down to neighbouring doubles."""
    if chi2 is not None:
        if p is not _EPI_P:
            raise ValueError("give the cut as p or as chi2, not both")
        if isinstance(chi2, bool) or not isinstance(chi2, (int, float, np.integer, np.floating)) or not (np.isfinite(chi2) and chi2 >= 0):
            raise ValueError(f"chi2 must be a finite number >= 0, not {chi2!r}")
        return float(chi2)
    if isinstance(p, bool) or not isinstance(p, (int, float, np.integer, np.floating)) or not 0 < p <= 1:
        raise ValueError(f"p must lie in (0, 1], not {p!r}")
    lo, hi = 0.0, 40.0                          # erfc(lo / sqrt 2) >= p > erfc(hi / sqrt 2)
    if p == 1:
        return 0.0
    if math.erfc(hi / math.sqrt(2.0)) >= p:
        return hi * hi
    while True:
        mid = 0.5 * (lo + hi)
        if mid <= lo or mid >= hi:
            return lo * lo
        if math.erfc(mid / math.sqrt(2.0)) >= p:
            lo = mid
        else:
            hi = mid


def _epi_group(y, n, case_only):
    """The int8 group of every sample from a 0/1 phenotype: 1 case, 0 control, -1 (NaN) in neither."""
    y = np.asarray(y)
    if y.ndim == 2 and y.shape[1] == 1:
        y = y[:, 0]
    if y.ndim != 1 or y.shape[0] != n:
        raise ValueError(f"shape mismatch: y has shape {y.shape} for {n} samples")
    if y.dtype.kind not in "biuf":
        raise ValueError(f"y must hold 0, 1 or NaN, not dtype {y.dtype}")
    y = y.astype(np.float64)
    if not (np.isnan(y) | (y == 0) | (y == 1)).all():
        raise ValueError("y must hold 0 (control), 1 (case) or NaN (excluded) and nothing else")
    if not (y == 1).any():
        raise ValueError("y holds no case")
    if not case_only and not (y == 0).any():
        raise ValueError("y holds no control: a case/control test needs both (case_only=True tests the cases alone)")
    return np.where(y == 1, 1, np.where(y == 0, 0, -1)).astype(np.int8)


def epistasis(X, y, *, a=None, b=None, p=_EPI_P, chi2=None, case_only=False, snp_batch=None, device=0, verbose=0, stats=None):
    """Pairwise SNP x SNP interaction scan of a case/control trait: PLINK's --fast-epistasis (the allele-table odds-ratio test) over
    every pair of SNPs, on the int8 matrix pipe (csrc/epistasis.hip); only the pairs above the cut and a per-SNP summary leave the device.

    X (n, p) as for `ld`: hard calls only, a SNP with another observed value counts as all missing.  y (n,): 1 case, 0 control (bool
    allowed), NaN excluded.  `a`, `b`: masks or indices as for `ld`; the default is every pair i < j of all SNPs, `a` alone every pair
    within the selection (earlier against later in its order), with `b` given every SNP of `a` (None: all) against every SNP of `b`.
    For a pair and a group (cases, controls) the four int32 sums over the group's samples where both are called,
      N = sum m_a m_b, Sa = sum x_a m_b, Sb = sum m_a x_b, Sab = sum x_a x_b
    give the allele table A = 4N - 2Sa - 2Sb + Sab, B = 2Sb - Sab, C = 2Sa - Sab, D = Sab exactly; the group is defined when all four
    margins are positive; when a cell is 0, 1/2 is added to every cell; in fp64 L = log(A D / (B C)), v = 1/A + 1/B + 1/C + 1/D, and
    z = (L_case - L_control) / sqrt(v_case + v_control), or with `case_only` z = L_case / sqrt(v_case) (valid for SNPs in linkage
    equilibrium in the population).  chi2 = z^2 on 1 df, p = erfc(|z| / sqrt 2).  z(a, b) = z(b, a), bit for bit.
    The cut is on chi2: `chi2`, or the chi2 whose p-value is `p` (default 1e-4).  The SNPs are encoded once into a device image
    (through the two-slot feed in batches of `snp_batch`), cut into blocks of `snp_batch` SNPs (default: all of them, when they fit),
    and the block pairs I <= J are walked; a block pair with more hits than its buffer holds is rerun with a buffer of the counted size.
    Returns an EpistasisResult:
      pairs     DataFrame i, j (columns of X), z, chi2, p of the pairs with chi2 >= chi2_min, sorted by (i, j)
      summary   DataFrame, a row per SNP of the selection (`a`, then `b` when given): snp, n_tot (defined pairs it is in), n_sig (those
                above the cut), best_chi2 (float32; NaN without a defined pair), best_partner (-1 likewise; ties to the earlier
                SNP of the selection): PLINK's .epi.cc.summary
      chi2_min  the cut
    `stats` receives blocks (block pairs), reruns, pairs_defined, bytes_in, seconds.  Refused with ValueError before any device work:
    what `ld` refuses for X, `a`, `b`; y of another length or with values other than 0, 1, NaN; no case; no control unless
    `case_only`; both `p` and `chi2`; p outside (0, 1]; a negative or non-finite chi2; a bad snp_batch."""
    t0 = time.time()
    _check_snp_batch(snp_batch)
    chi2_min = _epi_chi2_min(p, chi2)
    X = _ld_source(X, "epistasis")
    group = _epi_group(y, X.shape[0], case_only)
    XA, ia = _ld_take(X, a)
    sets = b is not None
    XB, ib = _ld_take(X, b) if sets else (XA, ia)
    if len(ia) + (len(ib) if sets else 0) > _EPI_MAX_SNPS:
        raise ValueError("epistasis indexes SNPs in int32: the selection holds 2^31 or more")
    L = _lib.load()
    _gpus()
    srcs = [_describe(XA)] + ([_describe(XB)] if sets else [])
    n, na, nb = srcs[0].n, len(ia), len(ib)
    total = na + (nb if sets else 0)
    cap = int(os.environ.get("PYGEMMA_EPI_CAP", _EPI_CAP))
    nblocks = reruns = 0
    found = []
    with _lib.Context(device) as ctx:
        dgroup = ctx.to_device(group)
        images = []
        for src in srcs:
            ld_bytes, epi_bytes = int(L.pg_ld_image_bytes(n, src.p)), int(L.pg_epi_image_bytes(n, src.p))
            pb = _fit_batch(ctx, snp_batch, _lm_batch(src), src.p, 128, lambda pb: ld_bytes + epi_bytes + 2 * pb * src.row_bytes + 16 * (cap + total),
                            f"epistasis: n={n}, {src.p} SNPs", "int8 images 9 n bytes per SNP, two batch slots, the hit buffer")
            ldim = ctx.alloc(ld_bytes)
            _ld_encode(L, ctx, src, pb, ldim, src.p)
            image = ctx.alloc(epi_bytes)
            _lib.check(L.pg_epi_split_dev(ctx.handle, n, ldim.ptr, src.p, 0, src.p, dgroup.ptr, image.ptr), "pg_epi_split_dev")
            ctx.sync()
            ldim.free()
            images.append(image)
        imA, imB = images[0], images[-1]
        dcount, dhits = ctx.alloc(8), ctx.alloc(16 * max(cap, 1))
        dtot, dsig, dbest = ctx.alloc(4 * total), ctx.alloc(4 * total), ctx.alloc(8 * total)
        for buf in (dtot, dsig, dbest):
            _lib.check(L.pg_memset(ctx.handle, buf.ptr, 0, buf.nbytes), "pg_memset")
        mode = 1 if case_only else 0
        step = int(snp_batch or max(na, nb))

        def block(a0, a1, b0, b1, hits, room, per_snp):
            _lib.check(L.pg_memset(ctx.handle, dcount.ptr, 0, 8), "pg_memset")
            _lib.check(L.pg_epi_block_dev(ctx.handle, n, imA.ptr, na, a0, a1 - a0, a0, imB.ptr, nb, b0, b1 - b0, (na if sets else 0) + b0, mode,
                                          0 if sets else 1, chi2_min, dcount.ptr, hits.ptr, room, *(per_snp or (None, None, None)), None),
                       "pg_epi_block_dev")
            ctx.sync()
            return int(dcount.download((1,), np.uint64)[0])

        for a0 in range(0, na, step):
            for b0 in range(0 if sets else a0, nb, step):
                a1, b1 = min(a0 + step, na), min(b0 + step, nb)
                count = block(a0, a1, b0, b1, dhits, cap, (dtot.ptr, dsig.ptr, dbest.ptr))
                nblocks += 1
                if count > cap:                    # the counter is exact: once more with room for all, the per-SNP arrays left alone
                    big = ctx.alloc(16 * count)
                    assert block(a0, a1, b0, b1, big, count, None) == count
                    found.append(big.download((count,), _EPI_HIT))
                    big.free()
                    reruns += 1
                elif count:
                    found.append(dhits.download((count,), _EPI_HIT))
                _log(verbose - 1, f"epistasis: SNPs [{a0},{a1}) x [{b0},{b1}): {count} pairs above the cut")
        ntot, nsig, best = dtot.download((total,), np.int32), dsig.download((total,), np.int32), dbest.download((total,), np.uint64)
    rec = np.concatenate(found) if found else np.empty(0, _EPI_HIT)
    col = np.concatenate([ia, ib]) if sets else ia           # global index -> column of X
    i, j, z = col[rec["a"]], col[rec["b"]], rec["z"]
    order = np.lexsort((j, i))
    i, j, z = i[order], j[order], z[order]
    pairs = pd.DataFrame({"i": i, "j": j, "z": z, "chi2": z * z,
                          "p": np.array([math.erfc(abs(v) / math.sqrt(2.0)) for v in z.tolist()], np.float64)})
    some = ntot > 0
    partner = (~best & np.uint64(0xffffffff)).astype(np.int64)
    summary = pd.DataFrame({"snp": col, "n_tot": ntot.astype(np.int64), "n_sig": nsig.astype(np.int64),
                            "best_chi2": np.where(some, (best >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(np.nan)),
                            "best_partner": np.where(some, col[np.where(some, partner, 0)], -1)})
    if stats is not None:
        stats.update({"blocks": nblocks, "reruns": reruns, "pairs_defined": int(ntot.sum(dtype=np.int64)) // 2,
                      "bytes_in": sum(s.p * s.row_bytes for s in srcs), "seconds": time.time() - t0})
    _log(verbose, f"epistasis: {na} x {nb} SNPs with {n} individuals, {len(pairs)} pairs at chi2 >= {chi2_min:.3f} in {time.time() - t0:.3f} s")
    return EpistasisResult(pairs, summary, chi2_min)


# ---- per-SNP case/control tests on contingency tables (csrc/case_control.hip) ---------------------------------------------------
_CC_MAX_STRATA = 16            # PG_CC_MAX_STRATA
_CC_COUNTS = ("case0", "case1", "case2", "case_miss", "ctrl0", "ctrl1", "ctrl2", "ctrl_miss")
_CC_STAT = ("af_case", "af_ctrl", "or", "chi2_allelic", "chi2_trend", "chi2_geno", "chi2_dom", "chi2_rec", "p_fisher", "chi2_cmh", "or_mh")   # stat's columns
_CC_COLS = _CC_COUNTS + ("hard", "af_case", "af_ctrl", "or", "chi2_allelic", "p_allelic", "chi2_trend", "p_trend", "chi2_geno", "p_geno", "chi2_dom",
                         "p_dom", "chi2_rec", "p_rec", "p_fisher", "cmh_u", "cmh_v", "chi2_cmh", "p_cmh", "or_mh")
_CC_CMH = ("cmh_u", "cmh_v", "chi2_cmh", "p_cmh", "or_mh")


def _cc_p1(chi2):
    """The upper tail of chi2 on 1 df, erfc(sqrt(chi2 / 2)), in one vectorised call; NaN stays NaN."""
    from scipy import special as _spc      # lazily, as pygemma_lm does
    return _spc.erfc(np.sqrt(np.asarray(chi2, np.float64) / 2.0))


def _cc_p2(chi2):
    """The upper tail of chi2 on 2 df, exp(-chi2 / 2); NaN stays NaN."""
    return np.exp(-np.asarray(chi2, np.float64) / 2.0)


def _cc_strata(strata, n):
    """(int32 stratum of every sample in 0..S-1, -1 excluded; S) from integer labels or a pandas categorical: the labels in sorted order,
    NaN and negative labels excluded.  (None, 1) without strata."""
    if strata is None:
        return None, 1
    if isinstance(strata, pd.Categorical) or isinstance(getattr(strata, "dtype", None), pd.CategoricalDtype):
        lab = np.asarray(pd.Categorical(strata).codes, np.float64)             # -1 where the label is missing
    else:
        lab = np.asarray(strata)
        if lab.dtype.kind not in "biuf":
            raise ValueError(f"strata must hold integer labels (or be a pandas categorical), not dtype {lab.dtype}")
        lab = lab.astype(np.float64)
    if lab.ndim != 1 or lab.shape[0] != n:
        raise ValueError(f"shape mismatch: strata has shape {lab.shape} for {n} samples")
    keep = np.isfinite(lab) & (lab >= 0)
    if np.isinf(lab).any() or (lab[keep] != np.floor(lab[keep])).any():
        raise ValueError("strata must hold integer labels; NaN or a negative label excludes the sample")
    levels = np.unique(lab[keep])
    if len(levels) < 1:
        raise ValueError("strata leaves no sample in a stratum")
    if len(levels) > _CC_MAX_STRATA:
        raise ValueError(f"case_control takes at most {_CC_MAX_STRATA} strata, strata holds {len(levels)} labels")
    code = np.full(n, -1, np.int32)
    code[keep] = np.searchsorted(levels, lab[keep])
    return code, len(levels)


def case_control(X, y, *, strata=None, fisher=True, snps=None, device=0, snp_batch=None, verbose=0, stats=None):
    """Per-SNP tests of a case/control trait on contingency tables: what PLINK prints with --assoc, --model, --fisher and --mh, every
    statistic a function of exact integer counts that a popcount kernel reads from packed .bed words (csrc/case_control.hip).

    X (n, p): whatever snp_stats takes — a PackedBed (honouring count_A1), or an int8, uint8, float32 or float64 array in C or Fortran
    order, pinned or pageable — streamed in SNP batches of `snp_batch` columns through the two-slot feed; an array batch is packed into
    2-bit records on the device first.  The results stay on the device until one download at the end and do not depend on the batch
    boundaries.  .bed code 01, NaN and +-Inf are missing.  Only a hard-call SNP is tested (every observed value exactly 0, 1 or 2, as
    for `ld`): any other SNP has `hard` False, counts 0 and NaN statistics.
    y (n,): 1 case, 0 control (bool allowed), NaN excluded.  strata: None, or (n,) integer labels or a pandas categorical, mapped to
    0..S-1 in sorted order, S <= 16; a sample with a NaN or negative stratum is excluded.
    With r_i, s_i the cases and controls of genotype i among the called samples that have a status and a stratum, n_i = r_i + s_i,
    R = sum r_i, S' = sum s_i, N = R + S', and per group A = n1 + 2 n2 alleles of the counted allele and 2 (group size) - A of the other,
    the frame has p rows:
      case0, case1, case2, case_miss, ctrl0, ctrl1, ctrl2, ctrl_miss (int64)   the 2 x 4 table, pooled over the strata
      hard                           the SNP is hard-call
      af_case, af_ctrl               A / (2 group size)
      or                             a d / (b c) of the allelic 2 x 2 table; +inf when b c = 0 < a d, NaN when both are 0
      chi2_allelic, p_allelic        1 df on the allelic table (--assoc)
      chi2_trend, p_trend            Cochran-Armitage, weights 0, 1, 2, 1 df
      chi2_geno, p_geno              2 df on the 2 x 3 table; NaN when a genotype is unseen
      chi2_dom, p_dom, chi2_rec, p_rec   1 df: 1 + 2 against 0, and 2 against 0 + 1
      p_fisher                       the two-sided exact test on the allelic table; absent with fisher=False
      cmh_u, cmh_v, chi2_cmh, p_cmh, or_mh   Cochran-Mantel-Haenszel over the strata's allelic tables, no continuity correction:
                                     u = sum a_k - row1_k col1_k / T_k, v = sum row1 row2 col1 col2 / (T^2 (T - 1)), chi2 = u^2 / v (NaN
                                     when v = 0), or_mh = sum (a d / T) / sum (b c / T) (NaN when the divisor is 0), over the strata that
                                     hold a called case and a called control; absent with strata=None
      SNPs                           `snps`, when given
    A 2 x 2 chi2 is NaN when a margin is 0; every statistic of a row is NaN when R = 0 or S' = 0 (the counts are still reported).
    p-values on the host from the chi2 columns: erfc(sqrt(chi2 / 2)) on 1 df, exp(-chi2 / 2) on 2.
    `stats` receives batches, bytes_in, seconds and lambda_gc = median(chi2_trend over its non-NaN rows) / chi2.ppf(0.5, 1).  Refused
    with ValueError before any device work: X not 2-D or of another dtype, an empty X, y of another length or with values other than
    0, 1, NaN, no case, no control, strata of another length, not integer or with more than 16 labels, `snps` of another length, a bad
    snp_batch."""
    _check_snp_batch(snp_batch)
    X = _genotypes(X, "case_control")
    n, p = X.shape
    if n < 1 or p < 1:
        raise ValueError(f"case_control needs at least one sample and one SNP: X holds n={n}, p={p}")
    if snps is not None and len(snps) != p:
        raise ValueError(f"shape mismatch: {len(snps)} SNP names for {p} SNPs")
    group = _epi_group(y, n, False)
    strat, S = _cc_strata(strata, n)
    cnt, cmh, st, hard = _cc_stream(X, group, strat, S, bool(fisher), device, snp_batch, verbose, stats)
    out = {col: cnt[:, k] for k, col in enumerate(_CC_COUNTS)}
    out["hard"] = hard
    out.update({col: st[:, k] for k, col in enumerate(_CC_STAT)})
    out["cmh_u"], out["cmh_v"] = cmh[:, 0], cmh[:, 1]
    for name in ("allelic", "trend", "dom", "rec", "cmh"):
        out["p_" + name] = _cc_p1(out["chi2_" + name])
    out["p_geno"] = _cc_p2(out["chi2_geno"])
    drop = (() if fisher else ("p_fisher",)) + (_CC_CMH if strata is None else ())
    if stats is not None:
        z = out["chi2_trend"][~np.isnan(out["chi2_trend"])]
        stats["lambda_gc"] = float(np.median(z) / _CHI2_MEDIAN) if z.size else float("nan")
    return _frame(out, [col for col in _CC_COLS if col not in drop], snps)


def _cc_stream(X, group, strat, S, fisher, device, snp_batch, verbose, stats):
    """The streamed case/control pass: pg_cc_setup_dev once, then SNP batches from the feed (_feed._Feed) — records as they are, an array
    batch through pg_cc_pack_x_dev into one record buffer — through pg_cc_count_dev into windows of the (p, 8) count and (p, 4) CMH
    arrays on the device, then pg_cc_stats_dev on all p rows.  Returns the host arrays (counts, cmh, stat, hard)."""
    L, K, t0 = _lib.load(), _lib.load_cc(), time.time()
    src = _describe(X)
    n, p = src.n, src.p
    _gpus()
    with _lib.Context(device) as ctx, contextlib.closing(_Feed(ctx, src)) as feed:
        ldb = 0 if src.packed else -(-((n + 3) // 4) // 16) * 16           # the records of an array batch: rows on 16 bytes
        work_bytes = int(K.pg_cc_work_bytes(n, S))
        pb = _fit_batch(ctx, snp_batch, _lm_batch(src), p, 128, lambda pb: 185 * p + 5 * n + work_bytes + 2 * pb * src.row_bytes + pb * ldb,
                        f"case_control: n={n}, p={p}", "185 p bytes of results, the group masks, two batch slots, the records of an array batch")
        work, dgroup = ctx.alloc(work_bytes), ctx.to_device(group)
        dstrat = None if strat is None else ctx.to_device(strat)
        _lib.check(K.pg_cc_setup_dev(ctx.handle, n, S, dgroup.ptr, None if dstrat is None else dstrat.ptr, work.ptr), "pg_cc_setup_dev")
        dc, dcmh, dst = ctx.alloc(64 * p), ctx.alloc(32 * p), ctx.alloc(8 * len(_CC_STAT) * p)
        if not src.packed:
            drec, dhard = ctx.alloc(pb * ldb), ctx.alloc(p)
        for s, e, slot in feed.batches(pb):
            out = (dc.ptr + 64 * s, dcmh.ptr + 32 * s)
            if src.packed:
                _call_dev(K, "pg_cc_count_dev", src, (ctx.handle, n, e - s), slot, e - s, (S, work.ptr, None, *out))
            else:
                _call_dev(K, "pg_cc_pack_{}_dev", src, (ctx.handle, n, e - s), slot, e - s, (drec.ptr, ldb, dhard.ptr + s))
                _lib.check(K.pg_cc_count_dev(ctx.handle, n, e - s, drec.ptr, ldb, 0, S, work.ptr, dhard.ptr + s, *out), "pg_cc_count_dev")
            _log(verbose - 1, f"case_control: SNPs [{s},{e}) queued")
        _lib.check(K.pg_cc_stats_dev(ctx.handle, p, dc.ptr, dcmh.ptr, int(fisher), dst.ptr), "pg_cc_stats_dev")
        ctx.sync()
        hard = np.ones(p, np.bool_) if src.packed else dhard.download((p,), np.uint8).astype(np.bool_)
        res = dc.download((p, 8), np.int64), dcmh.download((p, 4), np.float64), dst.download((p, len(_CC_STAT)), np.float64), hard
    _stream_stats(stats, src, pb, t0)
    _log(verbose, f"Case/control tests: {p} SNPs with {n} individuals, {S} strata in {time.time() - t0:.3f} s")
    return res


# ---- max(T) permutation tests of a case/control trait (csrc/perm.hip) ----------------------------------------------------------
_PERM_TESTS = {"allelic": 0, "trend": 1}     # PG_PERM_ALLELIC, PG_PERM_TREND
_PERM_COLS = ("hard", "chi2", "p", "n_ge", "emp1", "emp2")


def _perm_study(group, strat):
    """The study flag of every sample: it has a status and (with strata) a stratum."""
    return (group >= 0) if strat is None else ((group >= 0) & (strat >= 0))


def _perm_labels(group, strat, S, nperm, seed):
    """(nperm, n) int8 labellings: row b shuffles the case labels of the study samples within each of the S strata (all of them one
    stratum without `strat`), so it keeps every stratum's number of cases and labels no excluded sample.  Row b is a function of
    (seed, b, group, strat) alone — its own generator np.random.default_rng((seed, b)) — whatever nperm is."""
    study = _perm_study(group, strat)
    members = [np.flatnonzero(study & ((strat == k) if strat is not None else True)) for k in range(S)]
    ncase = [int((group[idx] == 1).sum()) for idx in members]
    out = np.zeros((nperm, group.shape[0]), np.int8)
    for b in range(nperm):
        rng = np.random.default_rng((int(seed), b))
        for idx, r in zip(members, ncase):           # in stratum order: part of the definition of row b
            out[b, idx[rng.permutation(idx.size)[:r]]] = 1
    return out


def _perm_emp2(max_null, chi2):
    """(#{b: max_null[b] >= chi2} + 1) / (nperm + 1) per SNP; NaN where chi2 is."""
    srt = np.sort(np.asarray(max_null, np.float64))
    chi2 = np.asarray(chi2, np.float64)
    bad = np.isnan(chi2)
    ge = srt.size - np.searchsorted(srt, np.where(bad, 0.0, chi2), side="left")
    return np.where(bad, np.nan, (ge + 1.0) / (srt.size + 1.0))


class PermResult:
    """What case_control_perm returns: .snps (a row per SNP: hard, chi2, p, n_ge, emp1, emp2, and SNPs when given), .max_null (nperm,)
    the largest statistic over the SNPs under every labelling, .test, .nperm, and threshold(alpha)."""

    def __init__(self, snps, max_null, test):
        self.snps, self.max_null, self.test, self.nperm = snps, max_null, test, int(max_null.shape[0])

    def threshold(self, alpha=0.05):
        """The family-wise critical chi2 at level alpha: the ceil((1 - alpha)(nperm + 1))-th smallest of max_null (a SNP whose chi2
        exceeds it has emp2 <= alpha); inf when that rank exceeds nperm, that is when nperm is too small for alpha.  The rank is taken
        1e-9 below the product, so that (1 - 0.05) * 20 is the rank 19 it stands for."""
        if isinstance(alpha, bool) or not isinstance(alpha, (int, float, np.integer, np.floating)) or not 0 < alpha < 1:
            raise ValueError(f"alpha must lie in (0, 1), not {alpha!r}")
        rank = max(1, math.ceil((1.0 - alpha) * (self.nperm + 1) - 1e-9))
        return float("inf") if rank > self.nperm else float(np.sort(self.max_null)[rank - 1])


def _perm_check_labels(labels, n, study):
    labels = np.asarray(labels)
    if labels.ndim != 2 or labels.shape[1] != n or labels.shape[0] < 1:
        raise ValueError(f"shape mismatch: labels has shape {labels.shape}, not (nperm >= 1, {n})")
    if labels.dtype.kind not in "biuf" or not ((labels == 0) | (labels == 1)).all():
        raise ValueError("labels must hold 0 and 1 and nothing else")
    if (labels[:, ~study] != 0).any():
        raise ValueError("labels names a case among the samples that are out of the study (no status, or no stratum)")
    return labels.astype(np.int8)


def case_control_perm(X, y, *, nperm=1000, test="allelic", strata=None, seed=0, labels=None, snps=None, device=0, snp_batch=None, verbose=0,
                      stats=None):
    """max(T) permutation tests of a case/control trait: PLINK's --assoc --mperm nperm (test="allelic") and --model trend --mperm nperm
    (test="trend"), on the int8 matrix pipe (csrc/perm.hip).  The case labels are shuffled nperm times, every SNP's statistic is
    recomputed under every labelling from exact integer sums, and only a count per SNP and a maximum per labelling leave the device.

    X (n, p) as for `ld`: hard calls only, a SNP with another observed value counts as all missing and has NaN statistics.  y (n,):
    1 case, 0 control (bool allowed), NaN excluded.  strata: as for case_control; the shuffles stay within each stratum (PLINK's
    --within) and a sample without a stratum is out of the study; the statistic stays the pooled one.  `labels`: an explicit
    (nperm, n) 0/1 matrix of labellings in place of the generator's (then `nperm` and `seed` are not read); it must be 0 where a
    sample is out of the study.  The generator's row b depends on (seed, b, y, strata) alone.
    The frame .snps of the PermResult has p rows:
      hard     the SNP is hard-call
      chi2, p  the observed statistic — bit-equal to case_control's chi2_allelic / chi2_trend — and its asymptotic p on 1 df
      n_ge     labellings whose statistic is >= chi2 (exact ties count: the sums are integers); a NaN on either side never counts
      emp1     (n_ge + 1) / (nperm + 1), the pointwise empirical p (PLINK's EMP1)
      emp2     (#{b: max_null[b] >= chi2} + 1) / (nperm + 1), the family-wise empirical p (EMP2)
      SNPs     `snps`, when given
    emp1 and emp2 are NaN where chi2 is.  .max_null[b] is the largest defined statistic over all SNPs under labelling b (0 when none
    is defined), .threshold(alpha) the family-wise critical chi2.  The labellings are uploaded once, the SNPs streamed once in batches
    of `snp_batch` through the two-slot feed; the result does not depend on the batch boundaries or the source kind.
    `stats` receives batches, bytes_in, seconds.  Refused with ValueError before any device work: what case_control refuses for X, y,
    strata, snps and snp_batch; nperm < 1; an unknown test; labels of another shape, with other values or naming an excluded sample;
    a negative seed."""
    _check_snp_batch(snp_batch)
    if test not in _PERM_TESTS:
        raise ValueError(f"test must be one of {sorted(_PERM_TESTS)}, not {test!r}")
    X = _ld_source(X, "case_control_perm")
    n, p = X.shape
    if snps is not None and len(snps) != p:
        raise ValueError(f"shape mismatch: {len(snps)} SNP names for {p} SNPs")
    group = _epi_group(y, n, False)
    strat, S = _cc_strata(strata, n)
    study = _perm_study(group, strat)
    if labels is not None:
        lab = _perm_check_labels(labels, n, study)
    else:
        if isinstance(nperm, bool) or not isinstance(nperm, (int, np.integer)) or nperm < 1:
            raise ValueError(f"nperm must be a positive integer, not {nperm!r}")
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or seed < 0:
            raise ValueError(f"seed must be a non-negative integer, not {seed!r}")
        lab = _perm_labels(group, strat, S, int(nperm), seed)
    nperm = lab.shape[0]
    ldk = -(-n // 128) * 128
    rows = np.zeros((2 + nperm, ldk), np.int8)       # the label image: the study flags, the observed status, the labellings
    rows[0, :n] = study
    rows[1, :n] = study & (group == 1)
    rows[2:, :n] = lab
    tot, obs, nge, mx, pb, src, t0 = _perm_stream(X, rows, nperm, _PERM_TESTS[test], device, snp_batch, verbose)
    bad = np.isnan(obs)
    out = {"hard": (tot[:, 3] & 2) == 0, "chi2": obs, "p": _cc_p1(obs), "n_ge": nge.astype(np.int64),
           "emp1": np.where(bad, np.nan, (nge + 1.0) / (nperm + 1.0)), "emp2": _perm_emp2(mx, obs)}
    _stream_stats(stats, src, pb, t0)
    return PermResult(_frame(out, _PERM_COLS, snps), mx, test)


def _perm_stream(X, rows, nperm, test, device, snp_batch, verbose):
    """The streamed permutation pass: the label image up once and pg_perm_label_counts_dev on it, then SNP batches from the feed
    (_feed._Feed) through pg_ld_encode_*_dev into one LD image of a batch, pg_perm_totals_dev, pg_perm_block_dev on the observed row
    (dense: the observed statistics) and on all labellings (n_ge, max_null); one download at the end.  Returns the host arrays
    (totals (p, 4) int32, obs, n_ge, max_null) and (pb, src, t0) for the stream's statistics."""
    t0 = time.time()
    src = _describe(X)
    n, p = src.n, src.p
    L, P = _lib.load(), _lib.load_perm()
    _gpus()
    nrows = rows.shape[0]
    with _lib.Context(device) as ctx, contextlib.closing(_Feed(ctx, src)) as feed:
        lab_bytes = int(P.pg_perm_label_bytes(n, nrows))
        pb = _fit_batch(ctx, snp_batch, min(_LD_BATCH, _lm_batch(src)), p, 128,
                        lambda pb: lab_bytes + 4 * nrows + 8 * nperm + 28 * p + int(L.pg_ld_image_bytes(n, pb)) + 2 * pb * src.row_bytes,
                        f"case_control_perm: n={n}, p={p}, nperm={nperm}", "the labellings n bytes each, 28 p bytes of results, an int8 image of a batch, two batch slots")
        dlab, dlabc = ctx.alloc(lab_bytes).upload(rows), ctx.alloc(4 * nrows)
        _lib.check(P.pg_perm_label_counts_dev(ctx.handle, n, dlab.ptr, nrows, dlabc.ptr), "pg_perm_label_counts_dev")
        image = ctx.alloc(L.pg_ld_image_bytes(n, pb))
        dtot, dobs, dnge, dmax = ctx.alloc(16 * p), ctx.alloc(8 * p), ctx.alloc(4 * p), ctx.alloc(8 * nperm)
        for buf in (dnge, dmax):
            _lib.check(L.pg_memset(ctx.handle, buf.ptr, 0, buf.nbytes), "pg_memset")
        for s, e, slot in feed.batches(pb):
            _call_dev(L, "pg_ld_encode_{}_dev", src, (ctx.handle, n, e - s), slot, e - s, (image.ptr, pb, 0))
            _lib.check(P.pg_perm_totals_dev(ctx.handle, n, image.ptr, pb, 0, e - s, dlab.ptr, dtot.ptr + 16 * s), "pg_perm_totals_dev")
            head = (ctx.handle, n, image.ptr, pb, 0, e - s, dtot.ptr + 16 * s, dlab.ptr, dlabc.ptr)
            _lib.check(P.pg_perm_block_dev(*head, 1, 1, test, dobs.ptr + 8 * s, 1, None, None, None), "pg_perm_block_dev")
            _lib.check(P.pg_perm_block_dev(*head, 2, nperm, test, None, 0, dobs.ptr + 8 * s, dnge.ptr + 4 * s, dmax.ptr), "pg_perm_block_dev")
            _log(verbose - 1, f"case_control_perm: SNPs [{s},{e}) queued")
        ctx.sync()
        res = (dtot.download((p, 4), np.int32), dobs.download((p,), np.float64), dnge.download((p,), np.uint32),
               dmax.download((nperm,), np.uint64).view(np.float64))
    _log(verbose, f"Permutation tests: {p} SNPs x {nperm} labellings with {n} individuals in {time.time() - t0:.3f} s")
    return res + (pb, src, t0)


# ---- KING-robust relatedness and sample QC (csrc/king.hip) -------------------------------------------------------------------
# SNPs per batch by default: the read-modify-write of the int32 accumulators (up to 20 n^2 bytes per batch on and below the diagonal) is
# about 650 / pb of the batch's products (5 n^2 pb int8 operations) at 5 TB/s and 2.5 POP/s: 4 % at 16 384
_KING_BATCH = 16384
_SAMPLE_COLS = ("n_obs", "n_miss", "n0", "n1", "n2", "miss", "het")


def _king_source(X, who, snp_batch):
    _check_snp_batch(snp_batch)
    X = _ld_source(X, who)
    if X.shape[1] >= 2 ** 31:
        raise ValueError(f"{who} counts in int32: p = {X.shape[1]} SNPs is 2^31 or more")
    return X


def _sample_frame(cnt, samples=None):
    """The per-sample frame of an (n, 5) int64 array n_obs, n_miss, n0, n1, n2."""
    out = {col: cnt[:, k] for k, col in enumerate(_SAMPLE_COLS[:5])}
    tot = cnt[:, 0] + cnt[:, 1]
    out["miss"] = cnt[:, 1] / tot.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        out["het"] = np.where(cnt[:, 0] > 0, cnt[:, 3] / cnt[:, 0].astype(np.float64), np.nan)
    df = pd.DataFrame(out, columns=list(_SAMPLE_COLS))
    if samples is not None:
        df["samples"] = samples
    return df


def _king_stream(X, what, counts, device, snp_batch, verbose, stats, who):
    """The streamed pair counts: SNP batches from the feed (_feed._Feed) through pg_king_{bed,x}_acc_dev into the int32 accumulators, then
    pg_king_finish_dev (what: 0 phi, 1 ibs) and, with `counts`, pg_king_counts_dev.  Returns the matrix, or (matrix, dict)."""
    L, t0 = _lib.load(), time.time()
    src = _describe(X)
    n, p = src.n, src.p
    if not L.pg_king_acc_bytes(n, 1):
        raise ValueError(f"{who} takes fewer than 2^20 samples, not n={n}")
    _gpus()
    with _lib.Context(device) as ctx, contextlib.closing(_Feed(ctx, src)) as feed:
        # everything that lives beside the accumulators until the context closes: the float32 result and, with `counts`, the five int32
        # matrices and the n x 5 counts that pg_king_counts_dev writes after the stream; _fit_batch must see them to size the batch honestly
        out_bytes = 4 * n * n + ((20 * n * n + 40 * n) if counts else 0)
        pb = _fit_batch(ctx, snp_batch, _KING_BATCH, p, 128, lambda pb: int(L.pg_king_acc_bytes(n, pb)) + out_bytes + 2 * pb * src.row_bytes,
                        f"{who}: n={n}", "int32 accumulators 16 n^2, the result 4 n^2 (24 n^2 with counts), int8 planes 3 n per SNP, two batch slots")
        dacc = ctx.alloc(L.pg_king_acc_bytes(n, pb))
        dout = ctx.alloc(4 * n * n)
        batches = feed.batches(pb)
        _lib.check(L.pg_memset(ctx.handle, dacc.ptr, 0, L.pg_king_zero_bytes(n)), "pg_memset")
        for s, e, slot in batches:
            _call_dev(L, "pg_king_{}_acc_dev", src, (ctx.handle, n, e - s), slot, e - s, (dacc.ptr,))
            _log(verbose - 1, f"{who}: SNPs [{s},{e}) queued")
        _lib.check(L.pg_king_finish_dev(ctx.handle, n, dacc.ptr, what, dout.ptr), "pg_king_finish_dev")
        if counts:
            dc, ds = ctx.alloc(20 * n * n), ctx.alloc(40 * n)
            _lib.check(L.pg_king_counts_dev(ctx.handle, n, dacc.ptr, dc.ptr, ds.ptr), "pg_king_counts_dev")
        ctx.sync()
        out = dout.download((n, n), np.float32)
        if counts:
            mats = dc.download((5, n, n), np.int32)
            extra = {"N": mats[0], "HH": mats[1], "IBS0": mats[2], "Hij": mats[3], "samples": _sample_frame(ds.download((n, 5), np.int64))}
    _stream_stats(stats, src, pb, t0)
    _log(verbose, f"{who}: {p} SNPs with {n} individuals in {time.time() - t0:.3f} s")
    return (out, extra) if counts else out


def king(X, *, counts=False, device=0, snp_batch=None, verbose=0, stats=None):
    """The KING-robust kinship matrix of the samples (Manichaikul et al. 2010; the estimator of plink2 --make-king): the (n, n) float32
    matrix phi, both triangles, bit-symmetric.  It needs no allele frequencies, so one stream over the genotypes is enough: duplicates and
    twins, sample swaps and close relatives show before the first scan.

    X (n, p): whatever snp_stats takes — a PackedBed, or an int8, uint8, float32 or float64 array in C or Fortran order, pinned or
    pageable — streamed in SNP batches of `snp_batch` columns through the two-slot feed, encoded into int8 planes on the device and
    multiplied on the int8 matrix pipe (csrc/king.hip).  Hard calls only, as for `ld`: missing is .bed code 01, NaN or +-Inf; a SNP with
    an observed value other than 0, 1, 2 counts as all missing for every sample.  Over the SNPs where both samples of a pair are called,
      N = jointly called SNPs, HH = both het, IBS0 = opposite homozygotes, Hij = i's het calls where j is called (Hji its transpose)
      phi = (HH - 2 IBS0) / (Hij + Hji): one fp64 division of exact int32 counts, one rounding to float32; NaN when Hij + Hji == 0.
    A sample against itself or an exact duplicate gives exactly 0.5; unrelated pairs scatter around 0 (negative values mean population
    structure); phi does not depend on count_A1, nor, bit for bit, on the batch boundaries.  `counts=True` returns (phi, dict) with the
    (n, n) int32 matrices N, HH, IBS0, Hij (Hij in full, not symmetric) and `samples`, the frame of sample_stats from the same stream.
    `stats` receives batches, bytes_in, seconds.  Accumulators that do not fit the device raise PgError.  Refused with ValueError before
    any device work: X not 2-D or of another dtype, an empty X, n >= 2^20, p >= 2^31, a bad snp_batch."""
    return _king_stream(_king_source(X, "king", snp_batch), 0, bool(counts), device, snp_batch, verbose, stats, "king")


def ibs(X, *, counts=False, device=0, snp_batch=None, verbose=0, stats=None):
    """The identity-by-state similarity of the samples from the stream of `king` (same arguments, same counts): the (n, n) float32 matrix
    1 - (IBS1 + 2 IBS0) / (2 N), the share of alleles two samples have in common over the SNPs where both are called (PLINK's --distance
    ibs), IBS1 = Hij + Hji - 2 HH; NaN when N == 0.  A sample against itself gives exactly 1."""
    return _king_stream(_king_source(X, "ibs", snp_batch), 1, bool(counts), device, snp_batch, verbose, stats, "ibs")


def sample_stats(X, samples=None, device=0, snp_batch=None, verbose=0, stats=None):
    """Per-sample quality control from the raw genotypes, read once where they lie (PLINK's --missing and --het on samples): a DataFrame
    of n rows with n_obs, n_miss, n0, n1, n2 (int64: called and missing calls, calls that are 0, 1, 2; count_A1 swaps n0 and n2),
    miss = n_miss / p and het = n1 / n_obs (NaN at n_obs == 0), and `samples` when given.  X as for `king`, with its hard-call rule: a
    SNP that is not hard-call adds 1 to every n_miss.  This is the count kernel of `king` alone, bandwidth-bound, without pair products.
    `stats` receives batches, bytes_in, seconds.  Refused with ValueError before any device work: X not 2-D or of another dtype, an empty
    X, `samples` of another length, a bad snp_batch."""
    X = _king_source(X, "sample_stats", snp_batch)
    L, t0 = _lib.load(), time.time()
    src = _describe(X)
    n, p = src.n, src.p
    if samples is not None and len(samples) != n:
        raise ValueError(f"shape mismatch: {len(samples)} sample names for {n} samples")
    if not L.pg_king_acc_bytes(n, 1):
        raise ValueError(f"sample_stats takes fewer than 2^20 samples, not n={n}")
    _gpus()
    with _lib.Context(device) as ctx, contextlib.closing(_Feed(ctx, src)) as feed:
        pb = _fit_batch(ctx, snp_batch, _lm_batch(src), p, 128, lambda pb: 40 * n + 4 * pb + 2 * pb * src.row_bytes,
                        f"sample_stats: n={n}, p={p}", "40 n bytes of counts, two batch slots")
        ds = ctx.alloc(40 * n)
        batches = feed.batches(pb)
        _lib.check(L.pg_memset(ctx.handle, ds.ptr, 0, 40 * n), "pg_memset")
        for s, e, slot in batches:
            _call_dev(L, "pg_sample_stats_{}_acc_dev", src, (ctx.handle, n, e - s), slot, e - s, (ds.ptr,))
            _log(verbose - 1, f"sample_stats: SNPs [{s},{e}) queued")
        ctx.sync()
        cnt = ds.download((n, 5), np.int64)
    _stream_stats(stats, src, pb, t0)
    _log(verbose, f"Sample statistics: {p} SNPs with {n} individuals in {time.time() - t0:.3f} s")
    return _sample_frame(cnt, samples)


def _check_phi(phi, cutoff):
    phi = np.asarray(phi)
    if phi.ndim != 2 or phi.shape[0] != phi.shape[1]:
        raise ValueError(f"phi must be a square (n, n) matrix, not of shape {phi.shape}")
    if isinstance(cutoff, bool) or not isinstance(cutoff, (int, float, np.integer, np.floating)) or not -np.inf < cutoff <= 0.5:
        raise ValueError(f"cutoff must be a number of at most 0.5 (a duplicate's kinship), not {cutoff!r}")
    return phi


def related_pairs(phi, cutoff=0.0884):
    """The related pairs of a kinship matrix of `king`: a DataFrame i, j, phi of the pairs i < j with phi[i, j] > cutoff, sorted by
    descending phi, then i, then j; pure NumPy.  NaN is never related.  The usual cut-offs are the geometric midpoints between the
    expected kinships of the degrees: 0.354 duplicates and monozygotic twins, 0.177 first degree, 0.0884 second degree (the default),
    0.0442 third degree.  Refused with ValueError: a phi that is not square, a cutoff above 0.5 or not a number."""
    phi = _check_phi(phi, cutoff)
    with np.errstate(invalid="ignore"):
        i, j = np.nonzero(np.triu(phi > cutoff, 1))
    v = phi[i, j]
    order = np.lexsort((j, i, -v.astype(np.float64)))
    return pd.DataFrame({"i": i[order].astype(np.int64), "j": j[order].astype(np.int64), "phi": v[order]}, columns=["i", "j", "phi"])


def unrelated(phi, cutoff=0.0884):
    """A boolean keep-mask over the samples of a kinship matrix of `king` in which no two kept samples are related (phi > cutoff, the
    cut-offs of related_pairs): hand it to PackedBed.take_samples or index the rows of X with it.  The rule is greedy and deterministic
    on the graph of related pairs: while an edge remains, drop the vertex of largest current degree, ties going to the largest index.
    That is NOT the algorithm of plink2 --king-cutoff, which may keep another (equally unrelated) subset; pure NumPy and Python on the
    thresholded pairs.  Refusals as for related_pairs."""
    import heapq
    phi = _check_phi(phi, cutoff)
    n = phi.shape[0]
    pairs = related_pairs(phi, cutoff)
    adj = [set() for _ in range(n)]
    for i, j in zip(pairs["i"].tolist(), pairs["j"].tolist()):
        adj[i].add(j)
        adj[j].add(i)
    keep = np.ones(n, bool)
    heap = [(-len(adj[v]), -v) for v in range(n) if adj[v]]      # entries go stale when a neighbour leaves: checked when popped
    heapq.heapify(heap)
    while heap:
        d, v = heapq.heappop(heap)
        d, v = -d, -v
        if not keep[v] or d != len(adj[v]) or d == 0:
            continue
        keep[v] = False
        for u in adj[v]:
            adj[u].discard(v)
            if adj[u]:
                heapq.heappush(heap, (-len(adj[u]), -u))
        adj[v] = set()
    return keep


# ---- polygenic scores (csrc/prs.hip) -----------------------------------------------------------------------------------------
_PRS_CHUNK = 256     # PG_PRS_CHUNK: batches are multiples of the summation chunk, so the bits do not depend on the batch size
_PRS_MAX_T = 64      # PG_PRS_MAX_T: weight columns per kernel call
_PRS_DROP = 0.5      # SNPs whose weights are all zero are dropped on the host when they are at least this share of the SNPs


def _chunk_up(snps):
    return -(-int(snps) // _PRS_CHUNK) * _PRS_CHUNK


def _weight_columns(weights):
    """(labels, (p, t) float64 array) of a weights argument: (p,), (p, t), a Series or a DataFrame (labelled by its columns, anything
    else by 0..t-1)."""
    if isinstance(weights, pd.DataFrame):
        labels, Wm = list(weights.columns), weights.to_numpy()
    else:
        Wm = np.asarray(weights)
        if Wm.ndim == 1:
            Wm = Wm.reshape(-1, 1)
        labels = list(range(Wm.shape[1])) if Wm.ndim == 2 else []
    if Wm.ndim != 2:
        raise ValueError(f"weights must be (p,) or (p, t), got shape {Wm.shape}")
    try:
        Wm = np.ascontiguousarray(Wm, np.float64)
    except (TypeError, ValueError) as exc:
        raise ValueError(f"weights must be numbers: {exc}") from None
    if Wm.shape[1] < 1:
        raise ValueError("weights has no score column")
    if not np.isfinite(Wm).all():
        raise ValueError("weights must be finite: set the weight of a SNP that is not to count to 0")
    return labels, Wm


def prs(X, weights, *, missing="mean", counts=False, samples=None, device=0, snp_batch=None, verbose=0, stats=None):
    """Polygenic scores S = G W (PLINK's --score; the clumping-and-thresholding score with prs_weights): the effect sizes of a scan
    applied to a cohort, read once where its genotypes lie — no host decode of a .bed file, no float copy of X.

    X (n, p): whatever snp_stats takes — a PackedBed, or an int8, uint8, float32 or float64 array in C or Fortran order, pinned or
    pageable.  weights: (p,), (p, t), a Series or a DataFrame of finite numbers, cast to float64; a DataFrame's columns label the
    scores, anything else is labelled 0..t-1.  Values are snp_stats' (float64 rounded to float32 per element; .bed code 01, NaN and
    +-Inf are missing, an 8-bit array has no missing code).  missing="mean": a missing call takes the mean of the called genotypes
    of its SNP in X — the very number snp_stats reports as `mean` — and every call of an all-missing SNP is 0; missing="skip": a
    missing call is 0.  Returns a DataFrame of n rows (indexed by `samples` when given) with one float64 column per label,
      S[i, k] = sum_g x_gi w_gk                                  in fp64 on the matrix pipe (csrc/prs.hip);
    with counts=True a pair (scores, n_called), n_called[i, k] = #{g : sample i is called at g and w_gk != 0} as int64 in the same
    shape (it does not depend on `missing`): PLINK's per-sample allele-count denominator, divided by two.
    SNPs whose weights are all zero contribute nothing and are left on the host when they are at least half of the SNPs (PackedBed.take /
    X[:, idx], as clump uploads only its candidates); when no SNP has a weight the result is zero and no device is touched.  The
    rest streams through the two-slot feed in SNP batches; more than 64 weight columns run in groups of 64 over the same stream, so
    X leaves the host once.  Sums run in chunks of 256 SNPs, added in order, and `snp_batch` (default: from n and the free device
    memory) is rounded up to a multiple of 256: the returned bits do not depend on it, on the source's pitch or alignment, or on the run
    (only on which SNPs are streamed).  `stats` receives batches, bytes_in, seconds and snps_used.  Refused with ValueError before any
    device work: a non-finite weight, X not 2-D, of another dtype or empty, weights with other than p rows or without a column,
    `samples` of another length, a bad snp_batch, `missing` other than "mean" or "skip"."""
    _check_snp_batch(snp_batch)
    if missing not in ("mean", "skip"):
        raise ValueError(f'missing must be "mean" or "skip", not {missing!r}')
    X = _genotypes(X, "prs")
    n, p = X.shape
    if n < 1 or p < 1:
        raise ValueError(f"prs needs at least one sample and one SNP: X holds n={n}, p={p}")
    labels, Wm = _weight_columns(weights)
    if Wm.shape[0] != p:
        raise ValueError(f"shape mismatch: {Wm.shape[0]} rows of weights for {p} SNPs")
    if samples is not None and len(samples) != n:
        raise ValueError(f"shape mismatch: {len(samples)} sample labels for {n} samples")
    t, t0 = Wm.shape[1], time.time()
    used = np.flatnonzero((Wm != 0).any(axis=1))
    if used.size == 0:
        S, Cn = np.zeros((t, n)), np.zeros((t, n), np.int64)
        if stats is not None:
            stats.update({"batches": 0, "bytes_in": 0, "seconds": time.time() - t0})
    else:
        if used.size <= (1 - _PRS_DROP) * p:
            X, Wm = _ld_take(X, used)[0], Wm[used]
        S, Cn = _prs_stream(X, np.ascontiguousarray(Wm.T), missing == "mean", bool(counts), device, snp_batch, verbose, stats)
    if stats is not None:
        stats["snps_used"] = int(X.shape[1]) if used.size else 0
    index = None if samples is None else pd.Index(samples)
    scores = pd.DataFrame(S.T, columns=labels, index=index)
    return (scores, pd.DataFrame(Cn.T, columns=labels, index=index)) if counts else scores


def _prs_stream(X, Wt, impute, counts, device, snp_batch, verbose, stats):
    """The streamed score: the (t, p) score-major weights uploaded once, then SNP batches from the feed (_feed._Feed) through
    pg_prs_{bed,x}_acc_dev — every group of 64 weight columns on each batch before the next is taken — into (t, n) accumulators on
    the device.  Returns the host arrays (scores, counts or None)."""
    L, t0 = _lib.load(), time.time()
    src = _describe(X)
    n, p = src.n, src.p
    t = Wt.shape[0]
    tg = min(t, _PRS_MAX_T)
    _gpus()
    with _lib.Context(device) as ctx, contextlib.closing(_Feed(ctx, src)) as feed:
        fixed = 8 * t * p + (16 if counts else 8) * t * n
        pb = _fit_batch(ctx, None if snp_batch is None else _chunk_up(snp_batch), _chunk_up(_lm_batch(src)), p, _PRS_CHUNK,
                        lambda pb: fixed + 2 * pb * src.row_bytes + int(L.pg_prs_work_bytes(n, pb, tg)),
                        f"prs: n={n}, p={p}, t={t}", "weights, score rows, two batch slots, the pre-pass and the chunk partials")
        if pb < p:
            pb = max(_PRS_CHUNK, pb // _PRS_CHUNK * _PRS_CHUNK)
        dW = ctx.to_device(Wt)
        work = ctx.alloc(L.pg_prs_work_bytes(n, pb, tg))
        dS, dC = ctx.alloc(8 * t * n), ctx.alloc(8 * t * n) if counts else None
        for buf in (dS, dC):
            if buf is not None:
                _lib.check(L.pg_memset(ctx.handle, buf.ptr, 0, 8 * t * n), "pg_memset")
        for s, e, slot in feed.batches(pb):
            for k0 in range(0, t, _PRS_MAX_T):
                tk = min(_PRS_MAX_T, t - k0)
                _call_dev(L, "pg_prs_{}_acc_dev", src, (ctx.handle, n, e - s), slot, e - s,
                          (tk, dW.ptr + 8 * (k0 * p + s), p, int(impute), work.ptr, dS.ptr + 8 * k0 * n, dC.ptr + 8 * k0 * n if counts else None, n))
            _log(verbose - 1, f"prs: SNPs [{s},{e}) queued")
        ctx.sync()
        out = dS.download((t, n), np.float64), dC.download((t, n), np.int64) if counts else None
    _stream_stats(stats, src, pb, t0)
    _log(verbose, f"Polygenic scores: {p} SNPs x {t} score(s) for {n} individuals in {time.time() - t0:.3f} s")
    return out


def prs_weights(df, loci=None, thresholds=(5e-8, 1e-5, 1e-3, 1e-2, 0.05, 1.0), col="p_wald", beta="beta"):
    """The weights of a clumping-and-thresholding score (PRSice's C+T) from a scan frame; pure NumPy.  df: the frame of a scan over p
    SNPs with its p-value column `col` and effect column `beta`; loci: the frame clump(df, X) returned, or None for no clumping.
    Returns a (p, t) float64 DataFrame with one column per threshold, labelled by it: column k holds beta_g where p_g <= thresholds[k]
    (equality counts), p_g and beta_g are finite and — with loci — g is one of loci["index"]; 0 elsewhere.  Hand it to prs.  ValueError:
    a missing column, a threshold outside [0, 1], an index outside the frame."""
    for name in (col, beta):
        if name not in df:
            raise ValueError(f"the frame has no column {name!r}")
    thresholds = list(thresholds)
    _check_unit(**{f"thresholds[{k}]": v for k, v in enumerate(thresholds)})
    pv, b = np.asarray(df[col], np.float64), np.asarray(df[beta], np.float64)
    p = len(pv)
    keep = np.isfinite(pv) & np.isfinite(b)
    if loci is not None:
        if "index" not in loci:
            raise ValueError("loci has no column 'index': it is not a frame of clump")
        idx = np.asarray(loci["index"])
        if idx.size and (idx.dtype.kind not in "iu" or idx.min() < 0 or idx.max() >= p):
            raise ValueError(f"loci holds an index outside the frame's {p} SNPs")
        index = np.zeros(p, bool)
        index[idx.astype(np.int64)] = True
        keep &= index
    with np.errstate(invalid="ignore"):
        cols = [np.where(keep & (pv <= thr), b, 0.0) for thr in thresholds]
    return pd.DataFrame(np.stack(cols, axis=1) if cols else np.zeros((p, 0)), columns=list(thresholds), index=df.index)


_PCA_MAX_L = 64      # PG_PCA_MAX_L: columns of the iterated block
_PCA_RESIDENT_BATCH = 65536      # SNPs per kernel call from a resident source: 512 strips of 128 SNPs for proj, two per compute unit
PcaResult = namedtuple("PcaResult", "pcs eigenvalues explained loadings stat")


def _pca_orth(A):
    """The orthonormal factor of the host fp64 Householder QR of A (n, l), with the diagonal of R made positive."""
    Q, R = np.linalg.qr(A)
    return Q * np.where(np.diagonal(R) < 0, -1.0, 1.0)[None, :]


def _pca_signs(U):
    """Every column of U with its entry of largest magnitude made positive."""
    U = np.array(U)
    for j in range(U.shape[1]):
        if U[np.argmax(np.abs(U[:, j])), j] < 0:
            U[:, j] = -U[:, j]
    return U


class _PcaPanel:
    """The genotypes of lmm.pca / lmm.pca_project on one GPU, for any number of passes of pg_pca_{stat,proj,back}_*: uploaded once and
    read from HBM in windows (`resident`: the source, stat, T, the panels and the work area fit into 0.9 of the free memory and no
    `snp_batch` was given), or streamed through a two-slot feed of its own per pass.  Either way a pass takes the SNPs in batches that
    are multiples of the summation chunk, so the bits are the same.  stat (p, 2) and T (l, p) stay on the device; Q and Y are (l, n)."""

    def __init__(self, ctx, X, l, snp_batch, who):
        L = self.L = _lib.load()
        src = self.src = _describe(X)
        self.ctx, self.l, self.passes = ctx, l, 0
        n, p = src.n, src.p
        fixed = 16 * p + 8 * l * p + 16 * l * n
        default = _chunk_up(_lm_batch(src))
        free, _total = ctx.mem_info()
        # from HBM a kernel call takes up to _PCA_RESIDENT_BATCH SNPs, halved down to the feed's batch while the chunk partials do not fit
        # (a sample-major source lies there batch by batch as the feed would put it, so its calls keep the upload's size)
        pbr = max(default, _PCA_RESIDENT_BATCH) if src.snp_major else default
        need = lambda pb: fixed + p * src.row_bytes + int(L.pg_pca_work_bytes(n, min(p, pb), l))      # noqa: E731
        while pbr > default and need(pbr) > 0.9 * free:
            pbr = max(default, pbr // 2)
        self.resident = snp_batch is None and need(pbr) <= 0.9 * free
        if self.resident:
            pb = min(p, pbr)
        else:
            pb = _fit_batch(ctx, None if snp_batch is None else _chunk_up(snp_batch), default, p, _PRS_CHUNK,
                            lambda pb: fixed + 2 * pb * src.row_bytes + int(L.pg_pca_work_bytes(n, pb, l)),
                            f"{who}: n={n}, p={p}, l={l}", "stat, T, two panels, two batch slots, the pre-pass and the chunk partials")
            if pb < p:
                pb = max(_PRS_CHUNK, pb // _PRS_CHUNK * _PRS_CHUNK)
        self.pb = pb
        self.work = ctx.alloc(L.pg_pca_work_bytes(n, pb, l))
        self.dstat, self.dT, self.dQ, self.dY = ctx.alloc(16 * p), ctx.alloc(8 * l * p), ctx.alloc(8 * l * n), ctx.alloc(8 * l * n)
        self.dX = None
        if self.resident:      # every batch where the feed would put it: SNP-major rows back to back, a sample-major window as n x (e - s)
            self.dX = ctx.alloc(p * src.row_bytes)
            up = min(p, default)
            ring = _Ring(ctx, up * src.row_bytes, staged=not src.direct)
            try:
                for j, s in enumerate(range(0, p, up)):
                    e = min(s + up, p)
                    ring.put(j, src.src, s, e, self.dX.ptr + s * src.row_bytes, None if src.snp_major else (e - s) * src.esz)
                ctx.sync()
            finally:
                ring.close()

    @contextlib.contextmanager
    def _batches(self):
        src, pb = self.src, self.pb
        self.passes += 1
        if self.resident:
            yield ((s, min(s + pb, src.p), self.dX.ptr + s * src.row_bytes) for s in range(0, src.p, pb))
        else:
            with contextlib.closing(_Feed(self.ctx, src)) as feed:
                yield feed.batches(pb)

    def sweep(self, stat=False, proj=0, back=0):
        """One pass over the SNPs: per batch its stat, then T = Z'Q for the first `proj` rows of dQ, then dY += Z T for the first `back`
        rows of dT.  Returns Y (back, n) from the device, or None."""
        L, ctx, src = self.L, self.ctx, self.src
        n, p = src.n, src.p
        if back:
            _lib.check(L.pg_memset(ctx.handle, self.dY.ptr, 0, 8 * back * n), "pg_memset")
        with self._batches() as batches:
            for s, e, slot in batches:
                head, st = (ctx.handle, n, e - s), self.dstat.ptr + 16 * s
                if stat:
                    _call_dev(L, "pg_pca_stat_{}_dev", src, head, slot, e - s, (self.work.ptr, st))
                if proj:
                    _call_dev(L, "pg_pca_proj_{}_dev", src, head, slot, e - s, (st, proj, self.dQ.ptr, n, self.dT.ptr + 8 * s, p))
                if back:
                    _call_dev(L, "pg_pca_back_{}_dev", src, head, slot, e - s, (st, back, self.dT.ptr + 8 * s, p, self.work.ptr, self.dY.ptr, n))
            ctx.sync()
        return self.dY.download((back, n), np.float64) if back else None

    def stream_stats(self, stats, t0, **more):
        if stats is not None:
            nb = -(-self.src.p // self.pb)
            stats.update({"resident": self.resident, "batches": nb * self.passes,
                          "bytes_in": self.src.p * self.src.row_bytes * (1 if self.resident else self.passes), "seconds": time.time() - t0, **more})


def _pca_source(X, who, samples, snps=None):
    X = _genotypes(X, who)
    n, p = X.shape
    if n < 1 or p < 1:
        raise ValueError(f"{who} needs at least one sample and one SNP: X holds n={n}, p={p}")
    if samples is not None and len(samples) != n:
        raise ValueError(f"shape mismatch: {len(samples)} sample labels for {n} samples")
    if snps is not None and len(snps) != p:
        raise ValueError(f"shape mismatch: {len(snps)} SNP names for {p} SNPs")
    return X, n, p


def pca(X, k=10, *, oversample=10, iters=12, tol=1e-10, seed=0, loadings=True, samples=None, snps=None, device=0, snp_batch=None, verbose=0,
        stats=None):
    """The top k principal components of the standardised genotypes — the covariates W of every scan here (plink2's --pca approx) —
    straight from the genotypes as they are stored, without the n x n kinship matrix and its eigensolver: randomised block subspace
    iteration with two skinny fp64 products per pass on the matrix pipe (csrc/pca.hip).

    X (n, p): whatever prs takes — a PackedBed, or an int8, uint8, float32 or float64 array in C or Fortran order, pinned or pageable.
    Values are snp_stats' (rounded to float32 per element; .bed code 01, NaN and +-Inf are missing, an 8-bit array has no missing
    code).  Z is lmm.kinship(standardize=True)'s: z_gi = (x_gi - mu_g) / sd_g with mu_g the mean of the called genotypes — the number
    snp_stats reports — sd_g the population sd over all n samples after mean imputation, and 0 for a missing call; a constant or
    all-missing SNP contributes zeros and still counts in p.  The eigenvalues are those of K = Z Z' / p.
    With l = min(k + oversample, 64, n):  Q = orth(default_rng(seed).standard_normal((n, l)));  per pass T = Z'Q, Y = Z T / p,
    B = sym(Q'Y) and its Ritz values by host eigh; stop when the top k moved less than `tol` relative to the largest, or after `iters`
    passes; otherwise Q = orth(Y).  orth is a host fp64 Householder QR with R's diagonal made positive.  pcs = Q V[:, :k], each column's
    entry of largest magnitude positive.  With `loadings` one more product gives L = Z' pcs / (p lambda), so that Z L = pcs for a
    converged component (pca_project).  Axes of ancestry, which have an eigenvalue gap, converge to rounding in a dozen passes; components
    inside the bulk of the spectrum have none and stay a few percent short (stats["converged"] says which case it was).
    Returns a PcaResult: pcs (n x k DataFrame PC1..PCk, indexed by `samples`), eigenvalues (k,), explained = eigenvalues / trace K
    (trace K = n p_used / p, p_used the SNPs with sd > 0), loadings (p x k DataFrame indexed by `snps`, or None) and stat (p, 2): mu_g
    and 1 / sd_g (0 for an unusable SNP).  Use it as  W = np.c_[np.ones(n), res.pcs]  in lmm.pygemma.
    When the source, stat, T and the work area fit into the free device memory and `snp_batch` is None, X is uploaded once and every
    pass runs from HBM; otherwise every pass streams through the two-slot feed in batches rounded up to 256 SNPs: the returned bits
    are the same.  `stats` receives resident, passes, converged, batches, bytes_in, seconds and seconds_orth (download, QR and upload
    of the n x l panel).  Single GPU.  Refused with ValueError before any device work: k < 1, k + oversample > 64, k > min(n, p),
    iters < 1, tol < 0, X not 2-D, empty or of another dtype, label lengths that do not match, a bad snp_batch; RuntimeError when no
    SNP is usable."""
    _check_snp_batch(snp_batch)
    for name, v, lo in (("k", k, 1), ("oversample", oversample, 0), ("iters", iters, 1)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < lo:
            raise ValueError(f"{name} must be an integer >= {lo}, not {v!r}")
    if k + oversample > _PCA_MAX_L:
        raise ValueError(f"pca iterates k + oversample <= {_PCA_MAX_L} columns, got k = {k}, oversample = {oversample}")
    if not tol >= 0:
        raise ValueError(f"tol must be >= 0, not {tol!r}")
    X, n, p = _pca_source(X, "pca", samples, snps)
    if k > min(n, p):
        raise ValueError(f"k = {k} components of a panel of n={n}, p={p}: at most min(n, p)")
    k, l, t0, t_orth = int(k), int(min(k + oversample, _PCA_MAX_L, n)), time.time(), 0.0
    Q = _pca_orth(np.random.default_rng(seed).standard_normal((n, l)))
    _gpus()
    with _lib.Context(device) as ctx:
        panel = _PcaPanel(ctx, X, l, snp_batch, "pca")
        panel.sweep(stat=True)
        stat = panel.dstat.download((p, 2), np.float64)
        p_used = int((stat[:, 1] > 0).sum())
        if p_used == 0:
            raise RuntimeError("pca: no SNP is usable (every SNP is constant or all missing)")
        prev, converged, done = None, False, 0
        for it in range(int(iters)):
            t1 = time.time()
            panel.dQ.upload(np.ascontiguousarray(Q.T))
            t_orth += time.time() - t1
            Yt = panel.sweep(proj=l, back=l)
            t1 = time.time()
            Y = np.ascontiguousarray(Yt.T) / p
            t_orth += time.time() - t1
            B = Q.T @ Y
            w, V = np.linalg.eigh((B + B.T) / 2)
            w, V = w[::-1], V[:, ::-1]
            done = it + 1
            _log(verbose - 1, f"pca: pass {done}, Ritz values {w[:k]}")
            if prev is not None and np.max(np.abs(w[:k] - prev[:k])) < tol * abs(w[0]):
                converged = True
                break
            prev = w
            if it + 1 < iters:
                t1 = time.time()
                Q = _pca_orth(Y)
                t_orth += time.time() - t1
        pcs, lam = _pca_signs(Q @ V[:, :k]), w[:k].copy()
        Lm = None
        if loadings:
            panel.dQ.upload(np.ascontiguousarray(pcs.T))
            panel.sweep(proj=k)
            Lm = panel.dT.download((l, p), np.float64)[:k].T / (p * lam)[None, :]
        panel.stream_stats(stats, t0, passes=done, converged=converged, seconds_orth=t_orth)
    cols = [f"PC{j + 1}" for j in range(k)]
    _log(verbose, f"PCA: {k} components of {p} SNPs x {n} individuals in {done} passes, {time.time() - t0:.3f} s")
    return PcaResult(pd.DataFrame(pcs, columns=cols, index=None if samples is None else pd.Index(samples)), lam, lam / (n * p_used / p),
                     None if Lm is None else pd.DataFrame(Lm, columns=cols, index=None if snps is None else pd.Index(snps)), stat)


def pca_project(X_new, res, *, samples=None, device=0, snp_batch=None, verbose=0, stats=None):
    """The samples of X_new (n_new, p) on the components of res = lmm.pca(..., loadings=True): Z_new L as an n_new x k DataFrame PC1..PCk
    indexed by `samples`.  X_new is standardised with res.stat — the TRAINING panel's means and sds, so a missing call is the training
    mean — and the product is one stream of pg_pca_back_* (chunks of 256 SNPs added in order: the bits do not depend on `snp_batch`).
    On the training panel itself it reproduces res.pcs for a converged component.  `stats` receives resident, batches, bytes_in,
    seconds.  Refused with ValueError before any device work: a result without loadings, X_new with another SNP count, not 2-D, empty
    or of another dtype, `samples` of another length, a bad snp_batch."""
    _check_snp_batch(snp_batch)
    if getattr(res, "loadings", None) is None:
        raise ValueError("pca_project needs the loadings of lmm.pca(..., loadings=True)")
    X_new, n, p = _pca_source(X_new, "pca_project", samples)
    Lm, stat = np.asarray(res.loadings, np.float64), np.ascontiguousarray(res.stat, np.float64)
    if Lm.ndim != 2 or Lm.shape[0] != p or stat.shape != (p, 2):
        raise ValueError(f"shape mismatch: X_new holds {p} SNPs, the result's loadings {Lm.shape[0]} and its stat {stat.shape[0]}")
    k, t0 = Lm.shape[1], time.time()
    if not 1 <= k <= _PCA_MAX_L:
        raise ValueError(f"pca_project takes 1 to {_PCA_MAX_L} components, got {k}")
    _gpus()
    with _lib.Context(device) as ctx:
        panel = _PcaPanel(ctx, X_new, k, snp_batch, "pca_project")
        panel.dstat.upload(stat)
        panel.dT.upload(np.ascontiguousarray(Lm.T))
        P = panel.sweep(back=k).T
        panel.stream_stats(stats, t0)
    _log(verbose, f"PCA projection: {n} individuals x {p} SNPs on {k} components in {time.time() - t0:.3f} s")
    return pd.DataFrame(P, columns=list(res.loadings.columns) if isinstance(res.loadings, pd.DataFrame) else [f"PC{j + 1}" for j in range(k)],
                        index=None if samples is None else pd.Index(samples))


def _zkzt(L, Z, K):
    """K <- Z K Z' (lmm/lmm.py:124-125) on GPU 0: Z (n, q), K (q, q), float32 or float64 each; returns the float32 (n, n) matrix that
    lmm.py:127-128 would hand to the eigensolver.  The reference does this as host BLAS products (4e12 flops at n = q = 10 000)."""
    if Z.ndim != 2 or K.ndim != 2 or K.shape[0] != K.shape[1] or Z.shape[1] != K.shape[0]:
        raise ValueError(f"Z {Z.shape} and K {K.shape} do not multiply as Z K Z'")
    def dev_ready(a):
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        return np.ascontiguousarray(a)
    Z, K = dev_ready(Z), dev_ready(K)
    n, q = Z.shape
    with _lib.scope() as ctx:
        dZ, dK, dO = ctx.to_device(Z), ctx.to_device(K), ctx.alloc(n * n * 4)
        _lib.check(L.pg_zkzt_dev(ctx.handle, n, q, dZ.ptr, int(Z.dtype == np.float64), q, dK.ptr, int(K.dtype == np.float64), q, dO.ptr, n),
                   "pg_zkzt_dev")
        return dO.download((n, n), np.float32)


def pygemma(Y, X, W, K, Z=None, snps=None, verbose=0, disable_checks=True, de=False, grid=False, eigen=True, nproc=1,
            checkpoint=None, lrt=False, eigenpairs=None, stats=None):
    """Per-SNP LMM association scan (GEMMA-style REML + Wald test) — signature of lmm/lmm.py:87.

    Y (n,1) phenotype; X (n,p) genotypes; W (n,c) covariates; K (n,n) relatedness matrix — or, with
    eigen=False, the (n,) vector of its eigenvalues with X, Y, W already rotated (lmm.py:164-167).
    Returns a pandas.DataFrame with columns beta, se_beta, tau, lambda, F_wald, p_wald[, SNPs].
    Beyond the reference (all keyword-only in spirit, defaults reproduce the reference):
      * X may be a `pygemma_amd.bed.PackedBed` (PLINK .bed kept packed; missing calls mean-imputed on the device, as the
        reference's callers do on the host before calling);
      * `checkpoint` names a directory that receives every finished SNP batch; a rerun with the same inputs picks up from
        what is there (the reference has no restart), a rerun with other inputs is refused;
      * `lrt=True` appends l_alt, l_null, D_lrt, p_lrt — the likelihood-ratio columns the reference sketches and leaves
        commented out (lmm.py:137-141, 277-300), from its own ML functions (lmm.py:22-84, pygemma_model.pyx:1542-1603);
      * `eigenpairs=(eigenVals, U)`: a precomputed eigendecomposition of K (U column j = eigenvector j, as scipy.linalg.eigh
        returns it) — K is ignored, U is streamed to the GPU(s) from host memory (pinned if made with `pinned_empty`) and the
        rotation runs on the device (BASELINE config 5);
      * `stats`: a dict that receives streaming counters (batches, bytes_in, seconds).
    """
    if de:
        # calculate_de is broken upstream (unpacks 4 of SampleIter's 5-tuple, lmm/lmm.py:499 vs :434)
        raise NotImplementedError("de=True is broken in the reference (lmm/lmm.py:499) and is not provided")
    out = _scan(Y, X, W, K, Z=Z, verbose=verbose, disable_checks=disable_checks, grid=grid, eigen=eigen, nproc=nproc,
                checkpoint=checkpoint, lrt=lrt, eigenpairs=eigenpairs, stats=stats)
    return _frame(out, list(out), snps)


def pygemma_multi(Y, X, W, K, Z=None, snps=None, verbose=0, disable_checks=True, grid=False, eigen=True, nproc=1,
                  eigenpairs=None, stats=None):
    """lmm.pygemma for several phenotypes over the same X, W and K (the loop the reference's callers write by hand:
    experiments/wtccc/run_pygemma_imputed.py:516-532, experiments/animal_gwas/run_gwas.py:167-175).

    Y: (n, t) array or DataFrame, or (n,); every column is cast to float32 as lmm.pygemma casts its Y (lmm.py:115-116).
    Returns a dict in column order — keys: Y's column labels for a DataFrame, else 0..t-1 — of DataFrames that are
    bit-identical to lmm.pygemma(Y[:, k], X, W, K, ...) with the same arguments.  The eigendecomposition, the transport and
    rotation of every SNP batch and the phenotype-free part of the decade scan are done once for all phenotypes.  Samples are
    never dropped per phenotype: a NaN phenotype yields the rows a single run would give (disable_checks=False raises instead),
    the other phenotypes are unaffected — mean-impute missing values beforehand as the reference's callers do.  No lrt,
    checkpoint or de.  `stats` receives lmm.pygemma's counters plus `phenotypes`."""
    labels, cols = _pheno_columns(Y)
    n = X.shape[0]
    if cols[0].shape[0] != n:
        raise ValueError(f"shape mismatch: Y has {cols[0].shape[0]} rows, X {n}")
    Y32 = np.stack(cols, axis=1)
    out = _scan(Y32, X, W, K, Z=Z, verbose=verbose, disable_checks=disable_checks, grid=grid, eigen=eigen, nproc=nproc,
                eigenpairs=eigenpairs, stats=stats, npheno=len(cols))
    return {lab: _frame(out, _COLS, snps, k) for k, lab in enumerate(labels)}


def pygemma_score(Y, X, W, K, Z=None, snps=None, verbose=0, disable_checks=True, eigen=True, nproc=1, eigenpairs=None, stats=None):
    """Score test over every SNP at the null model's ML lambda (GEMMA's -lmm 3) — the usual first screen of a whole genome: score
    everything, then run lmm.pygemma (Wald, or lrt=True) on the hits.  Same inputs as lmm.pygemma (Y, X, W, K, Z, snps, eigen,
    nproc, eigenpairs; every X kind it takes).

    lambda0 = the ML lambda of y ~ W (calc_lambda, lmm/lmm.py:22-84) is fitted once, on GPU 0, and every SNP is evaluated at it:
    with h = 1/(lambda0 d + 1) and P0 = H - HW (W'HW)^-1 W'H in the eigenbasis (fp64), P_xx = x'P0x, P_xy = x'P0y, P_yy = y'P0y,
    Px_yy = P_yy - P_xy^2/P_xx, df = n - c - 1:
      beta = P_xy/P_xx, se_beta = sqrt(Px_yy/(df P_xx)), tau = df/Px_yy, lambda = lambda0   (float32; float64 for lambda)
      F_score = n P_xy^2/(P_yy P_xx), p_score = F(1, df).sf(F_score)                        (float64)
    A SNP that is constant or lies in span(W) (P_xx <= 1e-10 x'Hx), or holds a NaN/inf, gets NaN in every column but lambda; a
    rank-deficient W gives NaN rows throughout.  No grid (the null search is Brent's), lrt or checkpoint.  `stats` receives
    lmm.pygemma's counters plus `lambda_null`."""
    out = _scan(Y, X, W, K, Z=Z, verbose=verbose, disable_checks=disable_checks, eigen=eigen, nproc=nproc, eigenpairs=eigenpairs,
                stats=stats, score=True)
    return _frame(out, list(out), snps).rename(columns={"F_wald": "F_score", "p_wald": "p_score"})


def _e_in_span(W, e):
    """True when the float32 column e lies in the span of W's columns, up to float32 rounding: the least-squares residual of e on W
    (fp64) is within a few float32 ulps of e's own terms.  Scale-invariant: an uncentred e beside an intercept (a blood pressure
    of 130 +- 15, a birth year) has a residual of its spread's size and is accepted at any n."""
    W64, e64 = W.astype(np.float64), e.astype(np.float64)
    coef = np.linalg.lstsq(W64, e64, rcond=None)[0]
    r = e64 - W64 @ coef
    scale = np.linalg.norm(e64) + np.abs(coef) @ np.linalg.norm(W64, axis=0)
    return bool(np.linalg.norm(r) <= 16 * np.finfo(np.float32).eps * scale)


def pygemma_gxe(Y, X, W, K, E, Z=None, snps=None, verbose=0, disable_checks=True, eigen=True, nproc=1, eigenpairs=None, checkpoint=None,
                stats=None):
    """SNP-by-environment interaction scan (GEMMA's -gxe): per SNP j, the REML Wald test of beta_gxe in

        y = W alpha + e gamma + x_j beta_x + (x_j o e) beta_gxe + g + eps,   g ~ N(0, lambda/tau K),  eps ~ N(0, 1/tau I)

    with lambda searched per SNP under this full model (lmm.pygemma's decade scan + brentq + Newton; no grid).  E: the environment
    e, (n,) or (n, 1), cast to float32 like W; it always enters the model as a covariate (appended to W).  Same inputs otherwise as
    lmm.pygemma (Y, X, W, K, Z, snps, eigen=True, nproc, eigenpairs, checkpoint, stats; every X kind it takes).  Returns the columns
    beta, se_beta, tau, lambda, F_wald, p_wald[, SNPs] of lmm.pygemma, with beta = beta_gxe and p_wald from F(1, n - c - 3).

    In the eigenbasis row j is calculate(d, U'y, [U'W, U'e, U'x_j], U'(x_j o e)).  U'(x o e) = (diag(e) U)' x: each GPU scales
    its copy of U once and rotates every SNP batch twice, by the path lmm.pygemma picks for X (which depends on X only).  A
    missing .bed call is imputed before e is applied, as in host X o e.  On the int8 x 3 genotype path diag(e) U is held per
    eigenvector in fixed point relative to max_i |e_i u_ik|: an eigenvector whose weight e concentrates on few samples loses
    relative precision elsewhere, the error class of localised eigenvectors on that path.  Degenerate SNPs (constant, x o e
    in span([W, e, x]), non-finite) give NaN where calculate() does.  Refused before any device work: E not (n,) / (n, 1) or not
    finite, e in span(W) (rank of [W, e] in fp64), W with other than 1..28 columns, n - c - 3 <= 0, eigen=False (x o e cannot be
    formed from rotated X: use ops.gxe with U'X and U'(X o e)).  The checkpoint manifest records the interaction run (`gxe`,
    `e_crc`), so a Wald run's directory is refused and vice versa."""
    if not eigen:
        raise ValueError("pygemma_gxe needs eigen=True: x o e cannot be formed from rotated genotypes; in the eigenbasis call "
                         "ops.gxe(d, [U'W, U'e], U'y, U'X, U'(X o e)) instead")
    W = np.asarray(W)
    if W.ndim != 2 or not 1 <= W.shape[1] <= 28:
        raise ValueError(f"the interaction scan takes W with 1 to 28 columns (e makes one more covariate), got W {W.shape}")
    n = X.shape[0]
    e = np.asarray(E)
    if e.shape not in ((n,), (n, 1)):
        raise ValueError(f"E must be of shape ({n},) or ({n}, 1), got {e.shape}")
    e = e.reshape(-1).astype(np.float32)
    if not np.isfinite(e).all():
        raise ValueError("E holds non-finite values")
    if W.shape[0] != n:
        raise ValueError(f"shape mismatch: X has {n} rows, W {W.shape[0]}")
    W32 = W.astype(np.float32)
    We = np.concatenate([W32, e[:, None]], axis=1)
    if _e_in_span(W32, e):
        raise ValueError("[W, e] is rank-deficient: e lies in the span of W's columns")
    c = We.shape[1]
    if n - c - 2 <= 0:
        raise ValueError(f"the interaction scan needs n - c - 3 > 0 (n = {n}, c = {c - 1} columns of W)")
    out = _scan(Y, X, We, K, Z=Z, verbose=verbose, disable_checks=disable_checks, eigen=True, nproc=nproc, eigenpairs=eigenpairs,
                checkpoint=checkpoint, stats=stats, gxe=e)
    return _frame(out, list(out), snps)


def _null_lambda(L, n, c, d, Wr, yr):
    """lambda0 of the score test: the ML lambda of y ~ W on GPU 0 (pg_score_null_dev), read back as one float32."""
    with _lib.scope() as ctx:
        dd, dW, dy, dl = ctx.to_device(d), ctx.to_device(Wr), ctx.to_device(yr), ctx.alloc(4)
        _lib.check(L.pg_score_null_dev(ctx.handle, n, c, dd.ptr, dW.ptr, dy.ptr, dl.ptr), "pg_score_null_dev")
        ctx.sync()
        return np.float32(dl.download((1,), np.float32)[0])


def _inputs(L, Y, X, W, K, Z, eigen, eigenpairs, score):
    """Checks and casts of the inputs (lmm.py:113-128), all before any device is touched but _zkzt's: Y, X, W, K as the scan takes
    them."""
    packed = isinstance(X, PackedBed)                         # extension: a PLINK .bed image instead of the float matrix
    if packed and not eigen:
        raise ValueError("a PackedBed holds raw genotypes: it cannot be used with eigen=False (pre-rotated inputs)")
    if eigenpairs is not None and not eigen:
        raise ValueError("eigenpairs supplies U for the rotation: it goes with eigen=True")
    Y, W = np.asarray(Y), np.asarray(W)
    K = np.asarray(K) if K is not None else None
    if not packed:
        X = np.asarray(X)
    if Y.dtype != np.float32:
        Y = Y.astype(np.float32).reshape(-1, 1)              # lmm.py:115-116
    if W.dtype != np.float32:
        W = W.astype(np.float32)                             # lmm.py:118-119
    # int8/uint8/float64 X stays as it is up to the device when it is rotated there: the kernels convert each element to
    # float32 as they read it, which is what the cast below does (round to nearest) — no host copy of the matrix
    x8 = (not packed) and eigen and X.dtype in (np.int8, np.uint8, np.float64)
    if not packed and not x8 and X.dtype != np.float32:
        X = X.astype(np.float32)                             # lmm.py:121-122
    if eigenpairs is None:
        if Z is not None:
            K = _zkzt(L, np.asarray(Z), K)                   # lmm.py:124-125, on GPU 0 (two fp64-MFMA products, one rounding to float32)
        k64 = eigen and K.dtype == np.float64                # rounded to float32 on the device instead (same values, no host copy)
        if K.dtype != np.float32 and not k64:
            K = K.astype(np.float32)                         # lmm.py:127-128
    # A Fortran-ordered float32 X is the SNP-major image (p rows of n samples): its batches are contiguous byte ranges that go to the
    # device as they are (and are turned sample-major there when they have to be rotated) — no transposing host copy of the matrix
    if not packed and not X.flags.c_contiguous and not (X.ndim == 2 and X.dtype == np.float32 and X.flags.f_contiguous):
        X = np.ascontiguousarray(X)
    n, c = X.shape[0], W.shape[1]
    if Y.shape[0] != n or W.shape[0] != n:
        raise ValueError(f"shape mismatch: Y {Y.shape}, X {X.shape}, W {W.shape}")
    if score:
        if W.ndim != 2 or not 1 <= c <= 30:
            raise ValueError(f"the score test takes 1 to 30 covariates, got W {W.shape}")
        if n - c - 1 <= 0:
            raise ValueError(f"the score test needs n - c - 1 > 0 (n = {n}, c = {c})")
    return Y, X, W, K


def _eigenbasis(L, ectx, n, Y, W, K, eigenpairs, ty, verbose, t0):
    """U on GPU 0 (ectx's device) — from the host `eigenpairs`, or pg_syevd_dev of K — and [Y | W] rotated by it: returns the
    eigenvalues, U and the rotated first `ty` columns of Y and W."""
    if eigenpairs is not None:
        ev, Uh = eigenpairs
        Uh = np.asarray(Uh)
        if Uh.shape != (n, n):
            raise ValueError(f"eigenpairs: U must be ({n},{n}), got {Uh.shape}")
        if Uh.dtype != np.float32 or not Uh.flags.c_contiguous:
            Uh = np.ascontiguousarray(Uh, np.float32)                       # lmm.py:154
        eigenVals = np.maximum(0.0, np.asarray(ev)).astype(np.float32).reshape(-1)   # lmm.py:157-160
        if eigenVals.shape[0] != n:
            raise ValueError(f"eigenpairs: {n} eigenvalues expected, got {eigenVals.shape}")
        dU0 = ectx.alloc(n * n * 4)
        # U's n rows of n floats are the SNP-major rows of Uh.T
        if _lib.is_pinned(Uh):     # one DMA straight out of the caller's pinned array
            _put_window(ectx, Uh.T, 0, n, dU0.ptr)
            ectx.sync()
        else:                      # pageable: row panels through two pinned buffers, copy threads ahead of the DMA
            rows = max(1, min(n, _U_PANEL_BYTES // (n * 4)))
            with contextlib.closing(_Ring(ectx, rows * n * 4)) as ring:
                for j, r0 in enumerate(range(0, n, rows)):
                    ring.put(j, Uh.T, r0, min(n, r0 + rows), dU0.ptr + r0 * n * 4)
                ectx.sync()
        _log(verbose, f"Eigenvectors uploaded ({n * n * 4 / 1e9:.2f} GB) - {time.time() - t0:.3f} s")
    else:
        if K.shape != (n, n):
            raise ValueError(f"K must be ({n},{n}) when eigen=True, got {K.shape}")
        if K.dtype == np.float64:
            dK64 = ectx.to_device(np.ascontiguousarray(K))
            dK = ectx.alloc(n * n * 4)
            _lib.check(L.pg_cast_f64_f32_dev(ectx.handle, n, n, dK64.ptr, n, dK.ptr, n), "pg_cast_f64_f32_dev")   # lmm.py:127-128
            ectx.sync()
            dK64.free()
        else:
            dK = ectx.to_device(K)
        dev, dU0 = ectx.alloc(n * 4), ectx.alloc(n * n * 4)
        _lib.check(L.pg_syevd_dev(ectx.handle, n, dK.ptr, dev.ptr, dU0.ptr, None, None), "pg_syevd_dev")
        dK.free()
        eigenVals = dev.download((n,), np.float32)       # ascending, clamped >= 0, float32 (lmm.py:152-160)
        _log(verbose, f"Eigendecomposition computed - {time.time() - t0:.3f} s")
    assert (eigenVals >= 0).all()                        # lmm.py:162
    t1 = time.time()
    # [Y | W] in one rotation: an output column's bits do not depend on the columns beside it (rotate.hip)
    YW = _rotate_small(ectx, L, n, dU0, np.concatenate([Y.reshape(n, -1)[:, :ty], W], axis=1))
    _log(verbose, f"Left multiplied Y, W by U.T - {time.time() - t1:.3f} s")
    return eigenVals, dU0, YW[:, :ty], np.ascontiguousarray(YW[:, ty:])


def _check_manifest(checkpoint, key):
    """The checkpoint directory's manifest.json: written on the first run, and a rerun with another `key` is refused."""
    os.makedirs(checkpoint, exist_ok=True)
    mf = os.path.join(checkpoint, "manifest.json")
    if os.path.exists(mf):
        with open(mf) as f:
            if json.load(f) != key:
                raise ValueError(f"checkpoint directory {checkpoint} belongs to a different run (manifest mismatch)")
    else:
        with open(mf, "w") as f:
            json.dump(key, f)


def _scan(Y, X, W, K, *, Z=None, verbose=0, disable_checks=True, grid=False, eigen=True, nproc=1, checkpoint=None, lrt=False,
          eigenpairs=None, stats=None, npheno=0, score=False, gxe=None):
    """The pipeline under pygemma (npheno = 0: Y is one phenotype), pygemma_multi (Y: float32 (n, npheno)), pygemma_score
    (score = True: F_wald / p_wald hold F_score / p_score) and pygemma_gxe (gxe: the float32 environment (n,), already the last
    column of W).  Returns the result columns: arrays of p values, or npheno x p with npheno > 0."""
    L = _lib.load()
    Y, X, W, K = _inputs(L, Y, X, W, K, Z, eigen, eigenpairs, score)
    nproc = min(int(nproc), X.shape[1])                      # lmm.py:113
    src = _describe(X)                                       # (src.direct: as X is now; settled once X has been page-locked below)
    n, p, c = src.n, src.p, W.shape[1]
    ty = npheno or 1                                         # phenotype columns of Y that are used
    blocks = list(SampleIter(p, max(1, min(nproc, _gpus()))))   # one contiguous block per GPU, none empty
    ndev = len(blocks)

    t0 = time.time()
    ectx = dU0 = None  # the eigensolver's context on GPU 0 and U resident there (reused by GPU 0's SNP loop)
    xpin = pre = pin_thread = comms = None
    pin_box = {}       # page-locking of a pageable X, beside the eigensolver or before the blocks start

    def page_lock():   # in place (hipHostRegister); a refusal is kept for the log
        try:
            pin_box["h"] = _lib.pin(X)
        except _lib.PgError as ex:
            pin_box["err"] = ex
    errs = []
    # ONE try/finally owns every resource made from here on (prefetch contexts and threads, the page-lock of X, the communicators,
    # the eigensolver's context): whatever raises in between — a bad K or U, NaNs, the manifest, a GPU's block — releases them all
    # in the order of the finally clause
    try:
        if eigen and eigenpairs is None and not checkpoint and _PREFETCH_MAX > 0 and not src.snp_major and src.direct:
            # the eigensolver leaves PCIe idle for ~0.6 s at n = 10 000 (52 s at 50 000): a pinned sample-major X starts moving now
            try:
                pre = _Prefetch(L, src, blocks, verbose, gxe is not None)
            except _lib.PgError as ex:
                _log(verbose, f"prefetch not started ({ex})")
        if eigen and not src.packed and not src.direct and X.nbytes >= (256 << 20):
            # Page-locking a pageable X in place costs ~0.06 s/GB the first time a range is registered (0.23 s for 4 GB: the kernel pins a million
            # pages; 2 ms on a repeat) — as long as the eigensolver runs anyway, it happens beside it on a thread of its own (r4: lmm.pygemma
            # from a pageable 4 GB X 0.77 -> ~0.5 s)
            pin_thread = threading.Thread(target=page_lock, daemon=True)
            pin_thread.start()
        if eigen:
            ectx = _lib.Context(0)
            eigenVals, dU0, Yr, Wr = _eigenbasis(L, ectx, n, Y, W, K, eigenpairs, ty, verbose, t0)
        else:
            eigenVals = np.maximum(0.0, K).astype(np.float32).reshape(-1)   # lmm.py:166-167
            if eigenVals.shape[0] != n:
                raise ValueError(f"with eigen=False K must hold the {n} eigenvalues, got {K.shape}")
            Yr, Wr = Y.reshape(n, -1)[:, :ty], np.ascontiguousarray(W)

        if not disable_checks:
            # lmm.py:253-256 (the reference tests the rotated arrays; a NaN anywhere in a raw column makes that
            # whole rotated column NaN, so testing the inputs raises in exactly the same cases)
            if (not src.packed and X.dtype.kind == 'f' and np.isnan(X).any()) or np.isnan(Yr).any() or np.isnan(Wr).any():
                raise ValueError("NaNs present in data")

        _log(verbose, f"Running {p} SNPs with {n} individuals on {ndev} GPU(s)...")
        shp = (npheno, p) if npheno else p
        out = {col: np.empty(shp, np.float32 if k < 3 else np.float64) for k, col in enumerate(_COLS)}
        out.update({col: np.empty(p, np.float64) for col in _LRT_COLS if lrt})
        if stats is not None:
            stats.update({"batches": 0, "bytes_in": 0, "batch_s": 0.0, "gpus": ndev})
            if npheno:
                stats["phenotypes"] = npheno
        yr1 = np.ascontiguousarray(Yr.T if npheno else Yr.reshape(-1), np.float32)    # (npheno, n): phenotype-major rows
        lam0 = None
        if score:      # once per call, on GPU 0; every GPU's shard gets the same float
            lam0 = _null_lambda(L, n, c, eigenVals, np.ascontiguousarray(Wr, np.float32), yr1)
            _log(verbose, f"Null model: lambda0 = {float(lam0):.6g}")
            if stats is not None:
                stats["lambda_null"] = float(lam0)
        if checkpoint:
            # identity of the run: shapes, options, batch geometry and the SNP-independent inputs themselves (rotated y, W and the
            # eigenvalues, byte for byte); the genotypes are fingerprinted per part (_block_fingerprint)
            key = {
                "n": int(n), "p": int(p), "c": int(c), "grid": bool(grid), "eigen": bool(eigen), "ndev": int(ndev), "lrt": bool(lrt),
                "batch_snps": int(_BATCH_SNPS), "batch_bytes": int(_BATCH_BYTES), "batch_min": int(_BATCH_MIN), "batch_count": int(_BATCH_COUNT),
                "y_crc": _crc(yr1), "w_crc": _crc(Wr), "d_crc": _crc(eigenVals)}
            if gxe is not None:        # an interaction run: never mixed with a Wald run's parts (whose manifest has no such keys)
                key.update({"gxe": True, "e_crc": _crc(gxe)})
            _check_manifest(checkpoint, key)
        t2 = time.time()
        if pre is not None:
            pre.join()
            if stats is not None:
                stats["prefetched_bytes"] = int(pre.bytes)
        if pin_thread is not None:
            pin_thread.join()
        elif not src.packed and not src.direct:
            # page-lock the caller's X in place for the duration of the scan (hipHostRegister: 2 ms/GB for a range the kernel has pinned
            # before, ~60 ms/GB the first time: tools/probe_pageable.py) so that every batch is one 2-D DMA straight out of it; if the
            # range cannot be registered (e.g. a read-only file mapping) the workers fall back to copy threads + a pinned staging buffer
            page_lock()
        xpin = pin_box.pop("h", None)
        if "err" in pin_box:
            _log(verbose, f"X could not be page-locked in place ({pin_box['err']}); staging through pinned buffers")
        src = src._replace(direct=src.direct or xpin is not None)
        if stats is not None:      # (pinned_input: what the DMA reads directly here, see _block_setup)
            stats.update(pinned_input=src.direct and not src.packed, registered_in_place=xpin is not None)
        dUs = [dU0] + [None] * (ndev - 1)
        if ndev > 1 and eigen:
            comms = _make_comms(L, ndev)      # RCCL communicator over the GPUs of this process: U goes GPU 0 -> all over xGMI
            for g in range(1, ndev):          # receive buffers made here: an allocation failure surfaces before any thread waits in the collective
                dUs[g] = comms[g].ctx.alloc(n * n * 4)
        job = _Job(n, c, eigenVals, Wr, yr1, src, grid, eigen, _scan_mode(L, n, c, grid, lrt, npheno, lam0, gxe is not None), checkpoint,
                   stats, pre, verbose, out, errs, gxe)
        _run_threads(_run_block, [(job, g, a, b, dUs[g], comms[g] if comms else None) for g, (a, b) in enumerate(blocks)])
        if stats is not None:
            stats["blocks_s"] = time.time() - t2          # page-locking + every GPU's block; what follows is teardown (frees)
    finally:
        if pre is not None:
            pre.close()                   # frees the prefetched batches only now: hipFree inside the loop would drain the device
        if pin_thread is not None:        # something raised while X was being page-locked: wait for it, and undo it below
            pin_thread.join()
            xpin = xpin or pin_box.pop("h", None)
        if xpin is not None:
            xpin.close()
        for cm in comms or ():
            L.pg_comm_destroy(cm.handle)
            cm.ctx.close()
        if ectx is not None:
            ectx.close()
    if errs:
        raise errs[0]
    if stats is not None:
        stats["seconds"] = time.time() - t2
    _log(verbose, f"Finished testing {p} SNPs in {time.time() - t2:.3f} s")
    return out
