"""gfrs_read_queue on the GPU: crc32block verify, ReconstructData and unframe
of a segment per job, in one call (include/gfrs.h, read-queue contract).

Every queue comes from tests/_readq.py and every expectation from the oracle
alone (original data bytes of the segment; pyoracle.crc32 of every touched
frame against its stored header); tests/test_read_queue_cpu.py checks on the
CPU that those expectations are self-consistent.  Each run compares both
guarded arenas in full: in out the n rows of every job hold the segment and
no other byte - padding between rows, guards - has changed (rows of a job are
left out only where the oracle's word for it is nonzero); framed is
byte-for-byte unchanged.
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _arena as A  # noqa: E402
import _encq as E  # noqa: E402
import _readq as G  # noqa: E402
from _arena import Arena  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", G.CLEAN_QUEUES)
def test_clean_queues(dev, name):
    """RS(6+3), RS(4+4) up to R = 4, RS(12+4), LRC12P2L2 (a pattern names a
    local parity) and RS(6+6) with R <= 4: empty, data-only, parity-only and
    mixed patterns in every bucket, every segment shape; words all 0."""
    assert not any(G.words(name))
    G.run(dev, name)


@pytest.mark.parametrize("name", G.SLOW_QUEUES)
def test_slow_and_identity(dev, name):
    """RS(6+6) with 5 and 6 missing data shards (one job at a time) next to
    fused jobs; the 17-shard tactic: identity items for the copy-only
    patterns, the slow path for a rebuild."""
    G.run(dev, name)


@pytest.mark.parametrize("name", G.CORRUPT_QUEUES)
def test_corruption(dev, name):
    """One flipped bit per odd job - payload bytes at vector, pass and frame
    edges, a stored header, a frame outside the segment, a non-input shard -
    on the fused, slow and identity paths.  The word is the oracle's; the
    clean half of the queue, and every job whose flip the segment does not
    touch, is compared in full."""
    assert sum(1 for w in G.words(name) if w == 0) * 2 >= len(G.words(name))
    G.run(dev, name)


@pytest.mark.parametrize("grid", ["1", "3"])
def test_forced_walk_and_restage(dev, monkeypatch, grid):
    """GFRS_CRC_GRID is read on every launch: with 1 block, one block walks
    every frame of a bucket across every job and descriptor change; with 3,
    a block starts in the middle of a bucket."""
    monkeypatch.setenv("GFRS_CRC_GRID", grid)
    G.run(dev, "rs63", what="grid=%s" % grid)
    G.run(dev, "corrupt_rs63", what="grid=%s" % grid)
    G.run(dev, "rs134_w17", what="grid=%s" % grid)


@pytest.mark.parametrize("waves", ["3", "4"])
def test_both_wave_builds(dev, monkeypatch, waves):
    """GFRS_RD_WAVES is read on every launch: both builds of every R = 0..4,
    whichever the launcher picks by default."""
    monkeypatch.setenv("GFRS_RD_WAVES", waves)
    G.run(dev, "rs44", what="waves=%s" % waves)


def test_python_surface(dev):
    q = G.build("corrupt_rs63")
    src, dst = G.load(q, dev, seed=72)
    enc = A.encoder(q.t)
    w = enc.read_queue(
        dst.dev, src.dev,
        [(src.off + job[0],) + job[1:5] + (dst.off + job[5],) + job[6:]
         for job in q.jobs], q.patterns)
    assert isinstance(w, np.ndarray) and w.dtype == np.uint32
    G.check(q, src, dst, [int(x) for x in w], what="Encoder.read_queue")


def test_reads_back_what_the_encode_queue_wrote(dev):
    """PUT then degraded GET: images from gfrs_encode_frame_queue, read with a
    pattern that misses m data shards; out equals the source data."""
    eq = E.build("rs63_mixed")
    enc = A.encoder(eq.t)
    src, framed = E.load(eq, dev, seed=74)
    A.ok(E.call(enc, src, framed, eq), "encode queue")
    t = eq.t
    pats = [[0, 2, 5], [1, 3, 4], []]
    jobs, at = [], 0
    for j, (_, slen, img_off, stride) in enumerate(eq.jobs):
        ostride = G.round4(slen) + 4 * (j % 3)
        jobs.append((img_off, stride, slen, 0, slen, at, ostride, j % 3))
        at += t.N * ostride + 4 * (j % 2)
    dst = Arena(dev, at, 4, seed=75)
    dst.upload()
    bad, boff = G.pattern_arrays(pats)
    w = (ctypes.c_uint32 * len(jobs))()
    rc = A.L().gfrs_read_queue(enc._ctx, A.vp(dst.ptr), A.vp(framed.ptr),
                               G.gjob_array(jobs), len(jobs), bad, boff,
                               len(pats), A.BLOCK, w)
    A.ok(rc, "read queue over the encode queue's images")
    assert list(w) == [0] * len(jobs)
    want = dst.expect()
    for j, job in enumerate(jobs):
        for i in range(t.N):
            dst.put(job[5] + i * job[6], eq.data[j][i], want)
    dst.check(want, what="read after encode: rows")


def test_errors_write_nothing(dev):
    q = G.build("rs44")
    enc = A.encoder(q.t)
    src, dst = G.load(q, dev, seed=76)
    jobs = list(q.jobs)
    n = len(jobs)

    def refused(code, what, enc=enc, src=src, dst=dst, q=q, **kw):
        rc, _ = G.call(enc, src, dst, q, **kw)
        assert rc == code, (what, rc)
        src.check(src.expect(), what="refused (framed): " + what)
        dst.check(dst.expect(), what="refused (out): " + what)

    names = ["img_off", "img_stride", "slen", "seg_off", "seg_len", "out_off",
             "out_stride", "pattern", "reserved"]

    def swap(j, **f):
        v = dict(zip(names, jobs[j] + (0,)))
        v.update(f)
        return jobs[:j] + [tuple(v[k] for k in names)] + jobs[j + 1:]

    whole = [j for j, job in enumerate(jobs)
             if job[3] == 0 and job[4] == job[2] >= 64][-1]
    refused(G.ERR_BLOCK, "block_len 0", block_len=0)
    refused(G.ERR_BLOCK, "block_len 65540", block_len=65540)
    refused(G.ERR_UNSUPPORTED, "block_len 4096", block_len=4096)
    refused(G.ERR_UNSUPPORTED, "block_len 131072", block_len=131072)
    refused(G.ERR_INVALID, "pattern index out of range",
            patterns=q.patterns + [[q.total]])
    refused(G.ERR_INVALID, "repeated index in an unused pattern",
            patterns=q.patterns + [[1, 1]])
    refused(G.ERR_TOO_FEW, "m + 1 global losses",
            patterns=q.patterns + [[0, 1, 2, 6, 7]])
    refused(G.ERR_INVALID, "njobs = 0", njobs=0)
    refused(G.ERR_INVALID, "npat = 0", npat=0)
    refused(G.ERR_INVALID, "bad_off not starting at 0",
            bad_off=[1] * (len(q.patterns) + 1))
    refused(G.ERR_INVALID, "pattern outside [0, npat)",
            jobs=swap(n - 1, pattern=len(q.patterns)))
    refused(G.ERR_INVALID, "reserved != 0", jobs=swap(3, reserved=1))
    refused(G.ERR_INVALID, "seg_off misaligned",
            jobs=swap(whole, seg_off=2, seg_len=8))
    refused(G.ERR_INVALID, "out_off misaligned",
            jobs=swap(n - 2, out_off=jobs[n - 2][5] + 2))
    refused(G.ERR_INVALID, "out misaligned", dst_shift=2)
    refused(G.ERR_INVALID, "out_stride misaligned",
            jobs=swap(5, out_stride=jobs[5][6] + 2))
    refused(G.ERR_INVALID, "out_stride below seg_len",
            jobs=swap(whole, out_stride=G.round4(jobs[whole][4]) - 4))
    refused(G.ERR_INVALID, "img_stride below the image size",
            jobs=swap(n - 1, img_stride=A.enc_size(jobs[n - 1][2]) - 1))
    refused(G.ERR_INVALID, "segment past the shard",
            jobs=swap(whole, seg_off=4))
    refused(G.ERR_NO_DATA, "zero shard_len in the last job",
            jobs=swap(n - 1, slen=0))
    refused(G.ERR_NO_DATA, "zero seg_len", jobs=swap(2, seg_len=0))
    # slow and identity paths refuse before their first job runs, too
    for name in G.SLOW_QUEUES:
        qs = G.build(name)
        es = A.encoder(qs.t)
        ss, ds = G.load(qs, dev, seed=78)
        js = list(qs.jobs)
        refused(G.ERR_NO_DATA, name + ": zero seg_len in the last job",
                enc=es, src=ss, dst=ds, q=qs,
                jobs=js[:-1] + [js[-1][:4] + (0,) + js[-1][5:]])
        refused(G.ERR_UNSUPPORTED, name + ": block_len 4096", enc=es, src=ss,
                dst=ds, q=qs, block_len=4096)
        rc, w = G.call(es, ss, ds, qs)
        A.ok(rc, name + " after the refusals")
        G.check(qs, ss, ds, w, what="after the refusals " + name)
    # and the same arenas still serve a good call afterwards
    rc, w = G.call(enc, src, dst, q)
    A.ok(rc, "after the refusals")
    G.check(q, src, dst, w, what="after the refusals rs44")
