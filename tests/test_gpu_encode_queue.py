"""gfrs_encode_frame_queue on the GPU: per-job shard lengths and image places
in one call (include/gfrs.h, encode-queue contract).

Every queue comes from tests/_encq.py and every image from the oracle alone
(rs_encode / lrc_encode, then crc32b_encode per shard);
tests/test_encode_queue_cpu.py checks on the CPU that those expectations are
self-consistent.  Each run compares both guarded arenas in full: in framed
the n+m+l images of every job equal the oracle's and no other byte - padding
between images, guards - has changed; base is byte-for-byte unchanged for the
fused tactics, and for a slow tactic nothing but the parity shards, which then
hold the oracle's parity.
"""
import pytest

torch = pytest.importorskip("torch")

import _arena as A  # noqa: E402
import _encq as E  # noqa: E402
from _arena import L, Arena, vp  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def test_mixed_queue_rs63(dev):
    """Every length from 1 byte to 1 MiB and a byte in one call: all four
    wave buckets and both frame buckets, six launches."""
    E.run(dev, "rs63_mixed")


def test_small_queue_rs63(dev):
    """The PUT path's common case: 91 jobs of at most 4 KiB, one wave each."""
    E.run(dev, "rs63_small")


@pytest.mark.parametrize("name", ["rs42", "rs124_k12"])
def test_other_row_counts(dev, name):
    """RS(4+2) (two rows) and RS(12+4) (four rows, k = 12 tables)."""
    E.run(dev, name)


def test_lrc_fused(dev):
    """LRC12P2L2 through the composed fused plan: the images of the local
    parities included."""
    E.run(dev, "lrc_fused")


def test_slow_tactic_rs66(dev):
    """RS(6+6) has no fused kernel: one job at a time, encode_batch then
    crc32b_encode_batch; the parity lands in base as well."""
    E.run(dev, "rs66_slow")


@pytest.mark.parametrize("grid", ["1", "3"])
def test_forced_walk_and_prefetch(dev, monkeypatch, grid):
    """GFRS_CRC_GRID is read on every launch: with 1 block, one block walks
    every frame of a bucket and crosses every job boundary with its prefetch,
    and four waves share all the small jobs; with 3, a block takes every
    third frame, so its prefetch skips over whole jobs."""
    monkeypatch.setenv("GFRS_CRC_GRID", grid)
    E.run(dev, "rs63_mixed", what="grid=%s" % grid)
    E.run(dev, "rs63_small", what="grid=%s" % grid)


def test_jobs_equal_single_stripe_batch_calls(dev):
    """The per-job clause: a job's images are those of gfrs_encode_frame_batch
    on the same bytes, one stripe."""
    q = E.build("rs63_mixed")
    enc = A.encoder(q.t)
    src, dst = E.load(q, dev, seed=92)
    A.ok(E.call(enc, src, dst, q), "queue")
    after_queue = dst.dev.cpu().numpy().copy()
    picks = [j for j, job in enumerate(q.jobs)
             if job[1] in (17, 2049, 4096, 4097, 65533, 65596, 131065,
                           1048577)]
    assert len(picks) == 8
    src2, dst2 = E.load(q, dev, seed=92)
    want = dst2.expect()
    for j in picks:
        off, slen, img_off, stride = q.jobs[j]
        A.ok(L().gfrs_encode_frame_batch(enc._ctx, vp(dst2.ptr + img_off),
                                         stride, vp(src2.ptr + off), slen,
                                         q.total * slen, 1, A.BLOCK),
             "batch call of job %d" % j)
        for o, n in q.image_regions(j):
            want[dst2.off + o:dst2.off + o + n] = \
                after_queue[dst.off + o:dst.off + o + n]
    A.sync(enc)
    dst2.check(want, what="single-stripe batch calls vs the queue")


@pytest.mark.parametrize("slen", [4096, 4097])
def test_one_job_at_a_class_edge(dev, slen):
    """One job alone: the last wave-kernel length and the first frame-kernel
    length."""
    t = A.tactic(4, 2)
    enc = A.encoder(t)
    total = t.N + t.M
    ref = A.ref_stripes(t, 1, slen, seed=33)[0]
    src = Arena(dev, total * slen, 3, seed=94)
    for i in range(t.N):
        src.put(i * slen, ref[i])
    src.upload()
    size = A.enc_size(slen)
    stride = E.round4(size) + 8
    dst = Arena(dev, (total - 1) * stride + size, 4, seed=95)
    dst.upload()
    rc = L().gfrs_encode_frame_queue(enc._ctx, vp(dst.ptr), vp(src.ptr),
                                     E.ejob_array([(0, slen, 0, stride)]), 1,
                                     A.BLOCK)
    A.ok(rc, "one job of %d" % slen)
    want = dst.expect()
    for i in range(total):
        dst.put(i * stride, A.oracle.crc32b_encode(ref[i].copy()), want)
    dst.check(want, what="one job of %d: images" % slen)
    src.check(src.expect(), what="one job of %d: base" % slen)


def test_python_surface(dev):
    q = E.build("rs63_mixed")
    src, dst = E.load(q, dev, seed=96)
    enc = A.encoder(q.t)
    enc.encode_frame_queue(
        dst.dev, src.dev, [(src.off + off, slen, dst.off + img_off, stride)
                           for off, slen, img_off, stride in q.jobs])
    E.check(q, src, dst, what="Encoder.encode_frame_queue")


def test_errors_write_nothing(dev):
    q = E.build("rs63_mixed")
    enc = A.encoder(q.t)
    src, dst = E.load(q, dev, seed=98)
    jobs = list(q.jobs)
    n = len(jobs)

    def refused(code, what, enc=enc, src=src, dst=dst, q=q, **kw):
        rc = E.call(enc, src, dst, q, **kw)
        assert rc == code, (what, rc)
        src.check(src.expect(), what="refused (base): " + what)
        dst.check(dst.expect(), what="refused (images): " + what)

    def swap(j, **f):
        off, slen, img_off, stride = jobs[j]
        new = dict(off=off, slen=slen, img_off=img_off, stride=stride,
                   reserved=0)
        new.update(f)
        return jobs[:j] + [(new["off"], new["slen"], new["img_off"],
                            new["stride"], new["reserved"])] + jobs[j + 1:]

    refused(E.ERR_BLOCK, "block_len 0", block_len=0)
    refused(E.ERR_BLOCK, "block_len -65536", block_len=-65536)
    refused(E.ERR_BLOCK, "block_len 65540", block_len=65540)
    refused(E.ERR_UNSUPPORTED, "block_len 4096", block_len=4096)
    refused(E.ERR_UNSUPPORTED, "block_len 131072", block_len=131072)
    refused(E.ERR_INVALID, "njobs = 0", njobs=0)
    refused(E.ERR_INVALID, "njobs = -1", njobs=-1)
    refused(E.ERR_INVALID, "reserved != 0", jobs=swap(7, reserved=1))
    refused(E.ERR_NO_DATA, "zero shard_len in the last job",
            jobs=swap(n - 1, slen=0))
    refused(E.ERR_INVALID, "img_off misaligned",
            jobs=swap(9, img_off=jobs[9][2] + 2))
    refused(E.ERR_INVALID, "framed misaligned", dst_shift=2)
    refused(E.ERR_INVALID, "img_stride misaligned",
            jobs=swap(8, stride=jobs[8][3] + 2))
    refused(E.ERR_INVALID, "img_stride below the image size",
            jobs=swap(n - 2, stride=E.round4(A.enc_size(jobs[n - 2][1])) - 4))
    # a slow tactic refuses before its first job runs, too
    q66 = E.build("rs66_slow")
    s66, d66 = E.load(q66, dev, seed=99)
    e66 = A.encoder(q66.t)
    j66 = list(q66.jobs)
    refused(E.ERR_NO_DATA, "RS(6+6): zero shard_len in the last job", enc=e66,
            src=s66, dst=d66, q=q66,
            jobs=j66[:-1] + [(j66[-1][0], 0) + j66[-1][2:]])
    refused(E.ERR_UNSUPPORTED, "RS(6+6): block_len 4096", enc=e66, src=s66,
            dst=d66, q=q66, block_len=4096)
    # and the same arenas still serve a good call afterwards
    for enc_, s_, d_, q_ in [(enc, src, dst, q), (e66, s66, d66, q66)]:
        A.ok(E.call(enc_, s_, d_, q_), "after the refusals")
        E.check(q_, s_, d_, what="after the refusals " + q_.name)
