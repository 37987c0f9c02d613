"""gfrs_put_queue on the GPU: per-job shard lengths, image places, bids and
vuid sets in one call, for narrow and wide tactics (include/gfrs.h, put-queue
contract).

Every queue comes from tests/_putq.py and every image and crc from the oracle
alone (rs_encode / lrc_encode, then shard_write and crc32 per shard);
tests/test_put_queue_cpu.py checks on the CPU that those expectations are
self-consistent.  Each run compares both guarded arenas in full: in disk_dst
the n+m+l images of every job equal the oracle's and no other byte - padding
between images, guards - has changed; base, which holds the data shards only,
is byte-for-byte unchanged for every tactic.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _arena as A  # noqa: E402
import _encq as E  # noqa: E402
import _putq as P  # noqa: E402
import _sequence as Q  # noqa: E402
import _shardq as S  # noqa: E402
from _arena import L, vp  # noqa: E402

from cubefs_amd import codemode  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", P.GPU_QUEUES)
def test_queue(dev, name):
    """rs63: the encode queue's kernels on the shifted items.  The others:
    the put frame kernel, one launch per bucket and row group - rows 4+2,
    4+4+4 with odd k, k = 16 / 24 / 32, the composed LRC rows, 22 rows in six
    groups."""
    P.run(dev, name)


@pytest.mark.parametrize("grid", ["1", "3"])
@pytest.mark.parametrize("name", ["rs66", "rs1512"])
def test_forced_walk_and_prefetch(dev, monkeypatch, name, grid):
    """GFRS_CRC_GRID is read on every launch: with 1 block, one block walks
    every frame of a bucket and crosses every job boundary with its prefetch;
    with 3, a block takes every third frame, so its prefetch skips over whole
    jobs.  Group 0 (DATA) and the later groups walk alike."""
    monkeypatch.setenv("GFRS_CRC_GRID", grid)
    P.run(dev, name, what="grid=%s" % grid)


@pytest.mark.parametrize("name", P.GPU_QUEUES)
def test_one_job_reads_back(dev, name):
    """One job alone; its images then go through gfrs_shard_read_queue with
    FOOTER: status 0, the ids, and the crc the put call returned."""
    q = P.build(name)
    enc = A.encoder(q.t)
    j = max(range(len(q.jobs)), key=lambda i: (q.jobs[i][1] < (1 << 20),
                                               q.jobs[i][1]))
    src, dst = P.load(q, dev, seed=132)
    rc, crcs = P.call(enc, src, dst, q, jobs=[q.jobs[j]])
    A.ok(rc, "one job of " + name)
    P.check(q, src, dst, crcs, "one job of " + name, jobs=[j])
    _, slen, _, _, bid, vol = q.jobs[j]
    sjobs = [(off, slen, bid, q.vuids[vol][i], 0, slen, 0,
              S.NO_OUT | S.FOOTER)
             for i, (off, _) in enumerate(q.image_regions(j))]
    res = S.fresh_results(len(sjobs))
    A.ok(L().gfrs_shard_read_queue(enc._ctx, None, vp(dst.ptr),
                                   S.sjob_array(sjobs), len(sjobs), A.BLOCK,
                                   res), "read back")
    for i, r in enumerate(S.as_dicts(res, len(sjobs))):
        assert r == dict(status=0, crc=int(crcs[0][i]), bad_block=-1, bid=bid,
                         vuid=q.vuids[vol][i], size=slen), (name, i, r)


def test_bodies_equal_the_encode_queue(dev):
    """An EC6P3 queue: bytes 32 .. 32+body of every image are what
    gfrs_encode_frame_queue writes for the same job."""
    q = P.build("rs63")
    enc = A.encoder(q.t)
    src, dst = P.load(q, dev, seed=134)
    rc, _ = P.call(enc, src, dst, q)
    A.ok(rc, "put queue")
    disk = dst.read()[dst.off:]
    # the encode queue reads shard i at off + i*slen, i < n only
    body = A.Arena(dev, q.img_bytes, 4, seed=135)
    body.upload()
    ejobs = [(off, slen, img_off, stride)
             for off, slen, img_off, stride, _, _ in q.jobs]
    A.ok(L().gfrs_encode_frame_queue(enc._ctx, vp(body.ptr), vp(src.ptr),
                                     E.ejob_array(ejobs), len(ejobs),
                                     A.BLOCK), "encode queue")
    framed = body.read()[body.off:]
    for j, (off, slen, img_off, stride, _, _) in enumerate(q.jobs):
        n = A.enc_size(slen)
        for i in range(q.total):
            at = img_off + i * stride
            assert np.array_equal(disk[at + 32:at + 32 + n],
                                  framed[at:at + n]), (j, i)
    src.check(src.expect(), what="base after both calls")


@pytest.mark.parametrize("name", ["rs63", "rs66"])
def test_null_crcs_writes_the_same_images(dev, name):
    q = P.build(name)
    enc = A.encoder(q.t)
    src, dst = P.load(q, dev, seed=136)
    rc, crcs = P.call(enc, src, dst, q, want_crcs=False)
    A.ok(rc, "crcs == NULL")
    assert crcs is None
    P.check(q, src, dst, None, "crcs == NULL " + name)


def test_behind_async_write_twice_and_growing(dev):
    """On one fresh context, nothing between the calls and every arena
    compared only after all were issued: an async gfrs_shard_write_batch whose
    id upload is still queued when the queue stages its blob (the window
    before the queue is asserted), the same queue twice, then a larger queue
    that grows the scratch."""
    t = codemode.get_tactic("EC6P6")
    r = Q.Runner(dev, t)
    writer = A.ShardWriteBatch(70001, 4, pad=3, delta=1, extra=8,
                               what="producer")
    first = A.QueueCall("_putq", "seq_tiny", what="first")
    again = A.QueueCall("_putq", "seq_tiny", what="again")
    bigger = A.QueueCall("_putq", "seq_more", what="bigger")
    r.run([writer, first, again, bigger], cold=[bigger],
          what="write_batch -> put queue x2 -> larger put queue")


def test_python_surface(dev):
    for name in ("rs63", "lrc442"):
        q = P.build(name)
        src, dst = P.load(q, dev, seed=138)
        enc = A.encoder(q.t)
        crcs = enc.put_queue(
            dst.dev, src.dev,
            [(src.off + off, slen, dst.off + img_off, stride, bid, vol)
             for off, slen, img_off, stride, bid, vol in q.jobs], q.vuids)
        assert crcs.shape == (len(q.jobs), q.total)
        P.check(q, src, dst, crcs, what="Encoder.put_queue " + name)


def test_errors_write_nothing(dev):
    q63, q66 = P.build("rs63"), P.build("rs66")
    for q in (q63, q66):
        enc = A.encoder(q.t)
        src, dst = P.load(q, dev, seed=140)
        jobs = list(q.jobs)
        n = len(jobs)

        def refused(code, what, enc=enc, src=src, dst=dst, q=q, **kw):
            rc, crcs = P.call(enc, src, dst, q, **kw)
            what = "%s: %s" % (q.name, what)
            assert rc == code, (what, rc)
            assert (crcs == P.FILL).all(), what
            src.check(src.expect(), what="refused (base): " + what)
            dst.check(dst.expect(), what="refused (images): " + what)

        def swap(j, **f):
            off, slen, img_off, stride, bid, vol = jobs[j]
            new = dict(off=off, slen=slen, img_off=img_off, stride=stride,
                       bid=bid, vol=vol, reserved=0)
            new.update(f)
            return jobs[:j] + [(new["off"], new["slen"], new["img_off"],
                                new["stride"], new["bid"], new["vol"],
                                new["reserved"])] + jobs[j + 1:]

        refused(P.ERR_BLOCK, "block_len 0", block_len=0)
        refused(P.ERR_BLOCK, "block_len -65536", block_len=-65536)
        refused(P.ERR_BLOCK, "block_len 65540", block_len=65540)
        refused(P.ERR_UNSUPPORTED, "block_len 4096", block_len=4096)
        refused(P.ERR_UNSUPPORTED, "block_len 131072", block_len=131072)
        refused(P.ERR_INVALID, "njobs = 0", njobs=0)
        refused(P.ERR_INVALID, "njobs = -1", njobs=-1)
        refused(P.ERR_INVALID, "nvol = 0", nvol=0)
        refused(P.ERR_INVALID, "vol out of range in the last job",
                jobs=swap(n - 1, vol=P.NVOL))
        refused(P.ERR_INVALID, "vol < 0", jobs=swap(3, vol=-1))
        refused(P.ERR_INVALID, "reserved != 0", jobs=swap(7, reserved=1))
        refused(P.ERR_NO_DATA, "zero shard_len in the last job",
                jobs=swap(n - 1, slen=0))
        refused(P.ERR_INVALID, "shard_len 2^32",
                jobs=swap(n - 1, slen=1 << 32, stride=1 << 33))
        refused(P.ERR_INVALID, "img_off misaligned",
                jobs=swap(9, img_off=jobs[9][2] + 2))
        refused(P.ERR_INVALID, "disk_dst misaligned", dst_shift=2)
        refused(P.ERR_INVALID, "img_stride misaligned",
                jobs=swap(8, stride=jobs[8][3] + 2))
        refused(P.ERR_INVALID, "img_stride below the disk size",
                jobs=swap(n - 2,
                          stride=E.round4(A.disk_size(jobs[n - 2][1])) - 4))
        # the tactic's width: n = 33 and a replicate tactic, on the same
        # arenas (nothing of them is read before the refusal)
        for t in (P.rs334_tactic(), codemode.get_tactic("Replica3")):
            refused(P.ERR_UNSUPPORTED, "tactic %d+%d" % (t.N, t.M),
                    enc=A.encoder(t))
        # and the same arenas still serve a good call afterwards
        rc, crcs = P.call(enc, src, dst, q)
        A.ok(rc, "after the refusals")
        P.check(q, src, dst, crcs, what="after the refusals " + q.name)
