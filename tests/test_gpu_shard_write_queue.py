"""GPU checks of gfrs_shard_write_queue (include/gfrs.h, shard-write-queue
contract) on the queues of tests/_shardwq.py, whose expectations come from the
oracle alone (tests/test_shard_write_queue_cpu.py checks them without a
device).

Every run compares the whole dst arena (guards between and around the new
images), the whole src arena and every field of every result.
"""
import numpy as np
import pytest
import torch

import _arena as A
import _sequence as Q
import _shardq as S
import _shardwq as W
from _arena import L, Arena, oracle, vp

from cubefs_amd import codemode, shard

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def enc():
    return A.encoder(A.tactic(4, 2))


@pytest.mark.parametrize("name", W.CLEAN_QUEUES)
def test_clean_queues(dev, name):
    """Every size as a raw and as a SRC_IMAGE job, interleaved; all raw; all
    SRC_IMAGE; one job; four frames per bucket.  Status 0 everywhere, every
    image the oracle's, crc the payload's."""
    W.run(dev, name)


def test_one_flip_per_job(dev):
    """One flipped site per source image: stored frame CRCs, payload at
    vector, piece, pass and frame edges, two bad frames, every header field,
    wrong ids on intact images, the footer, the garbage behind the image.
    Exact bits, bad_block and crc; the new image is the oracle's write of the
    payload as stored, with fresh frame CRCs and the new ids."""
    W.run(dev, "flips")


@pytest.mark.parametrize("grid", ["1", "3"])
def test_forced_grids(dev, monkeypatch, grid):
    """GFRS_CRC_GRID is read on every launch: with 1 block, one block walks
    every frame of a bucket across every job; with 3, a block starts in the
    middle of a bucket, and on `tiny` (4 frames per bucket, 2 per block) the
    third block has no frame at all."""
    monkeypatch.setenv("GFRS_CRC_GRID", grid)
    for name in ("tiny", "clean"):
        W.run(dev, name, what="grid=%s" % grid)


@pytest.mark.parametrize("waves", ["4", "8"])
def test_both_wave_builds(dev, monkeypatch, waves):
    """GFRS_SWR_WAVES is read on every launch: both builds of both kernels."""
    monkeypatch.setenv("GFRS_SWR_WAVES", waves)
    W.run(dev, "clean", what="waves=%s" % waves)
    W.run(dev, "flips", what="waves=%s" % waves)


def test_errors_write_nothing(dev):
    q = W.build("clean")
    e = enc()
    src, dst = W.load(q, dev, seed=113)
    names = ["src_off", "size", "bid", "vuid", "src_bid", "src_vuid",
             "img_off", "flags", "reserved"]
    last = len(q.jobs) - 1

    def swap(**f):
        v = dict(zip(names, q.jobs[last] + (0,)))
        v.update(f)
        return q.jobs[:last] + [tuple(v[n] for n in names)]

    img_off = q.jobs[last][6]
    cases = [(dict(block_len=0), W.ERR_BLOCK),
             (dict(block_len=-65536), W.ERR_BLOCK),
             (dict(block_len=65540), W.ERR_BLOCK),
             (dict(block_len=4096), W.ERR_UNSUPPORTED),
             (dict(block_len=131072), W.ERR_UNSUPPORTED),
             (dict(jobs=swap(size=0)), W.ERR_NO_DATA),
             (dict(njobs=0), W.ERR_INVALID),
             (dict(njobs=-3), W.ERR_INVALID),
             (dict(jobs=swap(size=1 << 32)), W.ERR_INVALID),
             (dict(jobs=swap(reserved=1)), W.ERR_INVALID),
             (dict(jobs=swap(flags=2)), W.ERR_INVALID),
             (dict(jobs=swap(flags=0x80000001)), W.ERR_INVALID),
             (dict(jobs=swap(img_off=img_off + 2)), W.ERR_INVALID),
             (dict(jobs=swap(img_off=img_off + 1)), W.ERR_INVALID),
             (dict(dst_shift=2), W.ERR_INVALID)]
    for kw, want in cases:
        rc, got = W.call(e, src, dst, q, **kw)
        assert rc == want, (kw.keys(), rc, want)
        assert all(g["status"] == W.DEAD and g["crc"] == W.DEAD and
                   g["bid"] == W.DEAD and g["bad_block"] == -W.DEAD
                   for g in got), kw.keys()
        dst.check(dst.expect(), what="error %d dst" % want)
        src.check(src.expect(), what="error %d src" % want)
    # and the queue still runs afterwards
    rc, got = W.call(e, src, dst, q)
    A.ok(rc, "after errors")
    W.check(q, src, dst, got, "after errors")


def test_raw_job_equals_write_batch(dev):
    """A raw job alone writes the bytes of gfrs_shard_write_batch with
    nshards = 1 on the same source bytes and ids."""
    q = W.build("clean")
    e = enc()
    src, _ = W.load(q, dev, seed=114)
    picked = [j for j, job in enumerate(q.jobs) if not job[7]]
    assert len(picked) == len(W.LENS)
    for j in picked:
        src_off, size, bid, vuid = q.jobs[j][:4]
        disk = A.disk_size(size)
        one = Arena(dev, disk, 4, seed=115)
        two = Arena(dev, disk, 4, seed=115)     # the same garbage
        one.upload()
        two.upload()
        rc, got = W.call(e, src, one, q,
                         jobs=[(src_off, size, bid, vuid, 0, 0, 0, 0)])
        A.ok(rc, "single raw job %d" % j)
        A.ok(L().gfrs_shard_write_batch(
            e._ctx, vp(two.ptr), disk, vp(src.ptr + src_off), size, size,
            A.BLOCK, A.u64s([bid]), A.u64s([vuid]), 1), "write_batch")
        A.sync(e)
        assert np.array_equal(one.read(), two.read()), j
        assert got[0] == W.expected("clean")[j], j
    src.check(src.expect(), what="raw equivalence src")


@pytest.mark.parametrize("name", ["clean", "flips"])
def test_image_job_equals_read_queue_job(dev, name):
    """A SRC_IMAGE job's result is that of the gfrs_shard_read_queue job the
    contract names - whole shard, FOOTER, the source's ids - on the same
    image, and the payload that job stores is the payload of the new image."""
    q = W.build(name)
    e = enc()
    src, dst = W.load(q, dev, seed=116)
    rc, got = W.call(e, src, dst, q)
    A.ok(rc, "write queue")
    picked = [j for j, job in enumerate(q.jobs) if job[7] & W.SRC_IMAGE]
    rjobs, at = [], 0
    for j in picked:
        r = W.read_job(q.jobs[j])
        rjobs.append(r[:6] + (at, r[7]))
        at = (at + r[1] + 3) // 4 * 4 + 4
    out = Arena(dev, at, 4, seed=117)
    out.upload()
    res = S.fresh_results(len(rjobs))
    A.ok(L().gfrs_shard_read_queue(e._ctx, vp(out.ptr), vp(src.ptr),
                                   S.sjob_array(rjobs), len(rjobs), A.BLOCK,
                                   res), "read queue")
    rgot = S.as_dicts(res, len(rjobs))
    nzero = 0
    for j, r, rj in zip(picked, rgot, rjobs):
        assert got[j] == r, (name, j, got[j], r)
        nzero += r["status"] == 0
    assert nzero == len(picked) if name == "clean" else 0 < nzero < len(picked)
    # the bytes the reader stripped are the bytes the new images carry
    new = dst.read()
    stripped = out.read()
    for j, rj in zip(picked, rjobs):
        size, img_off = q.jobs[j][1], q.jobs[j][6]
        img = new[dst.off + img_off:dst.off + img_off + A.disk_size(size)]
        assert np.array_equal(
            S.payload_of(img, size),
            stripped[out.off + rj[6]:out.off + rj[6] + size]), (name, j)
    W.check(q, src, dst, got, "equivalence " + name)


@pytest.mark.parametrize("name", ["clean", "flips"])
def test_round_trip_through_read_queue(dev, name):
    """The written images, fed to gfrs_shard_read_queue as whole-shard FOOTER
    jobs with the new ids: status 0, the payload bytes, the same crc - also
    for the images made from corrupted sources (always self-consistent)."""
    q = W.build(name)
    e = enc()
    src, dst = W.load(q, dev, seed=118)
    rc, got = W.call(e, src, dst, q)
    A.ok(rc, "write queue")
    rjobs, at = [], 0
    for job in q.jobs:
        _, size, bid, vuid, _, _, img_off, _ = job
        rjobs.append((img_off, size, bid, vuid, 0, size, at, S.FOOTER))
        at = (at + size + 3) // 4 * 4 + 4
    out = Arena(dev, at, 4, seed=119)
    out.upload()
    res = S.fresh_results(len(rjobs))
    A.ok(L().gfrs_shard_read_queue(e._ctx, vp(out.ptr), vp(dst.ptr),
                                   S.sjob_array(rjobs), len(rjobs), A.BLOCK,
                                   res), "read back")
    want = out.expect()
    for j, (r, rj) in enumerate(zip(S.as_dicts(res, len(rjobs)), rjobs)):
        pay = q.payload(j)
        assert r == dict(status=0, crc=oracle.crc32(pay.copy()), bad_block=-1,
                         bid=rj[2], vuid=rj[3], size=rj[1]), (name, j, r)
        assert r["crc"] == got[j]["crc"], (name, j)
        out.put(rj[6], pay, want)
    out.check(want, what="round trip out")
    W.check(q, src, dst, got, "round trip " + name)


def test_behind_async_write_twice_and_growing(dev):
    """On one fresh context, nothing between the calls and every arena
    compared only after all were issued: an async gfrs_shard_write_batch whose
    id upload is still queued when the queue stages its blob (the window
    before the queue is asserted), the same queue twice, then a larger queue
    that grows the scratch."""
    t = codemode.get_tactic("EC6P3")
    r = Q.Runner(dev, t)
    writer = A.ShardWriteBatch(70001, 4, pad=3, delta=1, extra=8,
                               what="producer")
    first = A.QueueCall("_shardwq", "tiny", what="first")
    again = A.QueueCall("_shardwq", "tiny", what="again")
    bigger = A.QueueCall("_shardwq", "clean", what="bigger")
    r.run([writer, first, again, bigger], cold=[bigger],
          what="write_batch -> write queue x2 -> larger write queue")


def test_python_surface(dev):
    for k, name in enumerate(["clean", "flips"]):
        q = W.build(name)
        src, dst = W.load(q, dev, seed=120 + 2 * k)
        codec = shard.ShardCodec()
        got = codec.write_queue(dst.dev[dst.off:], src.dev[src.off:], q.jobs)
        W.check(q, src, dst, got, "python surface " + name)
    with pytest.raises(shard.GfrsError):
        codec.write_queue(dst.dev[dst.off + 2:], src.dev[src.off:], q.jobs)
    with pytest.raises(shard.GfrsError):
        codec.write_queue(dst.dev[dst.off:], src.dev[src.off:], [])
