"""GPU checks of gfrs_shard_read_queue (include/gfrs.h, shard-read-queue
contract) on the queues of tests/_shardq.py, whose expectations come from the
oracle alone (tests/test_shard_read_queue_cpu.py checks them without a
device).

Every run compares the whole out arena (guards between and around the rows),
the whole chunk arena and every field of every result.
"""
import ctypes

import numpy as np
import pytest
import torch

import _arena as A
import _repairimgq as R
import _shardq as S
from _arena import L, Arena, oracle, vp

from cubefs_amd import shard

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def enc():
    return A.encoder(A.tactic(4, 2))


@pytest.mark.parametrize("name", S.CLEAN_QUEUES)
def test_clean_queues(dev, name):
    """Every size and range, with and without NO_OUT, whole shards also with
    FOOTER; one job; all NO_OUT; none NO_OUT.  Status 0 everywhere."""
    S.run(dev, name)


def test_one_flip_per_job(dev):
    """One flipped site per job: stored frame CRCs, payload at vector, piece,
    pass and frame edges, frames outside the range, the garbage between
    images, every header field, wrong ids on intact images, the footer with
    and without FOOTER.  Exact bits, bad_block and crc; storing jobs still
    receive the image's payload bytes."""
    S.run(dev, "flips")


@pytest.mark.parametrize("grid", ["1", "3"])
def test_forced_grids(dev, monkeypatch, grid):
    """GFRS_CRC_GRID is read on every launch: with 1 block, one block walks
    every frame of a bucket across every job; with 3, a block starts in the
    middle of a bucket, and on `tiny` (4 frames per bucket, 2 per block) the
    third block has no frame at all."""
    monkeypatch.setenv("GFRS_CRC_GRID", grid)
    for name in ("clean", "flips", "tiny"):
        S.run(dev, name, what="grid=%s" % grid)


@pytest.mark.parametrize("waves", ["4", "8"])
def test_both_wave_builds(dev, monkeypatch, waves):
    """GFRS_SRD_WAVES is read on every launch: both builds of both kernels."""
    monkeypatch.setenv("GFRS_SRD_WAVES", waves)
    S.run(dev, "clean", what="waves=%s" % waves)
    S.run(dev, "flips", what="waves=%s" % waves)


def test_null_out_for_inspection(dev):
    q = S.build("all_no_out")
    src, dst = S.load(q, dev, seed=92)
    rc, got = S.call(enc(), src, dst, q, null_out=True)
    A.ok(rc, "null out")
    S.check(q, src, dst, got, "null out")


def test_errors_write_nothing(dev):
    q = S.build("none_no_out")
    e = enc()
    src, dst = S.load(q, dev, seed=93)
    names = ["img_off", "size", "bid", "vuid", "frm", "to", "out_off",
             "flags", "reserved"]
    last = len(q.jobs) - 1

    def swap(**f):
        v = dict(zip(names, q.jobs[last] + (0,)))
        v.update(f)
        return q.jobs[:last] + [tuple(v[n] for n in names)]

    size = q.jobs[last][1]
    cases = [(dict(block_len=0), S.ERR_BLOCK),
             (dict(block_len=-65536), S.ERR_BLOCK),
             (dict(block_len=65540), S.ERR_BLOCK),
             (dict(block_len=4096), S.ERR_UNSUPPORTED),
             (dict(block_len=131072), S.ERR_UNSUPPORTED),
             (dict(jobs=swap(size=0)), S.ERR_NO_DATA),
             (dict(njobs=0), S.ERR_INVALID),
             (dict(njobs=-3), S.ERR_INVALID),
             (dict(jobs=swap(size=1 << 32, to=1 << 32)), S.ERR_INVALID),
             (dict(jobs=swap(reserved=1)), S.ERR_INVALID),
             (dict(jobs=swap(flags=4)), S.ERR_INVALID),
             (dict(jobs=swap(frm=size, to=size)), S.ERR_INVALID),
             (dict(jobs=swap(frm=0, to=size + 1)), S.ERR_INVALID),
             (dict(jobs=swap(frm=2, to=size)), S.ERR_INVALID),
             (dict(jobs=swap(frm=4, to=size, flags=S.FOOTER)), S.ERR_INVALID),
             (dict(jobs=swap(frm=0, to=size - 1, flags=S.FOOTER)),
              S.ERR_INVALID),
             (dict(jobs=swap(out_off=2)), S.ERR_INVALID),
             (dict(dst_shift=2), S.ERR_INVALID),
             (dict(null_out=True), S.ERR_INVALID)]
    for kw, want in cases:
        rc, got = S.call(e, src, dst, q, **kw)
        assert rc == want, (kw.keys(), rc, want)
        assert all(g["status"] == S.DEAD and g["bid"] == S.DEAD and
                   g["bad_block"] == -S.DEAD for g in got), kw.keys()
        dst.check(dst.expect(), what="error %d out" % want)
        src.check(src.expect(), what="error %d chunk" % want)
    # and the queue still runs afterwards
    rc, got = S.call(e, src, dst, q)
    A.ok(rc, "after errors")
    S.check(q, src, dst, got, "after errors")


def _whole_footer_jobs(q):
    return [j for j, job in enumerate(q.jobs)
            if job[7] == S.FOOTER and (job[4], job[5]) == (0, job[1])]


@pytest.mark.parametrize("name", ["clean", "flips"])
def test_equals_parse_batch_and_decode_per_job(dev, name):
    """Per single job: status == 0 exactly when gfrs_shard_parse_batch on the
    image alone reports err == 0 and the job's ids; bad_block is that call's;
    the bytes are gfrs_crc32b_decode's of the body."""
    q = S.build(name)
    e = enc()
    src, dst = S.load(q, dev, seed=94)
    picked = _whole_footer_jobs(q)
    assert len(picked) >= 10
    nzero = 0
    for j in picked:
        job = q.jobs[j]
        off, size, bid, vuid = job[:4]
        one = job[:6] + (0, S.FOOTER)
        out = Arena(dev, size, 0, seed=95)
        out.upload()
        rc, got = S.call(e, src, out, q, jobs=[one])
        A.ok(rc, "single job %d" % j)
        meta = (ctypes.c_uint64 * 4)()
        badb = (ctypes.c_int64 * 1)()
        A.ok(L().gfrs_shard_parse_batch(e._ctx, vp(src.ptr + off), 0, size,
                                        A.BLOCK, meta, badb, 1), "parse")
        err = ctypes.c_int64(meta[3]).value
        accepted = err == 0 and (meta[0], meta[1], meta[2]) == \
            (bid, vuid, size)
        assert (got[0]["status"] == 0) == accepted, (j, got[0], err)
        assert got[0]["bad_block"] == badb[0], (j, got[0], badb[0])
        assert (got[0]["bid"], got[0]["vuid"], got[0]["size"]) == \
            (meta[0], meta[1], meta[2])
        nzero += got[0]["status"] == 0
        dec = Arena(dev, size, 0, seed=95)
        dec.upload()
        n = L().gfrs_crc32b_decode(e._ctx, vp(dec.ptr),
                                   vp(src.ptr + off + 32), A.enc_size(size),
                                   A.BLOCK)
        A.sync(e)
        if got[0]["bad_block"] < 0:
            assert n == size, (j, n)
            assert np.array_equal(out.read(), dec.read()), j
        else:
            assert n == -9, (j, n)
    want = S.expected(name)
    assert nzero == sum(1 for j in picked if want[j]["status"] == 0)
    assert nzero == len(picked) if name == "clean" else nzero < len(picked)
    src.check(src.expect(), what="equivalence chunk")


def _prepare_read(placed, dev):
    """placed: [(offset, raw, bid, vuid)]; whole-shard FOOTER jobs, every
    third one NO_OUT.  Everything that touches the device happens here."""
    jobs, at, rows = [], 0, []
    for k, (off, raw, bid, vuid) in enumerate(placed):
        flags = S.FOOTER | (S.NO_OUT if k % 3 == 2 else 0)
        jobs.append((off, raw.size, bid, vuid, 0, raw.size, at, flags))
        if not flags & S.NO_OUT:
            rows.append((at, raw))
            at = (at + raw.size + 3) // 4 * 4 + 4
    out = Arena(dev, max(4, at), 4, seed=96)
    out.upload()
    return placed, jobs, rows, out, S.fresh_results(len(jobs))


def _read_back(e, chunk_ptr, prepared, what):
    """The call alone, then: clean and byte-exact."""
    placed, jobs, rows, out, res = prepared
    rc = L().gfrs_shard_read_queue(e._ctx, vp(out.ptr), vp(chunk_ptr),
                                   S.sjob_array(jobs), len(jobs), A.BLOCK,
                                   res)
    A.ok(rc, what)
    for k, (g, (off, raw, bid, vuid)) in enumerate(
            zip(S.as_dicts(res, len(jobs)), placed)):
        assert g == dict(status=0, crc=oracle.crc32(raw.copy()), bad_block=-1,
                         bid=bid, vuid=vuid, size=raw.size), (what, k, g)
    want = out.expect()
    for at, raw in rows:
        out.put(at, raw, want)
    out.check(want, what=what + " out")


def test_reads_back_what_write_batch_wrote(dev):
    """gfrs_shard_write_batch, then the queue directly behind it on the same
    context with no sync between: the write's id upload is still queued when
    the queue stages its blob."""
    e = enc()
    for slen, nsh in [(70001, 7), (4093, 5)]:
        w = A.ShardWriteBatch(slen, nsh, pad=3, delta=1, extra=8, ids=2,
                              what="round trip")
        w.prepare(dev)
        prepared = _prepare_read(
            [(w.rows.off(j), w.raw[j], w.bids[j], w.vuids[j])
             for j in range(nsh)], dev)
        w.issue(e)                      # async: nothing waited for
        _read_back(e, w.dst.ptr, prepared, "behind write_batch %d" % slen)
        w.check(e)                      # and the images are the oracle's


def test_reads_back_what_repair_queue_wrote(dev):
    r = R.build("seq_small")
    src, dst, fails = R.run(dev, "seq_small", what="round trip")
    exp = R.expectations("seq_small")
    placed = []
    for j in range(len(r.rjobs)):
        if j in fails:      # that queue corrupts some jobs: images unspecified
            continue
        for b, ((off, _), idx) in enumerate(zip(r.image_regions(j),
                                                r.bad_of(j))):
            placed.append((off, exp[j][0][idx], r.bids[r.ids[j] + b],
                           r.vuids[r.ids[j] + b]))
    assert len(placed) >= 4
    _read_back(A.encoder(r.t), dst.ptr, _prepare_read(placed, dev),
               "behind repair_queue")


def test_python_surface(dev):
    q = S.build("flips")
    src, dst = S.load(q, dev, seed=97)
    codec = shard.ShardCodec()
    chunk = src.dev[src.off:]
    out = dst.dev[dst.off:]
    got = codec.read_queue(out, chunk, q.jobs)
    S.check(q, src, dst, got, "python surface")
    q2 = S.build("all_no_out")
    src2, dst2 = S.load(q2, dev, seed=98)
    got2 = codec.read_queue(None, src2.dev[src2.off:], q2.jobs)
    S.check(q2, src2, dst2, got2, "python surface, no out")
    with pytest.raises(shard.GfrsError):
        codec.read_queue(None, chunk, q.jobs)
