"""gfrs_reconstruct_verify_queue on the GPU: per-job erasure patterns and
shard lengths in one call (include/gfrs.h, queue contract).

Every queue comes from tests/_repairq.py and every expectation from the
oracle's Reconstruct + Verify of the single job (_verdict.expected);
tests/test_queue_cpu.py checks on the CPU that each queue holds failing and
clean jobs and nothing undecodable.  Each run compares the whole guarded
arena: the bad shards equal the oracle's reconstruction and no other byte
- survivors, the odd gaps between jobs, the guards - has changed.
"""
import pytest

torch = pytest.importorskip("torch")

import _arena as A  # noqa: E402
import _repairq as Q  # noqa: E402
from _arena import L, vp  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def test_mixed_queue_rs63(dev):
    """54 jobs, nine lengths from 1 to 8209, six patterns of 3..6 plan rows
    interleaved so that ordering by pattern permutes the jobs; a flipped bit
    in a survivor of every third job."""
    _, got = Q.run(dev, "rs63_mixed")
    assert got and got != list(range(0, 54, 3))   # [0,2,4] detects nothing


def test_uniform_queue_equals_batch(dev):
    """The same bytes through the queue and through
    gfrs_reconstruct_verify_batch: same arena, same bitmap."""
    q = Q.build("rs63_uniform")
    a, got = Q.run(dev, "rs63_uniform")
    after_queue = a.dev.cpu().numpy().copy()
    enc = A.encoder(q.t)
    b = Q.load(q, dev)
    slen, bad = q.jobs[0][1], q.patterns[0]
    stride = q.jobs[1][0] - q.jobs[0][0]
    assert all(job == (j * stride, slen, 0) for j, job in enumerate(q.jobs))
    bm = A.bitmap(len(q.jobs))
    A.ok(L().gfrs_reconstruct_verify_batch(enc._ctx, vp(b.ptr), slen, stride,
                                           len(q.jobs), A.i32s(bad),
                                           len(bad), bm), "batch")
    A.sync(enc)
    assert A.bits(bm, len(q.jobs)) == got
    b.check(after_queue, what="uniform queue vs batch")


@pytest.mark.parametrize("name", ["rs66_depth", "rs124_k12", "rs134_w17"])
def test_row_depth_and_width(dev, name):
    """RS(6+6) with 3..6 bad: up to 12 rows = three steps; RS(12+4): k = 12
    tables (two input batches); RS(13+4): 17 shards."""
    Q.run(dev, name)


def test_lrc_single_pass(dev):
    """LRC12P2L2 through the composed single-pass plans; the flips sit in
    surviving local parities, which only the local check rows can see."""
    _, got = Q.run(dev, "lrc_single")
    assert got


def test_lrc_slow_patterns(dev):
    """EC6P3L3 has no single-pass plan (m + l = 6): every job runs as
    reconstruct + verify behind the queue launches, local-stripe patterns of
    the verdict sweeps included; bits still follow the caller's order."""
    _, got = Q.run(dev, "lrc_slow")
    assert got


def test_python_surface(dev):
    q = Q.build("rs63_mixed")
    a = Q.load(q, dev, seed=71)
    enc = A.encoder(q.t)
    fails = enc.reconstruct_verify_queue(
        a.dev, [(a.off + off, slen, pat) for off, slen, pat in q.jobs],
        q.patterns)
    want, wfails, unspec = Q.wanted(q, a)
    assert [j for j, f in enumerate(fails) if f] == wfails
    a.check(want, unspec, what="Encoder.reconstruct_verify_queue")


@pytest.mark.parametrize("grid", ["1", "3"])
def test_forced_grid_stride_and_restage(dev, monkeypatch, grid):
    """GFRS_RS_GRID is read on every launch (as tests/test_gpu_gridstride.py
    relies on): with 1 block, one block walks every tile of a bucket and
    restages its tables at each pattern change; with 3, the contiguous
    ranges split inside jobs and patterns."""
    monkeypatch.setenv("GFRS_RS_GRID", grid)
    Q.run(dev, "rs63_mixed", what="grid=%s" % grid)
    Q.run(dev, "rs66_depth", what="grid=%s" % grid)


def test_errors_write_nothing(dev):
    q = Q.build("rs63_mixed")
    enc = A.encoder(q.t)
    a = Q.load(q, dev, seed=72)
    jobs = list(q.jobs)

    def refused(code, jobs=jobs, patterns=q.patterns, what=""):
        rc, _ = Q.call(enc, a, q, jobs, patterns)
        assert rc == code, (what, rc)
        a.check(a.expect(), what="refused: " + what)

    refused(Q.ERR_INVALID, patterns=q.patterns + [[9]],
            what="shard index out of range in an unused pattern")
    refused(Q.ERR_INVALID, patterns=[[-1]] + q.patterns[1:],
            what="negative shard index")
    refused(Q.ERR_TOO_FEW, patterns=q.patterns + [[0, 1, 2, 3]],
            what="m + 1 bad shards")
    refused(Q.ERR_INVALID, jobs=jobs[:5] + [(jobs[5][0], jobs[5][1], 6)] +
            jobs[6:], what="pattern out of range")
    refused(Q.ERR_INVALID, jobs=jobs[:5] + [(jobs[5][0], jobs[5][1], -1)],
            what="negative pattern")
    refused(Q.ERR_NO_DATA, jobs=jobs[:-1] + [(jobs[-1][0], 0, 0)],
            what="zero shard_len in the last job")
    bad, boff = q.bad_lists()
    qj = q.qjobs()
    qj[7].reserved = 1
    bm = A.bitmap(len(jobs))
    args = (bad, boff, len(q.patterns), bm)
    assert L().gfrs_reconstruct_verify_queue(enc._ctx, vp(a.ptr), qj,
                                             len(jobs), *args) == Q.ERR_INVALID
    qj = q.qjobs()
    assert L().gfrs_reconstruct_verify_queue(enc._ctx, vp(a.ptr), qj, 0,
                                             *args) == Q.ERR_INVALID
    assert L().gfrs_reconstruct_verify_queue(enc._ctx, vp(a.ptr), qj,
                                             len(jobs), bad, boff, 0,
                                             bm) == Q.ERR_INVALID
    a.check(a.expect(), what="refused: reserved / njobs / npat")
    # LRC: three global losses are undecodable for the full-width call
    lq = Q.build("lrc_single")
    la = Q.load(lq, dev, seed=73)
    rc, _ = Q.call(A.encoder(lq.t), la, lq, lq.jobs,
                   lq.patterns + [[0, 1, 2]])
    assert rc == Q.ERR_TOO_FEW
    la.check(la.expect(), what="refused: LRC12P2L2 [0,1,2]")
    # and the arena still serves a good call afterwards
    rc, got = Q.call(enc, a, q)
    A.ok(rc, "after the refusals")
    want, fails, unspec = Q.wanted(q, a)
    assert got == fails
    a.check(want, unspec, what="after the refusals")
