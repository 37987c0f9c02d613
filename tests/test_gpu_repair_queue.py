"""gfrs_repair_queue on the GPU: per-job erasure patterns, shard lengths and
disk images in one call (include/gfrs.h, repair-queue contract).

Every queue comes from tests/_repairimgq.py, every verdict from the oracle's
Reconstruct + Verify of the single job (_verdict.expected) and every image
from oracle.shard_write of that reconstruction; tests/test_repair_queue_cpu.py
checks on the CPU that each queue holds failing jobs only among the corrupted
ones, a clean job for every pattern and nothing undecodable.  Each run
compares both guarded arenas in full: in disk_dst the images of every passing
job equal the oracle's and no other byte - padding between images, guards -
has changed (a failed job's images are unspecified); in base nothing but the
bad shards' regions (unspecified) has changed.
"""
import pytest

torch = pytest.importorskip("torch")

import _arena as A  # noqa: E402
import _repairimgq as R  # noqa: E402
from _arena import L, vp  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def test_mixed_queue_rs63(dev):
    """36 jobs, eighteen lengths from 1 byte to two frames and a byte, six
    patterns (two of them the same erasures in another column order) through
    the fused frame kernel; a flipped bit in a survivor of every third job."""
    _, _, got = R.run(dev, "rs63_mixed")
    assert got


def test_k12_queue(dev):
    """RS(12+4): k = 12 tables, four rows."""
    R.run(dev, "rs124_k12")


def test_lrc_fused(dev):
    """LRC12P2L2 through the composed fused plans, a lost local parity
    included; the flips sit in surviving local parities, which only the
    local check rows can see."""
    _, _, got = R.run(dev, "lrc_single")
    assert got


@pytest.mark.parametrize("name", ["rs66_inplace", "rs134_w17"])
def test_inplace_identity_items(dev, name):
    """RS(6+6) (six rows) and RS(13+4) (17 shards) have no fused plan: the
    jobs are reconstructed and verified in base, every repaired shard framed
    by an identity item."""
    _, _, got = R.run(dev, name)
    assert got


def test_lrc_slow_patterns(dev):
    """EC6P3L3 (m + l = 6): reconstruct + verify one job at a time, then
    the identity items; bits still follow the caller's order."""
    _, _, got = R.run(dev, "lrc_slow")
    assert got


def test_uniform_queue_equals_repair_batch(dev):
    """The same bytes through the queue and through gfrs_repair_batch:
    identical image arena, identical bitmap."""
    r = R.build("rs63_uniform")
    _, dst, got = R.run(dev, "rs63_uniform")
    after_queue = dst.dev.cpu().numpy().copy()
    enc = A.encoder(r.t)
    src2, dst2 = R.load(r, dev)
    n = len(r.rjobs)
    slen, bad = r.rjobs[0][1], r.patterns[0]
    stride, img_stride = r.rjobs[1][0], r.rjobs[0][4]
    assert all(job == (j * stride, slen, 0, j * len(bad) * img_stride,
                       img_stride) for j, job in enumerate(r.rjobs))
    bm = A.bitmap(n)
    A.ok(L().gfrs_repair_batch(enc._ctx, vp(src2.ptr), slen, stride, n,
                               A.i32s(bad), len(bad), vp(dst2.ptr),
                               img_stride, A.BLOCK, A.u64s(r.bids),
                               A.u64s(r.vuids), bm), "repair_batch")
    A.sync(enc)
    assert A.bits(bm, n) == got
    # failed stripes' images included: both run the same plan on the same
    # bytes
    dst2.check(after_queue, what="uniform repair queue vs repair_batch")


@pytest.mark.parametrize("grid", ["1", "3"])
def test_forced_frame_walk_and_restage(dev, monkeypatch, grid):
    """GFRS_CRC_GRID is read on every launch: with 1 block, one block walks
    every frame of the bucket, restages at every descriptor change and
    crosses every job boundary with its prefetch; with 3, the contiguous
    ranges split inside multi-frame jobs."""
    monkeypatch.setenv("GFRS_CRC_GRID", grid)
    R.run(dev, "rs63_mixed", what="grid=%s" % grid)
    R.run(dev, "rs66_inplace", what="grid=%s" % grid)


def test_python_surface(dev):
    r = R.build("rs63_mixed")
    src, dst = R.load(r, dev, seed=82)
    enc = A.encoder(r.t)
    fails = enc.repair_queue(
        src.dev, [(src.off + off, slen, pat, dst.off + img_off, stride)
                  for off, slen, pat, img_off, stride in r.rjobs],
        r.patterns, dst.dev, r.bids, r.vuids)
    R.check(r, src, dst, [j for j, f in enumerate(fails) if f],
            what="Encoder.repair_queue")


def test_errors_write_nothing(dev):
    r = R.build("rs63_mixed")
    enc = A.encoder(r.t)
    src, dst = R.load(r, dev, seed=84)
    jobs = list(r.rjobs)
    n = len(jobs)

    def refused(code, what, enc=enc, src=src, dst=dst, r=r, **kw):
        rc, _ = R.call(enc, src, dst, r, **kw)
        assert rc == code, (what, rc)
        src.check(src.expect(), what="refused (base): " + what)
        dst.check(dst.expect(), what="refused (images): " + what)

    def swap(j, **f):
        off, slen, pat, img_off, stride = jobs[j]
        new = dict(off=off, slen=slen, pat=pat, img_off=img_off,
                   stride=stride, reserved=0)
        new.update(f)
        return jobs[:j] + [(new["off"], new["slen"], new["pat"],
                            new["img_off"], new["stride"],
                            new["reserved"])] + jobs[j + 1:]

    pats = r.patterns
    refused(R.ERR_INVALID, "shard index out of range in an unused pattern",
            patterns=pats + [[9]])
    refused(R.ERR_INVALID, "negative shard index",
            patterns=[[-1]] + pats[1:])
    refused(R.ERR_TOO_FEW, "m + 1 bad shards",
            patterns=pats + [[0, 1, 2, 3]])
    refused(R.ERR_INVALID, "empty pattern", patterns=pats + [[]])
    refused(R.ERR_INVALID, "repeated index", patterns=pats + [[1, 1]])
    refused(R.ERR_INVALID, "njobs = 0", njobs=0)
    refused(R.ERR_INVALID, "npat = 0", npat=0)
    refused(R.ERR_INVALID, "bad_off not starting at 0",
            boff=[1] + [sum(len(p) for p in pats[:i + 1])
                        for i in range(len(pats))])
    refused(R.ERR_INVALID, "pattern out of range",
            jobs=swap(5, pat=len(pats)))
    refused(R.ERR_INVALID, "negative pattern", jobs=swap(n - 1, pat=-1))
    refused(R.ERR_INVALID, "reserved != 0", jobs=swap(7, reserved=1))
    refused(R.ERR_NO_DATA, "zero shard_len in the last job",
            jobs=swap(n - 1, slen=0))
    refused(R.ERR_INVALID, "img_off misaligned",
            jobs=swap(9, img_off=jobs[9][3] + 2))
    refused(R.ERR_INVALID, "disk_dst misaligned", dst_shift=2)
    refused(R.ERR_INVALID, "img_stride misaligned",
            jobs=swap(8, stride=jobs[8][4] + 2))
    refused(R.ERR_INVALID, "img_stride below the image size",
            jobs=swap(n - 2, stride=R.round4(A.disk_size(jobs[n - 2][1])) - 4))
    refused(R.ERR_UNSUPPORTED, "block_len 4096", block_len=4096)
    refused(R.ERR_UNSUPPORTED, "block_len 131072", block_len=131072)
    # strict for every tactic: RS(6+6), whose batch path tolerates a repeat
    r66 = R.build("rs66_inplace")
    s66, d66 = R.load(r66, dev, seed=86)
    e66 = A.encoder(r66.t)
    for what, extra, code in [("repeat", [2, 3, 2], R.ERR_INVALID),
                              ("empty", [], R.ERR_INVALID),
                              ("m + 1 bad", list(range(7)), R.ERR_TOO_FEW)]:
        refused(code, "RS(6+6) " + what, enc=e66, src=s66, dst=d66, r=r66,
                patterns=r66.patterns + [extra])
    # LRC: three global losses are undecodable for the full-width call
    rl = R.build("lrc_single")
    sl, dl = R.load(rl, dev, seed=88)
    refused(R.ERR_TOO_FEW, "LRC12P2L2 [0,1,2]", enc=A.encoder(rl.t), src=sl,
            dst=dl, r=rl, patterns=rl.patterns + [[0, 1, 2]])
    # and the same arenas still serve a good call afterwards
    for enc_, s_, d_, r_ in [(enc, src, dst, r), (e66, s66, d66, r66)]:
        rc, got = R.call(enc_, s_, d_, r_)
        A.ok(rc, "after the refusals")
        R.check(r_, s_, d_, got, what="after the refusals " + r_.name)
