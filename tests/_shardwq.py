"""Shard write queues for the gfrs_shard_write_queue tests.

A queue is what the write side of a blobnode sees: a batch of PUTs
(datafile.go:342-384, raw shards of many sizes) and the bids of a chunk under
compaction (compact.go:236-344, disk images read through the CRC-checking
reader and written into the new chunk).  Everything the GPU module
(tests/test_gpu_shard_write_queue.py) feeds to the engine is generated here,
so tests/test_shard_write_queue_cpu.py can check the same queues against the
schedule builder and against the oracle alone.

Expectations come from the oracle only.  The payload of a raw job is its
source bytes; that of a SRC_IMAGE job the payload bytes of its source image as
they are after the flips (_shardq.payload_of).  The expected image is
pyoracle.shard_write(payload, bid, vuid), the expected crc pyoracle.crc32 of
the payload, the expected result of a SRC_IMAGE job _shardq.expect_one of the
whole-shard FOOTER job over the source image.

Sizes are those of _readq.LENS, each issued once as a raw job and once as a
SRC_IMAGE job, interleaved.  Sources - raw shards, and images written by the
oracle with other ids - lie at odd addresses with garbage between them; the
new images are 4-aligned with uneven guarded gaps, in another order than the
jobs, and their ids use all eight bytes.
"""
import ctypes
import functools

import numpy as np

import _arena as A
import _shardq as S
from _arena import L, Arena, oracle, vp

from cubefs_amd import runtime

LENS = S.LENS
PAYLOAD = S.PAYLOAD
BLOCK = A.BLOCK
SRC_IMAGE = runtime.WJOB_SRC_IMAGE
ERR_NO_DATA, ERR_INVALID, ERR_BLOCK, ERR_NOMEM, ERR_UNSUPPORTED = \
    S.ERR_NO_DATA, S.ERR_INVALID, S.ERR_BLOCK, S.ERR_NOMEM, S.ERR_UNSUPPORTED
DEAD = S.DEAD


def nframes(size):
    return (size - 1) // PAYLOAD + 1


def new_ids(j):
    """bid and vuid of the image job j writes: all eight bytes of both in
    use, and none of _shardq.ids."""
    return (0x8877665544332211 + 0x0102030405 * j) & (2 ** 64 - 1), \
        (0xA1B2C3D4E5F60718 - 0x01000203 * j) & (2 ** 64 - 1)


class WQueue:
    """sources[j] = (offset in src, bytes there after the flips - a raw shard
    or a disk image); jobs[j] = (src_off, size, bid, vuid, src_bid, src_vuid,
    img_off, flags); flips = [(job, byte relative to the source start - may
    lie in the gap behind it -, mask)]."""

    def __init__(self, name, specs, flips=()):
        """specs: (size, flags[, src_bid delta, src_vuid delta]) per job."""
        self.name = name
        self.flips = list(flips)
        self.sources, at, gaps = [], 0, []
        for j, s in enumerate(specs):
            size, flags = s[:2]
            r = S.raw(size, j)
            if flags & SRC_IMAGE:
                sb, sv = S.ids(j)
                data = oracle.shard_write(r.copy(), bid=sb, vuid=sv)
                assert data.size == A.disk_size(size)
            else:
                data = r.copy()
            self.sources.append([at, data])
            gap = 2 + 2 * (j % 3) + data.size % 2   # every source at an even
            gaps.append(gap)                        # offset of an odd base
            at += data.size + gap
        self.src_bytes = at
        self.gap_flips = []
        for j, byte, mask in self.flips:
            data = self.sources[j][1]
            if byte < data.size:
                data[byte] ^= mask
            else:
                assert byte - data.size < gaps[j]
                self.gap_flips.append((self.sources[j][0] + byte, mask))
        # new images: odd jobs first, then the even ones backwards; uneven
        # guarded gaps, every image 4-aligned
        n = len(specs)
        place = [None] * n
        at = 0
        order = [j for j in range(n) if j % 2] + \
            [j for j in range(n) if j % 2 == 0][::-1]
        for j in order:
            place[j] = at
            self.dst_bytes = at + A.disk_size(specs[j][0])
            at = S.G.round4(self.dst_bytes) + 4 * (1 + (5 * j) % 4)
        self.jobs = []
        for j, s in enumerate(specs):
            size, flags = s[:2]
            bid, vuid = new_ids(j)
            sb, sv = S.ids(j) if flags & SRC_IMAGE else (0, 0)
            db, dv = (s[2], s[3]) if len(s) > 2 else (0, 0)
            self.jobs.append((self.sources[j][0], size, bid, vuid, sb ^ db,
                              sv ^ dv, place[j], flags))

    def payload(self, j):
        """The payload bytes job j carries into its new image."""
        _, size, _, _, _, _, _, flags = self.jobs[j]
        data = self.sources[j][1]
        return S.payload_of(data, size) if flags & SRC_IMAGE else data


def _flip_queue(name):
    specs, flips, kinds = [], [], []
    for size in S.FLIP_LENS:
        for kind, fl in S._sites(size, 0, size):
            if kind.endswith("_plain"):     # the same sites as without it
                continue
            j = len(specs)
            db = 1 << (j % 64) if kind == "want_bid" else 0
            dv = 1 << ((3 * j) % 64) if kind == "want_vuid" else 0
            specs.append((size, SRC_IMAGE, db, dv))
            flips += [(j, byte, mask) for byte, mask in fl]
            kinds.append(kind)
    q = WQueue(name, specs, flips)
    q.kinds = kinds
    return q


@functools.lru_cache(maxsize=None)
def build(name):
    if name == "clean":
        return WQueue(name, [(s, f) for s in LENS for f in (0, SRC_IMAGE)])
    if name == "all_raw":
        return WQueue(name, [(s, 0) for s in (1, 4096, 65597, 131064)])
    if name == "all_image":
        return WQueue(name, [(s, SRC_IMAGE) for s in (17, 65533, 131065)])
    if name == "one":
        return WQueue(name, [(65533, SRC_IMAGE)])
    if name == "tiny":
        # four frames per bucket: with three workgroups the last one is idle
        return WQueue(name, [(131065, 0), (131065, SRC_IMAGE), (17, SRC_IMAGE),
                             (17, 0)])
    if name == "flips":
        return _flip_queue(name)
    raise KeyError(name)


CLEAN_QUEUES = ["clean", "all_raw", "all_image", "one", "tiny"]
GPU_QUEUES = CLEAN_QUEUES + ["flips"]


# ---- the oracle's answers ----------------------------------------------------

def read_job(job):
    """The gfrs_shard_read_queue job the contract names for a SRC_IMAGE job:
    the whole shard with FOOTER, the source's ids."""
    src_off, size, _, _, sb, sv, _, _ = job
    return (src_off, size, sb, sv, 0, size, 0, S.FOOTER)


def expect_one(q, j):
    job = q.jobs[j]
    _, size, bid, vuid, _, _, _, flags = job
    if flags & SRC_IMAGE:
        return S.expect_one(q.sources[j][1], read_job(job))
    return dict(status=0, crc=oracle.crc32(q.payload(j).copy()), bad_block=-1,
                bid=bid, vuid=vuid, size=size)


@functools.lru_cache(maxsize=None)
def expected(name):
    q = build(name)
    return [expect_one(q, j) for j in range(len(q.jobs))]


@functools.lru_cache(maxsize=None)
def expected_images(name):
    q = build(name)
    out = []
    for j, job in enumerate(q.jobs):
        img = oracle.shard_write(q.payload(j).copy(), bid=job[2], vuid=job[3])
        img.setflags(write=False)
        out.append(img)
    return out


# ---- C ABI arguments ------------------------------------------------------------

def wjob_array(jobs):
    """jobs: (src_off, size, bid, vuid, src_bid, src_vuid, img_off, flags[,
    reserved])."""
    arr = (runtime.WJob * max(1, len(jobs)))()
    for j, job in enumerate(jobs):
        arr[j] = runtime.WJob(*job[:8], job[8] if len(job) > 8 else 0)
    return arr


class Schedule:
    pass


def schedule(jobs, block_len=BLOCK, item_cap=None, njobs=None):
    """gfrs_compute_shard_write_queue_schedule -> (rc, Schedule or None)."""
    nj = len(jobs)
    if item_cap is None:
        item_cap = nj
    items = (runtime.WItem * max(1, item_cap))()
    prefix = (ctypes.c_uint64 * (max(1, item_cap) + 2))()
    buckets = (runtime.WBucket * 2)()
    ni, nb, tot = ctypes.c_int(), ctypes.c_int(), ctypes.c_uint64()
    rc = L().gfrs_compute_shard_write_queue_schedule(
        wjob_array(jobs), nj if njobs is None else njobs, block_len, item_cap,
        items, prefix, ctypes.byref(ni), buckets, ctypes.byref(nb),
        ctypes.byref(tot))
    if rc != 0:
        return rc, None
    s = Schedule()
    s.items = [(i.job, i.src, i.size, i.img, i.flags)
               for i in items[:ni.value]]
    s.buckets = [(b.src_image, b.first, b.count) for b in buckets[:nb.value]]
    s.prefix = list(prefix[:ni.value + nb.value])
    s.total_frames = tot.value
    return 0, s


# ---- GPU runner: one call, both arenas checked --------------------------------

def load(q, dev, seed=110):
    """(src arena, dst arena), both uploaded."""
    src = Arena(dev, q.src_bytes, 1, seed=seed)
    for off, data in q.sources:
        src.put(off, data)
    for off, mask in q.gap_flips:
        src.host[src.off + off] ^= mask
    src.upload()
    dst = Arena(dev, q.dst_bytes, 4, seed=seed + 1)
    dst.upload()
    return src, dst


fresh_results = S.fresh_results
as_dicts = S.as_dicts


def call(enc, src, dst, q, jobs=None, block_len=BLOCK, njobs=None,
         dst_shift=0):
    """-> (rc, list of result dicts)."""
    jobs = q.jobs if jobs is None else jobs
    res = fresh_results(len(jobs))
    rc = L().gfrs_shard_write_queue(
        enc._ctx, vp(dst.ptr + dst_shift), vp(src.ptr), wjob_array(jobs),
        len(jobs) if njobs is None else njobs, block_len, res)
    return rc, as_dicts(res, len(jobs))


def check(q, src, dst, got, what=""):
    """Every result field equals the oracle's; dst: the expected image of
    every job and not one other byte; src unchanged."""
    want = expected(q.name)
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        assert g == w, (what, j, q.jobs[j], getattr(q, "kinds", None) and
                        q.kinds[j], g, w)
    img = dst.expect()
    for job, image in zip(q.jobs, expected_images(q.name)):
        dst.put(job[6], image, img)
    dst.check(img, what=what + " dst")
    src.check(src.expect(), what=what + " src")


def run(dev, name, what=""):
    q = build(name)
    enc = A.encoder(A.tactic(4, 2))
    src, dst = load(q, dev)
    what = "%s shard write queue %s" % (what, name)
    rc, got = call(enc, src, dst, q)
    A.ok(rc, what)
    check(q, src, dst, got, what)
    return src, dst
