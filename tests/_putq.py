"""Put queues for the gfrs_put_queue tests.

A queue is what the access gateway's PUT path hands to blobnode: concurrent
blobs of different sizes, each to be encoded into the n+m+l disk images of
its stripe - header, crc32block body, footer - with its bid and the vuids of
its volume.  Everything the GPU module (tests/test_gpu_put_queue.py) feeds to
the engine is generated here, so tests/test_put_queue_cpu.py can check the
same queues against the schedule builder and against the oracle alone.

Expectations come from the oracle only: pyoracle.rs_encode / lrc_encode of
the job's data shards, then pyoracle.shard_write(shard, bid, vuid) of every
shard and pyoracle.crc32(shard) for the crcs - never from the engine.

The source arena holds the DATA shards only (n per job, odd offsets, odd
gaps): behind shard n-1 of the last job there is nothing but the guard.

Shard lengths are the smallest at which each path can still go wrong
(tests/_encq.py explains the edges):
  1, 16, 17, 4095, 4096, 4097, 8209     ragged tail / vector / the class edge
                                        a wide tactic does not have
  16383, 16385, 49153                   pass edges
  65531, 65532, 65533, 65596, 65597     frame edges
  131064, 131065                        two exact frames; a third of one byte
  1048576, 1048577                      the 3-wave variant (one queue only)

  queue       tactic      covers
  rs63        EC6P3       narrow: the encode queue's kernels, small buckets
  rs66        EC6P6       G = 2, rows 4+2; every length, both 1 MiB ones
  rs1512      EC15P12     G = 3, odd k
  rs164       EC16P4      k = 16, G = 1: first index past the 16-slot rows
  rs248       EC24P8      k = 24, G = 2
  lrc442      EC4P4L2     LRC, composed rows, G = 2
  lrc16202    EC16P20L2   22 rows, groups 4,4,4,4,4,2
  rs324       RS(32+4)    k = 32, the gate's edge, 36 header lanes
"""
import ctypes
import functools

import numpy as np

import _arena as A
import _encq as E
from _arena import L, Arena, oracle, vp
from _encq import (ERR_BLOCK, ERR_INVALID, ERR_NO_DATA,  # noqa: F401
                   ERR_NOMEM, ERR_UNSUPPORTED, frames, interleave, round4)

from cubefs_amd import codemode, runtime
from cubefs_amd.ec import _tactic_struct

ERR_CODEMODE = -1
WIDE_FRAME = [1, 16, 17, 4095, 4096, 4097, 8209, 16383, 16385, 49153, 65531,
              65532, 65533, 65596, 65597, 131064, 131065]
LARGE = E.LARGE
ROWS = 4                      # parity rows per group
HEADER, FOOTER = 32, 8
GAPS = E.GAPS
NVOL = 2


def rs324_tactic():
    """RS(32+4): the widest tactic the put queue serves."""
    codemode.extend(248, "EC32P4", codemode.Tactic(32, 4, 0, 1, 35, 0, 2048))
    return codemode.get_tactic("EC32P4")


def rs334_tactic():
    """RS(33+4): one data shard past the gate."""
    codemode.extend(249, "EC33P4", codemode.Tactic(33, 4, 0, 1, 36, 0, 2048))
    return codemode.get_tactic("EC33P4")


def wide_gate(t):
    """Outside the gate of the fused encode kernels (include/gfrs.h)."""
    return not E.fused_gate(t)


def group_rows(t):
    rows = t.M + t.L
    return [min(ROWS, rows - r) for r in range(0, rows, ROWS)]


def bucket_of(t, slen):
    """(kind, param) the schedule must give a job of this length."""
    if wide_gate(t) and slen <= E.SMALL_MAX:
        return E.KIND_FRAME, E.VAR_BELOW
    return E.bucket_of(slen)


def vuid_sets(total, nvol=NVOL):
    """nvol lists of `total` vuids, no two alike."""
    return [[((v + 3) << 44) | (0x51ED00 + 4096 * v + i) for i in range(total)]
            for v in range(nvol)]


class PQueue:
    """jobs[j] = (off, slen, img_off, img_stride, bid, vol); data[j] = the
    oracle's (total, slen) stripe of job j (read-only); vuids[vol][i]."""

    def __init__(self, name, t, lens, delta=1):
        self.name, self.t = name, t
        self.total = t.N + t.M + t.L
        self.delta = delta
        self.vuids = vuid_sets(self.total)
        n = len(lens)
        need, seen = {}, {}
        for slen in lens:
            need[slen] = need.get(slen, 0) + 1
        self.data, src = [], []
        off = 0
        for j, slen in enumerate(lens):
            ref = A.ref_stripes(t, need[slen], slen, seed=37)
            s = seen.get(slen, 0)
            seen[slen] = s + 1
            self.data.append(ref[s])
            src.append(off)
            off += t.N * slen + GAPS[j % len(GAPS)]   # data shards only
        self.nbytes = src[-1] + t.N * lens[-1]
        # image order is not job order: odd jobs first, then the even ones
        # backwards; uneven 4-aligned padding; tight stride for odd jobs,
        # padded for even ones
        place = [None] * n
        at = end = 0
        order = [j for j in range(n) if j % 2] + \
            [j for j in range(n) if j % 2 == 0][::-1]
        for j in order:
            size = A.disk_size(lens[j])
            stride = round4(size) + (0 if j % 2 else 4 * (1 + j % 3))
            place[j] = (at, stride)
            end = at + (self.total - 1) * stride + size
            at = round4(end) + 4 * ((5 * j) % 4)
        self.img_bytes = end     # the arena ends with the last image placed
        self.jobs = [(src[j], lens[j]) + place[j] +
                     ((1 << 40) | (7919 * (j + 1)), (j + j // 3) % NVOL)
                     for j in range(n)]

    def image_regions(self, j):
        """[(offset in disk_dst, size)] of job j's n+m+l images."""
        _, slen, img_off, stride = self.jobs[j][:4]
        return [(img_off + i * stride, A.disk_size(slen))
                for i in range(self.total)]

    def flat_vuids(self):
        return [v for vol in self.vuids for v in vol]


@functools.lru_cache(maxsize=None)
def build(name):
    get = codemode.get_tactic
    if name == "rs63":
        return PQueue(name, get("EC6P3"),
                      interleave(E.SMALL + E.NI3, E.FRAME))
    if name == "rs66":
        return PQueue(name, get("EC6P6"), interleave(WIDE_FRAME, LARGE))
    if name == "rs1512":
        return PQueue(name, get("EC15P12"), interleave(WIDE_FRAME))
    if name == "rs164":
        return PQueue(name, get("EC16P4"), interleave(WIDE_FRAME))
    if name == "rs248":
        return PQueue(name, get("EC24P8"), [17, 4097, 16385, 65533, 131065])
    if name == "lrc442":
        return PQueue(name, get("EC4P4L2"), interleave(WIDE_FRAME))
    if name == "lrc16202":
        return PQueue(name, get("EC16P20L2"), [17, 65533, 65597])
    if name == "rs324":
        return PQueue(name, rs324_tactic(), [1, 4097, 65533])
    if name == "seq_tiny":
        # steps of the sequence test: a small and a growing queue
        return PQueue(name, get("EC6P6"), [1000, 70001, 17])
    if name == "seq_more":
        return PQueue(name, get("EC6P6"),
                      [4097, 65533, 131065, 16, 200001, 8209, 65597])
    raise KeyError(name)


GPU_QUEUES = ["rs63", "rs66", "rs1512", "rs164", "rs248", "lrc442",
              "lrc16202", "rs324"]


@functools.lru_cache(maxsize=None)
def expectations(name):
    """Per job: (the n+m+l disk images, their crcs), oracle.shard_write and
    oracle.crc32 of the oracle-encoded stripe."""
    q = build(name)
    out = []
    for j, job in enumerate(q.jobs):
        bid, vol = job[4], job[5]
        imgs = [oracle.shard_write(q.data[j][i].copy(), bid=bid,
                                   vuid=q.vuids[vol][i])
                for i in range(q.total)]
        crcs = [oracle.crc32(q.data[j][i].copy()) for i in range(q.total)]
        out.append((imgs, crcs))
    return out


# ---- C ABI arguments --------------------------------------------------------

def pjob_array(jobs):
    """jobs: (off, slen, img_off, img_stride, bid, vol[, reserved])."""
    arr = (runtime.PJob * max(1, len(jobs)))()
    for j, job in enumerate(jobs):
        arr[j] = runtime.PJob(job[0], job[1], job[2], job[3], job[4], job[5],
                              job[6] if len(job) > 6 else 0)
    return arr


# ---- schedule (GPU-free export) ---------------------------------------------

class Schedule:
    pass


def schedule(t, jobs, vuids=None, nvol=None, block_len=A.BLOCK, item_cap=None,
             image_cap=None):
    """gfrs_compute_put_queue_schedule -> (rc, Schedule or None)."""
    nj = len(jobs)
    total = t.N + t.M + t.L
    vuids = vuid_sets(total) if vuids is None else vuids
    nvol = len(vuids) if nvol is None else nvol
    flat = [v for vol in vuids for v in vol]
    item_cap = nj if item_cap is None else item_cap
    image_cap = nj * total if image_cap is None else image_cap
    items = (runtime.EItem * max(1, item_cap))()
    prefix = (ctypes.c_uint64 * (max(1, item_cap) + 2))()
    buckets = (runtime.EBucket * E.MAX_BUCKETS)()
    images = (runtime.RImage * max(1, image_cap))()
    rows = (ctypes.c_int32 * 64)()
    ni, nb, nimg = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    wide, ng = ctypes.c_int(-1), ctypes.c_int()
    ts = _tactic_struct(t)
    rc = L().gfrs_compute_put_queue_schedule(
        ctypes.byref(ts), pjob_array(jobs), nj, A.u64s(flat or [0]), nvol,
        block_len, item_cap, image_cap, items, prefix, ctypes.byref(ni),
        buckets, ctypes.byref(nb), images, ctypes.byref(nimg),
        ctypes.byref(wide), ctypes.byref(ng), rows)
    if rc != 0:
        return rc, None
    s = Schedule()
    s.items = [(i.job, i.off, i.shard_len, i.img, i.img_stride, i.reserved)
               for i in items[:ni.value]]
    s.buckets = [(b.kind, b.param, b.first, b.count)
                 for b in buckets[:nb.value]]
    nframe = sum(1 for b in s.buckets if b[0] == E.KIND_FRAME)
    nfitems = sum(b[3] for b in s.buckets if b[0] == E.KIND_FRAME)
    s.prefix = list(prefix[:nfitems + nframe])
    s.images = [(i.off, i.size, i.bid, i.vuid) for i in images[:nimg.value]]
    s.wide = wide.value
    s.group_rows = list(rows[:ng.value])
    return 0, s


# ---- GPU runner: one call, both arenas checked ------------------------------

def load(q, dev, seed=130):
    """(source arena with the data shards only, image arena), both
    uploaded."""
    src = Arena(dev, q.nbytes, q.delta, seed=seed)
    for j, job in enumerate(q.jobs):
        off, slen = job[0], job[1]
        for i in range(q.t.N):
            src.put(off + i * slen, q.data[j][i])
    src.upload()
    dst = Arena(dev, q.img_bytes, 4, seed=seed + 1)
    dst.upload()
    return src, dst


FILL = 0xA5A5A5A5


def call(enc, src, dst, q, jobs=None, block_len=A.BLOCK, njobs=None,
         dst_shift=0, vuids=None, nvol=None, want_crcs=True):
    """-> (rc, crcs): crcs a (len(jobs), total) uint32 array preset to FILL,
    or None when the call passes NULL."""
    jobs = q.jobs if jobs is None else jobs
    flat = q.flat_vuids() if vuids is None else vuids
    crcs = np.full((max(1, len(jobs)), q.total), FILL, dtype=np.uint32)
    rc = L().gfrs_put_queue(
        enc._ctx, vp(dst.ptr + dst_shift), vp(src.ptr), pjob_array(jobs),
        len(jobs) if njobs is None else njobs, A.u64s(flat),
        NVOL if nvol is None else nvol, block_len,
        crcs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
        if want_crcs else None)
    return rc, (crcs[:len(jobs)] if want_crcs else None)


def check(q, src, dst, crcs, what="", jobs=None):
    """disk_dst: the oracle's images and not one other byte changed; base
    unchanged; crcs (unless None) the oracle's."""
    exp = expectations(q.name)
    want = dst.expect()
    picks = range(len(q.jobs)) if jobs is None else jobs
    for j in picks:
        for (off, size), img in zip(q.image_regions(j), exp[j][0]):
            assert img.size == size
            dst.put(off, img, want)
    dst.check(want, what=what + " images")
    src.check(src.expect(), what=what + " base")
    if crcs is not None:
        for r, j in enumerate(picks):
            assert [int(x) for x in crcs[r]] == exp[j][1], (what, j)


def run(dev, name, what=""):
    q = build(name)
    enc = A.encoder(q.t)
    src, dst = load(q, dev)
    what = "%s put queue %s" % (what, name)
    rc, crcs = call(enc, src, dst, q)
    A.ok(rc, what)
    check(q, src, dst, crcs, what)
    return src, dst
