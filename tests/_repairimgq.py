"""Repair-image queues for the gfrs_repair_queue tests.

A queue of tests/_repairq.py (jobs of different shard lengths and erasure
patterns in one buffer) plus the place of every job's disk images in a second
buffer.  Everything the GPU module (tests/test_gpu_repair_queue.py) feeds to
the engine is generated here, so tests/test_repair_queue_cpu.py can check the
same queues against the schedule builder and against the oracle alone.

Expectations come from _verdict.expected (the reference's Reconstruct +
Verify of one stripe) and oracle.shard_write of its reconstruction, job by
job - never from the engine.

Shard lengths come from the frame kernel's constants (16-byte vectors,
4096-byte pieces, 16384-byte passes, 65532-byte frame payloads):
  1, 15, 16, 17, 33          ragged tail only / one vector / vectors + tail
  4095, 4096, 4097, 8209     piece edge; two pieces + vector + ragged byte
  16383, 16385, 49153        pass edge; one byte into the fourth pass
  65531, 65532, 65533        one byte short of / exactly / one byte past a frame
  70005                      a full frame + a 4473-byte one
  131064, 131065             two exact frames; and a third of one byte
"""
import ctypes
import functools

import _arena as A
import _repairq as Q
import _verdict as V
from _arena import L, Arena, oracle, vp

from cubefs_amd import runtime
from cubefs_amd.ec import _tactic_struct

LENS = [1, 15, 16, 17, 33, 4095, 4096, 4097, 8209, 16383, 16385, 49153,
        65531, 65532, 65533, 70005, 131064, 131065]
PAYLOAD = 65532
ROWS = 4
FUSED, INPLACE, INPLACE_SLOW = 0, 1, 2
ERR_TOO_FEW, ERR_NO_DATA, ERR_INVALID, ERR_NOMEM, ERR_UNSUPPORTED = \
    Q.ERR_TOO_FEW, Q.ERR_NO_DATA, Q.ERR_INVALID, Q.ERR_NOMEM, \
    Q.ERR_UNSUPPORTED
BID0, VUID0 = 9000, 0x99AABBCCDD


def frames(slen):
    return (slen + PAYLOAD - 1) // PAYLOAD


def round4(n):
    return (n + 3) // 4 * 4


class RQueue:
    """q: the _repairq.Queue (jobs, data, flips).  rjobs[j] = (off, slen,
    pattern, img_off, img_stride); ids[j] = index of job j's first image in
    bids / vuids."""

    def __init__(self, q, uniform=False):
        self.q, self.name, self.t = q, q.name, q.t
        self.total, self.patterns = q.total, q.patterns
        n = len(q.jobs)
        place = [None] * n
        at = 0
        if uniform:
            # the layout of gfrs_repair_batch: image (s, b) at
            # (s * nbad + b) * stride
            stride = round4(A.disk_size(q.jobs[0][1])) + 8
            nb = len(q.patterns[0])
            for j in range(n):
                place[j] = (j * nb * stride, stride)
            at = (n * nb - 1) * stride + A.disk_size(q.jobs[0][1])
        else:
            # image order is not job order: odd jobs first, then the even
            # ones backwards; uneven 4-aligned padding; tight stride for odd
            # jobs, padded for even ones
            order = [j for j in range(n) if j % 2] + \
                [j for j in range(n) if j % 2 == 0][::-1]
            for j in order:
                slen, nb = q.jobs[j][1], len(q.patterns[q.jobs[j][2]])
                stride = round4(A.disk_size(slen)) + \
                    (0 if j % 2 else 4 * (1 + j % 3))
                place[j] = (at, stride)
                end = at + (nb - 1) * stride + A.disk_size(slen)
                at = round4(end) + 4 * ((5 * j) % 4)
            at = end    # the arena ends with the last image placed
        self.img_bytes = at
        self.rjobs = [(off, slen, pat) + place[j]
                      for j, (off, slen, pat) in enumerate(q.jobs)]
        self.ids, k = [], 0
        for _, _, pat in q.jobs:
            self.ids.append(k)
            k += len(q.patterns[pat])
        self.nimg = k
        self.bids = [BID0 + i for i in range(k)]
        self.vuids = [VUID0 + 3 * i for i in range(k)]

    def bad_of(self, j):
        return self.q.bad_of(j)

    def image_regions(self, j):
        """[(offset in disk_dst, size)] of job j's images, pattern order."""
        _, slen, pat, img_off, stride = self.rjobs[j]
        return [(img_off + b * stride, A.disk_size(slen))
                for b in range(len(self.patterns[pat]))]


def _interleaved(lens, npat, njobs):
    return Q._interleaved(lens, npat, njobs)


@functools.lru_cache(maxsize=None)
def build(name):
    if name == "rs63_mixed":
        # [1,8] and [8,1] share a plan (same erasures) but not a colpack
        pats = [[1], [0, 5], [0, 2, 4], [7], [1, 8], [8, 1]]
        return RQueue(Q.Queue(name, "EC6P3", pats,
                              _interleaved(LENS, 6, 36)))
    if name == "rs63_uniform":
        # constant length, gap and image stride: also one gfrs_repair_batch
        return RQueue(Q.Queue(name, "EC6P3", [[1, 7]], [(65533, 0)] * 7,
                              gap=lambda j: 5), uniform=True)
    if name == "rs124_k12":
        pats = [[1], [0, 13], [2, 5, 11, 15], [14, 3]]
        lens = [70005, 33, 4097, 65533, 16385, 1, 131065, 4096, 49153, 15]
        return RQueue(Q.Queue(name, "EC12P4", pats,
                              _interleaved(lens, 4, 12)))
    if name == "lrc_single":
        # LRC12P2L2 inside the fused budget: data, global parity, a lost
        # local parity alone and with data, data + global parity; every flip
        # lands in a surviving LOCAL parity (14 or 15)
        pats = [[0], [12], [14], [3, 15], [0, 13]]
        lens = [33, 65533, 4097, 17, 70005, 8209, 16383]
        return RQueue(Q.Queue(name, "LRC12P2L2", pats,
                              _interleaved(lens, 5, 15), cols=[14, 15]))
    if name == "rs66_inplace":
        # RS(6+6): m + l = 6 rows do not fit the fused kernel; 3..6 bad,
        # every job reconstructed in place and framed by identity items
        pats = [[0, 1, 2], [8, 1, 5, 3], [0, 1, 2, 3, 4],
                [5, 4, 3, 2, 1, 0], [4, 9, 10, 11]]
        lens = [17, 4097, 65533, 8209, 16, 70005, 1, 131064, 16383, 33]
        return RQueue(Q.Queue(name, "EC6P6", pats,
                              _interleaved(lens, 5, 20)))
    if name == "rs134_w17":
        # 17 shards: in place by width
        pats = [[16], [0, 12], [3], [14, 1, 2]]
        lens = [4097, 15, 65533, 16, 33, 8209, 131065]
        return RQueue(Q.Queue(name, "EC13P4", pats,
                              _interleaved(lens, 4, 14)))
    if name == "lrc_slow":
        # EC6P3L3 (m + l = 6): in place, one job at a time
        t = V.get_tactic("EC6P3L3")
        n, m, l = t.N, t.M, t.L
        pats = [[n + m], [n + m + l - 1, 0], [n, n + m], [0, n + m, n]]
        lens = [33, 4097, 17, 65533, 16]
        return RQueue(Q.Queue(name, "EC6P3L3", pats,
                              _interleaved(lens, 4, 14),
                              cols=list(range(n + m, n + m + l))))
    if name == "seq_small":
        # a step of tests/test_gpu_sequences.py: small and frame class
        return RQueue(Q.Queue(name, "EC6P3", [[1], [0, 5], [8, 1]],
                              _interleaved([1000, 4093, 70001], 3, 6)))
    raise KeyError(name)


GPU_QUEUES = ["rs63_mixed", "rs124_k12", "lrc_single", "rs66_inplace",
              "rs134_w17", "lrc_slow", "rs63_uniform"]


@functools.lru_cache(maxsize=None)
def expectations(name):
    """[(reconstructed (total, slen), failed) or UNDECODABLE] per job."""
    r = build(name)
    return [V.expected(r.t, r.q.data[j], r.bad_of(j))
            for j in range(len(r.rjobs))]


@functools.lru_cache(maxsize=None)
def images(name):
    """Per job: None when the job fails, else its images in pattern order
    (oracle.shard_write of the oracle's reconstruction)."""
    r = build(name)
    out = []
    for j, (rec, failed) in enumerate(expectations(name)):
        if failed:
            out.append(None)
            continue
        out.append([oracle.shard_write(rec[idx].copy(),
                                       bid=r.bids[r.ids[j] + b],
                                       vuid=r.vuids[r.ids[j] + b])
                    for b, idx in enumerate(r.bad_of(j))])
    return out


# ---- C ABI arguments --------------------------------------------------------

def rjob_array(jobs):
    """jobs: (off, slen, pattern, img_off, img_stride[, reserved])."""
    arr = (runtime.RJob * max(1, len(jobs)))()
    for j, job in enumerate(jobs):
        off, slen, pat, img_off, stride = job[:5]
        arr[j] = runtime.RJob(off, slen, img_off, stride, pat,
                              job[5] if len(job) > 5 else 0)
    return arr


# ---- schedule (GPU-free export) -------------------------------------------------

class Schedule:
    pass


def schedule(t, jobs, patterns, bids=None, vuids=None, block_len=A.BLOCK,
             item_cap=None, image_cap=None, boff=None):
    """gfrs_compute_repair_queue_schedule -> (rc, Schedule or None)."""
    nj, npat = len(jobs), len(patterns)
    bad, off = Q.bad_lists(patterns)
    if boff is not None:
        off = A.i32s(boff)
    nimg = sum(len(patterns[job[2]]) for job in jobs
               if 0 <= job[2] < npat) if boff is None else 64
    item_cap = max(nimg, nj) if item_cap is None else item_cap
    image_cap = nimg if image_cap is None else image_cap
    items = (runtime.RItem * max(1, item_cap))()
    prefix = (ctypes.c_uint64 * (max(1, item_cap) + ROWS))()
    buckets = (runtime.RBucket * ROWS)()
    imgs = (runtime.RImage * max(1, image_cap))()
    cls = (ctypes.c_int32 * max(1, npat))()
    gm = (ctypes.c_int32 * max(1, npat))()
    nw = (ctypes.c_int32 * max(1, npat))()
    colpack = (ctypes.c_uint32 * max(1, npat))()
    inplace = (ctypes.c_int32 * max(1, nj))()
    ni, nb, nim, nin = (ctypes.c_int(), ctypes.c_int(), ctypes.c_int(),
                        ctypes.c_int())
    ts = _tactic_struct(t)
    rc = L().gfrs_compute_repair_queue_schedule(
        ctypes.byref(ts), rjob_array(jobs), nj, bad, off, npat, block_len,
        A.u64s(bids) if bids else None, A.u64s(vuids) if vuids else None,
        item_cap, image_cap, items, prefix, ctypes.byref(ni), buckets,
        ctypes.byref(nb), imgs, ctypes.byref(nim), cls, gm, nw, colpack,
        inplace, ctypes.byref(nin))
    if rc != 0:
        return rc, None
    s = Schedule()
    s.items = [(i.job, i.desc, i.off, i.shard_len, i.img, i.img_stride)
               for i in items[:ni.value]]
    s.buckets = [(b.gm, b.first, b.count) for b in buckets[:nb.value]]
    s.prefix = list(prefix[:ni.value + nb.value])
    s.images = [(i.off, i.size, i.bid, i.vuid) for i in imgs[:nim.value]]
    s.cls, s.gm = list(cls[:npat]), list(gm[:npat])
    s.nw, s.colpack = list(nw[:npat]), list(colpack[:npat])
    s.inplace = list(inplace[:nin.value])
    return 0, s


def fused_plan(t, bad):
    """(rc, nout, colpack) of gfrs_compute_plan's fused repair plan."""
    cap = 64
    total = t.N + t.M + t.L
    inn, out = (ctypes.c_int32 * cap)(), (ctypes.c_int32 * cap)()
    rows = (ctypes.c_uint8 * (cap * total))()
    nin, nout, rowk = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    cmp_mask, colpack = ctypes.c_uint32(), ctypes.c_uint32()
    ts = _tactic_struct(t)
    rc = L().gfrs_compute_plan(ctypes.byref(ts), 3, A.i32s(bad), len(bad),
                               cap, inn, ctypes.byref(nin), out,
                               ctypes.byref(nout), rows, ctypes.byref(rowk),
                               ctypes.byref(cmp_mask), ctypes.byref(colpack))
    return rc, nout.value, colpack.value


def fused_gate(t, bad):
    """The gate of gfrs_repair_batch's fused path (include/gfrs.h)."""
    nglob = sum(1 for i in bad if i < t.N + t.M)
    return (t.M >= 1 and t.M + t.L <= 4 and t.N + t.M + t.L <= 16 and
            nglob <= t.M)


# ---- GPU runner: one call, both arenas checked ------------------------------------

def load(r, dev, seed=80):
    """(base arena with the survivors, image arena), both uploaded."""
    src = Q.load(r.q, dev, seed=seed)
    dst = Arena(dev, r.img_bytes, 4, seed=seed + 1)
    dst.upload()
    return src, dst


def call(enc, src, dst, r, jobs=None, patterns=None, block_len=A.BLOCK,
         njobs=None, npat=None, boff=None, dst_shift=0):
    jobs = r.rjobs if jobs is None else jobs
    patterns = r.patterns if patterns is None else patterns
    bad, off = Q.bad_lists(patterns)
    if boff is not None:
        off = A.i32s(boff)
    nj = len(jobs) if njobs is None else njobs
    bm = A.bitmap(max(1, len(jobs)))
    rc = L().gfrs_repair_queue(
        enc._ctx, vp(src.ptr), rjob_array(jobs), nj, bad, off,
        len(patterns) if npat is None else npat, vp(dst.ptr + dst_shift),
        block_len, A.u64s(r.bids), A.u64s(r.vuids), bm)
    return rc, A.bits(bm, len(jobs))


def bad_regions(r):
    return [(off + i * slen, slen)
            for off, slen, pat, _, _ in r.rjobs for i in r.patterns[pat]]


def check(r, src, dst, got, what=""):
    """Bits equal the oracle's; every image of a passing job equals the
    oracle's; no other byte of either arena changed (a failed job's images
    and every bad shard's region of base are unspecified)."""
    exp = expectations(r.name)
    fails = [j for j, e in enumerate(exp) if e[1]]
    assert got == fails, (what, got, fails)
    want = dst.expect()
    unspec = []
    for j, imgs in enumerate(images(r.name)):
        regions = r.image_regions(j)
        if imgs is None:
            unspec += regions
            continue
        for (off, size), img in zip(regions, imgs):
            assert img.size == size
            dst.put(off, img, want)
    dst.check(want, unspec, what=what + " images")
    src.check(src.expect(), bad_regions(r), what=what + " base")


def run(dev, name, what=""):
    r = build(name)
    enc = A.encoder(r.t)
    src, dst = load(r, dev)
    rc, got = call(enc, src, dst, r)
    what = "%s repair queue %s" % (what, name)
    A.ok(rc, what)
    check(r, src, dst, got, what)
    return src, dst, got
