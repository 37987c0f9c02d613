"""Read queues for the gfrs_read_queue tests.

A queue is what the read side sees (datafile.go:410-434, stream_get.go:
382-465): the framed shard images of many blobs, each with its own length,
its own set of unreadable shards and the segment of the data shards a GET
wants.  Everything the GPU module (tests/test_gpu_read_queue.py) feeds to the
engine is generated here, so tests/test_read_queue_cpu.py can check the same
queues against the schedule builder and against the oracle alone.

Expectations come from the oracle only: data shards from A.ref_stripes,
parity from pyoracle.rs_encode / lrc_encode (inside ref_stripes), images from
pyoracle.crc32b_encode; the expected rows are the original data bytes of the
segment, the expected word is pyoracle.crc32 of every touched frame's payload
against its stored header.

Shard lengths (16-byte vectors, 4096-byte pieces, 16384-byte passes,
65532-byte frame payloads):
  1, 17                  ragged tail only / one vector + one byte
  4096, 16385            one piece; one byte into the second pass
  65531, 65532, 65533    one byte short of / exactly / one byte past a frame
  65597                  a trailing frame of 65 bytes
  131064, 131065         two exact frames; and a third of one byte
Segments per length (those that exist for it, duplicates dropped):
  the whole shard; (0, 1); (4, 1); (shard_len rounded down to 4, the rest);
  across a frame edge (65528, 8); starting on one (65532, min(5, rest));
  the last frame only.

The images of every shard named in a pattern, and of every parity that is
not an input, are filled with garbage: their CRCs are wrong and their payload
is not the shard's, so anything read from them shows in the word or the rows.
"""
import ctypes
import functools
import math

import numpy as np

import _arena as A
import _verdict as V
from _arena import L, Arena, oracle, vp

from cubefs_amd import runtime
from cubefs_amd.ec import _tactic_struct

LENS = [1, 17, 4096, 16385, 65531, 65532, 65533, 65597, 131064, 131065]
PAYLOAD = 65532
ROWS = 4
MAX_BUCKETS = 5
FUSED, IDENTITY, SLOW = 0, 1, 2
ERR_TOO_FEW, ERR_NO_DATA, ERR_INVALID, ERR_BLOCK, ERR_NOMEM, \
    ERR_UNSUPPORTED = -2, -4, -6, -10, -102, -103


def round4(n):
    return (n + 3) // 4 * 4


def segments(slen):
    """The segment list of the module docstring for one shard length."""
    segs = [(0, slen), (0, 1)]
    if slen > 4:
        segs.append((4, 1))
    down = slen // 4 * 4
    if slen > down:
        segs.append((down, slen - down))
    if slen > PAYLOAD:
        segs.append((65528, min(8, slen - 65528)))
        segs.append((PAYLOAD, min(5, slen - PAYLOAD)))
        last = (slen - 1) // PAYLOAD * PAYLOAD
        segs.append((last, slen - last))
    return list(dict.fromkeys(segs))


def cases(lens=LENS):
    """[(slen, seg_off, seg_len)], neighbours differing in length."""
    per = [[(s,) + seg for seg in segments(s)] for s in lens]
    out = []
    while any(per):
        for p in per:
            if p:
                out.append(p.pop(0))
    return out


def touched(seg_off, seg_len):
    return range(seg_off // PAYLOAD, (seg_off + seg_len - 1) // PAYLOAD + 1)


def inputs(t, bad):
    """First n present of the n+m global shards, index order."""
    return [i for i in range(t.N + t.M) if i not in bad][:t.N]


def classify(t, bad):
    """(class, R) of a pattern (include/gfrs.h, launch bound)."""
    r = len([b for b in bad if b < t.N])
    if t.N + t.M + t.L <= 16:
        return (FUSED if r <= ROWS else SLOW), r
    return (IDENTITY if r == 0 else SLOW), r


class GQueue:
    """jobs[j] = (img_off, img_stride, slen, seg_off, seg_len, out_off,
    out_stride, pattern); data[j] = the oracle's (total, slen) stripe of job j
    (read-only); flips = [(job, shard, image byte, mask)]."""

    def __init__(self, name, t, patterns, specs, delta=1, flips=()):
        self.name, self.t, self.patterns = name, t, patterns
        self.total = t.N + t.M + t.L
        self.delta = delta
        self.flips = list(flips)
        n = len(specs)
        need, seen = {}, {}
        for slen, _, _, _ in specs:
            need[slen] = need.get(slen, 0) + 1
        self.data = []
        for slen, _, _, _ in specs:
            ref = A.ref_stripes(t, need[slen], slen, seed=41)
            s = seen.get(slen, 0)
            seen[slen] = s + 1
            self.data.append(ref[s])
        # images: odd gaps between jobs, padded strides of any parity
        img, at = [], 0
        for j, (slen, _, _, _) in enumerate(specs):
            stride = A.enc_size(slen) + (j % 4) * 3
            img.append((at, stride))
            at += (self.total - 1) * stride + A.enc_size(slen) + 1 + 2 * (j % 5)
        self.img_bytes = img[-1][0] + (self.total - 1) * img[-1][1] + \
            A.enc_size(specs[-1][0])
        # rows: not in job order (odd jobs first, then the even ones
        # backwards); uneven 4-aligned padding; tight stride for odd jobs
        place = [None] * n
        at = end = 0
        order = [j for j in range(n) if j % 2] + \
            [j for j in range(n) if j % 2 == 0][::-1]
        for j in order:
            seg_len = specs[j][2]
            stride = round4(seg_len) + (0 if j % 2 else 4 * (1 + j % 3))
            place[j] = (at, stride)
            end = at + (t.N - 1) * stride + seg_len
            at = round4(end) + 4 * ((5 * j) % 4)
        self.out_bytes = end
        self.jobs = [img[j] + specs[j][:3] + place[j] + (specs[j][3],)
                     for j in range(n)]

    def bad_of(self, j):
        return self.patterns[self.jobs[j][7]]

    def inputs_of(self, j):
        return inputs(self.t, self.bad_of(j))

    def row_regions(self, j):
        """[(offset in out, size)] of job j's n rows."""
        _, _, _, _, seg_len, out_off, stride, _ = self.jobs[j]
        return [(out_off + i * stride, seg_len) for i in range(self.t.N)]


def _specs(lens, npat, step=1, start=0):
    """Jobs from cases(lens)[start::step]; patterns cycle so that the items of
    one bucket change descriptor from job to job."""
    cs = cases(lens)[start::step]
    mul = [m for m in (3, 2, 5, 1) if math.gcd(m, npat) == 1][0]
    return [c + ((mul * j) % npat,) for j, c in enumerate(cs)]


@functools.lru_cache(maxsize=None)
def build(name):
    if name == "rs63":
        # empty, data only (R = 1, 2, 3), parity only, mixed
        pats = [[], [1], [0, 5], [0, 2, 4], [7], [6, 8], [1, 8], [8, 3, 2]]
        return GQueue(name, V.get_tactic("EC6P3"), pats, _specs(LENS, 8))
    if name == "rs44":
        pats = [[], [3], [0, 1], [1, 2, 3], [0, 1, 2, 3], [4, 7], [2, 6, 0],
                [5, 0, 6, 3]]
        return GQueue(name, A.tactic(4, 4), pats, _specs(LENS, 8, 2))
    if name == "rs124":
        pats = [[], [1], [0, 13], [2, 5, 11, 15], [14, 12], [3, 7, 9, 10],
                [8, 4]]
        return GQueue(name, V.get_tactic("EC12P4"), pats,
                      _specs([1, 17, 4096, 16385, 65533, 131065], 7, 2, 1))
    if name == "lrc":
        # LRC12P2L2: 15 names a local parity (ignored); data via the globals
        pats = [[], [0], [15], [3, 15], [12], [0, 13], [5, 6], [14, 1, 15]]
        return GQueue(name, A.lrc_tactic(), pats,
                      _specs([17, 4096, 65532, 65597, 131064], 8, 2))
    if name == "rs66":
        # R <= 4 of RS(6+6): fused
        pats = [[], [2], [0, 5], [1, 2, 3, 4], [6, 11], [0, 7, 8, 3],
                [5, 4, 3, 6, 7, 8]]
        return GQueue(name, V.get_tactic("EC6P6"), pats,
                      _specs([1, 17, 4096, 16385, 65531, 65597, 131065], 7,
                             2, 1))
    if name == "rs66_slow":
        # R = 5 and 6: one job at a time; mixed with fused jobs
        pats = [[0, 1, 2, 3, 4], [5, 4, 3, 2, 1, 0], [1], [0, 2, 3, 4, 5, 9]]
        return GQueue(name, V.get_tactic("EC6P6"), pats,
                      _specs([1, 17, 4096, 65533, 131065], 4, 2))
    if name == "rs134_w17":
        # 17 shards: a copy-only pattern is IDENTITY, a rebuild SLOW
        pats = [[], [16], [0, 12], [14, 15], [3]]
        return GQueue(name, V.get_tactic("EC13P4"), pats,
                      _specs([1, 17, 4096, 65533, 131065], 5, 2, 1))
    if name == "seq_small":
        # a step of tests/test_gpu_sequences.py: one and two frames
        pats = [[], [1], [0, 5], [7]]
        return GQueue(name, V.get_tactic("EC6P3"), pats,
                      _specs([1000, 4093, 70001], 4))
    if name.startswith("corrupt_"):
        return _corrupt(name)
    raise KeyError(name)


CLEAN_QUEUES = ["rs63", "rs44", "rs124", "lrc", "rs66"]
SLOW_QUEUES = ["rs66_slow", "rs134_w17"]
CORRUPT_QUEUES = ["corrupt_rs63", "corrupt_rs66_slow", "corrupt_w17"]
GPU_QUEUES = CLEAN_QUEUES + SLOW_QUEUES + CORRUPT_QUEUES


def _corrupt(name):
    """One flipped bit per odd job; even jobs stay clean.  The kind of flip
    cycles: payload bytes of an input at the vector, pass and frame edges of
    the segment's first frame, a stored CRC header, a frame outside the
    segment, a non-input shard."""
    tname, pats, lens = {
        "corrupt_rs63": ("EC6P3", [[], [1], [0, 5], [7], [2, 8, 4]],
                         [17, 16385, 65533, 131065]),
        "corrupt_rs66_slow": ("EC6P6", [[0, 1, 2, 3, 4], [2],
                                        [5, 4, 3, 2, 1, 0]],
                              [17, 65533, 131065]),
        "corrupt_w17": ("EC13P4", [[], [3], [14]], [17, 65533, 131065]),
    }[name]
    t = V.get_tactic(tname)
    specs = _specs(lens, len(pats))
    q = GQueue(name, t, pats, specs)
    flips = []
    for j in range(1, len(specs), 2):
        slen, seg_off, seg_len, pat = specs[j]
        ins = inputs(t, pats[pat])
        fr = list(touched(seg_off, seg_len))
        nfr = (slen + PAYLOAD - 1) // PAYLOAD
        kind = ["payload", "header", "non-input", "outside", "payload",
                "payload"][(j // 2) % 6]
        sh = ins[(j // 2) % len(ins)]
        f = fr[(j // 4) % len(fr)]
        plen = min(PAYLOAD, slen - f * PAYLOAD)
        edges = [0, 15, 16, 4095, 4096, 16383, 16384, plen - 1,
                 plen // 16 * 16, plen // 16 * 16 - 1]
        edges = [e for e in edges if 0 <= e < plen]
        if kind == "outside" and len(fr) < nfr:  # a frame outside the segment
            f = [x for x in range(nfr) if x not in fr][0]
            byte = f * A.BLOCK + 4
        elif kind == "non-input":
            others = [i for i in range(q.total) if i not in ins]
            sh = others[(j // 2) % len(others)]
            byte = f * A.BLOCK + 4
        elif kind == "header":               # a stored CRC header
            byte = f * A.BLOCK + (j // 2) % 4
        else:                                # a payload byte of an input
            byte = f * A.BLOCK + 4 + edges[(j // 2 + j // 12) % len(edges)]
        flips.append((j, sh, byte, 1 << (j % 8)))
    q.flips = flips
    return q


# ---- the images and the oracle's answers -----------------------------------

def _garbage(size, seed):
    return np.random.default_rng(0x6A5B ^ seed).integers(0, 256, size,
                                                         dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def images(name):
    """Per job: the total images as they lie in framed - oracle framing for
    the inputs and the unnamed data shards, garbage for every shard named in
    the pattern and every non-input parity - with the queue's flips applied."""
    q = build(name)
    out = []
    for j, job in enumerate(q.jobs):
        slen = job[2]
        bad, ins = q.bad_of(j), q.inputs_of(j)
        imgs = []
        for i in range(q.total):
            if i in bad or (i >= q.t.N and i not in ins):
                imgs.append(_garbage(A.enc_size(slen), 1000 * j + i))
            else:
                imgs.append(oracle.crc32b_encode(q.data[j][i].copy()))
        out.append(imgs)
    for j, sh, byte, mask in q.flips:
        out[j][sh][byte] ^= mask
    return out


@functools.lru_cache(maxsize=None)
def words(name):
    """Per job: bit i set when input i has a touched frame whose stored header
    differs from pyoracle.crc32 of its payload."""
    q = build(name)
    imgs = images(name)
    out = []
    for j, job in enumerate(q.jobs):
        slen, seg_off, seg_len = job[2:5]
        w = 0
        for i in q.inputs_of(j):
            img = imgs[j][i]
            for f in touched(seg_off, seg_len):
                plen = min(PAYLOAD, slen - f * PAYLOAD)
                at = f * A.BLOCK
                stored = int.from_bytes(img[at:at + 4].tobytes(), "little")
                if oracle.crc32(img[at + 4:at + 4 + plen].copy()) != stored:
                    w |= 1 << i
        out.append(w)
    return out


# ---- C ABI arguments --------------------------------------------------------

def gjob_array(jobs):
    """jobs: (img_off, img_stride, slen, seg_off, seg_len, out_off,
    out_stride, pattern[, reserved])."""
    arr = (runtime.GJob * max(1, len(jobs)))()
    for j, job in enumerate(jobs):
        arr[j] = runtime.GJob(*job[:8], job[8] if len(job) > 8 else 0)
    return arr


def pattern_arrays(patterns):
    flat = [i for p in patterns for i in p]
    offs = [0]
    for p in patterns:
        offs.append(offs[-1] + len(p))
    return A.i32s(flat or [0]), A.i32s(offs)


# ---- schedule (GPU-free export) ---------------------------------------------

class Schedule:
    pass


def schedule(t, jobs, patterns, block_len=A.BLOCK, item_cap=None,
             bad_off=None, njobs=None, npat=None):
    """gfrs_compute_read_queue_schedule -> (rc, Schedule or None)."""
    nj = len(jobs)
    if item_cap is None:
        item_cap = nj * max(1, t.N)
    items = (runtime.GItem * max(1, item_cap))()
    prefix = (ctypes.c_uint64 * (max(1, item_cap) + MAX_BUCKETS))()
    buckets = (runtime.GBucket * MAX_BUCKETS)()
    ni, nb, ns = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    np_ = len(patterns)
    pcls = (ctypes.c_int32 * max(1, np_))()
    pr = (ctypes.c_int32 * max(1, np_))()
    slow = (ctypes.c_int32 * max(1, nj))()
    bad, boff = pattern_arrays(patterns)
    if bad_off is not None:
        boff = A.i32s(bad_off)
    ts = _tactic_struct(t)
    rc = L().gfrs_compute_read_queue_schedule(
        ctypes.byref(ts), gjob_array(jobs), nj if njobs is None else njobs,
        bad, boff, np_ if npat is None else npat, block_len, item_cap, items,
        prefix, ctypes.byref(ni), buckets, ctypes.byref(nb), pcls, pr, slow,
        ctypes.byref(ns))
    if rc != 0:
        return rc, None
    s = Schedule()
    s.items = [(i.job, i.desc, i.img, i.img_stride, i.shard_len, i.seg_off,
                i.seg_len, i.out, i.out_stride) for i in items[:ni.value]]
    s.buckets = [(b.r, b.first, b.count) for b in buckets[:nb.value]]
    s.prefix = list(prefix[:ni.value + nb.value])
    s.pat_class = list(pcls[:np_])
    s.pat_r = list(pr[:np_])
    s.slow_jobs = list(slow[:ns.value])
    return 0, s


# ---- GPU runner: one call, both arenas checked ------------------------------

def load(q, dev, seed=70):
    """(image arena, row arena), both uploaded."""
    src = Arena(dev, q.img_bytes, q.delta, seed=seed)
    for j, job in enumerate(q.jobs):
        for i, img in enumerate(images(q.name)[j]):
            src.put(job[0] + i * job[1], img)
    src.upload()
    dst = Arena(dev, q.out_bytes, 4, seed=seed + 1)
    dst.upload()
    return src, dst


def call(enc, src, dst, q, jobs=None, patterns=None, block_len=A.BLOCK,
         njobs=None, npat=None, dst_shift=0, bad_off=None):
    """-> (rc, words list)."""
    jobs = q.jobs if jobs is None else jobs
    patterns = q.patterns if patterns is None else patterns
    bad, boff = pattern_arrays(patterns)
    if bad_off is not None:
        boff = A.i32s(bad_off)
    w = (ctypes.c_uint32 * max(1, len(jobs)))(*([0xDEAD] * max(1, len(jobs))))
    rc = L().gfrs_read_queue(
        enc._ctx, vp(dst.ptr + dst_shift), vp(src.ptr), gjob_array(jobs),
        len(jobs) if njobs is None else njobs, bad, boff,
        len(patterns) if npat is None else npat, block_len, w)
    return rc, list(w[:len(jobs)])


def check(q, src, dst, got_words, what=""):
    """Words equal the oracle's; out: the segment of the original data in
    every row of every job whose oracle word is 0 - the rows of the others
    are unspecified - and not one other byte changed; framed unchanged."""
    want_words = words(q.name)
    assert got_words == want_words, (
        what, [(j, hex(g), hex(w)) for j, (g, w) in
               enumerate(zip(got_words, want_words)) if g != w])
    want = dst.expect()
    unspec = []
    for j, job in enumerate(q.jobs):
        seg_off, seg_len = job[3:5]
        if want_words[j]:
            unspec += q.row_regions(j)
            continue
        for i, (off, size) in enumerate(q.row_regions(j)):
            dst.put(off, q.data[j][i][seg_off:seg_off + seg_len], want)
    dst.check(want, unspec, what=what + " rows")
    src.check(src.expect(), what=what + " framed")


def run(dev, name, what=""):
    q = build(name)
    enc = A.encoder(q.t)
    src, dst = load(q, dev)
    what = "%s read queue %s" % (what, name)
    rc, w = call(enc, src, dst, q)
    A.ok(rc, what)
    check(q, src, dst, w, what)
    return src, dst
