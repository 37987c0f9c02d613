"""Shard read queues for the gfrs_shard_read_queue tests.

A queue is what a reader of one chunk file sees (datainspect.go:197-283,
shards_decoder.go:48-295, datafile.go:410-445): disk images of many sizes
back to back, and per job the meta's bid, vuid and size, a range of the raw
shard and whether the bytes are wanted at all.  Everything the GPU module
(tests/test_gpu_shard_read_queue.py) feeds to the engine is generated here, so
tests/test_shard_read_queue_cpu.py can check the same queues against the
schedule builder and against the oracle alone.

Expectations come from the oracle only: images from pyoracle.shard_write, the
expected bytes are the original payload slice (with the flipped bits of a
corrupted job, which are the image's payload bytes), the expected status,
bad_block and crc from pyoracle.crc32 over the image bytes as they are after
the flips.

Sizes are those of _readq.LENS, ranges per size those of _readq.segments (the
whole shard; (0, 1); (4, 1); the sub-dword tail; across a frame edge; starting
on one; the last frame only), each issued with and without NO_OUT, the whole
shard also with FOOTER.  Images lie at odd addresses with garbage between
them; outputs are 4-aligned with guarded gaps, in another order than the jobs.
"""
import ctypes
import functools

import numpy as np

import _arena as A
import _readq as G
from _arena import L, Arena, oracle, vp

from cubefs_amd import runtime

LENS = G.LENS
PAYLOAD = G.PAYLOAD
BLOCK = A.BLOCK
NO_OUT, FOOTER = runtime.SJOB_NO_OUT, runtime.SJOB_FOOTER
HDR_MAGIC, HDR_CRC, HDR_MISMATCH, BODY_CRC, FTR_MAGIC, FTR_CRC = \
    1, 2, 4, 8, 16, 32
ERR_NO_DATA, ERR_INVALID, ERR_BLOCK, ERR_NOMEM, ERR_UNSUPPORTED = \
    -4, -6, -10, -102, -103
DEAD = 0xDEADBEEF


def touched(frm, to):
    return range(frm // PAYLOAD, (to - 1) // PAYLOAD + 1)


def ids(k):
    """bid and vuid of image k: all eight bytes of both in use."""
    return (0x0102030405060708 + 0x1111 * k) & (2 ** 64 - 1), \
        (0xF1E2D3C4B5A69788 - 0x0101 * k) & (2 ** 64 - 1)


@functools.lru_cache(maxsize=None)
def raw(size, seed=0):
    arr = np.random.default_rng(0x5A4D ^ (seed * 7919 + size)).integers(
        0, 256, size, dtype=np.uint8)
    arr.setflags(write=False)
    return arr


class SQueue:
    """images[k] = (offset in chunk, size, bid, vuid, raw, image bytes after
    the flips); jobs[j] = (img_off, size, bid, vuid, from, to, out_off,
    flags); image_of[j] = k; flips = [(image, byte relative to the image
    start - may lie in the gap behind it -, mask)]."""

    def __init__(self, name, sizes, specs, flips=()):
        """sizes: raw size per image; specs: (image, from, to, flags[, bid
        delta, vuid delta]) per job."""
        self.name = name
        self.flips = list(flips)
        self.images, at = [], 0
        gaps = []
        for k, size in enumerate(sizes):
            bid, vuid = ids(k)
            r = raw(size, k)
            img = oracle.shard_write(r.copy(), bid=bid, vuid=vuid)
            assert img.size == A.disk_size(size)
            self.images.append([at, size, bid, vuid, r, img])
            gap = 2 + 2 * (k % 3) + img.size % 2    # every image at an even
            gaps.append(gap)                        # offset of an odd base
            at += img.size + gap
        self.chunk_bytes = at
        self.gap_flips = []
        for k, byte, mask in self.flips:
            img = self.images[k][5]
            if byte < img.size:
                img[byte] ^= mask
            else:
                assert byte - img.size < gaps[k]
                self.gap_flips.append((self.images[k][0] + byte, mask))
        n = len(specs)
        self.image_of = [s[0] for s in specs]
        # rows: odd jobs first, then the even ones backwards; uneven guarded
        # gaps; a NO_OUT job has no row and a misaligned out_off
        place = [None] * n
        at = 0
        order = [j for j in range(n) if j % 2] + \
            [j for j in range(n) if j % 2 == 0][::-1]
        self.out_bytes = 4
        for j in order:
            _, frm, to, flags = specs[j][:4]
            if flags & NO_OUT:
                place[j] = 3 + 8 * j
                continue
            place[j] = at
            self.out_bytes = at + (to - frm)
            at = G.round4(at + to - frm) + 4 * (1 + (5 * j) % 4)
        self.jobs = []
        for j, s in enumerate(specs):
            k, frm, to, flags = s[:4]
            off, size, bid, vuid = self.images[k][:4]
            db, dv = (s[4], s[5]) if len(s) > 4 else (0, 0)
            self.jobs.append((off, size, bid ^ db, vuid ^ dv, frm, to,
                              place[j], flags))

    def flipped_images(self):
        return {k for k, _, _ in self.flips}


def _range_specs(k, size):
    """The jobs of one image: every range with and without NO_OUT, the whole
    shard also with FOOTER."""
    out = []
    for off, n in G.segments(size):
        out.append((k, off, off + n, 0))
        out.append((k, off, off + n, NO_OUT))
        if (off, n) == (0, size):
            out.append((k, 0, size, FOOTER))
            out.append((k, 0, size, FOOTER | NO_OUT))
    return out


def _interleave(per):
    per = [list(p) for p in per]
    out = []
    while any(per):
        for p in per:
            if p:
                out.append(p.pop(0))
    return out


# flip sites of one image, relative to its start
def _sites(size, frm, to):
    """[(kind, [(byte, mask)])] for one (size, range): what a test may flip,
    one kind per job."""
    fr = list(touched(frm, to))
    nfr = (size - 1) // PAYLOAD + 1
    whole = (frm, to) == (0, size)
    f = fr[-1]
    plen = min(PAYLOAD, size - f * PAYLOAD)
    body = 32 + f * BLOCK
    ftr = 32 + A.enc_size(size)
    edges = [0, 15, 16, 4095, 4096, 16383, 16384, plen - 1, plen // 16 * 16,
             plen // 16 * 16 - 1]
    edges = sorted({e for e in edges if 0 <= e < plen})
    if not whole:
        edges = [edges[0], edges[-1]]
    out = [("fcrc", [(body + (size + f) % 4, 0x10)])]
    out += [("payload", [(body + 4 + e, 1 << (e % 8))]) for e in edges]
    if len(fr) < nfr:
        o = [x for x in range(nfr) if x not in fr][0]
        out.append(("outside", [(32 + o * BLOCK + 4, 0x02)]))
        out.append(("outside", [(32 + o * BLOCK, 0x02)]))
    if len(fr) > 1:                 # two bad frames: the lowest is reported
        out.append(("payload", [(32 + fr[-1] * BLOCK + 4, 1),
                                (32 + fr[0] * BLOCK + 4 + 4097, 0x80)]))
    out.append(("gap", [(A.disk_size(size) + 1, 0xFF)]))
    hdr = [("hdr_crc", 1), ("hdr_magic", 6), ("hdr_bid", 8 + size % 8),
           ("hdr_vuid", 16 + size % 7), ("hdr_size", 27), ("hdr_reserved", 30)]
    out += [(kind, [(byte, 0x40)]) for kind, byte in
            (hdr if whole else hdr[:2])]
    out += [("want_bid", []), ("want_vuid", [])] if whole else []
    # the footer is looked at by FOOTER jobs only (_plain: without the flag)
    foot = [("ftr_magic", [(ftr + 2, 0x08)]), ("ftr_crc", [(ftr + 5, 0x20)])]
    out += foot if whole else []
    out += [(kind + "_plain", fl) for kind, fl in foot]
    return out


FLIP_LENS = [17, 16385, 65533, 131065]


def _flip_queue(name):
    sizes, specs, flips, kinds = [], [], [], []
    for size in FLIP_LENS:
        ranges = [(0, size), (0, 1)]
        if size > PAYLOAD:
            last = (size - 1) // PAYLOAD * PAYLOAD
            ranges += [(last, size), (65528, min(size, 65536))]
        for frm, to in ranges:
            for kind, fl in _sites(size, frm, to):
                k = len(sizes)
                sizes.append(size)
                flags = [0, NO_OUT, FOOTER, FOOTER | NO_OUT][k % 4]
                if (frm, to) != (0, size):
                    flags &= NO_OUT
                if kind.endswith("_plain"):
                    flags &= NO_OUT
                elif kind.startswith("ftr"):
                    flags |= FOOTER
                db = 1 << (k % 64) if kind == "want_bid" else 0
                dv = 1 << ((3 * k) % 64) if kind == "want_vuid" else 0
                specs.append((k, frm, to, flags, db, dv))
                flips += [(k, byte, mask) for byte, mask in fl]
                kinds.append(kind)
    q = SQueue(name, sizes, specs, flips)
    q.kinds = kinds
    return q


@functools.lru_cache(maxsize=None)
def build(name):
    if name == "clean":
        per = [_range_specs(k, s) for k, s in enumerate(LENS)]
        return SQueue(name, LENS, _interleave(per))
    if name == "all_no_out":
        per = [[s for s in _range_specs(k, sz) if s[3] & NO_OUT]
               for k, sz in enumerate([17, 65533, 131065])]
        return SQueue(name, [17, 65533, 131065], _interleave(per))
    if name == "none_no_out":
        per = [[s for s in _range_specs(k, sz) if not s[3] & NO_OUT]
               for k, sz in enumerate([1, 4096, 65597, 131064])]
        return SQueue(name, [1, 4096, 65597, 131064], _interleave(per))
    if name == "one":
        return SQueue(name, [65533], [(0, 0, 65533, FOOTER)])
    if name == "tiny":
        # four frames per bucket: with three workgroups the last one is idle
        sizes = [131065, 17]
        return SQueue(name, sizes, [(0, 0, 131065, FOOTER), (1, 0, 17, 0),
                                    (0, 0, 131065, FOOTER | NO_OUT),
                                    (1, 0, 17, FOOTER | NO_OUT)])
    if name == "flips":
        return _flip_queue(name)
    raise KeyError(name)


CLEAN_QUEUES = ["clean", "all_no_out", "none_no_out", "one", "tiny"]
GPU_QUEUES = CLEAN_QUEUES + ["flips"]


# ---- the oracle's answers ----------------------------------------------------

def be(b):
    return int.from_bytes(b.tobytes(), "big")


def payload_of(img, size):
    """The image's payload bytes as they are: header, frame CRCs and footer
    stripped by the job's size."""
    parts = []
    for f in range((size - 1) // PAYLOAD + 1):
        plen = min(PAYLOAD, size - f * PAYLOAD)
        at = 32 + f * BLOCK + 4
        parts.append(img[at:at + plen])
    return np.concatenate(parts)


def expect_one(img, job):
    """dict(status, crc, bad_block, bid, vuid, size) of one job over the
    bytes of its image, by pyoracle.crc32 alone."""
    _, size, bid, vuid, frm, to, _, flags = job
    st = 0
    if img[4:8].tobytes() != b"\xab\xcd\xef\xcc":
        st |= HDR_MAGIC
    if be(img[0:4]) != oracle.crc32(img[4:32].copy()):
        st |= HDR_CRC
    got = (be(img[8:16]), be(img[16:24]), be(img[24:28]))
    if got != (bid, vuid, size):
        st |= HDR_MISMATCH
    bad = -1
    for f in touched(frm, to):
        plen = min(PAYLOAD, size - f * PAYLOAD)
        at = 32 + f * BLOCK
        stored = int.from_bytes(img[at:at + 4].tobytes(), "little")
        if oracle.crc32(img[at + 4:at + 4 + plen].copy()) != stored:
            st |= BODY_CRC
            bad = f if bad < 0 else bad
    crc = 0
    if flags & FOOTER:
        crc = oracle.crc32(payload_of(img, size).copy())
        ftr = img[32 + A.enc_size(size):]
        if ftr[0:4].tobytes() != b"\xcc\xef\xcd\xab":
            st |= FTR_MAGIC
        if be(ftr[4:8]) != crc:
            st |= FTR_CRC
    return dict(status=st, crc=crc, bad_block=bad, bid=got[0], vuid=got[1],
                size=got[2])


@functools.lru_cache(maxsize=None)
def expected(name):
    q = build(name)
    return [expect_one(q.images[k][5], job)
            for k, job in zip(q.image_of, q.jobs)]


def want_bytes(q, j):
    """Bytes [from, to) a storing job receives."""
    k = q.image_of[j]
    _, size, _, _, frm, to, _, _ = q.jobs[j]
    if k not in q.flipped_images():
        return q.images[k][4][frm:to]
    return payload_of(q.images[k][5], size)[frm:to]


# ---- C ABI arguments ------------------------------------------------------------

def sjob_array(jobs):
    """jobs: (img_off, size, bid, vuid, from, to, out_off, flags[,
    reserved])."""
    arr = (runtime.SJob * max(1, len(jobs)))()
    for j, job in enumerate(jobs):
        arr[j] = runtime.SJob(*job[:8], job[8] if len(job) > 8 else 0)
    return arr


class Schedule:
    pass


def schedule(jobs, block_len=BLOCK, item_cap=None, njobs=None):
    """gfrs_compute_shard_read_queue_schedule -> (rc, Schedule or None)."""
    nj = len(jobs)
    if item_cap is None:
        item_cap = nj
    items = (runtime.SItem * max(1, item_cap))()
    prefix = (ctypes.c_uint64 * (max(1, item_cap) + 2))()
    buckets = (runtime.SBucket * 2)()
    ni, nb, tot = ctypes.c_int(), ctypes.c_int(), ctypes.c_uint64()
    rc = L().gfrs_compute_shard_read_queue_schedule(
        sjob_array(jobs), nj if njobs is None else njobs, block_len, item_cap,
        items, prefix, ctypes.byref(ni), buckets, ctypes.byref(nb),
        ctypes.byref(tot))
    if rc != 0:
        return rc, None
    s = Schedule()
    s.items = [(i.job, i.img, i.size, i.from_, i.to, i.out, i.flags)
               for i in items[:ni.value]]
    s.buckets = [(b.no_out, b.first, b.count) for b in buckets[:nb.value]]
    s.prefix = list(prefix[:ni.value + nb.value])
    s.total_frames = tot.value
    return 0, s


# ---- GPU runner: one call, both arenas checked --------------------------------

def load(q, dev, seed=90):
    """(chunk arena, out arena), both uploaded."""
    src = Arena(dev, q.chunk_bytes, 1, seed=seed)
    for off, _, _, _, _, img in q.images:
        src.put(off, img)
    for off, mask in q.gap_flips:
        src.host[src.off + off] ^= mask
    src.upload()
    dst = Arena(dev, q.out_bytes, 4, seed=seed + 1)
    dst.upload()
    return src, dst


def fresh_results(n):
    res = (runtime.SResult * max(1, n))()
    for r in res:
        r.status, r.crc, r.bad_block = DEAD, DEAD, -DEAD
        r.bid = r.vuid = r.size = DEAD
    return res


def as_dicts(res, n):
    return [dict(status=r.status, crc=r.crc, bad_block=r.bad_block,
                 bid=r.bid, vuid=r.vuid, size=r.size) for r in res[:n]]


def call(enc, src, dst, q, jobs=None, block_len=BLOCK, njobs=None,
         dst_shift=0, null_out=False):
    """-> (rc, list of result dicts)."""
    jobs = q.jobs if jobs is None else jobs
    res = fresh_results(len(jobs))
    rc = L().gfrs_shard_read_queue(
        enc._ctx, None if null_out else vp(dst.ptr + dst_shift), vp(src.ptr),
        sjob_array(jobs), len(jobs) if njobs is None else njobs, block_len,
        res)
    return rc, as_dicts(res, len(jobs))


def check(q, src, dst, got, what=""):
    """Every result field equals the oracle's; out: the range of every
    storing job and not one other byte; chunk unchanged."""
    want = expected(q.name)
    assert len(got) == len(want)
    for j, (g, w) in enumerate(zip(got, want)):
        assert g == w, (what, j, q.jobs[j], getattr(q, "kinds", None) and
                        q.kinds[q.image_of[j]], g, w)
    img = dst.expect()
    for j, job in enumerate(q.jobs):
        if not job[7] & NO_OUT:
            dst.put(job[6], want_bytes(q, j), img)
    dst.check(img, what=what + " out")
    src.check(src.expect(), what=what + " chunk")


def run(dev, name, what=""):
    q = build(name)
    enc = A.encoder(A.tactic(4, 2))
    src, dst = load(q, dev)
    what = "%s shard read queue %s" % (what, name)
    rc, got = call(enc, src, dst, q)
    A.ok(rc, what)
    check(q, src, dst, got, what)
    return src, dst
