"""Shared helpers for the layout / instantiation / grid-stride GPU tests.

Arena: a flat uint8 device buffer (lead guard | payload | trail guard)
filled with seeded random bytes.  A test writes its inputs into the host
image, uploads, calls the C ABI directly (runtime.lib(), so stride and
base offset are free parameters), then builds the expected arena from the
pre-call host copy by overwriting ONLY the regions the ABI declares as
output.  check() compares the whole arena, so every byte that is not a
declared output (guards, inter-stripe / inter-image padding, all inputs)
must come back bit-identical.  Regions the ABI leaves unspecified are
masked explicitly.
"""
import ctypes
import functools

import numpy as np
import torch

from cubefs_amd import codemode, ec, runtime
from oracle import pyoracle as oracle

GUARD = 512
BLOCK = 65536
ERR_UNSUPPORTED = -103


class Arena:
    def __init__(self, dev, nbytes, delta=0, seed=0, guard=GUARD):
        self.off = guard + delta
        self.nbytes = nbytes
        rng = np.random.default_rng(0xA7E4A ^ (seed * 7919 + nbytes))
        self.host = rng.integers(0, 256, guard + delta + nbytes + guard,
                                 dtype=np.uint8)
        self.dev = torch.empty(self.host.size, dtype=torch.uint8, device=dev)
        # torch device allocations are 512-B aligned, so the payload sits
        # at exactly `delta` modulo 512
        assert self.dev.data_ptr() % 512 == 0
        self.ptr = self.dev.data_ptr() + self.off

    def put(self, off, data, arr=None):
        """Write `data` at payload offset `off` (host image by default)."""
        arr = self.host if arr is None else arr
        data = np.asarray(data, dtype=np.uint8).reshape(-1)
        assert 0 <= off and off + data.size <= self.nbytes
        arr[self.off + off:self.off + off + data.size] = data

    def upload(self):
        self.dev.copy_(torch.from_numpy(self.host))
        torch.cuda.synchronize()

    def expect(self):
        """Copy of the pre-call arena; overwrite declared outputs in it."""
        return self.host.copy()

    def check(self, want, unspecified=(), what=""):
        """Whole-arena bit comparison; `unspecified` = [(payload_off, n)]."""
        torch.cuda.synchronize()
        got = self.dev.cpu().numpy()
        if unspecified:
            got = got.copy()
            want = want.copy()
            for off, n in unspecified:
                got[self.off + off:self.off + off + n] = 0
                want[self.off + off:self.off + off + n] = 0
        if np.array_equal(got, want):
            return
        bad = np.flatnonzero(got != want)
        first = int(bad[0]) - self.off
        raise AssertionError(
            "%s: %d bytes differ, first at payload offset %d (payload %d "
            "bytes; negative / beyond = guard), got %d want %d" %
            (what, bad.size, first, self.nbytes, got[bad[0]], want[bad[0]]))


class Stripes:
    """ec.Buffer batch layout with free stripe_stride padding."""

    def __init__(self, ns, total, slen, pad=0):
        self.ns, self.total, self.slen = ns, total, slen
        self.stride = total * slen + pad
        self.nbytes = (ns - 1) * self.stride + total * slen

    def off(self, s, i):
        return s * self.stride + i * self.slen


class Rows:
    """nrows images of row_len bytes at a 4-aligned stride."""

    def __init__(self, nrows, row_len, extra=0):
        self.nrows, self.row_len = nrows, row_len
        self.stride = (row_len + 3) // 4 * 4 + extra
        self.nbytes = (nrows - 1) * self.stride + row_len

    def off(self, r):
        return r * self.stride


# ---- tactics -------------------------------------------------------------

def tactic(n, m):
    """Plain RS(n+m) tactic through codemode.extend (idempotent)."""
    table = {(4, 2): (241, "EC4P2", 5),      # same definition as
                                             # test_gpu_parity.py
             (4, 1): (242, "EC4P1", 4),
             (4, 3): (243, "EC4P3", 6),
             (4, 4): (244, "EC4P4", 7),
             (15, 1): (245, "EC15P1", 15),
             (12, 4): (246, "EC12P4W", 15),
             (13, 4): (247, "EC13P4", 16)}
    code, name, quorum = table[(n, m)]
    codemode.extend(code, name, codemode.Tactic(n, m, 0, 1, quorum, 0, 2048))
    return codemode.get_tactic(name)


def lrc_tactic():
    codemode.extend(240, "LRC12P2L2",
                    codemode.Tactic(12, 2, 2, 2, 14, 0, 2048))
    return codemode.get_tactic("LRC12P2L2")


_ENCODERS = {}


def encoder(t):
    key = (t.N, t.M, t.L, t.AZCount)
    if key not in _ENCODERS:
        _ENCODERS[key] = ec.Encoder(t)
    return _ENCODERS[key]


# ---- oracle references (computed once, shared, never mutated) -------------

@functools.lru_cache(maxsize=None)
def _ref(n, m, l, az, ns, slen, seed):
    rng = np.random.default_rng(0x5EED ^ (seed * 104729 + slen * 31 + n))
    arr = rng.integers(0, 256, (ns, n + m + l, slen), dtype=np.uint8)
    for s in range(ns):
        sh = [arr[s, i].copy() for i in range(n + m + l)]
        if l:
            oracle.lrc_encode(n, m, l, az, sh)
        else:
            oracle.rs_encode(n, m, sh)
        for i in range(n, n + m + l):
            arr[s, i] = sh[i]
    arr.setflags(write=False)
    return arr


def ref_stripes(t, ns, slen, seed=0):
    """(ns, total, slen) oracle-encoded stripes; read-only."""
    return _ref(t.N, t.M, t.L, t.AZCount, ns, slen, seed)


def enc_size(slen):
    return oracle.crc32b_encode_size(slen, BLOCK)


def disk_size(slen):
    return oracle.shard_disk_size(slen, BLOCK)


# ---- ctypes glue -----------------------------------------------------------

def L():
    return runtime.lib()


def vp(x):
    return ctypes.c_void_p(x)


def i32s(v):
    return (ctypes.c_int32 * len(v))(*v)


def u64s(v):
    return (ctypes.c_uint64 * len(v))(*v)


def bitmap(ns):
    return (ctypes.c_uint64 * ((ns + 63) // 64))()


def bits(bm, ns):
    return [s for s in range(ns) if (bm[s // 64] >> (s % 64)) & 1]


def ok(rc, what):
    assert rc == 0, (what, rc, L().gfrs_last_error())


def sync(enc):
    ok(L().gfrs_synchronize(enc._ctx), "synchronize")


def load_stripes(a, lay, ref, skip=()):
    """Place every shard of `ref` except `skip` into arena `a` (host)."""
    for s in range(lay.ns):
        for i in range(lay.total):
            if i not in skip:
                a.put(lay.off(s, i), ref[s, i])


# ---- one-call runners: each does call + whole-arena check ------------------

def run_rs_apply(dev, t, ref, pad=0, delta=0, bad=(1, 7), what=""):
    """encode_batch, verify_batch (one corrupt stripe) and
    reconstruct_verify_batch on one layout, arena-checked."""
    enc = encoder(t)
    ns, total, slen = ref.shape
    lay = Stripes(ns, total, slen, pad)
    a = Arena(dev, lay.nbytes, delta, seed=5)
    load_stripes(a, lay, ref, skip=range(t.N, total))
    a.upload()
    ok(L().gfrs_encode_batch(enc._ctx, vp(a.ptr), slen, lay.stride, ns),
       what + " encode_batch")
    sync(enc)
    want = a.expect()
    for s in range(ns):
        for i in range(t.N, total):
            a.put(lay.off(s, i), ref[s, i], want)
    a.check(want, what=what + " encode_batch")

    hit = ns - 2
    a = Arena(dev, lay.nbytes, delta, seed=6)
    load_stripes(a, lay, ref)
    a.host[a.off + lay.off(hit, t.N) + slen - 1] ^= 0x40
    a.upload()
    bm = bitmap(ns)
    ok(L().gfrs_verify_batch(enc._ctx, vp(a.ptr), slen, lay.stride, ns, bm),
       what + " verify_batch")
    assert bits(bm, ns) == [hit], (what, bits(bm, ns))
    a.check(a.expect(), what=what + " verify_batch")

    bad = list(bad)
    a = Arena(dev, lay.nbytes, delta, seed=7)
    load_stripes(a, lay, ref, skip=bad)
    a.upload()
    bm = bitmap(ns)
    ok(L().gfrs_reconstruct_verify_batch(enc._ctx, vp(a.ptr), slen,
                                         lay.stride, ns, i32s(bad), len(bad),
                                         bm), what + " reconstruct_verify")
    sync(enc)
    assert bits(bm, ns) == [], (what, bits(bm, ns))
    want = a.expect()
    for s in range(ns):
        for i in bad:
            a.put(lay.off(s, i), ref[s, i], want)
    a.check(want, what=what + " reconstruct_verify")

    a = Arena(dev, lay.nbytes, delta, seed=8)
    load_stripes(a, lay, ref, skip=bad)
    a.upload()
    ok(L().gfrs_reconstruct_batch(enc._ctx, vp(a.ptr), slen, lay.stride, ns,
                                  i32s(bad), len(bad), 0),
       what + " reconstruct_batch")
    sync(enc)
    a.check(want_like(a, lay, ref, bad), what=what + " reconstruct_batch")


def want_like(a, lay, ref, filled):
    want = a.expect()
    for s in range(lay.ns):
        for i in filled:
            a.put(lay.off(s, i), ref[s, i], want)
    return want


@functools.lru_cache(maxsize=None)
def _raw(nsh, slen, seed):
    rng = np.random.default_rng(0xC4C ^ (seed * 977 + slen))
    arr = rng.integers(0, 256, (nsh, slen), dtype=np.uint8)
    arr.setflags(write=False)
    return arr


def run_crc(dev, enc, slen, nsh, pad=0, delta=0, extra=0, what=""):
    """crc32b encode_batch, verify_batch (one bad shard) and a
    single-shard decode, arena-checked against the oracle framing."""
    raw = _raw(nsh, slen, 1)
    frames = [oracle.crc32b_encode(raw[j].copy()) for j in range(nsh)]
    fl = enc_size(slen)
    srows = Stripes(nsh, 1, slen, pad)
    src = Arena(dev, srows.nbytes, delta, seed=20)
    for j in range(nsh):
        src.put(srows.off(j, 0), raw[j])
    src.upload()
    rows = Rows(nsh, fl, extra)
    dst = Arena(dev, rows.nbytes, 4 if extra else 0, seed=21)
    dst.upload()
    ok(L().gfrs_crc32b_encode_batch(enc._ctx, vp(dst.ptr), rows.stride,
                                    vp(src.ptr), srows.stride, slen, BLOCK,
                                    nsh), what + " crc encode")
    sync(enc)
    want = dst.expect()
    for j in range(nsh):
        dst.put(rows.off(j), frames[j], want)
    dst.check(want, what=what + " crc encode")
    src.check(src.expect(), what=what + " crc encode source")

    # verify: the framed images are now the (possibly misaligned) source
    frows = Stripes(nsh, 1, fl, pad)
    a = Arena(dev, frows.nbytes, delta, seed=22)
    for j in range(nsh):
        a.put(frows.off(j, 0), frames[j])
    hit = nsh - 2
    a.host[a.off + frows.off(hit, 0) + fl - 1] ^= 1  # last payload byte
    a.upload()
    badb = (ctypes.c_int64 * nsh)()
    ok(L().gfrs_crc32b_verify_batch(enc._ctx, vp(a.ptr), frows.stride, fl,
                                    BLOCK, nsh, badb), what + " crc verify")
    assert list(badb) == [(fl - 1) // BLOCK if j == hit else -1
                          for j in range(nsh)], (what, list(badb))
    a.check(a.expect(), what=what + " crc verify")

    # decode shard 0 (clean) out of the same arena, then the bad shard
    out = Arena(dev, slen, 0, seed=23)
    out.upload()
    n = L().gfrs_crc32b_decode(enc._ctx, vp(out.ptr), vp(a.ptr), fl, BLOCK)
    assert n == slen, (what, n)
    want = out.expect()
    out.put(0, raw[0], want)
    out.check(want, what=what + " crc decode")
    n = L().gfrs_crc32b_decode(enc._ctx, vp(out.ptr),
                               vp(a.ptr + frows.off(hit, 0)), fl, BLOCK)
    assert n == -9, (what, n)
    a.check(a.expect(), what=what + " crc decode source")


def run_shard_images(dev, enc, slen, nsh, pad=0, delta=0, extra=0, what=""):
    """shard_write_batch then shard_parse_batch (one corrupt image)."""
    raw = _raw(nsh, slen, 3)
    bids = [(1 << 40) | j for j in range(nsh)]
    vuids = [0xABCDEF00 + j for j in range(nsh)]
    imgs = [oracle.shard_write(raw[j].copy(), bid=bids[j], vuid=vuids[j])
            for j in range(nsh)]
    dl = disk_size(slen)
    srows = Stripes(nsh, 1, slen, pad)
    src = Arena(dev, srows.nbytes, delta, seed=24)
    for j in range(nsh):
        src.put(srows.off(j, 0), raw[j])
    src.upload()
    rows = Rows(nsh, dl, extra)
    dst = Arena(dev, rows.nbytes, 4 if extra else 0, seed=25)
    dst.upload()
    ok(L().gfrs_shard_write_batch(enc._ctx, vp(dst.ptr), rows.stride,
                                  vp(src.ptr), srows.stride, slen, BLOCK,
                                  u64s(bids), u64s(vuids), nsh),
       what + " shard write")
    sync(enc)
    want = dst.expect()
    for j in range(nsh):
        dst.put(rows.off(j), imgs[j], want)
    dst.check(want, what=what + " shard write")
    src.check(src.expect(), what=what + " shard write source")

    irows = Stripes(nsh, 1, dl, pad)
    a = Arena(dev, irows.nbytes, delta, seed=26)
    for j in range(nsh):
        a.put(irows.off(j, 0), imgs[j])
    hit = nsh - 3
    fl = enc_size(slen)
    a.host[a.off + irows.off(hit, 0) + 32 + fl - 1] ^= 0x80  # last body byte
    a.upload()
    meta = (ctypes.c_uint64 * (4 * nsh))()
    badb = (ctypes.c_int64 * nsh)()
    ok(L().gfrs_shard_parse_batch(enc._ctx, vp(a.ptr), irows.stride, slen,
                                  BLOCK, meta, badb, nsh),
       what + " shard parse")
    for j in range(nsh):
        assert (meta[4 * j], meta[4 * j + 1], meta[4 * j + 2]) == \
            (bids[j], vuids[j], slen), (what, j)
        err = ctypes.c_int64(meta[4 * j + 3]).value
        assert err == (-9 if j == hit else 0), (what, j, err)
        assert badb[j] == ((fl - 1) // BLOCK if j == hit else -1), (what, j)
    a.check(a.expect(), what=what + " shard parse")


def run_sized(dev, enc, n, what=""):
    """rpc2 sized coder: encode, verify (clean + corrupt), decode."""
    raw = _raw(1, n, 9)[0]
    want_f, tail = oracle.sized_encode(raw.copy())
    src = Arena(dev, n, 3, seed=27)
    src.put(0, raw)
    src.upload()
    dst = Arena(dev, want_f.size, 0, seed=28)
    dst.upload()
    w = L().gfrs_sized_encode(enc._ctx, vp(dst.ptr), vp(src.ptr), n, BLOCK)
    assert w == want_f.size, (what, w)
    want = dst.expect()
    dst.put(0, want_f, want)
    dst.check(want, what=what + " sized encode")
    src.check(src.expect(), what=what + " sized encode source")
    badb = ctypes.c_int64(7)
    ok(L().gfrs_sized_verify(enc._ctx, vp(dst.ptr), want_f.size, tail, BLOCK,
                             ctypes.byref(badb)), what + " sized verify")
    assert badb.value == -1, (what, badb.value)
    out = Arena(dev, n, 0, seed=29)
    out.upload()
    w = L().gfrs_sized_decode(enc._ctx, vp(out.ptr), vp(dst.ptr),
                              want_f.size, tail, BLOCK)
    assert w == n, (what, w)
    want = out.expect()
    out.put(0, raw, want)
    out.check(want, what=what + " sized decode")
    # corrupt the last payload byte of the last frame
    last = want_f.size - tail - 5
    dst.host[:] = dst.dev.cpu().numpy()
    dst.host[dst.off + last] ^= 1
    dst.upload()
    ok(L().gfrs_sized_verify(enc._ctx, vp(dst.ptr), want_f.size, tail, BLOCK,
                             ctypes.byref(badb)), what + " sized verify")
    assert badb.value == last // BLOCK, (what, badb.value)


def run_encode_frame(dev, t, ref, pad=0, delta=0, extra=0, what="",
                     composed=False):
    """gfrs_encode_frame_batch on a padded/offset source arena; every image
    row equals the oracle framing, source + all padding untouched.
    composed=True: the shape takes the documented encode_batch +
    crc32b_encode_batch composition, which also materialises the parity in
    `base`."""
    enc = encoder(t)
    ns, total, slen = ref.shape
    lay = Stripes(ns, total, slen, pad)
    src = Arena(dev, lay.nbytes, delta, seed=1)
    # parity regions of the source stay random: the fused path must not
    # read or write them
    load_stripes(src, lay, ref, skip=range(t.N, total))
    src.upload()
    rows = Rows(ns * total, enc_size(slen), extra)
    dst = Arena(dev, rows.nbytes, 4 if extra else 0, seed=2)
    dst.upload()
    rc = L().gfrs_encode_frame_batch(enc._ctx, vp(dst.ptr), rows.stride,
                                     vp(src.ptr), slen, lay.stride, ns, BLOCK)
    ok(rc, what)
    sync(enc)
    want = dst.expect()
    for s in range(ns):
        for i in range(total):
            dst.put(rows.off(s * total + i),
                    oracle.crc32b_encode(ref[s, i].copy()), want)
    dst.check(want, what=what + " images")
    src.check(want_like(src, lay, ref, range(t.N, total) if composed else ()),
              what=what + " source")


def run_repair(dev, t, ref, bad, pad=0, delta=0, extra=0, corrupt=None,
               what=""):
    """gfrs_repair_batch: images equal oracle.shard_write of the original
    shards in the caller's column order; `base` untouched outside the bad
    shards' regions.  corrupt = (stripe, shard, byte, mask) is applied to
    a surviving shard; returns the failed-stripe list."""
    enc = encoder(t)
    ns, total, slen = ref.shape
    nb = len(bad)
    lay = Stripes(ns, total, slen, pad)
    src = Arena(dev, lay.nbytes, delta, seed=3)
    load_stripes(src, lay, ref, skip=bad)
    if corrupt:
        s, i, b, mask = corrupt
        src.host[src.off + lay.off(s, i) + b] ^= mask
    src.upload()
    rows = Rows(ns * nb, disk_size(slen), extra)
    dst = Arena(dev, rows.nbytes, 4 if extra else 0, seed=4)
    dst.upload()
    bids = [7000 + j for j in range(ns * nb)]
    vuids = [0x1122334455 + j for j in range(ns * nb)]
    bm = bitmap(ns)
    rc = L().gfrs_repair_batch(enc._ctx, vp(src.ptr), slen, lay.stride, ns,
                               i32s(bad), nb, vp(dst.ptr), rows.stride,
                               BLOCK, u64s(bids), u64s(vuids), bm)
    ok(rc, what)
    sync(enc)
    fails = bits(bm, ns)
    want = dst.expect()
    for s in range(ns):
        if s in fails:
            # failed stripes' images are written but their content is not
            # defined by the (corrupt) inputs
            continue
        for b, idx in enumerate(bad):
            j = s * nb + b
            dst.put(rows.off(j), oracle.shard_write(ref[s, idx].copy(),
                                                    bid=bids[j],
                                                    vuid=vuids[j]), want)
    unspec = [(rows.off(s * nb + b), rows.row_len)
              for s in fails for b in range(nb)]
    dst.check(want, unspec, what=what + " images")
    src.check(src.expect(),
              [(lay.off(s, i), slen) for s in range(ns) for i in bad],
              what=what + " base")
    return fails
