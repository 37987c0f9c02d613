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

Every call is a Step with three phases - prepare, issue, check - so that
tests/_sequence.py can issue several calls back to back before it checks
any of them; the run_* helpers are compositions of steps run one at a time.
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

    def read(self):
        return self.dev.cpu().numpy()

    def expect(self):
        """Copy of the pre-call arena; overwrite declared outputs in it."""
        return self.host.copy()

    def check(self, want, unspecified=(), what=""):
        """Whole-arena bit comparison; `unspecified` = [(payload_off, n)]."""
        torch.cuda.synchronize()
        got = self.read()
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


class HostArena(Arena):
    """The same guarded image in host memory, for GFRS_MEM_HOST calls:
    upload() takes the live copy the call works on, ptr points into it and
    check() compares it."""

    def __init__(self, dev, nbytes, delta=0, seed=0, guard=GUARD):
        self.off = guard + delta
        self.nbytes = nbytes
        rng = np.random.default_rng(0xA7E4A ^ (seed * 7919 + nbytes))
        self.host = rng.integers(0, 256, guard + delta + nbytes + guard,
                                 dtype=np.uint8)
        self.live = self.ptr = None

    def upload(self):
        self.live = self.host.copy()
        self.ptr = self.live.ctypes.data + self.off

    def read(self):
        return self.live


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


# ---- three-phase steps -------------------------------------------------------

class Step:
    """One ABI call in three phases, so that a test can put other calls
    between the issue of a call and its check (tests/_sequence.py):

      prepare(dev)  host image, oracle expectation, upload, every ctypes
                    argument; builds fresh arenas each time it is called
      issue(enc)    the ABI call only: no gfrs_synchronize, no torch sync;
                    return code and host outputs are kept, not looked at
      check(enc)    gfrs_synchronize, then every assertion: return code,
                    host outputs, whole-arena comparison

    blocking: the call synchronizes the context's stream before it returns
    (False: it returns with its work queued)."""
    blocking = True
    what = ""

    def run(self, dev, enc):
        self.prepare(dev)
        self.issue(enc)
        self.check(enc)
        return self


class _StripeStep(Step):
    """A strided batch of oracle stripes in one arena."""

    def __init__(self, t, ref, pad=0, delta=0, seed=0, what=""):
        self.t, self.ref, self.what = t, ref, what
        self.ns, self.total, self.slen = ref.shape
        self.lay = Stripes(self.ns, self.total, self.slen, pad)
        self.delta, self.seed = delta, seed

    def arena(self, dev, skip=()):
        a = Arena(dev, self.lay.nbytes, self.delta, seed=self.seed)
        load_stripes(a, self.lay, self.ref, skip=skip)
        return a


class EncodeBatch(_StripeStep):
    blocking = False

    def __init__(self, t, ref, pad=0, delta=0, seed=5, what=""):
        super().__init__(t, ref, pad, delta, seed, what + " encode_batch")

    def prepare(self, dev):
        par = range(self.t.N, self.total)
        self.a = self.arena(dev, skip=par)
        self.a.upload()
        self.want = want_like(self.a, self.lay, self.ref, par)

    def issue(self, enc):
        self.rc = L().gfrs_encode_batch(enc._ctx, vp(self.a.ptr), self.slen,
                                        self.lay.stride, self.ns)

    def check(self, enc):
        ok(self.rc, self.what)
        sync(enc)
        self.a.check(self.want, what=self.what)


class VerifyBatch(_StripeStep):
    """One bit flipped in the last byte of the first parity of stripe
    `hit`; that stripe and no other is reported."""

    def __init__(self, t, ref, pad=0, delta=0, hit=None, seed=6, what=""):
        super().__init__(t, ref, pad, delta, seed, what + " verify_batch")
        self.hit = self.ns - 2 if hit is None else hit

    def prepare(self, dev):
        a = self.a = self.arena(dev)
        a.host[a.off + self.lay.off(self.hit, self.t.N) + self.slen - 1] \
            ^= 0x40
        a.upload()
        self.bm = bitmap(self.ns)

    def issue(self, enc):
        self.rc = L().gfrs_verify_batch(enc._ctx, vp(self.a.ptr), self.slen,
                                        self.lay.stride, self.ns, self.bm)

    def check(self, enc):
        ok(self.rc, self.what)
        sync(enc)
        assert bits(self.bm, self.ns) == [self.hit], \
            (self.what, bits(self.bm, self.ns))
        self.a.check(self.a.expect(), what=self.what)


class ReconstructVerifyBatch(_StripeStep):
    def __init__(self, t, ref, bad=(1, 7), pad=0, delta=0, seed=7, what=""):
        super().__init__(t, ref, pad, delta, seed,
                         what + " reconstruct_verify")
        self.bad = list(bad)

    def prepare(self, dev):
        self.a = self.arena(dev, skip=self.bad)
        self.a.upload()
        self.bm = bitmap(self.ns)
        self.badv = i32s(self.bad)
        self.want = want_like(self.a, self.lay, self.ref, self.bad)

    def issue(self, enc):
        self.rc = L().gfrs_reconstruct_verify_batch(
            enc._ctx, vp(self.a.ptr), self.slen, self.lay.stride, self.ns,
            self.badv, len(self.bad), self.bm)

    def check(self, enc):
        ok(self.rc, self.what)
        sync(enc)
        assert bits(self.bm, self.ns) == [], \
            (self.what, bits(self.bm, self.ns))
        self.a.check(self.want, what=self.what)


class ReconstructBatch(_StripeStep):
    blocking = False

    def __init__(self, t, ref, bad=(1, 7), pad=0, delta=0, seed=8, what=""):
        super().__init__(t, ref, pad, delta, seed,
                         what + " reconstruct_batch")
        self.bad = list(bad)

    def prepare(self, dev):
        self.a = self.arena(dev, skip=self.bad)
        self.a.upload()
        self.badv = i32s(self.bad)
        self.want = want_like(self.a, self.lay, self.ref, self.bad)

    def issue(self, enc):
        self.rc = L().gfrs_reconstruct_batch(
            enc._ctx, vp(self.a.ptr), self.slen, self.lay.stride, self.ns,
            self.badv, len(self.bad), 0)

    def check(self, enc):
        ok(self.rc, self.what)
        sync(enc)
        self.a.check(self.want, what=self.what)


def run_rs_apply(dev, t, ref, pad=0, delta=0, bad=(1, 7), what=""):
    """encode_batch, verify_batch (one corrupt stripe),
    reconstruct_verify_batch and reconstruct_batch on one layout,
    arena-checked."""
    enc = encoder(t)
    for step in (EncodeBatch(t, ref, pad, delta, what=what),
                 VerifyBatch(t, ref, pad, delta, what=what),
                 ReconstructVerifyBatch(t, ref, bad, pad, delta, what=what),
                 ReconstructBatch(t, ref, bad, pad, delta, what=what)):
        step.run(dev, enc)


# ---- crc32block, shard images, sized coder -----------------------------------

class _RowStep(Step):
    """nsh raw shards (source stride padded by `pad`, base at `delta`) and
    their images as rows (stride padded by `extra`)."""

    def __init__(self, slen, nsh, pad=0, delta=0, extra=0, seed=0, raw_seed=1,
                 what=""):
        self.slen, self.nsh, self.what = slen, nsh, what
        self.pad, self.delta, self.extra, self.seed = pad, delta, extra, seed
        self.raw = _raw(nsh, slen, raw_seed)

    def source(self, dev, rows, seed):
        """The arena holding `rows` (a list of equal-length images) as a
        padded one-shard-per-stripe batch."""
        lay = Stripes(len(rows), 1, rows[0].size, self.pad)
        a = Arena(dev, lay.nbytes, self.delta, seed=seed)
        for j, r in enumerate(rows):
            a.put(lay.off(j, 0), r)
        return a, lay

    def dest(self, dev, row_len, seed):
        rows = Rows(self.nsh, row_len, self.extra)
        dst = Arena(dev, rows.nbytes, 4 if self.extra else 0, seed=seed)
        dst.upload()
        return dst, rows


class CrcEncodeBatch(_RowStep):
    blocking = False

    def __init__(self, slen, nsh, pad=0, delta=0, extra=0, seed=20, what=""):
        super().__init__(slen, nsh, pad, delta, extra, seed, 1,
                         what + " crc encode")

    def prepare(self, dev):
        self.src, self.srows = self.source(dev, list(self.raw), self.seed)
        self.src.upload()
        self.dst, self.rows = self.dest(dev, enc_size(self.slen),
                                        self.seed + 1)
        self.want = self.dst.expect()
        for j in range(self.nsh):
            self.dst.put(self.rows.off(j),
                         oracle.crc32b_encode(self.raw[j].copy()), self.want)

    def issue(self, enc):
        self.rc = L().gfrs_crc32b_encode_batch(
            enc._ctx, vp(self.dst.ptr), self.rows.stride, vp(self.src.ptr),
            self.srows.stride, self.slen, BLOCK, self.nsh)

    def check(self, enc):
        ok(self.rc, self.what)
        sync(enc)
        self.dst.check(self.want, what=self.what)
        self.src.check(self.src.expect(), what=self.what + " source")


class CrcVerifyBatch(_RowStep):
    """The framed images as the (possibly misaligned) source; the last
    payload byte of image `hit` is flipped."""

    def __init__(self, slen, nsh, pad=0, delta=0, hit=None, seed=22, what=""):
        super().__init__(slen, nsh, pad, delta, 0, seed, 1,
                         what + " crc verify")
        self.hit = nsh - 2 if hit is None else hit
        self.fl = enc_size(slen)

    def prepare(self, dev):
        frames = [oracle.crc32b_encode(self.raw[j].copy())
                  for j in range(self.nsh)]
        a, self.frows = self.source(dev, frames, self.seed)
        a.host[a.off + self.frows.off(self.hit, 0) + self.fl - 1] ^= 1
        a.upload()
        self.a = a
        self.badb = (ctypes.c_int64 * self.nsh)()

    def issue(self, enc):
        self.rc = L().gfrs_crc32b_verify_batch(
            enc._ctx, vp(self.a.ptr), self.frows.stride, self.fl, BLOCK,
            self.nsh, self.badb)

    def check(self, enc):
        ok(self.rc, self.what)
        sync(enc)
        assert list(self.badb) == [(self.fl - 1) // BLOCK if j == self.hit
                                   else -1 for j in range(self.nsh)], \
            (self.what, list(self.badb))
        self.a.check(self.a.expect(), what=self.what)


class CrcDecode(Step):
    """Decode image j out of a prepared CrcVerifyBatch's arena: the raw
    shard for a clean image, GFRS_ERR_MISMATCHED_CRC (and an unspecified
    destination) for the flipped one; the source stays untouched."""

    def __init__(self, images, j, seed=23, what=""):
        self.images, self.j, self.seed = images, j, seed
        self.what = what + " crc decode"

    def prepare(self, dev):
        v = self.images
        self.out = Arena(dev, v.slen, 0, seed=self.seed)
        self.out.upload()
        self.src = v.a.ptr + v.frows.off(self.j, 0)

    def issue(self, enc):
        v = self.images
        self.n = L().gfrs_crc32b_decode(enc._ctx, vp(self.out.ptr),
                                        vp(self.src), v.fl, BLOCK)

    def check(self, enc):
        v = self.images
        sync(enc)
        if self.j == v.hit:
            assert self.n == -9, (self.what, self.n)
        else:
            assert self.n == v.slen, (self.what, self.n)
            want = self.out.expect()
            self.out.put(0, v.raw[self.j], want)
            self.out.check(want, what=self.what)
        v.a.check(v.a.expect(), what=self.what + " source")


def run_crc(dev, enc, slen, nsh, pad=0, delta=0, extra=0, what=""):
    """crc32b encode_batch, verify_batch (one bad shard) and two
    single-shard decodes (clean, bad), arena-checked against the oracle
    framing."""
    CrcEncodeBatch(slen, nsh, pad, delta, extra, what=what).run(dev, enc)
    v = CrcVerifyBatch(slen, nsh, pad, delta, what=what).run(dev, enc)
    CrcDecode(v, 0, what=what).run(dev, enc)
    CrcDecode(v, v.hit, what=what).run(dev, enc)


def shard_ids(nsh, k=0):
    """Distinct bids and vuids; k selects another set."""
    return ([(1 << 40) | (j + 1000 * k) for j in range(nsh)],
            [0xABCDEF00 + j + 4096 * k for j in range(nsh)])


class ShardWriteBatch(_RowStep):
    blocking = False

    def __init__(self, slen, nsh, pad=0, delta=0, extra=0, ids=0, seed=24,
                 what=""):
        super().__init__(slen, nsh, pad, delta, extra, seed, 3,
                         what + " shard write")
        self.bids, self.vuids = shard_ids(nsh, ids)

    def prepare(self, dev):
        self.src, self.srows = self.source(dev, list(self.raw), self.seed)
        self.src.upload()
        self.dst, self.rows = self.dest(dev, disk_size(self.slen),
                                        self.seed + 1)
        self.want = self.dst.expect()
        for j in range(self.nsh):
            self.dst.put(self.rows.off(j),
                         oracle.shard_write(self.raw[j].copy(),
                                            bid=self.bids[j],
                                            vuid=self.vuids[j]), self.want)
        self.args = (u64s(self.bids), u64s(self.vuids))

    def issue(self, enc):
        self.rc = L().gfrs_shard_write_batch(
            enc._ctx, vp(self.dst.ptr), self.rows.stride, vp(self.src.ptr),
            self.srows.stride, self.slen, BLOCK, self.args[0], self.args[1],
            self.nsh)

    def check(self, enc):
        ok(self.rc, self.what)
        sync(enc)
        self.dst.check(self.want, what=self.what)
        self.src.check(self.src.expect(), what=self.what + " source")


class ShardParseBatch(_RowStep):
    """The oracle's images as the source; the last body byte of image
    `hit` is flipped."""

    def __init__(self, slen, nsh, pad=0, delta=0, hit=None, seed=26, what=""):
        super().__init__(slen, nsh, pad, delta, 0, seed, 3,
                         what + " shard parse")
        self.bids, self.vuids = shard_ids(nsh)
        self.hit = nsh - 3 if hit is None else hit
        self.fl = enc_size(slen)

    def prepare(self, dev):
        imgs = [oracle.shard_write(self.raw[j].copy(), bid=self.bids[j],
                                   vuid=self.vuids[j])
                for j in range(self.nsh)]
        a, self.irows = self.source(dev, imgs, self.seed)
        a.host[a.off + self.irows.off(self.hit, 0) + 32 + self.fl - 1] ^= 0x80
        a.upload()
        self.a = a
        self.meta = (ctypes.c_uint64 * (4 * self.nsh))()
        self.badb = (ctypes.c_int64 * self.nsh)()

    def issue(self, enc):
        self.rc = L().gfrs_shard_parse_batch(
            enc._ctx, vp(self.a.ptr), self.irows.stride, self.slen, BLOCK,
            self.meta, self.badb, self.nsh)

    def check(self, enc):
        ok(self.rc, self.what)
        sync(enc)
        meta, what = self.meta, self.what
        for j in range(self.nsh):
            assert (meta[4 * j], meta[4 * j + 1], meta[4 * j + 2]) == \
                (self.bids[j], self.vuids[j], self.slen), (what, j)
            err = ctypes.c_int64(meta[4 * j + 3]).value
            assert err == (-9 if j == self.hit else 0), (what, j, err)
            assert self.badb[j] == ((self.fl - 1) // BLOCK if j == self.hit
                                    else -1), (what, j)
        self.a.check(self.a.expect(), what=what)


def run_shard_images(dev, enc, slen, nsh, pad=0, delta=0, extra=0, what=""):
    """shard_write_batch then shard_parse_batch (one corrupt image)."""
    ShardWriteBatch(slen, nsh, pad, delta, extra, what=what).run(dev, enc)
    ShardParseBatch(slen, nsh, pad, delta, what=what).run(dev, enc)


class _SizedStep(Step):
    def __init__(self, n, what=""):
        self.n, self.what = n, what
        self.raw = _raw(1, n, 9)[0]
        self.framed, self.tail = oracle.sized_encode(self.raw.copy())

    def image(self, dev, flip=None):
        """The oracle's framed body in an arena of its own."""
        a = Arena(dev, self.framed.size, 0, seed=28)
        a.put(0, self.framed)
        if flip is not None:
            a.host[a.off + flip] ^= 1
        a.upload()
        return a


class SizedEncode(_SizedStep):
    def prepare(self, dev):
        self.src = Arena(dev, self.n, 3, seed=27)
        self.src.put(0, self.raw)
        self.src.upload()
        self.dst = Arena(dev, self.framed.size, 0, seed=28)
        self.dst.upload()

    def issue(self, enc):
        self.w = L().gfrs_sized_encode(enc._ctx, vp(self.dst.ptr),
                                       vp(self.src.ptr), self.n, BLOCK)

    def check(self, enc):
        sync(enc)
        assert self.w == self.framed.size, (self.what, self.w)
        want = self.dst.expect()
        self.dst.put(0, self.framed, want)
        self.dst.check(want, what=self.what + " sized encode")
        self.src.check(self.src.expect(),
                       what=self.what + " sized encode source")


class SizedVerify(_SizedStep):
    """corrupt=True flips the last payload byte of the last frame."""

    def __init__(self, n, corrupt=False, what=""):
        super().__init__(n, what)
        self.last = self.framed.size - self.tail - 5 if corrupt else None

    def prepare(self, dev):
        self.a = self.image(dev, self.last)
        self.badb = ctypes.c_int64(7)

    def issue(self, enc):
        self.rc = L().gfrs_sized_verify(enc._ctx, vp(self.a.ptr),
                                        self.framed.size, self.tail, BLOCK,
                                        ctypes.byref(self.badb))

    def check(self, enc):
        ok(self.rc, self.what + " sized verify")
        sync(enc)
        want = -1 if self.last is None else self.last // BLOCK
        assert self.badb.value == want, (self.what, self.badb.value)
        self.a.check(self.a.expect(), what=self.what + " sized verify")


class SizedDecode(_SizedStep):
    def prepare(self, dev):
        self.a = self.image(dev)
        self.out = Arena(dev, self.n, 0, seed=29)
        self.out.upload()

    def issue(self, enc):
        self.w = L().gfrs_sized_decode(enc._ctx, vp(self.out.ptr),
                                       vp(self.a.ptr), self.framed.size,
                                       self.tail, BLOCK)

    def check(self, enc):
        sync(enc)
        assert self.w == self.n, (self.what, self.w)
        want = self.out.expect()
        self.out.put(0, self.raw, want)
        self.out.check(want, what=self.what + " sized decode")
        self.a.check(self.a.expect(), what=self.what + " sized decode source")


def run_sized(dev, enc, n, what=""):
    """rpc2 sized coder: encode, verify (clean + corrupt), decode."""
    for step in (SizedEncode(n, what), SizedVerify(n, what=what),
                 SizedDecode(n, what), SizedVerify(n, True, what)):
        step.run(dev, enc)


# ---- fused encode+frame, repair ------------------------------------------------

class EncodeFrameBatch(_StripeStep):
    """gfrs_encode_frame_batch on a padded/offset source arena; every image
    row equals the oracle framing, source + all padding untouched.
    composed=True: the shape takes the documented encode_batch +
    crc32b_encode_batch composition, which also materialises the parity in
    `base`."""
    blocking = False

    def __init__(self, t, ref, pad=0, delta=0, extra=0, composed=False,
                 what=""):
        super().__init__(t, ref, pad, delta, 1, what)
        self.extra, self.composed = extra, composed

    def prepare(self, dev):
        par = range(self.t.N, self.total)
        # parity regions of the source stay random: the fused path must not
        # read or write them
        self.src = self.arena(dev, skip=par)
        self.src.upload()
        self.rows = rows = Rows(self.ns * self.total, enc_size(self.slen),
                                self.extra)
        self.dst = Arena(dev, rows.nbytes, 4 if self.extra else 0, seed=2)
        self.dst.upload()
        self.want = self.dst.expect()
        for s in range(self.ns):
            for i in range(self.total):
                self.dst.put(rows.off(s * self.total + i),
                             oracle.crc32b_encode(self.ref[s, i].copy()),
                             self.want)
        self.want_src = want_like(self.src, self.lay, self.ref,
                                  par if self.composed else ())

    def issue(self, enc):
        self.rc = L().gfrs_encode_frame_batch(
            enc._ctx, vp(self.dst.ptr), self.rows.stride, vp(self.src.ptr),
            self.slen, self.lay.stride, self.ns, BLOCK)

    def check(self, enc):
        ok(self.rc, self.what)
        sync(enc)
        self.dst.check(self.want, what=self.what + " images")
        self.src.check(self.want_src, what=self.what + " source")


def run_encode_frame(dev, t, ref, pad=0, delta=0, extra=0, what="",
                     composed=False):
    EncodeFrameBatch(t, ref, pad, delta, extra, composed, what).run(
        dev, encoder(t))


class RepairBatch(_StripeStep):
    """gfrs_repair_batch: images equal oracle.shard_write of the original
    shards in the caller's column order; `base` untouched outside the bad
    shards' regions.  corrupt = (stripe, shard, byte, mask) is applied to
    a surviving shard; fails = the failed-stripe list after check().
    Both paths synchronize for the fail words; the legacy path (m + l > 4)
    then still queues one shard_write_batch per lost column and returns
    with the last one's work queued."""

    def __init__(self, t, ref, bad, pad=0, delta=0, extra=0, corrupt=None,
                 what=""):
        super().__init__(t, ref, pad, delta, 3, what)
        self.bad, self.extra, self.corrupt = list(bad), extra, corrupt

    def prepare(self, dev):
        nb = len(self.bad)
        src = self.src = self.arena(dev, skip=self.bad)
        if self.corrupt:
            s, i, b, mask = self.corrupt
            src.host[src.off + self.lay.off(s, i) + b] ^= mask
        src.upload()
        self.rows = Rows(self.ns * nb, disk_size(self.slen), self.extra)
        self.dst = Arena(dev, self.rows.nbytes, 4 if self.extra else 0,
                         seed=4)
        self.dst.upload()
        self.bids = [7000 + j for j in range(self.ns * nb)]
        self.vuids = [0x1122334455 + j for j in range(self.ns * nb)]
        self.args = (i32s(self.bad), u64s(self.bids), u64s(self.vuids))
        self.bm = bitmap(self.ns)

    def issue(self, enc):
        self.rc = L().gfrs_repair_batch(
            enc._ctx, vp(self.src.ptr), self.slen, self.lay.stride, self.ns,
            self.args[0], len(self.bad), vp(self.dst.ptr), self.rows.stride,
            BLOCK, self.args[1], self.args[2], self.bm)

    def check(self, enc):
        ok(self.rc, self.what)
        sync(enc)
        nb, rows = len(self.bad), self.rows
        fails = self.fails = bits(self.bm, self.ns)
        want = self.dst.expect()
        for s in range(self.ns):
            if s in fails:
                # failed stripes' images are written but their content is
                # not defined by the (corrupt) inputs
                continue
            for b, idx in enumerate(self.bad):
                j = s * nb + b
                self.dst.put(rows.off(j),
                             oracle.shard_write(self.ref[s, idx].copy(),
                                                bid=self.bids[j],
                                                vuid=self.vuids[j]), want)
        unspec = [(rows.off(s * nb + b), rows.row_len)
                  for s in fails for b in range(nb)]
        self.dst.check(want, unspec, what=self.what + " images")
        self.src.check(self.src.expect(),
                       [(self.lay.off(s, i), self.slen)
                        for s in range(self.ns) for i in self.bad],
                       what=self.what + " base")


def run_repair(dev, t, ref, bad, pad=0, delta=0, extra=0, corrupt=None,
               what=""):
    """One RepairBatch step; returns the failed-stripe list."""
    return RepairBatch(t, ref, bad, pad, delta, extra, corrupt, what).run(
        dev, encoder(t)).fails


# ---- single-stripe calls: pointer tables and GFRS_MEM_HOST ---------------------

MEM_DEVICE, MEM_HOST = runtime.MEM_DEVICE, runtime.MEM_HOST


class _PtrStep(Step):
    """All shards of stripe 0 of `ref` as views at odd, non-contiguous
    offsets of one arena - device memory and a pointer table, or, with
    host=True, host memory and GFRS_MEM_HOST (the engine stages the
    stripe).

    gap: distance between shard starts (default slen + 3; gap = slen is the
    contiguous ec.Buffer layout, still at an odd base address).
    members: global shard indices presented as an nshards = len(members)
    call, e.g. one local stripe of an LRC tactic; every shard index of the
    step (skip, bad, flipped shard) is then a position in that list, and
    total, the call's shard count, is its length."""

    def __init__(self, t, ref, host=False, seed=30, what="", gap=None,
                 members=None):
        self.t, self.ref, self.host, self.seed = t, ref, host, seed
        self.slen = ref.shape[2]
        self.members = list(range(t.total) if members is None else members)
        self.total = len(self.members)
        self.rows = ref[0, self.members]
        self.gap = self.slen + 3 if gap is None else gap
        self.memloc = MEM_HOST if host else MEM_DEVICE
        self.what = "%s%s" % (what, " (host)" if host else "")

    def arena(self, dev, skip=(), extra_shards=0):
        gap = self.gap
        n = self.total + extra_shards
        a = (HostArena if self.host else Arena)(dev, n * gap, 1,
                                                seed=self.seed)
        self.offs = [i * gap for i in range(n)]
        for i in range(self.total):
            if i not in skip:
                a.put(self.offs[i], self.rows[i])
        return a

    def table(self, idx):
        return (ctypes.c_void_p * len(idx))(*[self.a.ptr + self.offs[i]
                                              for i in idx])

    def filled(self, shards, src=None):
        want = self.a.expect()
        for i in shards:
            self.a.put(self.offs[i],
                       (self.rows if src is None else src)[i], want)
        return want


class Encode(_PtrStep):
    def prepare(self, dev):
        par = range(self.t.N, self.total)
        self.a = self.arena(dev, skip=par)
        self.a.upload()
        self.ptrs = self.table(range(self.total))
        self.want = self.filled(par)

    def issue(self, enc):
        self.rc = L().gfrs_encode(enc._ctx, self.ptrs, self.slen, self.total,
                                  self.memloc)

    def check(self, enc):
        ok(self.rc, self.what + " gfrs_encode")
        sync(enc)
        self.a.check(self.want, what=self.what + " gfrs_encode")


class Verify(_PtrStep):
    """flip=True: one bit in byte `byte` (default: the last) of shard
    `shard` (default: data shard 3)."""

    def __init__(self, t, ref, host=False, flip=False, seed=31, what="",
                 shard=3, byte=None, **kw):
        super().__init__(t, ref, host, seed, what, **kw)
        self.flip, self.shard = flip, shard
        self.byte = self.slen - 1 if byte is None else byte

    def prepare(self, dev):
        a = self.a = self.arena(dev)
        if self.flip:
            assert 0 <= self.byte < self.slen
            a.host[a.off + self.offs[self.shard] + self.byte] ^= 2
        a.upload()
        self.ptrs = self.table(range(self.total))
        self.okv = ctypes.c_int(-1)

    def issue(self, enc):
        self.rc = L().gfrs_verify(enc._ctx, self.ptrs, self.slen, self.total,
                                  self.memloc, ctypes.byref(self.okv))

    def check(self, enc):
        ok(self.rc, self.what + " gfrs_verify")
        sync(enc)
        assert self.okv.value == (0 if self.flip else 1), \
            (self.what, self.okv.value)
        self.a.check(self.a.expect(), what=self.what + " gfrs_verify")


class Reconstruct(_PtrStep):
    """`bad` is in the call's own index space: positions in `members` for a
    local-stripe step.  The erased shards keep the arena's random fill, so a
    shard the call must not rebuild (data_only) has to come back as it was."""

    def __init__(self, t, ref, host=False, bad=(8, 0), data_only=0, seed=32,
                 what="", **kw):
        super().__init__(t, ref, host, seed, what, **kw)
        self.bad, self.data_only = list(bad), data_only

    def prepare(self, dev):
        self.a = self.arena(dev, skip=self.bad)
        self.a.upload()
        self.ptrs = self.table(range(self.total))
        self.badv = i32s(self.bad)
        self.want = self.filled([i for i in self.bad
                                 if not self.data_only or i < self.t.N])

    def issue(self, enc):
        self.rc = L().gfrs_reconstruct(enc._ctx, self.ptrs, self.slen,
                                       self.total, self.memloc, self.badv,
                                       len(self.bad), self.data_only)

    def check(self, enc):
        what = "%s gfrs_reconstruct data_only=%d" % (self.what,
                                                      self.data_only)
        ok(self.rc, what)
        sync(enc)
        self.a.check(self.want, what=what)


class EncodeIdx(Step):
    """gfrs_encode_idx of every data shard in `idxs` into zeroed parity, for
    each stripe of `ref` in turn: call k accumulates into another stripe's
    parity buffers than call k - 1, so len(ref) accumulations run
    interleaved.  The parity of a stripe ends as the oracle's encode of its
    data with every shard outside `idxs` taken as zero (all of them: the
    oracle's parity)."""

    def __init__(self, t, ref, idxs=None, seed=33, what=""):
        self.t, self.ref, self.seed = t, ref, seed
        self.ns, self.total, self.slen = ref.shape
        self.idxs = list(range(t.N) if idxs is None else idxs)
        self.what = what + " gfrs_encode_idx"

    def prepare(self, dev):
        t, gap = self.t, self.slen + 3
        a = self.a = Arena(dev, self.ns * self.total * gap, 1, seed=self.seed)
        want_par = []
        for s in range(self.ns):
            sh = [self.ref[s, i].copy() if i in self.idxs
                  else np.zeros(self.slen, np.uint8)
                  for i in range(self.total)]
            sh = sh[:t.N + t.M]
            oracle.rs_encode(t.N, t.M, sh)
            want_par.append(sh)
            # local parities (l > 0) are no part of the call: they lie in
            # the arena as encoded and must come back untouched
            for i in range(self.total):
                a.put(self.off(s, i), np.zeros(self.slen, np.uint8)
                      if t.N <= i < t.N + t.M else self.ref[s, i])
        a.upload()
        self.want = a.expect()
        for s in range(self.ns):
            for i in range(t.N, t.N + t.M):
                a.put(self.off(s, i), want_par[s][i], self.want)
        self.pptrs = [(ctypes.c_void_p * t.M)(
            *[a.ptr + self.off(s, i) for i in range(t.N, t.N + t.M)])
            for s in range(self.ns)]
        self.rcs = []

    def off(self, s, i):
        return (s * self.total + i) * (self.slen + 3)

    def issue(self, enc):
        f, ctx, a = L().gfrs_encode_idx, enc._ctx, self.a
        for i in self.idxs:
            for s in range(self.ns):
                self.rcs.append(f(ctx, vp(a.ptr + self.off(s, i)), i,
                                  self.pptrs[s], self.slen, self.t.M))

    def check(self, enc):
        for rc in self.rcs:
            ok(rc, self.what)
        sync(enc)
        self.a.check(self.want, what=self.what)


class UpdateIdx(_PtrStep):
    """Replace data shard `idx`: the global parity equals a fresh encode;
    local parities (l > 0) are no part of the call and stay.  same=True:
    the new shard has the old one's content, so the parity must come back
    unchanged."""

    def __init__(self, t, ref, idx=2, seed=34, what="", same=False):
        super().__init__(t, ref, False, seed, what)
        self.idx, self.same = idx, same

    def prepare(self, dev):
        t = self.t
        par = range(t.N, t.N + t.M)
        self.a = self.arena(dev, extra_shards=1)
        if self.same:
            new = self.ref[0, self.idx].copy()
        else:
            new = np.random.default_rng(77).integers(0, 256, self.slen,
                                                     dtype=np.uint8)
        self.a.put(self.offs[self.total], new)
        self.a.upload()
        self.pptrs = self.table(par)
        sh = [self.ref[0, i].copy() for i in range(t.N + t.M)]
        sh[self.idx] = new.copy()
        oracle.rs_encode(t.N, t.M, sh)
        self.want = self.filled(par, sh)

    def issue(self, enc):
        a = self.a
        self.rc = L().gfrs_update_idx(
            enc._ctx, vp(a.ptr + self.offs[self.idx]),
            vp(a.ptr + self.offs[self.total]), self.idx, self.pptrs,
            self.slen, self.t.M)

    def check(self, enc):
        ok(self.rc, self.what + " gfrs_update_idx")
        sync(enc)
        self.a.check(self.want, what=self.what + " gfrs_update_idx")


# ---- the four queues -----------------------------------------------------------

class QueueCall(Step):
    """One queue call through the load / call / check of its helper module
    (_repairq, _repairimgq, _encq or _readq) and a queue that module builds
    by name."""

    def __init__(self, module, name, what=""):
        self.module, self.name = module, name
        self.what = "%s %s %s" % (what, module, name)

    def prepare(self, dev):
        import importlib
        self.m = importlib.import_module(self.module)
        self.q = self.m.build(self.name)
        loaded = self.m.load(self.q, dev)
        self.arenas = loaded if isinstance(loaded, tuple) else (loaded,)

    def issue(self, enc):
        self.out = self.m.call(enc, *self.arenas, self.q)

    def check(self, enc):
        m, q, out, what = self.m, self.q, self.out, self.what
        ok(out if isinstance(out, int) else out[0], what)
        sync(enc)
        if self.module == "_repairq":
            want, fails, unspec = m.wanted(q, self.arenas[0])
            assert out[1] == fails, (what, out[1], fails)
            self.arenas[0].check(want, unspec, what=what)
        elif self.module == "_encq":
            m.check(q, *self.arenas, what)
        else:
            m.check(q, *self.arenas, out[1], what)


