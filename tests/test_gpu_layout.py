"""C-ABI layouts the Python wrapper cannot express: stripe_stride with
padding between stripes, batch bases at odd byte offsets, shard lengths
that leave every later shard misaligned, tight and padded image strides.

Every call runs inside a guarded arena (tests/_arena.py): declared outputs
are compared bit-exactly with the CPU oracle and every other byte of the
arena (guards, padding, inputs) must come back unchanged.
"""
import itertools

import pytest

torch = pytest.importorskip("torch")

import _arena as A  # noqa: E402
from _arena import L, Arena, Rows, Stripes, vp  # noqa: E402

pytestmark = pytest.mark.gpu

SLENS = [33, 1000, 4093, 4097 + 3]
PADS = [0, 1, 52]
DELTAS = [0, 1, 7]
EXTRAS = [0, 12]
NS = 5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def t63():
    from cubefs_amd import codemode
    return codemode.get_tactic("EC6P3")


def layouts():
    return itertools.product(PADS, DELTAS)


@pytest.mark.parametrize("slen", SLENS)
def test_encode_batch_layout(dev, t63, slen):
    t, enc = t63, A.encoder(t63)
    ref = A.ref_stripes(t, NS, slen)
    for pad, delta in layouts():
        lay = Stripes(NS, t.total, slen, pad)
        a = Arena(dev, lay.nbytes, delta, seed=10)
        A.load_stripes(a, lay, ref, skip=range(t.N, t.total))
        a.upload()
        A.ok(L().gfrs_encode_batch(enc._ctx, vp(a.ptr), slen, lay.stride, NS),
             "encode_batch")
        A.sync(enc)
        want = a.expect()
        for s in range(NS):
            for i in range(t.N, t.total):
                a.put(lay.off(s, i), ref[s, i], want)
        a.check(want, what="encode_batch slen=%d pad=%d delta=%d"
                % (slen, pad, delta))


@pytest.mark.parametrize("slen", SLENS)
def test_verify_batch_layout(dev, t63, slen):
    t, enc = t63, A.encoder(t63)
    ref = A.ref_stripes(t, NS, slen)
    for pad, delta in layouts():
        lay = Stripes(NS, t.total, slen, pad)
        a = Arena(dev, lay.nbytes, delta, seed=11)
        A.load_stripes(a, lay, ref)
        # one corrupt byte in stripe 3 so "all clean" is not the only answer
        a.host[a.off + lay.off(3, t.N + 1) + slen // 2] ^= 0x20
        a.upload()
        bm = A.bitmap(NS)
        A.ok(L().gfrs_verify_batch(enc._ctx, vp(a.ptr), slen, lay.stride, NS,
                                   bm), "verify_batch")
        what = "verify_batch slen=%d pad=%d delta=%d" % (slen, pad, delta)
        assert A.bits(bm, NS) == [3], what
        a.check(a.expect(), what=what)


@pytest.mark.parametrize("data_only", [0, 1])
@pytest.mark.parametrize("slen", SLENS)
def test_reconstruct_batch_layout(dev, t63, slen, data_only):
    t, enc = t63, A.encoder(t63)
    ref = A.ref_stripes(t, NS, slen)
    bad = [7, 1]  # one parity, one data
    rebuilt = [1] if data_only else bad
    for pad, delta in layouts():
        lay = Stripes(NS, t.total, slen, pad)
        a = Arena(dev, lay.nbytes, delta, seed=12)
        A.load_stripes(a, lay, ref, skip=bad)
        a.upload()
        A.ok(L().gfrs_reconstruct_batch(enc._ctx, vp(a.ptr), slen, lay.stride,
                                        NS, A.i32s(bad), len(bad), data_only),
             "reconstruct_batch")
        A.sync(enc)
        want = a.expect()  # with data_only the lost parity stays as it was
        for s in range(NS):
            for i in rebuilt:
                a.put(lay.off(s, i), ref[s, i], want)
        a.check(want, what="reconstruct_batch slen=%d pad=%d delta=%d do=%d"
                % (slen, pad, delta, data_only))


@pytest.mark.parametrize("slen", SLENS)
def test_reconstruct_verify_batch_layout(dev, t63, slen):
    t, enc = t63, A.encoder(t63)
    ref = A.ref_stripes(t, NS, slen)
    bad = [2, 6]
    for pad, delta in layouts():
        lay = Stripes(NS, t.total, slen, pad)
        a = Arena(dev, lay.nbytes, delta, seed=13)
        A.load_stripes(a, lay, ref, skip=bad)
        a.upload()
        bm = A.bitmap(NS)
        A.ok(L().gfrs_reconstruct_verify_batch(
            enc._ctx, vp(a.ptr), slen, lay.stride, NS, A.i32s(bad), len(bad),
            bm), "reconstruct_verify_batch")
        A.sync(enc)
        what = "reconstruct_verify slen=%d pad=%d delta=%d" % (slen, pad,
                                                               delta)
        assert A.bits(bm, NS) == [], what
        want = a.expect()
        for s in range(NS):
            for i in bad:
                a.put(lay.off(s, i), ref[s, i], want)
        a.check(want, what=what)


@pytest.mark.parametrize("extra", EXTRAS)
@pytest.mark.parametrize("slen", SLENS)
def test_encode_frame_batch_layout(dev, t63, slen, extra):
    ref = A.ref_stripes(t63, NS, slen)
    for pad, delta in layouts():
        A.run_encode_frame(dev, t63, ref, pad, delta, extra,
                           "encode_frame slen=%d pad=%d delta=%d extra=%d"
                           % (slen, pad, delta, extra))


@pytest.mark.parametrize("extra", EXTRAS)
@pytest.mark.parametrize("slen", SLENS)
def test_repair_batch_layout(dev, t63, slen, extra):
    ref = A.ref_stripes(t63, NS, slen)
    for pad, delta in layouts():
        fails = A.run_repair(dev, t63, ref, [8, 4], pad, delta, extra,
                             what="repair slen=%d pad=%d delta=%d extra=%d"
                             % (slen, pad, delta, extra))
        assert fails == []


@pytest.mark.parametrize("slen", [1000, 4093])
def test_lrc_batch_layout(dev, slen):
    """LRC: global + per-AZ local rs_apply launches and the one-pass mixed
    reconstruct+verify on a padded, odd-based batch."""
    t = A.lrc_tactic()
    A.run_rs_apply(dev, t, A.ref_stripes(t, NS, slen), pad=52, delta=7,
                   bad=(1, 13), what="LRC slen=%d" % slen)


def test_encode_frame_fallback_layout(dev):
    """m+l > 4 composes encode_batch + crc32b_encode_batch, which needs the
    contiguous stripe stride: a padded one is refused without touching
    memory, the contiguous one matches the oracle."""
    from cubefs_amd import codemode
    t = codemode.get_tactic("EC6P6")
    enc = A.encoder(t)
    slen = 1000
    ref = A.ref_stripes(t, NS, slen)
    for pad in (1, 52):
        lay = Stripes(NS, t.total, slen, pad)
        src = Arena(dev, lay.nbytes, 0, seed=14)
        A.load_stripes(src, lay, ref, skip=range(t.N, t.total))
        src.upload()
        rows = Rows(NS * t.total, A.enc_size(slen))
        dst = Arena(dev, rows.nbytes, 0, seed=15)
        dst.upload()
        rc = L().gfrs_encode_frame_batch(enc._ctx, vp(dst.ptr), rows.stride,
                                         vp(src.ptr), slen, lay.stride, NS,
                                         A.BLOCK)
        assert rc == A.ERR_UNSUPPORTED, (pad, rc)
        A.sync(enc)
        src.check(src.expect(), what="fallback refused: source")
        dst.check(dst.expect(), what="fallback refused: images")
    # contiguous stride: the composition runs; it materialises the parity
    # in `base` (declared output of encode_batch), data stays read-only
    for delta, extra in ((0, 0), (7, 12)):
        A.run_encode_frame(dev, t, ref, 0, delta, extra,
                           "fallback delta=%d extra=%d" % (delta, extra),
                           composed=True)


# ---- crc32block / shard image batches ------------------------------------
# The pad goes on the SOURCE stride of each call: the raw shards for
# encode/write, the framed images for verify/parse.

NSH = 7


@pytest.mark.parametrize("extra", EXTRAS)
@pytest.mark.parametrize("slen", SLENS)
def test_crc32b_batch_layout(dev, t63, slen, extra):
    """gfrs_crc32b_encode_batch + gfrs_crc32b_verify_batch (+ decode)."""
    enc = A.encoder(t63)
    for pad, delta in layouts():
        A.run_crc(dev, enc, slen, NSH, pad, delta, extra,
                  "slen=%d pad=%d delta=%d extra=%d" % (slen, pad, delta,
                                                        extra))


@pytest.mark.parametrize("extra", EXTRAS)
@pytest.mark.parametrize("slen", SLENS)
def test_shard_image_batch_layout(dev, t63, slen, extra):
    """gfrs_shard_write_batch + gfrs_shard_parse_batch."""
    enc = A.encoder(t63)
    for pad, delta in layouts():
        A.run_shard_images(dev, enc, slen, NSH, pad, delta, extra,
                           "slen=%d pad=%d delta=%d extra=%d" % (
                               slen, pad, delta, extra))


# ---- pointer-table single-stripe calls ---------------------------------------

def test_pointer_table_calls_layout(dev, t63):
    """All shards of one stripe as views at odd, non-contiguous offsets
    (the steps of tests/_arena.py, one at a time)."""
    t, enc = t63, A.encoder(t63)
    ref = A.ref_stripes(t, 1, 4093, seed=5)
    steps = [A.Encode(t, ref),
             # clean, then one bit in the last byte of a data shard
             A.Verify(t, ref, flip=False), A.Verify(t, ref, flip=True),
             A.Reconstruct(t, ref, bad=[8, 0], data_only=0),
             A.Reconstruct(t, ref, bad=[8, 0], data_only=1),
             # accumulate every data shard into zeroed parity
             A.EncodeIdx(t, ref),
             # replace data shard 2, parity equals a fresh encode
             A.UpdateIdx(t, ref, idx=2)]
    for step in steps:
        step.run(dev, enc)


# ---- detection in the byte-tail paths, wide fail bitmaps -------------------

def _flip_positions(slen):
    """Last byte (per-byte tail path) and a byte of the last full 16-B
    piece (last vector iteration)."""
    return [slen - 1, (slen // 16) * 16 - 9]


@pytest.mark.parametrize("slen", [1000, 4093])
def test_tail_corruption_flags_only_that_stripe(dev, t63, slen):
    t, enc = t63, A.encoder(t63)
    ref = A.ref_stripes(t, NS, slen)
    assert slen % 16
    for pos in _flip_positions(slen):
        what = "slen=%d pos=%d" % (slen, pos)
        # verify_batch: surviving shard = any shard; take parity 7, stripe 1
        lay = Stripes(NS, t.total, slen, 0)
        a = Arena(dev, lay.nbytes, 0, seed=40)
        A.load_stripes(a, lay, ref)
        a.host[a.off + lay.off(1, 7) + pos] ^= 0x01
        a.upload()
        bm = A.bitmap(NS)
        A.ok(L().gfrs_verify_batch(enc._ctx, vp(a.ptr), slen, lay.stride, NS,
                                   bm), "verify_batch")
        assert A.bits(bm, NS) == [1], what
        # reconstruct_verify_batch, nbad < m: corrupt surviving parity 8
        bad = [3]
        a = Arena(dev, lay.nbytes, 0, seed=41)
        A.load_stripes(a, lay, ref, skip=bad)
        a.host[a.off + lay.off(4, 8) + pos] ^= 0x80
        a.upload()
        bm = A.bitmap(NS)
        A.ok(L().gfrs_reconstruct_verify_batch(
            enc._ctx, vp(a.ptr), slen, lay.stride, NS, A.i32s(bad), 1, bm),
            "reconstruct_verify_batch")
        assert A.bits(bm, NS) == [4], what


@pytest.mark.parametrize("slen", [1000, 4093, 70000 + 5])
def test_repair_tail_corruption_flags_only_that_stripe(dev, t63, slen):
    """Small (<= 4096) and big fused repair with check rows: a bit flipped
    in the byte tail / last 16-B piece of a surviving check shard."""
    ref = A.ref_stripes(t63, NS, slen)
    assert slen % 16
    for pos in _flip_positions(slen):
        # bad=[5]: inputs are shards 0-4,6; 7 and 8 are check rows
        fails = A.run_repair(dev, t63, ref, [5], corrupt=(2, 8, pos, 0x10),
                             what="repair tail slen=%d pos=%d" % (slen, pos))
        assert fails == [2], (slen, pos, fails)
        # corrupt an INPUT shard: the check rows must catch that as well
        fails = A.run_repair(dev, t63, ref, [5], corrupt=(0, 1, pos, 0x04),
                             what="repair tail(in) slen=%d pos=%d"
                             % (slen, pos))
        assert fails == [0], (slen, pos, fails)


def test_fail_bitmap_three_words(dev, t63):
    t, enc = t63, A.encoder(t63)
    ns, slen = 130, 33
    ref = A.ref_stripes(t, ns, slen, seed=6)
    hit = [0, 63, 64, 129]
    lay = Stripes(ns, t.total, slen, 0)

    def arena(skip=()):
        a = Arena(dev, lay.nbytes, 0, seed=42)
        A.load_stripes(a, lay, ref, skip=skip)
        for s in hit:
            a.host[a.off + lay.off(s, 7) + (s % slen)] ^= 0x08
        a.upload()
        return a

    a = arena()
    bm = A.bitmap(ns)
    assert len(bm) == 3
    A.ok(L().gfrs_verify_batch(enc._ctx, vp(a.ptr), slen, lay.stride, ns, bm),
         "verify_batch")
    assert A.bits(bm, ns) == hit
    a = arena(skip=[2])
    bm = A.bitmap(ns)
    A.ok(L().gfrs_reconstruct_verify_batch(
        enc._ctx, vp(a.ptr), slen, lay.stride, ns, A.i32s([2]), 1, bm),
        "reconstruct_verify_batch")
    assert A.bits(bm, ns) == hit
    # fused small repair: same four stripes through the repair bitmap
    assert _repair_bitmap(dev, t, ref, hit) == hit


def _repair_bitmap(dev, t, ref, hit):
    ns, total, slen = ref.shape
    enc = A.encoder(t)
    lay = Stripes(ns, total, slen, 0)
    src = Arena(dev, lay.nbytes, 0, seed=43)
    A.load_stripes(src, lay, ref, skip=[2])
    for s in hit:
        src.host[src.off + lay.off(s, 7) + (s % slen)] ^= 0x08
    src.upload()
    rows = Rows(ns, A.disk_size(slen))
    dst = Arena(dev, rows.nbytes, 0, seed=44)
    dst.upload()
    bm = A.bitmap(ns)
    A.ok(L().gfrs_repair_batch(enc._ctx, vp(src.ptr), slen, lay.stride, ns,
                               A.i32s([2]), 1, vp(dst.ptr), rows.stride,
                               A.BLOCK, A.u64s(list(range(ns))),
                               A.u64s([1] * ns), bm), "repair_batch")
    A.sync(enc)
    return A.bits(bm, ns)
