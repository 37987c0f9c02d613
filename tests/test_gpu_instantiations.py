"""Launch every shipped instantiation of the fused kernels from a fixed
test: GM (output rows) 1-4, the small kernels' NI axis (1 KiB sub-tiles
per lane; NI >= 6 is the 3-wave build), both size policies of the big
kernels (4-wave below 1 MiB, 3-wave from 1 MiB), the tiny-last-frame
fold, nbad == 4 with no check rows, and the widest fused shape
(n + gm == 16) next to the first shape that falls back.

All comparisons are bit-exact against the CPU oracle inside a guarded
arena (tests/_arena.py), so stride padding and the source are checked too.
"""
import pytest

torch = pytest.importorskip("torch")

import _arena as A  # noqa: E402

pytestmark = pytest.mark.gpu

NS = 5           # one full 4-wave block plus a one-wave block
RS = (1, 1009, 1024)
MIB5 = (1 << 20) + 5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def small_axis():
    """(GM, NI) pairs the small encode kernel is instantiated for."""
    return [(gm, ni) for gm in (1, 2, 3, 4)
            for ni in range(1, (4 if gm == 4 else 8) + 1)]


@pytest.mark.parametrize("gm,ni", small_axis())
def test_encode_frame_small_matrix(dev, gm, ni):
    """rs_encode_frame_small_k<GM, NI>: shard_len = 1024*(NI-1) + r hits one
    tail byte, a ragged tail and the exact sub-tile; NI = 4 / 8 with
    r = 1024 are the 4096 / 8192 upper boundaries of the small path."""
    t = A.tactic(4, gm)
    for r in RS:
        slen = 1024 * (ni - 1) + r
        A.run_encode_frame(dev, t, A.ref_stripes(t, NS, slen), extra=12,
                           what="small GM=%d NI=%d slen=%d" % (gm, ni, slen))


def big_lengths(gm):
    first = 4097 if gm == 4 else 8193  # first length past the small kernel
    return [first, 65531, 65532, 65533, 65532 + 64, 65532 + 65,
            2 * 65532 + 1, 200001]


@pytest.mark.parametrize("gm,slen", [(gm, s) for gm in (1, 2, 3, 4)
                                     for s in big_lengths(gm)])
def test_encode_frame_big_matrix(dev, gm, slen):
    """rs_encode_frame_reg_k<GM>, default policy below 1 MiB (4-wave
    nontemporal form).  65533, 65532+64 and 2*65532+1 end in a last frame
    of <= 64 payload bytes that the previous frame's workgroup emits
    (tiny-last-frame fold); 65532+65 is the first length that does not."""
    t = A.tactic(4, gm)
    A.run_encode_frame(dev, t, A.ref_stripes(t, 3, slen),
                       what="big GM=%d slen=%d" % (gm, slen))


@pytest.mark.parametrize("gm", [1, 2, 3, 4])
def test_encode_frame_big_3wave(dev, gm):
    """>= 1 MiB shards take the 3-wave register-CRC pipeline."""
    t = A.tactic(4, gm)
    A.run_encode_frame(dev, t, A.ref_stripes(t, 2, MIB5), extra=12,
                       what="big3w GM=%d" % gm)


@pytest.mark.parametrize("n,m,composed", [(15, 1, False), (12, 4, False),
                                          (13, 4, True)])
@pytest.mark.parametrize("slen", [3000, 70001])
def test_encode_frame_width_edges(dev, n, m, composed, slen):
    """n + gm == 16 is the last fused shape; 13+4 is the first that takes
    the encode_batch + crc32b_encode_batch composition."""
    t = A.tactic(n, m)
    A.run_encode_frame(dev, t, A.ref_stripes(t, 3, slen), composed=composed,
                       what="width %d+%d slen=%d" % (n, m, slen))


# GM of the fused repair plan = rebuilt rows + check rows (at most 4)
REPAIR = [
    (1, 1, [2]),            # 4+1: no spare parity, GM 1
    (2, 2, [0]),            # 4+2: 1 rebuild + 1 check
    (2, 2, [5, 1]),         # 4+2: 2 rebuilds, unsorted
    (3, 3, [6, 0, 2]),      # 4+3: 3 rebuilds, unsorted
    (4, 4, [7, 0, 4, 1]),   # 4+4: nbad == 4, 4-nibble colpack, no checks
]
REPAIR_IDS = ["GM1", "GM2chk", "GM2", "GM3", "GM4"]


@pytest.mark.parametrize("ni", [1, 2, 3, 4])
@pytest.mark.parametrize("gm,m,bad", REPAIR, ids=REPAIR_IDS)
def test_repair_small_matrix(dev, gm, m, bad, ni):
    """rs_repair_frame_small_k<GM, NI>."""
    t = A.tactic(4, m)
    for r in RS:
        slen = 1024 * (ni - 1) + r
        fails = A.run_repair(dev, t, A.ref_stripes(t, NS, slen), bad,
                             extra=12, what="repair small GM=%d NI=%d slen=%d"
                             % (gm, ni, slen))
        assert fails == []


@pytest.mark.parametrize("slen,ns", [(70000, 3), (MIB5, 2)],
                         ids=["4wave", "3wave"])
@pytest.mark.parametrize("gm,m,bad", REPAIR, ids=REPAIR_IDS)
def test_repair_big_matrix(dev, gm, m, bad, slen, ns):
    """rs_repair_frame_k<GM, waves>: 4 waves below 1 MiB, 3 waves from
    1 MiB."""
    t = A.tactic(4, m)
    fails = A.run_repair(dev, t, A.ref_stripes(t, ns, slen), bad,
                         what="repair big GM=%d slen=%d" % (gm, slen))
    assert fails == []


def test_repair_small_lrc(dev):
    """LRC small-shard fused repair: a lost local parity and a lost data
    shard, surviving parities as check rows."""
    t = A.lrc_tactic()
    fails = A.run_repair(dev, t, A.ref_stripes(t, NS, 3000), [14, 5],
                         what="repair small LRC")
    assert fails == []


@pytest.mark.parametrize("slen", [3000, 70001])
def test_encode_frame_lrc_layout(dev, slen):
    """LRC runs fused through the composed plan (global and local parity
    as rows over the data shards), n + m + l == 16; padded stripe stride
    and an odd base."""
    t = A.lrc_tactic()
    A.run_encode_frame(dev, t, A.ref_stripes(t, 3, slen), pad=52, delta=1,
                       extra=12, what="LRC encode_frame slen=%d" % slen)
