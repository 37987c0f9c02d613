"""Return codes and fallbacks of the three batch reconstruct entry points
for bad lists no plan can be built from: out of range, duplicate, too many,
empty.  Raw C ABI on 2 stripes of 33-byte shards in guarded arenas
(tests/_arena.py).  Every refused call returns before a kernel is launched,
so the whole arena - erased regions included - comes back bit-identical.

The two accepted cases pin what a duplicate does where it is tolerated:
plain RS reconstruct+verify treats the list as a set, and RS(6+6) repair
(m + l > 4: reconstruct+verify, then one image column per list entry)
writes the same shard into both columns.
"""
import pytest

torch = pytest.importorskip("torch")

import _arena as A  # noqa: E402
import _verdict as V  # noqa: E402
from _arena import L, Arena, Rows, Stripes, oracle, vp  # noqa: E402

pytestmark = pytest.mark.gpu

NS, SLEN = 2, 33
INVALID_SHARDS, TOO_FEW = -6, -2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _base(dev, t, bad, seed):
    ref = A.ref_stripes(t, NS, SLEN, seed=13)
    lay = Stripes(NS, ref.shape[1], SLEN, 0)
    a = Arena(dev, lay.nbytes, 0, seed=seed)
    A.load_stripes(a, lay, ref, skip=[b for b in bad if 0 <= b < lay.total])
    a.upload()
    return ref, lay, a


def reconstruct_verify(dev, t, bad, ns=NS):
    ref, lay, a = _base(dev, t, bad, 70)
    bm = A.bitmap(NS)
    rc = L().gfrs_reconstruct_verify_batch(A.encoder(t)._ctx, vp(a.ptr), SLEN,
                                           lay.stride, ns, A.i32s(bad),
                                           len(bad), bm)
    A.sync(A.encoder(t))
    return rc, ref, lay, a, bm


def reconstruct(dev, t, bad):
    ref, lay, a = _base(dev, t, bad, 71)
    rc = L().gfrs_reconstruct_batch(A.encoder(t)._ctx, vp(a.ptr), SLEN,
                                    lay.stride, NS, A.i32s(bad), len(bad), 0)
    A.sync(A.encoder(t))
    return rc, ref, lay, a


def repair(dev, t, bad, nbad=None):
    nbad = len(bad) if nbad is None else nbad
    ref, lay, src = _base(dev, t, bad, 72)
    rows = Rows(NS * max(nbad, 1), A.disk_size(SLEN))
    dst = Arena(dev, rows.nbytes, 0, seed=73)
    dst.upload()
    nimg = NS * max(nbad, 1)
    bids = [4000 + j for j in range(nimg)]
    vuids = [0x55667788 + j for j in range(nimg)]
    bm = A.bitmap(NS)
    rc = L().gfrs_repair_batch(A.encoder(t)._ctx, vp(src.ptr), SLEN,
                               lay.stride, NS, A.i32s(bad), nbad, vp(dst.ptr),
                               rows.stride, A.BLOCK, A.u64s(bids),
                               A.u64s(vuids), bm)
    A.sync(A.encoder(t))
    return rc, ref, lay, src, rows, dst, bids, vuids, bm


RV_REFUSED = [("EC6P3", [9], NS, INVALID_SHARDS),
              ("EC6P3", [-1], NS, INVALID_SHARDS),
              ("EC6P3", [0], 0, INVALID_SHARDS),
              ("EC6P3", [0, 1, 2, 3], NS, TOO_FEW),
              ("LRC12P2L2", [16], NS, INVALID_SHARDS),
              ("LRC12P2L2", [0, 0], NS, INVALID_SHARDS),
              ("LRC12P2L2", [0, 1, 2], NS, TOO_FEW)]


@pytest.mark.parametrize("name,bad,ns,want", RV_REFUSED,
                         ids=["%s-%s-ns%d" % (c[0], c[1], c[2])
                              for c in RV_REFUSED])
def test_reconstruct_verify_refused(dev, name, bad, ns, want):
    rc, _, _, a, _ = reconstruct_verify(dev, V.get_tactic(name), bad, ns)
    assert rc == want
    a.check(a.expect(), what="refused reconstruct_verify %s" % bad)


def test_reconstruct_verify_duplicate_is_a_set(dev):
    """Plain RS: bad [0, 0] is accepted and leaves the same bytes as [0]."""
    t = V.get_tactic("EC6P3")
    got = []
    for bad in ([0], [0, 0]):
        rc, ref, lay, a, bm = reconstruct_verify(dev, t, bad)
        assert rc == 0, bad
        assert A.bits(bm, NS) == [], bad
        a.check(A.want_like(a, lay, ref, [0]), what="bad=%s" % bad)
        got.append(a.dev.cpu().numpy())
    assert (got[0] == got[1]).all()


RECON_REFUSED = [([9], INVALID_SHARDS), ([0, 1, 2, 3], TOO_FEW),
                 ([1, 4, 6, 8], TOO_FEW)]


@pytest.mark.parametrize("bad,want", RECON_REFUSED,
                         ids=[str(c[0]) for c in RECON_REFUSED])
def test_reconstruct_refused(dev, bad, want):
    rc, _, _, a = reconstruct(dev, V.get_tactic("EC6P3"), bad)
    assert rc == want
    a.check(a.expect(), what="refused reconstruct %s" % bad)


REPAIR_REFUSED = [([0], 0, INVALID_SHARDS), ([9], None, INVALID_SHARDS),
                  ([0, 0], None, INVALID_SHARDS),
                  ([0, 1, 2, 3], None, TOO_FEW)]


@pytest.mark.parametrize("bad,nbad,want", REPAIR_REFUSED,
                         ids=["%s-nbad%s" % (c[0], c[1])
                              for c in REPAIR_REFUSED])
def test_repair_refused(dev, bad, nbad, want):
    rc, _, _, src, _, dst, _, _, _ = repair(dev, V.get_tactic("EC6P3"), bad,
                                            nbad)
    assert rc == want
    src.check(src.expect(), what="refused repair %s base" % bad)
    dst.check(dst.expect(), what="refused repair %s images" % bad)


def test_repair_rs66_duplicate_writes_both_columns(dev):
    """RS(6+6) has no fused repair: bad [0, 0] reconstructs shard 0 in place
    (duplicates form a set there) and frames it once per list entry."""
    t = V.get_tactic("EC6P6")
    rc, ref, lay, src, rows, dst, bids, vuids, bm = repair(dev, t, [0, 0])
    assert rc == 0
    assert A.bits(bm, NS) == []
    want = dst.expect()
    for s in range(NS):
        for b in range(2):
            j = s * 2 + b
            dst.put(rows.off(j), oracle.shard_write(ref[s, 0].copy(),
                                                    bid=bids[j],
                                                    vuid=vuids[j]), want)
    dst.check(want, what="rs66 duplicate images")
    src.check(A.want_like(src, lay, ref, [0]), what="rs66 duplicate base")
