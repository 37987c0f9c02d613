"""Grid-stride is what production shapes execute (every launcher caps its
grid far below the headline 1024 stripes x 129 frames), yet test-sized
launches never loop.  The caps are read from the environment on every
launch (env_grid in gfrs_kernels.hip: GFRS_RS_GRID for rs_apply,
GFRS_CRC_GRID for the CRC, fused encode+frame and fused repair kernels,
big and small), so forcing them to 3 makes tiny shapes take the stride
loops: the second iteration's per-frame state, the coprime grid
adjustment and the loop-tail barriers all run.

crc32b_small_k has a fixed 2048-block cap and is run past it for real.
"""
import pytest

torch = pytest.importorskip("torch")

import _arena as A  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture
def t63():
    from cubefs_amd import codemode
    return codemode.get_tactic("EC6P3")


@pytest.fixture
def cap3(monkeypatch):
    monkeypatch.setenv("GFRS_CRC_GRID", "3")
    monkeypatch.setenv("GFRS_RS_GRID", "3")


@pytest.mark.parametrize("slen,ns", [(1000, 23),   # packed: 4 stripes/tile,
                                                   # 6 tiles over 3 blocks
                                     (9000, 5)])   # tiled: 15 tiles
def test_rs_apply_grid_stride(dev, t63, cap3, slen, ns):
    A.run_rs_apply(dev, t63, A.ref_stripes(t63, ns, slen), pad=52, delta=1,
                   what="rs_apply stride slen=%d" % slen)


@pytest.mark.parametrize("slen", [3000, 6000])  # 4-wave NI=3, 3-wave NI=6
def test_encode_frame_small_grid_stride(dev, t63, cap3, slen):
    # 37 stripes = 10 wave-groups over 3 blocks, ragged last group
    A.run_encode_frame(dev, t63, A.ref_stripes(t63, 37, slen), pad=1,
                       what="small encode stride slen=%d" % slen)


def test_encode_frame_big_grid_stride(dev, t63, cap3):
    # 4 frames per shard x 5 stripes = 20 frames over 3 blocks
    A.run_encode_frame(dev, t63, A.ref_stripes(t63, 5, 200001), extra=12,
                       what="big encode stride")


def test_encode_frame_big_coprime_adjust(dev, t63, monkeypatch):
    """fps = 2 with a cap of 4: gcd(4, 2) != 1, so the launcher steps the
    grid down to 3."""
    monkeypatch.setenv("GFRS_CRC_GRID", "4")
    A.run_encode_frame(dev, t63, A.ref_stripes(t63, 6, 70000),
                       what="big encode coprime")


def test_encode_frame_tiny_fold_grid_stride(dev, t63, cap3):
    """The folded tiny last frame inside the stride loop: the per-frame
    fold state must not leak into the block's next frame."""
    A.run_encode_frame(dev, t63, A.ref_stripes(t63, 4, 2 * 65532 + 1),
                       what="big encode stride + tiny fold")


@pytest.mark.parametrize("slen,ns", [(3000, 37), (70000, 5)],
                         ids=["small", "big"])
def test_repair_grid_stride(dev, t63, cap3, slen, ns):
    ref = A.ref_stripes(t63, ns, slen)
    assert A.run_repair(dev, t63, ref, [7, 2], what="repair stride") == []
    # a corrupt surviving shard in a stripe only the second loop
    # iteration reaches must flag that stripe alone
    hit = ns - 1
    fails = A.run_repair(dev, t63, ref, [4], corrupt=(hit, 8, slen - 1, 2),
                         what="repair stride corrupt")
    assert fails == [hit]


def test_crc_grid_stride(dev, t63, cap3):
    enc = A.encoder(t63)
    # 4 frames per shard x 5 shards; decode walks one shard's 4 frames
    A.run_crc(dev, enc, 200001, 5, pad=1, delta=1, what="crc stride")
    A.run_sized(dev, enc, 200001 + 65532, what="sized stride")


def test_shard_image_grid_stride(dev, t63, cap3):
    A.run_shard_images(dev, A.encoder(t63), 200001, 5, pad=1, delta=0,
                       what="shard image stride")


def test_crc_small_fixed_cap(dev, t63):
    """crc32b_small_k: one wave per 33-byte shard, 4 per block, capped at
    2048 blocks; 8203 shards need 2051, so the last 11 shards are the
    second loop iteration of blocks 0-2."""
    enc = A.encoder(t63)
    A.run_crc(dev, enc, 33, 8203, what="crc small cap")
    A.run_shard_images(dev, enc, 33, 8203, what="shard small cap")
