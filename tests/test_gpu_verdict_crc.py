"""CRC, sized-coder and shard-image verdicts against the oracle.

One batch call per shape, shard j carrying corruption case j; the expected
bad-block index / error comes from running the oracle
(crc32b_verify, sized_verify, shard_parse) on the same bytes.  The cases
(tests/_verdict.py) flip one bit in each stored-CRC byte of the first and
the last frame, in the first payload byte, on both sides of the 4096-B
piece stride, the 16384-B pass edge and the start of the short fourth pass
of crc32b_verify_reg_k, in the last byte of a full and of the partial
frame; one shard is clean and one has two bad blocks (the lower index is
reported).  Payload sizes sit on both sides of every kernel threshold:
1, 100, 8192 | 8193 (crc32b_small_k ends), 65532 | 65533 (one full frame /
plus a 1-byte frame) and 3*65532+5.
"""
import os
import subprocess
import sys

import pytest

torch = pytest.importorskip("torch")

import _arena as A  # noqa: E402
import _verdict as V  # noqa: E402

pytestmark = pytest.mark.gpu

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def enc():
    from cubefs_amd import codemode
    return A.encoder(codemode.get_tactic("EC6P3"))


@pytest.mark.parametrize("block_len", [65536, 4096, 8192])
@pytest.mark.parametrize("n", V.CRC_SIZES)
def test_crc32b_verdicts(dev, enc, n, block_len):
    """gfrs_crc32b_verify_batch, gfrs_crc32b_verify, gfrs_crc32b_decode;
    block_len 4096 / 8192 take the crc32b_k path."""
    V.run_crc_cases(dev, enc, n, block_len)


@pytest.mark.parametrize("n", V.SIZED_SIZES)
def test_sized_verdicts(dev, enc, n):
    """gfrs_sized_verify / gfrs_sized_decode: each byte of the first and
    last big-endian tail CRC, the payload edges, one flip in the zero pad."""
    V.run_sized_cases(dev, enc, n)


@pytest.mark.parametrize("slen", [100, 70005])
def test_shard_parse_verdicts(dev, enc, slen):
    """gfrs_shard_parse_batch over 42 images: each header byte (header CRC,
    magic, bid, vuid, size, reserved), each footer byte (magic, CRC), one
    body byte, one clean image."""
    V.run_shard_cases(dev, enc, slen)


_SCRIPT = r"""
import os
import sys
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import torch
import _arena as A
import _verdict as V
from cubefs_amd import codemode

dev = torch.device("cuda:0")
enc = A.encoder(codemode.get_tactic("EC6P3"))
for n in V.CRC_SIZES:
    V.run_crc_cases(dev, enc, n, 65536)
print("verify variant OK")
"""


@pytest.mark.parametrize("vrfy", ["10", "14", "16", "18"])
def test_verify_variant_verdicts(vrfy):
    """The measured crc32b_verify_reg_k variants (legacy per-pass
    operators, load lookahead at 4 / 6 / 8 waves) on the 65536-block
    verify and decode cases.  The selector is read once per process: a
    fresh child each.  90 / 91 are measurement skeletons that compute wrong
    CRCs by design and stay uncovered."""
    env = dict(os.environ, GFRS_VRFY=vrfy)
    r = subprocess.run([sys.executable, "-c", _SCRIPT], env=env, cwd=_REPO,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (vrfy, r.stdout[-2000:], r.stderr[-3000:])
    assert "verify variant OK" in r.stdout
