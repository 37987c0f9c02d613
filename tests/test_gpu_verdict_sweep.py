"""Erasure pattern x corrupted column sweep: the fail bitmap of
gfrs_reconstruct_verify_batch, gfrs_repair_batch and the unfused pair
gfrs_reconstruct_batch + gfrs_verify_batch equals the reference's
Reconstruct followed by Verify (local stripes included), computed by the
CPU oracle for the very bytes the engine gets (tests/_verdict.py).

One call per (tactic, pattern, entry point) on a batch of total + 1
stripes: stripe s has one flipped bit in column s (offset and mask cycle
through the position list of that shard length), the last stripe is
clean.  Erased shards are not loaded at all: their regions hold arena noise,
so a flip in an erased column sits in bytes the call overwrites or ignores
and must neither be flagged nor change an output.  Every call runs in a
guarded arena: rewritten shards / disk images
equal the oracle's reconstruction, every other byte is unchanged, an
undecodable pattern returns a negative code.  One long-lived encoder per
tactic serves the whole sweep, so the plan caches meet every pattern in
sequence; each sorted pattern with nbad >= 2 is followed by the same
erasures in reversed caller order (a cache hit whose images must swap).

Cases (patterns; the reversed twins come on top), shard_len 33:
  EC6P3   129 = all with 1 <= nbad <= 3        + 1 undecodable
  EC4P2    21 = all with nbad <= 2             + 1
  EC3P3    41 = all with nbad <= 3             + 1
  EC12P4  136 (nbad <= 2) + 48 + 48 sampled    + 1
  EC13P4  153 (nbad <= 2) + 48 + 48 sampled    + 1   (width 17: unfused)
  EC6P6    78 (nbad <= 2) + 4 x 48 sampled     + 1   (two output groups)
  LRC12P2L2 136, EC6P3L3 78, EC4P4L2 55 (nbad <= 2), each + 64 sampled with
  nbad 3..4 + 1, the oracle deciding which of them decode
(The reversed twin reuses the plan its sorted twin built; a plan BUILT
from an unsorted list is met through the fixed patterns below, half of
which come in descending caller order and several for the first time.)
and 12 fixed patterns per tactic at 4093 and 8209, and at 70005 for the
tactics that have a fused repair path.  The sample seed is in _verdict.py.
"""
import os
import subprocess
import sys

import pytest

torch = pytest.importorskip("torch")

import _verdict as V  # noqa: E402

pytestmark = pytest.mark.gpu

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.mark.parametrize("name,grp", V.group_ids(),
                         ids=["%s-%s" % g for g in V.group_ids()])
def test_verdict_sweep(dev, name, grp):
    V.run_group(dev, name, grp)


@pytest.mark.parametrize("name,slen", V.WIDE)
def test_wide_bitmap(dev, name, slen):
    """130 stripes (three bitmap words), every third corrupted, the flips
    walking every column: the exact set of flagged stripes."""
    V.run_wide(dev, name, slen)


_SCRIPT = r"""
import os
import sys
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import torch
import _verdict as V

dev = torch.device("cuda:0")
for name, slen in V.WIDE:
    V.run_wide(dev, name, slen)
print("wide bitmap OK")
"""


def test_wide_bitmap_grid_stride():
    """The same four batches with the rs_apply and small-repair grids
    capped at 3 blocks, so every block walks many tiles.  The caps are
    read once per process: a fresh child."""
    env = dict(os.environ, GFRS_RS_GRID="3", GFRS_CRC_GRID="3")
    r = subprocess.run([sys.executable, "-c", _SCRIPT], env=env, cwd=_REPO,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "wide bitmap OK" in r.stdout
