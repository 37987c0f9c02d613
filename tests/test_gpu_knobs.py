"""Parity of the measured-variant knobs that select other kernels or
templates: GFRS_NT (nontemporal stores), GFRS_RS_SEQ (sequential tile
partition), GFRS_RP_WAVES (repair occupancy build), GFRS_CRC_CHUNK (staged
CRC geometry), GFRS_SMALL_MAX and GFRS_FUSED_MIN (kernel thresholds).

All of them are cached in function-local statics on first use, so each
setting gets one fresh child process running the same script: rs_apply
encode / verify / reconstruct, CRC encode / verify / decode, fused
encode+frame and fused repair, arena-checked against the CPU oracle
(tests/_arena.py).
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SCRIPT = r"""
import os
import sys
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import torch
import _arena as A
from cubefs_amd import codemode

dev = torch.device("cuda:0")
t = codemode.get_tactic("EC6P3")
enc = A.encoder(t)
fused_min = int(os.environ.get("GFRS_FUSED_MIN", "4097"))
small_max = int(os.environ.get("GFRS_SMALL_MAX", "8192"))

# rs_apply: packed (7 tiles, so a 3-block sequential partition is 3+3+1)
# and tiled
A.run_rs_apply(dev, t, A.ref_stripes(t, 26, 1000), what="rs packed")
A.run_rs_apply(dev, t, A.ref_stripes(t, 5, 9000), pad=52, delta=1,
               what="rs tiled")
# staged CRC kernels (multi-frame) and the sized coder
A.run_crc(dev, enc, 200001, 3, pad=1, delta=1, what="crc")
A.run_sized(dev, enc, 200001, what="sized")
# fused encode+frame: small 4-wave, small 3-wave / big, big
for slen in (3000, 6000, 70000):
    small = slen <= 4096 or slen <= small_max
    A.run_encode_frame(dev, t, A.ref_stripes(t, 5, slen),
                       composed=not small and slen < fused_min,
                       what="encode_frame %d" % slen)
# fused repair: small, big 4-wave policy, big 3-wave policy
for slen, ns in ((3000, 5), (70000, 3), ((1 << 20) + 5, 2)):
    ref = A.ref_stripes(t, ns, slen)
    assert A.run_repair(dev, t, ref, [7, 2], what="repair %d" % slen) == []
    assert A.run_repair(dev, t, ref, [4], corrupt=(ns - 1, 8, slen - 1, 2),
                        what="repair corrupt %d" % slen) == [ns - 1]
print("knob parity OK")
"""

SETTINGS = [
    {"GFRS_NT": "1"},
    {"GFRS_RS_SEQ": "1", "GFRS_RS_GRID": "3"},
    {"GFRS_RP_WAVES": "3"},
    {"GFRS_RP_WAVES": "4"},
    {"GFRS_CRC_CHUNK": "32"},
    {"GFRS_CRC_CHUNK": "128"},
    {"GFRS_CRC_CHUNK": "256"},
    {"GFRS_SMALL_MAX": "4096"},
    {"GFRS_FUSED_MIN": "1048576"},
]


@pytest.mark.parametrize(
    "setting", SETTINGS,
    ids=["-".join("%s=%s" % kv for kv in s.items()) for s in SETTINGS])
def test_knob_parity(setting):
    env = dict(os.environ, **setting)
    r = subprocess.run([sys.executable, "-c", _SCRIPT], env=env, cwd=_REPO,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (setting, r.stdout[-2000:], r.stderr[-3000:])
    assert "knob parity OK" in r.stdout
