"""Aligned fused encode+frame kernel (GFRS_EF=79, rs_encode_frame_al_k):
destination-space 16-B chunks, aligned loads and stores, one-lane DPP
rotation.  Every framed image is compared byte for byte with the CPU oracle
(encoder.go:114 Encode + crc32block encode.go:48-109 framing), so a
mis-rotated dword, a wrong wave-edge donor or a slipped CRC position
operator shows up as a payload or header mismatch.

GFRS_EF is read once per process, so each forced variant runs in a
subprocess; one subprocess checks a whole group of shapes.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SCRIPT = r"""
import json
import sys
import numpy as np
import torch
from cubefs_amd import codemode, crc32block, ec
from oracle import pyoracle as oracle

codemode.extend(240, "LRC12P2L2", codemode.Tactic(12, 2, 2, 2, 14, 0, 2048))
codemode.extend(241, "EC6P1", codemode.Tactic(6, 1, 0, 1, 6, 0, 2048))
# (mode, shard_len, stripes, padded image stride, source byte offset)
for name, slen, ns, pad, off in json.loads(sys.argv[1]):
    t = codemode.get_tactic(name)
    rng = np.random.default_rng(slen ^ t.N ^ (off << 20))
    arr = rng.integers(0, 256, (ns, t.total, slen), dtype=np.uint8)
    flat = torch.zeros(arr.size + 16, dtype=torch.uint8, device="cuda:0")
    batch = flat[off:off + arr.size].view(ns, t.total, slen)
    batch.copy_(torch.from_numpy(arr))
    assert batch.data_ptr() % 16 == off
    enc_sz = crc32block.encode_size(slen)
    stride = (enc_sz + 255) // 256 * 256 if pad else enc_sz
    framed = torch.zeros((ns * t.total, stride), dtype=torch.uint8,
                         device="cuda:0")
    enc = ec.Encoder(t)
    enc.encode_frame_batch(framed, batch)
    enc.synchronize()
    got = framed.cpu().numpy()
    for s in range(ns):
        sh = [arr[s, i].copy() for i in range(t.total)]
        oracle.lrc_encode(t.N, t.M, t.L, t.AZCount, sh)
        for j in range(t.total):
            want = oracle.crc32b_encode(sh[j])
            if not np.array_equal(got[s * t.total + j, :enc_sz], want):
                bad = np.flatnonzero(got[s * t.total + j, :enc_sz] != want)
                raise AssertionError((name, slen, pad, off, s, j,
                                      int(bad[0]), int(bad[-1]), len(bad)))
        assert not got[s * t.total:(s + 1) * t.total, enc_sz:].any(), \
            (name, slen, "bytes written past the image")
print("aligned frame parity OK")
"""

# all shard lengths are multiples of 16 (eligible with the padded stride)
_ELIGIBLE = [
    ("EC6P3", 262128, 3, 1, 0),    # 4 full frames: r = 3, 2, 1, 0
    ("EC6P3", 262208, 3, 1, 0),    # last frame 80 B: pass 0 only, 5 chunks
    ("EC6P3", 300000, 3, 1, 0),    # last frame 37872 B: 2 passes + 5104 B
    ("EC6P3", 262144, 3, 1, 0),    # 16-B last frame: tiny fold after 4
    ("EC6P3", 65536, 3, 1, 0),     # 4-B tiny fold on frame 0
    ("EC6P3", 1 << 20, 3, 1, 0),   # auto threshold: 16 frames + 64-B fold
    ("EC6P3", 5008, 3, 1, 0),      # a single short frame
    ("EC12P4", 262128, 3, 1, 0),   # GM = 4, k = 12
    ("LRC12P2L2", 262128, 3, 1, 0),  # composed GM = 4
    ("EC6P1", 262128, 3, 1, 0),    # GM = 1, m = 1
]

_INELIGIBLE = [
    ("EC6P3", 65532, 3, 1, 0),
    ("EC6P3", 5000, 3, 1, 0),
    ("EC6P3", 17, 3, 1, 0),
    ("EC6P3", 262128, 3, 0, 0),    # tight image stride
    ("EC6P3", 262128, 3, 1, 4),    # source view 4 bytes into its allocation
]


def _run(cases, **env_set):
    env = {k: v for k, v in os.environ.items()
           if k not in ("GFRS_EF", "GFRS_EF_ABL", "GFRS_EF_C0",
                        "GFRS_CRC_GRID")}
    env.update(env_set)
    r = subprocess.run([sys.executable, "-c", _SCRIPT, json.dumps(cases)],
                       env=env, cwd=_REPO, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (env_set, r.stdout[-2000:], r.stderr[-2000:])


@pytest.mark.parametrize("ef", ["79", None], ids=["ef79", "auto"])
def test_aligned_frame_parity(ef):
    """Eligible layouts under the new id and under the auto policy."""
    _run(_ELIGIBLE, **({"GFRS_EF": ef} if ef else {}))


def test_aligned_frame_chunk0_in_lds():
    """The measured alternative for chunk 0 (GM = 3 only): payload bytes
    0..11 wait in LDS and leave as one aligned uint4 with the header."""
    _run([c for c in _ELIGIBLE if c[0] == "EC6P3"], GFRS_EF="79",
         GFRS_EF_C0="1")


def test_ineligible_shapes_keep_old_path():
    """With the new id forced, layouts that are not 16-B aligned throughout
    produce the same bytes through the kernel they used before."""
    _run(_INELIGIBLE, GFRS_EF="79")


@pytest.mark.parametrize("ef", ["79", None], ids=["ef79", "auto"])
def test_aligned_frame_gridstride(ef):
    """Three blocks walk 20 frames: each block meets frames of different
    rotation and crosses stripes, so leaked per-frame state shows."""
    env = {"GFRS_CRC_GRID": "3"}
    if ef:
        env["GFRS_EF"] = ef
    _run([("EC6P3", 262128, 5, 1, 0)], **env)
