"""Aligned fused encode+frame kernel (GFRS_EF=79, rs_encode_frame_al_k):
state carried across passes and across frames.  A full frame's CRC is one
Horner chain per lane and shard, parked between passes in an LDS slab
[k+GM][256] and folded by the lane's position operator once per shard.
Every framed image is compared byte for byte with the CPU oracle, so a
running value or slab entry that is not reset, a wrong inter-pass step or a
wrong fold operator shows up as a header mismatch.

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


def check(name, slen, arr):
    t = codemode.get_tactic(name)
    ns = arr.shape[0]
    batch = torch.from_numpy(arr).to("cuda:0")
    assert batch.data_ptr() % 16 == 0
    enc_sz = crc32block.encode_size(slen)
    stride = (enc_sz + 255) // 256 * 256
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
                raise AssertionError((name, slen, s, j, int(bad[0]),
                                      int(bad[-1]), len(bad)))
        assert not got[s * t.total:(s + 1) * t.total, enc_sz:].any(), \
            (name, slen, "bytes written past the image")


# (mode, shard_len, stripes, payload offsets of a single nonzero byte | null)
for name, slen, ns, hot in json.loads(sys.argv[1]):
    t = codemode.get_tactic(name)
    if hot is None:
        rng = np.random.default_rng(slen ^ t.N)
        check(name, slen, rng.integers(0, 256, (ns, t.total, slen),
                                       dtype=np.uint8))
    else:
        for p in hot:
            arr = np.zeros((ns, t.total, slen), dtype=np.uint8)
            arr[0, 0, p] = 0xA5
            try:
                check(name, slen, arr)
            except AssertionError as e:
                raise AssertionError(("single byte at payload offset", p,
                                      e.args))
print("aligned fold parity OK")
"""

# five full frames (r = 3, 2, 1, 0, 3), then a two-pass ragged frame:
# 5 * 65532 + 37872 = 365532, rounded up to a multiple of 16
_CHAIN = [("EC6P3", 365536, 3, None)]

# k + GM = 16 and GM = 1: two full frames and a short last frame.  Two full
# frames are 131064 B = 8 (mod 16), so an 80-B last frame gives a shard
# length the aligned kernel is not eligible for (131144, kept: the launch
# must still produce the same bytes through the kernel it used before);
# the nearest eligible lengths have a 72-B or 88-B last frame.
_WIDE = [(m, n, 2, None)
         for m in ("EC12P4", "LRC12P2L2", "EC6P1")
         for n in (131144, 131136, 131152)]

# one nonzero source byte in frame 0 of a 131072-B shard: first and last
# byte of each pass (image offset = payload offset + 4, a pass is 16384
# image bytes, chunk 0 holds payload bytes 0..11), and first and last lane
# of each wave (wave w of pass 0 starts at image byte 4096 w)
_HOT = sorted({0, 11, 12, 16379, 16380, 32763, 32764, 49147, 49148, 65531} |
              {4096 * w + d for w in (1, 2, 3)
               for d in (-16, 0, 16, -20, -5, -4, 11)})
_ONEBYTE = [("EC6P3", 131072, 1, _HOT)]


def _run(cases, **env_set):
    env = {k: v for k, v in os.environ.items()
           if k not in ("GFRS_EF", "GFRS_EF_ABL", "GFRS_EF_C0",
                        "GFRS_CRC_GRID")}
    env.update(env_set)
    r = subprocess.run([sys.executable, "-c", _SCRIPT, json.dumps(cases)],
                       env=env, cwd=_REPO, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (env_set, r.stdout[-2000:], r.stderr[-2000:])


def _env(ef, **more):
    env = dict(more)
    if ef:
        env["GFRS_EF"] = ef
    return env


@pytest.mark.parametrize("grid", ["1", "2", "5"])
@pytest.mark.parametrize("ef", ["79", None], ids=["ef79", "auto"])
def test_chain_and_slab_under_gridstride(ef, grid):
    """One, two or five blocks walk 3 x 6 frames, so a block meets full ->
    ragged -> full frames across stripe boundaries."""
    _run(_CHAIN, **_env(ef, GFRS_CRC_GRID=grid))


@pytest.mark.parametrize("grid", ["1", "5"])
def test_chain_with_chunk0_in_lds(grid):
    _run(_CHAIN, GFRS_EF="79", GFRS_EF_C0="1", GFRS_CRC_GRID=grid)


@pytest.mark.parametrize("ef", ["79", None], ids=["ef79", "auto"])
def test_slab_indexing_at_its_widest(ef):
    _run(_WIDE, **_env(ef))


@pytest.mark.parametrize("ef", ["79", None], ids=["ef79", "auto"])
def test_single_byte_positions(ef):
    """All-zero source but one byte: a wrong operator cannot cancel out."""
    _run(_ONEBYTE, **_env(ef))


def test_single_byte_positions_chunk0_in_lds():
    _run(_ONEBYTE, GFRS_EF="79", GFRS_EF_C0="1")
