"""Aligned fused encode+frame kernel (GFRS_EF=79, rs_encode_frame_al_k):
the 12-gather piece form of a full frame's CRC chain.  A piece enters the
chain as u(piece) = two dwords reduced over the slice-by-8 tables, the
third over four of them, the fourth raw, and the lane's fold operator
carries the missing x^32.  Each dword of a piece takes a different way into
u, so a single nonzero byte is put at every byte position of one chunk, in
two frames with different rotations; every framed image is compared byte for
byte with the CPU oracle.  GFRS_EF_CRC16=1 runs the 16+4-gather form of the
same build, which must give the same bytes.  GFRS_EF=76 runs the same
cases through rs_encode_frame_reg_k, which builds its per-pass chains from
the same 12-gather pieces.

The knobs are read once per process, so each variant runs in a subprocess;
one subprocess checks a whole group.
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


# (mode, shard_len, stripes, [[shard, shard offset], ...] | null, values)
for name, slen, ns, hot, vals in json.loads(sys.argv[1]):
    t = codemode.get_tactic(name)
    if hot is None:
        rng = np.random.default_rng(slen ^ t.N ^ 12)
        check(name, slen, rng.integers(0, 256, (ns, t.total, slen),
                                       dtype=np.uint8))
        continue
    for c, p in hot:
        for v in vals:
            arr = np.zeros((ns, t.total, slen), dtype=np.uint8)
            arr[0, c, p] = v
            try:
                check(name, slen, arr)
            except AssertionError as e:
                raise AssertionError(("single byte", c, p, hex(v), e.args))
print("aligned crc12 parity OK")
"""


def _chunk(h, w, i, lane):
    """image chunk of pass h, wave w, piece i, lane"""
    return 1024 * h + 256 * w + 64 * i + lane


# 131072-B shards: frames 0 and 1 are full (rotations r = 3 and 2), the
# 8-B rest is the folded tiny frame.  Image byte b of chunk q of frame f is
# payload offset 16q - 4 + b, shard offset 65532 f + 16q - 4 + b.  Both
# chunks are away from lanes 0 and 63 and from a wave's first piece.
_Q0 = _chunk(1, 2, 1, 21)
_Q1 = _chunk(2, 1, 3, 37)
_HOT = [[0, 16 * _Q0 - 4 + b] for b in range(16)] + \
       [[2, 65532 + 16 * _Q1 - 4 + b] for b in range(16)]
_ONEBYTE = [("EC6P3", 131072, 1, _HOT, [0x01, 0x80, 0xA5])]

# five full frames and a two-pass ragged one x 3 stripes (GM = 3); two full
# frames and a 72-B last frame x 2 stripes (GM = 4, k + GM = 16)
_RANDOM = [("EC6P3", 365536, 3, None, None),
           ("EC12P4", 131136, 2, None, None)]

_VARIANTS = [pytest.param({}, id="auto"),
             pytest.param({"GFRS_EF": "79"}, id="ef79"),
             pytest.param({"GFRS_EF": "79", "GFRS_EF_CRC16": "1"},
                          id="ef79-crc16"),
             pytest.param({"GFRS_EF": "76"}, id="ef76")]


def _run(cases, env_set):
    env = {k: v for k, v in os.environ.items()
           if k not in ("GFRS_EF", "GFRS_EF_ABL", "GFRS_EF_C0",
                        "GFRS_EF_CRC16", "GFRS_CRC_GRID")}
    env.update(env_set)
    r = subprocess.run([sys.executable, "-c", _SCRIPT, json.dumps(cases)],
                       env=env, cwd=_REPO, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (env_set, r.stdout[-2000:], r.stderr[-2000:])


@pytest.mark.parametrize("env_set", _VARIANTS)
def test_single_byte_at_every_position_of_a_chunk(env_set):
    """All-zero source but one byte: a wrong table slice for that byte, or a
    wrong operator, cannot cancel out."""
    _run(_ONEBYTE, env_set)


@pytest.mark.parametrize("env_set", _VARIANTS)
def test_random_shards(env_set):
    _run(_RANDOM, env_set)
