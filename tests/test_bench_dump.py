"""bench.py --dump-outputs: the sampling helpers on CPU tensors, and one
tiny plain run of the command line on the GPU whose dumped frames are
checked against the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bench  # noqa: E402  (repo root is on sys.path via conftest)

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rand(rows, cols, seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.empty((rows, cols), dtype=torch.uint8).random_(
        0, 256, generator=g)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_sample_seeded_and_bounded(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1 << 20)
    monkeypatch.setattr(bench, "DUMP_SEG", 4096)
    big = _rand(200, 20011, 1)[:, :20003]      # strided rows, odd width
    small = _rand(5, 1000, 2)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small},
                           {"fail": ([0, 1, 0, 1], 0),
                            "bad_block": ([-1, 3, -1], -1)})
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["bad_block", "bad_block_nonzero", "big",
                         "big_rowsum", "fail", "fail_nonzero", "small",
                         "small_rowsum"]
    for k in a:
        assert a[k].dtype in (np.float32, np.float64)
        assert np.array_equal(a[k], b[k]), k
    bn = big.numpy()
    # budget is split between the two arrays; 3 segments per sampled row
    assert a["big"].shape == ((1 << 19) // (3 * 4096), 3 * 4096)
    assert a["big"].nbytes <= 4 * (1 << 19)
    assert np.array_equal(a["big"][0, :4096], bn[0, :4096])
    assert np.array_equal(a["big"][-1, -4096:], bn[-1, -4096:])
    assert np.array_equal(a["small"], small.numpy())
    assert np.array_equal(a["big_rowsum"], bn.astype(np.int64).sum(axis=1))
    assert a["fail_nonzero"].tolist() == [2.0]
    assert a["bad_block_nonzero"].tolist() == [1.0]
    assert a["bad_block"].tolist() == [-1.0, 3.0, -1.0]


def test_dump_rowsum_groups_rows(monkeypatch):
    monkeypatch.setattr(bench, "DUMP_ROWS", 7)
    x = _rand(11, 333, 3)
    want = x.numpy().astype(np.int64).sum(axis=1)
    want = np.concatenate([want, [0]]).reshape(6, 2).sum(axis=1)
    got = bench._dump_rowsum(x)
    assert got.dtype == np.float64 and np.array_equal(got, want)


@pytest.mark.gpu
def test_bench_cli_dump_matches_oracle(tmp_path, oracle):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    k, m, S, ns = 6, 3, 128 << 10, 4
    args = [sys.executable, os.path.join(_REPO, "bench.py"), "--gpus", "1",
            "--steps", "3", "--warmup", "1", "--stripes", str(ns),
            "--shard-kib", str(S >> 10)]
    outs = []
    for d in ("a", "b"):
        r = subprocess.run(args + ["--dump-outputs", str(tmp_path / d)],
                           cwd=_REPO, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        res = json.loads(r.stdout.strip().splitlines()[-1])
        assert res["steps"] == 3 and res["ms_per_step"] > 0
        assert res["dtype"] == "u8" and res["unit"] == "GiB/s"
        assert res["cpu_baseline"] is None      # plain run: no CPU leg
        outs.append(_load(tmp_path / d))
    a, b = outs
    assert sorted(a) == ["framed", "framed_rowsum"]
    for name in a:
        assert np.array_equal(a[name], b[name]), name   # seeded inputs
    # small enough to be dumped whole: every frame image must decode, and
    # the decoded parity must be the oracle's parity of the decoded data
    enc_sz = oracle.crc32b_encode_size(S)
    assert a["framed"].shape == (ns * (k + m), enc_sz)
    framed = a["framed"].astype(np.uint8)
    assert np.array_equal(a["framed_rowsum"],
                          framed.astype(np.int64).sum(axis=1))
    for s in range(ns):
        got = [oracle.crc32b_decode(np.ascontiguousarray(framed[s * (k + m) + j]))
               for j in range(k + m)]
        ref = [g.copy() for g in got[:k]] + \
            [np.zeros(S, np.uint8) for _ in range(m)]
        assert any(r.any() for r in ref[:k])
        oracle.rs_encode(k, m, ref)
        for j in range(k + m):
            assert np.array_equal(got[j], ref[j]), (s, j)
