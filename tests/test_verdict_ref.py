"""CPU check of the reference verdict helper (tests/_verdict.py) and of
every input the GPU verdict sweeps use: the oracle alone must behave as
tests/test_gpu_verdict_sweep.py and tests/test_gpu_verdict_crc.py assume.

Plain RS: a stripe with one flipped bit fails Reconstruct+Verify exactly
when the corrupted column is a survivor and nbad < m (an MDS code with a
spare equation detects any single-column error; with nbad == m no equation
is left, and a flip in an erased column is overwritten).
LRC: the verdict is recorded as the oracle computes it; it must be
deterministic and a clean stripe never fails.
"""
import numpy as np
import pytest

import _verdict as V
from _verdict import oracle

BLOCKS = [65536, 4096, 8192]


def test_pattern_counts():
    n = {name: {g: len(c) for g, c in V.exhaustive(name).items()}
         for name in V.TACTICS}
    # 6+3: all 129 patterns with 1 <= nbad <= m, plus one undecodable
    assert n["EC6P3"] == {"nbad1": 9, "nbad2": 36, "nbad3": 84 + 1}
    assert n["EC4P2"] == {"nbad1": 6, "nbad2": 15 + 1}
    assert n["EC3P3"] == {"nbad1": 6, "nbad2": 15, "nbad3": 20 + 1}
    assert n["EC12P4"] == {"nbad1": 16, "nbad2": 120, "nbad3": 48,
                           "nbad4": 48 + 1}
    assert n["EC13P4"] == {"nbad1": 17, "nbad2": 136, "nbad3": 48,
                           "nbad4": 48 + 1}
    assert n["EC6P6"] == {"nbad1": 12, "nbad2": 66, "nbad3": 48, "nbad4": 48,
                          "nbad5": 48, "nbad6": 48 + 1}
    assert n["LRC12P2L2"] == {"nbad1": 16, "nbad2": 120, "nbad3-4": 64 + 1}
    assert n["EC6P3L3"] == {"nbad1": 12, "nbad2": 66, "nbad3-4": 64 + 1}
    assert n["EC4P4L2"] == {"nbad1": 10, "nbad2": 45, "nbad3-4": 64 + 1}
    for name in V.TACTICS:
        t = V.get_tactic(name)
        sub = V.subset(name)
        assert len(sub) == 12 and len({frozenset(p) for p in sub}) == 12
        assert any(len(p) == t.M for p in sub)
        assert any(max(p) < t.N for p in sub)                 # data only
        assert any(t.N <= min(p) < t.N + t.M and max(p) < t.N + t.M
                   for p in sub)                              # parity only
        assert any(min(p) < t.N <= max(p) for p in sub)       # mixed
        assert any(list(p) != sorted(p) for p in sub)         # caller order
        if t.L:
            assert any(max(p) >= t.N + t.M for p in sub)      # a lost local
        g = V.groups(name)
        assert ("len70005" in g) == (name in V.FUSED_REPAIR)
        # sorted first, reversed second, same rotation
        c = g["nbad2"]
        assert c[0][1] == c[1][1][::-1] and c[0][2] == c[1][2]


def test_position_lists():
    assert V.rs_positions(33) == [0, 15, 16, 31, 32]
    assert V.rs_positions(4093) == [0, 15, 16, 4079, 4080, 4092]
    assert V.rs_positions(8209) == [0, 15, 16, 8207, 8208, 4095, 4096]
    assert V.rs_positions(70005) == [0, 15, 16, 69999, 70000, 70004, 4095,
                                     4096, 16383, 16384, 65531, 65532]
    assert V.payload_positions(100, 65536) == [0, 99]
    assert V.payload_positions(65533, 65536) == [
        0, 4095, 4096, 16383, 16384, 49151, 49152, 65531, 65532]
    assert V.payload_positions(65532, 65536)[-1] == 65531


@pytest.mark.parametrize("name", V.TACTICS)
def test_sweep_verdicts(name):
    t = V.get_tactic(name)
    total = t.N + t.M + t.L
    seen_fail = seen_pass = seen_undec = 0
    masks, cols = set(), set()
    for grp, cases in V.groups(name).items():
        for slen, bad, rot in cases:
            if list(bad) != sorted(bad) and slen == 33:
                continue    # reversed twin: same erasures, same verdict
            cor = V.corrupt(t, slen, rot)
            ref = V.A.ref_stripes(t, total + 1, slen, seed=11)
            diff = cor ^ ref
            # exactly one bit per corrupted stripe, in its own column
            for s in range(total):
                nz = np.argwhere(diff[s])
                assert len(nz) == 1 and nz[0][0] == s
                assert nz[0][1] in V.rs_positions(slen)
                m = int(diff[s][tuple(nz[0])])
                assert m & (m - 1) == 0
                masks.add(m)
                cols.add((s, int(nz[0][1])) if slen == 33 else None)
            assert not diff[total].any()
            exp = V.verdicts(t, cor, bad)
            glob = sum(1 for b in bad if b < t.N + t.M)
            if exp == V.UNDECODABLE:
                assert glob > t.M, (name, bad)
                seen_undec += 1
                continue
            assert glob <= t.M, (name, bad)
            rec, fails = exp
            assert total not in fails, (name, bad)   # clean stripe
            if t.L == 0:
                want = [s for s in range(total)
                        if s not in bad and len(bad) < t.M]
                assert fails == want, (name, slen, bad, fails)
            else:
                again = V.verdicts(t, cor, bad)
                assert again[1] == fails
                assert np.array_equal(again[0], rec)
                assert not set(fails) & set(bad), (name, bad, fails)
            # the clean stripe reconstructs to the original
            assert np.array_equal(rec[total], ref[total])
            seen_fail += len(fails)
            seen_pass += total + 1 - len(fails)
    assert seen_fail and seen_pass and seen_undec
    assert len(masks) == 8
    # over the exhaustive sweep every column meets every position
    assert {c for c in cols if c} == {
        (s, p) for s in range(total) for p in V.rs_positions(33)}


@pytest.mark.parametrize("name,slen", V.WIDE)
def test_wide_batch(name, slen):
    t = V.get_tactic(name)
    cor = V.wide_batch(t, slen)
    every_third = list(range(0, V.WIDE_NS, 3))
    assert V.verdicts(t, cor, [])[1] == every_third
    bad = [2, t.N + 2]
    total = t.N + t.M
    want = [s for s in every_third if (s // 3) % total not in bad]
    assert V.verdicts(t, cor, bad)[1] == want
    assert {s // 64 for s in want} == {0, 1, 2}      # all three bitmap words


def _raw(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


@pytest.mark.parametrize("block_len", BLOCKS)
def test_crc_cases(block_len):
    for n in V.CRC_SIZES:
        framed = oracle.crc32b_encode(_raw(n, n), block_len)
        pl = block_len - 4
        nf = (n + pl - 1) // pl
        names = [c[0] for c in V.crc_cases(n, block_len)]
        assert len(set(names)) == len(names)
        for cname, flips in V.crc_cases(n, block_len):
            img = V.apply_flips(framed, flips)
            got = oracle.crc32b_verify(img, block_len)
            if not flips:
                assert got == -1
            elif len(flips) == 2:
                lo = 1 if nf > 2 else 0
                assert got == lo, (n, cname, got)    # the lower index
            else:
                assert got == flips[0][0] // block_len, (n, cname, got)
    # the interesting offsets exist where the frame is long enough
    names = [c[0] for c in V.crc_cases(3 * 65532 + 5, 65536)]
    for want in ("crc0[3]", "crcN[0]", "payload[0]", "payload[4095]",
                 "payload[16384]", "payload[49152]", "payload[65531]",
                 "payload[196600]", "blocks 1+3", "clean"):
        assert want in names, want


def test_sized_cases():
    for n in V.SIZED_SIZES:
        framed, tail = oracle.sized_encode(_raw(n, n + 1))
        body = framed.size - tail
        for cname, flips in V.sized_cases(n, 65536):
            img = V.apply_flips(framed, flips)
            got = oracle.sized_verify(img, tail)
            if not flips or cname == "tail pad":
                # the pad is outside every frame: the reference ignores it
                assert got == -1, (n, cname, got)
                assert cname != "tail pad" or flips[0][0] >= body
            elif len(flips) == 2:
                assert got == (1 if body > 2 * 65536 else 0), (n, cname)
            else:
                assert got == flips[0][0] // 65536, (n, cname, got)
    assert any(c[0] == "tail pad" for c in V.sized_cases(200001, 65536))


@pytest.mark.parametrize("slen", [100, 70005])
def test_shard_cases(slen):
    img = oracle.shard_write(_raw(slen, 5), bid=77, vuid=88)
    for cname, flips in V.shard_cases(slen):
        bad, bid, vuid, size = V.shard_parse_ref(V.apply_flips(img, flips))
        assert bad == bool(flips), cname
        if not flips:
            assert (bid, vuid, size) == (77, 88, slen)
