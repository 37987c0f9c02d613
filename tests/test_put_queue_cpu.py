"""CPU checks of the put queue (gfrs_put_queue):

 - the schedule the engine would upload (gfrs_compute_put_queue_schedule, the
   same builder, GPU-free) for every queue of tests/_putq.py and for a
   hundred seeded random ones: job classes, buckets, caller order, prefix
   sums, img = img_off + 32, the row groups and the image table;
 - the validation codes of the contract (include/gfrs.h);
 - `wide` for every mode of the registry;
 - the sanitized stand-alone selftest of the builder
   (put_queue_selftest.cpp);
 - the oracle alone on every queue the GPU module runs: every expected image
   parses to its ids, its body decodes to its shard and the decoded stripe
   verifies, so the GPU tests compare against something self-consistent.
"""
import os
import subprocess

import numpy as np
import pytest

import _arena as A
import _encq as E
import _putq as P
from _arena import oracle
from test_queue_cpu import _host_compiler

from cubefs_amd import codemode

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "cubefs_amd", "csrc")


def check_schedule(t, jobs, vuids, s):
    """Every property the kernels and the host rely on.  jobs: (off, slen,
    img_off, img_stride, bid, vol)."""
    total = t.N + t.M + t.L
    wide = P.wide_gate(t)
    assert s.wide == int(wide)
    assert s.group_rows == P.group_rows(t)
    assert sum(s.group_rows) == t.M + t.L
    assert all(r == 4 for r in s.group_rows[:-1])
    assert s.group_rows[-1] == t.M + t.L - 4 * (len(s.group_rows) - 1)
    order = [(E.KIND_SMALL, ni) for ni in (1, 2, 3, 4)] + \
        [(E.KIND_FRAME, E.VAR_BELOW), (E.KIND_FRAME, E.VAR_FROM)]
    keys = [(kind, param) for kind, param, _, _ in s.buckets]
    assert len(keys) <= (2 if wide else E.MAX_BUCKETS)
    assert keys == [k for k in order if k in keys]
    if wide:
        assert all(kind == E.KIND_FRAME for kind, _ in keys)
    seen = []
    at = pre = 0
    for kind, param, first, count in s.buckets:
        assert first == at and count > 0
        at += count
        last_job = -1
        if kind == E.KIND_FRAME:
            sums = s.prefix[pre:pre + count + 1]
            assert sums[0] == 0
            pre += count + 1
        for i in range(count):
            job, off, slen, img, stride, reserved = s.items[first + i]
            assert (off, slen, stride) == (jobs[job][0], jobs[job][1],
                                           jobs[job][3])
            assert img == jobs[job][2] + 32       # behind the header
            assert reserved == 0
            assert P.bucket_of(t, slen) == (kind, param), (job, slen)
            assert job > last_job                 # caller order in a bucket
            last_job = job
            seen.append(job)
            if kind == E.KIND_FRAME:
                assert sums[i + 1] - sums[i] == E.frames(slen)
    assert at == len(s.items) and pre == len(s.prefix)
    assert sorted(seen) == list(range(len(jobs)))
    # the image table: job-major, shard order
    assert len(s.images) == len(jobs) * total
    for j, (off, slen, img_off, stride, bid, vol) in enumerate(jobs):
        for i in range(total):
            assert s.images[j * total + i] == \
                (img_off + i * stride, slen, bid, vuids[vol][i]), (j, i)


@pytest.mark.parametrize("name", P.GPU_QUEUES)
def test_schedule_of_gpu_queues(name):
    q = P.build(name)
    rc, s = P.schedule(q.t, q.jobs, q.vuids)
    assert rc == 0
    check_schedule(q.t, q.jobs, q.vuids, s)
    keys = [(k, p) for k, p, _, _ in s.buckets]
    lens = {j[1] for j in q.jobs}
    want = {"rs63": (0, [3]), "rs66": (1, [4, 2]), "rs1512": (1, [4, 4, 4]),
            "rs164": (1, [4]), "rs248": (1, [4, 4]), "lrc442": (1, [4, 2]),
            "lrc16202": (1, [4, 4, 4, 4, 4, 2]), "rs324": (1, [4])}[name]
    assert (s.wide, s.group_rows) == want
    if name == "rs63":
        assert len(keys) == 5 and lens >= set(E.SMALL + E.NI3 + E.FRAME)
    if name == "rs66":
        assert keys == [(E.KIND_FRAME, E.VAR_BELOW), (E.KIND_FRAME, E.VAR_FROM)]
        assert lens == set(P.WIDE_FRAME + P.LARGE)
    if name in ("rs1512", "rs164", "lrc442"):
        assert keys == [(E.KIND_FRAME, E.VAR_BELOW)]
        assert lens == set(P.WIDE_FRAME)
    # at least two vuid sets and a distinct bid per job
    assert len({j[5] for j in q.jobs}) >= 2
    assert len({j[4] for j in q.jobs}) == len(q.jobs)
    assert len(set(q.flat_vuids())) == P.NVOL * q.total


def _random_jobs(rng, total):
    pick = [1, 2, 15, 16, 17, 1023, 1024, 1025, 2049, 3072, 3073, 4095, 4096,
            4097, 65531, 65532, 65533, 65596, 131064, 131065, (1 << 20) - 1,
            1 << 20, (1 << 20) + 1, 8 << 20, (1 << 32) - 1]
    nj = int(rng.integers(1, 40))
    jobs, off, img = [], int(rng.integers(0, 64)), 4 * int(rng.integers(0, 9))
    for j in range(nj):
        if rng.integers(0, 3) == 0:
            slen = int(rng.integers(1, 200000))
        else:
            slen = pick[int(rng.integers(0, len(pick)))]
        stride = E.round4(A.disk_size(slen)) + 4 * int(rng.integers(0, 3))
        jobs.append((off, slen, img, stride, int(rng.integers(0, 1 << 62)),
                     int(rng.integers(0, P.NVOL))))
        off += 6 * slen + int(rng.integers(0, 16))
        img += total * stride + 4 * int(rng.integers(0, 5))
    return jobs


def test_schedule_of_random_queues():
    rng = np.random.default_rng(0x9C7E)
    tactics = [codemode.get_tactic(n) for n in
               ("EC6P3", "EC6P6", "EC15P12", "EC4P4L2", "EC12P4")]
    nbuckets = set()
    for r in range(100):
        t = tactics[r % len(tactics)]
        vuids = P.vuid_sets(t.total)
        jobs = _random_jobs(rng, t.total)
        rc, s = P.schedule(t, jobs, vuids)
        assert rc == 0
        check_schedule(t, jobs, vuids, s)
        nbuckets.add((s.wide, len(s.buckets)))
    assert {w for w, _ in nbuckets} == {0, 1}
    assert max(n for w, n in nbuckets if w) == 2


def test_wide_of_registry_modes():
    """Four of the fifteen EC modes pass the gate of the fused encode
    kernels; the put queue serves all fifteen."""
    narrow = []
    for code in codemode.ec_code_modes():
        name = codemode.get_name(code)
        t = codemode.get_tactic(name)
        if code > 15:     # the fifteen pre-defined modes, codes 1..15
            continue
        size = A.disk_size(100)
        rc, s = P.schedule(t, [(0, 100, 0, size, 1, 0)])
        assert rc == 0, name
        assert s.wide == int(P.wide_gate(t)), name
        assert s.group_rows == P.group_rows(t), name
        assert len(s.images) == t.total
        if not s.wide:
            narrow.append(name)
    assert sorted(narrow) == ["EC10P4", "EC12P4", "EC3P3", "EC6P3"]


def test_schedule_validation():
    t = codemode.get_tactic("EC6P3")
    t66 = codemode.get_tactic("EC6P6")
    sz = A.disk_size(100)
    assert sz == 144
    good = (0, 100, 0, sz, 9, 0)
    ok = [good]

    def one(**f):
        d = dict(off=0, slen=100, img_off=0, stride=sz, bid=9, vol=0,
                 reserved=0)
        d.update(f)
        return [good, (d["off"], d["slen"], d["img_off"], d["stride"],
                       d["bid"], d["vol"], d["reserved"])]

    for tt in (t, t66):
        assert P.schedule(tt, ok)[0] == 0
        # block length: crc32block's code first, then the queues'
        for bl in (0, -65536, 100, 65536 + 4):
            assert P.schedule(tt, ok, block_len=bl)[0] == P.ERR_BLOCK
        for bl in (4096, 131072, 65536 * 3):
            assert P.schedule(tt, ok, block_len=bl)[0] == P.ERR_UNSUPPORTED
        assert P.schedule(tt, [])[0] == P.ERR_INVALID              # njobs <= 0
        assert P.schedule(tt, ok, nvol=0)[0] == P.ERR_INVALID
        assert P.schedule(tt, ok, nvol=-1)[0] == P.ERR_INVALID
        assert P.schedule(tt, one(vol=P.NVOL))[0] == P.ERR_INVALID
        assert P.schedule(tt, one(vol=-1))[0] == P.ERR_INVALID
        assert P.schedule(tt, one(vol=P.NVOL - 1))[0] == 0
        assert P.schedule(tt, one(reserved=1))[0] == P.ERR_INVALID
        assert P.schedule(tt, one(slen=0))[0] == P.ERR_NO_DATA
        assert P.schedule(tt, one(slen=1 << 32, stride=1 << 33))[0] == \
            P.ERR_INVALID
        big = (1 << 32) - 1
        assert P.schedule(tt, one(slen=big, stride=E.round4(
            A.disk_size(big))))[0] == 0
        # images: alignment of img_off and img_stride, stride below the size
        assert P.schedule(tt, one(img_off=2))[0] == P.ERR_INVALID
        assert P.schedule(tt, one(stride=sz + 2))[0] == P.ERR_INVALID
        assert P.schedule(tt, one(stride=sz - 4))[0] == P.ERR_INVALID
        assert P.schedule(tt, one(slen=101))[0] == P.ERR_INVALID
        assert P.schedule(tt, one(off=7, img_off=4 * sz, stride=sz + 4))[0] \
            == 0
        # a second frame adds its 4-byte CRC to the image
        two = A.disk_size(65533)
        assert two == 65533 + 8 + 40
        assert P.schedule(tt, one(slen=65533, stride=E.round4(two) - 4))[0] \
            == P.ERR_INVALID
        assert P.schedule(tt, one(slen=65533, stride=E.round4(two)))[0] == 0
        # capacities
        assert P.schedule(tt, one(), item_cap=1)[0] == P.ERR_NOMEM
        assert P.schedule(tt, one(), image_cap=2 * tt.total - 1)[0] == \
            P.ERR_NOMEM
    # the width of the tactic: n = 32 is served, n = 33 and replicas are not
    assert P.schedule(P.rs324_tactic(), ok)[0] == 0
    assert P.schedule(P.rs334_tactic(), ok)[0] == P.ERR_UNSUPPORTED
    assert P.schedule(codemode.get_tactic("Replica3"), ok)[0] == \
        P.ERR_UNSUPPORTED
    # ... after the block length
    assert P.schedule(P.rs334_tactic(), ok, block_len=0)[0] == P.ERR_BLOCK


def test_put_queue_selftest_sanitized(tmp_path):
    """The put schedule builder under ASan + UBSan as a stand-alone program:
    a plain host compiler, gfrs_plan.cpp + gfrs_gf.cpp, no Python in the
    process."""
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host compiler with the sanitizer runtimes")
    exe = str(tmp_path / "put_queue_selftest")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall",
                    "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    os.path.join(HERE, "put_queue_selftest.cpp"),
                    os.path.join(CSRC, "gfrs_plan.cpp"),
                    os.path.join(CSRC, "gfrs_gf.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "put queue selftest OK" in r.stdout


def test_oracle_encodes_the_tactics():
    """The oracle encodes every (n, m[, l]) the queues use, and shard_parse
    returns the ids shard_write was given."""
    for n, m, l, az in [(6, 6, 0, 3), (15, 12, 0, 3), (16, 4, 0, 1),
                        (24, 8, 0, 1), (32, 4, 0, 1), (4, 4, 2, 2),
                        (16, 20, 2, 2)]:
        rng = np.random.default_rng(n * 100 + m)
        sh = [rng.integers(0, 256, 333, dtype=np.uint8)
              for _ in range(n + m + l)]
        if l:
            oracle.lrc_encode(n, m, l, az, sh)
        else:
            oracle.rs_encode(n, m, sh)
        assert oracle.rs_verify(n, m, sh[:n + m]), (n, m, l)
        for i in (0, n, n + m + l - 1):
            img = oracle.shard_write(sh[i].copy(), bid=77 + i, vuid=(9 << 40) + i)
            assert oracle.shard_parse(img) == (77 + i, (9 << 40) + i, 333)


@pytest.mark.parametrize("name", P.GPU_QUEUES)
def test_gpu_queues_against_oracle(name):
    """What tests/test_gpu_put_queue.py assumes of its inputs."""
    q = P.build(name)
    t = q.t
    exp = P.expectations(name)
    assert len(exp) == len(q.jobs) >= 3
    for j, (off, slen, img_off, stride, bid, vol) in enumerate(q.jobs):
        imgs, crcs = exp[j]
        assert len(imgs) == len(crcs) == q.total
        shards = []
        for i, img in enumerate(imgs):
            assert img.size == A.disk_size(slen)
            assert oracle.shard_parse(img) == (bid, q.vuids[vol][i], slen)
            raw = oracle.crc32b_decode(img[P.HEADER:-P.FOOTER].copy())
            assert np.array_equal(raw, q.data[j][i]), (name, j, i)
            assert crcs[i] == oracle.crc32(raw)
            # the footer carries the same value, big-endian
            assert int.from_bytes(bytes(img[-4:]), "big") == crcs[i]
            shards.append(raw)
        # LRC: the global stripe verifies; the local parities are covered by
        # the decode comparison with the oracle's own lrc_encode above
        assert oracle.rs_verify(t.N, t.M, shards[:t.N + t.M]), (name, j)
        assert stride % 4 == 0 and stride >= A.disk_size(slen)
    # odd base, odd gaps, jobs do not overlap; data shards only, so the
    # arena ends with shard n-1 of the last job
    assert q.delta % 2 == 1
    end = 0
    gaps = set()
    for job in q.jobs:
        off, slen = job[0], job[1]
        assert off >= end
        if end:
            gaps.add(off - end)
        end = off + t.N * slen
    assert end == q.nbytes and all(g % 2 for g in gaps) and len(gaps) >= 2
    # images: 4-aligned, disjoint, inside the arena
    spans = sorted(reg for j in range(len(q.jobs))
                   for reg in q.image_regions(j))
    assert all(off % 4 == 0 for off, _ in spans)
    assert all(a[0] + a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    assert spans[-1][0] + spans[-1][1] == q.img_bytes
    # image order is not job order; tight and padded strides
    firsts = [job[2] for job in q.jobs]
    assert firsts != sorted(firsts)
    slack = [job[3] - E.round4(A.disk_size(job[1])) for job in q.jobs]
    assert 0 in slack and max(slack) > 0
