"""CPU checks of the encode+frame queue (gfrs_encode_frame_queue):

 - the schedule the engine would upload (gfrs_compute_encode_queue_schedule,
   the same builder, GPU-free) for every queue of tests/_encq.py and for a few
   hundred seeded random ones: job classes, buckets, caller order, prefix
   sums, image places;
 - the validation codes of the contract (include/gfrs.h);
 - the sanitized stand-alone selftest of the builder
   (encode_queue_selftest.cpp);
 - the oracle alone on every queue the GPU module runs: every expected image
   decodes to its shard and the decoded stripe verifies, so the GPU tests
   compare against something self-consistent.
"""
import os
import subprocess

import numpy as np
import pytest

import _arena as A
import _encq as E
import _verdict as V
from _arena import oracle
from test_queue_cpu import _host_compiler

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "cubefs_amd", "csrc")


def check_schedule(jobs, s):
    """Every property the kernels and the host rely on.  jobs: (off, slen,
    img_off, img_stride)."""
    # buckets: at most 6, small NI ascending, then frame 87, then frame 76
    order = [(E.KIND_SMALL, ni) for ni in (1, 2, 3, 4)] + \
        [(E.KIND_FRAME, E.VAR_BELOW), (E.KIND_FRAME, E.VAR_FROM)]
    keys = [(kind, param) for kind, param, _, _ in s.buckets]
    assert len(keys) <= E.MAX_BUCKETS
    assert keys == [k for k in order if k in keys]
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
            assert (off, slen, img, stride) == tuple(jobs[job][:4])
            assert reserved == 0
            # the class and param its length demands
            assert E.bucket_of(slen) == (kind, param), (job, slen)
            # caller order inside a bucket
            assert job > last_job
            last_job = job
            seen.append(job)
            if kind == E.KIND_FRAME:
                assert sums[i + 1] - sums[i] == E.frames(slen)
    assert at == len(s.items) and pre == len(s.prefix)
    # each job in exactly one bucket
    assert sorted(seen) == list(range(len(jobs)))


@pytest.mark.parametrize("name", E.GPU_QUEUES)
def test_schedule_of_gpu_queues(name):
    q = E.build(name)
    rc, s = E.schedule(q.t, q.jobs)
    assert rc == 0
    check_schedule(q.jobs, s)
    assert s.fused == (0 if name == "rs66_slow" else 1)
    keys = [(k, p) for k, p, _, _ in s.buckets]
    if name == "rs63_mixed":
        assert len(keys) == 6
        assert {j[1] for j in q.jobs} >= set(E.SMALL + E.FRAME + E.LARGE)
    if name == "rs63_small":
        assert keys == [(E.KIND_SMALL, ni) for ni in (1, 2, 3, 4)]
        # more jobs than 4 x grid waves when the grid is forced to 1 or 3
        assert all(count > 12 for _, _, _, count in s.buckets)
    if name in ("rs42", "rs124_k12", "lrc_fused"):
        assert len(keys) == 5 and (E.KIND_FRAME, E.VAR_FROM) not in keys
    # neighbours in a bucket differ in length
    for _, _, first, count in s.buckets:
        lens = [s.items[first + i][2] for i in range(count)]
        assert all(a != b for a, b in zip(lens, lens[1:])), (name, lens)


def _random_jobs(rng):
    pick = [1, 2, 15, 16, 17, 1023, 1024, 1025, 2047, 2048, 2049, 3072, 3073,
            4095, 4096, 4097, 65531, 65532, 65533, 65596, 131064, 131065,
            (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 8 << 20]
    nj = int(rng.integers(1, 40))
    jobs, off, img = [], int(rng.integers(0, 64)), 4 * int(rng.integers(0, 9))
    for _ in range(nj):
        if rng.integers(0, 3) == 0:
            slen = int(rng.integers(1, 200000))
        else:
            slen = pick[int(rng.integers(0, len(pick)))]
        stride = E.round4(A.enc_size(slen)) + 4 * int(rng.integers(0, 3))
        jobs.append((off, slen, img, stride))
        off += 9 * slen + int(rng.integers(0, 16))
        img += 9 * stride + 4 * int(rng.integers(0, 5))
    return jobs


def test_schedule_of_random_queues():
    t = V.get_tactic("EC6P3")
    rng = np.random.default_rng(0xE9C0DE)
    nbuckets = set()
    for _ in range(300):
        jobs = _random_jobs(rng)
        rc, s = E.schedule(t, jobs)
        assert rc == 0
        check_schedule(jobs, s)
        nbuckets.add(len(s.buckets))
    assert max(nbuckets) <= E.MAX_BUCKETS and len(nbuckets) > 3


def test_schedule_degenerate():
    t = V.get_tactic("EC6P3")
    sz = E.round4(A.enc_size(70005))
    one = [(3, 70005, 8, sz)]
    rc, s = E.schedule(t, one)
    assert rc == 0
    check_schedule(one, s)
    assert s.buckets == [(E.KIND_FRAME, E.VAR_BELOW, 0, 1)]
    assert s.prefix == [0, 2] and s.fused == 1
    # the class edges and the variant threshold
    for slen, want in [(1024, (0, 1)), (1025, (0, 2)), (3072, (0, 3)),
                       (3073, (0, 4)), (4096, (0, 4)), (4097, (1, 87)),
                       ((1 << 20) - 1, (1, 87)), (1 << 20, (1, 76))]:
        rc, s = E.schedule(t, [(0, slen, 0, E.round4(A.enc_size(slen)))])
        assert rc == 0 and s.buckets == [want + (0, 1)], slen
        assert s.prefix == ([] if want[0] == 0 else [0, E.frames(slen)])
    # only the large bucket: its sums start the prefix array
    jobs = [(j << 24, (1 << 20) + j, j << 24, 1 << 21) for j in range(3)]
    rc, s = E.schedule(t, jobs)
    assert rc == 0 and s.prefix == [0, 17, 34, 51]
    # capacity too small
    assert E.schedule(t, jobs, item_cap=2)[0] == E.ERR_NOMEM
    assert E.schedule(t, jobs, item_cap=0)[0] == E.ERR_NOMEM
    # the gate is the tactic's, not the queue's
    for name, fused in [("EC6P6", 0), ("EC13P4", 0), ("EC6P3L3", 0),
                        ("EC12P4", 1), ("EC4P2", 1), ("LRC12P2L2", 1)]:
        rc, s = E.schedule(V.get_tactic(name), one)
        assert rc == 0 and s.fused == fused, name


def test_schedule_validation():
    t = V.get_tactic("EC6P3")
    sz = A.enc_size(100)
    assert sz == 104
    ok = [(0, 100, 0, sz)]
    assert E.schedule(t, ok)[0] == 0
    # block length: the batch call's code first, then the repair queue's
    for bl in (0, -65536, 100, 65536 + 4):
        assert E.schedule(t, ok, block_len=bl)[0] == E.ERR_BLOCK
    for bl in (4096, 131072, 65536 * 3):
        assert E.schedule(t, ok, block_len=bl)[0] == E.ERR_UNSUPPORTED
    assert E.schedule(t, [])[0] == E.ERR_INVALID                # njobs <= 0
    assert E.schedule(t, [(0, 100, 0, sz, 1)])[0] == E.ERR_INVALID
    assert E.schedule(t, [(0, 100, 0, sz, 1 << 40)])[0] == E.ERR_INVALID
    assert E.schedule(t, ok + [(0, 0, 0, sz)])[0] == E.ERR_NO_DATA
    # images: alignment of img_off and img_stride, stride below the size
    assert E.schedule(t, [(0, 100, 2, sz)])[0] == E.ERR_INVALID
    assert E.schedule(t, [(0, 100, 0, sz + 2)])[0] == E.ERR_INVALID
    assert E.schedule(t, [(0, 100, 0, sz - 4)])[0] == E.ERR_INVALID
    assert E.schedule(t, [(0, 101, 0, sz)])[0] == E.ERR_INVALID
    assert E.schedule(t, [(7, 100, 4, sz + 4)])[0] == 0
    # a second frame adds its 4-byte CRC to the image
    two = A.enc_size(65533)
    assert two == 65533 + 8
    assert E.schedule(t, [(0, 65533, 0, E.round4(two) - 4)])[0] == \
        E.ERR_INVALID
    assert E.schedule(t, [(0, 65533, 0, E.round4(two))])[0] == 0
    # a slow tactic validates the same way
    t66 = V.get_tactic("EC6P6")
    assert E.schedule(t66, [(0, 0, 0, sz)])[0] == E.ERR_NO_DATA
    assert E.schedule(t66, [(0, 100, 0, sz - 4)])[0] == E.ERR_INVALID
    assert E.schedule(t66, ok, block_len=4096)[0] == E.ERR_UNSUPPORTED


def test_encode_queue_selftest_sanitized(tmp_path):
    """The encode schedule builder under ASan + UBSan as a stand-alone
    program: a plain host compiler, gfrs_plan.cpp + gfrs_gf.cpp, no Python
    in the process."""
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host compiler with the sanitizer runtimes")
    exe = str(tmp_path / "encode_queue_selftest")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall",
                    "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    os.path.join(HERE, "encode_queue_selftest.cpp"),
                    os.path.join(CSRC, "gfrs_plan.cpp"),
                    os.path.join(CSRC, "gfrs_gf.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "encode queue selftest OK" in r.stdout


@pytest.mark.parametrize("name", E.GPU_QUEUES)
def test_gpu_queues_against_oracle(name):
    """What tests/test_gpu_encode_queue.py assumes of its inputs."""
    q = E.build(name)
    t = q.t
    exp = E.expectations(name)
    assert len(exp) == len(q.jobs) >= 12
    for j, (off, slen, img_off, stride) in enumerate(q.jobs):
        assert len(exp[j]) == q.total
        shards = []
        for i, img in enumerate(exp[j]):
            assert img.size == A.enc_size(slen)
            raw = oracle.crc32b_decode(img.copy())
            assert np.array_equal(raw, q.data[j][i]), (name, j, i)
            shards.append(raw)
        # LRC: the global stripe verifies; the local parities are covered by
        # the decode comparison with the oracle's own lrc_encode above
        assert oracle.rs_verify(t.N, t.M, shards[:t.N + t.M]), (name, j)
        assert stride % 4 == 0 and stride >= A.enc_size(slen)
    # odd base, odd gaps, jobs do not overlap
    assert q.delta % 2 == 1
    end = 0
    gaps = set()
    for off, slen, _, _ in q.jobs:
        assert off >= end
        if end:
            gaps.add(off - end)
        end = off + q.total * slen
    assert end == q.nbytes and all(g % 2 for g in gaps) and len(gaps) > 2
    # images: 4-aligned, disjoint, inside the arena
    spans = sorted(reg for j in range(len(q.jobs))
                   for reg in q.image_regions(j))
    assert all(off % 4 == 0 for off, _ in spans)
    assert all(a[0] + a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    assert spans[-1][0] + spans[-1][1] == q.img_bytes
    # image order is not job order; tight and padded strides
    firsts = [job[2] for job in q.jobs]
    assert firsts != sorted(firsts)
    slack = [job[3] - E.round4(A.enc_size(job[1])) for job in q.jobs]
    assert 0 in slack and max(slack) > 0
