"""CPU checks of the repair-image queue (gfrs_repair_queue):

 - the schedule the engine would upload (gfrs_compute_repair_queue_schedule,
   the same builder, GPU-free) for every queue of tests/_repairimgq.py: work
   items, frame prefix sums, buckets, image table, pattern classes;
 - the validation codes of the contract (include/gfrs.h);
 - the sanitized stand-alone selftest of the builder
   (repair_queue_selftest.cpp);
 - the oracle alone on every queue the GPU module runs: nothing undecodable,
   failed jobs only among the corrupted ones, a failed job in every queue and
   a clean job for every pattern, so the GPU tests never filter a case at run
   time.
"""
import os
import subprocess

import pytest

import _arena as A
import _repairimgq as R
import _verdict as V
from test_queue_cpu import _host_compiler

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "cubefs_amd", "csrc")


def check_schedule(t, jobs, patterns, s, bids=None, vuids=None):
    """Every property the kernels and the host rely on.  jobs: (off, slen,
    pattern, img_off, img_stride)."""
    npat = len(patterns)
    total = t.N + t.M + t.L
    # pattern classes: the gate of gfrs_repair_batch; plan rows and colpack
    # as gfrs_compute_plan answers for the caller's order
    for p, bad in enumerate(patterns):
        if R.fused_gate(t, bad):
            rc, nout, colpack = R.fused_plan(t, bad)
            assert rc == 0 and s.cls[p] == R.FUSED, (p, bad)
            assert (s.gm[p], s.nw[p], s.colpack[p]) == \
                (nout, len(bad), colpack), (p, bad)
            assert len(bad) <= s.gm[p] <= R.ROWS
            # nibble r of colpack: the caller's column of the r-th bad
            # shard in ascending order
            for r, idx in enumerate(sorted(bad)):
                assert (colpack >> (4 * r)) & 0xF == bad.index(idx)
        else:
            want = R.INPLACE_SLOW if t.L else R.INPLACE
            assert s.cls[p] == want and s.gm[p] == 0, (p, bad)
    assert s.inplace == [j for j, job in enumerate(jobs)
                         if s.cls[job[2]] != R.FUSED]
    # buckets: at most one per row count, ascending, back to back
    gms = [gm for gm, _, _ in s.buckets]
    assert gms == sorted(set(gms)) and all(1 <= g <= R.ROWS for g in gms)
    covered = set()
    at = 0
    for b, (gm, first, count) in enumerate(s.buckets):
        assert first == at and count > 0
        at += count
        pre = s.prefix[first + b:first + b + count + 1]
        assert pre[0] == 0
        keys = []
        for i in range(count):
            job, desc, off, slen, img, stride = s.items[first + i]
            joff, jslen, pat, img_off, img_stride = jobs[job][:5]
            assert (off, slen, stride) == (joff, jslen, img_stride)
            assert pre[i + 1] - pre[i] == R.frames(slen)
            keys.append((desc, job))
            if desc < npat:          # a fused item: the job's whole pattern
                assert desc == pat and s.cls[pat] == R.FUSED
                assert gm == s.gm[pat] and img == img_off
                hit = [(job, idx) for idx in patterns[pat]]
            else:                    # an identity item: one bad shard
                idx = desc - npat
                assert s.cls[pat] != R.FUSED and gm == 1
                assert 0 <= idx < total and idx in patterns[pat]
                assert img == img_off + patterns[pat].index(idx) * img_stride
                hit = [(job, idx)]
            for h in hit:
                assert h not in covered
                covered.add(h)
        # ordered by descriptor, then by caller index
        assert keys == sorted(keys)
    assert at == len(s.items)
    assert covered == {(j, idx) for j, job in enumerate(jobs)
                       for idx in patterns[job[2]]}
    # image table: id order = job-major, the pattern's own order
    k = 0
    for j, (off, slen, pat, img_off, img_stride) in enumerate(jobs):
        for b in range(len(patterns[pat])):
            assert s.images[k] == (img_off + b * img_stride, slen,
                                   bids[k] if bids else 0,
                                   vuids[k] if vuids else 0), (j, b)
            k += 1
    assert k == len(s.images)


@pytest.mark.parametrize("name", R.GPU_QUEUES)
def test_schedule_of_gpu_queues(name):
    r = R.build(name)
    rc, s = R.schedule(r.t, r.rjobs, r.patterns, r.bids, r.vuids)
    assert rc == 0
    check_schedule(r.t, r.rjobs, r.patterns, s, r.bids, r.vuids)
    if name == "rs63_mixed":
        # m = 3: every plan has 3 rows, one bucket
        assert [gm for gm, _, _ in s.buckets] == [3]
        assert s.cls == [R.FUSED] * 6 and not s.inplace
        # [1,8] and [8,1]: the same erasures, another column order
        assert s.colpack[4] == 0x10 and s.colpack[5] == 0x01
        order = [it[0] for it in s.items]
        assert order != sorted(order)    # by descriptor: jobs are permuted
    if name == "rs124_k12":
        assert [gm for gm, _, _ in s.buckets] == [4]
    if name == "lrc_single":
        assert s.cls == [R.FUSED] * 5
    if name in ("rs66_inplace", "rs134_w17", "lrc_slow"):
        # identity items only: one bucket of one row, one item per image
        assert [gm for gm, _, _ in s.buckets] == [1]
        assert len(s.items) == r.nimg
        assert s.inplace == list(range(len(r.rjobs)))
        assert all(c == (R.INPLACE_SLOW if name == "lrc_slow"
                         else R.INPLACE) for c in s.cls)


@pytest.mark.parametrize("tname,pats", [
    ("EC4P1", [[0], [4], [3]]),
    ("EC4P2", [[0], [5, 4], [3, 0], [1]]),
    ("LRC12P2L2", [[15, 14], [13, 12, 14], [0], [12, 13, 14, 15]])])
def test_schedule_row_counts(tname, pats):
    """Every parity is rebuilt, an input or checked, so a fused plan has
    m + l rows whatever is lost: buckets of 1, 2 and 4 rows."""
    t = A.tactic(4, 1) if tname == "EC4P1" else V.get_tactic(tname)
    sz = R.round4(A.disk_size(100))
    jobs = [(j * 2000, 100, j % len(pats), j * 4 * sz, sz) for j in range(8)]
    rc, s = R.schedule(t, jobs, pats)
    assert rc == 0
    check_schedule(t, jobs, pats, s)
    assert [gm for gm, _, _ in s.buckets] == [t.M + t.L]


def test_schedule_degenerate():
    t = V.get_tactic("EC6P3")
    sz = R.round4(A.disk_size(70005))
    one = [(3, 70005, 0, 8, sz)]
    rc, s = R.schedule(t, one, [[5, 0]])
    assert rc == 0
    check_schedule(t, one, [[5, 0]], s)
    assert s.prefix == [0, 2] and s.colpack == [0x01]
    # all jobs one pattern, a second pattern unused
    jobs = [(j * 10 ** 6, 1 + 9000 * j, 1, j * 4 * 10 ** 5, 10 ** 5)
            for j in range(9)]
    rc, s = R.schedule(t, jobs, [[8], [2]])
    assert rc == 0
    check_schedule(t, jobs, [[8], [2]], s)
    assert [it[0] for it in s.items] == list(range(9))
    # capacity too small: items, then images
    assert R.schedule(t, jobs, [[8], [2]], item_cap=8)[0] == R.ERR_NOMEM
    assert R.schedule(t, jobs, [[8], [2]], image_cap=8)[0] == R.ERR_NOMEM


def test_schedule_validation():
    t = V.get_tactic("EC6P3")
    sz = A.disk_size(100)
    assert sz % 4 == 0
    ok = [(0, 100, 0, 0, sz)]
    assert R.schedule(t, ok, [[1]])[0] == 0
    assert R.schedule(t, [], [[1]])[0] == R.ERR_INVALID          # njobs <= 0
    assert R.schedule(t, ok, [])[0] == R.ERR_INVALID             # npat <= 0
    assert R.schedule(t, ok, [[1]], boff=[1, 1])[0] == R.ERR_INVALID
    assert R.schedule(t, ok, [[1], [2]], boff=[0, 2, 1])[0] == R.ERR_INVALID
    assert R.schedule(t, [(0, 100, 1, 0, sz)], [[1]])[0] == R.ERR_INVALID
    assert R.schedule(t, [(0, 100, -1, 0, sz)], [[1]])[0] == R.ERR_INVALID
    assert R.schedule(t, [(0, 100, 0, 0, sz, 1)], [[1]])[0] == R.ERR_INVALID
    assert R.schedule(t, [(0, 0, 0, 0, sz)], [[1]])[0] == R.ERR_NO_DATA
    # images: alignment of img_off and img_stride, stride below the size
    assert R.schedule(t, [(0, 100, 0, 2, sz)], [[1]])[0] == R.ERR_INVALID
    assert R.schedule(t, [(0, 100, 0, 0, sz + 2)], [[1]])[0] == R.ERR_INVALID
    assert R.schedule(t, [(0, 100, 0, 0, sz - 4)], [[1]])[0] == R.ERR_INVALID
    assert R.schedule(t, [(0, 101, 0, 0, sz)], [[1]])[0] == R.ERR_INVALID
    assert R.schedule(t, [(0, 100, 0, 4, sz + 4)], [[1]])[0] == 0
    # a second frame adds its 4-byte CRC to the image
    two = A.disk_size(65533)
    assert two == 32 + 65533 + 8 + 8
    assert R.schedule(t, [(0, 65533, 0, 0, R.round4(two) - 4)],
                      [[1]])[0] == R.ERR_INVALID
    assert R.schedule(t, [(0, 65533, 0, 0, R.round4(two))], [[1]])[0] == 0
    # block length
    for bl in (4096, 131072, 0):
        assert R.schedule(t, ok, [[1]], block_len=bl)[0] == R.ERR_UNSUPPORTED
    # every pattern is validated, used or not, with the reconstruct queue's
    # codes; empty and repeating patterns are refused for every tactic
    assert R.schedule(t, ok, [[1], [9]])[0] == R.ERR_INVALID
    assert R.schedule(t, ok, [[1], [-1]])[0] == R.ERR_INVALID
    assert R.schedule(t, ok, [[1], [0, 1, 2, 3]])[0] == R.ERR_TOO_FEW
    assert R.schedule(t, ok, [[1], []])[0] == R.ERR_INVALID
    assert R.schedule(t, ok, [[1, 1]])[0] == R.ERR_INVALID
    t66 = V.get_tactic("EC6P6")
    assert R.schedule(t66, ok, [[1], [2, 3, 2]])[0] == R.ERR_INVALID
    assert R.schedule(t66, ok, [[1], []])[0] == R.ERR_INVALID
    assert R.schedule(t66, ok, [[0, 1, 2, 3, 4, 5, 6]])[0] == R.ERR_TOO_FEW
    lrc = V.get_tactic("LRC12P2L2")
    assert R.schedule(lrc, ok, [[0], [0, 1, 2]])[0] == R.ERR_TOO_FEW
    assert R.schedule(lrc, ok, [[0, 0]])[0] == R.ERR_INVALID
    assert R.schedule(lrc, ok, [[0, 14, 15]])[0] == 0


def test_repair_queue_selftest_sanitized(tmp_path):
    """The repair schedule builder under ASan + UBSan as a stand-alone
    program: a plain host compiler, gfrs_plan.cpp + gfrs_gf.cpp, no Python
    in the process."""
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host compiler with the sanitizer runtimes")
    exe = str(tmp_path / "repair_queue_selftest")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall",
                    "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    os.path.join(HERE, "repair_queue_selftest.cpp"),
                    os.path.join(CSRC, "gfrs_plan.cpp"),
                    os.path.join(CSRC, "gfrs_gf.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "repair queue selftest OK" in r.stdout


@pytest.mark.parametrize("name", R.GPU_QUEUES)
def test_gpu_queues_against_oracle(name):
    """What tests/test_gpu_repair_queue.py assumes of its inputs."""
    r = R.build(name)
    q = r.q
    assert 2 <= len(r.rjobs) <= 64
    exp = R.expectations(name)
    assert all(e != V.UNDECODABLE for e in exp)
    fails = {j for j, e in enumerate(exp) if e[1]}
    corrupted = {j for j, f in enumerate(q.flips) if f}
    assert corrupted == set(range(0, len(r.rjobs), 3))
    assert fails and fails <= corrupted, (name, fails)
    assert all(f[1] in V.rs_positions(q.jobs[j][1])
               for j, f in enumerate(q.flips) if f)
    # every pattern has a clean job whose images are compared in full
    for p in range(len(r.patterns)):
        assert any(job[2] == p and j not in corrupted
                   for j, job in enumerate(r.rjobs)), (name, p)
    imgs = R.images(name)
    assert all((imgs[j] is None) == (j in fails) for j in range(len(imgs)))
    # no empty pattern; odd base, jobs do not overlap
    assert all(r.patterns) and q.delta % 2 == 1
    end = 0
    for off, slen, pat in q.jobs:
        assert off >= end
        end = off + q.total * slen
    assert end == q.nbytes
    # images: 4-aligned, disjoint, inside the arena, ids job-major
    spans = sorted(reg for j in range(len(r.rjobs))
                   for reg in r.image_regions(j))
    assert all(off % 4 == 0 for off, _ in spans)
    assert all(a[0] + a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    assert spans[-1][0] + spans[-1][1] == r.img_bytes
    assert r.ids == [sum(len(r.bad_of(i)) for i in range(j))
                     for j in range(len(r.rjobs))]
    for off, slen, pat, img_off, stride in r.rjobs:
        assert stride % 4 == 0 and stride >= A.disk_size(slen)
    if name == "rs63_uniform":
        return
    # image order is not job order; uneven padding; tight and padded strides
    firsts = [job[3] for job in r.rjobs]
    assert firsts != sorted(firsts)
    gaps = {b[0] - (a[0] + a[1]) for a, b in zip(spans, spans[1:])}
    assert len(gaps) > 2
    slack = [job[4] - R.round4(A.disk_size(job[1])) for job in r.rjobs]
    assert 0 in slack and max(slack) > 0
    if name == "rs63_mixed":
        assert {job[1] for job in r.rjobs} == set(R.LENS)
    if r.t.L:
        assert all(f[0] >= r.t.N + r.t.M for f in q.flips if f)
        # a lost local parity is among the patterns
        assert any(i >= r.t.N + r.t.M for p in r.patterns for i in p)
