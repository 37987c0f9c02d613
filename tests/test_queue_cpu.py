"""CPU checks of the repair queue (gfrs_reconstruct_verify_queue):

 - the launch schedule the engine would build (gfrs_compute_queue_schedule,
   the same builder, GPU-free) for every queue of tests/_repairq.py;
 - the validation codes;
 - the sanitized stand-alone selftest of the builder (queue_selftest.cpp);
 - the oracle alone on every queue the GPU module runs: each must hold a
   failing and a clean job and no undecodable one, so the GPU tests never
   filter a case at run time.
"""
import os
import shutil
import subprocess

import pytest

import _repairq as Q
import _verdict as V

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "cubefs_amd", "csrc")


def _host_compiler():
    """A host C++ compiler that links the address + UB sanitizer runtimes
    (the probe of tests/test_plan_cpu.py)."""
    probe = "int main() { return 0; }\n"
    for cxx in ("g++", "clang++", "c++"):
        path = shutil.which(cxx)
        if not path:
            continue
        r = subprocess.run([path, "-fsanitize=address,undefined", "-x",
                            "c++", "-", "-o", os.devnull], input=probe,
                           capture_output=True, text=True)
        if r.returncode == 0:
            return path
    return None


def tiles(slen):
    return (slen + Q.TILE - 1) // Q.TILE


def check_schedule(t, jobs, patterns, s):
    """Every property the kernel and the host rely on."""
    # patterns: rows and slow marks as the plan builder answers
    for p, bad in enumerate(patterns):
        rc, nout = Q.plan_rows(t, bad)
        if Q.single_pass_budget(t) and rc == 0:
            assert not s.slow[p] and s.nout[p] == nout, (p, bad)
        else:
            assert rc in (0, Q.ERR_UNSUPPORTED), (p, bad, rc)
            assert s.slow[p] and s.nout[p] == 0, (p, bad)
    assert s.slow_jobs == [j for j, job in enumerate(jobs)
                           if s.slow[job[2]]]
    # buckets: ascending (g, gm), distinct, bounded in number
    keys = [(g, gm) for g, gm, _, _ in s.buckets]
    assert keys == sorted(set(keys))
    max_nout = max(s.nout)
    assert len(s.buckets) <= Q.ROWS * ((max_nout + Q.ROWS - 1) // Q.ROWS)
    covered = {}
    at = 0
    for b, (g, gm, first, count) in enumerate(s.buckets):
        assert first == at and count > 0
        at += count
        assert 1 <= gm <= Q.ROWS
        pats_seen = []
        pre = s.prefix[first + b:first + b + count + 1]
        assert pre[0] == 0
        for i in range(count):
            job, pat, row_off, off, slen, reserved = s.items[first + i]
            assert (off, slen, pat) == tuple(jobs[job][:3])
            assert reserved == 0 and row_off == Q.ROWS * g
            assert gm == min(Q.ROWS, s.nout[pat] - row_off), (job, g, gm)
            assert pre[i + 1] - pre[i] == tiles(slen)
            for r in range(row_off, row_off + gm):
                assert (job, r) not in covered
                covered[(job, r)] = b
            if not pats_seen or pats_seen[-1] != pat:
                pats_seen.append(pat)
        # grouped by pattern: no pattern comes back after another one
        assert len(pats_seen) == len(set(pats_seen))
    assert at == len(s.items)
    want = {(j, r) for j, job in enumerate(jobs) if not s.slow[job[2]]
            for r in range(s.nout[job[2]])}
    assert set(covered) == want


@pytest.mark.parametrize("name", Q.GPU_QUEUES)
def test_schedule_of_gpu_queues(name):
    q = Q.build(name)
    rc, s = Q.schedule(q.t, q.jobs, q.patterns)
    assert rc == 0
    check_schedule(q.t, q.jobs, q.patterns, s)
    if name == "rs63_mixed":
        # rows 3,4,5,6,3,4: buckets (0,3) (0,4) (1,1) (1,2)
        assert [(g, gm) for g, gm, _, _ in s.buckets] == \
            [(0, 3), (0, 4), (1, 1), (1, 2)]
        # ordering by pattern permutes the jobs
        order = [it[0] for it in s.items[:s.buckets[0][3]]]
        assert order != sorted(order)
    if name == "rs66_depth":
        assert max(s.nout) == 12 and max(g for g, _, _, _ in s.buckets) == 2
    if name == "lrc_slow":
        assert all(s.slow) and not s.items and not s.buckets
        assert s.slow_jobs == list(range(len(q.jobs)))
    if name == "lrc_single":
        assert not any(s.slow)


def test_schedule_degenerate():
    t = V.get_tactic("EC6P3")
    one = [(3, 5000, 0)]
    rc, s = Q.schedule(t, one, [[0, 5]])
    assert rc == 0
    check_schedule(t, one, [[0, 5]], s)
    assert s.prefix == [0, 2, 0, 2]
    # all jobs one pattern, a second pattern unused
    jobs = [(j * 100000, 1 + 900 * j, 1) for j in range(9)]
    rc, s = Q.schedule(t, jobs, [[8], [2]])
    assert rc == 0
    check_schedule(t, jobs, [[8], [2]], s)
    assert [it[0] for it in s.items] == list(range(9))
    # every job its own pattern
    pats = [[i] for i in range(9)]
    jobs = [(j * 100000, 4096 * (j + 1), 8 - j) for j in range(9)]
    rc, s = Q.schedule(t, jobs, pats)
    assert rc == 0
    check_schedule(t, jobs, pats, s)
    # capacity too small: items, then buckets
    assert Q.schedule(t, jobs, pats, item_cap=len(s.items) - 1)[0] == \
        Q.ERR_NOMEM
    assert Q.schedule(t, jobs, pats, bucket_cap=len(s.buckets) - 1)[0] == \
        Q.ERR_NOMEM
    assert Q.schedule(t, jobs, pats, item_cap=len(s.items),
                      bucket_cap=len(s.buckets))[0] == 0


def test_schedule_validation():
    t = V.get_tactic("EC6P3")
    ok = [(0, 100, 0)]
    assert Q.schedule(t, ok, [[1]])[0] == 0
    assert Q.schedule(t, [], [[1]])[0] == Q.ERR_INVALID          # njobs <= 0
    assert Q.schedule(t, ok, [])[0] == Q.ERR_INVALID             # npat <= 0
    assert Q.schedule(t, [(0, 100, 1)], [[1]])[0] == Q.ERR_INVALID
    assert Q.schedule(t, [(0, 100, -1)], [[1]])[0] == Q.ERR_INVALID
    assert Q.schedule(t, [(0, 0, 0)], [[1]])[0] == Q.ERR_NO_DATA
    assert Q.schedule(t, [(0, 100, 0, 1)], [[1]])[0] == Q.ERR_INVALID
    # every pattern is validated, used or not
    assert Q.schedule(t, ok, [[1], [9]])[0] == Q.ERR_INVALID
    assert Q.schedule(t, ok, [[1], [-1]])[0] == Q.ERR_INVALID
    assert Q.schedule(t, ok, [[1], [0, 1, 2, 3]])[0] == Q.ERR_TOO_FEW
    assert Q.schedule(t, ok, [[1, 1]])[0] == 0     # RS tolerates a repeat
    # LRC: more than m global losses are undecodable for the full-width
    # Reconstruct, whatever the local parities could restore
    lrc = V.get_tactic("LRC12P2L2")
    assert Q.schedule(lrc, ok, [[0], [0, 1, 2]])[0] == Q.ERR_TOO_FEW
    assert Q.plan_rows(lrc, [0, 1, 2])[0] == Q.ERR_UNSUPPORTED
    assert V.expected(lrc, V.A.ref_stripes(lrc, 1, 33, seed=21)[0],
                      [0, 1, 2]) == V.UNDECODABLE
    assert Q.schedule(lrc, ok, [[0, 0]])[0] == Q.ERR_INVALID
    assert Q.schedule(lrc, ok, [[0, 14, 15]])[0] == 0


def test_queue_selftest_sanitized(tmp_path):
    """The schedule builder under ASan + UBSan as a stand-alone program: a
    plain host compiler, gfrs_plan.cpp + gfrs_gf.cpp, no Python in the
    process."""
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host compiler with the sanitizer runtimes")
    exe = str(tmp_path / "queue_selftest")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall",
                    "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    os.path.join(HERE, "queue_selftest.cpp"),
                    os.path.join(CSRC, "gfrs_plan.cpp"),
                    os.path.join(CSRC, "gfrs_gf.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "queue selftest OK" in r.stdout


@pytest.mark.parametrize("name", Q.GPU_QUEUES)
def test_gpu_queues_against_oracle(name):
    """What tests/test_gpu_queue.py assumes of its inputs."""
    q = Q.build(name)
    assert 2 <= len(q.jobs) <= 64
    assert max(slen for _, slen, _ in q.jobs) <= 8209
    exp = Q.expectations(name)
    assert all(e != V.UNDECODABLE for e in exp)
    fails = [j for j, e in enumerate(exp) if e[1]]
    assert fails and len(fails) < len(q.jobs), (name, fails)
    for j in fails:
        assert q.flips[j] is not None
    # odd base, odd gaps: jobs do not overlap and sit at mixed alignments
    assert q.delta % 2 == 1
    end = 0
    for off, slen, pat in q.jobs:
        assert off >= end
        end = off + q.total * slen
    assert end == q.nbytes
    if name != "rs63_uniform":
        assert len({off % 16 for off, _, _ in q.jobs}) > 4
        assert len({pat for _, _, pat in q.jobs}) == len(q.patterns)
    if name == "rs63_mixed":
        assert {slen for _, slen, _ in q.jobs} == set(Q.LENS)
        # a flip every third job, at the kernels' edge positions
        assert [j for j, f in enumerate(q.flips) if f] == \
            list(range(0, len(q.jobs), 3))
        assert all(f[1] in V.rs_positions(q.jobs[j][1])
                   for j, f in enumerate(q.flips) if f)
    if q.t.L:
        # the flips sit in surviving local parities
        assert all(f[0] >= q.t.N + q.t.M for f in q.flips if f)
