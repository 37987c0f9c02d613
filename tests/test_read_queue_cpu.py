"""CPU checks of the read queue (gfrs_read_queue):

 - the schedule the engine would upload (gfrs_compute_read_queue_schedule,
   the same builder, GPU-free) against a Python restatement, for every queue
   of tests/_readq.py and for a few hundred seeded random ones: pattern
   classes, buckets, item order, touched-frame prefix sums, slow jobs;
 - the validation codes of the contract (include/gfrs.h) and the capacity
   refusals of the export;
 - the read plan (gfrs_compute_plan kind 4): inputs, rows and pass-through
   set for every pattern of 6+3, 4+2 and 3+3 and the sampled ones of 12+4,
   6+6 and LRC12P2L2, applied with the oracle's multiplication table;
 - the sanitized stand-alone selftest of the builder
   (read_queue_selftest.cpp);
 - the oracle alone on every queue the GPU module runs, so the GPU tests
   compare against something self-consistent.
"""
import os
import subprocess

import numpy as np
import pytest

import _arena as A
import _readq as G
import _verdict as V
from _arena import oracle
from test_plan_cpu import check_rows, compute_plan, mul, patterns  # noqa: F401
from test_queue_cpu import _host_compiler

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "cubefs_amd", "csrc")
READ = 4


# ---- the schedule, restated ---------------------------------------------------

def want_schedule(t, jobs, pats):
    """(buckets, items, prefix, slow_jobs, classes) as gfrs.h states them."""
    cls = [G.classify(t, p) for p in pats]
    per = {}
    slow = []
    for j, job in enumerate(jobs):
        c, r = cls[job[7]]
        if c == G.FUSED:
            per.setdefault(r, []).append((job[7], j))
        elif c == G.IDENTITY:
            per.setdefault(0, []).extend((len(pats) + s, j)
                                         for s in range(t.N))
        else:
            slow.append(j)
    buckets, items, prefix = [], [], []
    for r in sorted(per):
        ordered = sorted(per[r])          # by descriptor, then caller index
        buckets.append((r, len(items), len(ordered)))
        sums = [0]
        for desc, j in ordered:
            img_off, stride, slen, so, sl, out_off, ostride, _ = jobs[j][:8]
            items.append((j, desc, img_off, stride, slen, so, sl, out_off,
                          ostride))
            sums.append(sums[-1] + len(G.touched(so, sl)))
        prefix += sums
    return buckets, items, prefix, slow, cls


def check_schedule(t, jobs, pats, s):
    buckets, items, prefix, slow, cls = want_schedule(t, jobs, pats)
    assert s.pat_class == [c for c, _ in cls]
    assert s.pat_r == [r for _, r in cls]
    assert s.buckets == buckets
    assert s.items == items
    assert s.prefix == prefix
    assert s.slow_jobs == slow
    assert len(s.buckets) <= G.MAX_BUCKETS
    assert [b[0] for b in s.buckets] == sorted({b[0] for b in s.buckets})


@pytest.mark.parametrize("name", G.GPU_QUEUES)
def test_schedule_of_gpu_queues(name):
    q = G.build(name)
    rc, s = G.schedule(q.t, q.jobs, q.patterns)
    assert rc == 0
    check_schedule(q.t, q.jobs, q.patterns, s)
    rs = [b[0] for b in s.buckets]
    if name in ("rs63",):
        assert rs == [0, 1, 2, 3]
    if name in ("rs44", "rs124", "rs66"):
        assert rs == [0, 1, 2, 3, 4]
    if name in ("rs66_slow", "corrupt_rs66_slow"):
        assert s.slow_jobs and rs == [1]
        assert {q.jobs[j][7] for j in s.slow_jobs} == \
            {p for p, c in enumerate(s.pat_class) if c == G.SLOW}
    if name in ("rs134_w17", "corrupt_w17"):
        assert rs == [0] and s.slow_jobs
        assert G.IDENTITY in s.pat_class and G.SLOW in s.pat_class
        # identity items: one per data shard
        nid = sum(1 for j in q.jobs if s.pat_class[j[7]] == G.IDENTITY)
        assert len(s.items) == nid * q.t.N
    if name in G.CLEAN_QUEUES:
        assert not s.slow_jobs
        # descriptors change inside every bucket that holds two patterns
        for r, first, count in s.buckets:
            descs = [s.items[first + i][1] for i in range(count)]
            assert descs == sorted(descs)
    # a touched-frame sum, not a shard-frame sum: some item of a two- or
    # three-frame shard counts one frame only
    if any(j[2] > G.PAYLOAD for j in q.jobs):
        assert any(len(G.touched(j[3], j[4])) <
                   (j[2] + G.PAYLOAD - 1) // G.PAYLOAD for j in q.jobs)


def _random_queue(rng, t):
    total = t.N + t.M + t.L
    npat = int(rng.integers(1, 7))
    pats = []
    for _ in range(npat):
        nb = int(rng.integers(0, t.M + 1))
        bad = [int(x) for x in rng.permutation(t.N + t.M)[:nb]]
        if t.L and rng.integers(0, 2):
            bad.append(int(rng.integers(t.N + t.M, total)))
        pats.append(bad)
    pick = [1, 3, 4, 5, 17, 4096, 65531, 65532, 65533, 65597, 131064, 131065,
            200000, 1 << 20]
    jobs, img, out = [], int(rng.integers(0, 64)), 4 * int(rng.integers(0, 9))
    for _ in range(int(rng.integers(1, 40))):
        slen = pick[int(rng.integers(0, len(pick)))] \
            if rng.integers(0, 3) else int(rng.integers(1, 300000))
        so = 4 * int(rng.integers(0, (slen + 3) // 4))
        sl = int(rng.integers(1, slen - so + 1))
        stride = A.enc_size(slen) + int(rng.integers(0, 5))
        ostride = G.round4(sl) + 4 * int(rng.integers(0, 3))
        jobs.append((img, stride, slen, so, sl, out, ostride,
                     int(rng.integers(0, npat))))
        img += total * stride + int(rng.integers(0, 7))
        out += t.N * ostride + 4 * int(rng.integers(0, 5))
    return jobs, pats


@pytest.mark.parametrize("tname", ["EC6P3", "EC6P6", "EC13P4", "LRC12P2L2"])
def test_schedule_of_random_queues(tname):
    t = V.get_tactic(tname)
    rng = np.random.default_rng(0x9E7D + len(tname) + t.N)
    nb = set()
    for _ in range(120):
        jobs, pats = _random_queue(rng, t)
        rc, s = G.schedule(t, jobs, pats)
        assert rc == 0, (jobs, pats)
        check_schedule(t, jobs, pats, s)
        nb.add(len(s.buckets))
    assert max(nb) <= G.MAX_BUCKETS and len(nb) > 1


def test_schedule_degenerate():
    t = V.get_tactic("EC6P3")
    sz = A.enc_size(200000)
    # one job, one pattern; a segment inside the third of four frames
    one = [(3, sz + 1, 200000, 140000, 8, 8, 8, 0)]
    rc, s = G.schedule(t, one, [[2]])
    assert rc == 0
    check_schedule(t, one, [[2]], s)
    assert s.buckets == [(1, 0, 1)] and s.prefix == [0, 1]
    # the segment edges of the touched-frame rule
    for so, sl, nf in [(0, 65532, 1), (0, 65533, 2), (65528, 4, 1),
                       (65528, 5, 2), (65532, 1, 1), (4, 200000 - 4, 4),
                       (131064, 1, 1), (131060, 8, 2), (196596, 3404, 1)]:
        job = [(0, sz, 200000, so, sl, 0, G.round4(sl), 0)]
        rc, s = G.schedule(t, job, [[]])
        assert rc == 0 and s.buckets == [(0, 0, 1)], (so, sl)
        assert s.prefix == [0, nf], (so, sl, s.prefix)
    # an unused slow pattern costs nothing; a used one lists its job
    t66 = V.get_tactic("EC6P6")
    job = [(0, sz, 200000, 0, 4, 0, 4, 0)]
    rc, s = G.schedule(t66, job, [[1], [0, 1, 2, 3, 4]])
    assert rc == 0 and s.pat_class == [G.FUSED, G.SLOW] and not s.slow_jobs
    rc, s = G.schedule(t66, [job[0][:7] + (1,)], [[1], [0, 1, 2, 3, 4]])
    assert rc == 0 and s.slow_jobs == [0] and not s.items and not s.buckets
    # the class is the pattern's number of missing DATA shards
    for tname, bad, want in [
            ("EC6P6", [6, 7, 8, 9, 10, 11], (G.FUSED, 0)),
            ("EC6P6", [0, 1, 2, 3, 11], (G.FUSED, 4)),
            ("EC6P6", [0, 1, 2, 3, 4], (G.SLOW, 5)),
            ("EC13P4", [13, 16], (G.IDENTITY, 0)),
            ("EC13P4", [0], (G.SLOW, 1)),
            ("EC12P4", [0, 1, 2, 3], (G.FUSED, 4)),
            ("LRC12P2L2", [14, 15], (G.FUSED, 0)),
            ("LRC12P2L2", [14, 0, 12], (G.FUSED, 1)),
            ("EC6P3L3", [9], (G.FUSED, 0)),
            ("EC4P4L2", [0, 1, 2, 3, 8], (G.FUSED, 4))]:
        tt = V.get_tactic(tname)
        rc, s = G.schedule(tt, [(0, sz, 200000, 0, 4, 0, 4, 0)], [bad])
        assert rc == 0 and (s.pat_class[0], s.pat_r[0]) == want, (tname, bad)
        assert G.classify(tt, bad) == want
    # capacity too small
    jobs = [(j << 20, 1 << 19, 1 << 18, 0, 4, 64 * j, 4, 0) for j in range(3)]
    assert G.schedule(t, jobs, [[]], item_cap=2)[0] == G.ERR_NOMEM
    assert G.schedule(t, jobs, [[]], item_cap=0)[0] == G.ERR_NOMEM
    assert G.schedule(t, jobs, [[]], item_cap=3)[0] == 0
    t17 = V.get_tactic("EC13P4")      # identity: n items per job
    assert G.schedule(t17, jobs, [[]], item_cap=3 * 13 - 1)[0] == G.ERR_NOMEM
    assert G.schedule(t17, jobs, [[]], item_cap=3 * 13)[0] == 0


def test_schedule_validation():
    t = V.get_tactic("EC6P3")
    sz = A.enc_size(100)
    assert sz == 104
    ok = (0, sz, 100, 0, 100, 0, 100, 0)
    pats = [[], [1]]

    def rc(job=ok, pats=pats, **kw):
        return G.schedule(t, [job] if isinstance(job, tuple) else job, pats,
                          **kw)[0]

    def swap(**f):
        names = ["img_off", "img_stride", "slen", "seg_off", "seg_len",
                 "out_off", "out_stride", "pattern", "reserved"]
        v = dict(zip(names, ok + (0,)))
        v.update(f)
        return tuple(v[n] for n in names)

    assert rc() == 0
    # block length
    for bl in (0, -65536, 100, 65536 + 4):
        assert rc(block_len=bl) == G.ERR_BLOCK
    for bl in (4096, 131072, 65536 * 3):
        assert rc(block_len=bl) == G.ERR_UNSUPPORTED
    # patterns, used or not
    assert rc(pats=[[], [9]]) == G.ERR_INVALID
    assert rc(pats=[[], [-1]]) == G.ERR_INVALID
    assert rc(pats=[[], [1, 1]]) == G.ERR_INVALID
    assert rc(pats=[[], [8, 2, 8]]) == G.ERR_INVALID
    assert rc(pats=[[], [0, 1, 2, 3]]) == G.ERR_TOO_FEW
    assert rc(pats=[[], [5, 6, 7, 8]]) == G.ERR_TOO_FEW
    assert rc(pats=[[], [6, 7, 8]]) == 0
    lrc = A.lrc_tactic()
    one = [(0, sz, 100, 0, 100, 0, 100, 0)]
    assert G.schedule(lrc, one, [[0, 1, 14, 15]])[0] == 0   # locals ignored
    assert G.schedule(lrc, one, [[0, 1, 12]])[0] == G.ERR_TOO_FEW
    assert G.schedule(lrc, one, [[15, 15]])[0] == G.ERR_INVALID
    assert G.schedule(lrc, one, [[16]])[0] == G.ERR_INVALID
    # njobs, npat, bad_off, pattern index, reserved
    assert rc(job=[]) == G.ERR_INVALID
    assert rc(njobs=-1) == G.ERR_INVALID
    assert rc(npat=0) == G.ERR_INVALID
    assert rc(npat=-2) == G.ERR_INVALID
    assert rc(bad_off=[1, 1, 2]) == G.ERR_INVALID
    assert rc(bad_off=[0, 1, 0]) == G.ERR_INVALID
    assert rc(swap(pattern=2)) == G.ERR_INVALID
    assert rc(swap(pattern=-1)) == G.ERR_INVALID
    assert rc(swap(reserved=1)) == G.ERR_INVALID
    # alignment
    assert rc(swap(seg_off=2, seg_len=4)) == G.ERR_INVALID
    assert rc(swap(out_off=2)) == G.ERR_INVALID
    assert rc(swap(out_stride=102)) == G.ERR_INVALID
    # sizes
    assert rc(swap(out_stride=96)) == G.ERR_INVALID
    assert rc(swap(seg_len=97, out_stride=96)) == G.ERR_INVALID
    assert rc(swap(seg_len=96, out_stride=96)) == 0
    assert rc(swap(img_stride=sz - 1)) == G.ERR_INVALID
    assert rc(swap(img_stride=sz + 1)) == 0          # any value >= the size
    assert rc(swap(seg_off=4, seg_len=97)) == G.ERR_INVALID
    assert rc(swap(seg_off=4, seg_len=96)) == 0
    assert rc(swap(seg_off=104, seg_len=1)) == G.ERR_INVALID
    assert rc(swap(seg_off=1 << 63, seg_len=1 << 63)) == G.ERR_INVALID
    assert rc(swap(slen=65533, img_stride=65533 + 4, seg_len=4)) == \
        G.ERR_INVALID                                # two frames, two CRCs
    assert rc(swap(slen=65533, img_stride=65533 + 8, seg_len=4)) == 0
    assert rc(swap(slen=0)) == G.ERR_NO_DATA
    assert rc(swap(seg_len=0)) == G.ERR_NO_DATA
    assert rc([ok, swap(seg_len=0)]) == G.ERR_NO_DATA
    # slow and identity patterns validate the same way
    t66 = V.get_tactic("EC6P6")
    assert G.schedule(t66, [swap(seg_len=0)], [[0, 1, 2, 3, 4]])[0] == \
        G.ERR_NO_DATA
    assert G.schedule(t66, [swap(out_off=2)], [[0, 1, 2, 3, 4]])[0] == \
        G.ERR_INVALID
    t17 = V.get_tactic("EC13P4")
    assert G.schedule(t17, [swap(seg_off=2, seg_len=2)], [[]])[0] == \
        G.ERR_INVALID
    assert G.schedule(t17, [ok], [[]], block_len=4096)[0] == \
        G.ERR_UNSUPPORTED


# ---- the read plan --------------------------------------------------------------

def want_read(t, bad):
    total = t.N + t.M + t.L
    if len(set(bad)) != len(bad) or any(b < 0 or b >= total for b in bad):
        return G.ERR_INVALID, None
    glob = [b for b in bad if b < t.N + t.M]
    if len(glob) > t.M:
        return G.ERR_TOO_FEW, None
    valid = G.inputs(t, glob)
    out = sorted(b for b in bad if b < t.N)
    pass_mask = sum(1 << c for c, i in enumerate(valid) if i < t.N)
    return 0, dict(inp=valid, out=out, cmp_mask=0, colpack=pass_mask)


@pytest.mark.parametrize("name", ["EC6P3", "EC4P2", "EC3P3", "EC12P4",
                                  "EC6P6", "LRC12P2L2"])
def test_read_plans(mul, name):  # noqa: F811
    t = V.get_tactic(name)
    nplans = nrefused = nrows = 0
    for bad in patterns(name) + [[]]:
        what = "%s read bad=%s" % (name, bad)
        rc, plan = compute_plan(t, READ, bad)
        wrc, w = want_read(t, bad)
        assert rc == wrc, (what, rc, wrc)
        if rc != 0:
            nrefused += 1
            continue
        assert plan["rowk"] == t.N, what
        for f in ("inp", "out", "cmp_mask", "colpack"):
            assert plan[f] == w[f], (what, f, plan[f], w[f])
        # the rows rebuild the missing data from the inputs
        check_rows(mul, t, plan, what)
        nplans += 1
        nrows += len(plan["out"])
    assert nplans > 40 and nrefused >= 1 and nrows > 40, (nplans, nrefused)


def test_read_plan_error_codes():
    rs = V.get_tactic("EC6P3")
    for bad, want in [([0, 1, 2, 3], G.ERR_TOO_FEW), ([9], G.ERR_INVALID),
                      ([-1], G.ERR_INVALID), ([0, 0], G.ERR_INVALID)]:
        assert compute_plan(rs, READ, bad)[0] == want, bad


# ---- the builder under the sanitizers, as a host program -----------------------

def test_read_queue_selftest_sanitized(tmp_path):
    """The read plan, the pattern classes and the schedule builder under ASan
    + UBSan as a stand-alone program: a plain host compiler, gfrs_plan.cpp +
    gfrs_gf.cpp, no Python in the process."""
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host compiler with the sanitizer runtimes")
    exe = str(tmp_path / "read_queue_selftest")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall",
                    "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    os.path.join(HERE, "read_queue_selftest.cpp"),
                    os.path.join(CSRC, "gfrs_plan.cpp"),
                    os.path.join(CSRC, "gfrs_gf.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "read queue selftest OK" in r.stdout


# ---- the oracle alone on the GPU queues -----------------------------------------

@pytest.mark.parametrize("name", G.GPU_QUEUES)
def test_gpu_queues_against_oracle(name):
    """What tests/test_gpu_read_queue.py assumes of its inputs."""
    q = G.build(name)
    t = q.t
    imgs, words = G.images(name), G.words(name)
    assert len(q.jobs) >= 6
    flipped = {f[0] for f in q.flips}
    for j, job in enumerate(q.jobs):
        img_off, stride, slen, seg_off, seg_len, out_off, ostride, pat = job
        bad, ins = q.bad_of(j), q.inputs_of(j)
        assert len(ins) == t.N and not set(ins) & set(bad)
        assert stride >= A.enc_size(slen)
        assert seg_off % 4 == 0 and 0 < seg_len <= slen - seg_off
        assert ostride % 4 == 0 and ostride >= seg_len and out_off % 4 == 0
        if j in flipped:
            continue
        # a clean job: every input decodes to its shard, and the oracle's
        # ReconstructData over the inputs alone restores the missing data
        assert words[j] == 0, (name, j)
        shards = [None] * (t.N + t.M)
        for i in ins:
            raw = oracle.crc32b_decode(imgs[j][i].copy())
            assert np.array_equal(raw, q.data[j][i]), (name, j, i)
            shards[i] = raw
        if j % 5 == 0 and any(b < t.N for b in bad):
            present = [s is not None for s in shards]
            full = [s if s is not None else np.zeros(slen, np.uint8)
                    for s in shards]
            oracle.rs_reconstruct(t.N, t.M, full, present, data_only=True)
            for i in range(t.N):
                assert np.array_equal(full[i], q.data[j][i]), (name, j, i)
        # every shard named in the pattern, and every non-input parity, is
        # garbage whose frame CRCs are wrong
        for i in range(q.total):
            if i in bad or (i >= t.N and i not in ins):
                assert oracle.crc32b_verify(imgs[j][i].copy()) == 0, (j, i)
    # odd image base, strides of both parities, image order == job order but
    # row order is not
    assert q.delta % 2 == 1
    assert {job[1] % 2 for job in q.jobs} == {0, 1}
    rows = [job[5] for job in q.jobs]
    assert rows != sorted(rows)
    spans = sorted(reg for j in range(len(q.jobs)) for reg in q.row_regions(j))
    assert all(a[0] + a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    assert spans[-1][0] + spans[-1][1] == q.out_bytes
    ispans = sorted((job[0] + i * job[1], A.enc_size(job[2]))
                    for job in q.jobs for i in range(q.total))
    assert all(a[0] + a[1] <= b[0] for a, b in zip(ispans, ispans[1:]))
    assert ispans[-1][0] + ispans[-1][1] == q.img_bytes
    # patterns change from job to job
    assert all(a[7] != b[7] for a, b in zip(q.jobs, q.jobs[1:])
               if len(q.patterns) > 1)


@pytest.mark.parametrize("name", G.CORRUPT_QUEUES)
def test_corruption_queues_against_oracle(name):
    """Each flip does what its kind says, by the oracle alone, and at least
    half the jobs stay clean."""
    q = G.build(name)
    words = G.words(name)
    assert sum(1 for w in words if w == 0) * 2 >= len(words)
    assert sum(1 for w in words if w) >= 3
    seen = set()
    for j, sh, byte, mask in q.flips:
        slen, seg_off, seg_len = q.jobs[j][2:5]
        ins = q.inputs_of(j)
        f = byte // A.BLOCK
        if sh not in ins:
            kind = "non-input"
            assert words[j] == 0
        elif f not in G.touched(seg_off, seg_len):
            kind = "outside"
            assert words[j] == 0
        else:
            kind = "header" if byte % A.BLOCK < 4 else "payload"
            assert words[j] == 1 << sh, (name, j, hex(words[j]))
        seen.add(kind)
    assert {"payload", "header", "non-input"} <= seen, seen
    if name == "corrupt_rs63":
        assert "outside" in seen
    # jobs without a flip are clean
    flipped = {f[0] for f in q.flips}
    assert all(words[j] == 0 for j in range(len(words)) if j not in flipped)
