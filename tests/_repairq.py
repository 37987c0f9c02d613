"""Repair queues for the gfrs_reconstruct_verify_queue tests.

A queue is what ShardRecover.repair sees (worker_slice_recover.go:804-888):
jobs of different shard lengths, each with its own erasure pattern, laid out
in one buffer.  Everything the GPU module (tests/test_gpu_queue.py) feeds to
the engine is generated here, so tests/test_queue_cpu.py can check the same
queues against the schedule builder and against the oracle alone.

Expectations come from _verdict.expected (the reference's Reconstruct +
Verify of one stripe), job by job - never from the engine.

Shard lengths come from the queue kernel's constants (16-byte vectors,
4096-byte tiles): 1, 15 (ragged path only), 16 (one vector), 17, 33 (vectors
+ ragged tail), 4095, 4096, 4097 (tile edge), 8209 (two tiles + vector +
ragged byte).
"""
import ctypes
import functools

import _arena as A
import _verdict as V
from _arena import L, Arena, vp

from cubefs_amd import runtime
from cubefs_amd.ec import _tactic_struct

LENS = [1, 15, 16, 17, 33, 4095, 4096, 4097, 8209]
TILE = 4096
ROWS = 4          # rows per launch
GAPS = [1, 3, 7, 5, 11, 1, 9, 3, 13, 7, 5]   # odd bytes between jobs
PLAN_RS, PLAN_LRC = 1, 2
ERR_TOO_FEW, ERR_NO_DATA, ERR_INVALID, ERR_NOMEM, ERR_UNSUPPORTED = \
    -2, -4, -6, -102, -103


class Queue:
    """jobs: [(off, slen, pattern index)]; data[j]: the (total, slen)
    stripe of job j as the engine finds it, one bit flipped in a surviving
    shard where flips[j] = (column, byte, mask) is set."""

    def __init__(self, name, tname, patterns, picks,
                 gap=lambda j: GAPS[j % len(GAPS)], delta=1,
                 corrupt=lambda j: j % 3 == 0, cols=None):
        self.name, self.tname = name, tname
        self.t = V.get_tactic(tname)
        self.total = self.t.N + self.t.M + self.t.L
        self.patterns = [list(p) for p in patterns]
        self.delta = delta
        self.jobs, self.data, self.flips = [], [], []
        off, seen = 0, {}
        need = {}
        for slen, _ in picks:
            need[slen] = need.get(slen, 0) + 1
        for j, (slen, pat) in enumerate(picks):
            ref = A.ref_stripes(self.t, need[slen], slen, seed=21)
            s = seen.get(slen, 0)
            seen[slen] = s + 1
            stripe = ref[s].copy()
            flip = None
            if corrupt(j):
                bad = self.patterns[pat]
                alive = [c for c in (cols or range(self.total))
                         if c not in bad]
                col = alive[(j // 3) % len(alive)]
                pos = V.rs_positions(slen)
                flip = (col, pos[(j // 3) % len(pos)], 1 << (j % 8))
                stripe[flip[0], flip[1]] ^= flip[2]
            self.jobs.append((off, slen, pat))
            self.data.append(stripe)
            self.flips.append(flip)
            off += self.total * slen + gap(j)
        last = self.jobs[-1]
        self.nbytes = last[0] + self.total * last[1]

    # ---- C ABI arguments ----
    def qjobs(self, jobs=None):
        jobs = self.jobs if jobs is None else jobs
        arr = (runtime.QJob * len(jobs))()
        for j, (off, slen, pat) in enumerate(jobs):
            arr[j] = runtime.QJob(off, slen, pat, 0)
        return arr

    def bad_lists(self, patterns=None):
        return bad_lists(self.patterns if patterns is None else patterns)

    def bad_of(self, j):
        return self.patterns[self.jobs[j][2]]


def bad_lists(patterns):
    flat = [i for p in patterns for i in p]
    offs = [0]
    for p in patterns:
        offs.append(offs[-1] + len(p))
    return A.i32s(flat or [0]), A.i32s(offs)


def _interleaved(lens, npat, njobs):
    """Job j: length j mod len(lens); the pattern advances by one more every
    len(lens) jobs, so ordering by pattern permutes the jobs and every
    length meets several patterns."""
    return [(lens[j % len(lens)], (j + j // len(lens)) % npat)
            for j in range(njobs)]


@functools.lru_cache(maxsize=None)
def build(name):
    if name == "rs63_mixed":
        # [] 3 compare rows; [1] 4 rows; [0,5] 5 rows = steps of 4 + 1;
        # [0,2,4] 6 rows (nbad = m: nothing left to detect with);
        # [7] a parity written; [1,8] data + parity
        pats = [[], [1], [0, 5], [0, 2, 4], [7], [1, 8]]
        return Queue(name, "EC6P3", pats, _interleaved(LENS, 6, 54))
    if name == "rs63_uniform":
        # constant length and gap: also a gfrs_reconstruct_verify_batch
        return Queue(name, "EC6P3", [[1, 7]], [(4097, 0)] * 7,
                     gap=lambda j: 5)
    if name == "rs66_depth":
        # 3..6 bad of RS(6+6): 9, 9, 11 and 12 rows = three steps
        pats = [[0, 1, 2], [1, 3, 5, 8], [0, 1, 2, 3, 4],
                [0, 1, 2, 3, 4, 5], [4, 9, 10, 11]]
        return Queue(name, "EC6P6", pats,
                     _interleaved([17, 4097, 33, 8209, 16], 5, 20))
    if name == "rs124_k12":
        pats = [[], [1], [0, 13], [2, 5, 11, 15]]
        return Queue(name, "EC12P4", pats,
                     _interleaved([4095, 33, 8209, 1, 4096], 4, 15))
    if name == "rs134_w17":
        pats = [[16], [0, 12], [3], [1, 2, 14]]
        return Queue(name, "EC13P4", pats,
                     _interleaved([4097, 15, 8209, 16, 33], 4, 15))
    if name == "lrc_single":
        # LRC12P2L2 single-pass plans: nothing lost, data, global parity,
        # local parity, mixes; every flip lands in a surviving LOCAL parity
        # (14 or 15), which only the local check rows can detect
        pats = [[], [0], [12], [14], [3, 15], [0, 13]]
        return Queue(name, "LRC12P2L2", pats,
                     _interleaved([33, 4097, 17, 8209], 6, 24),
                     cols=[14, 15])
    if name == "lrc_slow":
        # EC6P3L3 is outside the single-pass budget (m + l = 6): every
        # pattern is slow.  The local-stripe patterns of _verdict.subset.
        t = V.get_tactic("EC6P3L3")
        n, m, l = t.N, t.M, t.L
        pats = [[n + m], [n + m + l - 1, 0], [n, n + m], [0, n + m, n], []]
        return Queue(name, "EC6P3L3", pats,
                     _interleaved([33, 4097, 17], 5, 10),
                     cols=list(range(n + m, n + m + l)))
    if name == "seq_small":
        # a step of tests/test_gpu_sequences.py: six short jobs
        return Queue(name, "EC6P3", [[1], [0, 5], [7]],
                     _interleaved([1000, 4093, 33], 3, 6))
    raise KeyError(name)


GPU_QUEUES = ["rs63_mixed", "rs63_uniform", "rs66_depth", "rs124_k12",
              "rs134_w17", "lrc_single", "lrc_slow"]


@functools.lru_cache(maxsize=None)
def expectations(name):
    """[(reconstructed (total, slen), failed) or UNDECODABLE] per job."""
    q = build(name)
    return [V.expected(q.t, q.data[j], q.bad_of(j))
            for j in range(len(q.jobs))]


# ---- schedule (GPU-free export) ---------------------------------------------

class Schedule:
    pass


def schedule(t, jobs, patterns, item_cap=None, bucket_cap=64):
    """gfrs_compute_queue_schedule -> (rc, Schedule or None)."""
    nj = len(jobs)
    qj = (runtime.QJob * max(1, nj))()
    for j, job in enumerate(jobs):
        qj[j] = runtime.QJob(*job) if len(job) == 4 else \
            runtime.QJob(job[0], job[1], job[2], 0)
    bad, boff = bad_lists(patterns)
    item_cap = nj * 8 if item_cap is None else item_cap
    items = (runtime.QItem * max(1, item_cap))()
    prefix = (ctypes.c_uint64 * max(1, item_cap + bucket_cap))()
    buckets = (runtime.QBucket * max(1, bucket_cap))()
    nout = (ctypes.c_int32 * max(1, len(patterns)))()
    slow = (ctypes.c_uint8 * max(1, len(patterns)))()
    slow_jobs = (ctypes.c_int32 * max(1, nj))()
    ni, nb, ns = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    ts = _tactic_struct(t)
    rc = L().gfrs_compute_queue_schedule(
        ctypes.byref(ts), qj, nj, bad, boff, len(patterns), item_cap,
        bucket_cap, items, prefix, ctypes.byref(ni), buckets,
        ctypes.byref(nb), nout, slow, slow_jobs, ctypes.byref(ns))
    if rc != 0:
        return rc, None
    s = Schedule()
    s.items = [(i.job, i.pattern, i.row_off, i.off, i.shard_len, i.reserved)
               for i in items[:ni.value]]
    s.buckets = [(b.g, b.gm, b.first, b.count) for b in buckets[:nb.value]]
    s.prefix = list(prefix[:ni.value + nb.value])
    s.nout = list(nout[:len(patterns)])
    s.slow = [bool(x) for x in slow[:len(patterns)]]
    s.slow_jobs = list(slow_jobs[:ns.value])
    return 0, s


def plan_rows(t, bad):
    """(rc, nout) of the single-pass plan gfrs_compute_plan builds."""
    kind = PLAN_LRC if t.L else PLAN_RS
    cap = 64
    total = t.N + t.M + t.L
    inn, out = (ctypes.c_int32 * cap)(), (ctypes.c_int32 * cap)()
    rows = (ctypes.c_uint8 * (cap * max(t.N, total)))()
    nin, nout, rowk = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    cmp_mask, colpack = ctypes.c_uint32(), ctypes.c_uint32()
    ts = _tactic_struct(t)
    rc = L().gfrs_compute_plan(ctypes.byref(ts), kind, A.i32s(bad or [0]),
                               len(bad), cap, inn, ctypes.byref(nin), out,
                               ctypes.byref(nout), rows, ctypes.byref(rowk),
                               ctypes.byref(cmp_mask), ctypes.byref(colpack))
    return rc, nout.value


def single_pass_budget(t):
    """The engine's LRC single-pass budget (include/gfrs.h, slow patterns)."""
    return t.L == 0 or (t.M + t.L <= 4 and t.N + t.M + t.L <= 16)


# ---- GPU runner: one call, whole arena checked ---------------------------------

def load(q, dev, seed=70):
    a = Arena(dev, q.nbytes, q.delta, seed=seed)
    for j, (off, slen, pat) in enumerate(q.jobs):
        for i in range(q.total):
            if i not in q.patterns[pat]:
                a.put(off + i * slen, q.data[j][i])
    a.upload()
    return a


def call(enc, a, q, jobs=None, patterns=None):
    jobs = q.jobs if jobs is None else jobs
    bad, boff = q.bad_lists(patterns)
    bm = A.bitmap(len(jobs))
    npat = len(q.patterns if patterns is None else patterns)
    rc = L().gfrs_reconstruct_verify_queue(enc._ctx, vp(a.ptr), q.qjobs(jobs),
                                           len(jobs), bad, boff, npat, bm)
    return rc, A.bits(bm, len(jobs))


def wanted(q, a):
    """(expected arena, failed jobs, unspecified regions) from the oracle."""
    exp = expectations(q.name)
    want = a.expect()
    fails, unspec = [], []
    for j, (off, slen, pat) in enumerate(q.jobs):
        rec, failed = exp[j]
        for i in q.patterns[pat]:
            a.put(off + i * slen, rec[i], want)
        if failed:
            fails.append(j)
            if q.t.L:   # LRC: a failed stripe's bad regions are unspecified
                unspec += [(off + i * slen, slen) for i in q.patterns[pat]]
    return want, fails, unspec


def run(dev, name, what=""):
    q = build(name)
    enc = A.encoder(q.t)
    a = load(q, dev)
    rc, got = call(enc, a, q)
    what = "%s queue %s" % (what, name)
    A.ok(rc, what)
    want, fails, unspec = wanted(q, a)
    assert got == fails, (what, got, fails)
    a.check(want, unspec, what=what)
    return a, got
