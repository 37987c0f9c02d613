"""CPU checks of the shard read queue (gfrs_shard_read_queue):

 - the schedule the engine would upload (gfrs_compute_shard_read_queue_schedule,
   the same builder, GPU-free) against a Python restatement, for every queue of
   tests/_shardq.py: buckets, order, prefix sums of touched frames, total
   frames; and the degenerate queues (one job, all NO_OUT, none NO_OUT);
 - every validation code of the contract (include/gfrs.h) and the capacity
   refusal of the export;
 - the yardstick on its own: on clean and corrupted images the generator's
   expected status of a whole-shard FOOTER job is 0 exactly when
   pyoracle.shard_parse accepts the image and the ids match;
 - the sanitized stand-alone selftest of the builder
   (shard_read_queue_selftest.cpp).
"""
import os
import subprocess

import numpy as np
import pytest

import _arena as A
import _shardq as S
from _arena import oracle
from test_queue_cpu import _host_compiler

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "cubefs_amd", "csrc")


# ---- the schedule, restated -----------------------------------------------------

def want_schedule(jobs):
    buckets, items, prefix, total = [], [], [], 0
    for no_out in (0, 1):
        mine = [(j, job) for j, job in enumerate(jobs)
                if bool(job[7] & S.NO_OUT) == bool(no_out)]
        if not mine:
            continue
        buckets.append((no_out, len(items), len(mine)))
        sums = [0]
        for j, (img, size, _, _, frm, to, out, flags) in mine:
            items.append((j, img, size, frm, to, out, flags))
            sums.append(sums[-1] + len(S.touched(frm, to)))
        prefix += sums
        total += sums[-1]
    return buckets, items, prefix, total


def check_schedule(jobs, s):
    buckets, items, prefix, total = want_schedule(jobs)
    assert s.buckets == buckets
    assert s.items == items
    assert s.prefix == prefix
    assert s.total_frames == total
    assert len(s.buckets) <= 2


@pytest.mark.parametrize("name", S.GPU_QUEUES)
def test_schedule_of_gpu_queues(name):
    q = S.build(name)
    rc, s = S.schedule(q.jobs)
    assert rc == 0
    check_schedule(q.jobs, s)
    kinds = [b[0] for b in s.buckets]
    if name in ("clean", "flips", "tiny"):
        assert kinds == [0, 1]
    if name == "all_no_out":
        assert kinds == [1]
    if name in ("none_no_out", "one"):
        assert kinds == [0]
    if name == "one":
        assert s.prefix == [0, 2] and s.total_frames == 2
    if name == "tiny":
        assert s.prefix == [0, 3, 4, 0, 3, 4] and s.total_frames == 8
    if name == "clean":
        # a touched-frame sum, not a shard-frame sum
        assert any(len(S.touched(j[4], j[5])) < (j[1] - 1) // S.PAYLOAD + 1
                   for j in q.jobs)
        assert s.total_frames < sum((j[1] - 1) // S.PAYLOAD + 1
                                    for j in q.jobs)


def test_schedule_touched_frame_edges():
    size = 200000
    for frm, to, nf in [(0, 65532, 1), (0, 65533, 2), (65528, 65532, 1),
                        (65528, 65533, 2), (65532, 65533, 1), (4, size, 4),
                        (131064, 131065, 1), (131060, 131068, 2),
                        (196596, size, 1)]:
        rc, s = S.schedule([(5, size, 1, 2, frm, to, 0, 0)])
        assert rc == 0 and s.buckets == [(0, 0, 1)], (frm, to)
        assert s.prefix == [0, nf] and s.total_frames == nf, (frm, to)
    jobs = [(j << 20, 1 << 18, 0, 0, 0, 4, 64 * j, 0) for j in range(3)]
    assert S.schedule(jobs, item_cap=2)[0] == S.ERR_NOMEM
    assert S.schedule(jobs, item_cap=0)[0] == S.ERR_NOMEM
    assert S.schedule(jobs, item_cap=3)[0] == 0


def test_schedule_validation():
    ok = (1, 100, 7, 9, 4, 100, 8, 0)

    def rc(job=ok, **kw):
        return S.schedule([job] if isinstance(job, tuple) else job, **kw)[0]

    def swap(**f):
        names = ["img_off", "size", "bid", "vuid", "frm", "to", "out_off",
                 "flags", "reserved"]
        v = dict(zip(names, ok + (0,)))
        v.update(f)
        return tuple(v[n] for n in names)

    assert rc() == 0
    # block length
    for bl in (0, -65536, 100, 65536 + 4):
        assert rc(block_len=bl) == S.ERR_BLOCK
    for bl in (4096, 131072, 65536 * 3):
        assert rc(block_len=bl) == S.ERR_UNSUPPORTED
    # size
    assert rc(swap(size=0)) == S.ERR_NO_DATA
    assert rc([ok, swap(size=0)]) == S.ERR_NO_DATA
    assert rc(swap(size=1 << 32, to=1 << 32)) == S.ERR_INVALID
    assert rc(swap(size=(1 << 32) - 1, to=(1 << 32) - 1)) == 0
    # njobs
    assert rc(job=[]) == S.ERR_INVALID
    assert rc(njobs=-1) == S.ERR_INVALID
    # reserved, unknown flags
    assert rc(swap(reserved=1)) == S.ERR_INVALID
    assert rc(swap(flags=4)) == S.ERR_INVALID
    assert rc(swap(flags=0x80000000 | S.NO_OUT)) == S.ERR_INVALID
    # the range
    assert rc(swap(frm=100)) == S.ERR_INVALID
    assert rc(swap(frm=8, to=4)) == S.ERR_INVALID
    assert rc(swap(to=101)) == S.ERR_INVALID
    assert rc(swap(frm=2)) == S.ERR_INVALID
    assert rc(swap(frm=96, to=97)) == 0
    assert rc(swap(frm=(1 << 64) - 4, to=(1 << 64) - 1)) == S.ERR_INVALID
    # FOOTER wants the whole shard
    assert rc(swap(flags=S.FOOTER)) == S.ERR_INVALID
    assert rc(swap(flags=S.FOOTER, frm=0, to=96)) == S.ERR_INVALID
    assert rc(swap(flags=S.FOOTER, frm=0)) == 0
    assert rc(swap(flags=S.FOOTER | S.NO_OUT, frm=0)) == 0
    # alignment of the output (out itself counts as 4-aligned here)
    assert rc(swap(out_off=6)) == S.ERR_INVALID
    assert rc(swap(out_off=6, flags=S.NO_OUT)) == 0
    assert rc([ok, swap(out_off=1)]) == S.ERR_INVALID


# ---- the yardstick on its own -------------------------------------------------

def _parses(img, job):
    """pyoracle.shard_parse accepts the image and tells the job's ids."""
    try:
        got = oracle.shard_parse(img.copy())
    except ValueError:
        return False
    return got == (job[2], job[3], job[1])


@pytest.mark.parametrize("name", ["clean", "flips"])
def test_expected_status_against_shard_parse(name):
    q = S.build(name)
    want = S.expected(name)
    nclean = nbad = 0
    for j, job in enumerate(q.jobs):
        img = q.images[q.image_of[j]][5]
        whole = job[:4] + (0, job[1], job[6], S.FOOTER)
        e = S.expect_one(img, whole)
        assert (e["status"] == 0) == _parses(img, whole), (name, j, e)
        nclean += e["status"] == 0
        nbad += e["status"] != 0
        if job[7] & S.FOOTER:
            assert want[j] == e
    assert nclean >= 10
    if name == "flips":
        assert nbad >= 40
    else:
        assert nbad == 0


def test_generator_shapes():
    """What tests/test_gpu_shard_read_queue.py assumes of its inputs."""
    q = S.build("clean")
    want = S.expected("clean")
    assert [im[1] for im in q.images] == S.LENS
    seen = set()
    for j, job in enumerate(q.jobs):
        off, size, bid, vuid, frm, to, out, flags = job
        assert off % 2 == 0                 # on an odd arena base
        assert frm % 4 == 0 and 0 <= frm < to <= size
        if flags & S.FOOTER:
            assert (frm, to) == (0, size)
            assert want[j]["crc"] == oracle.crc32(q.images[q.image_of[j]][4]
                                                  .copy())
        else:
            assert want[j]["crc"] == 0
        assert want[j]["status"] == 0 and want[j]["bad_block"] == -1
        assert (want[j]["bid"], want[j]["vuid"], want[j]["size"]) == \
            (bid, vuid, size)
        assert np.array_equal(S.want_bytes(q, j),
                              S.payload_of(q.images[q.image_of[j]][5],
                                           size)[frm:to])
        seen.add((size, frm, to - frm, flags))
    for size in S.LENS:
        for off, n in S.G.segments(size):
            assert (size, off, n, 0) in seen and (size, off, n, S.NO_OUT) in seen
        assert (size, 0, size, S.FOOTER) in seen
        assert (size, 0, size, S.FOOTER | S.NO_OUT) in seen
    rows = sorted((j[6], j[5] - j[4]) for j in q.jobs if not j[7] & S.NO_OUT)
    assert all(a[0] + a[1] < b[0] for a, b in zip(rows, rows[1:]))  # guarded
    assert all(r[0] % 4 == 0 for r in rows)
    assert rows[-1][0] + rows[-1][1] == q.out_bytes
    assert [j[6] for j in q.jobs if not j[7] & S.NO_OUT] != [r[0] for r in rows]
    spans = sorted((im[0], im[5].size) for im in q.images)
    assert all(a[0] + a[1] < b[0] for a, b in zip(spans, spans[1:]))


def test_flip_queue_against_oracle():
    """Each flip does what its kind says, by the oracle alone."""
    q = S.build("flips")
    want = S.expected("flips")
    bits = {"fcrc": S.BODY_CRC, "payload": S.BODY_CRC, "outside": 0, "gap": 0,
            "hdr_crc": S.HDR_CRC, "hdr_magic": S.HDR_MAGIC | S.HDR_CRC,
            "hdr_bid": S.HDR_CRC | S.HDR_MISMATCH,
            "hdr_vuid": S.HDR_CRC | S.HDR_MISMATCH,
            "hdr_size": S.HDR_CRC | S.HDR_MISMATCH, "hdr_reserved": S.HDR_CRC,
            "want_bid": S.HDR_MISMATCH, "want_vuid": S.HDR_MISMATCH,
            "ftr_magic": S.FTR_MAGIC, "ftr_crc": S.FTR_CRC,
            "ftr_magic_plain": 0, "ftr_crc_plain": 0}
    seen = set()
    for j, job in enumerate(q.jobs):
        kind, w = q.kinds[j], want[j]
        footer = bool(job[7] & S.FOOTER)
        st = bits[kind]
        if kind == "payload" and footer:
            st |= S.FTR_CRC                 # the payload's CRC moved too
        assert w["status"] == st, (j, kind, job, w)
        assert (w["bad_block"] >= 0) == bool(st & S.BODY_CRC)
        if st & S.BODY_CRC:
            assert w["bad_block"] in S.touched(job[4], job[5])
        if not footer:
            assert w["crc"] == 0
        seen.add((kind, footer, bool(job[7] & S.NO_OUT)))
    assert set(bits) == {k for k, _, _ in seen}
    for kind in ("fcrc", "payload", "hdr_crc", "ftr_magic_plain"):
        assert {(kind, False, False), (kind, False, True)} <= seen, kind
    assert ("ftr_crc", True, False) in seen or ("ftr_crc", True, True) in seen
    # two bad frames: the lowest is reported
    two = [j for j in range(len(q.jobs))
           if sum(1 for k, _, _ in q.flips if k == q.image_of[j]) == 2]
    assert two and all(want[j]["bad_block"] ==
                       S.touched(q.jobs[j][4], q.jobs[j][5])[0] for j in two)
    assert any(want[j]["bad_block"] > 0 for j in range(len(q.jobs)))


# ---- the builder under the sanitizers, as a host program -------------------------

def test_shard_read_queue_selftest_sanitized(tmp_path):
    """The schedule builder under ASan + UBSan as a stand-alone program: a
    plain host compiler, gfrs_plan.cpp + gfrs_gf.cpp, no Python in the
    process."""
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host compiler with the sanitizer runtimes")
    exe = str(tmp_path / "shard_read_queue_selftest")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall",
                    "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    os.path.join(HERE, "shard_read_queue_selftest.cpp"),
                    os.path.join(CSRC, "gfrs_plan.cpp"),
                    os.path.join(CSRC, "gfrs_gf.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "shard read queue selftest OK" in r.stdout
