"""CPU checks of the shard write queue (gfrs_shard_write_queue):

 - the schedule the engine would upload (gfrs_compute_shard_write_queue_schedule,
   the same builder, GPU-free) against a Python restatement, for every queue of
   tests/_shardwq.py: bucket order, caller order, prefix sums of frames, total
   frames;
 - every validation code of the contract (include/gfrs.h) and the capacity
   refusal of the export;
 - the generator on its own: every expected image is accepted by
   pyoracle.shard_parse with the new ids and its footer CRC is the expected
   crc; on flipped sources the expected status is 0 exactly when
   pyoracle.shard_parse accepts the source and the ids match;
 - the sanitized stand-alone selftest of the builder
   (shard_write_queue_selftest.cpp).
"""
import os
import subprocess

import numpy as np
import pytest

import _arena as A
import _shardq as S
import _shardwq as W
from _arena import oracle
from test_queue_cpu import _host_compiler

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "cubefs_amd", "csrc")


# ---- the schedule, restated -----------------------------------------------------

def want_schedule(jobs):
    buckets, items, prefix, total = [], [], [], 0
    for src_image in (0, 1):
        mine = [(j, job) for j, job in enumerate(jobs)
                if bool(job[7] & W.SRC_IMAGE) == bool(src_image)]
        if not mine:
            continue
        buckets.append((src_image, len(items), len(mine)))
        sums = [0]
        for j, (src, size, _, _, _, _, img, flags) in mine:
            items.append((j, src, size, img, flags))
            sums.append(sums[-1] + -(-size // 65532))
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


@pytest.mark.parametrize("name", W.GPU_QUEUES)
def test_schedule_of_gpu_queues(name):
    q = W.build(name)
    rc, s = W.schedule(q.jobs)
    assert rc == 0
    check_schedule(q.jobs, s)
    kinds = [b[0] for b in s.buckets]
    if name in ("clean", "tiny"):
        assert kinds == [0, 1]
    if name == "all_raw":
        assert kinds == [0]
    if name in ("all_image", "one", "flips"):
        assert kinds == [1]
    if name == "one":
        assert s.prefix == [0, 2] and s.total_frames == 2
    if name == "tiny":
        assert s.prefix == [0, 3, 4, 0, 3, 4] and s.total_frames == 8
        assert [i[0] for i in s.items] == [0, 3, 1, 2]    # caller order
    if name == "clean":
        assert [i[0] for i in s.items] == \
            list(range(0, 20, 2)) + list(range(1, 20, 2))
        assert s.total_frames == 2 * sum(W.nframes(n) for n in W.LENS)


def test_schedule_frame_edges_and_caps():
    for size, nf in [(1, 1), (65531, 1), (65532, 1), (65533, 2), (131064, 2),
                     (131065, 3), ((1 << 32) - 1, 65541)]:
        for flags in (0, W.SRC_IMAGE):
            rc, s = W.schedule([(5, size, 1, 2, 3, 4, 8, flags)])
            assert rc == 0 and s.buckets == [(flags, 0, 1)], size
            assert s.prefix == [0, nf] and s.total_frames == nf, size
    jobs = [(j << 20, 1 << 18, 0, 0, 0, 0, j << 19, j % 2) for j in range(3)]
    assert W.schedule(jobs, item_cap=2)[0] == W.ERR_NOMEM
    assert W.schedule(jobs, item_cap=0)[0] == W.ERR_NOMEM
    assert W.schedule(jobs, item_cap=-1)[0] == W.ERR_NOMEM
    assert W.schedule(jobs, item_cap=3)[0] == 0


def test_schedule_validation():
    ok = (1, 100, 7, 9, 11, 13, 8, 0)
    names = ["src_off", "size", "bid", "vuid", "src_bid", "src_vuid",
             "img_off", "flags", "reserved"]

    def rc(job=ok, **kw):
        return W.schedule([job] if isinstance(job, tuple) else job, **kw)[0]

    def swap(**f):
        v = dict(zip(names, ok + (0,)))
        v.update(f)
        return tuple(v[n] for n in names)

    assert rc() == 0
    assert rc(swap(flags=W.SRC_IMAGE)) == 0
    # block length
    for bl in (0, -65536, 100, 65536 + 4):
        assert rc(block_len=bl) == W.ERR_BLOCK
    for bl in (4096, 131072, 65536 * 3):
        assert rc(block_len=bl) == W.ERR_UNSUPPORTED
    # size
    assert rc(swap(size=0)) == W.ERR_NO_DATA
    assert rc([ok, swap(size=0)]) == W.ERR_NO_DATA
    assert rc(swap(size=1 << 32)) == W.ERR_INVALID
    assert rc(swap(size=(1 << 32) - 1)) == 0
    # njobs
    assert rc(job=[]) == W.ERR_INVALID
    assert rc(njobs=-1) == W.ERR_INVALID
    # reserved, unknown flags
    assert rc(swap(reserved=1)) == W.ERR_INVALID
    assert rc(swap(flags=2)) == W.ERR_INVALID
    assert rc(swap(flags=0x80000000 | W.SRC_IMAGE)) == W.ERR_INVALID
    # alignment of the new image (dst itself counts as 4-aligned here); the
    # source needs none
    for off in (1, 2, 3, 6):
        assert rc(swap(img_off=off)) == W.ERR_INVALID
        assert rc(swap(src_off=off)) == 0
    assert rc([ok, swap(img_off=1, flags=W.SRC_IMAGE)]) == W.ERR_INVALID
    # the source ids are free
    assert rc(swap(src_bid=(1 << 64) - 1, src_vuid=0)) == 0


# ---- the generator on its own ---------------------------------------------------

def _parses(img):
    try:
        return oracle.shard_parse(img.copy())
    except ValueError:
        return None


@pytest.mark.parametrize("name", W.GPU_QUEUES)
def test_expected_images_against_shard_parse(name):
    """Every expected image is self-consistent by the oracle's reader, holds
    the new ids and the payload, and its footer carries the expected crc."""
    q = W.build(name)
    want = W.expected(name)
    for j, (job, img) in enumerate(zip(q.jobs, W.expected_images(name))):
        _, size, bid, vuid = job[:4]
        assert img.size == A.disk_size(size)
        assert _parses(img) == (bid, vuid, size), (name, j)
        assert S.be(img[-4:]) == want[j]["crc"], (name, j)
        assert want[j]["crc"] == oracle.crc32(q.payload(j).copy())
        assert np.array_equal(S.payload_of(img, size), q.payload(j))
        if not job[7] & W.SRC_IMAGE:
            assert want[j] == dict(status=0, crc=want[j]["crc"], bad_block=-1,
                                   bid=bid, vuid=vuid, size=size)


@pytest.mark.parametrize("name", ["clean", "flips"])
def test_expected_status_against_shard_parse(name):
    q = W.build(name)
    want = W.expected(name)
    nclean = nbad = 0
    for j, job in enumerate(q.jobs):
        if not job[7] & W.SRC_IMAGE:
            continue
        got = _parses(q.sources[j][1])
        accepted = got == (job[4], job[5], job[1])
        assert (want[j]["status"] == 0) == accepted, (name, j, want[j])
        nclean += accepted
        nbad += not accepted
    if name == "flips":
        assert nclean >= 4 and nbad >= 40       # the gap flips stay clean
    else:
        assert nclean == len(W.LENS) and nbad == 0


def test_generator_shapes():
    """What tests/test_gpu_shard_write_queue.py assumes of its inputs."""
    q = W.build("clean")
    assert [job[1] for job in q.jobs] == [s for s in W.LENS for _ in (0, 1)]
    assert [job[7] for job in q.jobs] == [0, W.SRC_IMAGE] * len(W.LENS)
    new = set()
    for j, job in enumerate(q.jobs):
        src_off, size, bid, vuid, sb, sv, img_off, flags = job
        assert src_off % 2 == 0                 # on an odd arena base
        assert img_off % 4 == 0
        assert all(x >> 56 and x & 0xFFFFFFFF and (x >> 32) & 0xFFFFFF
                   for x in (bid, vuid))        # all eight bytes in use
        if flags & W.SRC_IMAGE:
            assert (sb, sv) == S.ids(j) and (sb, sv) != (bid, vuid)
            assert _parses(q.sources[j][1]) == (sb, sv, size)
            assert np.array_equal(q.payload(j), S.raw(size, j))
        else:
            assert q.sources[j][1].size == size
        new.add((bid, vuid))
    assert len(new) == len(q.jobs)
    spans = sorted((job[6], A.disk_size(job[1])) for job in q.jobs)
    assert all(a[0] + a[1] < b[0] for a, b in zip(spans, spans[1:]))  # guarded
    assert spans[-1][0] + spans[-1][1] == q.dst_bytes
    assert [job[6] for job in q.jobs] != [s[0] for s in spans]
    gaps = {b[0] - (a[0] + a[1]) for a, b in zip(spans, spans[1:])}
    assert len(gaps) > 2                        # uneven
    # the dst arena's base is 4 mod 16 (tests/_arena.py): images whose payload
    # is 16-byte aligned and images whose payload is not both occur, at
    # multi-pass sizes
    al = {(job[6] + 4 + 36) % 16 == 0 for job in q.jobs if job[1] > 16384}
    assert al == {True, False}
    srcs = sorted((s[0], s[1].size) for s in q.sources)
    assert all(a[0] + a[1] < b[0] for a, b in zip(srcs, srcs[1:]))
    assert srcs[-1][0] + srcs[-1][1] < q.src_bytes
    t = W.build("tiny")
    assert sum(W.nframes(job[1]) for job in t.jobs if job[7]) == 4
    assert sum(W.nframes(job[1]) for job in t.jobs if not job[7]) == 4


def test_flip_queue_against_oracle():
    """Each flip does what its kind says, by the oracle alone; the expected
    image carries the flipped payload."""
    q = W.build("flips")
    want = W.expected("flips")
    bits = {"fcrc": S.BODY_CRC, "payload": S.BODY_CRC | S.FTR_CRC, "gap": 0,
            "hdr_crc": S.HDR_CRC, "hdr_magic": S.HDR_MAGIC | S.HDR_CRC,
            "hdr_bid": S.HDR_CRC | S.HDR_MISMATCH,
            "hdr_vuid": S.HDR_CRC | S.HDR_MISMATCH,
            "hdr_size": S.HDR_CRC | S.HDR_MISMATCH, "hdr_reserved": S.HDR_CRC,
            "want_bid": S.HDR_MISMATCH, "want_vuid": S.HDR_MISMATCH,
            "ftr_magic": S.FTR_MAGIC, "ftr_crc": S.FTR_CRC}
    assert set(q.kinds) == set(bits)
    assert all(job[7] == W.SRC_IMAGE for job in q.jobs)
    assert sorted({job[1] for job in q.jobs}) == S.FLIP_LENS
    for j, job in enumerate(q.jobs):
        kind, w = q.kinds[j], want[j]
        assert w["status"] == bits[kind], (j, kind, job, w)
        assert (w["bad_block"] >= 0) == bool(w["status"] & S.BODY_CRC)
        clean = S.raw(job[1], j)
        assert np.array_equal(q.payload(j), clean) == (kind != "payload")
        assert (w["crc"] == oracle.crc32(clean.copy())) == (kind != "payload")
    two = [j for j in range(len(q.jobs))
           if sum(1 for k, _, _ in q.flips if k == j) == 2]
    assert two and all(want[j]["bad_block"] == 0 for j in two)
    assert any(w["bad_block"] > 0 for w in want)
    assert q.gap_flips


# ---- the builder under the sanitizers, as a host program -------------------------

def test_shard_write_queue_selftest_sanitized(tmp_path):
    """The schedule builder under ASan + UBSan as a stand-alone program: a
    plain host compiler, gfrs_plan.cpp + gfrs_gf.cpp, no Python in the
    process."""
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host compiler with the sanitizer runtimes")
    exe = str(tmp_path / "shard_write_queue_selftest")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall",
                    "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    os.path.join(HERE, "shard_write_queue_selftest.cpp"),
                    os.path.join(CSRC, "gfrs_plan.cpp"),
                    os.path.join(CSRC, "gfrs_gf.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "shard write queue selftest OK" in r.stdout
