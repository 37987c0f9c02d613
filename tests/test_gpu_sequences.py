"""Back-to-back call sequences: what a call does to the call before it.

Every sequence runs on one fresh context with the stream held busy by a
plug (tests/_sequence.py): the steps are issued in order with nothing in
between, the context is synchronized once, and then every step's arenas
are compared with the oracle, guards and padding included.  This pins the
ordering contract of include/gfrs.h: the declared outputs of a call are
what that call alone would produce, whatever calls follow it.

The named sequence (first test) failed before the engine waited out a
queued id upload in every writer of the context's pinned staging:
gfrs_shard_write_batch returns with the copy of its bids/vuids out of
stage_pin still queued, and the pointer table of a following
gfrs_encode_idx, gfrs_update_idx or pointer-table gfrs_encode / gfrs_verify /
gfrs_reconstruct overwrote them, so the images' headers carried pointer
values and a header CRC over them.  The stream-switch sequences failed too
(ptr_buf rewritten from the new stream under the finalize kernel queued on
the old one), and so did the legacy repair tail.  The GFRS_MEM_HOST and
growth sequences never failed: hipHostFree / hipFree drain the device.
DESIGN.md section 16 has the table.
"""
import os
import subprocess
import sys

import pytest

torch = pytest.importorskip("torch")

import _arena as A  # noqa: E402
import _sequence as S  # noqa: E402

pytestmark = pytest.mark.gpu

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = 5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def tactic(name):
    from cubefs_amd import codemode
    return codemode.get_tactic(name)


def writer(k=0, slen=4093, nsh=4):
    """gfrs_shard_write_batch of nsh shards with id set k, odd layout."""
    return A.ShardWriteBatch(slen, nsh, pad=1, delta=1, extra=12, ids=k,
                             seed=24 + 2 * k, what="write#%d" % k)


def named_followers(t):
    """name -> (step, cold): every call that writes the context's pinned
    staging from the host.  The GFRS_MEM_HOST stripes ((n+m) x 4093 B) are
    larger than the id block, so stage_pin has to grow under the pending
    copy: those steps stay out of the warm-up."""
    ref = A.ref_stripes(t, 1, 4093, seed=5)
    f = {"encode_idx": (A.EncodeIdx(t, ref), False),
         "update_idx": (A.UpdateIdx(t, ref), False),
         "shard_write_again": (writer(1, slen=1000), False)}
    for host in (False, True):
        tag = "host" if host else "ptr"
        f["encode_" + tag] = (A.Encode(t, ref, host), host)
        f["verify_" + tag] = (A.Verify(t, ref, host, flip=True), host)
        f["reconstruct_" + tag] = (A.Reconstruct(t, ref, host), host)
    return f


NAMED = ["update_idx", "encode_ptr", "verify_ptr", "reconstruct_ptr",
         "encode_host", "verify_host", "reconstruct_host",
         "shard_write_again"]


def run_pair(r, producer, follower, cold, what):
    r.run([producer, follower], cold=[follower] if cold else (), what=what)


# ---- the named sequence ------------------------------------------------------

def test_shard_write_then_encode_idx(dev):
    """plug -> gfrs_shard_write_batch (4 shards, distinct bids and vuids) ->
    gfrs_encode_idx over all data shards.  With RS(6+3) the first
    encode_idx pointer table ((1 + m) x 8 = 32 bytes) lands on bids[0..3]
    in the pinned staging.  All four images equal oracle.shard_write(raw_j,
    bid_j, vuid_j) and the parity equals the oracle's."""
    t = tactic("EC6P3")
    r = S.Runner(dev, t)
    f, _ = named_followers(t)["encode_idx"]
    r.run([writer(), f], what="shard_write -> encode_idx")


@pytest.mark.parametrize("name", NAMED)
def test_shard_write_then(dev, name):
    t = tactic("EC6P3")
    r = S.Runner(dev, t)
    f, cold = named_followers(t)[name]
    run_pair(r, writer(), f, cold, "shard_write -> " + name)


@pytest.mark.parametrize("name", ["encode_idx"] + NAMED)
def test_shard_write_pair_then(dev, name):
    """Two gfrs_shard_write_batch back to back behind the plug, then the
    follower: the call pattern of the legacy repair tail (one
    shard_write_batch per lost column), issued by hand.  The second write
    waits in the engine's guard until the first one's upload ran, which
    drains the plug: the window is asserted before the two writes."""
    t = tactic("EC6P6")
    r = S.Runner(dev, t)
    f, cold = named_followers(t)[name]
    r.run([writer(0), writer(2, slen=1000, nsh=5), f],
          cold=[f] if cold else (), what="write, write -> " + name,
          windows=2)


@pytest.mark.parametrize("name", ["encode_idx"] + NAMED)
def test_legacy_repair_tail_then(dev, name):
    """gfrs_repair_batch on RS(6+6) with two lost shards takes the legacy
    path: reconstruct+verify (which synchronizes for the fail words), then
    one async gfrs_shard_write_batch per lost column.  The follower comes
    right behind that tail.  The plug cannot outlast the call's own
    synchronize, so the window is asserted before the repair call only.
    (Before the fix the followers that upload a pointer table first thing
    failed here all the same: the tail's last id copy had not run yet.)"""
    t = tactic("EC6P6")
    r = S.Runner(dev, t)
    f, cold = named_followers(t)[name]
    p = A.RepairBatch(t, A.ref_stripes(t, 4, 4093), [1, 7], pad=52, delta=1,
                      extra=12, what="legacy repair")
    run_pair(r, p, f, cold, "legacy repair -> " + name)
    assert p.fails == []


# ---- growth under queued work ------------------------------------------------

def test_id_table_growth_under_queued_write(dev):
    """4 ids, then 3000: ptr_buf and stage_pin both grow (free + allocate)
    while the first call's copy, CRC and finalize kernels are still queued.
    Both sets of images are exact."""
    t = tactic("EC6P3")
    r = S.Runner(dev, t)
    big = A.ShardWriteBatch(1000, 3000, ids=3, seed=50, what="write 3000")
    r.run([writer(), big], cold=[big], what="growth")


# ---- producer x follower -----------------------------------------------------

def producers(t):
    ref = A.ref_stripes(t, NS, 4093)
    if t.M > 3:
        # m + l > 4: encode_frame_batch composes encode_batch +
        # crc32b_encode_batch (contiguous stripes only)
        return {"encode_frame_composed": A.EncodeFrameBatch(
            t, A.ref_stripes(t, NS, 1000), 0, 7, 12, composed=True,
            what="P encode_frame composed")}
    return {
        "encode_batch": A.EncodeBatch(t, ref, 52, 1, what="P"),
        "reconstruct_batch": A.ReconstructBatch(t, ref, [1, 7], 52, 1,
                                                what="P"),
        "encode_frame_small": A.EncodeFrameBatch(
            t, A.ref_stripes(t, NS, 1000), 52, 1, 12,
            what="P encode_frame small"),
        "encode_frame_fused": A.EncodeFrameBatch(
            t, A.ref_stripes(t, 4, 70001), 52, 1, 12,
            what="P encode_frame fused"),
        "crc32b_encode_batch": A.CrcEncodeBatch(4093, 4, 1, 1, 12, what="P"),
        "shard_write_batch": writer(),
    }


PRODUCERS = [("EC6P3", "encode_batch"), ("EC6P3", "reconstruct_batch"),
             ("EC6P3", "encode_frame_small"), ("EC6P3", "encode_frame_fused"),
             ("EC6P6", "encode_frame_composed"),
             ("EC6P3", "crc32b_encode_batch"), ("EC6P3", "shard_write_batch")]


def families(t):
    """One step per entry-point family, in arenas of their own."""
    ref = A.ref_stripes(t, NS, 1000, seed=2)
    one = A.ref_stripes(t, 1, 4093, seed=5)
    small = t.M <= 3
    queues = (("_repairq", "seq_small" if small else "rs66_depth"),
              ("_repairimgq", "seq_small" if small else "rs66_inplace"),
              ("_encq", "seq_small" if small else "rs66_slow"),
              ("_readq", "seq_small" if small else "rs66_slow"))
    return [A.Reconstruct(t, one, what="F"),
            A.EncodeIdx(t, one, what="F"),
            A.VerifyBatch(t, ref, 1, 7, what="F"),
            A.ReconstructVerifyBatch(t, ref, [2, 6], 1, 7, what="F"),
            # fused for m + l <= 4, the legacy path otherwise
            A.RepairBatch(t, ref, [7, 2], 1, 7, 12, what="F repair_batch"),
            A.CrcVerifyBatch(4093, 4, 1, 7, what="F"),
            A.SizedEncode(70001, what="F"),
            A.ShardParseBatch(1000, 4, 1, 7, what="F")] + \
        [A.QueueCall(m, n, what="F") for m, n in queues]


@pytest.mark.parametrize("tname,pname", PRODUCERS,
                         ids=[p for _, p in PRODUCERS])
def test_async_producer_then_every_family(dev, tname, pname):
    """P returns with its work queued; F follows with nothing in between, in
    arenas of its own.  P's arena comes back exact whatever F is, and F's
    too.  A failure names the pair."""
    t = tactic(tname)
    r = S.Runner(dev, t)
    p = producers(t)[pname]
    for f in families(t):
        r.run([p, f], what="%s -> %s" % (pname, f.what))


# ---- same call twice, different arguments, no sync between ------------------

def test_reconstruct_batch_twice(dev):
    t = tactic("EC6P3")
    ref = A.ref_stripes(t, NS, 4093)
    S.Runner(dev, t).run(
        [A.ReconstructBatch(t, ref, [1, 7], 52, 1, seed=8, what="first"),
         A.ReconstructBatch(t, ref, [0, 8], 1, 7, seed=9, what="second")],
        what="reconstruct_batch x2")


def test_encode_idx_two_accumulations(dev):
    """encode_idx over all data shards of two stripes, alternating: call k
    uploads another pointer table than call k - 1."""
    t = tactic("EC6P3")
    S.Runner(dev, t).run([writer(),
                          A.EncodeIdx(t, A.ref_stripes(t, 2, 4093, seed=6))],
                         what="encode_idx x2")


def test_shard_write_batch_three_times(dev):
    """Other ids and counts each time.  Every write but the first waits in
    the engine's guard for its predecessor's upload, which drains the plug:
    the window is asserted before the first two."""
    t = tactic("EC6P3")
    S.Runner(dev, t).run([writer(0), writer(1, slen=1000, nsh=7),
                          writer(2, slen=1000, nsh=5)],
                         what="shard_write_batch x3", windows=2)


# ---- stream switch -----------------------------------------------------------

@pytest.mark.parametrize("target", ["other", "own"])
def test_set_stream_with_work_queued(dev, target):
    """Stream A: plug -> shard_write_batch.  gfrs_set_stream to stream B (or
    back to the context's own with NULL), then shard_write_batch with other
    ids and encode_idx there.  The scratch both writes share (ptr_buf, the
    pinned staging) must not be reused before A's work has read it: both
    image sets and the parity are exact."""
    t = tactic("EC6P3")
    r = S.Runner(dev, t)
    sa = r.stream
    w1, w2 = writer(0), writer(1, slen=1000)
    e = A.EncodeIdx(t, A.ref_stripes(t, 1, 4093, seed=5))
    r.warm([w1, w2, e])
    for s in (w1, w2, e):
        s.prepare(dev)
    ev = r.plug()
    r.issue([w1], ev, "A: plug -> shard_write")
    assert not ev.query(), "the stream was idle before gfrs_set_stream"
    r.use(torch.cuda.Stream(dev) if target == "other" else None)
    r.issue([w2, e], None)
    sa.synchronize()
    r.drain()
    for s in (w1, w2, e):
        s.check(r.enc)


# ---- the context's own stream, lanes off -------------------------------------

_SCRIPT = r"""
import os
import sys
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import torch
import _sequence as S
import test_gpu_sequences as T

dev = torch.device("cuda:0")
t = T.tactic("EC6P3")
assert os.environ["GFRS_LANES"] == "0"
for name, (f, cold) in T.named_followers(t).items():
    # pin=False: the context's own stream, which cannot be queried
    T.run_pair(S.Runner(dev, t, pin=False), T.writer(), f, cold,
               "own stream: shard_write -> " + name)
print("sequences OK")
"""


def test_own_stream_lanes_off():
    """The named sequence and its variants with GFRS_LANES=0 on the
    context's own stream: the single-stripe calls then use the context's
    scratch without a caller stream being pinned.  No window assertion."""
    env = dict(os.environ, GFRS_LANES="0")
    r = subprocess.run([sys.executable, "-c", _SCRIPT], env=env, cwd=_REPO,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "sequences OK" in r.stdout
