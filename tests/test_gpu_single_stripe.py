"""The single-stripe contract of include/gfrs.h: gfrs_encode, gfrs_verify,
gfrs_reconstruct (the ec.Encoder interface itself), gfrs_encode_idx and
gfrs_update_idx across tactics, forms and lengths.

Everything goes through the C ABI inside guarded arenas (tests/_arena.py):
every declared output is compared bit-exactly with the CPU oracle, every
other byte - guards, gaps, surviving shards, inputs - has to come back
unchanged.  There is no tolerance anywhere.

Lengths: the smallest that reach each branch of rs_apply_k with one stripe
(16-byte vector pieces, a per-byte tail, 4096-byte tiles, small shards packed
while padded * 2 <= 4096):
  1, 15        byte tail only (shortest, longest)
  16, 17       exactly one vector piece; one piece plus a tail byte
  2048, 2049   last packed shape; first unpacked shape
  4095, 4096   one tile with a 15-byte tail; one tile, exact
  4097         a second tile holding one tail byte
  8197         three tiles, ragged

Tactics: one per size of the last output group of a launch sequence (the
host splits the output rows of a plan into groups of 4):
  RS(15+1) 1 | RS(4+2) 2 | EC6P3 3 | EC12P4 4 | EC15P12 4+4+4 |
  LRC12P2L2 2, local stripe 8 = 7+1 | EC6P10L2 4+4+2, local stripe 9 |
  EC16P20L2 38 shards, local stripe 19
EC6P3 and LRC12P2L2 run every length, the others 17, 2048 and 4097, so each
group size meets a tail, the packed shape and a second tile in the encode,
the accumulate (gfrs_encode_idx / gfrs_update_idx) and the verify kernels.
"""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _arena as A  # noqa: E402
from _arena import L, oracle, vp  # noqa: E402

from cubefs_amd import codemode  # noqa: E402
from cubefs_amd.runtime import GfrsError  # noqa: E402

pytestmark = pytest.mark.gpu

TOO_FEW, SHARD_SIZE, NO_DATA, INVALID_SHARDS = -2, -3, -4, -6

LENGTHS = [1, 15, 16, 17, 2048, 2049, 4095, 4096, 4097, 8197]
CORE = [17, 2048, 4097]
TACTICS = {"RS15P1": CORE, "RS4P2": CORE, "EC6P3": LENGTHS, "EC12P4": CORE,
           "EC15P12": CORE, "LRC12P2L2": LENGTHS, "EC6P10L2": CORE,
           "EC16P20L2": CORE}
LRC = [n for n in TACTICS if "L" in n[2:]]
CASES = [(n, s) for n, lens in TACTICS.items() for s in lens]
LRC_CASES = [c for c in CASES if c[0] in LRC]
ERR_TACTICS = ["EC6P3", "LRC12P2L2"]
ERR_LEN = 4097


def case_ids(cases):
    return ["%s-%d" % c for c in cases]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def get_tactic(name):
    if name == "RS15P1":
        return A.tactic(15, 1)
    if name == "RS4P2":
        return A.tactic(4, 2)
    if name == "LRC12P2L2":
        return A.lrc_tactic()
    return codemode.get_tactic(name)


def stripe(name, slen):
    t = get_tactic(name)
    return t, A.ref_stripes(t, 1, slen, seed=21)


def setup(name, slen):
    t, ref = stripe(name, slen)
    return t, ref, A.encoder(t)


def flip_bytes(slen):
    """Byte 0, the last byte of the last full 16-byte piece (when there is
    one) and the last byte."""
    pos = [0, slen - 1]
    if slen >= 16:
        pos.append(slen // 16 * 16 - 1)
    return sorted(set(pos))


# ---- the oracle's own answer for what a step expects ---------------------------
# The steps take their expected bytes from the oracle-encoded stripe; these
# checks (cached, CPU only) make sure the oracle's Reconstruct of the same
# erasures returns exactly those bytes, so the expectation is the reference's.

@functools.lru_cache(maxsize=None)
def oracle_rebuilds(name, slen, bad, data_only):
    t, ref = stripe(name, slen)
    sh = [ref[0, i].copy() for i in range(t.total)]
    present = np.ones(t.total, np.uint8)
    for b in bad:
        present[b] = 0
        sh[b][:] = 0x5A
    if t.L:
        rc = oracle.lrc_reconstruct(t.N, t.M, t.L, t.AZCount, sh, present,
                                    data_only=bool(data_only))
    else:
        rc = oracle.rs_reconstruct(t.N, t.M, sh, present,
                                   data_only=bool(data_only))
    assert rc == 0, (name, bad, rc)
    for i in range(t.total):
        if i in bad and data_only and i >= t.N:
            assert (sh[i] == 0x5A).all(), (name, bad, i)   # left alone
        else:
            assert np.array_equal(sh[i], ref[0, i]), (name, bad, i)
    return True


@functools.lru_cache(maxsize=None)
def oracle_local_stripe(name, slen, az):
    """The members of AZ `az`, after checking that they form a plain
    RS(local_n + local_m) stripe for the oracle: rs_verify holds and
    rs_reconstruct rebuilds every single member."""
    t, ref = stripe(name, slen)
    members, ln, lm = t.local_stripe_in_az(az)
    assert len(members) == ln + lm == t.total // t.AZCount
    rows = [ref[0, i].copy() for i in members]
    assert oracle.rs_verify(ln, lm, [r.copy() for r in rows])
    for j in range(len(members)):
        loc = [r.copy() for r in rows]
        loc[j][:] = 0
        present = np.ones(len(members), np.uint8)
        present[j] = 0
        assert oracle.rs_reconstruct(ln, lm, loc, present) == 0
        assert np.array_equal(loc[j], rows[j]), (name, az, j)
    return tuple(members)


# ---- Encode ----------------------------------------------------------------------

@pytest.mark.parametrize("name,slen", CASES, ids=case_ids(CASES))
def test_encode(dev, name, slen):
    """Device pointer table at odd gaps, device contiguous (the ec.Buffer
    layout, which skips the pointer table) and host memory: the same
    parity, nothing else written."""
    t, ref, enc = setup(name, slen)
    what = "%s len %d" % (name, slen)
    tab = A.Encode(t, ref, what=what + " table").run(dev, enc)
    con = A.Encode(t, ref, gap=slen, what=what + " contiguous").run(dev, enc)
    got_tab, got_con = tab.a.read(), con.a.read()
    for i in range(t.N, t.total):
        x = got_tab[tab.a.off + tab.offs[i]:][:slen]
        y = got_con[con.a.off + con.offs[i]:][:slen]
        assert np.array_equal(x, y), (what, "contiguous != table", i)
    A.Encode(t, ref, host=True, what=what).run(dev, enc)


# ---- Verify ----------------------------------------------------------------------

def verify_shards(t):
    """A data shard, the first and the last global parity (the last one is
    in the last output group) and, for LRC, every local parity - which the
    global check passes and only the local one can catch."""
    return sorted({t.N // 2, t.N, t.N + t.M - 1} |
                  set(range(t.N + t.M, t.total)))


@pytest.mark.parametrize("name,slen", CASES, ids=case_ids(CASES))
def test_verify(dev, name, slen):
    t, ref, enc = setup(name, slen)
    what = "%s len %d" % (name, slen)
    for host in (False, True):
        A.Verify(t, ref, host, flip=False, what=what + " clean").run(dev, enc)
        for shard in verify_shards(t):
            for byte in flip_bytes(slen):
                A.Verify(t, ref, host, flip=True, shard=shard, byte=byte,
                         what="%s flip shard %d byte %d" %
                         (what, shard, byte)).run(dev, enc)


# ---- Reconstruct -----------------------------------------------------------------

def erasures(t):
    """Bad lists (unsorted on purpose): one data shard; m losses mixing data
    and parity; parities only; for LRC one local parity alone, a local
    parity with m global losses, both local parities."""
    n, m = t.N, t.M
    nd = max(1, m // 2)
    mixed = list(range(n - nd, n)) + list(range(n + m - (m - nd), n + m))
    pats = [[n // 2], mixed[::-1], list(range(n, n + m))[::-1]]
    if t.L:
        pats += [[n + m], [t.total - 1] + mixed,
                 list(range(n + m, t.total))]
    return pats


@pytest.mark.parametrize("name,slen", CASES, ids=case_ids(CASES))
def test_reconstruct(dev, name, slen):
    """Rebuilt shards equal the oracle's; data_only = 1 leaves every lost
    parity exactly as the caller left it; the host form copies back only
    what it rebuilt."""
    t, ref, enc = setup(name, slen)
    for bad in erasures(t):
        assert len([b for b in bad if b < t.N + t.M]) <= t.M
        for data_only in (0, 1):
            assert oracle_rebuilds(name, slen, tuple(bad), data_only)
            for host in (False, True):
                A.Reconstruct(t, ref, host, bad=bad, data_only=data_only,
                              what="%s len %d bad %s" % (name, slen, bad)
                              ).run(dev, enc)


# ---- LRC local form: one local stripe given on its own -----------------------------

@pytest.mark.parametrize("name,slen", LRC_CASES, ids=case_ids(LRC_CASES))
def test_local_form(dev, name, slen):
    """nshards == total / az_count (lrcencoder.go:93-99,147-152), every AZ,
    device and host: Verify clean and with a flip in a data member, a
    global-parity member and the local parity; Reconstruct of each single
    member, the local parity included; Reconstruct of nothing."""
    t, ref, enc = setup(name, slen)
    for az in range(t.AZCount):
        members = list(oracle_local_stripe(name, slen, az))
        nsh = len(members)
        first_gp = next(j for j, i in enumerate(members) if i >= t.N)
        assert members[nsh - 1] >= t.N + t.M
        for host in (False, True):
            what = "%s len %d az %d local form" % (name, slen, az)
            A.Verify(t, ref, host, flip=False, members=members,
                     what=what + " clean").run(dev, enc)
            for pos in (0, first_gp, nsh - 1):
                for byte in flip_bytes(slen):
                    A.Verify(t, ref, host, flip=True, shard=pos, byte=byte,
                             members=members,
                             what="%s flip member %d byte %d" %
                             (what, pos, byte)).run(dev, enc)
            for j in range(nsh):
                A.Reconstruct(t, ref, host, bad=[j], members=members,
                              what="%s lost member %d" % (what, j)
                              ).run(dev, enc)
            A.Reconstruct(t, ref, host, bad=[], members=members,
                          what=what + " nbad 0").run(dev, enc)


# ---- EncodeIdx / UpdateIdx ---------------------------------------------------------

@pytest.mark.parametrize("name,slen", CASES, ids=case_ids(CASES))
def test_encode_idx(dev, name, slen):
    """All data shards into zeroed parity give the oracle's global parity; a
    strict subset gives the oracle's encode with the others taken as zero.
    Local parities are no part of the call."""
    t, ref, enc = setup(name, slen)
    what = "%s len %d" % (name, slen)
    A.EncodeIdx(t, ref, what=what + " all").run(dev, enc)
    subset = list(range(t.N - 1, -1, -2))
    assert 0 < len(subset) < t.N
    A.EncodeIdx(t, ref, idxs=subset, what=what + " subset").run(dev, enc)


@pytest.mark.parametrize("name,slen", CASES, ids=case_ids(CASES))
def test_update_idx(dev, name, slen):
    """Shard 0 and shard n-1 replaced: the parity equals a fresh encode;
    a replacement with the same content leaves it unchanged."""
    t, ref, enc = setup(name, slen)
    what = "%s len %d" % (name, slen)
    for idx in (0, t.N - 1):
        A.UpdateIdx(t, ref, idx=idx, what="%s idx %d" % (what, idx)
                    ).run(dev, enc)
    A.UpdateIdx(t, ref, idx=t.N // 2, same=True,
                what=what + " same content").run(dev, enc)


# ---- error table -------------------------------------------------------------------
# Each refused call writes nothing: the arena is prepared as for the valid
# call (erased shards hold the random fill) and has to come back as it was.

def untouched(step, enc, what):
    A.sync(enc)
    step.a.check(step.a.expect(), what=what)


def wide_table(step):
    """The step's pointer table with one more (valid) entry, for calls that
    announce one shard too many."""
    idx = list(range(step.total)) + [step.total - 1]
    return step.table(idx)


def wrong_counts(t):
    counts = [t.total - 1, t.total + 1]
    if t.L:
        counts += [t.total // t.AZCount - 1, t.total // t.AZCount + 1]
    return counts


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("name", ERR_TACTICS)
def test_wrong_shard_count(dev, name, host):
    t, ref, enc = setup(name, ERR_LEN)
    for ns in (t.total - 1, t.total + 1):
        s = A.Encode(t, ref, host)
        s.prepare(dev)
        rc = L().gfrs_encode(enc._ctx, wide_table(s), ERR_LEN, ns, s.memloc)
        assert rc == INVALID_SHARDS, ("encode", ns, rc)
        untouched(s, enc, "encode nshards %d" % ns)
    for ns in wrong_counts(t):
        s = A.Verify(t, ref, host)
        s.prepare(dev)
        rc = L().gfrs_verify(enc._ctx, wide_table(s), ERR_LEN, ns, s.memloc,
                             ctypes.byref(s.okv))
        assert rc == INVALID_SHARDS, ("verify", ns, rc)
        assert s.okv.value == -1
        untouched(s, enc, "verify nshards %d" % ns)
        s = A.Reconstruct(t, ref, host, bad=[0])
        s.prepare(dev)
        rc = L().gfrs_reconstruct(enc._ctx, wide_table(s), ERR_LEN, ns,
                                  s.memloc, s.badv, 1, 0)
        assert rc == INVALID_SHARDS, ("reconstruct", ns, rc)
        untouched(s, enc, "reconstruct nshards %d" % ns)


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("name", ERR_TACTICS)
def test_zero_length(dev, name, host):
    """shard_len = 0 is ErrShardNoData (checkShards, reedsolomon.go:1314),
    for either memloc, before anything is staged or launched."""
    t, ref, enc = setup(name, ERR_LEN)
    s = A.Encode(t, ref, host)
    s.prepare(dev)
    assert L().gfrs_encode(enc._ctx, s.ptrs, 0, t.total, s.memloc) == NO_DATA
    untouched(s, enc, "encode len 0")
    s = A.Verify(t, ref, host)
    s.prepare(dev)
    assert L().gfrs_verify(enc._ctx, s.ptrs, 0, t.total, s.memloc,
                           ctypes.byref(s.okv)) == NO_DATA
    assert s.okv.value == -1
    untouched(s, enc, "verify len 0")
    s = A.Reconstruct(t, ref, host, bad=[0])
    s.prepare(dev)
    assert L().gfrs_reconstruct(enc._ctx, s.ptrs, 0, t.total, s.memloc,
                                s.badv, 1, 0) == NO_DATA
    untouched(s, enc, "reconstruct len 0")


def refused_reconstructs(t):
    """(bad list, members or None, data_only, code)."""
    n, m = t.N, t.M
    over = list(range(m + 1))
    rows = [([0, -1], None, 0, INVALID_SHARDS),
            ([t.total], None, 0, INVALID_SHARDS),
            (over, None, 0, TOO_FEW),
            (over, None, 1, TOO_FEW),
            # more data than parity can carry, split over data and parity
            (list(range(m)) + [n], None, 0, TOO_FEW)]
    if t.L:
        az0 = t.local_stripe_in_az(0)[0]
        rows += [(over + [n + m], None, 0, TOO_FEW),
                 ([t.total - 1] + over, None, 0, TOO_FEW),
                 ([0, 1], az0, 0, TOO_FEW),
                 ([len(az0) - 1, 2], az0, 0, TOO_FEW),
                 ([len(az0)], az0, 0, INVALID_SHARDS),
                 ([-1], az0, 0, INVALID_SHARDS)]
    return rows


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("name", ERR_TACTICS)
def test_reconstruct_refused(dev, name, host):
    t, ref, enc = setup(name, ERR_LEN)
    for bad, members, data_only, want in refused_reconstructs(t):
        what = "reconstruct bad %s members %s" % (bad, members)
        s = A.Reconstruct(t, ref, host, members=members, data_only=data_only,
                          bad=[b for b in bad if 0 <= b < len(members or
                                                             range(t.total))])
        s.prepare(dev)
        rc = L().gfrs_reconstruct(enc._ctx, s.ptrs, ERR_LEN, s.total,
                                  s.memloc, A.i32s(bad), len(bad), data_only)
        assert rc == want, (what, rc)
        untouched(s, enc, what)


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("name", ERR_TACTICS)
def test_data_only_with_parities_lost_is_ok(dev, name, host):
    """data_only = 1 with only parities lost: GFRS_OK, nothing written."""
    t, ref, enc = setup(name, ERR_LEN)
    s = A.Reconstruct(t, ref, host, bad=list(range(t.N, t.total)),
                      data_only=1)
    s.prepare(dev)
    s.issue(enc)
    assert s.rc == 0
    untouched(s, enc, "data_only, parities lost")


def idx_calls(enc, s, idx, parity, slen, nparity):
    """gfrs_encode_idx and gfrs_update_idx with the same arguments, on the
    arena of a prepared UpdateIdx step."""
    a = s.a
    old, new = vp(a.ptr + s.offs[0]), vp(a.ptr + s.offs[s.total])
    return (L().gfrs_encode_idx(enc._ctx, old, idx, parity, slen, nparity),
            L().gfrs_update_idx(enc._ctx, old, new, idx, parity, slen,
                                nparity))


@pytest.mark.parametrize("name", ERR_TACTICS)
def test_idx_calls_refused(dev, name):
    """The reference's order (reedsolomon.go:632-647): the parity count,
    then the index, then the length.  A refused gfrs_update_idx has run
    neither of its two passes."""
    t, ref, enc = setup(name, ERR_LEN)
    n, m = t.N, t.M
    s = A.UpdateIdx(t, ref, idx=0)
    s.prepare(dev)
    wide = s.table(range(n, n + m + 1))
    rows = [(0, wide, ERR_LEN, m + 1, TOO_FEW),
            (0, s.pptrs, ERR_LEN, m - 1, TOO_FEW),
            (-1, wide, ERR_LEN, m + 1, TOO_FEW),      # count before index
            (-1, s.pptrs, ERR_LEN, m, INVALID_SHARDS),
            (n, s.pptrs, ERR_LEN, m, INVALID_SHARDS),
            (n, s.pptrs, 0, m, INVALID_SHARDS),       # index before length
            (0, s.pptrs, 0, m, NO_DATA)]
    for idx, parity, slen, nparity, want in rows:
        got = idx_calls(enc, s, idx, parity, slen, nparity)
        assert got == (want, want), (idx, slen, nparity, got)
        untouched(s, enc, "idx %d len %d nparity %d" % (idx, slen, nparity))


def test_encode_idx_on_replicate_is_a_no_op(dev):
    """m = 0: nparity = 0 is GFRS_OK whatever idx is (reedsolomon.go:
    635-637), and there is no plan to run."""
    enc = A.encoder(codemode.get_tactic("Replica3"))
    gap = ERR_LEN + 3
    a = A.Arena(dev, 3 * gap, 1, seed=35)
    a.upload()
    old, new = vp(a.ptr), vp(a.ptr + gap)
    none = (ctypes.c_void_p * 1)()
    one = (ctypes.c_void_p * 1)(a.ptr + 2 * gap)
    f, g, ctx = L().gfrs_encode_idx, L().gfrs_update_idx, enc._ctx
    for idx in (0, 2, -1, 3, 1000):
        for slen in (ERR_LEN, 0):
            assert f(ctx, old, idx, none, slen, 0) == 0, (idx, slen)
            assert g(ctx, old, new, idx, none, slen, 0) == 0, (idx, slen)
    assert f(ctx, old, 0, one, ERR_LEN, 1) == TOO_FEW
    assert g(ctx, old, new, 0, one, ERR_LEN, 1) == TOO_FEW
    A.sync(enc)
    a.check(a.expect(), what="replicate encode_idx")


# ---- the Python wrapper ------------------------------------------------------------

def test_wrapper_checks_buffers(dev):
    """ec.Encoder.encode_idx / update_idx refuse a buffer of another length
    (ErrShardSize) or outside device memory before the C call: a parity one
    byte short would be written past its end."""
    t, ref, enc = setup("EC6P3", ERR_LEN)
    data = torch.from_numpy(ref[0, 0].copy()).to(dev)
    new = torch.from_numpy(ref[0, 1].copy()).to(dev)
    seen = []

    def parity(short=None):
        return [torch.full((ERR_LEN - (r == short),), 7, dtype=torch.uint8,
                           device=dev) for r in range(t.M)]

    def expect(code, call):
        with pytest.raises(GfrsError) as e:
            call()
        assert e.value.code == code, e.value

    for short in range(t.M):
        par = parity(short)
        seen.append(par)
        expect(SHARD_SIZE, lambda: enc.encode_idx(data, 0, par))
        expect(SHARD_SIZE, lambda: enc.update_idx(data, new, 0, par))
    par = parity()
    seen.append(par)
    expect(SHARD_SIZE, lambda: enc.update_idx(data, new[:-1], 0, par))
    expect(SHARD_SIZE, lambda: enc.encode_idx(data[:-1], 0, par))
    host_par = [np.zeros(ERR_LEN, np.uint8) for _ in range(t.M)]
    expect(INVALID_SHARDS, lambda: enc.update_idx(data, new, 0, host_par))
    expect(INVALID_SHARDS, lambda: enc.encode_idx(data, 0, host_par))
    expect(INVALID_SHARDS,
           lambda: enc.update_idx(data, new.cpu(), 0, parity()))
    torch.cuda.synchronize()
    for par in seen:                     # no GPU work: nothing was written
        for p in par:
            assert (p.cpu().numpy() == 7).all()
    assert all((h == 0).all() for h in host_par)
    # and the accepted call still runs
    par = [torch.zeros(ERR_LEN, dtype=torch.uint8, device=dev)
           for _ in range(t.M)]
    for i in range(t.N):
        enc.encode_idx(torch.from_numpy(ref[0, i].copy()).to(dev), i, par)
    for r in range(t.M):
        assert np.array_equal(par[r].cpu().numpy(), ref[0, t.N + r])
