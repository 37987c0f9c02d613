"""Coding plans checked without a GPU: gfrs_compute_plan runs the builders of
cubefs_amd/csrc/gfrs_plan.cpp - the same functions the engine calls before
it uploads a plan - and returns `in`, `out`, `rows`, `rowk`, `cmp_mask`
and `colpack`.

For every tactic of tests/_verdict.py and every erasure pattern of its
exhaustive() and subset() lists, once in ascending and once in descending
caller order, each plan kind that applies is
  - compared with the index lists the conventions prescribe (computed here
    in Python; gfrs_plan.h states them), and
  - applied in numpy, with the oracle's multiplication table, to the `in`
    shards of one oracle-encoded stripe of 64-byte shards: every row, write
    or compare, must give the original shard out[r].
The selftest at the end runs the builders under the address and
undefined-behaviour sanitizers as a stand-alone host program.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import _verdict as V

from cubefs_amd import runtime
from cubefs_amd.runtime import Tactic
from oracle import pyoracle

ENCODE, RS_RV, LRC_RV, REPAIR = 0, 1, 2, 3
TOO_FEW, INVALID_SHARDS, UNSUPPORTED = -2, -6, -103
SLEN = 64
CAP = 64

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compute_plan(t, kind, bad):
    """(rc, plan dict) from the export."""
    ct = Tactic(t.N, t.M, t.L, t.AZCount, t.PutQuorum, t.GetQuorum,
                t.MinShardSize)
    cin = (ctypes.c_int32 * CAP)()
    cout = (ctypes.c_int32 * CAP)()
    rows = np.zeros(CAP * t.N, dtype=np.uint8)
    nin, nout, rowk = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    cmp_mask, colpack = ctypes.c_uint32(), ctypes.c_uint32()
    cbad = (ctypes.c_int32 * max(len(bad), 1))(*bad)
    rc = runtime.lib().gfrs_compute_plan(
        ctypes.byref(ct), kind, cbad, len(bad), CAP, cin, ctypes.byref(nin),
        cout, ctypes.byref(nout),
        rows.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
        ctypes.byref(rowk), ctypes.byref(cmp_mask), ctypes.byref(colpack))
    if rc != 0:
        return rc, None
    k = rowk.value
    return 0, dict(inp=list(cin[:nin.value]), out=list(cout[:nout.value]),
                   rows=rows[:nout.value * k].reshape(nout.value, k).copy(),
                   rowk=k, cmp_mask=cmp_mask.value, colpack=colpack.value)


@pytest.fixture(scope="module")
def mul():
    return pyoracle.gf_tables()[766:766 + 65536].reshape(256, 256)


_STRIPES = {}


def stripe(t):
    """One oracle-encoded stripe (total, SLEN); read-only, shared."""
    key = (t.N, t.M, t.L, t.AZCount)
    if key not in _STRIPES:
        rng = np.random.default_rng(0x91A5 + 131 * t.N + t.M)
        sh = [rng.integers(0, 256, SLEN, dtype=np.uint8)
              for _ in range(t.N + t.M + t.L)]
        pyoracle.lrc_encode(t.N, t.M, t.L, t.AZCount, sh)
        arr = np.stack(sh)
        arr.setflags(write=False)
        _STRIPES[key] = arr
    return _STRIPES[key]


def check_rows(mul, t, plan, what):
    """rows x the `in` shards == the original shard of every output row."""
    st = stripe(t)
    src = st[plan["inp"][:plan["rowk"]]]                  # (k, SLEN)
    got = np.bitwise_xor.reduce(
        mul[plan["rows"][:, :, None], src[None, :, :]], axis=1)
    for r, sh in enumerate(plan["out"]):
        kind = "compare" if plan["cmp_mask"] >> r & 1 else "write"
        assert np.array_equal(got[r], st[sh]), (what, kind, r, sh)


# ---- the conventions, restated ------------------------------------------------

def inputs(t, bad):
    """First k present of the k+m global shards in index order, or None."""
    v = [i for i in range(t.N + t.M) if i not in bad][:t.N]
    return v if len(v) == t.N else None


def checks(t, bad, valid):
    """Surviving global parities that are not inputs, then surviving local
    parities, ascending."""
    return [p for p in range(t.N, t.N + t.M)
            if p not in bad and p not in valid] + \
           [q for q in range(t.N + t.M, t.N + t.M + t.L) if q not in bad]


def want_rs_rv(t, bad):
    valid = inputs(t, bad)
    if valid is None:
        return TOO_FEW, None
    miss = sorted(set(b for b in bad if b < t.N))
    out = miss + list(range(t.N, t.N + t.M))
    mask = sum(1 << (len(miss) + p - t.N)
               for p in range(t.N, t.N + t.M) if p not in bad)
    return 0, dict(inp=valid, out=out, cmp_mask=mask, colpack=0)


def want_lrc_rv(t, bad):
    if len(set(bad)) != len(bad):
        return INVALID_SHARDS, None
    valid = inputs(t, bad)
    if valid is None:
        return UNSUPPORTED, None
    out = list(bad) + checks(t, bad, valid)
    if len(out) > 32:
        return UNSUPPORTED, None
    mask = sum(1 << r for r in range(len(bad), len(out)))
    return 0, dict(inp=valid, out=out, cmp_mask=mask, colpack=0)


def want_repair(t, bad):
    total = t.N + t.M + t.L
    if len(set(bad)) != len(bad) or any(b < 0 or b >= total for b in bad):
        return INVALID_SHARDS, None
    valid = inputs(t, bad)
    if valid is None:
        return TOO_FEW, None
    sbad = sorted(bad)
    chk = checks(t, bad, valid)[:4 - len(bad)]
    out = sbad + chk
    mask = sum(1 << r for r in range(len(bad), len(out)))
    colpack = sum(list(bad).index(b) << (4 * r) for r, b in enumerate(sbad))
    return 0, dict(inp=valid + chk, out=out, cmp_mask=mask, colpack=colpack)


def kinds(t, bad):
    ks = [(LRC_RV, want_lrc_rv) if t.L else (RS_RV, want_rs_rv)]
    if 1 <= len(bad) <= 4:           # the fused kernel's row budget
        ks.append((REPAIR, want_repair))
    return ks


def patterns(name):
    """Every erasure set of exhaustive() and subset(), ascending then
    descending caller order."""
    sets = []
    for pats in V.exhaustive(name).values():
        sets += [tuple(sorted(p)) for p in pats]
    sets += [tuple(sorted(p)) for p in V.subset(name)]
    seen = []
    for s in dict.fromkeys(sets):
        seen.append(list(s))
        seen.append(list(s)[::-1])
    return seen


def check_plan(mul, t, kind, want, bad, what):
    rc, plan = compute_plan(t, kind, bad)
    wrc, w = want(t, bad)
    assert rc == wrc, (what, rc, wrc)
    if rc != 0:
        return None
    assert plan["rowk"] == t.N, what
    for f in ("inp", "out", "cmp_mask", "colpack"):
        assert plan[f] == w[f], (what, f, plan[f], w[f])
    check_rows(mul, t, plan, what)
    return plan


@pytest.mark.parametrize("name", V.TACTICS)
def test_plans_match_conventions_and_oracle(mul, name):
    t = V.get_tactic(name)
    nplans = nrefused = 0
    for bad in patterns(name):
        for kind, want in kinds(t, bad):
            plan = check_plan(mul, t, kind, want, bad,
                              "%s kind=%d bad=%s" % (name, kind, bad))
            nplans += plan is not None
            nrefused += plan is None
    # the sweep met decodable sets and the undecodable one
    assert nplans > 40 and nrefused >= 1, (nplans, nrefused)


@pytest.mark.parametrize("name", V.TACTICS)
def test_fused_encode_plan(mul, name):
    """All m global then all l local parities over the n data shards."""
    t = V.get_tactic(name)
    rc, plan = compute_plan(t, ENCODE, [])
    assert rc == 0
    assert plan["inp"] == list(range(t.N))
    assert plan["out"] == list(range(t.N, t.N + t.M + t.L))
    assert plan["rowk"] == t.N and plan["cmp_mask"] == 0
    check_rows(mul, t, plan, name + " encode")


def test_error_codes(mul):
    rs, lrc = V.get_tactic("EC6P3"), V.get_tactic("LRC12P2L2")
    for t, kind, bad, want in [
            (rs, RS_RV, [0, 1, 2, 3], TOO_FEW),
            (rs, RS_RV, [9], INVALID_SHARDS),
            (rs, RS_RV, [-1], INVALID_SHARDS),
            (rs, REPAIR, [0, 0], INVALID_SHARDS),
            (rs, REPAIR, [9], INVALID_SHARDS),
            (rs, REPAIR, [-1, 2], INVALID_SHARDS),
            (rs, REPAIR, [0, 1, 2, 3], TOO_FEW),
            (lrc, LRC_RV, [0, 0], INVALID_SHARDS),
            (lrc, LRC_RV, [16], INVALID_SHARDS),
            (lrc, LRC_RV, [0, 1, 2], UNSUPPORTED),      # globally undecodable
            (lrc, LRC_RV, [12, 13, 5], UNSUPPORTED),
            (lrc, REPAIR, [0, 1, 2], TOO_FEW),
            (lrc, REPAIR, [15, 15], INVALID_SHARDS)]:
        assert compute_plan(t, kind, bad)[0] == want, (kind, bad)
    # plain RS reconstruct+verify takes the bad list as a set
    one, two = compute_plan(rs, RS_RV, [0])[1], compute_plan(rs, RS_RV,
                                                             [0, 0])[1]
    assert one["out"] == two["out"] and one["inp"] == two["inp"]
    assert np.array_equal(one["rows"], two["rows"])
    assert one["cmp_mask"] == two["cmp_mask"]
    # a replicate tactic has no plans
    rep = V.codemode.get_tactic("Replica3")
    assert compute_plan(rep, RS_RV, [0])[0] == -1


def test_rs66_row_budget(mul):
    """RS(6+6): a fused-repair plan never exceeds the kernel's 4 rows (which
    is why the engine does not use it there: it would drop check rows),
    while the reconstruct+verify plan always carries all 6 parity rows."""
    t = V.get_tactic("EC6P6")
    for bad in patterns("EC6P6"):
        if 1 <= len(bad) <= 4:
            rc, plan = compute_plan(t, REPAIR, bad)
            assert rc == 0 and len(plan["out"]) <= 4, bad
            assert len(plan["inp"]) == t.N + len(plan["out"]) - len(bad)
        rc, plan = compute_plan(t, RS_RV, bad)
        if rc == 0:
            assert [o for o in plan["out"] if o >= t.N] == \
                list(range(t.N, t.N + t.M)), bad


# ---- the builders under the sanitizers, as a host program ------------------------

def _host_compiler():
    """A host C++ compiler that links the address + UB sanitizer runtimes."""
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


def test_plan_selftest_sanitized(tmp_path):
    """tests/plan_selftest.cpp + gfrs_plan.cpp + gfrs_gf.cpp, built with
    -fsanitize=address,undefined by a plain host compiler: every builder
    over every bad set of size <= 4 (out-of-range, duplicate and
    undecodable ones included), each plan checked by matrix identity."""
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host compiler with the sanitizer runtimes")
    csrc = os.path.join(_REPO, "cubefs_amd", "csrc")
    exe = str(tmp_path / "plan_selftest")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall",
                    "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all",
                    os.path.join(_REPO, "tests", "plan_selftest.cpp"),
                    os.path.join(csrc, "gfrs_plan.cpp"),
                    os.path.join(csrc, "gfrs_gf.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "plan selftest OK" in r.stdout
