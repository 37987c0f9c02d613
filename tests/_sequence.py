"""Back-to-back call sequences on one context (tests/test_gpu_sequences.py).

The engine is stateful: every call of a context shares one set of grow-only
scratch (pinned staging, pointer/id table, fail words, staging stripe, the
queue blobs, the plan caches), and the async batch calls return with their
work - and the uploads that feed it - still queued on the context's stream.
Device-side reuse of the scratch is ordered by the stream; the host's reuse
of the pinned staging is ordered only by the engine's own bookkeeping.  A
Runner issues the steps of tests/_arena.py in order on ONE fresh context
with nothing in between, synchronizes once, and only then checks every
step's arenas against the oracle: the result of step i must not depend on
what follows it.

Such a test is vacuous when the stream is idle while the follower's host
code runs, so the runner holds the stream busy and proves it:

  * the context is pinned (gfrs_set_stream) to a torch stream the runner
    owns, so that the test can see the stream's state;
  * a plug - PLUG_REPEAT async gfrs_encode_batch calls over a throwaway
    arena of PLUG_BYTES - is queued ahead of the first step, and a torch
    event is recorded behind it;
  * immediately before every step up to and including the first one that
    blocks, `not event.query()` is asserted: the plug, hence everything the
    earlier steps queued behind it, has not run yet.  A closed window fails
    the sequence.

First use of a plan (DevPlan::upload) and every growth of a scratch buffer
synchronize and would close the window, so every step runs once on the same
context - prepare, issue, check - before the measured pass.  Where the
growth is the subject, the growing step is left out of the warm-up
(`cold`); the window is then asserted before it like before any other.

Plug length, measured on an MI355X with measure() below (warm, idle
context, medians of 5):

  one plug repeat, gfrs_encode_batch over 288 MiB   0.068 ms RS(6+3)
                                                    0.099 ms RS(6+6)
  host wall clock of issuing producer + follower on the idle stream
    shard_write_batch -> encode_idx (x6)            0.241 ms RS(6+3)
                                                    0.333 ms RS(6+6)
    the slowest pair of the matrix tried,
    encode_frame_batch -> read queue                0.605 ms RS(6+3)

PLUG_REPEAT = 256 makes the plug 17.4 ms (25 ms for RS(6+6)): 72x the host
time of the named sequence and 28x that of the slowest pair, where 20x is
asked for so that scheduler jitter of the host thread cannot close the
window.

What the plug cannot do: a call that synchronizes drains it.  After a step
that blocks, and after a gfrs_shard_write_batch that had to wait for the
upload of an earlier one (the engine's own guard), the event behind the
plug has fired, so no window is asserted from there on (`windows`).
"""
import time

import torch

import _arena as A
from _arena import L, ok, vp

from cubefs_amd import ec

PLUG_SLEN = 1 << 20
PLUG_BYTES = 288 << 20          # 32 stripes of RS(6+3), 24 of RS(6+6)
PLUG_REPEAT_MS = 0.068          # measured, see the module docstring
ISSUE_HOST_MS = 0.605           # measured, the slowest pair
PLUG_REPEAT = 256
assert PLUG_REPEAT * PLUG_REPEAT_MS >= 20 * ISSUE_HOST_MS

_PLUG = {}


def _plug_buffer(dev):
    """The throwaway arena, one per process: its content does not matter
    and nothing ever reads it back."""
    if dev not in _PLUG:
        _PLUG[dev] = torch.empty(PLUG_BYTES, dtype=torch.uint8, device=dev)
        _PLUG[dev].random_(0, 256)
        torch.cuda.synchronize()
    return _PLUG[dev]


class WindowClosed(AssertionError):
    pass


class Runner:
    """One fresh context of tactic `t`.  pin=True: on a torch stream of the
    runner's own, windows asserted.  pin=False: on the context's own stream,
    which the test cannot query - no window assertion."""

    def __init__(self, dev, t, pin=True):
        self.dev, self.t = dev, t
        self.enc = ec.Encoder(t)    # not the cached one: own scratch
        self.stream = None
        self.warmed = {}
        self.buf = _plug_buffer(dev)
        self.ns = PLUG_BYTES // (t.total * PLUG_SLEN)
        if pin:
            self.use(torch.cuda.Stream(dev))
        self.plug(1)                # loads the kernel, outside any window
        self.drain()

    def use(self, stream):
        """gfrs_set_stream to a torch stream, or back to the context's own
        with None."""
        self.stream = stream
        ok(L().gfrs_set_stream(self.enc._ctx,
                               stream.cuda_stream if stream else None),
           "set_stream")

    def plug(self, repeat=None):
        """Queue the plug; returns the event behind it (None unpinned)."""
        ctx, base = self.enc._ctx, vp(self.buf.data_ptr())
        stride = self.t.total * PLUG_SLEN
        for _ in range(PLUG_REPEAT if repeat is None else repeat):
            rc = L().gfrs_encode_batch(ctx, base, PLUG_SLEN, stride, self.ns)
            if rc:
                ok(rc, "plug")
        if self.stream is None:
            return None
        ev = torch.cuda.Event()
        ev.record(self.stream)
        return ev

    def drain(self):
        A.sync(self.enc)
        torch.cuda.synchronize()

    def warm(self, steps):
        """Run each step alone, once per context: scratch only grows and
        plans stay cached."""
        for s in steps:
            if id(s) not in self.warmed:
                s.run(self.dev, self.enc)
                self.warmed[id(s)] = s

    def issue(self, steps, ev, what="", windows=None):
        """Issue in order, nothing in between; the window is asserted before
        every step until one that blocks has been issued, or before the
        first `windows` steps."""
        enc, is_open = self.enc, ev is not None
        for i, s in enumerate(steps):
            if windows is not None and i >= windows:
                is_open = False
            if is_open and ev.query():
                raise WindowClosed(
                    "%s: the stream was idle before step %d (%s): the plug "
                    "is too short for this sequence" % (what, i, s.what))
            s.issue(enc)
            is_open = is_open and not s.blocking

    def run(self, steps, cold=(), what="", windows=None):
        """prepare all, plug, issue all, sync once, check all."""
        self.warm([s for s in steps if s not in cold])
        for s in steps:
            s.prepare(self.dev)
        self.issue(steps, self.plug(), what, windows)
        self.drain()
        for s in steps:
            s.check(self.enc)


def measure(dev, t, make_steps, repeat=8, rounds=5):
    """(ms per plug repeat, host ms of issuing the steps on an idle stream),
    the medians of `rounds`.  Prints them; not a test."""
    r = Runner(dev, t)
    r.warm(make_steps())
    plug_ms, host_ms = [], []
    for _ in range(rounds):
        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        r.drain()
        e0.record(r.stream)
        r.plug(repeat)
        e1.record(r.stream)
        r.drain()
        plug_ms.append(e0.elapsed_time(e1) / repeat)
        steps = make_steps()
        for s in steps:
            s.prepare(dev)
        r.drain()
        t0 = time.perf_counter()
        for s in steps:
            s.issue(r.enc)
        host_ms.append((time.perf_counter() - t0) * 1e3)
        r.drain()
        for s in steps:
            s.check(r.enc)
    plug_ms.sort()
    host_ms.sort()
    out = plug_ms[rounds // 2], host_ms[rounds // 2]
    print("plug repeat %.3f ms (all %s); issue host %.3f ms (all %s)" % (
        out[0], ["%.3f" % x for x in plug_ms], out[1],
        ["%.3f" % x for x in host_ms]))
    return out
