"""Repair-queue probe: gfrs_reconstruct_verify_queue against what a caller
had before it, RS(12+4), wall time of the blocking calls.

 (a) uniform  512 jobs x 4 MiB, one pattern [1]: the queue vs ONE
     gfrs_reconstruct_verify_batch over the same buffer.
 (b) mixed    4096 jobs, lengths drawn from {64 KiB, 1 MiB, 4 MiB}, 8
     patterns: the queue vs a loop of single-job batch calls (nstripes = 1),
     the only gather-free alternative without the queue.
 (c) small    65536 jobs x 2 KiB, one pattern: the queue vs the same loop
     (what the missing small-job packing costs).

and gfrs_repair_queue (the same with the disk images) against
gfrs_repair_batch:

 (d) uniform  512 jobs x 4 MiB, one pattern [1]: the queue vs ONE
     gfrs_repair_batch over the same buffers, three interleaved medians of
     each - the batch call (an unchanged kernel) is the yardstick and its
     own spread between medians the noise floor.
 (e) mixed    the 4096-job queue of (b), [6] in place of the verify-only
     pattern: the queue vs a loop of single-job gfrs_repair_batch calls.

and gfrs_encode_frame_queue against gfrs_encode_frame_batch, RS(6+3)
(--only fpghi, p standing for f'):

 (f) uniform  1024 jobs x 8 MiB, the headline PUT shape: the queue vs ONE
     batch call, three interleaved medians of each.
 (f') the same with 64 KiB shards, whose trailing 4-byte frame the batch
     kernel folds into the preceding workgroup and the queue kernel does not.
 (g) mixed    4096 jobs of 64 KiB / 1 MiB / 4 MiB: the queue vs a loop of
     single-job batch calls, and vs one batch call per distinct size.
 (h) small    65536 jobs x 2 KiB: the queue vs ONE batch call, both on the
     wave-per-stripe kernel (the cost of the per-job operator setup).
 (i) 65536 jobs x 6 KiB: the batch call runs the wave kernel there, the
     queue the frame kernel.

and gfrs_read_queue, RS(12+4) (--only rs):

 (r) uniform  512 jobs x 4 MiB, pattern [1], the whole shard: the queue vs
     the composition a caller had before it - gfrs_crc32b_decode of the 12
     inputs of every job, then ONE gfrs_reconstruct_batch(data_only=1) - and
     vs the yardstick kernel, ONE gfrs_crc32b_decode of a single image of as
     many frames (the unchanged register-CRC decode kernel: read n framed,
     write n raw, the memory skeleton of the read kernel); three interleaved
     medians of queue and yardstick.
 (s) mixed    the 4096-job size mix of (b), 8 patterns, a quarter of the jobs
     with segments of 64 KiB or less: the queue vs a per-blob loop of the
     existing calls (12 decodes, reconstruct, slice copy).

and gfrs_shard_read_queue over disk images (--only uvw), three interleaved
medians of queue and yardstick each:

 (u) inspect  512 images x 4 MiB, all NO_OUT | FOOTER: the queue vs ONE
     gfrs_crc32b_verify_batch over the same bodies (the unchanged register-CRC
     verify kernel).
 (v) unframe  the same images, whole shard, storing: the queue vs ONE
     gfrs_crc32b_decode of a single image of as many frames, the yardstick of
     (r).
 (w) mixed    the 4096-job size mix of (b), half the jobs inspecting, a
     quarter reading the whole shard, a quarter a range of 64 KiB or less: the
     queue vs one gfrs_shard_parse_batch per distinct size, a sync each.

and gfrs_shard_write_queue (--only xyz), in the same form:

 (x) raw      512 raw shards x 4 MiB into 512 images: the queue vs ONE
     gfrs_shard_write_batch of the same shards (plus its sync).
 (y) compact  the same 512 images as SRC_IMAGE jobs into a new chunk: the
     queue vs the composition it replaces, gfrs_shard_read_queue (whole shard,
     storing, FOOTER) into a raw scratch buffer, then gfrs_shard_write_batch.
 (z) mixed    the 4096-job size mix of (b), half raw and half SRC_IMAGE: the
     queue vs one composition per distinct size (a write batch of the raw
     shards of that size; a read queue and a write batch of its images), a
     sync each.

and gfrs_put_queue (--only ABC), three interleaved medians of queue and
yardstick each, every yardstick built from the earlier entry points only:

 (A) RS(6+3)  1024 jobs x 8 MiB: the queue vs gfrs_encode_frame_queue, the
     same kernels without the 9216 head-wave items.
 (B) EC6P6 and EC15P12, 512 jobs x 4 MiB: the queue vs the only composition
     that yielded disk images before it - gfrs_encode_batch, then
     gfrs_shard_write_queue with one raw job per shard - and, beside it,
     gfrs_encode_frame_queue's slow path (no headers).
 (C) EC15P12, the 4096-job size mix of (b): the queue vs one such composition
     per distinct size.

(a) and (d) run on random data with encoded parity; the others on a zeroed buffer
(a valid stripe: zero parity), since the kernels' work does not depend on
the data.  One JSON line on stdout; --out also writes it to a file.
"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
from cubefs_amd import codemode, ec, runtime  # noqa: E402

KIB, MIB = 1 << 10, 1 << 20
PATTERNS = [[1], [], [0, 13], [2, 5, 11, 15], [12], [3, 7], [4, 14, 15], [9]]
# a repair has something to write: [6] stands in for the verify-only pattern
REPAIR_PATTERNS = [p or [6] for p in PATTERNS]


def timed(fn, reps):
    fn()                                    # warm-up: plans, buffers
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(out), 3),
            "min_ms": round(min(out), 3), "max_ms": round(max(out), 3),
            "reps": reps}


class Probe:
    def __init__(self):
        self.t = codemode.get_tactic("EC12P4")
        self.enc = ec.Encoder(self.t)
        self.L = runtime.lib()
        self.total = self.t.N + self.t.M

    def args(self, jobs, patterns):
        qj = (runtime.QJob * len(jobs))()
        for j, (off, ln, pat) in enumerate(jobs):
            qj[j] = runtime.QJob(off, ln, pat, 0)
        flat = [i for p in patterns for i in p] or [0]
        offs = [0]
        for p in patterns:
            offs.append(offs[-1] + len(p))
        self.bads = [((ctypes.c_int32 * max(1, len(p)))(*p), len(p))
                     for p in patterns]
        return (qj, len(jobs), (ctypes.c_int32 * len(flat))(*flat),
                (ctypes.c_int32 * len(offs))(*offs), len(patterns),
                (ctypes.c_uint64 * ((len(jobs) + 63) // 64))())

    def queue(self, buf, qargs):
        rc = self.L.gfrs_reconstruct_verify_queue(self.enc._ctx,
                                                  buf.data_ptr(), *qargs)
        assert rc == 0, rc
        assert not any(qargs[-1]), "verify failed"

    def loop(self, buf, jobs):
        bm = (ctypes.c_uint64 * 1)()
        base = buf.data_ptr()
        call = self.L.gfrs_reconstruct_verify_batch
        ctx = self.enc._ctx
        for off, ln, pat in jobs:
            bad, nbad = self.bads[pat]
            rc = call(ctx, base + off, ln, self.total * ln, 1, bad, nbad, bm)
            assert rc == 0 and bm[0] == 0, (rc, bm[0])

    def layout(self, lens, npat, seed=1):
        rng = random.Random(seed)
        jobs, off = [], 0
        for ln in lens:
            jobs.append((off, ln, rng.randrange(npat)))
            off += self.total * ln
        return jobs, off

    def uniform(self, njobs, slen, reps):
        jobs, nbytes = self.layout([slen] * njobs, 1)
        buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        for lo in range(0, nbytes, 1 << 30):
            part = buf[lo:lo + (1 << 30)]
            part.copy_(torch.randint(0, 256, (part.numel(),),
                                     dtype=torch.uint8, device="cuda"))
        stride = self.total * slen
        rc = self.L.gfrs_encode_batch(self.enc._ctx, buf.data_ptr(), slen,
                                      stride, njobs)
        assert rc == 0, rc
        self.enc.synchronize()
        qargs = self.args(jobs, PATTERNS[:1])
        bad, nbad = self.bads[0]
        bm = (ctypes.c_uint64 * ((njobs + 63) // 64))()

        def batch():
            rc = self.L.gfrs_reconstruct_verify_batch(
                self.enc._ctx, buf.data_ptr(), slen, stride, njobs, bad,
                nbad, bm)
            assert rc == 0 and not any(bm), rc

        # interleave the two so that drift hits both alike
        res = {"njobs": njobs, "shard_len": slen,
               "batch_1": timed(batch, reps),
               "queue_1": timed(lambda: self.queue(buf, qargs), reps),
               "batch_2": timed(batch, reps),
               "queue_2": timed(lambda: self.queue(buf, qargs), reps)}
        b = min(res["batch_1"]["median_ms"], res["batch_2"]["median_ms"])
        q = min(res["queue_1"]["median_ms"], res["queue_2"]["median_ms"])
        res["queue_over_batch"] = round(q / b, 4)
        res["moved_GB"] = round(njobs * slen * (self.t.N + 1) / 1e9, 3)
        return res

    def versus_loop(self, lens, npat, reps, loop_reps):
        jobs, nbytes = self.layout(lens, npat)
        buf = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        qargs = self.args(jobs, PATTERNS[:npat])
        res = {"njobs": len(jobs), "bytes": nbytes, "npat": npat,
               "queue": timed(lambda: self.queue(buf, qargs), reps),
               "loop": timed(lambda: self.loop(buf, jobs), loop_reps)}
        res["loop_over_queue"] = round(res["loop"]["median_ms"] /
                                       res["queue"]["median_ms"], 2)
        if len(set(lens)) == 1 and npat == 1:
            # a uniform queue is also one batch call, which packs sub-2 KiB
            # stripes into shared tiles: the price of the unpacked queue
            bad, nbad = self.bads[0]
            bm = (ctypes.c_uint64 * ((len(jobs) + 63) // 64))()

            def batch():
                rc = self.L.gfrs_reconstruct_verify_batch(
                    self.enc._ctx, buf.data_ptr(), lens[0],
                    self.total * lens[0], len(jobs), bad, nbad, bm)
                assert rc == 0 and not any(bm), rc

            res["batch"] = timed(batch, reps)
            res["queue_over_batch"] = round(res["queue"]["median_ms"] /
                                            res["batch"]["median_ms"], 2)
        return res


    # ---- gfrs_repair_queue (d, e): the same, with the disk images ----

    def image_layout(self, jobs, patterns):
        """Images back to back at the tight 4-aligned stride, job-major."""
        rjobs, at = [], 0
        for off, ln, pat in jobs:
            stride = (self.L.gfrs_shard_disk_size(ln, 65536) + 3) // 4 * 4
            rjobs.append((off, ln, pat, at, stride))
            at += stride * len(patterns[pat])
        return rjobs, at

    def rargs(self, rjobs, patterns):
        rj = (runtime.RJob * len(rjobs))()
        for j, (off, ln, pat, img_off, stride) in enumerate(rjobs):
            rj[j] = runtime.RJob(off, ln, img_off, stride, pat, 0)
        flat = [i for p in patterns for i in p]
        offs = [0]
        for p in patterns:
            offs.append(offs[-1] + len(p))
        nimg = sum(len(patterns[job[2]]) for job in rjobs)
        self.bads = [((ctypes.c_int32 * len(p))(*p), len(p))
                     for p in patterns]
        self.ids = ((ctypes.c_uint64 * nimg)(*range(1, nimg + 1)),
                    (ctypes.c_uint64 * nimg)(*range(7, nimg + 7)))
        return (rj, len(rjobs), (ctypes.c_int32 * len(flat))(*flat),
                (ctypes.c_int32 * len(offs))(*offs), len(patterns))

    def rqueue(self, buf, dst, rargs, njobs):
        bm = (ctypes.c_uint64 * ((njobs + 63) // 64))()
        rc = self.L.gfrs_repair_queue(self.enc._ctx, buf.data_ptr(), *rargs,
                                      dst.data_ptr(), 65536, self.ids[0],
                                      self.ids[1], bm)
        assert rc == 0 and not any(bm), rc

    def rloop(self, buf, dst, rjobs):
        bm = (ctypes.c_uint64 * 1)()
        base, out = buf.data_ptr(), dst.data_ptr()
        call = self.L.gfrs_repair_batch
        ctx = self.enc._ctx
        for off, ln, pat, img_off, stride in rjobs:
            bad, nbad = self.bads[pat]
            rc = call(ctx, base + off, ln, self.total * ln, 1, bad, nbad,
                      out + img_off, stride, 65536, self.ids[0], self.ids[1],
                      bm)
            assert rc == 0 and bm[0] == 0, (rc, bm[0])

    def repair_uniform(self, njobs, slen, reps):
        """(d): the queue vs ONE gfrs_repair_batch over the same buffers;
        three medians of each, interleaved, so that the batch call's own
        run-to-run spread is on record next to the difference."""
        jobs, nbytes = self.layout([slen] * njobs, 1)
        buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        for lo in range(0, nbytes, 1 << 30):
            part = buf[lo:lo + (1 << 30)]
            part.copy_(torch.randint(0, 256, (part.numel(),),
                                     dtype=torch.uint8, device="cuda"))
        stride = self.total * slen
        rc = self.L.gfrs_encode_batch(self.enc._ctx, buf.data_ptr(), slen,
                                      stride, njobs)
        assert rc == 0, rc
        self.enc.synchronize()
        rjobs, nimg_bytes = self.image_layout(jobs, PATTERNS[:1])
        dst = torch.empty(nimg_bytes, dtype=torch.uint8, device="cuda")
        rargs = self.rargs(rjobs, PATTERNS[:1])
        bad, nbad = self.bads[0]
        bm = (ctypes.c_uint64 * ((njobs + 63) // 64))()

        def batch():
            rc = self.L.gfrs_repair_batch(
                self.enc._ctx, buf.data_ptr(), slen, stride, njobs, bad,
                nbad, dst.data_ptr(), rjobs[0][4], 65536, self.ids[0],
                self.ids[1], bm)
            assert rc == 0 and not any(bm), rc

        res = {"njobs": njobs, "shard_len": slen}
        for i in (1, 2, 3):
            res["batch_%d" % i] = timed(batch, reps)
            res["queue_%d" % i] = timed(
                lambda: self.rqueue(buf, dst, rargs, njobs), reps)
        bs = [res["batch_%d" % i]["median_ms"] for i in (1, 2, 3)]
        qs = [res["queue_%d" % i]["median_ms"] for i in (1, 2, 3)]
        res["batch_medians_ms"], res["queue_medians_ms"] = bs, qs
        res["batch_spread"] = round(max(bs) / min(bs) - 1, 4)
        res["queue_over_batch"] = round(statistics.median(qs) /
                                        statistics.median(bs), 4)
        res["moved_GB"] = round(njobs * slen * (self.t.N + self.t.M) / 1e9, 3)
        return res

    def repair_versus_loop(self, lens, patterns, reps, loop_reps):
        """(e): the queue vs a loop of single-job gfrs_repair_batch calls."""
        jobs, nbytes = self.layout(lens, len(patterns))
        buf = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        rjobs, nimg_bytes = self.image_layout(jobs, patterns)
        dst = torch.empty(nimg_bytes, dtype=torch.uint8, device="cuda")
        rargs = self.rargs(rjobs, patterns)
        res = {"njobs": len(jobs), "bytes": nbytes, "image_bytes": nimg_bytes,
               "npat": len(patterns),
               "queue": timed(
                   lambda: self.rqueue(buf, dst, rargs, len(jobs)), reps),
               "loop": timed(lambda: self.rloop(buf, dst, rjobs), loop_reps)}
        res["loop_over_queue"] = round(res["loop"]["median_ms"] /
                                       res["queue"]["median_ms"], 2)
        return res


class EncodeProbe:
    """gfrs_encode_frame_queue against gfrs_encode_frame_batch, RS(6+3), on
    zeroed sources (the kernels' work does not depend on the data).  The
    batch call returns with its work queued, so every yardstick ends with
    gfrs_synchronize; the queue call blocks by itself."""

    def __init__(self):
        self.t = codemode.get_tactic("EC6P3")
        self.enc = ec.Encoder(self.t)
        self.L = runtime.lib()
        self.total = self.t.N + self.t.M

    def layout(self, lens):
        """ec.Buffer stripes back to back; images back to back at the tight
        4-aligned stride."""
        jobs, off, img = [], 0, 0
        for ln in lens:
            stride = (self.L.gfrs_crc32b_encode_size(ln, 65536) + 3) // 4 * 4
            jobs.append((off, ln, img, stride))
            off += self.total * ln
            img += self.total * stride
        return jobs, off, img

    def buffers(self, lens):
        jobs, nbytes, nimg = self.layout(lens)
        buf = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty(nimg, dtype=torch.uint8, device="cuda")
        ej = (runtime.EJob * len(jobs))()
        for j, (off, ln, img, stride) in enumerate(jobs):
            ej[j] = runtime.EJob(off, ln, img, stride, 0)
        return jobs, buf, dst, ej

    def queue(self, buf, dst, ej, njobs):
        rc = self.L.gfrs_encode_frame_queue(self.enc._ctx, dst.data_ptr(),
                                            buf.data_ptr(), ej, njobs, 65536)
        assert rc == 0, rc

    def batch(self, buf, dst, job, nstripes):
        off, ln, img, stride = job
        rc = self.L.gfrs_encode_frame_batch(
            self.enc._ctx, dst.data_ptr() + img, stride, buf.data_ptr() + off,
            ln, self.total * ln, nstripes, 65536)
        assert rc == 0, rc

    def uniform(self, njobs, slen, reps):
        """(f), (f'), (h), (i): the queue vs ONE gfrs_encode_frame_batch over
        the same buffers; three medians of each, interleaved, so that the
        batch call's own run-to-run spread is on record next to the
        difference."""
        jobs, buf, dst, ej = self.buffers([slen] * njobs)

        def batch():
            self.batch(buf, dst, jobs[0], njobs)
            self.enc.synchronize()

        res = {"njobs": njobs, "shard_len": slen}
        for i in (1, 2, 3):
            res["batch_%d" % i] = timed(batch, reps)
            res["queue_%d" % i] = timed(
                lambda: self.queue(buf, dst, ej, njobs), reps)
        bs = [res["batch_%d" % i]["median_ms"] for i in (1, 2, 3)]
        qs = [res["queue_%d" % i]["median_ms"] for i in (1, 2, 3)]
        res["batch_medians_ms"], res["queue_medians_ms"] = bs, qs
        res["batch_spread"] = round(max(bs) / min(bs) - 1, 4)
        res["queue_over_batch"] = round(statistics.median(qs) /
                                        statistics.median(bs), 4)
        res["moved_GB"] = round(njobs * slen * (self.t.N + self.total) / 1e9,
                                3)
        return res

    def mixed(self, lens, reps, loop_reps):
        """(g): the queue vs a loop of single-job batch calls, and vs one
        batch call per distinct size (what a size-sorting shim would issue:
        the same bytes, regrouped by size over the same buffers)."""
        jobs, buf, dst, ej = self.buffers(lens)

        def loop():
            for job in jobs:
                self.batch(buf, dst, job, 1)
            self.enc.synchronize()

        groups, off, img = [], 0, 0
        for ln in sorted(set(lens)):
            n = lens.count(ln)
            stride = (self.L.gfrs_crc32b_encode_size(ln, 65536) + 3) // 4 * 4
            groups.append(((off, ln, img, stride), n))
            off += n * self.total * ln
            img += n * self.total * stride

        def per_size():
            for job, n in groups:
                self.batch(buf, dst, job, n)
            self.enc.synchronize()

        res = {"njobs": len(jobs), "bytes": buf.numel(),
               "image_bytes": dst.numel(), "sizes": len(groups)}
        for i in (1, 2, 3):
            res["per_size_%d" % i] = timed(per_size, reps)
            res["queue_%d" % i] = timed(
                lambda: self.queue(buf, dst, ej, len(jobs)), reps)
        res["loop"] = timed(loop, loop_reps)
        ps = [res["per_size_%d" % i]["median_ms"] for i in (1, 2, 3)]
        qs = [res["queue_%d" % i]["median_ms"] for i in (1, 2, 3)]
        res["per_size_medians_ms"], res["queue_medians_ms"] = ps, qs
        res["per_size_spread"] = round(max(ps) / min(ps) - 1, 4)
        res["queue_over_per_size"] = round(statistics.median(qs) /
                                           statistics.median(ps), 4)
        res["loop_over_queue"] = round(res["loop"]["median_ms"] /
                                       statistics.median(qs), 2)
        return res


class ReadProbe:
    """gfrs_read_queue against the calls a caller had before it, RS(12+4), on
    zeroed shards (zero parity: a valid stripe; the kernels' work does not
    depend on the data).  Every image is the crc32block framing of a zero
    shard, built once per length by gfrs_crc32b_encode and copied."""

    def __init__(self):
        self.t = codemode.get_tactic("EC12P4")
        self.enc = ec.Encoder(self.t)
        self.L = runtime.lib()
        self.n, self.total = self.t.N, self.t.N + self.t.M

    def image(self, ln):
        size = self.L.gfrs_crc32b_encode_size(ln, 65536)
        raw = torch.zeros(ln, dtype=torch.uint8, device="cuda")
        img = torch.empty(size, dtype=torch.uint8, device="cuda")
        w = self.L.gfrs_crc32b_encode(self.enc._ctx, img.data_ptr(),
                                      raw.data_ptr(), ln, 65536)
        assert w == size, w
        return img

    def buffers(self, lens, segs, npat, seed=1):
        """jobs: (img_off, img_stride, ln, seg_off, seg_len, out_off,
        out_stride, pattern); images at the tight stride, rows at the tight
        4-aligned stride."""
        rng = random.Random(seed)
        jobs, img, out = [], 0, 0
        for ln, (so, sl) in zip(lens, segs):
            stride = self.L.gfrs_crc32b_encode_size(ln, 65536)
            ostride = (sl + 3) // 4 * 4
            jobs.append((img, stride, ln, so, sl, out, ostride,
                         rng.randrange(npat)))
            img += self.total * stride
            out += self.n * ostride
        framed = torch.empty(img, dtype=torch.uint8, device="cuda")
        images = {ln: self.image(ln) for ln in set(lens)}
        for job in jobs:
            framed[job[0]:job[0] + self.total * job[1]].view(
                self.total, job[1]).copy_(images[job[2]])
        dst = torch.empty(out, dtype=torch.uint8, device="cuda")
        gj = (runtime.GJob * len(jobs))()
        for j, job in enumerate(jobs):
            gj[j] = runtime.GJob(*job, 0)
        return jobs, framed, dst, gj

    def pattern_args(self, patterns):
        flat = [i for p in patterns for i in p] or [0]
        offs = [0]
        for p in patterns:
            offs.append(offs[-1] + len(p))
        self.bads = [((ctypes.c_int32 * max(1, len(p)))(*p), len(p))
                     for p in patterns]
        self.inputs = [[i for i in range(self.total) if i not in p][:self.n]
                       for p in patterns]
        return ((ctypes.c_int32 * len(flat))(*flat),
                (ctypes.c_int32 * len(offs))(*offs), len(patterns))

    def queue(self, framed, dst, gj, njobs, pargs):
        words = (ctypes.c_uint32 * njobs)()
        rc = self.L.gfrs_read_queue(self.enc._ctx, dst.data_ptr(),
                                    framed.data_ptr(), gj, njobs, *pargs,
                                    65536, words)
        assert rc == 0 and not any(words), rc

    def decode_inputs(self, framed, raw_ptr, job):
        img_off, stride, ln, _, _, _, _, pat = job
        size = self.L.gfrs_crc32b_encode_size(ln, 65536)
        for i in self.inputs[pat]:
            w = self.L.gfrs_crc32b_decode(
                self.enc._ctx, raw_ptr + i * ln,
                framed.data_ptr() + img_off + i * stride, size, 65536)
            assert w == ln, w

    def uniform(self, njobs, slen, reps, comp_reps):
        jobs, framed, dst, gj = self.buffers([slen] * njobs,
                                             [(0, slen)] * njobs, 1)
        pargs = self.pattern_args(PATTERNS[:1])
        bad, nbad = self.bads[0]
        raw = torch.empty(njobs * self.total * slen, dtype=torch.uint8,
                          device="cuda")

        def composition():
            for j, job in enumerate(jobs):
                self.decode_inputs(framed, raw.data_ptr() +
                                   j * self.total * slen, job)
            rc = self.L.gfrs_reconstruct_batch(
                self.enc._ctx, raw.data_ptr(), slen, self.total * slen, njobs,
                bad, nbad, 1)
            assert rc == 0, rc
            self.enc.synchronize()

        # the yardstick: ONE decode of one image of as many full frames as fit
        # the queue's own destination (the bytes the queue's inputs hold)
        nframes = njobs * self.n * slen // 65532
        yard = torch.empty(nframes * 65536, dtype=torch.uint8, device="cuda")
        yard.view(nframes, 65536).copy_(self.image(65532))

        def yardstick():
            w = self.L.gfrs_crc32b_decode(self.enc._ctx, dst.data_ptr(),
                                          yard.data_ptr(), yard.numel(), 65536)
            assert w == nframes * 65532, w

        res = {"njobs": njobs, "shard_len": slen}
        for i in (1, 2, 3):
            res["yardstick_%d" % i] = timed(yardstick, reps)
            res["queue_%d" % i] = timed(
                lambda: self.queue(framed, dst, gj, njobs, pargs), reps)
        res["composition"] = timed(composition, comp_reps)
        ys = [res["yardstick_%d" % i]["median_ms"] for i in (1, 2, 3)]
        qs = [res["queue_%d" % i]["median_ms"] for i in (1, 2, 3)]
        res["yardstick_medians_ms"], res["queue_medians_ms"] = ys, qs
        res["yardstick_spread"] = round(max(ys) / min(ys) - 1, 4)
        res["queue_over_yardstick"] = round(statistics.median(qs) /
                                            statistics.median(ys), 4)
        res["queue_over_composition"] = round(
            statistics.median(qs) / res["composition"]["median_ms"], 4)
        res["moved_GB"] = round(njobs * slen * 2 * self.n / 1e9, 3)
        for name in ("GFRS_RD_WAVES",):
            if name in os.environ:
                res[name] = os.environ[name]
        return res

    def mixed(self, lens, patterns, reps, loop_reps):
        rng = random.Random(11)
        segs = []
        for ln in lens:
            if rng.randrange(4) == 0:       # a ranged GET of <= 64 KiB
                sl = rng.choice([4 * KIB, 16 * KIB, 64 * KIB])
                segs.append((4 * rng.randrange((ln - sl) // 4 + 1), sl))
            else:
                segs.append((0, ln))
        jobs, framed, dst, gj = self.buffers(lens, segs, len(patterns), seed=1)
        pargs = self.pattern_args(patterns)
        raw = torch.empty(self.total * max(lens), dtype=torch.uint8,
                          device="cuda")

        def loop():
            for job in jobs:
                _, _, ln, so, sl, out_off, ostride, pat = job
                self.decode_inputs(framed, raw.data_ptr(), job)
                bad, nbad = self.bads[pat]
                rc = self.L.gfrs_reconstruct_batch(
                    self.enc._ctx, raw.data_ptr(), ln, self.total * ln, 1,
                    bad, nbad, 1)
                assert rc == 0, rc
                self.enc.synchronize()
                dst[out_off:out_off + self.n * ostride].view(
                    self.n, ostride)[:, :sl].copy_(
                        raw[:self.n * ln].view(self.n, ln)[:, so:so + sl])
            torch.cuda.synchronize()

        res = {"njobs": len(jobs), "image_bytes": framed.numel(),
               "out_bytes": dst.numel(), "npat": len(patterns),
               "ranged_jobs": sum(1 for s, ln in zip(segs, lens)
                                  if s[1] != ln),
               "queue": timed(
                   lambda: self.queue(framed, dst, gj, len(jobs), pargs),
                   reps),
               "loop": timed(loop, loop_reps)}
        res["loop_over_queue"] = round(res["loop"]["median_ms"] /
                                       res["queue"]["median_ms"], 2)
        return res


class ShardProbe:
    """gfrs_shard_read_queue against the parent's kernels, on disk images of
    zero shards written by gfrs_shard_write_batch (the kernels' work does not
    depend on the data).  The images of one size lie back to back at the tight
    4-aligned stride, sizes in ascending order, so that the same chunk also
    serves one gfrs_shard_parse_batch / gfrs_crc32b_verify_batch per size."""

    def __init__(self):
        self.enc = ec.Encoder(codemode.get_tactic("EC6P3"))
        self.L = runtime.lib()

    def chunk(self, lens):
        """-> (chunk tensor, {size: (first offset, stride, count)}, offsets in
        the order of lens)."""
        groups, at = {}, 0
        for ln in sorted(set(lens)):
            stride = (self.L.gfrs_shard_disk_size(ln, 65536) + 3) // 4 * 4
            groups[ln] = (at, stride, lens.count(ln))
            at += stride * lens.count(ln)
        chunk = torch.empty(at, dtype=torch.uint8, device="cuda")
        for ln, (first, stride, count) in groups.items():
            raw = torch.zeros(ln, dtype=torch.uint8, device="cuda")
            ids = (ctypes.c_uint64 * 1)(5), (ctypes.c_uint64 * 1)(9)
            rc = self.L.gfrs_shard_write_batch(
                self.enc._ctx, chunk.data_ptr() + first, stride,
                raw.data_ptr(), ln, ln, 65536, ids[0], ids[1], 1)
            assert rc == 0, rc
            self.enc.synchronize()
            rows = chunk[first:first + stride * count].view(count, stride)
            if count > 1:
                rows[1:].copy_(rows[0].clone().expand(count - 1, stride))
        seen, offs = {ln: 0 for ln in groups}, []
        for ln in lens:
            first, stride, _ = groups[ln]
            offs.append(first + stride * seen[ln])
            seen[ln] += 1
        torch.cuda.synchronize()
        return chunk, groups, offs

    def sjobs(self, specs):
        """specs: (img_off, size, from, to, out_off, flags)."""
        sj = (runtime.SJob * len(specs))()
        for j, (off, ln, frm, to, out, flags) in enumerate(specs):
            sj[j] = runtime.SJob(off, ln, 5, 9, frm, to, out, flags, 0)
        return sj, (runtime.SResult * len(specs))()

    def queue(self, out_ptr, chunk, sj, res, check=False):
        rc = self.L.gfrs_shard_read_queue(self.enc._ctx, out_ptr,
                                          chunk.data_ptr(), sj, len(sj),
                                          65536, res)
        assert rc == 0, rc
        if check:       # once, outside the timed calls: 4096 results in Python
            assert not any(r.status for r in res), "status"
            assert all(r.bad_block == -1 and r.size == j.size
                       for r, j in zip(res, sj)), "results"

    @staticmethod
    def three(res, yard, queue, reps):
        queue(check=True)
        for i in (1, 2, 3):
            res["yardstick_%d" % i] = timed(yard, reps)
            res["queue_%d" % i] = timed(queue, reps)
        ys = [res["yardstick_%d" % i]["median_ms"] for i in (1, 2, 3)]
        qs = [res["queue_%d" % i]["median_ms"] for i in (1, 2, 3)]
        res["yardstick_medians_ms"], res["queue_medians_ms"] = ys, qs
        res["yardstick_spread"] = round(max(ys) / min(ys) - 1, 4)
        res["queue_over_yardstick"] = round(statistics.median(qs) /
                                            statistics.median(ys), 4)
        if "GFRS_SRD_WAVES" in os.environ:
            res["GFRS_SRD_WAVES"] = os.environ["GFRS_SRD_WAVES"]
        return res

    def inspect(self, njobs, slen, reps):
        """(u): every image NO_OUT | FOOTER vs ONE gfrs_crc32b_verify_batch
        over the same bodies (the unchanged register-CRC verify kernel)."""
        chunk, groups, offs = self.chunk([slen] * njobs)
        first, stride, _ = groups[slen]
        sj, sres = self.sjobs([(off, slen, 0, slen, 0, 3) for off in offs])
        body = self.L.gfrs_crc32b_encode_size(slen, 65536)
        bad = (ctypes.c_int64 * njobs)()

        def yardstick():
            rc = self.L.gfrs_crc32b_verify_batch(
                self.enc._ctx, chunk.data_ptr() + first + 32, stride, body,
                65536, njobs, bad)
            assert rc == 0 and all(b == -1 for b in bad), rc

        res = {"njobs": njobs, "shard_len": slen,
               "moved_GB": round(njobs * body / 1e9, 3)}
        return self.three(res, yardstick,
                          lambda check=False: self.queue(None, chunk, sj, sres,
                                                         check), reps)

    def unframe(self, njobs, slen, reps):
        """(v): the same images, whole shard, storing, vs ONE
        gfrs_crc32b_decode of a single image of as many frames (the yardstick
        of (r))."""
        chunk, groups, offs = self.chunk([slen] * njobs)
        sj, sres = self.sjobs([(off, slen, 0, slen, j * slen, 0)
                               for j, off in enumerate(offs)])
        dst = torch.empty(njobs * slen, dtype=torch.uint8, device="cuda")
        nframes = njobs * slen // 65532
        yard = torch.empty(nframes * 65536, dtype=torch.uint8, device="cuda")
        first = groups[slen][0]
        yard.view(nframes, 65536).copy_(chunk[first + 32:first + 32 + 65536])

        def yardstick():
            w = self.L.gfrs_crc32b_decode(self.enc._ctx, dst.data_ptr(),
                                          yard.data_ptr(), yard.numel(), 65536)
            assert w == nframes * 65532, w

        res = {"njobs": njobs, "shard_len": slen,
               "moved_GB": round(njobs * slen * 2 / 1e9, 3)}
        return self.three(res, yardstick,
                          lambda check=False: self.queue(
                              dst.data_ptr(), chunk, sj, sres, check), reps)

    def mixed(self, lens, reps):
        """(w): half the jobs inspect (NO_OUT | FOOTER), a quarter read the
        whole shard, a quarter a range of 64 KiB or less, vs one
        gfrs_shard_parse_batch per distinct size (each with its sync), which
        answers the inspect half's question for every image and hands back no
        byte."""
        rng = random.Random(13)
        chunk, groups, offs = self.chunk(lens)
        specs, out = [], 0
        for off, ln in zip(offs, lens):
            kind = rng.randrange(4)
            if kind < 2:
                specs.append((off, ln, 0, ln, 0, 3))
                continue
            if kind == 2:
                frm, to = 0, ln
            else:
                sl = rng.choice([4 * KIB, 16 * KIB, 64 * KIB])
                frm = 4 * rng.randrange((ln - sl) // 4 + 1)
                to = frm + sl
            specs.append((off, ln, frm, to, out, 2 if kind == 2 else 0))
            out += (to - frm + 3) // 4 * 4
        sj, sres = self.sjobs(specs)
        dst = torch.empty(max(4, out), dtype=torch.uint8, device="cuda")
        meta = (ctypes.c_uint64 * (4 * len(lens)))()
        bad = (ctypes.c_int64 * len(lens))()

        def per_size():
            for ln, (first, stride, count) in groups.items():
                rc = self.L.gfrs_shard_parse_batch(
                    self.enc._ctx, chunk.data_ptr() + first, stride, ln,
                    65536, meta, bad, count)
                assert rc == 0 and meta[3] == 0, rc

        res = {"njobs": len(lens), "chunk_bytes": chunk.numel(),
               "out_bytes": dst.numel(), "sizes": len(groups),
               "inspect_jobs": sum(1 for s in specs if s[5] == 3),
               "ranged_jobs": sum(1 for s in specs if s[5] == 0)}
        return self.three(res, per_size,
                          lambda check=False: self.queue(
                              dst.data_ptr(), chunk, sj, sres, check), reps)


def shard_main(a, out):
    p = ShardProbe()
    if "u" in a.only:
        out["u_shard_inspect"] = p.inspect(512 // a.scale, 4 * MIB, reps=7)
        torch.cuda.empty_cache()
    if "v" in a.only:
        out["v_shard_unframe"] = p.unframe(512 // a.scale, 4 * MIB, reps=7)
        torch.cuda.empty_cache()
    if "w" in a.only:
        rng = random.Random(7)               # the lengths of (b)
        lens = [rng.choice([64 * KIB, MIB, 4 * MIB])
                for _ in range(4096 // a.scale)]
        out["w_shard_mixed"] = p.mixed(lens, reps=5)
        torch.cuda.empty_cache()


class ShardWriteProbe(ShardProbe):
    """gfrs_shard_write_queue against the parent's entry points.  Raw shards
    are zero bytes, source images those of ShardProbe.chunk (ids 5 and 9); the
    new images of one size lie back to back at the tight 4-aligned stride, so
    that the same destination serves one gfrs_shard_write_batch per size."""

    def wjobs(self, specs):
        """specs: (src_off, size, img_off, flags)."""
        wj = (runtime.WJob * len(specs))()
        for j, (src, ln, img, flags) in enumerate(specs):
            wj[j] = runtime.WJob(src, ln, 21 + j, 22, 5, 9, img, flags, 0)
        return wj, (runtime.SResult * len(specs))()

    def wqueue(self, dst, src, wj, res, check=False):
        rc = self.L.gfrs_shard_write_queue(self.enc._ctx, dst.data_ptr(),
                                           src.data_ptr(), wj, len(wj), 65536,
                                           res)
        assert rc == 0, rc
        if check:       # once, outside the timed calls
            assert not any(r.status for r in res), "status"
            assert all(r.bad_block == -1 and r.size == j.size
                       for r, j in zip(res, wj)), "results"
            assert len({r.crc for r, j in zip(res, wj)
                        if j.size == wj[0].size}) == 1, "crc"

    def write_batch(self, dst_ptr, stride, src_ptr, ln, count, ids):
        rc = self.L.gfrs_shard_write_batch(self.enc._ctx, dst_ptr, stride,
                                           src_ptr, ln, ln, 65536, ids[0],
                                           ids[1], count)
        assert rc == 0, rc

    @staticmethod
    def ids(n):
        return ((ctypes.c_uint64 * n)(*range(21, 21 + n)),
                (ctypes.c_uint64 * n)(*([22] * n)))

    def three(self, res, yard, queue, reps):
        res = ShardProbe.three(res, yard, queue, reps)
        if "GFRS_SWR_WAVES" in os.environ:
            res["GFRS_SWR_WAVES"] = os.environ["GFRS_SWR_WAVES"]
        return res

    def raw(self, njobs, slen, reps):
        """(x): raw shards vs ONE gfrs_shard_write_batch of the same shards."""
        stride = (self.L.gfrs_shard_disk_size(slen, 65536) + 3) // 4 * 4
        src = torch.zeros(njobs * slen, dtype=torch.uint8, device="cuda")
        dst = torch.empty(njobs * stride, dtype=torch.uint8, device="cuda")
        wj, wres = self.wjobs([(j * slen, slen, j * stride, 0)
                               for j in range(njobs)])
        ids = self.ids(njobs)

        def yardstick():
            self.write_batch(dst.data_ptr(), stride, src.data_ptr(), slen,
                             njobs, ids)
            self.enc.synchronize()

        res = {"njobs": njobs, "shard_len": slen,
               "moved_GB": round(njobs * (slen + stride) / 1e9, 3)}
        return self.three(res, yardstick,
                          lambda check=False: self.wqueue(dst, src, wj, wres,
                                                          check), reps)

    def compact(self, njobs, slen, reps):
        """(y): the images as SRC_IMAGE jobs vs gfrs_shard_read_queue (whole
        shard, storing, FOOTER) into a raw scratch buffer, then
        gfrs_shard_write_batch."""
        chunk, groups, offs = self.chunk([slen] * njobs)
        stride = groups[slen][1]
        dst = torch.empty(njobs * stride, dtype=torch.uint8, device="cuda")
        scratch = torch.empty(njobs * slen, dtype=torch.uint8, device="cuda")
        wj, wres = self.wjobs([(off, slen, j * stride, 1)
                               for j, off in enumerate(offs)])
        sj, sres = self.sjobs([(off, slen, 0, slen, j * slen, 2)
                               for j, off in enumerate(offs)])
        ids = self.ids(njobs)

        def yardstick():
            self.queue(scratch.data_ptr(), chunk, sj, sres)
            self.write_batch(dst.data_ptr(), stride, scratch.data_ptr(), slen,
                             njobs, ids)
            self.enc.synchronize()

        res = {"njobs": njobs, "shard_len": slen,
               "moved_GB": round(njobs * stride * 2 / 1e9, 3)}
        return self.three(res, yardstick,
                          lambda check=False: self.wqueue(dst, chunk, wj, wres,
                                                          check), reps)

    def mixed(self, lens, reps):
        """(z): half raw, half SRC_IMAGE, vs one composition per distinct
        size, each with its sync."""
        rng = random.Random(17)
        kinds = [rng.randrange(2) for _ in lens]
        img_lens = [ln for ln, k in zip(lens, kinds) if k]
        chunk, groups, offs = self.chunk(img_lens)
        # one source buffer: the images, then the raw shards per size
        raw_at, at = {}, chunk.numel()
        for ln in sorted(set(lens)):
            raw_at[ln] = at
            at += ln * sum(1 for x, k in zip(lens, kinds) if x == ln and not k)
        src = torch.zeros(at, dtype=torch.uint8, device="cuda")
        src[:chunk.numel()].copy_(chunk)
        del chunk
        # destination: per size, the raw jobs' images then the image jobs'
        dplace, at = {}, 0
        for ln in sorted(set(lens)):
            stride = (self.L.gfrs_shard_disk_size(ln, 65536) + 3) // 4 * 4
            nraw = sum(1 for x, k in zip(lens, kinds) if x == ln and not k)
            nimg = sum(1 for x, k in zip(lens, kinds) if x == ln and k)
            dplace[ln] = (at, stride, nraw, nimg)
            at += stride * (nraw + nimg)
        dst = torch.empty(at, dtype=torch.uint8, device="cuda")
        nscr = max(ln * d[3] for ln, d in dplace.items())
        scratch = torch.empty(max(4, nscr), dtype=torch.uint8, device="cuda")
        seen = {ln: [0, 0] for ln in dplace}
        specs, ioffs = [], iter(offs)
        for ln, k in zip(lens, kinds):
            first, stride, nraw, _ = dplace[ln]
            i = seen[ln][k]
            seen[ln][k] += 1
            if k:
                specs.append((next(ioffs), ln, first + stride * (nraw + i), 1))
            else:
                specs.append((raw_at[ln] + ln * i, ln, first + stride * i, 0))
        wj, wres = self.wjobs(specs)
        per = {}
        for ln, (first, stride, nraw, nimg) in dplace.items():
            g = groups.get(ln)
            sj = self.sjobs([(g[0] + g[1] * i, ln, 0, ln, i * ln, 2)
                             for i in range(nimg)]) if nimg else None
            per[ln] = (sj, self.ids(max(1, nraw)), self.ids(max(1, nimg)))

        def per_size():
            for ln, (first, stride, nraw, nimg) in dplace.items():
                sj, rid, iid = per[ln]
                if nraw:
                    self.write_batch(dst.data_ptr() + first, stride,
                                     src.data_ptr() + raw_at[ln], ln, nraw,
                                     rid)
                if nimg:
                    self.queue(scratch.data_ptr(), src, sj[0], sj[1])
                    self.write_batch(dst.data_ptr() + first + stride * nraw,
                                     stride, scratch.data_ptr(), ln, nimg, iid)
                self.enc.synchronize()

        res = {"njobs": len(lens), "src_bytes": src.numel(),
               "dst_bytes": dst.numel(), "sizes": len(dplace),
               "image_jobs": sum(kinds)}
        return self.three(res, per_size,
                          lambda check=False: self.wqueue(dst, src, wj, wres,
                                                          check), reps)


class PutProbe:
    """gfrs_put_queue against the calls that were there before it, on zeroed
    sources.  Every yardstick ends with gfrs_synchronize (or is a blocking
    queue call) and runs the earlier entry points only."""

    def __init__(self, name):
        self.t = codemode.get_tactic(name)
        self.enc = ec.Encoder(self.t)
        self.L = runtime.lib()
        self.total = self.t.N + self.t.M + self.t.L
        self.vuids = (ctypes.c_uint64 * self.total)(*range(100, 100 + self.total))

    def layout(self, lens):
        """ec.Buffer stripes back to back (the yardsticks encode in place;
        the put queue reads the n data shards of each); disk images back to
        back at the tight 4-aligned stride."""
        jobs, off, img = [], 0, 0
        for ln in lens:
            stride = (self.L.gfrs_shard_disk_size(ln, 65536) + 3) // 4 * 4
            jobs.append((off, ln, img, stride))
            off += self.total * ln
            img += self.total * stride
        return jobs, off, img

    def put(self, buf, dst, pj, crcs):
        rc = self.L.gfrs_put_queue(self.enc._ctx, dst.data_ptr(),
                                   buf.data_ptr(), pj, len(pj), self.vuids, 1,
                                   65536, crcs)
        assert rc == 0, rc

    def encode_queue(self, buf, dst, ej):
        rc = self.L.gfrs_encode_frame_queue(self.enc._ctx, dst.data_ptr(),
                                            buf.data_ptr(), ej, len(ej), 65536)
        assert rc == 0, rc

    def wjobs(self, groups):
        """One raw gfrs_wjob per shard of every stripe.  groups: ((off, ln,
        img, stride), nstripes), stripes and images back to back."""
        specs = []
        for (off, ln, img, stride), n in groups:
            for s in range(n):
                for i in range(self.total):
                    specs.append((off + (s * self.total + i) * ln, ln,
                                  img + (s * self.total + i) * stride, s))
        wj = (runtime.WJob * len(specs))()
        for k, (src, ln, im, bid) in enumerate(specs):
            wj[k] = runtime.WJob(src, ln, bid, 100 + k % self.total, 0, 0, im,
                                 0, 0)
        return wj, (runtime.SResult * len(specs))()

    def composition(self, buf, dst, groups, wj, wres):
        """gfrs_encode_batch per size, then ONE gfrs_shard_write_queue."""
        for (off, ln, _, _), n in groups:
            rc = self.L.gfrs_encode_batch(self.enc._ctx, buf.data_ptr() + off,
                                          ln, self.total * ln, n)
            assert rc == 0, rc
        rc = self.L.gfrs_shard_write_queue(self.enc._ctx, dst.data_ptr(),
                                           buf.data_ptr(), wj, len(wj), 65536,
                                           wres)
        assert rc == 0, rc
        self.enc.synchronize()

    def run(self, lens, reps, narrow):
        """narrow: the yardstick is gfrs_encode_frame_queue (same kernels, no
        header, footer or crc).  Otherwise: one composition per distinct size
        (gfrs_encode_batch, then gfrs_shard_write_queue with one raw job per
        shard - the only way to the disk images before this call), and beside
        it gfrs_encode_frame_queue's slow path, which yields no headers."""
        jobs, nbytes, nimg = self.layout(lens)
        buf = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty(nimg, dtype=torch.uint8, device="cuda")
        pj = (runtime.PJob * len(jobs))()
        ej = (runtime.EJob * len(jobs))()
        for j, (off, ln, img, stride) in enumerate(jobs):
            pj[j] = runtime.PJob(off, ln, img, stride, j, 0, 0)
            ej[j] = runtime.EJob(off, ln, img, stride, 0)
        crcs = (ctypes.c_uint32 * (len(jobs) * self.total))()
        res = {"tactic": "%d+%d+%d" % (self.t.N, self.t.M, self.t.L),
               "njobs": len(jobs), "sizes": len(set(lens)),
               "data_GB": round(sum(lens) * self.t.N / 1e9, 3),
               "image_GB": round(nimg / 1e9, 3)}
        queue = lambda: self.put(buf, dst, pj, crcs)        # noqa: E731
        if narrow:
            yard = lambda: self.encode_queue(buf, dst, ej)  # noqa: E731
        else:
            # regrouped by size over the same buffers: the same bytes
            groups, off, img = [], 0, 0
            for ln in sorted(set(lens)):
                n = lens.count(ln)
                stride = (self.L.gfrs_shard_disk_size(ln, 65536) + 3) // 4 * 4
                groups.append(((off, ln, img, stride), n))
                off += n * self.total * ln
                img += n * self.total * stride
            wj, wres = self.wjobs(groups)
            yard = lambda: self.composition(buf, dst, groups, wj,  # noqa: E731
                                            wres)
        for i in (1, 2, 3):
            res["yardstick_%d" % i] = timed(yard, reps)
            res["queue_%d" % i] = timed(queue, reps)
        ys = [res["yardstick_%d" % i]["median_ms"] for i in (1, 2, 3)]
        qs = [res["queue_%d" % i]["median_ms"] for i in (1, 2, 3)]
        res["yardstick_medians_ms"], res["queue_medians_ms"] = ys, qs
        res["yardstick_spread"] = round(max(ys) / min(ys) - 1, 4)
        res["queue_spread"] = round(max(qs) / min(qs) - 1, 4)
        res["queue_over_yardstick"] = round(statistics.median(qs) /
                                            statistics.median(ys), 4)
        if not narrow:
            res["encode_queue_slow_path"] = timed(
                lambda: self.encode_queue(buf, dst, ej), 2)
        return res


def put_main(a, out):
    if "A" in a.only:
        out["A_put_rs63"] = PutProbe("EC6P3").run(
            [8 * MIB] * (1024 // a.scale), reps=7, narrow=True)
        torch.cuda.empty_cache()
    if "B" in a.only:
        for name in ("EC6P6", "EC15P12"):
            out["B_put_" + name] = PutProbe(name).run(
                [4 * MIB] * (512 // a.scale), reps=7, narrow=False)
            torch.cuda.empty_cache()
    if "C" in a.only:
        rng = random.Random(7)               # the lengths of (b)
        lens = [rng.choice([64 * KIB, MIB, 4 * MIB])
                for _ in range(4096 // a.scale)]
        out["C_put_mixed_EC15P12"] = PutProbe("EC15P12").run(
            lens, reps=5, narrow=False)
        torch.cuda.empty_cache()


def shard_write_main(a, out):
    p = ShardWriteProbe()
    if "x" in a.only:
        out["x_shard_write_raw"] = p.raw(512 // a.scale, 4 * MIB, reps=7)
        torch.cuda.empty_cache()
    if "y" in a.only:
        out["y_shard_compact"] = p.compact(512 // a.scale, 4 * MIB, reps=7)
        torch.cuda.empty_cache()
    if "z" in a.only:
        rng = random.Random(7)               # the lengths of (b)
        lens = [rng.choice([64 * KIB, MIB, 4 * MIB])
                for _ in range(4096 // a.scale)]
        out["z_shard_write_mixed"] = p.mixed(lens, reps=7)
        torch.cuda.empty_cache()


def read_main(a, out):
    p = ReadProbe()
    out["read_tactic"] = "EC12P4"
    if "r" in a.only:
        out["r_read_uniform"] = p.uniform(512 // a.scale, 4 * MIB, reps=7,
                                          comp_reps=2)
        torch.cuda.empty_cache()
    if "s" in a.only:
        rng = random.Random(7)               # the lengths of (b)
        lens = [rng.choice([64 * KIB, MIB, 4 * MIB])
                for _ in range(4096 // a.scale)]
        out["s_read_mixed"] = p.mixed(lens, PATTERNS, reps=5, loop_reps=1)
        torch.cuda.empty_cache()


def encode_main(a, out):
    p = EncodeProbe()
    out["encode_tactic"] = "EC6P3"
    if "f" in a.only:
        out["f_encode_uniform"] = p.uniform(1024 // a.scale, 8 * MIB, reps=7)
        torch.cuda.empty_cache()
    if "p" in a.only:                        # (f') in the documents
        out["f2_encode_uniform_64k"] = p.uniform(1024 // a.scale, 64 * KIB,
                                                 reps=7)
        torch.cuda.empty_cache()
    if "g" in a.only:
        rng = random.Random(7)
        lens = [rng.choice([64 * KIB, MIB, 4 * MIB])
                for _ in range(4096 // a.scale)]
        out["g_encode_mixed"] = p.mixed(lens, reps=5, loop_reps=3)
        torch.cuda.empty_cache()
    if "h" in a.only:
        out["h_encode_small"] = p.uniform(65536 // a.scale, 2 * KIB, reps=7)
        torch.cuda.empty_cache()
    if "i" in a.only:
        out["i_encode_6k"] = p.uniform(65536 // a.scale, 6 * KIB, reps=7)
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--scale", type=int, default=1,
                    help="divide every job count by this (dry runs)")
    ap.add_argument("--only", default="abcde",
                    help="which configurations to run, e.g. 'ac'; the "
                    "encode+frame queue's are 'fpghi' (p = f'), the read "
                    "queue's 'rs', the shard read queue's 'uvw', the shard "
                    "write queue's 'xyz', the put queue's 'ABC'")
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "scale": a.scale}
    if set(a.only) & set("fpghi"):
        encode_main(a, out)
    if set(a.only) & set("rs"):
        read_main(a, out)
    if set(a.only) & set("uvw"):
        shard_main(a, out)
    if set(a.only) & set("xyz"):
        shard_write_main(a, out)
    if set(a.only) & set("ABC"):
        put_main(a, out)
    if not set(a.only) & set("abcde"):
        line = json.dumps(out)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    p = Probe()
    out["tactic"] = "EC12P4"
    for name in ("GFRS_RS_SEQ", "GFRS_RS_GRID"):
        if name in os.environ:
            out[name] = os.environ[name]
    if "a" in a.only:
        out["a_uniform"] = p.uniform(512 // a.scale, 4 * MIB, reps=7)
        torch.cuda.empty_cache()
    if "b" in a.only:
        rng = random.Random(7)
        lens = [rng.choice([64 * KIB, MIB, 4 * MIB])
                for _ in range(4096 // a.scale)]
        out["b_mixed"] = p.versus_loop(lens, 8, reps=5, loop_reps=3)
        torch.cuda.empty_cache()
    if "c" in a.only:
        out["c_small"] = p.versus_loop([2 * KIB] * (65536 // a.scale), 1,
                                       reps=5, loop_reps=2)
        torch.cuda.empty_cache()
    if "d" in a.only:
        out["d_repair_uniform"] = p.repair_uniform(512 // a.scale, 4 * MIB,
                                                   reps=7)
        torch.cuda.empty_cache()
    if "e" in a.only:
        rng = random.Random(7)               # the lengths and patterns of (b)
        lens = [rng.choice([64 * KIB, MIB, 4 * MIB])
                for _ in range(4096 // a.scale)]
        out["e_repair_mixed"] = p.repair_versus_loop(lens, REPAIR_PATTERNS,
                                                     reps=5, loop_reps=3)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
