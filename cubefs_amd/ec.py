"""cubefs_amd.ec — the blobstore/common/ec.Encoder surface over the gfrs
C ABI (include/gfrs.h).

Mirrors the ten-method Encoder interface (encoder.go:41-62) with the same
semantics: caller-owned equal-length shards, LRC layering handled inside,
sentinel errors surfaced as GfrsError.  Shards are 1-D uint8 torch tensors
(CUDA tensors run in-place on the GPU; CPU tensors/numpy arrays are staged
through pinned memory by the C library).

The compute path is hand-written HIP — torch supplies memory and streams
only.  If libgfrs.so is missing or no GPU is present, calls raise.
"""
import ctypes
import io

import numpy as np

from . import codemode, runtime
from .runtime import GfrsError, MEM_DEVICE, MEM_HOST, Tactic, check, lib


def _tactic_struct(t: codemode.Tactic) -> Tactic:
    return Tactic(t.N, t.M, t.L, t.AZCount, t.PutQuorum, t.GetQuorum,
                  t.MinShardSize)


def _shard_view(s):
    """Returns (pointer:int, nbytes:int, is_device:bool)."""
    if isinstance(s, np.ndarray):
        assert s.dtype == np.uint8 and s.flags["C_CONTIGUOUS"]
        return s.ctypes.data, s.nbytes, False
    # torch tensor
    assert s.dtype.itemsize == 1 and s.is_contiguous()
    return s.data_ptr(), s.numel() * s.element_size(), s.is_cuda


def buffer_sizes(t: codemode.Tactic, data_size: int):
    """ec.GetBufferSizes (buf.go:146-153)."""
    ts = _tactic_struct(t)
    ss, eds, es = (ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64())
    check(lib().gfrs_buffer_sizes(ctypes.byref(ts), data_size,
                                  ctypes.byref(ss), ctypes.byref(eds),
                                  ctypes.byref(es)), "buffer_sizes")
    return ss.value, eds.value, es.value


class Encoder:
    """ec.Encoder (encoder.go:41-62) on MI355X."""

    def __init__(self, tactic, device=-1, enable_verify=False):
        if isinstance(tactic, (str, int)):
            tactic = codemode.get_tactic(tactic)
        # Replicate tactics (M == 0) are valid per the reference
        # (codemode.Tactic.IsValid, encoder.go:78): Encode/Verify become
        # no-ops with zero parity and Reconstruct can only succeed when
        # nothing is missing — all handled by the C layer (m==0 paths).
        if not tactic.is_valid():
            raise GfrsError(-1, "invalid code mode for EC encoder")
        self.tactic = tactic
        self.enable_verify = enable_verify
        ts = _tactic_struct(tactic)
        self._ctx = lib().gfrs_create(ctypes.byref(ts), device)
        if not self._ctx:
            raise GfrsError(-100, lib().gfrs_last_error().decode())
        self._destroy = lib().gfrs_destroy

    def __del__(self):
        # interpreter shutdown can clear module globals before __del__
        # runs, so use the function handle captured at construction
        ctx = getattr(self, "_ctx", None)
        destroy = getattr(self, "_destroy", None)
        if ctx and destroy is not None:
            try:
                destroy(ctx)
            except TypeError:
                pass
            self._ctx = None

    # ---- helpers ----

    def _ptrs(self, shards, expect=None):
        expect = expect if expect is not None else self.tactic.total
        if len(shards) != expect:
            raise GfrsError(-6, "want %d shards, got %d" % (expect, len(shards)))
        views = [_shard_view(s) for s in shards]
        ln = views[0][1]
        dev = views[0][2]
        for p, n, d in views:
            if n != ln:
                raise GfrsError(-3, "unequal shard sizes")
            if d != dev:
                raise GfrsError(-6, "mixed host/device shards")
        arr = (ctypes.c_void_p * len(shards))(*[v[0] for v in views])
        return arr, ln, (MEM_DEVICE if dev else MEM_HOST)

    def _idx_ptrs(self, data_shard, others, parity):
        """Parity pointer table and shard length of an incremental-parity
        call.  These calls take device pointers only, and every buffer has
        the data shard's length (ErrShardSize, reedsolomon.go:641-647): a
        shorter parity would be written past its end."""
        views = [_shard_view(s) for s in (data_shard, *others, *parity)]
        ln = views[0][1]
        for p, n, d in views:
            if not d:
                raise GfrsError(-6, "incremental parity takes device shards")
        for p, n, d in views:
            if n != ln:
                raise GfrsError(-3, "unequal shard sizes")
        arr = (ctypes.c_void_p * len(parity))(
            *[v[0] for v in views[1 + len(others):]])
        return arr, ln

    # ---- the Encoder interface ----

    def encode(self, shards):
        """Encode (encoder.go:114, lrcencoder.go:35)."""
        arr, ln, loc = self._ptrs(shards)
        check(lib().gfrs_encode(self._ctx, arr, ln, len(shards), loc), "encode")
        if self.enable_verify and not self.verify(shards):
            raise GfrsError(-5, "verify after encode failed")

    def verify(self, shards):
        """Verify (encoder.go:133, lrcencoder.go:89).  Accepts a full set
        or, for LRC, one local stripe set."""
        t = self.tactic
        expect = len(shards) if (
            t.L > 0 and len(shards) == t.total // t.AZCount) else t.total
        arr, ln, loc = self._ptrs(shards, expect)
        ok = ctypes.c_int(0)
        check(lib().gfrs_verify(self._ctx, arr, ln, len(shards), loc,
                                ctypes.byref(ok)), "verify")
        return bool(ok.value)

    def reconstruct(self, shards, bad_idx):
        """Reconstruct (encoder.go:139, lrcencoder.go:133).  Accepts a full
        set or, for LRC, one local stripe set."""
        self._reconstruct(shards, bad_idx, data_only=0)

    def reconstruct_data(self, shards, bad_idx):
        """ReconstructData (encoder.go:146, lrcencoder.go:190)."""
        self._reconstruct(shards, bad_idx, data_only=1)

    def _reconstruct(self, shards, bad_idx, data_only):
        t = self.tactic
        expect = len(shards) if (
            t.L > 0 and len(shards) == t.total // t.AZCount) else t.total
        arr, ln, loc = self._ptrs(shards, expect)
        bad = (ctypes.c_int32 * max(1, len(bad_idx)))(*bad_idx)
        check(lib().gfrs_reconstruct(self._ctx, arr, ln, len(shards), loc,
                                     bad, len(bad_idx), data_only),
              "reconstruct")

    def split(self, data):
        """Split (reedsolomon.go:1574-1632 + lrcencoder.go:209-228): no-copy
        slicing into ceil(len/N) shards, zero-padded; parity/local shards
        allocated.  `data` is a 1-D uint8 tensor/array; returns a list of
        views over a (possibly re-allocated) contiguous buffer."""
        t = self.tactic
        n = int(data.shape[0]) if hasattr(data, "shape") else len(data)
        if n == 0:
            raise GfrsError(-7, "short data")
        per = (n + t.N - 1) // t.N
        total = per * t.total
        if isinstance(data, np.ndarray):
            buf = np.zeros(total, dtype=np.uint8)
            buf[:n] = data
        else:
            import torch
            buf = torch.zeros(total, dtype=torch.uint8, device=data.device)
            buf[:n] = data
        return [buf[i * per:(i + 1) * per] for i in range(t.total)]

    def get_data_shards(self, shards):
        return shards[:self.tactic.N]

    def get_parity_shards(self, shards):
        return shards[self.tactic.N:self.tactic.N + self.tactic.M]

    def get_local_shards(self, shards):
        if self.tactic.L == 0:
            return []
        return shards[self.tactic.N + self.tactic.M:]

    def get_shards_in_idc(self, shards, idx):
        """GetShardsInIdc (encoder.go:172-179 / lrcencoder.go:244-251)."""
        t = self.tactic
        if t.L > 0:
            locals_, _, _ = t.local_stripe_in_az(idx)
            return [shards[i] for i in locals_]
        n, m = t.N, t.M
        ln, lm = n // t.AZCount, m // t.AZCount
        return list(shards[idx * ln:(idx + 1) * ln]) + \
            list(shards[n + lm * idx:n + lm * (idx + 1)])

    def join(self, dst: io.RawIOBase, shards, out_size: int):
        """Join (reedsolomon.go:1646-1684): concatenates the data shards'
        first out_size bytes into dst."""
        t = self.tactic
        shards = shards[:t.N]
        have = sum(int(s.shape[0]) for s in shards)
        if have < out_size:
            raise GfrsError(-7, "short data")
        written = 0
        for s in shards:
            take = min(out_size - written, int(s.shape[0]))
            if take <= 0:
                break
            chunk = s[:take]
            if not isinstance(chunk, np.ndarray):
                chunk = chunk.cpu().numpy()
            dst.write(chunk.tobytes())
            written += take

    # ---- batched stripes (repair/migrate bulk path) ----
    # base: contiguous device tensor [nstripes, total, shard_len] uint8

    def _base(self, batch):
        assert batch.is_cuda and batch.is_contiguous()
        nstripes, total, ln = batch.shape
        assert total == self.tactic.total
        return batch.data_ptr(), ln, total * ln, nstripes

    def encode_batch(self, batch):
        p, ln, stride, ns = self._base(batch)
        check(lib().gfrs_encode_batch(self._ctx, p, ln, stride, ns),
              "encode_batch")

    def encode_frame_batch(self, framed, batch, block_len=65536):
        """Fused PUT pipeline: parity + crc32block framed images in one
        pass (stream_put.go:146 + datafile.go:342).  framed:
        [nstripes*(n+m), encode_size(shard_len)] device tensor."""
        p, ln, stride, ns = self._base(batch)
        check(lib().gfrs_encode_frame_batch(self._ctx, framed.data_ptr(),
                                            framed.stride(0), p, ln, stride,
                                            ns, block_len),
              "encode_frame_batch")

    def encode_frame_queue(self, framed, batch, jobs, block_len=65536):
        """Encode+frame queue: encode_frame_batch per job in one call (the
        PUT path over concurrent blobs of different sizes).  batch: flat
        uint8 device tensor holding every job; framed: flat uint8 device
        tensor for the images; jobs: [(off, shard_len, img_off,
        img_stride)], shard i of a job at byte off + i*shard_len of batch,
        the framed image of its shard j (all n+m+l of them) at byte
        img_off + j*img_stride of framed.  Blocks until the images are
        ready."""
        assert batch.is_cuda and batch.is_contiguous()
        assert framed.is_cuda and framed.is_contiguous()
        nj = len(jobs)
        ej = (runtime.EJob * max(1, nj))()
        for j, (off, ln, img_off, img_stride) in enumerate(jobs):
            ej[j] = runtime.EJob(off, ln, img_off, img_stride, 0)
        check(lib().gfrs_encode_frame_queue(self._ctx, framed.data_ptr(),
                                            batch.data_ptr(), ej, nj,
                                            block_len),
              "encode_frame_queue")

    def put_queue(self, disk_dst, batch, jobs, vuids, block_len=65536):
        """Put queue: encode every job straight into the n+m+l disk images
        blobnode writes - header, crc32block body, footer - in one call, for
        every tactic up to n = 32 (more than 4 parity rows run in row groups
        of 4).  batch: flat uint8 device tensor holding the data shards;
        disk_dst: flat uint8 device tensor for the images; jobs: [(off,
        shard_len, img_off, img_stride, bid, vol)], data shard i of a job at
        byte off + i*shard_len of batch, the disk image of its shard i at
        byte img_off + i*img_stride of disk_dst; vuids: [[n+m+l vuids]], one
        list per volume, a job's headers carrying vuids[vol].  Blocks until
        the images are ready and returns the CRC32-IEEE of every raw shard
        (the shard meta's Crc) as a numpy uint32 array of shape
        (njobs, n+m+l)."""
        assert batch.is_cuda and batch.is_contiguous()
        assert disk_dst.is_cuda and disk_dst.is_contiguous()
        nj, total = len(jobs), self.tactic.total
        pj = (runtime.PJob * max(1, nj))()
        for j, (off, ln, img_off, img_stride, bid, vol) in enumerate(jobs):
            pj[j] = runtime.PJob(off, ln, img_off, img_stride, bid, vol, 0)
        flat = [v for vol in vuids for v in vol]
        assert len(flat) == len(vuids) * total
        vu = (ctypes.c_uint64 * max(1, len(flat)))(*flat)
        crcs = np.zeros((max(1, nj), total), dtype=np.uint32)
        check(lib().gfrs_put_queue(
            self._ctx, disk_dst.data_ptr(), batch.data_ptr(), pj, nj, vu,
            len(vuids), block_len,
            crcs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))),
            "put_queue")
        return crcs[:nj]

    def verify_batch(self, batch):
        p, ln, stride, ns = self._base(batch)
        nwords = (ns + 63) // 64
        bm = (ctypes.c_uint64 * nwords)()
        check(lib().gfrs_verify_batch(self._ctx, p, ln, stride, ns, bm),
              "verify_batch")
        import numpy as np
        bmn = np.ctypeslib.as_array(bm)
        bits = np.unpackbits(bmn.view(np.uint8), bitorder="little")[:ns]
        return bits.astype(bool).tolist()

    def reconstruct_batch(self, batch, bad_idx, data_only=False):
        p, ln, stride, ns = self._base(batch)
        bad = (ctypes.c_int32 * max(1, len(bad_idx)))(*bad_idx)
        check(lib().gfrs_reconstruct_batch(self._ctx, p, ln, stride, ns, bad,
                                           len(bad_idx), int(data_only)),
              "reconstruct_batch")

    def encode_idx(self, data_shard, idx, parity):
        """EncodeIdx (reedsolomon.go:631): parity[r] ^= coeff[r][idx]*data.
        Parity must start zeroed; call once per data shard."""
        arr, ln = self._idx_ptrs(data_shard, (), parity)
        check(lib().gfrs_encode_idx(self._ctx, data_shard.data_ptr(), idx,
                                    arr, ln, len(parity)), "encode_idx")

    def update_idx(self, old_shard, new_shard, idx, parity):
        """Update (reedsolomon.go:676): patch parity for a replaced data
        shard: parity[r] ^= coeff[r][idx]*(old^new)."""
        arr, ln = self._idx_ptrs(old_shard, (new_shard,), parity)
        check(lib().gfrs_update_idx(self._ctx, old_shard.data_ptr(),
                                    new_shard.data_ptr(), idx, arr, ln,
                                    len(parity)), "update_idx")

    def reconstruct_verify_batch(self, batch, bad_idx):
        """Fused Reconstruct + mandatory Verify (worker_slice_recover.go:
        865-874) in one data pass.  Returns the per-stripe verify-fail
        list."""
        p, ln, stride, ns = self._base(batch)
        bad = (ctypes.c_int32 * max(1, len(bad_idx)))(*bad_idx)
        nwords = (ns + 63) // 64
        bm = (ctypes.c_uint64 * nwords)()
        check(lib().gfrs_reconstruct_verify_batch(self._ctx, p, ln, stride,
                                                  ns, bad, len(bad_idx), bm),
              "reconstruct_verify")
        import numpy as np
        bmn = np.ctypeslib.as_array(bm)
        bits = np.unpackbits(bmn.view(np.uint8), bitorder="little")[:ns]
        return bits.astype(bool).tolist()

    def reconstruct_verify_queue(self, batch, jobs, patterns):
        """Repair queue (worker_slice_recover.go:804-888, the loop over
        bids): every job has its own place, shard length and erasure
        pattern, and the whole queue is a bounded number of launches with
        one sync.  batch: flat uint8 device tensor holding every job;
        jobs: [(off, shard_len, pattern)], shard i of a job at byte
        off + i*shard_len of batch; patterns: [[bad shard indices]], an
        empty list meaning verify only.  Returns the per-job verify-fail
        list, in the caller's job order."""
        assert batch.is_cuda and batch.is_contiguous()
        nj = len(jobs)
        qj = (runtime.QJob * max(1, nj))()
        for j, (off, ln, pat) in enumerate(jobs):
            qj[j] = runtime.QJob(off, ln, pat, 0)
        flat = [i for p in patterns for i in p]
        offs = [0]
        for p in patterns:
            offs.append(offs[-1] + len(p))
        bad = (ctypes.c_int32 * max(1, len(flat)))(*flat)
        boff = (ctypes.c_int32 * len(offs))(*offs)
        bm = (ctypes.c_uint64 * max(1, (nj + 63) // 64))()
        check(lib().gfrs_reconstruct_verify_queue(self._ctx, batch.data_ptr(),
                                                  qj, nj, bad, boff,
                                                  len(patterns), bm),
              "reconstruct_verify_queue")
        bmn = np.ctypeslib.as_array(bm)
        bits = np.unpackbits(bmn.view(np.uint8), bitorder="little")[:nj]
        return bits.astype(bool).tolist()

    def repair_batch(self, batch, bad_idx, disk_dst, bids, vuids,
                     block_len=65536):
        """Fused repair tasklet (worker_slice_recover.go:804-888 +
        datafile.go:342): reconstruct bad shards, verify every stripe,
        frame each repaired shard into a pwrite-able disk image.
        disk_dst: [nstripes*len(bad_idx), disk_size] device tensor;
        bids/vuids: flat per (stripe, bad) row-major.
        Returns the per-stripe verify-fail list."""
        import numpy as np
        p, ln, stride, ns = self._base(batch)
        nb = len(bad_idx)
        bad = (ctypes.c_int32 * nb)(*bad_idx)
        # large batches: keep the id arrays and fail bitmap vectorized
        abn = np.ascontiguousarray(bids, dtype=np.uint64)
        avn = np.ascontiguousarray(vuids, dtype=np.uint64)
        ab = abn.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        av = avn.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        nwords = (ns + 63) // 64
        bmn = np.zeros(nwords, dtype=np.uint64)
        bm = bmn.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        check(lib().gfrs_repair_batch(self._ctx, p, ln, stride, ns, bad, nb,
                                      disk_dst.data_ptr(), disk_dst.stride(0),
                                      block_len, ab, av, bm), "repair_batch")
        bits = np.unpackbits(bmn.view(np.uint8), bitorder="little")[:ns]
        return bits.astype(bool).tolist()

    def repair_queue(self, batch, jobs, patterns, disk_dst, bids, vuids,
                     block_len=65536):
        """Repair-image queue: repair_batch per job in one call
        (worker_slice_recover.go:804-888, the loop over bids, with the disk
        images of datafile.go:342).  batch: flat uint8 device tensor holding
        every job; jobs: [(off, shard_len, pattern, img_off, img_stride)],
        shard i of a job at byte off + i*shard_len of batch, the image of
        the pattern's b-th bad shard at byte img_off + b*img_stride of
        disk_dst (flat uint8 device tensor); patterns: [[bad shard
        indices]], none empty; bids/vuids: one per image, job-major, in the
        pattern's own order.  Returns the per-job verify-fail list, in the
        caller's job order."""
        assert batch.is_cuda and batch.is_contiguous()
        assert disk_dst.is_cuda and disk_dst.is_contiguous()
        nj = len(jobs)
        rj = (runtime.RJob * max(1, nj))()
        for j, (off, ln, pat, img_off, img_stride) in enumerate(jobs):
            rj[j] = runtime.RJob(off, ln, img_off, img_stride, pat, 0)
        flat = [i for p in patterns for i in p]
        offs = [0]
        for p in patterns:
            offs.append(offs[-1] + len(p))
        bad = (ctypes.c_int32 * max(1, len(flat)))(*flat)
        boff = (ctypes.c_int32 * len(offs))(*offs)
        abn = np.ascontiguousarray(bids, dtype=np.uint64)
        avn = np.ascontiguousarray(vuids, dtype=np.uint64)
        ab = abn.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        av = avn.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        bm = (ctypes.c_uint64 * max(1, (nj + 63) // 64))()
        check(lib().gfrs_repair_queue(self._ctx, batch.data_ptr(), rj, nj,
                                      bad, boff, len(patterns),
                                      disk_dst.data_ptr(), block_len, ab, av,
                                      bm), "repair_queue")
        bmn = np.ctypeslib.as_array(bm)
        bits = np.unpackbits(bmn.view(np.uint8), bitorder="little")[:nj]
        return bits.astype(bool).tolist()

    def read_queue(self, out, framed, jobs, patterns, block_len=65536):
        """Read queue: the degraded GET (datafile.go:410-434 +
        stream_get.go:382-465) per job in one call - crc32block decode of
        the surviving shard images and ReconstructData of a segment, in one
        pass over the images.  framed: flat uint8 device tensor holding the
        images (what encode_frame_queue wrote); out: flat uint8 device
        tensor for the rows; jobs: [(img_off, img_stride, shard_len,
        seg_off, seg_len, out_off, out_stride, pattern)], the image of shard
        i at byte img_off + i*img_stride of framed, bytes [seg_off,
        seg_off+seg_len) of data shard i (i < n) at byte
        out_off + i*out_stride of out; patterns: [[bad shard indices]], an
        empty list meaning a plain verified read.  Returns the per-job words
        as a numpy uint32 array: bit i set when input shard i failed a frame
        CRC (the job's rows are then unspecified)."""
        assert out.is_cuda and out.is_contiguous()
        assert framed.is_cuda and framed.is_contiguous()
        nj = len(jobs)
        gj = (runtime.GJob * max(1, nj))()
        for j, job in enumerate(jobs):
            gj[j] = runtime.GJob(*job, 0)
        flat = [i for p in patterns for i in p]
        offs = [0]
        for p in patterns:
            offs.append(offs[-1] + len(p))
        bad = (ctypes.c_int32 * max(1, len(flat)))(*flat)
        boff = (ctypes.c_int32 * len(offs))(*offs)
        words = np.zeros(max(1, nj), dtype=np.uint32)
        check(lib().gfrs_read_queue(
            self._ctx, out.data_ptr(), framed.data_ptr(), gj, nj, bad, boff,
            len(patterns), block_len,
            words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))),
            "read_queue")
        return words[:nj]

    def synchronize(self):
        check(lib().gfrs_synchronize(self._ctx), "synchronize")

    def encode_matrix(self):
        t = self.tactic
        out = np.zeros(((t.N + t.M), t.N), dtype=np.uint8)
        check(lib().gfrs_encode_matrix(
            self._ctx, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))),
            "encode_matrix")
        return out


def new_encoder(cfg_codemode, device=-1, enable_verify=False):
    """ec.NewEncoder (encoder.go:78)."""
    return Encoder(cfg_codemode, device=device, enable_verify=enable_verify)
