"""cubefs_amd.runtime — ctypes binding of the product C ABI (include/gfrs.h).

Loads cubefs_amd/libgfrs.so (the hand-written HIP/CDNA4 engine).  There is
deliberately NO CPU fallback: if the library is missing or no GPU is
visible, compute calls raise.  PyTorch is used only for device memory and
streams (plumbing, not the compute path).
"""
import ctypes
import os

_DIR = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_DIR, "libgfrs.so")

MEM_DEVICE = 0
MEM_HOST = 1

ERRORS = {
    -1: "ErrInvalidCodeMode",
    -2: "ErrTooFewShards",
    -3: "ErrShardSize",
    -4: "ErrShardNoData",
    -5: "ErrVerify",
    -6: "ErrInvalidShards",
    -7: "ErrShortData",
    -8: "ErrSingular",
    -9: "ErrMismatchedCrc",
    -10: "ErrInvalidBlock",
    -11: "ErrReadOnClosed",
    -100: "ErrHIP",
    -101: "ErrNoGPU",
    -102: "ErrNoMem",
    -103: "ErrUnsupported",
}


class GfrsError(RuntimeError):
    def __init__(self, code, detail=""):
        self.code = code
        name = ERRORS.get(code, "Err%d" % code)
        super().__init__("%s%s" % (name, (": " + detail) if detail else ""))


class Tactic(ctypes.Structure):
    _fields_ = [
        ("n", ctypes.c_int32),
        ("m", ctypes.c_int32),
        ("l", ctypes.c_int32),
        ("az_count", ctypes.c_int32),
        ("put_quorum", ctypes.c_int32),
        ("get_quorum", ctypes.c_int32),
        ("min_shard_size", ctypes.c_int32),
    ]


class QJob(ctypes.Structure):
    """gfrs_qjob: one job of a repair queue."""
    _fields_ = [
        ("off", ctypes.c_uint64),
        ("shard_len", ctypes.c_uint64),
        ("pattern", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class QItem(ctypes.Structure):
    """gfrs_qitem: one (job, step) work item of a queue schedule."""
    _fields_ = [
        ("off", ctypes.c_uint64),
        ("shard_len", ctypes.c_uint64),
        ("job", ctypes.c_int32),
        ("pattern", ctypes.c_int32),
        ("row_off", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class QBucket(ctypes.Structure):
    """gfrs_qbucket: one launch of a queue schedule."""
    _fields_ = [
        ("g", ctypes.c_int32),
        ("gm", ctypes.c_int32),
        ("first", ctypes.c_int32),
        ("count", ctypes.c_int32),
    ]


class RJob(ctypes.Structure):
    """gfrs_rjob: one job of a repair-image queue."""
    _fields_ = [
        ("off", ctypes.c_uint64),
        ("shard_len", ctypes.c_uint64),
        ("img_off", ctypes.c_uint64),
        ("img_stride", ctypes.c_uint64),
        ("pattern", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class RItem(ctypes.Structure):
    """gfrs_ritem: one work item of a repair-image schedule."""
    _fields_ = [
        ("off", ctypes.c_uint64),
        ("shard_len", ctypes.c_uint64),
        ("img", ctypes.c_uint64),
        ("img_stride", ctypes.c_uint64),
        ("job", ctypes.c_int32),
        ("desc", ctypes.c_int32),
    ]


class RBucket(ctypes.Structure):
    """gfrs_rbucket: one frame launch of a repair-image schedule."""
    _fields_ = [
        ("gm", ctypes.c_int32),
        ("first", ctypes.c_int32),
        ("count", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class RImage(ctypes.Structure):
    """gfrs_rimage: one entry of a repair-image schedule's image table."""
    _fields_ = [
        ("off", ctypes.c_uint64),
        ("size", ctypes.c_uint64),
        ("bid", ctypes.c_uint64),
        ("vuid", ctypes.c_uint64),
    ]


class EJob(ctypes.Structure):
    """gfrs_ejob: one job of an encode+frame queue."""
    _fields_ = [
        ("off", ctypes.c_uint64),
        ("shard_len", ctypes.c_uint64),
        ("img_off", ctypes.c_uint64),
        ("img_stride", ctypes.c_uint64),
        ("reserved", ctypes.c_uint64),
    ]


class EItem(ctypes.Structure):
    """gfrs_eitem: one work item of an encode+frame schedule."""
    _fields_ = [
        ("off", ctypes.c_uint64),
        ("shard_len", ctypes.c_uint64),
        ("img", ctypes.c_uint64),
        ("img_stride", ctypes.c_uint64),
        ("job", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class EBucket(ctypes.Structure):
    """gfrs_ebucket: one launch of an encode+frame schedule."""
    _fields_ = [
        ("kind", ctypes.c_int32),
        ("param", ctypes.c_int32),
        ("first", ctypes.c_int32),
        ("count", ctypes.c_int32),
    ]


class GJob(ctypes.Structure):
    """gfrs_gjob: one job of a read queue."""
    _fields_ = [
        ("img_off", ctypes.c_uint64),
        ("img_stride", ctypes.c_uint64),
        ("shard_len", ctypes.c_uint64),
        ("seg_off", ctypes.c_uint64),
        ("seg_len", ctypes.c_uint64),
        ("out_off", ctypes.c_uint64),
        ("out_stride", ctypes.c_uint64),
        ("pattern", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class GItem(ctypes.Structure):
    """gfrs_gitem: one work item of a read schedule."""
    _fields_ = [
        ("img", ctypes.c_uint64),
        ("img_stride", ctypes.c_uint64),
        ("shard_len", ctypes.c_uint64),
        ("seg_off", ctypes.c_uint64),
        ("seg_len", ctypes.c_uint64),
        ("out", ctypes.c_uint64),
        ("out_stride", ctypes.c_uint64),
        ("job", ctypes.c_int32),
        ("desc", ctypes.c_int32),
    ]


class GBucket(ctypes.Structure):
    """gfrs_gbucket: one launch of a read schedule."""
    _fields_ = [
        ("r", ctypes.c_int32),
        ("first", ctypes.c_int32),
        ("count", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


SJOB_NO_OUT, SJOB_FOOTER = 1, 2
SHARD_HDR_MAGIC, SHARD_HDR_CRC, SHARD_HDR_MISMATCH = 1, 2, 4
SHARD_BODY_CRC, SHARD_FTR_MAGIC, SHARD_FTR_CRC = 8, 16, 32


class SJob(ctypes.Structure):
    """gfrs_sjob: one job of a shard read queue."""
    _fields_ = [
        ("img_off", ctypes.c_uint64),
        ("size", ctypes.c_uint64),
        ("bid", ctypes.c_uint64),
        ("vuid", ctypes.c_uint64),
        ("from_", ctypes.c_uint64),
        ("to", ctypes.c_uint64),
        ("out_off", ctypes.c_uint64),
        ("flags", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]


class SResult(ctypes.Structure):
    """gfrs_sresult: what one job of a shard read queue gets back."""
    _fields_ = [
        ("status", ctypes.c_uint32),
        ("crc", ctypes.c_uint32),
        ("bad_block", ctypes.c_int64),
        ("bid", ctypes.c_uint64),
        ("vuid", ctypes.c_uint64),
        ("size", ctypes.c_uint64),
    ]


class SItem(ctypes.Structure):
    """gfrs_sitem: one work item of a shard-read schedule."""
    _fields_ = [
        ("img", ctypes.c_uint64),
        ("size", ctypes.c_uint64),
        ("from_", ctypes.c_uint64),
        ("to", ctypes.c_uint64),
        ("out", ctypes.c_uint64),
        ("job", ctypes.c_int32),
        ("flags", ctypes.c_uint32),
    ]


class SBucket(ctypes.Structure):
    """gfrs_sbucket: one frame launch of a shard-read schedule."""
    _fields_ = [
        ("no_out", ctypes.c_int32),
        ("first", ctypes.c_int32),
        ("count", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


WJOB_SRC_IMAGE = 1


class WJob(ctypes.Structure):
    """gfrs_wjob: one job of a shard write queue."""
    _fields_ = [
        ("src_off", ctypes.c_uint64),
        ("size", ctypes.c_uint64),
        ("bid", ctypes.c_uint64),
        ("vuid", ctypes.c_uint64),
        ("src_bid", ctypes.c_uint64),
        ("src_vuid", ctypes.c_uint64),
        ("img_off", ctypes.c_uint64),
        ("flags", ctypes.c_uint32),
        ("reserved", ctypes.c_uint32),
    ]


class WItem(ctypes.Structure):
    """gfrs_witem: one work item of a shard-write schedule."""
    _fields_ = [
        ("src", ctypes.c_uint64),
        ("size", ctypes.c_uint64),
        ("img", ctypes.c_uint64),
        ("job", ctypes.c_int32),
        ("flags", ctypes.c_uint32),
    ]


class WBucket(ctypes.Structure):
    """gfrs_wbucket: one frame launch of a shard-write schedule."""
    _fields_ = [
        ("src_image", ctypes.c_int32),
        ("first", ctypes.c_int32),
        ("count", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


class PJob(ctypes.Structure):
    """gfrs_pjob: one job of a put queue."""
    _fields_ = [
        ("off", ctypes.c_uint64),
        ("shard_len", ctypes.c_uint64),
        ("img_off", ctypes.c_uint64),
        ("img_stride", ctypes.c_uint64),
        ("bid", ctypes.c_uint64),
        ("vol", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
    ]


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise ImportError(
                "cubefs_amd/libgfrs.so not built — run `make -C cubefs_amd` "
                "(or __graft_entry__.build()).  The gfrs engine has no CPU "
                "fallback by design.")
        # torch's wheel bundles its own ROCm runtime (unversioned
        # libamdhip64.so / libhsa-runtime64.so sonames), while libgfrs
        # links /opt/rocm's libamdhip64.so.7 — two HSA stacks coexist in
        # the process and only the "torch's stack initializes first"
        # order works (the second stack to init still enumerates the
        # device; the other order leaves gfrs with hipGetDeviceCount==0).
        # Enforce that order here so it doesn't depend on the caller's
        # import sequence.
        try:
            import torch
            if torch.cuda.is_available():
                torch.cuda.init()
        except ImportError:
            pass  # pure-ctypes consumers (no torch) manage init order
        L = ctypes.CDLL(_LIB_PATH)
        vp, vpp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)
        i32p = ctypes.POINTER(ctypes.c_int32)
        i64, i64p = ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)
        u64p = ctypes.POINTER(ctypes.c_uint64)

        L.gfrs_last_error.restype = ctypes.c_char_p
        L.gfrs_version.restype = ctypes.c_char_p
        L.gfrs_create.restype = vp
        L.gfrs_create.argtypes = [ctypes.POINTER(Tactic), ctypes.c_int]
        L.gfrs_destroy.argtypes = [vp]
        L.gfrs_set_stream.argtypes = [vp, vp]
        L.gfrs_synchronize.argtypes = [vp]
        L.gfrs_encode.argtypes = [vp, vpp, ctypes.c_size_t, ctypes.c_int, ctypes.c_int]
        L.gfrs_verify.argtypes = [vp, vpp, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                                  ctypes.POINTER(ctypes.c_int)]
        L.gfrs_reconstruct.argtypes = [vp, vpp, ctypes.c_size_t, ctypes.c_int,
                                       ctypes.c_int, i32p, ctypes.c_int, ctypes.c_int]
        L.gfrs_encode_batch.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int]
        L.gfrs_verify_batch.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_size_t,
                                        ctypes.c_int, u64p]
        L.gfrs_reconstruct_batch.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_size_t,
                                             ctypes.c_int, i32p, ctypes.c_int, ctypes.c_int]
        L.gfrs_crc32_host.restype = ctypes.c_uint32
        L.gfrs_crc32_host.argtypes = [ctypes.c_uint32, vp, i64]
        L.gfrs_crc32b_encode_size.restype = i64
        L.gfrs_crc32b_encode_size.argtypes = [i64, i64]
        L.gfrs_crc32b_decode_size.restype = i64
        L.gfrs_crc32b_decode_size.argtypes = [i64, i64]
        L.gfrs_crc32b_encode.restype = i64
        L.gfrs_crc32b_encode.argtypes = [vp, vp, vp, i64, i64]
        L.gfrs_crc32b_verify.argtypes = [vp, vp, i64, i64, i64p]
        L.gfrs_crc32b_decode.restype = i64
        L.gfrs_crc32b_decode.argtypes = [vp, vp, vp, i64, i64]
        L.gfrs_crc32b_encode_batch.argtypes = [vp, vp, ctypes.c_size_t, vp,
                                               ctypes.c_size_t, i64, i64, ctypes.c_int]
        L.gfrs_crc32b_verify_batch.argtypes = [vp, vp, ctypes.c_size_t, i64, i64,
                                               ctypes.c_int, i64p]
        L.gfrs_buffer_sizes.argtypes = [ctypes.POINTER(Tactic), i64, i64p, i64p, i64p]
        L.gfrs_sized_encode_size.argtypes = [i64, i64, i64p, i64p]
        L.gfrs_sized_decode_size.restype = i64
        L.gfrs_sized_decode_size.argtypes = [i64, i64, i64]
        L.gfrs_sized_encode.restype = i64
        L.gfrs_sized_encode.argtypes = [vp, vp, vp, i64, i64]
        L.gfrs_sized_verify.argtypes = [vp, vp, i64, i64, i64, i64p]
        L.gfrs_sized_decode.restype = i64
        L.gfrs_sized_decode.argtypes = [vp, vp, vp, i64, i64, i64]
        L.gfrs_shard_disk_size.restype = i64
        L.gfrs_shard_disk_size.argtypes = [i64, i64]
        L.gfrs_shard_write_batch.argtypes = [vp, vp, ctypes.c_size_t, vp,
                                             ctypes.c_size_t, i64, i64, u64p,
                                             u64p, ctypes.c_int]
        L.gfrs_shard_parse_batch.argtypes = [vp, vp, ctypes.c_size_t, i64, i64,
                                             u64p, i64p, ctypes.c_int]
        L.gfrs_encode_idx.argtypes = [vp, vp, ctypes.c_int, vpp,
                                      ctypes.c_size_t, ctypes.c_int]
        L.gfrs_encode_frame_batch.argtypes = [vp, vp, ctypes.c_size_t, vp,
                                              ctypes.c_size_t, ctypes.c_size_t,
                                              ctypes.c_int, i64]
        L.gfrs_reconstruct_verify_batch.argtypes = [vp, vp, ctypes.c_size_t,
                                                    ctypes.c_size_t,
                                                    ctypes.c_int, i32p,
                                                    ctypes.c_int, u64p]
        L.gfrs_update_idx.argtypes = [vp, vp, vp, ctypes.c_int, vpp,
                                      ctypes.c_size_t, ctypes.c_int]
        L.gfrs_repair_batch.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_size_t,
                                        ctypes.c_int, i32p, ctypes.c_int, vp,
                                        ctypes.c_size_t, i64, u64p, u64p, u64p]
        L.gfrs_encode_matrix.argtypes = [vp, ctypes.POINTER(ctypes.c_uint8)]
        u8p, ip = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int)
        u32p = ctypes.POINTER(ctypes.c_uint32)
        L.gfrs_compute_plan.argtypes = [ctypes.POINTER(Tactic), ctypes.c_int,
                                        i32p, ctypes.c_int, ctypes.c_int,
                                        i32p, ip, i32p, ip, u8p, ip, u32p,
                                        u32p]
        L.gfrs_reconstruct_verify_queue.argtypes = [vp, vp,
                                                    ctypes.POINTER(QJob),
                                                    ctypes.c_int, i32p, i32p,
                                                    ctypes.c_int, u64p]
        L.gfrs_compute_queue_schedule.argtypes = [
            ctypes.POINTER(Tactic), ctypes.POINTER(QJob), ctypes.c_int, i32p,
            i32p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
            ctypes.POINTER(QItem), u64p, ip, ctypes.POINTER(QBucket), ip,
            i32p, u8p, i32p, ip]
        L.gfrs_repair_queue.argtypes = [vp, vp, ctypes.POINTER(RJob),
                                        ctypes.c_int, i32p, i32p,
                                        ctypes.c_int, vp, i64, u64p, u64p,
                                        u64p]
        L.gfrs_compute_repair_queue_schedule.argtypes = [
            ctypes.POINTER(Tactic), ctypes.POINTER(RJob), ctypes.c_int, i32p,
            i32p, ctypes.c_int, i64, u64p, u64p, ctypes.c_int, ctypes.c_int,
            ctypes.POINTER(RItem), u64p, ip, ctypes.POINTER(RBucket), ip,
            ctypes.POINTER(RImage), ip, i32p, i32p, i32p, u32p, i32p, ip]
        L.gfrs_encode_frame_queue.argtypes = [vp, vp, vp,
                                              ctypes.POINTER(EJob),
                                              ctypes.c_int, i64]
        L.gfrs_compute_encode_queue_schedule.argtypes = [
            ctypes.POINTER(Tactic), ctypes.POINTER(EJob), ctypes.c_int, i64,
            ctypes.c_int, ctypes.POINTER(EItem), u64p, ip,
            ctypes.POINTER(EBucket), ip, ip]
        L.gfrs_read_queue.argtypes = [vp, vp, vp, ctypes.POINTER(GJob),
                                      ctypes.c_int, i32p, i32p, ctypes.c_int,
                                      i64, u32p]
        L.gfrs_compute_read_queue_schedule.argtypes = [
            ctypes.POINTER(Tactic), ctypes.POINTER(GJob), ctypes.c_int, i32p,
            i32p, ctypes.c_int, i64, ctypes.c_int, ctypes.POINTER(GItem),
            u64p, ip, ctypes.POINTER(GBucket), ip, i32p, i32p, i32p, ip]
        L.gfrs_shard_read_queue.argtypes = [vp, vp, vp, ctypes.POINTER(SJob),
                                            ctypes.c_int, i64,
                                            ctypes.POINTER(SResult)]
        L.gfrs_compute_shard_read_queue_schedule.argtypes = [
            ctypes.POINTER(SJob), ctypes.c_int, i64, ctypes.c_int,
            ctypes.POINTER(SItem), u64p, ip, ctypes.POINTER(SBucket), ip,
            u64p]
        L.gfrs_shard_write_queue.argtypes = [vp, vp, vp, ctypes.POINTER(WJob),
                                             ctypes.c_int, i64,
                                             ctypes.POINTER(SResult)]
        L.gfrs_compute_shard_write_queue_schedule.argtypes = [
            ctypes.POINTER(WJob), ctypes.c_int, i64, ctypes.c_int,
            ctypes.POINTER(WItem), u64p, ip, ctypes.POINTER(WBucket), ip,
            u64p]
        L.gfrs_put_queue.argtypes = [vp, vp, vp, ctypes.POINTER(PJob),
                                     ctypes.c_int, u64p, ctypes.c_int, i64,
                                     u32p]
        L.gfrs_compute_put_queue_schedule.argtypes = [
            ctypes.POINTER(Tactic), ctypes.POINTER(PJob), ctypes.c_int, u64p,
            ctypes.c_int, i64, ctypes.c_int, ctypes.c_int,
            ctypes.POINTER(EItem), u64p, ip, ctypes.POINTER(EBucket), ip,
            ctypes.POINTER(RImage), ip, ip, ip, i32p]
        _lib = L
    return _lib


def check(rc, what=""):
    if rc < 0:
        raise GfrsError(rc, "%s: %s" % (what, lib().gfrs_last_error().decode()))
    return rc


def available():
    try:
        return lib().gfrs_device_count() > 0
    except ImportError:
        return False


def version():
    return lib().gfrs_version().decode()
