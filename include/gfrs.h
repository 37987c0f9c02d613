/* include/gfrs.h — C ABI of the MI355X-native erasure-coding + checksum
 * engine for CubeFS blobstore ("gfrs" = GF(2^8) Reed-Solomon).
 *
 * This is the drop-in boundary replacing the compute underneath
 * blobstore/common/ec.Encoder (encoder.go:41-62) and
 * blobstore/common/crc32block.  The reference has no FFI of its own (the
 * arithmetic is reached through Go interfaces), so each entry point below
 * names the Go interface method it replaces; INTEGRATION.md shows the cgo
 * shim a CubeFS maintainer would add so access/stream and blobnode/worker
 * call this engine unchanged.
 *
 * Memory model: shard buffers are caller-owned, equal-length; data shards
 * are read-only during Encode (reedsolomon.go:30-32).  Pointers may be HIP
 * device pointers (GFRS_MEM_DEVICE) or plain host pointers
 * (GFRS_MEM_HOST, staged through pinned buffers internally — the cgo path).
 * A context is thread-safe and may be shared, like one ec.Encoder shared by
 * many goroutines (encoder.go:114-151).
 *
 * Layout contract (every entry point; pinned by tests/test_gpu_layout.py):
 *  - Sources need NO alignment: shard pointers, batch `base`, `src` and
 *    framed/image inputs may sit at any byte address, shard_len may be any
 *    positive length (so later shards of a stripe start misaligned), and
 *    stripe_stride / src_stride / input image strides may carry any
 *    padding beyond the packed size.  Alignment only affects speed.
 *  - Destination image rows (framed, dst, disk_dst) are 4-byte aligned:
 *    the base pointer and framed_stride / dst_stride are multiples of 4;
 *    the stride may be tight (the image size rounded up to 4) or padded.
 *    Shards written in place inside `base` (parity, reconstructed shards)
 *    follow the source rule: no alignment.
 *  - Only declared outputs are written.  Padding between stripes, between
 *    image rows and past the last row, and every input shard, are never
 *    written.  gfrs_encode_frame_batch returning GFRS_ERR_UNSUPPORTED
 *    writes nothing; when it runs as the encode_batch +
 *    crc32b_encode_batch composition the parity shards inside `base` are
 *    written too (encode_batch's declared output), the fused paths leave
 *    them untouched.
 *
 * Verdict contract (pinned by tests/test_gpu_verdict_sweep.py and
 * tests/test_gpu_verdict_crc.py, next to tests/test_gpu_layout.py): the
 * fail bitmap of gfrs_reconstruct_verify_batch, gfrs_repair_batch and
 * gfrs_reconstruct_batch + gfrs_verify_batch equals the reference's
 * Reconstruct followed by Verify on the same bytes, local stripes
 * included, for every erasure pattern and whichever surviving column is
 * corrupted; bad_block / err of the crc32block, sized-coder and shard-image
 * entry points equal the reference's answer for the same image.
 *
 * Ordering contract (pinned by tests/test_gpu_sequences.py): the declared
 * outputs of a call are what that call alone would produce, whatever calls
 * follow it on the same context, from any thread, with or without an
 * intervening gfrs_synchronize.  The async batch calls return with their
 * work - and the uploads of their ids that feed it - queued on the context's
 * stream; a later call that needs the scratch they still read waits for
 * that upload on the host (only then; an idle context pays one flag test),
 * everything else is ordered by the stream.  The caller's side of it: the
 * buffers handed to an async call stay untouched until gfrs_synchronize, and
 * two calls whose declared outputs overlap are the caller's to order.
 * gfrs_set_stream drains the stream the context leaves before it switches,
 * so nothing queued on the previous stream is still reading the context's
 * scratch when the first call on the new stream reuses it, and every output
 * of the calls issued before the switch is complete when it returns.
 */
#ifndef GFRS_H
#define GFRS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Error codes: one per Go sentinel the cgo shim maps back.
 * 0 = success; negative = failure. */
enum {
  GFRS_OK = 0,
  GFRS_ERR_INVALID_CODEMODE = -1, /* ec.ErrInvalidCodeMode (encoder.go:35) */
  GFRS_ERR_TOO_FEW_SHARDS = -2,   /* reedsolomon.ErrTooFewShards (:598) */
  GFRS_ERR_SHARD_SIZE = -3,       /* reedsolomon.ErrShardSize */
  GFRS_ERR_SHARD_NO_DATA = -4,    /* reedsolomon.ErrShardNoData */
  GFRS_ERR_VERIFY = -5,           /* ec.ErrVerify (encoder.go:36) */
  GFRS_ERR_INVALID_SHARDS = -6,   /* ec.ErrInvalidShards (encoder.go:37) */
  GFRS_ERR_SHORT_DATA = -7,       /* ec.ErrShortData / rs.ErrShortData */
  GFRS_ERR_SINGULAR = -8,         /* matrix.errSingular (matrix.go:186) */
  GFRS_ERR_MISMATCHED_CRC = -9,   /* crc32block.ErrMismatchedCrc */
  GFRS_ERR_INVALID_BLOCK = -10,   /* crc32block.ErrInvalidBlock */
  GFRS_ERR_READ_ON_CLOSED = -11,  /* crc32block.ErrReadOnClosed
                                     (request_body.go streaming bodies) */
  GFRS_ERR_HIP = -100,            /* HIP runtime failure (see gfrs_last_error) */
  GFRS_ERR_NO_GPU = -101,         /* no MI355X visible; the engine never
                                     falls back to CPU — by design */
  GFRS_ERR_NOMEM = -102,
  GFRS_ERR_UNSUPPORTED = -103,
};

/* Where shard pointers live. */
enum { GFRS_MEM_DEVICE = 0, GFRS_MEM_HOST = 1 };

/* codemode.Tactic (codemode.go:156-190). */
typedef struct gfrs_tactic {
  int32_t n;              /* data shards */
  int32_t m;              /* global parity shards */
  int32_t l;              /* local (AZ) parity shards, 0 for plain RS */
  int32_t az_count;       /* AZ count; n,m,l all divisible by it */
  int32_t put_quorum;     /* carried for the shim; unused by compute */
  int32_t get_quorum;
  int32_t min_shard_size; /* ec.Buffer alignment floor (buf.go:79-83) */
} gfrs_tactic;

typedef struct gfrs_ctx gfrs_ctx;

/* ---- lifecycle ---- */

/* ec.NewEncoder(ec.Config{CodeMode: t}) (encoder.go:78-112).
 * device < 0 selects the current HIP device.  Returns NULL on failure
 * (gfrs_last_error() has the reason). */
gfrs_ctx *gfrs_create(const gfrs_tactic *t, int device);
void gfrs_destroy(gfrs_ctx *ctx);
const char *gfrs_last_error(void);
const char *gfrs_version(void);
int gfrs_device_count(void);

/* Optional: run on an existing HIP stream (e.g. torch's). stream==NULL
 * reverts to the context's own stream.  Blocks until the work this context
 * queued on the stream it leaves is done (ordering contract above); not a
 * call for a hot path.  The stream that is left may have been destroyed by
 * its owner already. */
int gfrs_set_stream(gfrs_ctx *ctx, void *hip_stream);
int gfrs_synchronize(gfrs_ctx *ctx);

/* ---- single stripe (the ec.Encoder surface) ----
 * shards: n+m+l pointers, each shard_len bytes, all in `memloc` memory.
 * Single-stripe calls BLOCK until the result is ready (ec.Encoder
 * semantics: the caller owns the buffers on return).  The batch APIs
 * below are async on the ctx stream; synchronize with
 * gfrs_synchronize().  When the shards form one contiguous ec.Buffer
 * layout (buf.go:24-35) the pointer-table upload is skipped.
 *
 * Single-stripe contract (pinned by tests/test_gpu_single_stripe.py; it
 * covers gfrs_encode_idx and gfrs_update_idx further down as well):
 *  - Only declared outputs are written: the parities of gfrs_encode, the
 *    shards listed in bad_idx of gfrs_reconstruct (with data_only the data
 *    shards among them; a lost parity then keeps the caller's bytes), the m
 *    global parities of gfrs_encode_idx / gfrs_update_idx (never a local
 *    parity).  gfrs_verify writes *ok and nothing else.  Every input shard
 *    and every byte between and around the shards stay as they were, for any
 *    shard_len >= 1 and any alignment.  The contiguous and the pointer-table
 *    form of gfrs_encode write the same bytes.
 *  - A GFRS_MEM_HOST gfrs_reconstruct copies back only the shards it rebuilt;
 *    the buffers of surviving shards are never written.
 *  - An LRC context (l > 0) accepts two forms of gfrs_verify and
 *    gfrs_reconstruct: the full set, nshards == n+m+l, where Verify checks
 *    the global stripe and every local stripe and Reconstruct rebuilds global
 *    shards from the global stripe and lost local parities from their AZ's
 *    stripe; and one local stripe given on its own, nshards ==
 *    (n+m+l) / az_count (lrcencoder.go:93-99,147-152), the shards of one AZ in
 *    LocalStripeInAZ order, a plain RS((n+m)/az_count + l/az_count) stripe
 *    with bad_idx counting positions in that list.  data_only has no meaning
 *    in the local form (the reference's ReconstructData slices to n+m) and is
 *    not part of the contract there.  gfrs_encode takes the full set only.
 *  - Errors.  A refused call writes nothing (gfrs_verify leaves *ok alone)
 *    and launches nothing; all but gfrs_reconstruct's
 *    GFRS_ERR_TOO_FEW_SHARDS return before anything is staged or uploaded
 *    either.  Checks run in the order listed:
 *      gfrs_encode        nshards != n+m+l          GFRS_ERR_INVALID_SHARDS
 *                         shard_len == 0            GFRS_ERR_SHARD_NO_DATA
 *      gfrs_verify,       nshards neither n+m+l nor (l > 0) (n+m+l)/az_count
 *      gfrs_reconstruct                             GFRS_ERR_INVALID_SHARDS
 *                         shard_len == 0            GFRS_ERR_SHARD_NO_DATA
 *      gfrs_reconstruct   a bad index outside [0, nshards)
 *                                                   GFRS_ERR_INVALID_SHARDS
 *                         more than m of the n+m global shards lost, with or
 *                         without lost local parities (none of which is then
 *                         written); local form: more than l/az_count losses
 *                                                   GFRS_ERR_TOO_FEW_SHARDS
 *                         nbad == 0, or data_only with only parities lost
 *                                                   GFRS_OK, nothing written
 *      gfrs_encode_idx,   nparity != m              GFRS_ERR_TOO_FEW_SHARDS
 *      gfrs_update_idx    nparity == 0 (replicate)  GFRS_OK, nothing done,
 *                                                   whatever idx is
 *                         idx outside [0, n)        GFRS_ERR_INVALID_SHARDS
 *                         shard_len == 0            GFRS_ERR_SHARD_NO_DATA
 *    (reedsolomon.go:632-647, checkShards :1314-1318).  A replicate context
 *    (m == 0) keeps its own answers: Encode and Verify are no-ops that check
 *    nshards only, Reconstruct succeeds only when nothing is missing.  The
 *    batch calls below are not part of this table. */

/* Encoder.Encode (encoder.go:114 / lrcencoder.go:35): fills parity (and
 * local parity when l > 0) from the data shards. */
int gfrs_encode(gfrs_ctx *ctx, void *const *shards, size_t shard_len,
                int nshards, int memloc);

/* Encoder.Verify (encoder.go:133): *ok=1 when parity matches. */
int gfrs_verify(gfrs_ctx *ctx, void *const *shards, size_t shard_len,
                int nshards, int memloc, int *ok);

/* Encoder.Reconstruct / ReconstructData (encoder.go:139-151,
 * lrcencoder.go:133-207): bad_idx lists missing shard indices; their
 * buffers must be allocated (shard_len bytes) and are overwritten. */
int gfrs_reconstruct(gfrs_ctx *ctx, void *const *shards, size_t shard_len,
                     int nshards, int memloc, const int32_t *bad_idx,
                     int nbad, int data_only);

/* ---- stripe batches (blobnode repair/migrate bulk path,
 * worker_slice_recover.go:804-888) ----
 * Stripes laid out contiguously: stripe s shard i starts at
 * base + s*stripe_stride + i*shard_len (the ec.Buffer layout, buf.go:24-35).
 * base is always a device pointer. */

int gfrs_encode_batch(gfrs_ctx *ctx, void *base, size_t shard_len,
                      size_t stripe_stride, int nstripes);
/* fail_bitmap (host, optional): bit s set when stripe s fails verify. */
int gfrs_verify_batch(gfrs_ctx *ctx, const void *base, size_t shard_len,
                      size_t stripe_stride, int nstripes,
                      uint64_t *fail_bitmap);
/* One missing pattern shared by the whole batch (one repair tasklet). */
int gfrs_reconstruct_batch(gfrs_ctx *ctx, void *base, size_t shard_len,
                           size_t stripe_stride, int nstripes,
                           const int32_t *bad_idx, int nbad, int data_only);

/* ---- crc32block (blobstore/common/crc32block) ----
 * block_len must be a positive multiple of 4096 (util.go:40); frame =
 * 4 B LE CRC32-IEEE ‖ payload (block.go:22-49).  dst/src are device
 * pointers; *_host variants stage host memory. */

int64_t gfrs_crc32b_encode_size(int64_t size, int64_t block_len);
int64_t gfrs_crc32b_decode_size(int64_t size, int64_t block_len);

/* Host-side CRC32-IEEE in hash/crc32 Update semantics: pass the previous
 * finalized crc (0 for a fresh start) and get the finalized crc of the
 * concatenation.  This exists for the per-block STREAMING request-body
 * wrapper (crc32block/request_body.go:57-127), which in the reference
 * runs on the client/server host too — every bulk path computes CRCs on
 * device.  Needs no ctx and no GPU. */
uint32_t gfrs_crc32_host(uint32_t crc, const void *data, int64_t n);

/* Frame n raw bytes from src into dst (encode.go:86-106).
 * dst capacity must be gfrs_crc32b_encode_size(n).  Returns bytes
 * written or a negative error. */
int64_t gfrs_crc32b_encode(gfrs_ctx *ctx, void *dst, const void *src,
                           int64_t n, int64_t block_len);
/* Check all frames (decode.go:84-107).  *bad_block = first failing block
 * index or -1.  Returns GFRS_OK even when CRCs mismatch (inspect
 * *bad_block); negative only on launch/arg errors. */
int gfrs_crc32b_verify(gfrs_ctx *ctx, const void *framed, int64_t framed_len,
                       int64_t block_len, int64_t *bad_block);
/* Strip frames into dst, checking CRCs.  Returns payload bytes or
 * GFRS_ERR_MISMATCHED_CRC. */
int64_t gfrs_crc32b_decode(gfrs_ctx *ctx, void *dst, const void *framed,
                           int64_t framed_len, int64_t block_len);

/* Batched framing of many equal-length shards (datafile.go:342-445 write
 * path): shard i raw at src + i*src_stride, framed at dst + i*dst_stride. */
int gfrs_crc32b_encode_batch(gfrs_ctx *ctx, void *dst, size_t dst_stride,
                             const void *src, size_t src_stride, int64_t n,
                             int64_t block_len, int nshards);
int gfrs_crc32b_verify_batch(gfrs_ctx *ctx, const void *framed,
                             size_t stride, int64_t framed_len,
                             int64_t block_len, int nshards,
                             int64_t *bad_block_per_shard);

/* ---- fused encode+frame (the PUT pipeline: stream_put.go:146 encode +
 * datafile.go:342 framing in ONE pass) ----
 * Reads the data shards once, computes parity in registers and writes
 * ONLY the k+m crc32block-framed shard images (frame image j of stripe s
 * at framed + (s*(n+m)+j)*framed_stride); the unframed parity never
 * touches HBM.  Requires block_len 65536, 1<=m<=4, n+m<=16, l==0 and
 * framed_stride % 4 == 0; other shapes fall back to
 * encode_batch + crc32b_encode_batch (which needs
 * stripe_stride == (n+m)*shard_len so the shard rows form one strided
 * array).  Framed bytes are identical either way. */
int gfrs_encode_frame_batch(gfrs_ctx *ctx, void *framed,
                            size_t framed_stride, void *base,
                            size_t shard_len, size_t stripe_stride,
                            int nstripes, int64_t block_len);

/* ---- sized coder (crc32block/sized_coder.go, the rpc2 body framing) ----
 * Frame = payload (block_len-4) ‖ CRC32-IEEE big-endian (ModeEncode,
 * sized_coder.go:256-279); the encoded stream is zero-padded to the
 * transport alignment of 512 (PartialEncodeSizeWith, util.go:73-80).
 * *size returns total bytes incl. tail pad; *tail the pad length. */
int gfrs_sized_encode_size(int64_t actual_size, int64_t block_len,
                           int64_t *size, int64_t *tail);
int64_t gfrs_sized_decode_size(int64_t total, int64_t tail, int64_t block_len);
/* Encode n raw bytes into dst (device); writes the tail pad.  Returns
 * total bytes written (incl. pad) or negative error. */
int64_t gfrs_sized_encode(gfrs_ctx *ctx, void *dst, const void *src,
                          int64_t n, int64_t block_len);
/* Verify all frames of a sized body (total includes tail pad). */
int gfrs_sized_verify(gfrs_ctx *ctx, const void *framed, int64_t total,
                      int64_t tail, int64_t block_len, int64_t *bad_block);
int64_t gfrs_sized_decode(gfrs_ctx *ctx, void *dst, const void *framed,
                          int64_t total, int64_t tail, int64_t block_len);

/* ---- blobnode on-disk shard image (core/shard.go:42-111,
 * datafile.go:342-445) ----
 * image = 32 B header (crc|magic|bid|vuid|size|reserved, big-endian) ‖
 * crc32block body ‖ 8 B footer (magic | crc32 of the raw data).  Writing
 * a repaired shard through this produces bytes directly pwrite()-able by
 * blobnode. */
int64_t gfrs_shard_disk_size(int64_t size, int64_t block_len);
/* Frame shard j (raw at src + j*src_stride, size bytes) into a full disk
 * image at dst + j*dst_stride; bids/vuids are per-shard metadata. */
int gfrs_shard_write_batch(gfrs_ctx *ctx, void *dst, size_t dst_stride,
                           const void *src, size_t src_stride, int64_t size,
                           int64_t block_len, const uint64_t *bids,
                           const uint64_t *vuids, int nshards);
/* Parse + fully verify images (header crc+magic, every body block crc,
 * footer magic + whole-shard crc).  out_meta: per shard
 * {bid, vuid, size, err} as 4 uint64 (err 0 or GFRS_ERR_MISMATCHED_CRC
 * cast); bad_block_per_shard as in crc32b_verify_batch. */
int gfrs_shard_parse_batch(gfrs_ctx *ctx, const void *img, size_t stride,
                           int64_t size, int64_t block_len,
                           uint64_t *out_meta, int64_t *bad_block_per_shard,
                           int nshards);

/* Fused reconstruct+verify (worker_slice_recover.go:804-888: the
 * mandatory Verify after Reconstruct, :865-874) in ONE data pass: the
 * decode rows are substituted into the parity-check rows so every output
 * — reconstructed shard or parity comparison — is a matrix apply over the
 * same k valid inputs.  Stored parity is compared in-register; bad_idx
 * shards are rewritten.  fail_bitmap bit s set when stripe s's parity
 * does not match.  Plain RS only (l == 0); LRC falls back to
 * reconstruct_batch + verify_batch. */
int gfrs_reconstruct_verify_batch(gfrs_ctx *ctx, void *base,
                                  size_t shard_len, size_t stripe_stride,
                                  int nstripes, const int32_t *bad_idx,
                                  int nbad, uint64_t *fail_bitmap);

/* ---- repair queue (worker_slice_recover.go:804-888, the loop over bids) ----
 * ShardRecover.repair does not see uniform batches: every bid has its own
 * size and its own set of failed downloads (:826-840).  A queue is a list
 * of such jobs over one device buffer, served by a bounded number of
 * launches and ONE sync: at most 4 * ceil(max_rows / 4) kernel launches
 * whatever njobs and npat are (max_rows: missing data + m for plain RS, bad
 * shards + check rows, at most 32, for LRC).
 *
 * Pattern p is bad_idx[bad_off[p] .. bad_off[p+1]); bad_off has npat+1
 * non-decreasing entries starting at 0.  An empty pattern is legal and
 * means verify only.  jobs, bad_idx, bad_off and fail_bitmap are host
 * memory; base is a device pointer.
 *
 * Queue contract (pinned by tests/test_gpu_queue.py):
 *  - Per-job result.  For each job j the bytes written and bit j of
 *    fail_bitmap are exactly what gfrs_reconstruct_verify_batch(ctx,
 *    base + off, shard_len, <any stride>, 1, pattern...) produces for that
 *    stripe alone, i.e. the reference's Reconstruct followed by Verify,
 *    local stripes included.
 *  - Bit numbering.  Bit j refers to the caller's job order, whatever order
 *    the engine processes jobs in.  fail_bitmap holds (njobs+63)/64 words.
 *  - Layout.  No alignment is required of off or shard_len.  Only the bad
 *    shards of each job are written: nothing between jobs and no surviving
 *    shard.  Jobs must not overlap (not checked).
 *  - Validation.  Everything is validated before the first launch, and any
 *    error returns its code and writes nothing:
 *      every pattern, used by a job or not, with the codes the batch call
 *      returns - GFRS_ERR_INVALID_SHARDS for an index out of range (and,
 *      for LRC, a repeated index), GFRS_ERR_TOO_FEW_SHARDS when more than m
 *      of the n+m global shards are bad;
 *      GFRS_ERR_INVALID_SHARDS for njobs <= 0, npat <= 0, a malformed
 *      bad_off, pattern outside [0, npat) or reserved != 0;
 *      GFRS_ERR_SHARD_NO_DATA for shard_len == 0.
 *  - Blocking.  The call blocks until the bitmap is ready, like
 *    gfrs_reconstruct_verify_batch; it runs on the context stream and takes
 *    the context mutex once.
 *  - Slow patterns.  LRC tactics outside the single-pass budget (m + l > 4
 *    or n + m + l > 16) and LRC patterns whose plan needs more than 32 rows
 *    have no single-pass plan.  Their jobs run one at a time after the queue
 *    launches, as reconstruct + verify on the same stream: correct, but two
 *    data passes and several launches per job.
 *  - A job shorter than a 4096-byte tile still occupies a whole tile of the
 *    kernel (small jobs are not packed together). */
typedef struct gfrs_qjob {
  uint64_t off;       /* shard 0 of this job at base + off; shard i at
                         base + off + i*shard_len (ec.Buffer layout) */
  uint64_t shard_len; /* > 0, any value, no alignment */
  int32_t pattern;    /* 0 <= pattern < npat */
  int32_t reserved;   /* must be 0 */
} gfrs_qjob;

int gfrs_reconstruct_verify_queue(gfrs_ctx *ctx, void *base,
                                  const gfrs_qjob *jobs, int njobs,
                                  const int32_t *bad_idx,
                                  const int32_t *bad_off, int npat,
                                  uint64_t *fail_bitmap);

/* ---- incremental parity (reedsolomon.go:631-668 EncodeIdx) ----
 * Adds data shard idx's contribution into the m parity shards:
 * parity[r] ^= coeff[r][idx]*data.  Parity must be zeroed before the
 * first call; each data shard delivered exactly once.  Device pointers.
 * Errors as in the single-stripe contract above; an idx outside [0, n) is
 * the reference's ErrInvShardNum, which has no code of its own here and is
 * reported as GFRS_ERR_INVALID_SHARDS. */
int gfrs_encode_idx(gfrs_ctx *ctx, const void *data_shard, int idx,
                    void *const *parity, size_t shard_len, int nparity);

/* Update (reedsolomon.go:676-766): replace data shard idx's content and
 * patch the parity in place: parity[r] ^= coeff[r][idx]*(old ^ new) —
 * applied as two accumulate passes by GF(2^8) linearity.  old_shard and
 * new_shard are device pointers; the caller swaps its own data buffer. */
int gfrs_update_idx(gfrs_ctx *ctx, const void *old_shard,
                    const void *new_shard, int idx, void *const *parity,
                    size_t shard_len, int nparity);

/* ---- fused repair pipeline (worker_slice_recover.go:804-888 +
 * datafile.go:342-407) ----
 * One stream-ordered call per repair tasklet: reconstruct the bad shards
 * of every stripe, verify all parity (mandatory Verify, :865-874), then
 * frame each repaired shard into a pwrite()-able disk image.  Intermediate
 * data never leaves HBM; on the fused path the raw reconstruction is
 * never materialized, so the bad shards' regions of `base` are left
 * UNSPECIFIED after the call (the reference worker also only consumes
 * the repaired bytes through the written bids).  For LRC the surviving
 * local parities serve as extra verify equations, so corruption is
 * detected even when the global stripe has no spare parity.  The fused
 * kernel carries m + l <= 4 rows (rebuilt + checked); wider tactics
 * (e.g. RS(6+6)) reconstruct in place, verify every parity and then frame.
 *   disk_dst: nstripes*nbad images, image (s,b) at
 *             disk_dst + (s*nbad + b)*dst_stride
 *   bids/vuids: one per (stripe, bad shard), same order
 *   fail_bitmap: bit s set when stripe s failed verify (those images are
 *             still written; the caller drops them like the reference
 *             drops failed bids). */
int gfrs_repair_batch(gfrs_ctx *ctx, void *base, size_t shard_len,
                      size_t stripe_stride, int nstripes,
                      const int32_t *bad_idx, int nbad, void *disk_dst,
                      size_t dst_stride, int64_t block_len,
                      const uint64_t *bids, const uint64_t *vuids,
                      uint64_t *fail_bitmap);

/* ---- repair-image queue (worker_slice_recover.go:804-888 +
 * datafile.go:342-407: the loop over bids, with the disk images) ----
 * gfrs_repair_batch as a queue: every job has its own place, shard length
 * and erasure pattern (as in gfrs_reconstruct_verify_queue) and gets back a
 * verdict bit and one pwrite()-able disk image per bad shard of its pattern.
 * Patterns are given as for gfrs_reconstruct_verify_queue (bad_idx / bad_off,
 * npat + 1 offsets); jobs, bad_idx, bad_off, bids, vuids and fail_bitmap are
 * host memory, base and disk_dst device pointers.
 *
 * Repair-queue contract (pinned by tests/test_gpu_repair_queue.py):
 *  - Per-job result.  For each job j the images and bit j of fail_bitmap are
 *    exactly what gfrs_repair_batch(ctx, base + off, shard_len, <any stride>,
 *    1, pattern..., disk_dst + img_off, img_stride, ...) produces for that
 *    stripe alone: images byte-identical to the reference's shard write of
 *    its reconstruction, in the caller's column order within the pattern
 *    (the image of the pattern's b-th bad shard at img_off + b*img_stride);
 *    the verdict is the reference's Reconstruct followed by Verify, local
 *    stripes included.  A failed job's images are still written, their
 *    content unspecified, as for gfrs_repair_batch.
 *  - Ids.  bids and vuids hold one entry per image, job-major, in the
 *    pattern's own order: job j's first id sits at the sum of the pattern
 *    sizes of jobs 0..j-1.
 *  - Bit numbering.  Bit j refers to the caller's job order; fail_bitmap
 *    holds (njobs+63)/64 words.
 *  - Layout.  Sources need no alignment.  disk_dst + img_off and img_stride
 *    are multiples of 4.  In disk_dst only the declared images are written:
 *    nothing between images, nothing past an image's gfrs_shard_disk_size
 *    bytes.  In base, surviving shards and the gaps between jobs are never
 *    written; the bad shards' regions of base are unspecified after the
 *    call, as for gfrs_repair_batch.  Overlapping jobs or images are a
 *    caller error (not checked).
 *  - Validation.  Everything is validated before the first launch, and any
 *    error returns its code and writes nothing, neither in base nor in
 *    disk_dst:
 *      every pattern, used by a job or not, with the codes of
 *      gfrs_reconstruct_verify_queue (GFRS_ERR_INVALID_SHARDS for an index
 *      out of range, GFRS_ERR_TOO_FEW_SHARDS for more than m global losses);
 *      GFRS_ERR_INVALID_SHARDS for a pattern that is empty or repeats an
 *      index - this call is strict for every tactic, where the RS(6+6)
 *      legacy path of gfrs_repair_batch tolerates a repeat;
 *      GFRS_ERR_INVALID_SHARDS for njobs <= 0, npat <= 0, a malformed
 *      bad_off, pattern outside [0, npat), reserved != 0, a misaligned
 *      img_off or img_stride, or img_stride below the image size;
 *      GFRS_ERR_SHARD_NO_DATA for shard_len == 0;
 *      GFRS_ERR_UNSUPPORTED for block_len != 65536 (the only frame size
 *      blobnode writes; the fused kernels have it as a compile-time
 *      constant).
 *  - Blocking.  The call blocks until the bitmap is ready, runs on the
 *    context stream and takes the context mutex once.
 *  - Launch bound.  A pattern the fused kernel of gfrs_repair_batch serves
 *    (m >= 1, m + l <= 4, n + m + l <= 16, at most m global losses) is
 *    reconstructed, verified and framed in one pass; all such jobs of a queue
 *    share at most 4 launches (one per row count).  Every other pattern
 *    (RS(6+6), 17 shards, LRC outside the budget) is reconstructed and
 *    verified in base by the schedule of gfrs_reconstruct_verify_queue, at
 *    most 4 * ceil(max_rows / 4) launches, and its repaired shards are then
 *    framed from base by the same <= 4 launches.  One more launch writes
 *    every header and footer.  So a queue costs at most
 *    4 + 4 * ceil(max_rows / 4) + 1 kernel launches whatever njobs and npat
 *    are - except for jobs of LRC slow patterns (see the queue contract
 *    above), which are reconstructed and verified one at a time.
 *  - A job of at most 4096 bytes per shard still occupies one workgroup per
 *    image frame (small jobs are not packed together). */
typedef struct gfrs_rjob {
  uint64_t off;        /* shard i of the job at base + off + i*shard_len */
  uint64_t shard_len;  /* > 0, any value, no alignment */
  uint64_t img_off;    /* image of the pattern's b-th bad shard at
                          disk_dst + img_off + b*img_stride */
  uint64_t img_stride; /* >= gfrs_shard_disk_size(shard_len, 65536) */
  int32_t pattern;     /* 0 <= pattern < npat */
  int32_t reserved;    /* must be 0 */
} gfrs_rjob;

int gfrs_repair_queue(gfrs_ctx *ctx, void *base, const gfrs_rjob *jobs,
                      int njobs, const int32_t *bad_idx,
                      const int32_t *bad_off, int npat, void *disk_dst,
                      int64_t block_len, const uint64_t *bids,
                      const uint64_t *vuids, uint64_t *fail_bitmap);

/* ---- encode+frame queue (stream_put.go:146 + datafile.go:342: the PUT path
 * over concurrent blobs of different sizes) ----
 * gfrs_encode_frame_batch as a queue: every job has its own place, shard
 * length and image place, and gets back the n+m+l crc32block-framed images of
 * its stripe.  jobs is host memory, base and framed device pointers.
 *
 * Encode-queue contract (pinned by tests/test_gpu_encode_queue.py):
 *  - Per-job result.  For each job j the n+m+l images are byte-identical to
 *    what gfrs_encode_frame_batch(ctx, framed + img_off, img_stride,
 *    base + off, shard_len, <any stride>, 1, 65536) produces for that stripe
 *    alone: the reference's Encode followed by crc32block framing of every
 *    shard, local parities included (image of shard i at
 *    framed + img_off + i*img_stride).
 *  - Layout.  Sources need no alignment.  framed + img_off and img_stride are
 *    multiples of 4.  In framed only the declared images are written: nothing
 *    between images, nothing past an image's gfrs_crc32b_encode_size bytes.
 *    In base nothing is written for tactics the fused kernels serve; for the
 *    others (slow tactics, below) the parity shards of each job are written in
 *    base, which is gfrs_encode_batch's declared output.  Overlapping jobs or
 *    images are a caller error (not checked).
 *  - Validation.  Everything is validated before the first launch, and any
 *    error returns its code and writes nothing, neither in base nor in framed:
 *      GFRS_ERR_INVALID_BLOCK for block_len <= 0 or not a multiple of 4096 (as
 *      the batch call);
 *      GFRS_ERR_UNSUPPORTED for any other block_len != 65536 (as
 *      gfrs_repair_queue);
 *      GFRS_ERR_INVALID_SHARDS for njobs <= 0, reserved != 0, a misaligned
 *      framed + img_off or img_stride, or img_stride below the image size;
 *      GFRS_ERR_SHARD_NO_DATA for shard_len == 0.
 *  - Blocking.  The call blocks until the images are ready, like the other
 *    two queues; it runs on the context stream, takes the context mutex once
 *    and makes one upload of one blob and one sync.
 *  - Launch bound.  For a tactic the fused kernels serve - the gate of
 *    gfrs_encode_frame_batch: m >= 1, m + l <= 4, n + m + l <= 16 - a queue
 *    costs at most 6 kernel launches whatever njobs is: jobs of at most 4096
 *    bytes per shard run one wave per job, one launch per
 *    ceil(shard_len / 1024) = 1..4; longer jobs run one workgroup per 64 KiB
 *    frame, one launch below 1 MiB per shard and one from 1 MiB up (the two
 *    variants the batch call picks by that threshold).
 *  - Slow tactics.  Tactics outside that gate (RS(6+6), 17 shards, wide LRC)
 *    run their jobs one at a time after validation, each as the composition
 *    the batch call falls back to (gfrs_encode_batch, then
 *    gfrs_crc32b_encode_batch of the n+m+l shards): correct, but several
 *    launches per job. */
typedef struct gfrs_ejob {
  uint64_t off;        /* shard i of the job at base + off + i*shard_len,
                          i < n+m+l (ec.Buffer layout); data shards are read */
  uint64_t shard_len;  /* > 0, any value, no alignment */
  uint64_t img_off;    /* framed image of shard j at
                          framed + img_off + j*img_stride, j < n+m+l */
  uint64_t img_stride; /* multiple of 4, >= gfrs_crc32b_encode_size(shard_len,
                          65536) */
  uint64_t reserved;   /* must be 0 */
} gfrs_ejob;

int gfrs_encode_frame_queue(gfrs_ctx *ctx, void *framed, void *base,
                            const gfrs_ejob *jobs, int njobs,
                            int64_t block_len);

/* ---- read queue (datafile.go:410-434 + stream_get.go:382-465: the degraded
 * GET over concurrent blobs - crc32block decode of every shard read, then
 * ReconstructData on the shards or on a segment of them) ----
 * Every job names the framed images of its stripe (what
 * gfrs_encode_frame_queue wrote), an erasure pattern and a segment
 * [seg_off, seg_off + seg_len) of the raw shards, and gets back that segment
 * of all n data shards - surviving ones decoded, missing ones rebuilt - and a
 * word naming the inputs whose frame CRCs did not match.  The images are read
 * once; no raw shard is materialized.  Patterns are given as for the two
 * repair queues (bad_idx / bad_off, npat + 1 offsets); jobs, bad_idx, bad_off
 * and bad_shards are host memory, out and framed device pointers.
 *
 * Read-queue contract (pinned by tests/test_gpu_read_queue.py):
 *  - Per-job result.  Row i (i < n) of job j holds bytes
 *    [seg_off, seg_off + seg_len) of data shard i: for a missing shard what
 *    crc32block decode of the surviving images followed by
 *    ReconstructData(shards, bad) yields, for a surviving shard its own
 *    decoded bytes.
 *  - Inputs.  The inputs of a job are the first n present shards among the
 *    n+m in index order (reedsolomon.go:1453-1466) - the n data shards when
 *    none of them is bad.  No other image is read; local parities are never
 *    read, and pattern entries naming them are ignored.
 *  - Verdict.  Bit i of bad_shards[j] is set exactly when shard i is an input
 *    of job j and one of its frames touched by the segment - frames
 *    floor(seg_off / 65532) through floor((seg_off + seg_len - 1) / 65532) -
 *    stores a CRC that differs from the CRC32-IEEE of its payload.  Only
 *    those frames are read, and they are read whole.  When a job's word is
 *    nonzero its declared rows are written with unspecified content; the
 *    caller adds the named shards to the pattern and resubmits
 *    (stream_get.go:413-478).  An empty pattern is a plain verified read.
 *  - Layout.  Image sources need no alignment.  out + out_off and out_stride
 *    are multiples of 4, and so is seg_off (raw positions and destination
 *    addresses stay congruent; a caller with an odd offset rounds down and
 *    skips up to 3 bytes).  framed is never written.  In out only the n
 *    declared rows of each job are written, seg_len bytes each: nothing
 *    between rows or between jobs.  Overlapping rows are a caller error (not
 *    checked).
 *  - Validation.  Everything is validated before the first launch, and any
 *    error returns its code and writes nothing:
 *      GFRS_ERR_INVALID_BLOCK for block_len <= 0 or not a multiple of 4096;
 *      GFRS_ERR_UNSUPPORTED for any other block_len != 65536, and for a
 *      tactic of more than 32 global shards (the width of a word);
 *      every pattern, used by a job or not: GFRS_ERR_INVALID_SHARDS for an
 *      index out of range or a repeated index, GFRS_ERR_TOO_FEW_SHARDS when
 *      more than m of the n+m global shards are bad;
 *      GFRS_ERR_INVALID_SHARDS for njobs <= 0, npat <= 0, a malformed
 *      bad_off, pattern outside [0, npat), reserved != 0, a misaligned
 *      seg_off, out + out_off or out_stride, out_stride < seg_len, img_stride
 *      below the image size, or seg_off + seg_len > shard_len;
 *      GFRS_ERR_SHARD_NO_DATA for shard_len == 0 or seg_len == 0.
 *  - Blocking.  The call blocks until the words are ready; it runs on the
 *    context stream, takes the context mutex once and makes one upload of one
 *    blob and one sync.
 *  - Launch bound.  A pattern is classed by R, its number of missing data
 *    shards.  It is FUSED when R <= 4 and n+m+l <= 16: each of its jobs is
 *    one work item in the bucket of its R (0..4), so a queue costs at most 5
 *    kernel launches whatever njobs and npat are.  A copy-only pattern
 *    (R = 0) of a wider tactic is IDENTITY: one item per data shard in the
 *    R = 0 bucket.  Every other pattern (R > 4, rebuilds on wider tactics) is
 *    SLOW: its jobs run one at a time after the launches - the touched
 *    frames of the inputs are decoded into a context-owned scratch stripe,
 *    the decode plan runs there and the segment is copied out: same rows and
 *    words, several launches per job.
 *  - A job of at most 4096 bytes per shard still occupies one workgroup
 *    (small jobs are not packed together). */
typedef struct gfrs_gjob {
  uint64_t img_off;    /* framed image of shard i at framed + img_off +
                          i*img_stride, i < n+m+l */
  uint64_t img_stride; /* any value >= gfrs_crc32b_encode_size(shard_len,
                          65536); sources need no alignment */
  uint64_t shard_len;  /* raw shard length, > 0, any value */
  uint64_t seg_off;    /* first raw byte wanted of every data shard; multiple
                          of 4 */
  uint64_t seg_len;    /* > 0, seg_off + seg_len <= shard_len (stream_get.go
                          shardOffset / shardReadSize) */
  uint64_t out_off;    /* bytes [seg_off, seg_off+seg_len) of data shard i,
                          i < n, at out + out_off + i*out_stride */
  uint64_t out_stride; /* multiple of 4, >= seg_len */
  int32_t pattern;     /* 0 <= pattern < npat */
  int32_t reserved;    /* must be 0 */
} gfrs_gjob;

int gfrs_read_queue(gfrs_ctx *ctx, void *out, const void *framed,
                    const gfrs_gjob *jobs, int njobs, const int32_t *bad_idx,
                    const int32_t *bad_off, int npat, int64_t block_len,
                    uint32_t *bad_shards /* njobs words */);

/* ---- shard read queue (datainspect.go:197-283 inspectChunk / inspectShard,
 * shards_decoder.go:48-295 batch read, datafile.go:410-445 + chunk.go:448-589
 * shard GET: the loop over the bids of one chunk, in the read direction) ----
 * gfrs_shard_parse_batch and gfrs_crc32b_decode as a queue over disk images
 * of different sizes lying anywhere in one chunk: every job names one image
 * (what gfrs_shard_write_batch / gfrs_repair_queue wrote), what the shard meta
 * says its header must hold, and a range [from, to) of the raw shard.  It gets
 * back a word of independent status bits, the first bad frame, the header
 * fields as stored and - unless it carries GFRS_SJOB_NO_OUT, the inspect
 * form - the range with the frame CRCs stripped.  GFRS_SJOB_FOOTER adds the
 * footer check of a whole shard.  jobs and results are host memory, chunk and
 * out device pointers; out may be NULL when every job carries NO_OUT.
 *
 * Shard-read-queue contract (pinned by tests/test_gpu_shard_read_queue.py):
 *  - Per-job result.  The status bits are independent facts about the image
 *    bytes, each set exactly when its fact holds (the cgo shim picks the
 *    reference's precedence):
 *      HDR_MAGIC     bytes 4..8 are not ab cd ef cc;
 *      HDR_CRC       the big-endian word at 0 differs from the CRC32-IEEE of
 *                    bytes 4..32;
 *      HDR_MISMATCH  the stored bid, vuid or size differs from the job's;
 *      BODY_CRC      a touched frame - from / 65532 through (to - 1) / 65532 -
 *                    stores a CRC that differs from the CRC32-IEEE of its
 *                    payload;
 *      FTR_MAGIC     FOOTER jobs only: the footer magic is not cc ef cd ab;
 *      FTR_CRC       FOOTER jobs only: the footer's big-endian CRC differs
 *                    from `crc`.
 *    bad_block is the lowest touched frame (index within the image) with a
 *    CRC mismatch, or -1, as in gfrs_shard_parse_batch.  crc is computed from
 *    the payload bytes that were read, not folded from the stored frame
 *    words, so FTR_CRC is the comparison of compact.go:263.  Geometry follows
 *    the job's size, never the header's (the reference reads by the meta's
 *    size too).  For a job with from = 0, to = size and FOOTER, status == 0
 *    exactly when gfrs_shard_parse_batch on that image alone reports err == 0
 *    and the job's ids, and bad_block is that call's answer.
 *  - Output.  A job without NO_OUT gets bytes [from, to) of the image's
 *    payload at out + out_off, whatever its status: what was loaded is what
 *    is stored.  A job with NO_OUT writes nothing and costs no store.
 *  - Layout.  Sources need no alignment.  Only touched frames are read, and
 *    they are read whole; the 32-byte header is always read, the 8-byte
 *    footer only for FOOTER jobs.  chunk is never written.  out + out_off and
 *    from are multiples of 4 (raw positions and destination addresses stay
 *    congruent).  In out only the declared to - from bytes of each job are
 *    written.  Overlapping outputs are a caller error (not checked).
 *  - Validation.  Everything is validated before the first launch, and any
 *    error returns its code and writes nothing, neither in out nor in
 *    results:
 *      GFRS_ERR_INVALID_BLOCK for block_len <= 0 or not a multiple of 4096;
 *      GFRS_ERR_UNSUPPORTED for any other block_len != 65536;
 *      GFRS_ERR_SHARD_NO_DATA for size == 0;
 *      GFRS_ERR_INVALID_SHARDS for njobs <= 0, size >= 2^32, reserved != 0,
 *      unknown flag bits, from >= to, to > size, from % 4 != 0, FOOTER with
 *      from != 0 or to != size, and on a job without NO_OUT a misaligned
 *      out + out_off or out == NULL.
 *  - Blocking.  The call blocks until the results are ready; it runs on the
 *    context stream, takes the context mutex once and makes one upload of one
 *    blob, one read-back and one sync.  It obeys the ordering contract above:
 *    its upload waits out an id upload that an async gfrs_shard_write_batch
 *    left queued.
 *  - Launch bound.  At most 3 kernel launches whatever njobs is: the storing
 *    jobs, the NO_OUT jobs, and one launch of one wave per job that parses
 *    the headers and footers and writes the results.
 *  - A job of at most 4096 bytes still occupies one workgroup (small jobs are
 *    not packed together); the footer CRC of a FOOTER job is folded serially
 *    over its frames. */
enum { GFRS_SJOB_NO_OUT = 1, GFRS_SJOB_FOOTER = 2 };
enum {
  GFRS_SHARD_HDR_MAGIC = 1,    /* core.ErrShardHeaderMagic */
  GFRS_SHARD_HDR_CRC = 2,      /* core.ErrShardHeaderCrc */
  GFRS_SHARD_HDR_MISMATCH = 4, /* core.ErrShardHeaderNotMatch */
  GFRS_SHARD_BODY_CRC = 8,     /* crc32block.ErrMismatchedCrc */
  GFRS_SHARD_FTR_MAGIC = 16,
  GFRS_SHARD_FTR_CRC = 32,
};

typedef struct gfrs_sjob {
  uint64_t img_off;  /* image at chunk + img_off; no alignment needed */
  uint64_t size;     /* raw shard size from the shard meta, 1 .. 2^32-1 */
  uint64_t bid, vuid;/* what the meta says the header must hold */
  uint64_t from, to; /* raw bytes [from, to) wanted; from % 4 == 0,
                        from < to <= size */
  uint64_t out_off;  /* those bytes at out + out_off (multiple of 4); ignored
                        with NO_OUT */
  uint32_t flags;    /* GFRS_SJOB_* */
  uint32_t reserved; /* must be 0 */
} gfrs_sjob;

typedef struct gfrs_sresult {
  uint32_t status;   /* OR of GFRS_SHARD_*; 0 = clean */
  uint32_t crc;      /* FOOTER jobs: CRC32-IEEE of the size payload bytes in
                        the image; else 0 */
  int64_t bad_block; /* lowest touched frame (index within the image) whose
                        CRC differs, or -1 */
  uint64_t bid, vuid, size; /* header fields as stored, whatever the status */
} gfrs_sresult;

int gfrs_shard_read_queue(gfrs_ctx *ctx, void *out, const void *chunk,
                          const gfrs_sjob *jobs, int njobs, int64_t block_len,
                          gfrs_sresult *results /* njobs, host */);

/* ---- shard write queue (datafile.go:342-384 Write: the loop over the bids
 * of a batch of PUTs; compact.go:236-344 doCompact: the loop over the bids of
 * the chunk being compacted) ----
 * gfrs_shard_write_batch as a queue over shards of different sizes: every job
 * names a payload - raw bytes, or with GFRS_WJOB_SRC_IMAGE the payload of an
 * existing disk image - the ids of the new header and the place of the new
 * image.  The payload is read once, its frame CRCs are computed from the bytes
 * that were read, and the new image is written; a SRC_IMAGE job also gets the
 * answer gfrs_shard_read_queue would give about its source.  Every job gets
 * back the CRC32-IEEE of its payload, the shard meta's Crc.  jobs and results
 * are host memory, src and dst device pointers.
 *
 * Shard-write-queue contract (pinned by tests/test_gpu_shard_write_queue.py):
 *  - Per-job image.  The gfrs_shard_disk_size(size, 65536) bytes at
 *    dst + img_off are byte-identical to the reference's shard write of the
 *    job's payload with the job's bid and vuid: header, freshly computed frame
 *    CRCs, payload, footer.  The payload of a raw job is
 *    src[src_off, src_off + size); that of a SRC_IMAGE job the payload bytes
 *    of the source image as stored, whatever the job's status - geometry
 *    follows the job's size, never the source header's; what was loaded is
 *    what is stored.  The new image is always self-consistent; on
 *    status != 0 the caller drops it, as the reference fails the compaction of
 *    that bid.  A raw job alone writes the bytes of gfrs_shard_write_batch
 *    with nshards = 1.
 *  - Per-job result.  crc is the CRC32-IEEE of the size payload bytes written
 *    (shard.Crc of datafile.go:379, the footer's value).  A raw job reports
 *    status = 0, bad_block = -1 and bid, vuid, size as its own.  A SRC_IMAGE
 *    job reports exactly what a gfrs_shard_read_queue job with from = 0,
 *    to = size, GFRS_SJOB_FOOTER, bid = src_bid and vuid = src_vuid reports on
 *    the source image: the six independent status bits, bad_block, crc and the
 *    header fields as stored.
 *  - Layout.  Sources need no alignment; src is never written.  dst + img_off
 *    is a multiple of 4.  In dst only the declared images are written: nothing
 *    between them, nothing past an image's disk size.  Only the job's source
 *    bytes are read: for SRC_IMAGE the 32-byte header, every frame whole and
 *    the 8-byte footer; for a raw job its size bytes.  Overlapping images, or
 *    src overlapping dst, are caller errors (not checked).
 *  - Validation.  Everything is validated before the first launch, and any
 *    error returns its code and writes nothing, neither in dst nor in
 *    results:
 *      GFRS_ERR_INVALID_BLOCK for block_len <= 0 or not a multiple of 4096;
 *      GFRS_ERR_UNSUPPORTED for any other block_len != 65536;
 *      GFRS_ERR_SHARD_NO_DATA for size == 0;
 *      GFRS_ERR_INVALID_SHARDS for njobs <= 0, size >= 2^32, reserved != 0,
 *      unknown flag bits, or a misaligned dst + img_off.
 *  - Blocking.  The call blocks until the results are ready; it runs on the
 *    context stream, takes the context mutex once and makes one upload of one
 *    blob, one read-back and one sync.  It obeys the ordering contract above:
 *    its upload waits out an id upload that an async gfrs_shard_write_batch
 *    left queued.
 *  - Launch bound.  At most 3 kernel launches whatever njobs is: the raw
 *    jobs, the SRC_IMAGE jobs, and one launch of one wave per job that writes
 *    the new header and footer, checks the source header and footer of a
 *    SRC_IMAGE job and writes the results.
 *  - A job of at most 4096 bytes still occupies one workgroup (small jobs are
 *    not packed together); the footer CRC is folded serially over the job's
 *    frames. */
enum { GFRS_WJOB_SRC_IMAGE = 1 };

typedef struct gfrs_wjob {
  uint64_t src_off;   /* raw shard (size bytes) at src + src_off; with
                         SRC_IMAGE a disk image there; no alignment */
  uint64_t size;      /* raw shard size, 1 .. 2^32-1 */
  uint64_t bid, vuid; /* written into the new header */
  uint64_t src_bid, src_vuid; /* SRC_IMAGE: what the source header must hold
                                 (with size); ignored otherwise */
  uint64_t img_off;   /* new image at dst + img_off; multiple of 4 */
  uint32_t flags;     /* GFRS_WJOB_* */
  uint32_t reserved;  /* must be 0 */
} gfrs_wjob;

int gfrs_shard_write_queue(gfrs_ctx *ctx, void *dst, const void *src,
                           const gfrs_wjob *jobs, int njobs, int64_t block_len,
                           gfrs_sresult *results /* njobs, host */);

/* ---- put queue (stream_put.go:146 + datafile.go:342-384: the PUT path from
 * the blob's data shards to what blobnode writes, over concurrent blobs of
 * different sizes) ----
 * gfrs_encode_frame_queue and gfrs_shard_write_queue in one pass, for every
 * tactic up to n = 32: every job names its n data shards, the place of its
 * n+m+l disk images, a bid and a vuid set, and gets back the images - header,
 * crc32block body, footer - and the CRC32-IEEE of every raw shard, the shard
 * meta's Crc.  jobs, vuids and crcs are host memory, base and disk_dst device
 * pointers.
 *
 * Put-queue contract (pinned by tests/test_gpu_put_queue.py):
 *  - Per-job result.  Image i of job j (at disk_dst + img_off + i*img_stride,
 *    gfrs_shard_disk_size(shard_len, 65536) bytes) is byte-identical to the
 *    reference's shard write of shard i of the job's encoded stripe - the
 *    reference's Encode of the n data shards, local parities included - with
 *    bid, vuids[vol*(n+m+l) + i] and size = shard_len: header, freshly
 *    computed frame CRCs, payload, footer.  crcs[j*(n+m+l) + i] is the
 *    CRC32-IEEE of that raw shard (shard.Crc of datafile.go:379, the footer's
 *    value).
 *  - Layout.  Sources need no alignment.  disk_dst + img_off and img_stride
 *    are multiples of 4.  In disk_dst only the declared images are written:
 *    nothing between images, nothing past an image's disk size.  base is never
 *    written, for any tactic (gfrs_encode_frame_queue writes the parity there
 *    on its slow tactics; this call has none).  Only the n data shards of each
 *    job are read: the m+l parity places of the ec.Buffer layout need not
 *    exist behind them.  Overlapping images, or base overlapping disk_dst, are
 *    caller errors (not checked).
 *  - Validation.  Everything is validated before the first launch, and any
 *    error returns its code and writes nothing, neither in disk_dst nor in
 *    crcs:
 *      GFRS_ERR_INVALID_BLOCK for block_len <= 0 or not a multiple of 4096;
 *      GFRS_ERR_UNSUPPORTED for any other block_len != 65536, for m == 0 and
 *      for n > 32;
 *      GFRS_ERR_SHARD_NO_DATA for shard_len == 0;
 *      GFRS_ERR_INVALID_SHARDS for njobs <= 0, nvol <= 0, vol out of range,
 *      reserved != 0, shard_len >= 2^32, a misaligned disk_dst + img_off or
 *      img_stride, or img_stride below the disk size.
 *  - Blocking.  The call blocks until the images and crcs are ready; it runs
 *    on the context stream, takes the context mutex once and makes one upload
 *    of one blob, one read-back (none when crcs is NULL) and one sync.  (The
 *    first call of an LRC context outside the gate below also uploads its
 *    composed plan once.)  It obeys the ordering contract above: its upload
 *    waits out an id upload that an async gfrs_shard_write_batch left queued.
 *  - Launch bound.  The m+l parity rows run in G = ceil((m+l)/4) row groups
 *    of 4 rows (the last one of the rest).  A tactic inside the gate of
 *    gfrs_encode_frame_batch (G = 1, n+m+l <= 16) costs at most 6 + 1
 *    launches: the buckets of gfrs_encode_frame_queue, then one launch of one
 *    wave per image that writes header and footer and the crc.  Every other
 *    tactic costs at most 2*G + 1: per row group the two frame variants (below
 *    1 MiB per shard / from 1 MiB up); group 0 stores the data frames, a later
 *    group reads the data again and stores its parity frames only.
 *  - Limits.  On a tactic outside that gate a job of at most 4096 bytes runs
 *    the frame kernel, one workgroup per job per group: it is not packed into
 *    a wave.  The footer CRC is folded serially over the image's frames. */
typedef struct gfrs_pjob {
  uint64_t off;        /* data shard i at base + off + i*shard_len, i < n; no
                          alignment */
  uint64_t shard_len;  /* 1 .. 2^32-1 */
  uint64_t img_off;    /* disk image of shard i at
                          disk_dst + img_off + i*img_stride, i < n+m+l */
  uint64_t img_stride; /* multiple of 4, >= gfrs_shard_disk_size(shard_len,
                          65536) */
  uint64_t bid;        /* written into all n+m+l headers of the job */
  int32_t vol;         /* 0 <= vol < nvol: header of shard i carries
                          vuids[vol*(n+m+l) + i] */
  int32_t reserved;    /* must be 0 */
} gfrs_pjob;

int gfrs_put_queue(gfrs_ctx *ctx, void *disk_dst, const void *base,
                   const gfrs_pjob *jobs, int njobs, const uint64_t *vuids,
                   int nvol, int64_t block_len,
                   uint32_t *crcs /* njobs*(n+m+l), host, may be NULL */);

/* ---- ec.Buffer size math (buf.go:67-133) ---- */
int gfrs_buffer_sizes(const gfrs_tactic *t, int64_t data_size,
                      int64_t *shard_size, int64_t *ec_data_size,
                      int64_t *ec_size);

/* ---- introspection for tests ---- */
/* Copy the (n+m)×n encode matrix into out (row-major). */
int gfrs_encode_matrix(gfrs_ctx *ctx, uint8_t *out);
/* GPU-free: compute the klauspost default encode matrix (total×k) so CPU
 * tests can pin the host math without a device. */
int gfrs_compute_encode_matrix(int k, int total, uint8_t *out);
/* GPU-free: build the coding plan the engine would upload for one bad list,
 * with the same builder functions, so CPU tests can check every erasure
 * pattern without a device.  For each r < *nout,
 *   shard out[r] = XOR_c rows[r * *rowk + c] * shard in[c];
 * bit r of *cmp_mask marks a row the kernel compares instead of writing.
 * `in` and `out` hold `cap` entries, `rows` cap * n bytes (GFRS_ERR_NOMEM
 * when the plan is larger).  `bad` is ignored for the encode kind.
 * Returns the builder's error code. */
enum {
  GFRS_PLAN_FUSED_LRC_ENCODE = 0,       /* gfrs_encode_frame_batch, LRC */
  GFRS_PLAN_RS_RECONSTRUCT_VERIFY = 1,  /* gfrs_reconstruct_verify_batch */
  GFRS_PLAN_LRC_RECONSTRUCT_VERIFY = 2, /* the same, LRC single pass */
  GFRS_PLAN_FUSED_REPAIR = 3,           /* gfrs_repair_batch, fused kernel */
  GFRS_PLAN_READ = 4,                   /* gfrs_read_queue: `in` = the first n
                                           present of the n+m shards, `out` =
                                           the missing data shards ascending
                                           (all write rows); *colpack returns
                                           the pass-through set, bit c = in[c]
                                           is a data shard */
};
int gfrs_compute_plan(const gfrs_tactic *t, int kind, const int32_t *bad,
                      int nbad, int cap, int32_t *in, int *nin, int32_t *out,
                      int *nout, uint8_t *rows, int *rowk, uint32_t *cmp_mask,
                      uint32_t *colpack);
/* GPU-free: the launch schedule gfrs_reconstruct_verify_queue would build
 * for a queue, with the same builder, so CPU tests can check it without a
 * device.  A job whose pattern has nout plan rows runs ceil(nout/4) steps;
 * all (job, step) pairs with the same step index g and row count gm form one
 * bucket = one kernel launch.  Bucket b owns items[first, first+count),
 * ordered by pattern, and the count+1 exclusive prefix sums of
 * ceil(shard_len/4096) at tile_prefix[first + b ...].  pat_nout / pat_slow
 * have npat entries, slow_jobs njobs; items holds item_cap entries,
 * tile_prefix item_cap + bucket_cap, buckets bucket_cap (GFRS_ERR_NOMEM when
 * the schedule is larger).  Returns the validation codes of the queue call. */
typedef struct gfrs_qitem {
  uint64_t off, shard_len; /* of the job */
  int32_t job;             /* caller's index */
  int32_t pattern;
  int32_t row_off;         /* first plan row of this step, 4*g */
  int32_t reserved;
} gfrs_qitem;
typedef struct gfrs_qbucket {
  int32_t g, gm, first, count;
} gfrs_qbucket;
int gfrs_compute_queue_schedule(const gfrs_tactic *t, const gfrs_qjob *jobs,
                                int njobs, const int32_t *bad_idx,
                                const int32_t *bad_off, int npat,
                                int item_cap, int bucket_cap,
                                gfrs_qitem *items, uint64_t *tile_prefix,
                                int *nitems, gfrs_qbucket *buckets,
                                int *nbuckets, int32_t *pat_nout,
                                uint8_t *pat_slow, int32_t *slow_jobs,
                                int *nslow);
/* GPU-free: what gfrs_repair_queue would upload for a queue, with the same
 * builder, so CPU tests can check it without a device.
 *   Pattern class: GFRS_RPAT_FUSED patterns run the fused frame kernel over
 *   their plan (pat_gm rows of which pat_nw rebuild, pat_colpack nibble r =
 *   the caller's image column of rebuild row r); the others are reconstructed
 *   in base first (GFRS_RPAT_INPLACE_SLOW: one job at a time) and their jobs
 *   are listed in inplace_jobs, caller order.
 *   Work items: a fused job is one item of its pattern's descriptor (desc =
 *   pattern index) in the bucket of pat_gm rows; an in-place job is one
 *   identity item per bad shard s (desc = npat + s: k = 1, coefficient 1,
 *   one rebuild row, input s) in the 1-row bucket, img pointing at that
 *   shard's own image.  At most one bucket per row count, ascending; bucket
 *   b owns items[first, first+count), ordered by descriptor, then by caller
 *   index, and the count+1 exclusive prefix sums of ceil(shard_len / 65532)
 *   at frame_prefix[first + b ...].
 *   Image table: one entry per image in id order (job-major, the pattern's
 *   own order): byte offset in disk_dst, raw size, bid, vuid.
 * items holds item_cap entries, frame_prefix item_cap + 4, buckets 4, images
 * image_cap, pat_* npat, inplace_jobs njobs (GFRS_ERR_NOMEM when the
 * schedule is larger).  bids / vuids may be NULL (zeros).  Returns the
 * validation codes of gfrs_repair_queue, taking disk_dst as 4-aligned. */
enum { GFRS_RPAT_FUSED = 0, GFRS_RPAT_INPLACE = 1, GFRS_RPAT_INPLACE_SLOW = 2 };
typedef struct gfrs_ritem {
  uint64_t off, shard_len; /* of the job */
  uint64_t img;            /* byte offset in disk_dst of image column 0 */
  uint64_t img_stride;     /* between the item's image columns */
  int32_t job;             /* caller's index */
  int32_t desc;            /* descriptor index */
} gfrs_ritem;
typedef struct gfrs_rbucket {
  int32_t gm, first, count, reserved;
} gfrs_rbucket;
typedef struct gfrs_rimage {
  uint64_t off, size, bid, vuid;
} gfrs_rimage;
int gfrs_compute_repair_queue_schedule(
    const gfrs_tactic *t, const gfrs_rjob *jobs, int njobs,
    const int32_t *bad_idx, const int32_t *bad_off, int npat,
    int64_t block_len, const uint64_t *bids, const uint64_t *vuids,
    int item_cap, int image_cap, gfrs_ritem *items, uint64_t *frame_prefix,
    int *nitems, gfrs_rbucket *buckets, int *nbuckets, gfrs_rimage *images,
    int *nimages, int32_t *pat_class, int32_t *pat_gm, int32_t *pat_nw,
    uint32_t *pat_colpack, int32_t *inplace_jobs, int *ninplace);
/* GPU-free: what gfrs_encode_frame_queue would upload for a queue, with the
 * same builder, so CPU tests can check it without a device.
 *   Job classes: a job of at most 4096 bytes per shard is SMALL and runs one
 *   wave (param = NI = ceil(shard_len / 1024), 1..4: one bucket per NI); a
 *   longer job is a FRAME job and runs one workgroup per 64 KiB frame (param =
 *   the batch launcher's variant for its length: 87 - 4 waves, nontemporal
 *   stores - below 1 MiB per shard, 76 - 3 waves, plain stores - from 1 MiB).
 *   Buckets: at most 6, in the fixed order small NI ascending, then frame 87,
 *   then frame 76; bucket b owns items[first, first+count), in caller order.
 *   Prefix sums: only frame buckets have them.  The q-th frame bucket (q = 0
 *   or 1) owns the count+1 exclusive prefix sums of ceil(shard_len / 65532) at
 *   frame_prefix[first - nsmall + q ...], nsmall being the number of small
 *   items (all of which precede the frame items).
 * *fused tells whether the tactic passes the gate of the fused kernels; when
 * it is 0 the engine ignores the schedule and runs the jobs one at a time.
 * items holds item_cap entries, frame_prefix item_cap + 2, buckets 6
 * (GFRS_ERR_NOMEM when the schedule is larger).  Returns the validation codes
 * of gfrs_encode_frame_queue, taking framed as 4-aligned. */
enum { GFRS_EQ_SMALL = 0, GFRS_EQ_FRAME = 1 };
typedef struct gfrs_eitem {
  uint64_t off, shard_len; /* of the job */
  uint64_t img;            /* byte offset in framed of the image of shard 0 */
  uint64_t img_stride;     /* between the job's images */
  int32_t job;             /* caller's index */
  int32_t reserved;
} gfrs_eitem;
typedef struct gfrs_ebucket {
  int32_t kind, param, first, count;
} gfrs_ebucket;
int gfrs_compute_encode_queue_schedule(const gfrs_tactic *t,
                                       const gfrs_ejob *jobs, int njobs,
                                       int64_t block_len, int item_cap,
                                       gfrs_eitem *items,
                                       uint64_t *frame_prefix, int *nitems,
                                       gfrs_ebucket *buckets, int *nbuckets,
                                       int *fused);
/* GPU-free: what gfrs_read_queue would upload for a queue, with the same
 * builder, so CPU tests can check it without a device.
 *   Pattern class: GFRS_GPAT_FUSED patterns (pat_r = R missing data shards,
 *   0..4) run the fused read kernel over their plan; GFRS_GPAT_IDENTITY ones
 *   (R = 0 on a tactic wider than 16 shards) run it shard by shard;
 *   GFRS_GPAT_SLOW ones run one job at a time and are listed in slow_jobs,
 *   caller order.
 *   Work items: a fused job is one item of its pattern's descriptor (desc =
 *   pattern index) in the bucket of its R; an identity job is one item per
 *   data shard s (desc = npat + s: k = 1, one pass-through input s) in the
 *   R = 0 bucket.  At most one bucket per R, ascending; bucket b owns
 *   items[first, first+count), ordered by descriptor, then by caller index,
 *   and the count+1 exclusive prefix sums of the TOUCHED frames of its items -
 *   floor((seg_off + seg_len - 1) / 65532) - floor(seg_off / 65532) + 1, not
 *   ceil(shard_len / 65532) - at frame_prefix[first + b ...].
 * items holds item_cap entries, frame_prefix item_cap + 5, buckets 5, pat_*
 * npat, slow_jobs njobs (GFRS_ERR_NOMEM when the schedule is larger).  Returns
 * the validation codes of gfrs_read_queue, taking out as 4-aligned. */
enum { GFRS_GPAT_FUSED = 0, GFRS_GPAT_IDENTITY = 1, GFRS_GPAT_SLOW = 2 };
typedef struct gfrs_gitem {
  uint64_t img;        /* byte offset in framed of the image of shard 0 */
  uint64_t img_stride; /* between the job's images */
  uint64_t shard_len;
  uint64_t seg_off, seg_len;
  uint64_t out;        /* byte offset in out of row 0 */
  uint64_t out_stride; /* between the job's rows */
  int32_t job;         /* caller's index */
  int32_t desc;        /* descriptor index */
} gfrs_gitem;
typedef struct gfrs_gbucket {
  int32_t r, first, count, reserved;
} gfrs_gbucket;
int gfrs_compute_read_queue_schedule(
    const gfrs_tactic *t, const gfrs_gjob *jobs, int njobs,
    const int32_t *bad_idx, const int32_t *bad_off, int npat,
    int64_t block_len, int item_cap, gfrs_gitem *items,
    uint64_t *frame_prefix, int *nitems, gfrs_gbucket *buckets, int *nbuckets,
    int32_t *pat_class, int32_t *pat_r, int32_t *slow_jobs, int *nslow);
/* GPU-free: what gfrs_shard_read_queue would upload for a queue, with the same
 * builder, so CPU tests can check it without a device.
 *   Work items: one per job.  At most two buckets, in the fixed order storing
 *   jobs (no_out = 0), then NO_OUT jobs (no_out = 1); bucket b owns
 *   items[first, first+count), in caller order, and the count+1 exclusive
 *   prefix sums of the TOUCHED frames of its items -
 *   floor((to - 1) / 65532) - floor(from / 65532) + 1 - at
 *   frame_prefix[first + b ...].
 *   *total_frames is the sum over both buckets: the number of computed frame
 *   CRCs the engine keeps in scratch (the storing bucket's first, then the
 *   NO_OUT bucket's, each in walk order).
 * items holds item_cap entries, frame_prefix item_cap + 2, buckets 2
 * (GFRS_ERR_NOMEM when the schedule is larger).  Returns the validation codes
 * of gfrs_shard_read_queue, taking out as 4-aligned and not NULL. */
typedef struct gfrs_sitem {
  uint64_t img;      /* byte offset in chunk of the image */
  uint64_t size;     /* raw shard size */
  uint64_t from, to;
  uint64_t out;      /* byte offset in out of byte `from` */
  int32_t job;       /* caller's index */
  uint32_t flags;    /* of the job */
} gfrs_sitem;
typedef struct gfrs_sbucket {
  int32_t no_out, first, count, reserved;
} gfrs_sbucket;
int gfrs_compute_shard_read_queue_schedule(
    const gfrs_sjob *jobs, int njobs, int64_t block_len, int item_cap,
    gfrs_sitem *items, uint64_t *frame_prefix, int *nitems,
    gfrs_sbucket *buckets, int *nbuckets, uint64_t *total_frames);
/* GPU-free: what gfrs_shard_write_queue would upload for a queue, with the
 * same builder, so CPU tests can check it without a device.
 *   Work items: one per job.  At most two buckets, in the fixed order raw
 *   jobs (src_image = 0), then SRC_IMAGE jobs (src_image = 1); bucket b owns
 *   items[first, first+count), in caller order, and the count+1 exclusive
 *   prefix sums of the frames of its items - ceil(size / 65532) - at
 *   frame_prefix[first + b ...].
 *   *total_frames is the sum over both buckets: the number of computed frame
 *   CRCs the engine keeps in scratch (the raw bucket's first, then the
 *   SRC_IMAGE bucket's, each in walk order).
 * items holds item_cap entries, frame_prefix item_cap + 2, buckets 2
 * (GFRS_ERR_NOMEM when the schedule is larger).  Returns the validation codes
 * of gfrs_shard_write_queue, taking dst as 4-aligned. */
typedef struct gfrs_witem {
  uint64_t src;      /* byte offset in src of the raw shard or source image */
  uint64_t size;     /* raw shard size */
  uint64_t img;      /* byte offset in dst of the new image */
  int32_t job;       /* caller's index */
  uint32_t flags;    /* of the job */
} gfrs_witem;
typedef struct gfrs_wbucket {
  int32_t src_image, first, count, reserved;
} gfrs_wbucket;
int gfrs_compute_shard_write_queue_schedule(
    const gfrs_wjob *jobs, int njobs, int64_t block_len, int item_cap,
    gfrs_witem *items, uint64_t *frame_prefix, int *nitems,
    gfrs_wbucket *buckets, int *nbuckets, uint64_t *total_frames);
/* GPU-free: what gfrs_put_queue would upload for a queue, with the same
 * builder, so CPU tests can check it without a device.
 *   Work items: one gfrs_eitem per job, img = img_off + 32 - the body starts
 *   behind the header, so the frame kernels see an ordinary 4-aligned image
 *   row.  *wide = 0: the tactic passes the gate of the fused encode kernels
 *   and the buckets are those of gfrs_compute_encode_queue_schedule.
 *   *wide = 1: only the two frame buckets exist (87 below 1 MiB per shard, 76
 *   from it up), every job in one of them by its length, and the engine
 *   launches each once per row group.  Prefix sums as in the encode queue.
 *   Row groups: *ngroups = ceil((m+l)/4); group g carries group_rows[g] rows
 *   from parity row 4*g on: 4, the last one (m+l) - 4*(*ngroups - 1).
 *   Image table: one entry per image, job-major and in shard order within a
 *   job: byte offset in disk_dst, raw size, bid, vuids[vol*(n+m+l) + i].
 * items holds item_cap entries, frame_prefix item_cap + 2, buckets 6, images
 * image_cap, group_rows ceil((m+l)/4) (GFRS_ERR_NOMEM when the schedule is
 * larger).  Returns GFRS_ERR_INVALID_CODEMODE for an invalid tactic, else the
 * validation codes of gfrs_put_queue, taking disk_dst as 4-aligned. */
int gfrs_compute_put_queue_schedule(
    const gfrs_tactic *t, const gfrs_pjob *jobs, int njobs,
    const uint64_t *vuids, int nvol, int64_t block_len, int item_cap,
    int image_cap, gfrs_eitem *items, uint64_t *frame_prefix, int *nitems,
    gfrs_ebucket *buckets, int *nbuckets, gfrs_rimage *images, int *nimages,
    int *wide, int *ngroups, int32_t *group_rows);
/* Device probe used by tests: returns 1 when v_perm byte-select semantics
 * match the kernel's assumption (sel>=8 yields 0), 0 otherwise, <0 error. */
int gfrs_probe_perm(void);

#ifdef __cplusplus
}
#endif
#endif /* GFRS_H */
