/* cubefs_amd/csrc/gfrs_plan.h — GF(2^8) math and coding-plan construction.
 *
 * Plain host C++ with no device dependency: everything that decides which
 * coefficients multiply which shards lives here, so it can be built and
 * checked by a host compiler alone (tests/plan_selftest.cpp,
 * tests/test_plan_cpu.py through gfrs_compute_plan).  gfrs_host.cpp uploads
 * the plans and launches kernels; it holds no algebra.
 */
#ifndef GFRS_PLAN_H
#define GFRS_PLAN_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/gfrs.h"

namespace gfrs {

/* ---- GF(2^8) field, poly 0x11D (generator 29; galois.go:25) ---- */
struct GfTables {
  uint8_t log_t[256];
  uint8_t exp_t[510];
  uint8_t mul[256][256];
  /* nibble tables: lo[c][x] = mul[c][x], hi[c][x] = mul[c][x<<4]
   * (galois.go:340,596) */
  uint8_t lo[256][16];
  uint8_t hi[256][16];
  GfTables();
  uint8_t gexp(uint8_t a, int n) const; /* galois.go:892 */
  uint8_t div(uint8_t a, uint8_t b) const;
};
const GfTables &gft();

/* Row-major byte matrix helpers (matrix.go). */
bool gf_invert(const uint8_t *in, int n, uint8_t *out); /* false = singular */
/* klauspost default encode matrix: vandermonde(total,k) × inv(top k×k)
 * (reedsolomon.go:220-244).  out is total×k; its top k×k is the identity. */
bool gf_build_matrix(int k, int total, uint8_t *out);

/* ---- the code: what the plan builders need to know of a context ---- */
struct Code {
  gfrs_tactic t{};
  int total = 0;   /* n+m+l */
  int local_n = 0; /* (n+m)/az when l>0 */
  int local_m = 0; /* l/az */
  std::vector<uint8_t> enc_matrix;   /* (n+m)×n */
  std::vector<uint8_t> local_matrix; /* (local_n+local_m)×local_n */
};
bool tactic_valid(const gfrs_tactic *t);   /* codemode.go:291-299 */
bool code_build(const gfrs_tactic &t, Code *c); /* false = singular */
/* local stripe global indices for one AZ (codemode.go:301-318) */
std::vector<int32_t> local_stripe(const gfrs_tactic &t, int az_idx);

/* One RS engine inside the code: its matrix ((k+m)×k) and the global shard
 * slot of each of its k+m shards.  The global engine and the per-AZ local
 * engines differ only in these. */
struct Engine {
  int k, m;
  const uint8_t *matrix;
  const int32_t *idx;
};

/* ---- a plan before upload ----
 * For every output row r:  shard out[r] = XOR_c rows[r*rowk+c] * shard in[c].
 * Conventions shared by every builder:
 *   - decoding inputs are the first k present shards of the engine in index
 *     order (reedsolomon.go:1453-1466);
 *   - write rows come first, compare rows after them; cmp_mask has bit r
 *     set when row r is compared against the stored shard, not written;
 *   - `in` may carry more than rowk entries: the fused repair kernel finds
 *     the stored shard of its r-th check row at in[rowk + r'];
 *   - the fused repair kernel carries 4 rows in all (rebuild + check). */
struct Plan {
  std::vector<int32_t> in, out;
  std::vector<uint8_t> rows; /* out.size() × rowk */
  int rowk = 0;
  uint32_t cmp_mask = 0;
  uint32_t colpack = 0; /* fused repair: nibble r = caller's image column
                           of the r-th rebuild row */
  uint32_t pass_mask = 0; /* read plan: bit c = in[c] is a data shard, which
                             the read kernel passes through to row in[c] */
};

/* Every builder returns GFRS_OK or an error code and leaves *p complete.
 * `present` covers the engine's k+m shards. */

/* missing data shards of one engine from its first k present shards */
int plan_decode(const Engine &e, const uint8_t *present, Plan *p);
/* missing parity shards of one engine from its k data shards; an empty
 * `out` means there is nothing to do */
int plan_parity(const Engine &e, const uint8_t *present, Plan *p);
/* EncodeIdx accumulate: input slot 0, the m global parities at 1..m */
int plan_encode_idx(const Code &c, int idx, Plan *p);
/* all m global then all l local parities (az-major) as rows over the n
 * data shards */
int plan_fused_lrc(const Code &c, Plan *p);
/* plain RS reconstruct+verify: missing data ascending, then ALL m parity
 * rows; present parities are compared.  Duplicates in bad are tolerated. */
int plan_rs_reconstruct_verify(const Code &c, const int32_t *bad, int nbad,
                               Plan *p);
/* LRC reconstruct+verify: bad shards in caller order, then the check rows:
 * surviving global parities that are not inputs, surviving local parities.
 * GFRS_ERR_UNSUPPORTED when the bad set is not globally decodable or needs
 * more than 32 rows (the caller falls back to two passes). */
int plan_lrc_reconstruct_verify(const Code &c, const int32_t *bad, int nbad,
                                Plan *p);
/* fused repair: bad shards ascending, then the same check rows while the
 * 4-row budget lasts */
int plan_fused_repair(const Code &c, const int32_t *bad, int nbad, Plan *p);
/* the colpack of plan_fused_repair alone (it depends on the caller's order,
 * which a cached plan does not know); also its bad-list validation */
int repair_colpack(int total, const int32_t *bad, int nbad, uint32_t *colpack);

/* whether the LRC entry points take the composed single-pass plans for this
 * code (the row and width budget of the fused kernels) */
bool lrc_single_pass(const Code &c);

/* ---- the repair queue (gfrs_reconstruct_verify_queue) ----
 * Besides "which coefficients multiply which shards" the plan module decides
 * "which job runs in which launch".  A job whose pattern has nout rows needs
 * ceil(nout / QUEUE_ROWS) steps; step g carries gm = 1..QUEUE_ROWS rows at
 * row offset QUEUE_ROWS * g.  All (job, step) pairs with the same (g, gm)
 * form one bucket = one launch of the gm-row queue kernel, so a queue costs
 * at most QUEUE_ROWS * ceil(max_nout / QUEUE_ROWS) launches whatever njobs
 * and npat are.  Buckets are ordered by ascending g, then gm. */
constexpr int QUEUE_ROWS = 4;        /* rows per launch (the kernels' MT) */
constexpr uint64_t QUEUE_TILE = 4096; /* bytes of one shard per block step
                                         (the kernels' RS_TILE) */

struct QueuePattern {
  int nout = 0;      /* rows of the pattern's plan (0 when slow) */
  bool slow = false; /* no single-pass plan: the host runs its jobs one at a
                        time through reconstruct + verify */
};

/* Validate one erasure pattern the way gfrs_reconstruct_verify_batch would
 * and build its plan.  GFRS_OK with q->slow set leaves *p empty. */
int queue_pattern(const Code &c, const int32_t *bad, int nbad, Plan *p,
                  QueuePattern *q);
/* The validation alone (what a plan-cache hit still has to decide). */
int queue_pattern_check(const Code &c, const int32_t *bad, int nbad,
                        bool *slow);

struct QueueBucket {
  int g = 0, gm = 0;
  size_t first = 0, count = 0; /* its work items: items[first, first+count) */
  size_t prefix = 0; /* its count+1 tile prefix sums start at
                        tile_prefix[prefix] (= first + bucket index) */
};

struct QueueSchedule {
  std::vector<gfrs_qitem> items;     /* every bucket's items, back to back;
                                        inside a bucket ordered by pattern,
                                        then by caller index */
  std::vector<uint64_t> tile_prefix; /* exclusive prefix sums of
                                        ceil(shard_len / QUEUE_TILE) */
  std::vector<QueueBucket> buckets;
  std::vector<int32_t> slow_jobs;    /* caller order */
};

/* GFRS_ERR_INVALID_SHARDS: njobs <= 0, npat <= 0, pattern out of range,
 * reserved != 0; GFRS_ERR_SHARD_NO_DATA: shard_len == 0. */
int queue_schedule(const gfrs_qjob *jobs, int njobs, const QueuePattern *pats,
                   int npat, QueueSchedule *out);
/* bad_off: npat+1 non-decreasing entries starting at 0 */
int queue_offsets_check(const int32_t *bad_off, int npat);

/* ---- the repair-image queue (gfrs_repair_queue) ----
 * gfrs_repair_batch as a queue.  A pattern is FUSED when the gate of
 * gfrs_repair_batch holds for it; it then has a plan_fused_repair plan of
 * gm = rebuild + check rows <= 4 and runs the fused frame kernel.  Every
 * other pattern is IN-PLACE: the schedule of gfrs_reconstruct_verify_queue
 * reconstructs and verifies its jobs in `base`, and each repaired shard is
 * then framed from `base` by an IDENTITY work item - the fused frame kernel
 * over the one-input plan {k = 1, coefficient 1, one rebuild row, imap[0] =
 * the shard} is a pure "frame this shard" kernel - in the 1-row bucket.  So
 * framing costs at most REPAIR_ROWS launches whatever the tactic is.
 * Descriptor index of a work item: fused pattern p is p, the identity of
 * shard s is npat + s. */
constexpr int REPAIR_ROWS = 4;             /* rows of the fused frame kernel */
constexpr uint64_t REPAIR_PAYLOAD = 65532; /* raw bytes per image frame */
constexpr int64_t REPAIR_BLOCK = 65536;    /* the only block_len served */

struct RepairPattern {
  int cls = GFRS_RPAT_INPLACE;
  int nbad = 0;
  int gm = 0, nw = 0;   /* fused: rows of the plan / of them rebuild rows */
  uint32_t colpack = 0; /* fused: repair_colpack of the caller's order */
};

/* Validate one pattern (the codes of queue_pattern_check, and
 * GFRS_ERR_INVALID_SHARDS when it is empty or repeats an index) and class
 * it; nw and colpack are set, gm is the plan's to tell (repair_pattern, or
 * the cached plan's row count). */
int repair_pattern_check(const Code &c, const int32_t *bad, int nbad,
                         RepairPattern *r);
/* ... and build the plan_fused_repair plan of a fused pattern (*p stays
 * empty for an in-place one). */
int repair_pattern(const Code &c, const int32_t *bad, int nbad, Plan *p,
                   RepairPattern *r);

/* raw size -> bytes of the on-disk image (header + framed body + footer) */
uint64_t repair_image_size(uint64_t shard_len);

struct RepairBucket {
  int gm = 0;
  size_t first = 0, count = 0; /* items[first, first+count) */
  size_t prefix = 0; /* its count+1 frame prefix sums start here
                        (= first + bucket index) */
};

struct RepairSchedule {
  std::vector<gfrs_ritem> items;      /* every bucket's items, back to back;
                                         inside a bucket ordered by
                                         descriptor, then by caller index */
  std::vector<uint64_t> frame_prefix; /* exclusive prefix sums of
                                         ceil(shard_len / REPAIR_PAYLOAD) */
  std::vector<RepairBucket> buckets;  /* ascending gm, at most REPAIR_ROWS */
  std::vector<gfrs_rimage> images;    /* id order */
  std::vector<int32_t> inplace_jobs;  /* caller order */
};

/* Job validation (gfrs.h, repair-queue contract; dst_addr = the address of
 * disk_dst, for the alignment rule) and the schedule.  pats carry cls, nbad
 * and, for fused patterns, gm; bad_idx / bad_off as given by the caller;
 * bids / vuids may be null. */
int repair_schedule(const gfrs_rjob *jobs, int njobs,
                    const RepairPattern *pats, int npat,
                    const int32_t *bad_idx, const int32_t *bad_off,
                    uint64_t dst_addr, const uint64_t *bids,
                    const uint64_t *vuids, RepairSchedule *out);

/* ---- the encode+frame queue (gfrs_encode_frame_queue) ----
 * gfrs_encode_frame_batch as a queue.  There is one encode plan per context,
 * so the schedule only decides which kernel form serves which job:
 *   SMALL  shard_len <= ENCQ_SMALL_MAX: one wave per job, one bucket per
 *          NI = ceil(shard_len / 1024) = 1..4 (the wave kernel keeps its
 *          NI-long loops compile-time); item i of the bucket is wave i, so a
 *          small bucket has no prefix sums;
 *   FRAME  longer jobs: one workgroup per 64 KiB frame, split at the batch
 *          launcher's threshold of ENCQ_LARGE_MIN bytes per shard into the
 *          two variants it would pick (87 below, 76 from it up); each bucket
 *          has the count+1 exclusive prefix sums of ceil(shard_len / 65532).
 * Buckets come in a fixed order - small NI ascending, frame 87, frame 76 -
 * and hold their items in caller order: at most ENCQ_BUCKETS launches. */
constexpr uint64_t ENCQ_SMALL_MAX = 4096;
constexpr uint64_t ENCQ_LARGE_MIN = uint64_t(1) << 20;
constexpr int ENCQ_BUCKETS = 6;
constexpr int ENCQ_VAR_SMALL_SHARDS = 87; /* 4 waves, nontemporal stores */
constexpr int ENCQ_VAR_LARGE_SHARDS = 76; /* 3 waves, plain stores */

struct EncBucket {
  int kind = GFRS_EQ_SMALL, param = 0;
  size_t first = 0, count = 0; /* items[first, first+count) */
  size_t prefix = 0; /* frame buckets: its count+1 prefix sums start at
                        frame_prefix[prefix] */
};

struct EncSchedule {
  std::vector<gfrs_eitem> items;      /* every bucket's items, back to back */
  std::vector<uint64_t> frame_prefix; /* of the frame buckets, back to back */
  std::vector<EncBucket> buckets;
};

/* the gate of gfrs_encode_frame_batch's fused kernels, block_len aside */
bool encode_frame_fused(const Code &c);
/* crc32block image size of a shard at block_len 65536 */
uint64_t encode_image_size(uint64_t shard_len);
/* block_len of the encode queue: GFRS_ERR_INVALID_BLOCK / _UNSUPPORTED */
int encode_queue_block_check(int64_t block_len);
/* Job validation (gfrs.h, encode-queue contract; framed_addr = the address
 * of framed, for the alignment rule) and the schedule. */
int encode_queue_schedule(const gfrs_ejob *jobs, int njobs,
                          uint64_t framed_addr, EncSchedule *out);

/* ---- the read queue (gfrs_read_queue) ----
 * The degraded GET: crc32block decode of the surviving images and
 * ReconstructData of a segment, in one pass over the images.  A pattern is
 * classed by R, its number of missing data shards:
 *   FUSED     R <= READ_ROWS and total <= 16: a job is one work item of the
 *             pattern's plan_read descriptor in the bucket of its R;
 *   IDENTITY  R == 0 on a wider tactic: a job is one item per data shard s
 *             under the identity descriptor npat + s (k = 1, one pass-through
 *             input), in the R = 0 bucket;
 *   SLOW      everything else: one job at a time on the host's slow path.
 * So the fused launches number at most READ_ROWS + 1 whatever the queue. */
constexpr int READ_ROWS = 4; /* rebuilt rows of the read kernel */
constexpr int READ_WORD_BITS = 32; /* shards a verdict word can name */

struct ReadPattern {
  int cls = GFRS_GPAT_FUSED;
  int r = 0; /* missing data shards */
};

/* the read plan: `in` = the plan_decode inputs of the global engine (first n
 * present of the n+m, index order), `out` = the missing data shards ascending
 * (write rows only), pass_mask = which inputs are data shards.  Entries of
 * `bad` naming local parities are ignored.  With no data shard missing the
 * plan has inputs and no rows. */
int plan_read(const Code &c, const int32_t *bad, int nbad, Plan *p);
/* Validate one pattern (GFRS_ERR_INVALID_SHARDS for an index out of range or
 * repeated, GFRS_ERR_TOO_FEW_SHARDS for more than m global losses) and class
 * it. */
int read_pattern_check(const Code &c, const int32_t *bad, int nbad,
                       ReadPattern *r);
/* ... and build its plan_read plan (for every class: the slow path wants the
 * input list too). */
int read_pattern(const Code &c, const int32_t *bad, int nbad, Plan *p,
                 ReadPattern *r);

struct ReadBucket {
  int r = 0;
  size_t first = 0, count = 0; /* items[first, first+count) */
  size_t prefix = 0; /* its count+1 frame prefix sums start here
                        (= first + bucket index) */
};

struct ReadSchedule {
  std::vector<gfrs_gitem> items;      /* every bucket's items, back to back;
                                         inside a bucket ordered by
                                         descriptor, then by caller index */
  std::vector<uint64_t> frame_prefix; /* exclusive prefix sums of the frames
                                         TOUCHED by each item's segment */
  std::vector<ReadBucket> buckets;    /* ascending r, at most READ_ROWS + 1 */
  std::vector<int32_t> slow_jobs;     /* caller order */
};

/* frames [first, last] of a shard that the segment touches */
inline uint64_t read_first_frame(const gfrs_gjob &j) {
  return j.seg_off / REPAIR_PAYLOAD;
}
inline uint64_t read_last_frame(const gfrs_gjob &j) {
  return (j.seg_off + j.seg_len - 1) / REPAIR_PAYLOAD;
}

/* block_len and tactic width: GFRS_ERR_INVALID_BLOCK / _UNSUPPORTED */
int read_queue_gate(const Code &c, int64_t block_len);
/* Job validation (gfrs.h, read-queue contract; out_addr = the address of out,
 * for the alignment rule) and the schedule. */
int read_schedule(const Code &c, const gfrs_gjob *jobs, int njobs,
                  const ReadPattern *pats, int npat, uint64_t out_addr,
                  ReadSchedule *out);

/* ---- the shard read queue (gfrs_shard_read_queue) ----
 * Verify and unframe the disk images of one chunk.  There is no coding plan:
 * the schedule only splits the jobs into the two builds of the frame kernel,
 * storing jobs first, then NO_OUT jobs, each bucket in caller order with the
 * count+1 exclusive prefix sums of the frames its items touch.  The computed
 * CRC of the frame at walk position w of bucket b is kept at
 * frame_base(b) + w of the context's scratch, job_frame[j] being the place of
 * job j's first touched frame there (the header kernel folds a FOOTER job's
 * words from it). */
struct ShardReadBucket {
  int no_out = 0;
  size_t first = 0, count = 0; /* items[first, first+count) */
  size_t prefix = 0; /* its count+1 frame prefix sums start here
                        (= first + bucket index) */
  uint64_t frame_base = 0; /* frames of the buckets before it */
};

struct ShardReadSchedule {
  std::vector<gfrs_sitem> items;      /* both buckets' items, back to back */
  std::vector<uint64_t> frame_prefix; /* exclusive prefix sums of the frames
                                         TOUCHED by each item's range */
  std::vector<ShardReadBucket> buckets; /* storing, then NO_OUT */
  std::vector<uint64_t> job_frame;    /* njobs entries, caller order */
  uint64_t total_frames = 0;
};

/* frames [first, last] of an image that the range touches */
inline uint64_t shard_first_frame(const gfrs_sjob &j) {
  return j.from / REPAIR_PAYLOAD;
}
inline uint64_t shard_last_frame(const gfrs_sjob &j) {
  return (j.to - 1) / REPAIR_PAYLOAD;
}

/* Job validation (gfrs.h, shard-read-queue contract; out_addr = the address
 * of out, for the alignment rule, have_out = it is not NULL) and the
 * schedule.  block_len goes through encode_queue_block_check. */
int shard_read_schedule(const gfrs_sjob *jobs, int njobs, uint64_t out_addr,
                        bool have_out, ShardReadSchedule *out);

/* ---- the shard write queue (gfrs_shard_write_queue) ----
 * Frame payloads - raw bytes, or the body of an existing disk image - into
 * new disk images.  Again no coding plan: the schedule splits the jobs into
 * the two builds of the frame kernel, raw jobs first, then SRC_IMAGE jobs,
 * each bucket in caller order with the count+1 exclusive prefix sums of its
 * items' frames.  The computed CRC of the frame at walk position w of bucket
 * b is kept at frame_base(b) + w of the context's scratch, job_frame[j] being
 * the place of job j's first frame there (the head kernel folds every job's
 * words from it). */
struct ShardWriteBucket {
  int src_image = 0;
  size_t first = 0, count = 0; /* items[first, first+count) */
  size_t prefix = 0; /* its count+1 frame prefix sums start here
                        (= first + bucket index) */
  uint64_t frame_base = 0; /* frames of the bucket before it */
};

struct ShardWriteSchedule {
  std::vector<gfrs_witem> items;      /* both buckets' items, back to back */
  std::vector<uint64_t> frame_prefix; /* exclusive prefix sums of the items'
                                         frames, ceil(size / 65532) */
  std::vector<ShardWriteBucket> buckets; /* raw, then SRC_IMAGE */
  std::vector<uint64_t> job_frame;    /* njobs entries, caller order */
  uint64_t total_frames = 0;
};

/* Job validation (gfrs.h, shard-write-queue contract; dst_addr = the address
 * of dst, for the alignment rule) and the schedule.  block_len goes through
 * encode_queue_block_check. */
int shard_write_schedule(const gfrs_wjob *jobs, int njobs, uint64_t dst_addr,
                         ShardWriteSchedule *out);

/* ---- the put queue (gfrs_put_queue) ----
 * The encode+frame queue into disk images, for every tactic up to PUT_MAX_N
 * data shards.  A job is one work item of the encode schedule whose image row
 * starts behind the 32-byte header (img = img_off + 32).  The m+l parity rows
 * - the encode plan's, or plan_fused_lrc's for an LRC tactic - run in row
 * groups of PUT_ROWS: group g is rows [PUT_ROWS*g, PUT_ROWS*g + rows(g)).  A
 * tactic inside encode_frame_fused is NARROW: one group, the encode queue's
 * buckets and kernels.  Every other one is WIDE: only the two frame buckets,
 * each launched once per group with the put frame kernel.  The image table
 * (job-major, shard order) feeds the head launch. */
constexpr int PUT_ROWS = 4;   /* rows per group (the kernels' GM) */
constexpr int PUT_MAX_N = 32; /* data shards the put frame kernel's LDS holds */

struct PutSchedule {
  EncSchedule enc;
  std::vector<gfrs_rimage> images;
  bool wide = false;
  std::vector<int32_t> group_rows;
};

/* block_len and tactic width: GFRS_ERR_INVALID_BLOCK / _UNSUPPORTED */
int put_queue_gate(const Code &c, int64_t block_len);
/* Job validation (gfrs.h, put-queue contract; dst_addr = the address of
 * disk_dst, for the alignment rule) and the schedule. */
int put_queue_schedule(const Code &c, const gfrs_pjob *jobs, int njobs,
                       const uint64_t *vuids, int nvol, uint64_t dst_addr,
                       PutSchedule *out);

}  // namespace gfrs

#endif
