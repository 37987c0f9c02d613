/* cubefs_amd/csrc/gfrs_internal.h — internal declarations shared between
 * the host runtime (gfrs_host.cpp) and kernel launchers (gfrs_kernels.hip).
 * The GF(2^8) math and the plan builders are in gfrs_plan.h (no HIP).
 * Product code: independent of oracle/.
 */
#ifndef GFRS_INTERNAL_H
#define GFRS_INTERNAL_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include <hip/hip_runtime.h>

#include "gfrs_plan.h"

namespace gfrs {

/* ---- kernel launch interface ---- */

/* Matrix-apply over a stripe batch (serves encode and reconstruct).
 * For each stripe s (0..nstripes), output r (0..nout), byte i:
 *   out[r][i] = XOR_c coeff[r*k+c] * in[c][i]
 * where in/out shard pointers come from ptrs[s*nptr + idx]:
 *   in  c -> ptrs[s*nptr + in_idx[c]]
 *   out r -> ptrs[s*nptr + out_idx[r]]
 * tabs = device array [nout*k][32]: per-coefficient A|B|C linear-split
 * tables (DevPlan::upload in gfrs_host.cpp documents the layout).
 * All index/table arrays are device memory. */
void launch_rs_apply(const uint64_t *ptrs, int nptr, const int32_t *in_idx,
                     int k, const int32_t *out_idx, int nout,
                     const uint8_t *tabs, size_t shard_len, int nstripes,
                     hipStream_t s);

/* Verify: recompute parity from tabs and OR a nonzero flag into
 * fail[s] for any mismatching stripe. */
void launch_rs_verify(const uint64_t *ptrs, int nptr, const int32_t *in_idx,
                      int k, const int32_t *out_idx, int nout,
                      const uint8_t *tabs, size_t shard_len, int nstripes,
                      uint32_t *fail, hipStream_t s);

/* crc32block kernels.  Shards framed independently; shard j raw bytes at
 * src + j*src_stride (n bytes), framed at dst + j*dst_stride.
 * suffix_ops: device array of fold operators (see gfrs_kernels.hip). */
void launch_crc_encode(uint8_t *dst, size_t dst_stride, const uint8_t *src,
                       size_t src_stride, int64_t n, int64_t block_len,
                       int nshards, hipStream_t s);
/* bad[j] = first failing block index in shard j, or -1 (preset by host). */
void launch_crc_verify(const uint8_t *framed, size_t stride,
                       int64_t framed_len, int64_t block_len, int nshards,
                       int64_t *bad, hipStream_t s);
void launch_crc_decode(uint8_t *dst, size_t dst_stride, const uint8_t *framed,
                       size_t src_stride, int64_t framed_len,
                       int64_t block_len, int nshards, int64_t *bad,
                       hipStream_t s);

/* fused encode+frame: parity + crc32block framed images in one pass
 * (PUT/repair pipeline; data read once, framed written once). */
void launch_rs_encode_frame_small(uint8_t *dst, size_t dst_stride,
                                  uint64_t base, uint64_t stripe_stride,
                                  size_t shard_len, int k, int m,
                                  const uint8_t *tabs, int nstripes,
                                  hipStream_t s);

void launch_rs_repair_frame_small(uint8_t *dst, size_t dst_stride,
                                  uint64_t base, uint64_t stripe_stride,
                                  size_t shard_len, int k, int gm, int nw,
                                  const int32_t *imap, const uint8_t *tabs,
                                  uint32_t colpack, uint32_t *fail,
                                  int nstripes, hipStream_t s);

void launch_rs_repair_frame(uint8_t *dst, size_t dst_stride, uint64_t base,
                            uint64_t stripe_stride, size_t shard_len, int k,
                            int gm, int nw, const int32_t *imap,
                            const uint8_t *tabs, uint32_t colpack,
                            uint32_t *fail, int nstripes, hipStream_t s);

void launch_rs_encode_frame(uint8_t *dst, size_t dst_stride, uint64_t base,
                            uint64_t stripe_stride, size_t shard_len, int k,
                            int m, const uint8_t *tabs, int nstripes,
                            hipStream_t s);

/* Encode+frame queue: one bucket of the encode schedule (gfrs_plan.h).  An
 * item is launch_rs_encode_frame over its own job:
 *   data shard c at base + item.off + c * item.shard_len,
 *   image of shard j at dst + item.img + j * item.img_stride.
 * Frame buckets: frame_prefix holds the nitems+1 exclusive prefix sums of
 * ceil(shard_len / 65532), total_frames its last entry; var is the batch
 * launcher's variant (76: 3 waves, plain stores; 87: 4 waves, nontemporal).
 * Small buckets: every item has ceil(shard_len / 1024) == ni, and item i is
 * wave i.  tabs: the context's encode plan, [m*k][32]. */
void launch_rs_encode_frame_queue(uint8_t *dst, uint64_t base,
                                  const gfrs_eitem *items,
                                  const uint64_t *frame_prefix,
                                  uint32_t nitems, uint64_t total_frames,
                                  int k, int m, const uint8_t *tabs, int var,
                                  hipStream_t s);
void launch_rs_encode_frame_small_queue(uint8_t *dst, uint64_t base,
                                        const gfrs_eitem *items,
                                        uint32_t nitems, int k, int m, int ni,
                                        const uint8_t *tabs, hipStream_t s);

/* sized coder (crc32block/sized_coder.go): payload ‖ CRC32(BE) frames,
 * 512-B tail alignment handled by the host. */
void launch_sized_encode(uint8_t *dst, size_t dst_stride, const uint8_t *src,
                         size_t src_stride, int64_t n, int64_t block_len,
                         int nshards, hipStream_t s);
void launch_sized_verify(const uint8_t *framed, size_t stride,
                         int64_t body_len, int64_t block_len, int nshards,
                         int64_t *bad, hipStream_t s);
void launch_sized_decode(uint8_t *dst, size_t dst_stride,
                         const uint8_t *framed, size_t src_stride,
                         int64_t body_len, int64_t block_len, int nshards,
                         int64_t *bad, hipStream_t s);

/* Mixed write/compare strided apply (reconstruct+verify in one pass). */
void launch_rs_apply_mixed_strided(uint64_t base, uint64_t stripe_stride,
                                   const int32_t *in_idx, int k,
                                   const int32_t *out_idx, int nout,
                                   const uint8_t *tabs, uint32_t cmp_mask,
                                   size_t shard_len, int nstripes,
                                   uint32_t *fail, hipStream_t s);

/* Repair queue: one bucket of the schedule (gfrs_plan.h), i.e. every
 * (job, step) pair with the same step index and the same row count gm.
 * Each work item is a mixed write/compare apply of gm rows of its own
 * pattern's plan, starting at its row_off, over its own job:
 *   shard i of the job at base + item.off + i * item.shard_len.
 * pats[item.pattern] describes that plan (device pointers into the cached
 * DevPlans); tile_prefix holds the nitems+1 exclusive prefix sums of
 * ceil(shard_len / 4096), total_tiles its last entry.  Mismatches of compare
 * rows are ORed into fail[item.job].  All arrays are device memory. */
struct QueuePat {
  const int32_t *in_idx;  /* k inputs */
  const int32_t *out_idx; /* nout rows */
  const uint8_t *tabs;    /* [nout*k][32] */
  uint32_t cmp_mask;
  int32_t nout;
};
void launch_rs_apply_queue(uint64_t base, const gfrs_qitem *items,
                           const uint64_t *tile_prefix, uint32_t nitems,
                           uint64_t total_tiles, const QueuePat *pats, int k,
                           int gm, uint32_t *fail, hipStream_t s);

/* Repair-image queue: one bucket of the repair schedule (gfrs_plan.h), i.e.
 * every work item whose descriptor carries gm rows.  An item is the fused
 * repair of launch_rs_repair_frame over its own job:
 *   shard i at base + item.off + i * item.shard_len,
 *   body of image column c at dst + item.img + c * item.img_stride + 32,
 * under descs[item.desc] (device pointers into the cached DevPlans, or into
 * the call's blob for identity descriptors).  frame_prefix holds the
 * nitems+1 exclusive prefix sums of ceil(shard_len / 65532), total_frames
 * its last entry; kmax bounds every descriptor's k (it sizes the LDS
 * tables).  Mismatches of check rows are ORed into fail[item.job]. */
struct RepairDesc {
  const int32_t *imap; /* k inputs then gm - nw check shards */
  const uint8_t *tabs; /* [gm*k][32] */
  int32_t k, nw;
  uint32_t colpack;
  int32_t reserved;
};
void launch_rs_repair_frame_queue(uint8_t *dst, uint64_t base,
                                  const gfrs_ritem *items,
                                  const uint64_t *frame_prefix,
                                  uint32_t nitems, uint64_t total_frames,
                                  const RepairDesc *descs, int kmax, int gm,
                                  uint32_t *fail, hipStream_t s);
/* Headers and footers of every image of a repair queue: launch_shard_finalize
 * with the image's place, raw size and ids read from imgs[]; block_len is
 * 65536.  crcs: NULL, or a device array of nimg words that gets the footer's
 * CRC of every image (the put queue's read-back). */
void launch_shard_finalize_queue(uint8_t *dst, const gfrs_rimage *imgs,
                                 int nimg, uint32_t *crcs, hipStream_t s);

/* Put queue, wide tactics: one frame bucket of the put schedule (gfrs_plan.h)
 * for one row group.  An item is its own job:
 *   data shard c at base + item.off + c * item.shard_len, c < k <= 32,
 *   body of image column j at dst + item.img + j * item.img_stride.
 * The launch computes gm = 1..4 parity rows from tabs ([gm*k][32], the
 * group's slice of the plan) into image columns k + row0 + r; data = true
 * (group 0: row0 must be 0, the DATA build takes it as a constant) also frames
 * the k data shards into columns 0..k-1, data = false reads them only.
 * frame_prefix, total_frames and var as for launch_rs_encode_frame_queue. */
void launch_rs_put_frame_queue(uint8_t *dst, uint64_t base,
                               const gfrs_eitem *items,
                               const uint64_t *frame_prefix, uint32_t nitems,
                               uint64_t total_frames, int k, int gm, int row0,
                               const uint8_t *tabs, int var, bool data,
                               hipStream_t s);

/* Read queue: one bucket of the read schedule (gfrs_plan.h), i.e. every work
 * item whose descriptor rebuilds r rows (0..4).  An item reads the frames its
 * segment touches of the images of its descriptor's k inputs,
 *   payload of frame f of input c at
 *     framed + item.img + imap[c] * item.img_stride + f * 65536 + 4,
 * checks their CRCs against the stored headers, and writes the segment of
 *   every input with its pass bit set, to row imap[c], and
 *   the r rebuilt shards, to rows omap[0..r),
 * row i at out + item.out + i * item.out_stride.  descs[item.desc] points
 * into the cached DevPlans, or into the call's blob for identity descriptors;
 * frame_prefix holds the nitems+1 exclusive prefix sums of touched frames,
 * total_frames its last entry; kmax bounds every descriptor's k (it sizes the
 * LDS tables, at most 16).  A CRC mismatch of input c ORs 1 << imap[c] into
 * fail[item.job]. */
struct ReadDesc {
  const int32_t *imap; /* k inputs */
  const int32_t *omap; /* r rebuilt shards */
  const uint8_t *tabs; /* [r*k][32]; unused when r == 0 */
  int32_t k;
  uint32_t pass_mask; /* bit c: input c is copied to row imap[c] */
};
void launch_rs_read_frame_queue(uint8_t *out, uint64_t framed,
                                const gfrs_gitem *items,
                                const uint64_t *frame_prefix, uint32_t nitems,
                                uint64_t total_frames, const ReadDesc *descs,
                                int kmax, int r, uint32_t *fail,
                                hipStream_t s);

/* Shard read queue: one bucket of the shard-read schedule (gfrs_plan.h).  An
 * item reads the frames its range [from, to) touches of its image,
 *   payload of frame f at chunk + item.img + 32 + f * 65536 + 4,
 * writes the computed CRC of the frame at walk position w to fcrc[w] (fcrc
 * already offset by the bucket's frame_base), lowers bad[item.job] to f
 * when it differs from the stored word (bad preset to -1, compared unsigned),
 * and - store = true - writes bytes [from, to) of the payload at
 * out + item.out.  frame_prefix holds the nitems+1 exclusive prefix sums of
 * touched frames, total_frames its last entry. */
void launch_shard_read_frame_queue(uint8_t *out, uint64_t chunk,
                                   const gfrs_sitem *items,
                                   const uint64_t *frame_prefix,
                                   uint32_t nitems, uint64_t total_frames,
                                   bool store, uint32_t *fcrc, int64_t *bad,
                                   hipStream_t s);
/* ... and its results, one wave per job after the frame buckets: header bits
 * and fields, BODY_CRC from bad[j], and for FOOTER jobs the fold of the job's
 * fcrc words from fcrc[job_frame[j]] on and the two footer bits. */
void launch_shard_head_queue(uint64_t chunk, const gfrs_sjob *jobs,
                             const uint64_t *job_frame, const uint32_t *fcrc,
                             const int64_t *bad, gfrs_sresult *results,
                             int njobs, hipStream_t s);

/* Shard write queue: one bucket of the shard-write schedule (gfrs_plan.h).
 * An item frames its payload - img = false: raw bytes,
 *   payload of frame f at src + item.src + f * 65532,
 * img = true: the body of a disk image,
 *   payload of frame f at src + item.src + 32 + f * 65536 + 4 -
 * into the new image at dst + item.img: the payload at
 *   dst + item.img + 32 + f * 65536 + 4
 * and the computed CRC as the 4-byte LE word in front of it.  The CRC of the
 * frame at walk position w also goes to fcrc[w] (fcrc already offset by the
 * bucket's frame_base); with img = true bad[item.job] is lowered to f when the
 * source's stored word differs (bad preset to -1, compared unsigned).
 * frame_prefix holds the nitems+1 exclusive prefix sums of the items' frames,
 * total_frames its last entry. */
void launch_shard_write_frame_queue(uint8_t *dst, uint64_t src,
                                    const gfrs_witem *items,
                                    const uint64_t *frame_prefix,
                                    uint32_t nitems, uint64_t total_frames,
                                    bool img, uint32_t *fcrc, int64_t *bad,
                                    hipStream_t s);
/* ... and its headers, footers and results, one wave per job after the frame
 * buckets: the new header, the fold of the job's fcrc words from
 * fcrc[job_frame[j]] on into the new footer and the result's crc, and for
 * SRC_IMAGE jobs the source's header bits and fields, BODY_CRC from bad[j]
 * and the two footer bits. */
void launch_shard_write_head_queue(uint8_t *dst, uint64_t src,
                                   const gfrs_wjob *jobs,
                                   const uint64_t *job_frame,
                                   const uint32_t *fcrc, const int64_t *bad,
                                   gfrs_sresult *results, int njobs,
                                   hipStream_t s);

/* EncodeIdx-style accumulate apply (reedsolomon.go:631-668):
 * out[r] ^= coeff[r]*in for one input shard. */
void launch_rs_apply_xor(const uint64_t *ptrs, int nptr,
                         const int32_t *in_idx, int k,
                         const int32_t *out_idx, int nout,
                         const uint8_t *tabs, size_t shard_len, int nstripes,
                         hipStream_t s);

/* blobnode on-disk shard codec (core/shard.go, datafile.go:342-445). */
void launch_shard_finalize(uint8_t *dst, size_t dst_stride,
                           const uint64_t *bids, const uint64_t *vuids,
                           int64_t raw_size,
                           int64_t block_len, int nshards, hipStream_t s);
void launch_shard_parse(const uint8_t *img, size_t stride, int64_t raw_size,
                        int64_t block_len, int nshards, uint64_t *out,
                        hipStream_t s);

/* v_perm semantics probe: returns 1 when `sel byte >= 8 -> 0x00` holds. */
int probe_perm_device(void);

/* One-time CRC table upload for the current device. */
int crc_device_init_current(void);

/* Strided-layout variants (batch APIs; stripe s shard i at
 * base + s*stripe_stride + i*shard_len). */
void launch_rs_apply_strided(uint64_t base, uint64_t stripe_stride,
                             const int32_t *in_idx, int k,
                             const int32_t *out_idx, int nout,
                             const uint8_t *tabs, size_t shard_len,
                             int nstripes, hipStream_t s);
void launch_rs_verify_strided(uint64_t base, uint64_t stripe_stride,
                              const int32_t *in_idx, int k,
                              const int32_t *out_idx, int nout,
                              const uint8_t *tabs, size_t shard_len,
                              int nstripes, uint32_t *fail, hipStream_t s);

}  // namespace gfrs

#endif
