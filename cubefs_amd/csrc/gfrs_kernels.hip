/* cubefs_amd/csrc/gfrs_kernels.hip — CDNA4 (gfx950) kernels for the CubeFS
 * blobstore EC/CRC hot path.
 *
 * Replaces (same arithmetic, MI355X-native data path):
 *   galois_amd64.s / galois_gen_amd64.s  (GF(2^8) nibble-table multiply:
 *     out[i] ^= lo[c][in[i]&0xF] ^ hi[c][in[i]>>4]; tables galois.go:340,596)
 *   reedsolomon.go:807-985 codeSomeShards[P] (fused k-input × m-output
 *     matrix apply; the goroutine byte-range split becomes the wave/grid
 *     split)
 *   Go hash/crc32 CLMUL path + crc32block/block.go:22-49 framing
 *
 * Design notes (HBM-bound byte work; no MFMA — GF(2^8) is not a dense
 * contraction):
 *  - rs_apply: each lane owns 16 B columns (uint4 loads, 1 KiB per wave
 *    per instruction); all nout outputs accumulate in VGPRs so every input
 *    byte is read from HBM exactly once per output-group of 4.
 *  - GF multiply = two 16-entry nibble lookups done in-register with
 *    v_perm_b32 over the 32 B coefficient table (staged in LDS, broadcast
 *    reads) — no per-byte LDS gather.
 *  - crc32block: one 256-thread workgroup per 64 KiB frame; each thread
 *    CRCs a 256 B chunk (slice-by-4, tables in LDS), chunks are folded with
 *    the GF(2) x^(8·len) shift operator and reduced in LDS.  This is the
 *    parallel decomposition of the sequential Go loop; bit-identical.
 */
#include "gfrs_internal.h"

#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

namespace gfrs {

static int env_grid(const char *name, int dflt) {
  const char *v = getenv(name);
  if (!v) return dflt;
  int x = atoi(v);
  return x > 0 ? x : dflt;
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

static bool nt_enabled() {
  static int v = -1;
  if (v < 0) {
    const char *e = getenv("GFRS_NT");
    v = e ? (atoi(e) != 0) : 0;
  }
  return v == 1;
}

/* Streaming 16-B store; NT bypasses L2 (outputs are never re-read by the
 * producing kernel). */
template <bool NT>
__device__ __forceinline__ void store16(uint8_t *p, const uint4 v) {
  if (NT) {
    u32x4 x = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(x, reinterpret_cast<u32x4 *>(p));
  } else {
    *reinterpret_cast<uint4 *>(p) = v;
  }
}

#define GFRS_DEV __device__ __forceinline__

/* Pointers rebuilt from integers (stripe math, pointer tables) lose the
 * global address space and compile to flat_load/flat_store with per-access
 * 64-bit vaddr arithmetic.  A round-trip through an explicit AS(1) cast
 * lets InferAddressSpaces prove the access is global (global_load_* with
 * scalar base + 32-bit voffset). */
GFRS_DEV const uint8_t *as_global(uint64_t p) {
  return (const uint8_t *)(const __attribute__((address_space(1))) uint8_t *)p;
}

/* ------------------------------------------------------------------ */
/* GF(2^8) nibble multiply on packed u32, via v_perm_b32                */
/* ------------------------------------------------------------------ */

/* 16-entry byte table lookup for 4 packed nibbles (each byte of `nib` in
 * 0..15).  Table held as two uint4 (t01 = bytes 0..7 in .x/.y, plus 8..15
 * in .z/.w).  PERM0: rely on v_perm sel>=8 -> 0x00 (probed at runtime);
 * otherwise mask-and-blend. */
template <bool PERM0>
GFRS_DEV uint32_t lut16(const uint4 t, uint32_t nib) {
  if (PERM0) {
    /* sel>=8 yields 0, so the two halves OR together by XOR. */
    uint32_t a = __builtin_amdgcn_perm(t.y, t.x, nib);
    uint32_t b = __builtin_amdgcn_perm(t.w, t.z, nib ^ 0x08080808u);
    return a ^ b;
  } else {
    uint32_t s = nib & 0x07070707u;
    uint32_t a = __builtin_amdgcn_perm(t.y, t.x, s);
    uint32_t b = __builtin_amdgcn_perm(t.w, t.z, s);
    uint32_t m = (nib & 0x08080808u) >> 3;
    m *= 0xFFu; /* per-byte 0x00/0xFF, no carries */
    /* one v_bitop3_b32: imm bit index = src0*4 + src1*2 + src2, so
     * select(m ? b : a) = 0xD8 (bits 3,4,6,7) */
    return __builtin_amdgcn_bitop3_b32(a, b, m, 0xD8);
  }
}

/* out ^= mul_c(v) for 4 packed bytes; tlo/thi are c's 16-B low/high nibble
 * tables (galois_amd64.go:37-52 semantics). */
template <bool PERM0>
GFRS_DEV uint32_t gfmul4(uint32_t v, const uint4 tlo, const uint4 thi) {
  return lut16<PERM0>(tlo, v & 0x0F0F0F0Fu) ^
         lut16<PERM0>(thi, (v >> 4) & 0x0F0F0F0Fu);
}

template <bool PERM0>
GFRS_DEV void gfmac16(uint4 &acc, const uint4 v, const uint4 tlo,
                      const uint4 thi) {
  acc.x ^= gfmul4<PERM0>(v.x, tlo, thi);
  acc.y ^= gfmul4<PERM0>(v.y, tlo, thi);
  acc.z ^= gfmul4<PERM0>(v.z, tlo, thi);
  acc.w ^= gfmul4<PERM0>(v.w, tlo, thi);
}

/* ------------------------------------------------------------------ */
/* 3-way linear GF multiply (A|B|C split) on packed u32                 */
/* ------------------------------------------------------------------ */

/* GF(2^8) multiply-by-constant is GF(2)-linear, so it splits over bit
 * groups of the operand: mul_c(b) = A[b&7] ^ B[(b>>3)&7] ^ C[b>>6] with
 * A[i] = mul(c,i), B[i] = mul(c,8i), C[i] = mul(c,64i).  Each group is a
 * <=8-entry byte table — exactly what one v_perm_b32 can look up for 4
 * packed bytes — so a 4-byte multiply is 3 v_perm + 1 bitop3(xor3)
 * instead of the nibble path's 4 v_perm + 2 blends, and the selectors
 * (shared across all output rows) cost 5 VALU instead of ~9 incl. two
 * v_mul_lo mask broadcasts. */
GFRS_DEV uint32_t xor3_fwd(uint32_t a, uint32_t b, uint32_t c) {
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); /* a ^ b ^ c */
}

/* Frame-payload 16-B store with a selectable cache policy.  The streams
 * are write-once (never re-read by the producer), so the interesting
 * policies are: 0 plain (line stays dirty in the XCD L2), 1 nontemporal,
 * 2 sc1 write-through (line dropped from L2 — frees L2 for the read
 * streams).  Policy choice is measured, not assumed; see profiles/. */
template <int ST>
GFRS_DEV void fstore16(uint8_t *p, const uint4 v) {
  if (ST == 1) {
    u32x4 x = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(x, reinterpret_cast<u32x4 *>(p));
  } else if (ST == 2) {
    u32x4 x = {v.x, v.y, v.z, v.w};
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1"
                 :
                 : "v"(p), "v"(x)
                 : "memory");
  } else {
    *reinterpret_cast<uint4 *>(p) = v;
  }
}

struct LinTab {
  uint32_t a0, a1, b0, b1, cc;
};

GFRS_DEV LinTab lintab_load(const uint8_t *ctab, int idx) {
  const uint32_t *tp =
      reinterpret_cast<const uint32_t *>(ctab + size_t(idx) * 32);
  return LinTab{tp[0], tp[1], tp[2], tp[3], tp[4]};
}

GFRS_DEV uint32_t gfmul4_lin(uint32_t s012, uint32_t s345, uint32_t s67,
                             const LinTab &t) {
  return xor3_fwd(__builtin_amdgcn_perm(t.a1, t.a0, s012),
                  __builtin_amdgcn_perm(t.b1, t.b0, s345),
                  __builtin_amdgcn_perm(t.cc, t.cc, s67));
}

/* acc[r][comp] ^= mul_{row r}(w) for one packed dword w */
template <int GM>
GFRS_DEV void gfmac4_lin_rows(uint4 (&acc)[GM][4], int i, int d, uint32_t w,
                              const LinTab (&lt)[GM]) {
  const uint32_t s012 = w & 0x07070707u;
  const uint32_t s345 = (w >> 3) & 0x07070707u;
  const uint32_t s67 = (w >> 6) & 0x03030303u;
#pragma unroll
  for (int r = 0; r < GM; r++)
    (&acc[r][i].x)[d] ^= gfmul4_lin(s012, s345, s67, lt[r]);
}

/* variable-width accumulator form (acc[GM][NI]) */
template <int GM, int NI>
GFRS_DEV void gfmac4_lin_rows_n(uint4 (&acc)[GM][NI], int i, int d,
                                uint32_t w, const LinTab (&lt)[GM]) {
  const uint32_t s012 = w & 0x07070707u;
  const uint32_t s345 = (w >> 3) & 0x07070707u;
  const uint32_t s67 = (w >> 6) & 0x03030303u;
#pragma unroll
  for (int r = 0; r < GM; r++)
    (&acc[r][i].x)[d] ^= gfmul4_lin(s012, s345, s67, lt[r]);
}

/* byte-path form for tails/prologues (same tables) */
GFRS_DEV uint8_t gfmul1_lin(const uint8_t *tt, uint8_t b) {
  return tt[b & 7] ^ tt[8 + ((b >> 3) & 7)] ^ tt[16 + (b >> 6)];
}

/* ------------------------------------------------------------------ */
/* rs_apply / rs_verify                                                 */
/* ------------------------------------------------------------------ */

constexpr int RS_BLOCK = 256;
constexpr int RS_TILE = RS_BLOCK * 16; /* 4096 B of columns per tile */
constexpr int MT = 4;                  /* output registers per pass */

struct ShardAddr {
  const uint64_t *ptrs; /* nstripes*nptr pointer table, or nullptr */
  uint64_t base;        /* strided mode: base + s*stripe_stride + i*shard_len */
  uint64_t stripe_stride;
  int nptr;

  GFRS_DEV const uint8_t *shard(size_t stripe, int idx, size_t shard_len) const {
    if (ptrs) return as_global(ptrs[stripe * nptr + idx]);
    return as_global(base + stripe * stripe_stride + uint64_t(idx) * shard_len);
  }
};

/* For each stripe and each output r: out[r] = XOR_c mul(coeff[r][c], in[c]).
 * tabs: [nout*k][32] per-coefficient lo|hi tables, staged to LDS.
 * Outputs processed in groups of MT so inputs stream from HBM once per
 * group (arithmetic intensity k·m/(k+m) table-xors per byte; HBM-bound). */
template <bool PERM0, bool VERIFY, bool NT, int GM>
__global__ __launch_bounds__(RS_BLOCK) void rs_apply_k(
    ShardAddr addr, const int32_t *__restrict__ in_idx, int k,
    const int32_t *__restrict__ out_idx, int nout,
    const uint8_t *__restrict__ tabs, size_t shard_len, size_t nstripes,
    uint32_t *fail, int xor_acc, int seq_map, uint32_t cmp_mask) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4 *ltab = reinterpret_cast<uint4 *>(smem); /* [k*nout*2] */
  const int ncoef = k * nout;
  for (int i = threadIdx.x; i < ncoef * 2; i += RS_BLOCK)
    ltab[i] = reinterpret_cast<const uint4 *>(tabs)[i];
  __syncthreads();

  const size_t tiles_per_shard = (shard_len + RS_TILE - 1) / RS_TILE;
  /* small shards (< half a tile): pack several stripes per tile so all
   * 256 lanes have columns — e.g. the 2 KiB MinShardSize foreground
   * shapes would otherwise idle 7/8 of the block */
  const size_t padded = (shard_len + 15) & ~size_t(15);
  const size_t spb =
      (tiles_per_shard == 1 && padded * 2 <= size_t(RS_TILE))
          ? size_t(RS_TILE) / padded
          : 1;
  const size_t total_tiles =
      spb > 1 ? (nstripes + spb - 1) / spb : tiles_per_shard * nstripes;
  /* seq_map: block walks consecutive tiles (long sequential bursts per
   * stream, DRAM row locality) instead of grid-striding */
  const size_t per_blk =
      seq_map ? (total_tiles + gridDim.x - 1) / gridDim.x : 0;
  const size_t t_lo = seq_map ? size_t(blockIdx.x) * per_blk : blockIdx.x;
  const size_t t_hi =
      seq_map ? (t_lo + per_blk < total_tiles ? t_lo + per_blk : total_tiles)
              : total_tiles;
  const size_t t_step = seq_map ? 1 : gridDim.x;

  for (size_t tile = t_lo; tile < t_hi; tile += t_step) {
    size_t stripe, off;
    if (spb > 1) {
      const size_t lane_b = size_t(threadIdx.x) * 16;
      const size_t sub = lane_b / padded;
      stripe = tile * spb + sub;
      off = lane_b - sub * padded;
      /* lanes past spb*padded (4096 is rarely a multiple of padded) would
       * land on the NEXT tile's first stripe: redundant today, a double
       * accumulate under xor_acc */
      if (sub >= spb || stripe >= nstripes) continue;
    } else {
      stripe = tile / tiles_per_shard;
      off = (tile - stripe * tiles_per_shard) * size_t(RS_TILE) +
            size_t(threadIdx.x) * 16;
    }
    bool mismatch = false;

    if (off + 16 <= shard_len) {
      /* exactly GM outputs per launch — the host splits larger m into
       * groups so there is no runtime bound inside the unrolled loops */
      uint4 acc[GM];
#pragma unroll
      for (int r = 0; r < GM; r++) {
        if (!VERIFY && xor_acc) {
          const uint8_t *out = addr.shard(stripe, out_idx[r], shard_len);
          acc[r] = *reinterpret_cast<const uint4 *>(out + off);
        } else {
          acc[r] = uint4{0, 0, 0, 0};
        }
      }
      /* issue up to KB=8 input loads before consuming any — 8 KiB of
       * HBM reads in flight per wave instead of one dependent load per
       * coefficient chain (memory-level parallelism, G7) */
      constexpr int KB = 8;
      for (int c0 = 0; c0 < k; c0 += KB) {
        uint4 v[KB];
#pragma unroll
        for (int j = 0; j < KB; j++) {
          if (c0 + j < k) {
            const uint8_t *in = addr.shard(stripe, in_idx[c0 + j], shard_len);
            v[j] = *reinterpret_cast<const uint4 *>(in + off);
          }
        }
#pragma unroll
        for (int j = 0; j < KB; j++) {
          if (c0 + j < k) {
            LinTab lt[GM];
#pragma unroll
            for (int r = 0; r < GM; r++)
              lt[r] = lintab_load(smem, r * k + c0 + j);
#pragma unroll
            for (int d = 0; d < 4; d++) {
              const uint32_t w = (&v[j].x)[d];
              const uint32_t s012 = w & 0x07070707u;
              const uint32_t s345 = (w >> 3) & 0x07070707u;
              const uint32_t s67 = (w >> 6) & 0x03030303u;
#pragma unroll
              for (int r = 0; r < GM; r++)
                (&acc[r].x)[d] ^= gfmul4_lin(s012, s345, s67, lt[r]);
            }
          }
        }
      }
#pragma unroll
      for (int r = 0; r < GM; r++) {
        uint8_t *out = const_cast<uint8_t *>(
            addr.shard(stripe, out_idx[r], shard_len));
        if (VERIFY || (cmp_mask >> r) & 1) {
          const uint4 e = *reinterpret_cast<const uint4 *>(out + off);
          mismatch |= (e.x != acc[r].x) | (e.y != acc[r].y) |
                      (e.z != acc[r].z) | (e.w != acc[r].w);
        } else {
          store16<NT>(out + off, acc[r]);
        }
      }
    } else if (off < shard_len) {
      /* ragged tail: per-byte path using the byte view of the LDS tables */
      const uint8_t *bt = smem;
      const size_t nb = shard_len - off;
      for (int og = 0; og < GM; og++) {
        const uint8_t *trow = bt + size_t(og * k) * 32;
        uint8_t *out =
            const_cast<uint8_t *>(addr.shard(stripe, out_idx[og], shard_len));
        for (size_t i = 0; i < nb; i++) {
          uint8_t v = (!VERIFY && xor_acc) ? out[off + i] : uint8_t(0);
          for (int c = 0; c < k; c++) {
            const uint8_t b = addr.shard(stripe, in_idx[c], shard_len)[off + i];
            v ^= gfmul1_lin(trow + size_t(c) * 32, b);
          }
          if (VERIFY || (cmp_mask >> og) & 1)
            mismatch |= (out[off + i] != v);
          else
            out[off + i] = v;
        }
      }
    }
    if (VERIFY || cmp_mask) {
      if (spb > 1) {
        /* a wave spans several packed stripes: lane 0's stripe is not the
         * mismatching lane's, so every lane reports its own */
        if (mismatch) atomicOr(&fail[stripe], 1u);
      } else if (__ballot(mismatch) != 0) {
        if ((threadIdx.x & 63) == 0) atomicOr(&fail[stripe], 1u);
      }
    }
  }
}

static int rs_grid(size_t shard_len, size_t nstripes) {
  const size_t tps = (shard_len + RS_TILE - 1) / RS_TILE;
  const size_t padded = (shard_len + 15) & ~size_t(15);
  size_t tiles;
  if (tps == 1 && padded * 2 <= size_t(RS_TILE))
    tiles = (nstripes + size_t(RS_TILE) / padded - 1) /
            (size_t(RS_TILE) / padded);
  else
    tiles = tps * nstripes;
  if (tiles == 0) tiles = 1;
  /* memory-bound: cap and grid-stride (cdna_hip_programming.md G11) */
  const size_t cap = size_t(env_grid("GFRS_RS_GRID", 256 * 64));
  return int(tiles < cap ? tiles : cap);
}

static bool perm0_ok() __attribute__((unused)); /* below (diagnostics only now) */

template <bool VERIFY, int GM>
static void rs_launch_one(const ShardAddr &a, const int32_t *in_idx, int k,
                          const int32_t *out_idx, const uint8_t *tabs,
                          size_t shard_len, int nstripes, uint32_t *fail,
                          hipStream_t s, int xor_acc = 0,
                          uint32_t cmp_mask = 0) {
  const int lds = k * GM * 32;
  const int grid = rs_grid(shard_len, nstripes);
  static const int seq = []() {
    const char *e = getenv("GFRS_RS_SEQ");
    return e ? atoi(e) : 0;
  }();
  if (nt_enabled() && !VERIFY && !xor_acc && !cmp_mask)
    hipLaunchKernelGGL((rs_apply_k<false, VERIFY, true, GM>), dim3(grid),
                       dim3(RS_BLOCK), lds, s, a, in_idx, k, out_idx, GM,
                       tabs, shard_len, size_t(nstripes), fail, xor_acc, seq,
                       cmp_mask);
  else
    hipLaunchKernelGGL((rs_apply_k<false, VERIFY, false, GM>), dim3(grid),
                       dim3(RS_BLOCK), lds, s, a, in_idx, k, out_idx, GM,
                       tabs, shard_len, size_t(nstripes), fail, xor_acc, seq,
                       cmp_mask);
}

/* Mixed write/compare strided apply: rows with cmp_mask bit set are
 * verified against the stored shard (fail[stripe] ORed on mismatch),
 * others written — one data pass for reconstruct+verify. */
void launch_rs_apply_mixed_strided(uint64_t base, uint64_t stripe_stride,
                                   const int32_t *in_idx, int k,
                                   const int32_t *out_idx, int nout,
                                   const uint8_t *tabs, uint32_t cmp_mask,
                                   size_t shard_len, int nstripes,
                                   uint32_t *fail, hipStream_t s) {
  ShardAddr a{nullptr, base, stripe_stride, 0};
  for (int og = 0; og < nout; og += MT) {
    const int gm = nout - og < MT ? nout - og : MT;
    const int32_t *oi = out_idx + og;
    const uint8_t *tb = tabs + size_t(og) * k * 32;
    const uint32_t m = (cmp_mask >> og) & ((1u << gm) - 1);
    switch (gm) {
      case 1: rs_launch_one<false, 1>(a, in_idx, k, oi, tb, shard_len,
                                      nstripes, fail, s, 0, m); break;
      case 2: rs_launch_one<false, 2>(a, in_idx, k, oi, tb, shard_len,
                                      nstripes, fail, s, 0, m); break;
      case 3: rs_launch_one<false, 3>(a, in_idx, k, oi, tb, shard_len,
                                      nstripes, fail, s, 0, m); break;
      default: rs_launch_one<false, 4>(a, in_idx, k, oi, tb, shard_len,
                                       nstripes, fail, s, 0, m);
    }
  }
}

/* ---- repair queue: per-job pattern and shard length ---- */

/* One bucket of a queue schedule (gfrs_plan.h): GM rows of each work item's
 * own plan over its own job.  Same math as rs_apply_k; what differs is where
 * a tile comes from:
 *  - the grid is capped and block b walks the CONTIGUOUS tile range
 *    [b*per_blk, (b+1)*per_blk) of the bucket, so with the items ordered by
 *    pattern a block rarely changes tables;
 *  - tile -> work item: one binary search over the tile prefix sums at the
 *    block's first tile, then a forward walk (every item has >= 1 tile).
 *    Everything involved depends on blockIdx and kernel arguments only, so
 *    the search, the item and the pattern descriptor are scalar loads;
 *  - the k*GM*32 bytes of tables are restaged into LDS only when the pattern
 *    or the row offset of the next tile differs from what is loaded, between
 *    two barriers.  The test is block-uniform and no lane leaves the loop
 *    body early, so every lane reaches both barriers;
 *  - a job shorter than a tile still takes a whole tile (no packing of
 *    small jobs; lanes past shard_len idle);
 *  - a block works on one job at a time, so the ballot form of the fail
 *    report is exact. */
template <int GM>
__global__ __launch_bounds__(RS_BLOCK) void rs_apply_queue_k(
    uint64_t base, const gfrs_qitem *__restrict__ items,
    const uint64_t *__restrict__ tile_prefix, uint32_t nitems,
    uint64_t total_tiles, const QueuePat *__restrict__ pats, int k,
    uint32_t *fail) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4 *ltab = reinterpret_cast<uint4 *>(smem); /* [k*GM*2] */

  const uint64_t per_blk = (total_tiles + gridDim.x - 1) / gridDim.x;
  const uint64_t t_lo = uint64_t(blockIdx.x) * per_blk;
  const uint64_t t_hi =
      t_lo + per_blk < total_tiles ? t_lo + per_blk : total_tiles;
  if (t_lo >= t_hi) return; /* whole block, before any barrier */

  /* largest it with tile_prefix[it] <= t_lo (tile_prefix[0] == 0) */
  uint32_t it = 0;
  for (uint32_t hi = nitems; hi - it > 1;) {
    const uint32_t mid = it + (hi - it) / 2;
    if (tile_prefix[mid] <= t_lo)
      it = mid;
    else
      hi = mid;
  }

  /* the index lists arrive as pointers read from the descriptor table:
   * the constant address space keeps their (block-uniform) reads scalar,
   * as they are in rs_apply_k where the lists are kernel arguments */
  typedef const __attribute__((address_space(4))) int32_t *IdxList;
  int cur_pat = -1, cur_row = -1;
  IdxList in_idx = nullptr, out_idx = nullptr;
  uint32_t cmp_mask = 0;

  for (uint64_t tile = t_lo; tile < t_hi; tile++) {
    while (tile_prefix[it + 1] <= tile) it++; /* it + 1 <= nitems */
    const gfrs_qitem item = items[it];
    const size_t shard_len = item.shard_len;
    const uint64_t job_base = base + item.off;
    if (item.pattern != cur_pat || item.row_off != cur_row) {
      const QueuePat pat = pats[item.pattern];
      __syncthreads(); /* all lanes are done with the old tables */
      const uint4 *src = reinterpret_cast<const uint4 *>(as_global(
          uint64_t(pat.tabs) + uint64_t(item.row_off) * k * 32));
      for (int i = threadIdx.x; i < k * GM * 2; i += RS_BLOCK)
        ltab[i] = src[i];
      __syncthreads();
      cur_pat = item.pattern;
      cur_row = item.row_off;
      in_idx = (IdxList)(uint64_t)pat.in_idx;
      out_idx = (IdxList)(uint64_t)(pat.out_idx + item.row_off);
      cmp_mask = (pat.cmp_mask >> item.row_off) & ((1u << GM) - 1);
    }
    const size_t off = size_t(tile - tile_prefix[it]) * size_t(RS_TILE) +
                       size_t(threadIdx.x) * 16;
    bool mismatch = false;

    if (off + 16 <= shard_len) {
      uint4 acc[GM];
#pragma unroll
      for (int r = 0; r < GM; r++) acc[r] = uint4{0, 0, 0, 0};
      constexpr int KB = 8; /* input loads in flight, as in rs_apply_k */
      for (int c0 = 0; c0 < k; c0 += KB) {
        uint4 v[KB];
#pragma unroll
        for (int j = 0; j < KB; j++) {
          if (c0 + j < k) {
            const uint8_t *in =
                as_global(job_base + uint64_t(in_idx[c0 + j]) * shard_len);
            v[j] = *reinterpret_cast<const uint4 *>(in + off);
          }
        }
#pragma unroll
        for (int j = 0; j < KB; j++) {
          if (c0 + j < k) {
            LinTab lt[GM];
#pragma unroll
            for (int r = 0; r < GM; r++)
              lt[r] = lintab_load(smem, r * k + c0 + j);
#pragma unroll
            for (int d = 0; d < 4; d++) {
              const uint32_t w = (&v[j].x)[d];
              const uint32_t s012 = w & 0x07070707u;
              const uint32_t s345 = (w >> 3) & 0x07070707u;
              const uint32_t s67 = (w >> 6) & 0x03030303u;
#pragma unroll
              for (int r = 0; r < GM; r++)
                (&acc[r].x)[d] ^= gfmul4_lin(s012, s345, s67, lt[r]);
            }
          }
        }
      }
#pragma unroll
      for (int r = 0; r < GM; r++) {
        uint8_t *out = const_cast<uint8_t *>(
            as_global(job_base + uint64_t(out_idx[r]) * shard_len));
        if ((cmp_mask >> r) & 1) {
          const uint4 e = *reinterpret_cast<const uint4 *>(out + off);
          mismatch |= (e.x != acc[r].x) | (e.y != acc[r].y) |
                      (e.z != acc[r].z) | (e.w != acc[r].w);
        } else {
          store16<false>(out + off, acc[r]);
        }
      }
    } else if (off < shard_len) {
      /* ragged tail: per-byte path using the byte view of the LDS tables */
      const size_t nb = shard_len - off;
      for (int og = 0; og < GM; og++) {
        const uint8_t *trow = smem + size_t(og * k) * 32;
        uint8_t *out = const_cast<uint8_t *>(
            as_global(job_base + uint64_t(out_idx[og]) * shard_len));
        for (size_t i = 0; i < nb; i++) {
          uint8_t v = 0;
          for (int c = 0; c < k; c++) {
            const uint8_t b = as_global(
                job_base + uint64_t(in_idx[c]) * shard_len)[off + i];
            v ^= gfmul1_lin(trow + size_t(c) * 32, b);
          }
          if ((cmp_mask >> og) & 1)
            mismatch |= (out[off + i] != v);
          else
            out[off + i] = v;
        }
      }
    }
    if (cmp_mask && __ballot(mismatch) != 0) {
      if ((threadIdx.x & 63) == 0) atomicOr(&fail[item.job], 1u);
    }
  }
}

template <int GM>
static void rs_queue_launch_one(uint64_t base, const gfrs_qitem *items,
                                const uint64_t *tile_prefix, uint32_t nitems,
                                uint64_t total_tiles, const QueuePat *pats,
                                int k, uint32_t *fail, hipStream_t s) {
  /* the cap of rs_grid, so GFRS_RS_GRID forces the multi-tile walk and the
   * restage path at tiny shapes */
  const uint64_t cap = uint64_t(env_grid("GFRS_RS_GRID", 256 * 64));
  const int grid = int(total_tiles < cap ? total_tiles : cap);
  hipLaunchKernelGGL((rs_apply_queue_k<GM>), dim3(grid), dim3(RS_BLOCK),
                     k * GM * 32, s, base, items, tile_prefix, nitems,
                     total_tiles, pats, k, fail);
}

void launch_rs_apply_queue(uint64_t base, const gfrs_qitem *items,
                           const uint64_t *tile_prefix, uint32_t nitems,
                           uint64_t total_tiles, const QueuePat *pats, int k,
                           int gm, uint32_t *fail, hipStream_t s) {
  if (nitems == 0 || total_tiles == 0) return;
  switch (gm) {
    case 1: rs_queue_launch_one<1>(base, items, tile_prefix, nitems,
                                   total_tiles, pats, k, fail, s); break;
    case 2: rs_queue_launch_one<2>(base, items, tile_prefix, nitems,
                                   total_tiles, pats, k, fail, s); break;
    case 3: rs_queue_launch_one<3>(base, items, tile_prefix, nitems,
                                   total_tiles, pats, k, fail, s); break;
    default: rs_queue_launch_one<4>(base, items, tile_prefix, nitems,
                                    total_tiles, pats, k, fail, s);
  }
}

/* EncodeIdx-style accumulate apply: out[r] ^= coeff[r]*in (one input). */
void launch_rs_apply_xor(const uint64_t *ptrs, int nptr,
                         const int32_t *in_idx, int k,
                         const int32_t *out_idx, int nout,
                         const uint8_t *tabs, size_t shard_len, int nstripes,
                         hipStream_t s) {
  ShardAddr a{ptrs, 0, 0, nptr};
  for (int og = 0; og < nout; og += MT) {
    const int gm = nout - og < MT ? nout - og : MT;
    const int32_t *oi = out_idx + og;
    const uint8_t *tb = tabs + size_t(og) * k * 32;
    switch (gm) {
      case 1: rs_launch_one<false, 1>(a, in_idx, k, oi, tb, shard_len,
                                      nstripes, nullptr, s, 1); break;
      case 2: rs_launch_one<false, 2>(a, in_idx, k, oi, tb, shard_len,
                                      nstripes, nullptr, s, 1); break;
      case 3: rs_launch_one<false, 3>(a, in_idx, k, oi, tb, shard_len,
                                      nstripes, nullptr, s, 1); break;
      default: rs_launch_one<false, 4>(a, in_idx, k, oi, tb, shard_len,
                                       nstripes, nullptr, s, 1);
    }
  }
}

template <bool VERIFY>
static void rs_dispatch(const ShardAddr &a, const int32_t *in_idx, int k,
                        const int32_t *out_idx, int nout, const uint8_t *tabs,
                        size_t shard_len, int nstripes, uint32_t *fail,
                        hipStream_t s) {
  /* split outputs into groups of <= MT; each launch has a compile-time
   * group size so the inner loops carry no runtime bounds */
  for (int og = 0; og < nout; og += MT) {
    const int gm = nout - og < MT ? nout - og : MT;
    const int32_t *oi = out_idx + og;
    const uint8_t *tb = tabs + size_t(og) * k * 32;
    switch (gm) {
      case 1:
        rs_launch_one<VERIFY, 1>(a, in_idx, k, oi, tb, shard_len, nstripes,
                                 fail, s);
        break;
      case 2:
        rs_launch_one<VERIFY, 2>(a, in_idx, k, oi, tb, shard_len, nstripes,
                                 fail, s);
        break;
      case 3:
        rs_launch_one<VERIFY, 3>(a, in_idx, k, oi, tb, shard_len, nstripes,
                                 fail, s);
        break;
      default:
        rs_launch_one<VERIFY, 4>(a, in_idx, k, oi, tb, shard_len, nstripes,
                                 fail, s);
    }
  }
}

void launch_rs_apply(const uint64_t *ptrs, int nptr, const int32_t *in_idx,
                     int k, const int32_t *out_idx, int nout,
                     const uint8_t *tabs, size_t shard_len, int nstripes,
                     hipStream_t s) {
  ShardAddr a{ptrs, 0, 0, nptr};
  rs_dispatch<false>(a, in_idx, k, out_idx, nout, tabs, shard_len, nstripes,
                     nullptr, s);
}

void launch_rs_apply_strided(uint64_t base, uint64_t stripe_stride,
                             const int32_t *in_idx, int k,
                             const int32_t *out_idx, int nout,
                             const uint8_t *tabs, size_t shard_len,
                             int nstripes, hipStream_t s) {
  ShardAddr a{nullptr, base, stripe_stride, 0};
  rs_dispatch<false>(a, in_idx, k, out_idx, nout, tabs, shard_len, nstripes,
                     nullptr, s);
}

void launch_rs_verify(const uint64_t *ptrs, int nptr, const int32_t *in_idx,
                      int k, const int32_t *out_idx, int nout,
                      const uint8_t *tabs, size_t shard_len, int nstripes,
                      uint32_t *fail, hipStream_t s) {
  ShardAddr a{ptrs, 0, 0, nptr};
  rs_dispatch<true>(a, in_idx, k, out_idx, nout, tabs, shard_len, nstripes,
                    fail, s);
}

void launch_rs_verify_strided(uint64_t base, uint64_t stripe_stride,
                              const int32_t *in_idx, int k,
                              const int32_t *out_idx, int nout,
                              const uint8_t *tabs, size_t shard_len,
                              int nstripes, uint32_t *fail, hipStream_t s) {
  ShardAddr a{nullptr, base, stripe_stride, 0};
  rs_dispatch<true>(a, in_idx, k, out_idx, nout, tabs, shard_len, nstripes,
                    fail, s);
}

/* ------------------------------------------------------------------ */
/* v_perm semantics probe                                               */
/* ------------------------------------------------------------------ */

__global__ void probe_perm_k(uint32_t *out) {
  if (threadIdx.x == 0) {
    out[0] = __builtin_amdgcn_perm(0x44332211u, 0x88776655u, 0x03020100u);
    out[1] = __builtin_amdgcn_perm(0x44332211u, 0x88776655u, 0x07060504u);
    out[2] = __builtin_amdgcn_perm(0xAABBCCDDu, 0x11223344u, 0x0B0A0908u);
    out[3] = __builtin_amdgcn_perm(0xAABBCCDDu, 0x11223344u, 0x0F0E0D0Cu);
    out[4] = __builtin_amdgcn_perm(0x80808080u, 0x7F7F7F7Fu, 0x0B0A0908u);
  }
}

static int g_perm0 = -1; /* -1 unknown, 0 safe path, 1 fast path */

int probe_perm_device(void) {
  uint32_t *d = nullptr;
  uint32_t h[5] = {1, 1, 1, 1, 1};
  if (hipMalloc(&d, sizeof(h)) != hipSuccess) return -100;
  hipLaunchKernelGGL(probe_perm_k, dim3(1), dim3(64), 0, nullptr, d);
  if (hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) {
    hipFree(d);
    return -100;
  }
  hipFree(d);
  /* expected: sel 0-3 -> second operand's bytes, 4-7 -> first operand's,
   * >=8 -> 0x00 */
  const bool order_ok = (h[0] == 0x88776655u) && (h[1] == 0x44332211u);
  if (!order_ok) return -103; /* would need a different lut16 — flag loudly */
  fprintf(stderr,
          "gfrs perm probe: sel8-11(lo=0x11223344,hi=0xAABBCCDD)=%08x "
          "sel12-15=%08x sel8-11(sign)=%08x\n", h[2], h[3], h[4]);
  g_perm0 = (h[2] == 0u) ? 1 : 0;
  return g_perm0;
}

static bool perm0_ok() {
  if (g_perm0 < 0) {
    int r = probe_perm_device();
    if (r < 0) g_perm0 = 0; /* safe path */
  }
  return g_perm0 == 1;
}

/* ------------------------------------------------------------------ */
/* crc32block                                                           */
/* ------------------------------------------------------------------ */

#define CRC_POLY 0xEDB88320u
#define CRC_LEN 4

/* slice-by-8 tables (zlib BYFOUR construction extended), host-computed,
 * copied per device.  tab[0] is the base byte table. */
__device__ uint32_t g_crc_tab4[8][256];
/* multiply a reflected CRC value by x^(8*4096): byte-sliced tables so the
 * register-CRC fused kernel can Horner-chain a lane's four 4096-apart
 * uint4 pieces with 4 LDS gathers per step instead of a 32-step mulmod */
__device__ uint32_t g_shift4k[4][256];
/* same, for x^(8*1024): the small-shard fused kernel's piece stride */
__device__ uint32_t g_shift1k[4][256];
/* and x^(8*8192): the 32-B-piece dual-aligned kernel's lane stride */
__device__ uint32_t g_shift8k[4][256];
/* and x^(8*13312): the aligned kernel's step from a lane's last piece of one
 * pass to its first piece of the next (16384 - 3 * 1024 bytes) */
__device__ uint32_t g_shift13k[4][256];

/* x^(8*2^j) mod P, reflected domain — host-filled alongside the tables. */
__device__ uint32_t g_pow8[40];

/* reflected-domain carry-less multiply mod P (see oracle/crc_ref.c for the
 * derivation; independent implementation). */
GFRS_DEV int64_t i64min(int64_t a, int64_t b) { return a < b ? a : b; }

GFRS_DEV uint32_t gf2_mulmod_d(uint32_t a, uint32_t b) {
  uint32_t prod = 0;
#pragma unroll 8
  for (int i = 31; i >= 0; i--) {
    if ((a >> i) & 1) prod ^= b;
    b = (b & 1) ? (b >> 1) ^ CRC_POLY : (b >> 1);
  }
  return prod;
}

/* x^(8*len) mod P via binary expansion of len. */
GFRS_DEV uint32_t x8n_d(uint64_t len) {
  uint32_t op = 0x80000000u; /* identity */
  int j = 0;
  while (len) {
    if (len & 1) op = gf2_mulmod_d(op, g_pow8[j]);
    len >>= 1;
    j++;
  }
  return op;
}

constexpr int CRC_BLOCKT = 256;

GFRS_DEV uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96); /* a ^ b ^ c */
}

/* raw CRC of 16 bytes held in a register uint4 (slice-by-8, 2 steps) */
GFRS_DEV uint32_t crc16_reg(const uint4 q, const uint32_t (*tab)[256]) {
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const uint32_t w0 = (j == 0 ? q.x : q.z) ^ c;
    const uint32_t w1 = (j == 0 ? q.y : q.w);
    c = xor3(xor3(tab[7][w0 & 0xFF], tab[6][(w0 >> 8) & 0xFF],
                  tab[5][(w0 >> 16) & 0xFF]),
             xor3(tab[4][w0 >> 24], tab[3][w1 & 0xFF],
                  tab[2][(w1 >> 8) & 0xFF]),
             tab[1][(w1 >> 16) & 0xFF] ^ tab[0][w1 >> 24]);
  }
  return c;
}

/* u(q) = q(x) mod P of 16 bytes held in a register uint4: crc16_reg
 * without its last x^32, so crc16_reg(q) = u(q) * x^32.  The first two
 * dwords reduce over tab[7..0] (8 independent gathers), the third joins
 * and reduces over tab[3..0] (4 gathers), the fourth enters as it stands.
 * A caller that Horner-chains u values and multiplies the chain by x^(8n)
 * uses x^(8(n+4)) instead: 12 gathers per piece, not 16. */
GFRS_DEV uint32_t crc12u_reg(const uint4 q, const uint32_t (*tab)[256]) {
  const uint32_t c =
      xor3(xor3(tab[7][q.x & 0xFF], tab[6][(q.x >> 8) & 0xFF],
                tab[5][(q.x >> 16) & 0xFF]),
           xor3(tab[4][q.x >> 24], tab[3][q.y & 0xFF],
                tab[2][(q.y >> 8) & 0xFF]),
           tab[1][(q.y >> 16) & 0xFF] ^ tab[0][q.y >> 24]);
  const uint32_t w = c ^ q.z;
  return xor3(xor3(tab[3][w & 0xFF], tab[2][(w >> 8) & 0xFF],
                   tab[1][(w >> 16) & 0xFF]),
              tab[0][w >> 24], q.w);
}

GFRS_DEV uint32_t shift4k(uint32_t c, const uint32_t (*stab)[256]) {
  return xor3(stab[0][c & 0xFF], stab[1][(c >> 8) & 0xFF],
              stab[2][(c >> 16) & 0xFF]) ^
         stab[3][c >> 24];
}

/* Raw (no init/final complement) CRC update of a chunk, 4 B at a time via
 * LDS slice-by-4 tables, byte tail scalar.  When dst != nullptr the chunk
 * is simultaneously copied there (the frame/strip move fused into the CRC
 * pass so the payload crosses HBM exactly once each way). */
GFRS_DEV uint32_t crc_chunk(const uint8_t *p, int len,
                            const uint32_t (*tab)[256], uint8_t *dst) {
  uint32_t c = 0;
  int i = 0;
  for (; i + 4 <= len; i += 4) {
    const uint32_t w = *reinterpret_cast<const uint32_t *>(p + i);
    if (dst) *reinterpret_cast<uint32_t *>(dst + i) = w;
    c ^= w;
    c = tab[3][c & 0xFF] ^ tab[2][(c >> 8) & 0xFF] ^ tab[1][(c >> 16) & 0xFF] ^
        tab[0][c >> 24];
  }
  for (; i < len; i++) {
    if (dst) dst[i] = p[i];
    c = tab[0][(c ^ p[i]) & 0xFF] ^ (c >> 8);
  }
  return c;
}

/* Slice-by-4 CRC over a 16-B-aligned LDS chunk using uint4 reads
 * (ds_read_b128, conflict-free with the 272 B stage stride) — 4x fewer
 * LDS instructions than the byte-pointer path. */
GFRS_DEV uint32_t crc_chunk16(const uint8_t *p, int len,
                              const uint32_t (*tab)[256]) {
  /* slice-by-8: one chained step per 8 B (the 8 gathers within a step are
   * independent, so the serial chain is half as deep as slice-by-4) */
  uint32_t c = 0;
  int i = 0;
  for (; i + 16 <= len; i += 16) {
    const uint4 q = *reinterpret_cast<const uint4 *>(p + i);
#pragma unroll
    for (int j = 0; j < 2; j++) {
      const uint32_t w0 = (j == 0 ? q.x : q.z) ^ c;
      const uint32_t w1 = (j == 0 ? q.y : q.w);
      c = xor3(xor3(tab[7][w0 & 0xFF], tab[6][(w0 >> 8) & 0xFF],
                    tab[5][(w0 >> 16) & 0xFF]),
               xor3(tab[4][w0 >> 24], tab[3][w1 & 0xFF],
                    tab[2][(w1 >> 8) & 0xFF]),
               tab[1][(w1 >> 16) & 0xFF] ^ tab[0][w1 >> 24]);
    }
  }
  for (; i + 4 <= len; i += 4) {
    c ^= *reinterpret_cast<const uint32_t *>(p + i);
    c = tab[3][c & 0xFF] ^ tab[2][(c >> 8) & 0xFF] ^ tab[1][(c >> 16) & 0xFF] ^
        tab[0][c >> 24];
  }
  for (; i < len; i++) c = tab[0][(c ^ p[i]) & 0xFF] ^ (c >> 8);
  return c;
}

/* One workgroup per frame.  MODE: 0 = encode (raw src -> framed dst),
 * 1 = verify (framed src), 2 = decode (framed src -> raw dst). */
template <int MODE, bool TAILCRC = false>
__global__ __launch_bounds__(CRC_BLOCKT) void crc32b_k(
    uint8_t *__restrict__ dst, size_t dst_stride,
    const uint8_t *__restrict__ src, size_t src_stride, int64_t n,
    int64_t block_len, int64_t frames_per_shard, int64_t total_frames,
    int64_t *__restrict__ bad) {
  __shared__ uint32_t tab[8][256];
  __shared__ uint32_t fold[CRC_BLOCKT];
  for (int i = threadIdx.x; i < 2048; i += CRC_BLOCKT)
    (&tab[0][0])[i] = (&g_crc_tab4[0][0])[i];
  __syncthreads();

  const int64_t payload_full = block_len - CRC_LEN;
  /* per-thread chunk: covers any block_len; multiple of 4 so every chunk
   * start stays u32-aligned */
  const int64_t chunk =
      (((payload_full + CRC_BLOCKT - 1) / CRC_BLOCKT) + 3) & ~int64_t(3);
  /* full-frame fold operator depends only on the chunk position */
  const int64_t cend_full =
      i64min(i64min(int64_t(threadIdx.x) * chunk, payload_full) + chunk,
             payload_full);
  const uint32_t my_op_full = x8n_d(uint64_t(payload_full - cend_full));
  const uint32_t init_full =
      gf2_mulmod_d(x8n_d(uint64_t(payload_full)), 0xFFFFFFFFu);

  for (int64_t fr = blockIdx.x; fr < total_frames; fr += gridDim.x) {
    const int64_t shard = fr / frames_per_shard;
    const int64_t f = fr - shard * frames_per_shard;
    /* n = raw bytes per shard (encode) or derived from framed_len; the
     * launcher always passes raw payload total in n. */
    const int64_t praw0 = f * payload_full;
    const int64_t payload = i64min(payload_full, n - praw0);

    const uint8_t *sbase = src + shard * src_stride;
    uint8_t *dbase = dst ? dst + shard * dst_stride : nullptr;
    /* chunk for this thread */
    const int64_t c0 = int64_t(threadIdx.x) * chunk;
    int clen = int(i64min(chunk, payload - c0));
    if (clen < 0) clen = 0;
    const int64_t hdr_off = TAILCRC ? 0 : CRC_LEN;
    const uint8_t *payload_src =
        (MODE == 0) ? sbase + praw0 : sbase + f * block_len + hdr_off;
    uint8_t *payload_dst = nullptr;
    if (MODE == 0) payload_dst = dbase + f * block_len + hdr_off + c0;
    if (MODE == 2) payload_dst = dbase + praw0 + c0;

    uint32_t part = crc_chunk(payload_src + c0, clen, tab, payload_dst);
    /* fold: contribution = part * x^(8*suffix) */
    uint32_t op = my_op_full, init_term = init_full;
    if (payload != payload_full) { /* tail frame only */
      const int64_t suffix = clen > 0 ? payload - (c0 + clen) : 0;
      op = x8n_d(uint64_t(suffix));
      init_term = gf2_mulmod_d(x8n_d(uint64_t(payload)), 0xFFFFFFFFu);
    }
    part = clen > 0 ? gf2_mulmod_d(op, part) : 0;
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) part ^= __shfl_xor(part, sh, 64);
    if ((threadIdx.x & 63) == 0) fold[threadIdx.x >> 6] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
      /* crc = ~( x^(8*payload)·(~0) ^ fold )  — see DESIGN.md */
      const uint32_t raw =
          init_term ^ fold[0] ^ fold[1] ^ fold[2] ^ fold[3];
      const uint32_t crc = ~raw;
      uint8_t *hw = dbase ? dbase + f * block_len + (TAILCRC ? payload : 0)
                          : nullptr;
      const uint8_t *hr = sbase + f * block_len + (TAILCRC ? payload : 0);
      if (MODE == 0) {
        if (TAILCRC) { /* BE (sized_coder.go) */
          hw[0] = uint8_t(crc >> 24); hw[1] = uint8_t(crc >> 16);
          hw[2] = uint8_t(crc >> 8); hw[3] = uint8_t(crc);
        } else {
          *reinterpret_cast<uint32_t *>(hw) = crc;
        }
      } else {
        uint32_t want;
        if (TAILCRC)
          want = (uint32_t(hr[0]) << 24) | (uint32_t(hr[1]) << 16) |
                 (uint32_t(hr[2]) << 8) | uint32_t(hr[3]);
        else
          __builtin_memcpy(&want, hr, 4); /* LE load */
        if (want != crc)
          atomicMin(reinterpret_cast<unsigned long long *>(&bad[shard]),
                    static_cast<unsigned long long>(f));
      }
    }
    __syncthreads();
  }
}

static int crc_grid(int64_t total_frames, int64_t frames_per_shard) {
  if (total_frames <= 0) return 1;
  const int64_t cap = env_grid("GFRS_CRC_GRID", 256 * 8);
  int64_t g = total_frames < cap ? total_frames : cap;
  /* keep the stride coprime with fps so blocks see a mix of frame
   * positions (see fused_grid) */
  if (g < total_frames && frames_per_shard > 1)
    while (g > 1) {
      int64_t a = g, b = frames_per_shard;
      while (b) { int64_t t2 = a % b; a = b; b = t2; }
      if (a == 1) break;
      g--;
    }
  return int(g);
}

/* the pipelined fused kernels prefer many more blocks than the staged
 * CRC kernels: measured @512 stripes RS(6+3), grid 2048 -> 20.0 ms,
 * 8192-32768 -> 19.2-19.5 ms (better tail balance; the cross-frame
 * prefetch only helps within a block's own frame sequence) */
static int fused_grid(int64_t total_frames, int64_t frames_per_shard) {
  if (total_frames <= 0) return 1;
  const int64_t cap = env_grid("GFRS_CRC_GRID", 16384);
  int64_t g = total_frames < cap ? total_frames : cap;
  /* grid-stride must not alias the frame position within a shard, or
   * whole blocks end up with only the (tiny) last frames: with 64 KiB
   * shards (fps=2) an even grid halves effective parallelism (measured
   * 770 vs 1182 GiB/s).  Make the stride coprime with fps. */
  auto gcd = [](int64_t a, int64_t b) {
    while (b) { int64_t t2 = a % b; a = b; b = t2; }
    return a;
  };
  if (g < total_frames && frames_per_shard > 1)
    while (g > 1 && gcd(g, frames_per_shard) != 1) g--;
  return int(g);
}

/* LDS-staged crc32block kernel for the production 64 KiB block: the
 * whole frame is staged through LDS so every global access is coalesced —
 * read the payload once (fused copy to dst for encode/decode), CRC the
 * 256 B chunks out of LDS (chunk stride 272 B keeps ds_read_b128
 * conflict-free: lane t hits dword banks 68t+4i mod 64, distinct within
 * each 16-lane group).  Traffic = S read + S write, the algorithmic
 * minimum. */
/* Small-payload crc32block kernel: shards of at most 16 KiB produce one
 * short frame each; a 256-lane workgroup per frame would idle most lanes
 * (2 KiB MinShardSize shapes!).  Here each WAVE owns one frame: lane
 * chunks are ceil(pay/64) rounded to 4 B, reduction is wave-local
 * shfl_xor, there is no LDS staging and no barrier in the frame loop
 * (short frames are line-local; L1/L2 absorb the per-lane strides). */
template <int MODE, bool TAILCRC>
__global__ __launch_bounds__(CRC_BLOCKT) void crc32b_small_k(
    uint8_t *__restrict__ dst, size_t dst_stride,
    const uint8_t *__restrict__ src, size_t src_stride, int64_t n,
    int64_t block_len, int64_t total_frames, int64_t *__restrict__ bad) {
  __shared__ uint32_t tab[8][256];
  for (int i = threadIdx.x; i < 2048; i += CRC_BLOCKT)
    (&tab[0][0])[i] = (&g_crc_tab4[0][0])[i];
  __syncthreads();
  const int64_t payload = n; /* frames_per_shard == 1 */
  const int64_t chunk = ((payload + 63) / 64 + 3) & ~int64_t(3);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t c0 = int64_t(lane) * chunk;
  int clen = int(i64min(chunk, payload - c0));
  if (clen < 0) clen = 0;
  const uint32_t my_op =
      x8n_d(uint64_t(clen > 0 ? payload - (c0 + clen) : 0));
  const uint32_t init_term =
      gf2_mulmod_d(x8n_d(uint64_t(payload)), 0xFFFFFFFFu);

  const int64_t waves_total = int64_t(gridDim.x) * 4;
  for (int64_t fr = int64_t(blockIdx.x) * 4 + wave; fr < total_frames;
       fr += waves_total) {
    const int64_t shard = fr; /* one frame per shard */
    const uint8_t *psrc =
        (MODE == 0) ? src + shard * src_stride
                    : src + shard * src_stride + (TAILCRC ? 0 : CRC_LEN);
    uint8_t *pdst = nullptr;
    if (MODE == 0)
      pdst = dst + shard * dst_stride + (TAILCRC ? 0 : CRC_LEN);
    if (MODE == 2) pdst = dst + shard * dst_stride;

    uint32_t part = clen > 0
                        ? crc_chunk(psrc + c0, clen, tab,
                                    (MODE != 1 && pdst) ? pdst + c0 : nullptr)
                        : 0;
    part = clen > 0 ? gf2_mulmod_d(my_op, part) : 0;
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) part ^= __shfl_xor(part, sh, 64);
    if (lane == 0) {
      const uint32_t crc = ~(init_term ^ part);
      const int64_t hpos = TAILCRC ? payload : 0;
      if (MODE == 0) {
        uint8_t *h = dst + shard * dst_stride + hpos;
        if (TAILCRC) {
          h[0] = uint8_t(crc >> 24); h[1] = uint8_t(crc >> 16);
          h[2] = uint8_t(crc >> 8); h[3] = uint8_t(crc);
        } else {
          *reinterpret_cast<uint32_t *>(h) = crc;
        }
      } else {
        const uint8_t *h = src + shard * src_stride + hpos;
        uint32_t want;
        if (TAILCRC)
          want = (uint32_t(h[0]) << 24) | (uint32_t(h[1]) << 16) |
                 (uint32_t(h[2]) << 8) | uint32_t(h[3]);
        else
          __builtin_memcpy(&want, h, 4);
        if (want != crc)
          atomicMin(reinterpret_cast<unsigned long long *>(&bad[shard]), 0ull);
      }
    }
  }
}

/* Stage-pass chunk size trades LDS footprint (blocks/CU, latency overlap)
 * against barrier count: 256 -> 1 pass/frame, 2 blocks/CU; 128 -> 2
 * passes, 3 blocks/CU; 64 -> 4 passes, 6 blocks/CU (measured best);
 * 32 -> 8 passes, 8 blocks/CU.  GFRS_CRC_CHUNK overrides (default 64). */
template <int CHUNK> struct StgGeom {
  static constexpr int STRIDE = CHUNK + 16;
  static constexpr int HALF = 256 * CHUNK; /* payload bytes per pass */
  static constexpr int PASSES = (65532 + HALF - 1) / HALF;
  static constexpr int LDS = 8192 + 1024 + 256 * STRIDE;
};

template <int MODE, bool NT, bool TAILCRC, int CHUNK>
__global__ __launch_bounds__(CRC_BLOCKT) void crc32b_staged_k(
    uint8_t *__restrict__ dst, size_t dst_stride,
    const uint8_t *__restrict__ src, size_t src_stride, int64_t n,
    int64_t frames_per_shard, int64_t total_frames, int64_t *__restrict__ bad) {
  constexpr int64_t block_len = 65536;
  constexpr int64_t payload_full = block_len - CRC_LEN;
  using G = StgGeom<CHUNK>;
  constexpr int STG_CHUNK = CHUNK;
  constexpr int STG_STRIDE = G::STRIDE;
  constexpr int STG_HALF = G::HALF;
  constexpr int STG_PASSES = G::PASSES;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t(*tab)[256] = reinterpret_cast<uint32_t(*)[256]>(smem);
  uint32_t *fold = reinterpret_cast<uint32_t *>(smem + 8192);
  uint8_t *stage = smem + 8192 + 1024; /* 256 chunk slots x STRIDE B */
  for (int i = threadIdx.x; i < 2048; i += CRC_BLOCKT)
    (&tab[0][0])[i] = (&g_crc_tab4[0][0])[i];
  /* fold operators are a function of the thread's chunk positions only
   * for the block's UNIFORM frame payload (the full 65,532 B, or the
   * single short frame when every shard has one frame) — computed once
   * per block, not per frame */
  const int64_t pf_uniform =
      frames_per_shard == 1 ? i64min(payload_full, n) : payload_full;
  uint32_t op_full[STG_PASSES];
#pragma unroll
  for (int h = 0; h < STG_PASSES; h++) {
    const int64_t c0 =
        int64_t(h) * STG_HALF + int64_t(threadIdx.x) * STG_CHUNK;
    const int64_t cend = i64min(i64min(c0 + STG_CHUNK, pf_uniform),
                                c0 > pf_uniform ? c0 : pf_uniform);
    op_full[h] = x8n_d(uint64_t(pf_uniform - (cend > c0 ? cend : c0)));
  }
  const uint32_t init_full =
      gf2_mulmod_d(x8n_d(uint64_t(pf_uniform)), 0xFFFFFFFFu);
  __syncthreads();

  for (int64_t fr = blockIdx.x; fr < total_frames; fr += gridDim.x) {
    const int64_t shard = fr / frames_per_shard;
    const int64_t f = fr - shard * frames_per_shard;
    const int64_t praw0 = f * payload_full;
    const int64_t payload = i64min(payload_full, n - praw0);
    const uint8_t *sbase = src + shard * src_stride;
    uint8_t *dbase = dst ? dst + shard * dst_stride : nullptr;
    /* sized frames (sized_coder.go:256-279) put the CRC AFTER the
     * payload, big-endian; block frames put it first, little-endian */
    const int64_t hdr_off = TAILCRC ? 0 : CRC_LEN;
    const uint8_t *psrc =
        (MODE == 0) ? sbase + praw0 : sbase + f * block_len + hdr_off;
    uint8_t *pdst = nullptr;
    if (MODE == 0) pdst = dbase + f * block_len + hdr_off;
    if (MODE == 2) pdst = dbase + praw0;

    /* two half-frame passes: stage 32 KiB (coalesced, fused copy out),
     * CRC the 128 B chunks out of LDS */
    uint32_t acc = 0;
    const uint32_t init_term =
        payload == pf_uniform
            ? init_full
            : gf2_mulmod_d(x8n_d(uint64_t(payload)), 0xFFFFFFFFu);
#pragma unroll
    for (int h = 0; h < STG_PASSES; h++) {
      const int64_t h0 = int64_t(h) * STG_HALF;
      const int64_t hbytes = i64min(int64_t(STG_HALF), payload - h0);
      if (hbytes <= 0) break;
      const int64_t words = hbytes >> 2;
      for (int64_t w = threadIdx.x; w < words; w += CRC_BLOCKT) {
        const uint32_t x =
            *reinterpret_cast<const uint32_t *>(psrc + h0 + 4 * w);
        if (MODE != 1) {
          if (NT)
            __builtin_nontemporal_store(
                x, reinterpret_cast<uint32_t *>(pdst + h0 + 4 * w));
          else
            *reinterpret_cast<uint32_t *>(pdst + h0 + 4 * w) = x;
        }
        const int64_t p = 4 * w;
        *reinterpret_cast<uint32_t *>(
            &stage[(p / STG_CHUNK) * STG_STRIDE + (p & (STG_CHUNK - 1))]) = x;
      }
      if (threadIdx.x == 0)
        for (int64_t p = words * 4; p < hbytes; p++) {
          const uint8_t x = psrc[h0 + p];
          if (MODE != 1) pdst[h0 + p] = x;
          stage[(p / STG_CHUNK) * STG_STRIDE + (p & (STG_CHUNK - 1))] = x;
        }
      __syncthreads();
      const int64_t c0 = int64_t(threadIdx.x) * STG_CHUNK;
      int clen = int(i64min(int64_t(STG_CHUNK), hbytes - c0));
      if (clen < 0) clen = 0;
      uint32_t part = crc_chunk16(stage + threadIdx.x * STG_STRIDE, clen, tab);
      uint32_t op = op_full[h];
      if (payload != pf_uniform) { /* true tail frame only */
        const int64_t suffix =
            clen > 0 ? payload - (h0 + c0 + clen) : 0;
        op = x8n_d(uint64_t(suffix));
      }
      acc ^= clen > 0 ? gf2_mulmod_d(op, part) : 0;
      __syncthreads(); /* stage reused by next half */
    }
    uint32_t part = acc;
    /* wave xor-reduce, then one LDS word per wave */
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) part ^= __shfl_xor(part, sh, 64);
    if ((threadIdx.x & 63) == 0) fold[threadIdx.x >> 6] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint32_t raw =
          init_term ^ fold[0] ^ fold[1] ^ fold[2] ^ fold[3];
      const uint32_t crc = ~raw;
      uint8_t *hpos_w = dbase ? dbase + f * block_len +
                                    (TAILCRC ? payload : 0)
                              : nullptr;
      const uint8_t *hpos_r =
          sbase + f * block_len + (TAILCRC ? payload : 0);
      if (MODE == 0) {
        if (TAILCRC) { /* big-endian (sized_coder.go be.Uint32) */
          hpos_w[0] = uint8_t(crc >> 24); hpos_w[1] = uint8_t(crc >> 16);
          hpos_w[2] = uint8_t(crc >> 8); hpos_w[3] = uint8_t(crc);
        } else {
          *reinterpret_cast<uint32_t *>(hpos_w) = crc;
        }
      } else {
        uint32_t want;
        if (TAILCRC) {
          want = (uint32_t(hpos_r[0]) << 24) | (uint32_t(hpos_r[1]) << 16) |
                 (uint32_t(hpos_r[2]) << 8) | uint32_t(hpos_r[3]);
        } else {
          __builtin_memcpy(&want, hpos_r, 4);
        }
        if (want != crc)
          atomicMin(reinterpret_cast<unsigned long long *>(&bad[shard]),
                    static_cast<unsigned long long>(f));
      }
    }
    __syncthreads();
  }
}

/* Register-CRC verify for 64 KiB frames: the fused encode kernel's CRC
 * machinery with no MAC and no stores — one workgroup per frame, each
 * lane Horner-chains its four 4096-strided uint4 pieces (g_shift4k),
 * folds once by its position operator, wave-reduces into a 4-dword LDS
 * slab, and lane 0 compares the 4 B LE header.  The LDS-staged verify
 * kernel measured 2.2 TB/s (stage round-trip + per-chunk barriers on a
 * read-only job); this form is pure streaming reads. */
/* PIPE=1 adds the fused kernel's one-pass load lookahead (pass h+1's four
 * uint4 pieces issued before pass h's Horner chains consume theirs).
 * Costs 16 VGPRs of buffer, so PIPE variants instantiate at WPS < 8 —
 * and MEASURED SLOWER for exactly that reason (reconstruct workload
 * 8.38 ms plain @8 waves vs 8.73 @6 / 8.77 @4, gpurun_out/r3_vrfy_ab.log):
 * 8-way wave interleaving already hides the chain latency, so the
 * occupancy give-back buys nothing here (unlike the fused encode kernel,
 * whose MAC work left it at 3-4 waves anyway).  Kept as a measured
 * variant (GFRS_VRFY=16/14); default is plain @8. */
/* SKEL (measurement-only, wrong CRC results by design — never reachable
 * except via GFRS_VRFY=90/91): 1 = raw XOR instead of all CRC math (the
 * kernel-structure memory floor), 2 = CRC on pieces 0-1 only, raw XOR on
 * 2-3 (half the LDS-gather work) — separates the LDS-pipe cost from the
 * stream cost. */
/* TCHAIN=1: chain the per-pass raw CRCs with two staged 8192-shifts
 * (S = x^(8*16384)*S ^ t) and apply ONE final position mulmod per frame
 * instead of one ~96-VALU mulmod per pass — full frames only, the
 * partial-frame tail keeps the per-pass operator path. */
template <int MODE, int PIPE = 0, int WPS = 8, int SKEL = 0,
          int TCHAIN = 0>
__global__ __launch_bounds__(CRC_BLOCKT, WPS) void crc32b_verify_reg_k(
    uint8_t *__restrict__ dst, size_t dst_stride,
    const uint8_t *__restrict__ src, size_t src_stride, int64_t n,
    int64_t fps, int64_t total, int64_t *bad) {
  constexpr int EF_PASS = 16384;
  constexpr int EF_PASSES = 4;
  constexpr int64_t block_len = 65536;
  constexpr int64_t payload_full = block_len - CRC_LEN;
  constexpr uint32_t INV16K = 0x479933FCu;
  __shared__ __attribute__((aligned(16))) uint32_t tabS[8][256];
  __shared__ uint32_t stabS[4][256];
  __shared__ uint32_t stab8S[4][256]; /* x^(8*8192): split-chain combine */
  __shared__ uint32_t red[4];
  __shared__ uint32_t x8tabS[16];
  for (int i = threadIdx.x; i < 2048; i += CRC_BLOCKT)
    (&tabS[0][0])[i] = (&g_crc_tab4[0][0])[i];
  for (int i = threadIdx.x; i < 1024; i += CRC_BLOCKT)
    (&stabS[0][0])[i] = (&g_shift4k[0][0])[i];
  for (int i = threadIdx.x; i < 1024; i += CRC_BLOCKT)
    (&stab8S[0][0])[i] = (&g_shift8k[0][0])[i];
  if (threadIdx.x == 0) {
    uint32_t v = 0x80000000u;
    for (int j = 0; j < 16; j++) {
      x8tabS[j] = v;
      v = gf2_mulmod_d(v, g_pow8[0]);
    }
  }
  const int64_t lane16 = int64_t(threadIdx.x) * 16;
  const int lane16i = int(threadIdx.x) * 16;
  const uint32_t op_first =
      x8n_d(uint64_t(payload_full - (3 * 4096 + lane16 + 16)));
  const uint32_t op_p0 = op_first;
  const uint32_t op_p1 = gf2_mulmod_d(op_p0, INV16K);
  const uint32_t op_p2 = gf2_mulmod_d(op_p1, INV16K);
  const uint32_t op_p3 = gf2_mulmod_d(op_p2, INV16K);
  const uint32_t it_full =
      gf2_mulmod_d(x8n_d(uint64_t(payload_full)), 0xFFFFFFFFu);
  __syncthreads();

  /* track (shard, f) incrementally — one i64 division per block instead
   * of a ~100-instruction software divide serialized ahead of every
   * frame's first load (same fix as rs_encode_frame_reg_k) */
  int64_t shard = int64_t(blockIdx.x) / fps;
  int64_t f = int64_t(blockIdx.x) - shard * fps;
  const int64_t dshard = int64_t(gridDim.x) / fps;
  const int64_t drem = int64_t(gridDim.x) - dshard * fps;
  for (int64_t fr = blockIdx.x; fr < total; fr += gridDim.x,
               shard += dshard, f += drem,
               (f >= fps ? (f -= fps, ++shard) : int64_t(0))) {
    const int64_t p0 = f * payload_full;
    const int64_t payload = i64min(payload_full, n - p0);
    const uint8_t *fb = as_global(uint64_t(src) + shard * src_stride) +
                        f * block_len;
    const uint8_t *pb = fb + CRC_LEN;
    uint8_t *ob = MODE == 2 ? const_cast<uint8_t *>(as_global(
                                  uint64_t(dst) + shard * dst_stride)) +
                                  p0
                            : nullptr;
    if (threadIdx.x < 4) red[threadIdx.x] = 0;
    __syncthreads();

    uint4 vbuf[PIPE ? 4 : 1];
    if (PIPE) {
      const int rb0 = int(i64min(int64_t(EF_PASS), payload));
#pragma unroll
      for (int i = 0; i < (PIPE ? 4 : 1); i++) {
        const int off = i * 4096 + lane16i;
        vbuf[i] = off + 16 <= rb0
                      ? *reinterpret_cast<const uint4 *>(pb + off)
                      : uint4{0, 0, 0, 0};
      }
    }
    uint32_t Sc = 0; /* TCHAIN pass-chained raw CRC */
    for (int h = 0; h < EF_PASSES; h++) {
      const int64_t r0 = int64_t(h) * EF_PASS;
      const int64_t rbytes = i64min(int64_t(EF_PASS), payload - r0);
      if (rbytes <= 0) break;
      uint4 vcur[PIPE ? 4 : 1];
      if (PIPE) {
#pragma unroll
        for (int i = 0; i < (PIPE ? 4 : 1); i++) vcur[i] = vbuf[i];
        if (h + 1 < EF_PASSES) {
          const int64_t rn0 = int64_t(h + 1) * EF_PASS;
          const int rbn = int(i64min(int64_t(EF_PASS), payload - rn0));
#pragma unroll
          for (int i = 0; i < (PIPE ? 4 : 1); i++) {
            const int off = i * 4096 + lane16i;
            vbuf[i] = (rbn > 0 && off + 16 <= rbn)
                          ? *reinterpret_cast<const uint4 *>(pb + rn0 + off)
                          : uint4{0, 0, 0, 0};
          }
        }
      }
      /* full-frame per-pass operators are frame-independent: op_p0..3
       * were chained once in the prologue, replacing a ~96-VALU mulmod
       * sequence per pass per frame with a 3-select pick */
      uint32_t op = h == 0   ? op_p0
                    : h == 1 ? op_p1
                    : h == 2 ? op_p2
                             : op_p3;
      if (h == EF_PASSES - 1 && threadIdx.x == 255)
        op = shift4k(op, stabS); /* lane 255's last pass has 3 pieces */
      if (payload != payload_full) {
        int np = 0;
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (int64_t(i) * 4096 + lane16 + 16 <= rbytes) np = i + 1;
        const int64_t end =
            np ? r0 + int64_t(np - 1) * 4096 + lane16 + 16 : r0;
        op = x8n_d(uint64_t(payload - end));
      }
      const int rbi = int(rbytes);
      /* two independent Horner sub-chains (pieces 0-1 and 2-3) double
       * the ILP of the LDS-gather chain; the combine shift depends on
       * how many pieces landed in the second chain */
      uint32_t tA = 0, tB = 0;
      int nB = 0;
#pragma unroll
      for (int i = 0; i < 2; i++) {
        const int off = i * 4096 + lane16i;
        if (off + 16 <= rbi) {
          const uint4 v =
              PIPE ? vcur[PIPE ? i : 0]
                   : *reinterpret_cast<const uint4 *>(pb + r0 + off);
          if (MODE == 2) *reinterpret_cast<uint4 *>(ob + r0 + off) = v;
          if (SKEL == 1)
            tA ^= v.x ^ v.y ^ v.z ^ v.w;
          else
            tA = shift4k(tA, stabS) ^ crc16_reg(v, tabS);
        }
      }
#pragma unroll
      for (int i = 2; i < 4; i++) {
        const int off = i * 4096 + lane16i;
        if (off + 16 <= rbi) {
          const uint4 v =
              PIPE ? vcur[PIPE ? i : 0]
                   : *reinterpret_cast<const uint4 *>(pb + r0 + off);
          if (MODE == 2) *reinterpret_cast<uint4 *>(ob + r0 + off) = v;
          if (SKEL >= 1)
            tB ^= v.x ^ v.y ^ v.z ^ v.w;
          else
            tB = shift4k(tB, stabS) ^ crc16_reg(v, tabS);
          nB++;
        }
      }
      const uint32_t t = nB == 2   ? shift4k(tA, stab8S) ^ tB
                         : nB == 1 ? shift4k(tA, stabS) ^ tB
                                   : tA;
      uint32_t part;
      if (TCHAIN && !SKEL && payload == payload_full) {
        if (h < EF_PASSES - 1) {
          Sc = shift4k(shift4k(Sc, stab8S), stab8S) ^ t;
          part = 0;
        } else {
          Sc = shift4k(shift4k(Sc, stab8S), stab8S);
          if (threadIdx.x == 255) {
            /* lane 255's last pass has 3 pieces: its t sits one 4096
             * position higher than the chain's, so it gets its own
             * shifted operator (exactly the non-chained path's tweak) */
            part = (Sc ? gf2_mulmod_d(op_p3, Sc) : 0) ^
                   (t ? gf2_mulmod_d(shift4k(op_p3, stabS), t) : 0);
          } else {
            const uint32_t m = Sc ^ t;
            part = m ? gf2_mulmod_d(op_p3, m) : 0;
          }
        }
      } else {
        part = t ? gf2_mulmod_d(op, t) : 0;
      }
      if (rbi & 15) {
        const int t0 = rbi & ~15;
        const int p = t0 + int(threadIdx.x);
        if (p < rbi) {
          const uint8_t x = pb[r0 + p];
          if (MODE == 2) ob[r0 + p] = x;
          part ^= gf2_mulmod_d(x8tabS[rbi - 1 - p], tabS[0][x]);
        }
      }
#pragma unroll
      for (int sh = 32; sh > 0; sh >>= 1) part ^= __shfl_xor(part, sh, 64);
      if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] ^= part;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint32_t it =
          payload == payload_full
              ? it_full
              : gf2_mulmod_d(x8n_d(uint64_t(payload)), 0xFFFFFFFFu);
      const uint32_t crc = ~(it ^ red[0] ^ red[1] ^ red[2] ^ red[3]);
      uint32_t want;
      __builtin_memcpy(&want, fb, 4); /* LE header */
      if (want != crc)
        atomicMin(reinterpret_cast<unsigned long long *>(&bad[shard]),
                  static_cast<unsigned long long>(f));
    }
    __syncthreads();
  }
}

template <int MODE, bool TAILCRC = false>
static void crc_dispatch(uint8_t *dst, size_t dst_stride, const uint8_t *src,
                         size_t src_stride, int64_t n, int64_t block_len,
                         int64_t fps, int64_t total, int64_t *bad,
                         hipStream_t s) {
  const int grid = crc_grid(total, fps);
  if (fps == 1 && n <= 8192) {
    const int64_t g2l = (total + 3) / 4;
    const int g2 = int(g2l < 2048 ? g2l : 2048);
    hipLaunchKernelGGL((crc32b_small_k<MODE, TAILCRC>), dim3(g2 > 0 ? g2 : 1),
                       dim3(CRC_BLOCKT), 0, s, dst, dst_stride, src,
                       src_stride, n, block_len, total, bad);
    return;
  }
  static const int chunk_sel = []() {
    const char *e = getenv("GFRS_CRC_CHUNK");
    const int v = e ? atoi(e) : 64;
    return (v == 32 || v == 64 || v == 128 || v == 256) ? v : 64;
  }();
  if ((MODE == 1 || MODE == 2) && !TAILCRC && block_len == 65536) {
    const int g = fused_grid(total, fps);
    /* GFRS_VRFY: 0 = plain 8-wave (default), 16 = one-pass load
     * lookahead @6 waves, 14 = lookahead @4 waves */
    static const int vsel = []() {
      const char *e = getenv("GFRS_VRFY");
      const int v = e ? atoi(e) : 0;
      return (v == 16 || v == 14 || v == 18 || v == 10 || v == 90 ||
              v == 91)
                 ? v
                 : 0;
    }();
    if (vsel == 10) /* legacy per-pass position mulmods (pre-TCHAIN) */
      hipLaunchKernelGGL((crc32b_verify_reg_k<MODE, 0, 8, 0, 0>), dim3(g),
                         dim3(CRC_BLOCKT), 0, s, dst, dst_stride, src,
                         src_stride, n, fps, total, bad);
    else if (vsel == 18) /* lookahead at full 8 waves (base kernel is only
                       44 VGPRs, so the 16-VGPR buffer still fits 64) */
      hipLaunchKernelGGL((crc32b_verify_reg_k<MODE, 1, 8>), dim3(g),
                         dim3(CRC_BLOCKT), 0, s, dst, dst_stride, src,
                         src_stride, n, fps, total, bad);
    else if (vsel == 90) /* measurement skeleton: see kernel comment */
      hipLaunchKernelGGL((crc32b_verify_reg_k<MODE, 0, 8, 1>), dim3(g),
                         dim3(CRC_BLOCKT), 0, s, dst, dst_stride, src,
                         src_stride, n, fps, total, bad);
    else if (vsel == 91)
      hipLaunchKernelGGL((crc32b_verify_reg_k<MODE, 0, 8, 2>), dim3(g),
                         dim3(CRC_BLOCKT), 0, s, dst, dst_stride, src,
                         src_stride, n, fps, total, bad);
    else if (vsel == 16)
      hipLaunchKernelGGL((crc32b_verify_reg_k<MODE, 1, 6>), dim3(g),
                         dim3(CRC_BLOCKT), 0, s, dst, dst_stride, src,
                         src_stride, n, fps, total, bad);
    else if (vsel == 14)
      hipLaunchKernelGGL((crc32b_verify_reg_k<MODE, 1, 4>), dim3(g),
                         dim3(CRC_BLOCKT), 0, s, dst, dst_stride, src,
                         src_stride, n, fps, total, bad);
    else /* default: pass-chained raw CRC (one position mulmod per
            frame instead of one ~96-VALU mulmod per pass; measured
            5.51 -> 5.13 ms on the verify leg — at the structural
            skeleton floor) */
      hipLaunchKernelGGL((crc32b_verify_reg_k<MODE, 0, 8, 0, 1>), dim3(g),
                         dim3(CRC_BLOCKT), 0, s, dst, dst_stride, src,
                         src_stride, n, fps, total, bad);
    return;
  }
  if (block_len == 65536) {
    const bool nt = nt_enabled() && MODE != 1;
#define GFRS_CRC_GO(NTV, CH)                                                \
  hipLaunchKernelGGL((crc32b_staged_k<MODE, NTV, TAILCRC, CH>), dim3(grid), \
                     dim3(CRC_BLOCKT), StgGeom<CH>::LDS, s, dst,            \
                     dst_stride, src, src_stride, n, fps, total, bad)
    if (nt) {
      if (chunk_sel == 32) GFRS_CRC_GO(true, 32);
      else if (chunk_sel == 128) GFRS_CRC_GO(true, 128);
      else if (chunk_sel == 256) GFRS_CRC_GO(true, 256);
      else GFRS_CRC_GO(true, 64);
    } else {
      if (chunk_sel == 32) GFRS_CRC_GO(false, 32);
      else if (chunk_sel == 128) GFRS_CRC_GO(false, 128);
      else if (chunk_sel == 256) GFRS_CRC_GO(false, 256);
      else GFRS_CRC_GO(false, 64);
    }
#undef GFRS_CRC_GO
  } else {
    hipLaunchKernelGGL((crc32b_k<MODE, TAILCRC>), dim3(grid),
                       dim3(CRC_BLOCKT), 0, s, dst, dst_stride, src,
                       src_stride, n, block_len, fps, total, bad);
  }
}

void launch_sized_encode(uint8_t *dst, size_t dst_stride, const uint8_t *src,
                         size_t src_stride, int64_t n, int64_t block_len,
                         int nshards, hipStream_t s) {
  const int64_t payload = block_len - CRC_LEN;
  const int64_t fps = (n + payload - 1) / payload;
  crc_dispatch<0, true>(dst, dst_stride, src, src_stride, n, block_len, fps,
                        fps * nshards, nullptr, s);
}

void launch_sized_verify(const uint8_t *framed, size_t stride,
                         int64_t body_len, int64_t block_len, int nshards,
                         int64_t *bad, hipStream_t s) {
  const int64_t fps = (body_len + block_len - 1) / block_len;
  const int64_t n = body_len - CRC_LEN * fps;
  crc_dispatch<1, true>(nullptr, 0, framed, stride, n, block_len, fps,
                        fps * nshards, bad, s);
}

void launch_sized_decode(uint8_t *dst, size_t dst_stride,
                         const uint8_t *framed, size_t src_stride,
                         int64_t body_len, int64_t block_len, int nshards,
                         int64_t *bad, hipStream_t s) {
  const int64_t fps = (body_len + block_len - 1) / block_len;
  const int64_t n = body_len - CRC_LEN * fps;
  crc_dispatch<2, true>(dst, dst_stride, framed, src_stride, n, block_len,
                        fps, fps * nshards, bad, s);
}

/* ------------------------------------------------------------------ */
/* fused encode+frame: RS parity + crc32block framing in one pass        */
/* ------------------------------------------------------------------ */

/* The blobstore PUT/repair pipeline is encode (access/stream) followed by
 * per-shard crc32block framing (blobnode datafile.go:342).  Run as two
 * kernels that is 3 HBM passes over the data (encode: read k, write m;
 * frame: read k+m, write k+m).  Fused, each data byte is read ONCE, the
 * framed images are written ONCE, and the unframed parity never exists in
 * HBM: read k·S + write (k+m)·(S+headers) — a 1.8x traffic cut at 6+3.
 *
 * Geometry: one workgroup per (stripe, 64 KiB frame); the frame's 65,532
 * payload bytes are processed in 4 passes of 16,384 B.  Within a pass,
 * lane w owns columns {i·4096 + w·16 : i<4} for the parity MACs
 * (coalesced uint4 loads, identical to rs_apply) and chunk
 * [w·64, w·64+64) of the pass for the CRC fold (read back from a 20 KB
 * LDS stage with conflict-free b128 banking).  Each shard's range is
 * staged, CRC'd and framed-written in turn; parity accumulates in VGPRs
 * across the k data shards and then takes the same stage path. */

/* tables | per-frame CRC reduction slab (4 waves x 16 shards) | stage(s);
 * pass/chunk/stage geometry is a template parameter of the kernel (NI). */
constexpr int EF_RED = 4 * 16 * 4;

template <int GM, int NBUF, int WPS, int ABL = 0, int NI = 4>
__global__ __launch_bounds__(CRC_BLOCKT, WPS) void rs_encode_frame_k(
    uint8_t *__restrict__ dst, size_t dst_stride /* framed image stride */,
    uint64_t base, uint64_t stripe_stride, size_t shard_len, int k,
    const uint8_t *__restrict__ tabs /* [GM*k][32] */, int64_t total_frames,
    int64_t frames_per_shard) {
  /* NI = 4096-B subtiles per pass.  NI=4 is the 16 KiB geometry described
   * above; NI=2 halves the pass (8 KiB, 8 passes/frame): acc[] drops from
   * GM*4 to GM*2 uint4s and the stage from 20 KB to 12 KB, trading more
   * barriers + CRC folds for co-resident blocks (VGPR/LDS occupancy). */
  constexpr int EF_PASS = NI * 4096;
  constexpr int EF_CHUNK = NI * 16;          /* 256 lanes cover the pass */
  constexpr int EF_STRIDE = EF_CHUNK + 16;   /* odd-16 stride: bank-clean */
  constexpr int EF_PASSES = (65532 + EF_PASS - 1) / EF_PASS;
  constexpr int EF_STG_ONE = 256 * EF_STRIDE;
  constexpr int64_t block_len = 65536;
  constexpr int64_t payload_full = block_len - CRC_LEN;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t(*tab)[256] = reinterpret_cast<uint32_t(*)[256]>(smem);
  uint32_t *red = reinterpret_cast<uint32_t *>(smem + 8192);
  uint8_t *stage = smem + 8192 + EF_RED;
  /* coefficient tables live in registers: GM*k*32 B is too much for
   * k>4, so re-read from global per MAC via __ldg-style loads would be
   * slow; instead keep them in LDS *before* the stage area is used —
   * they are consumed only during the MAC phase of each pass, while the
   * stage is consumed in the CRC phase, so they can share space only if
   * reloaded per pass.  Simpler: put them in the tail of the table area
   * is impossible (4 KB exactly) — so carve GM*k*32 extra after stage. */
  /* coefficient tables, carved after the NBUF stage buffer(s) */
  uint8_t *ctab = smem + 8192 + EF_RED + NBUF * EF_STG_ONE;
  for (int i = threadIdx.x; i < 2048; i += CRC_BLOCKT)
    (&tab[0][0])[i] = (&g_crc_tab4[0][0])[i];
  for (int i = threadIdx.x; i < GM * k * 2; i += CRC_BLOCKT)
    reinterpret_cast<uint4 *>(ctab)[i] =
        reinterpret_cast<const uint4 *>(tabs)[i];
  /* per-(pass,lane) fold operator for full frames */
  uint32_t op_full[EF_PASSES];
#pragma unroll
  for (int h = 0; h < EF_PASSES; h++) {
    const int64_t c0 = int64_t(h) * EF_PASS + int64_t(threadIdx.x) * EF_CHUNK;
    const int64_t cend = i64min(c0 + EF_CHUNK, payload_full);
    op_full[h] = x8n_d(uint64_t(payload_full - (cend > c0 ? cend : c0)));
  }
  __syncthreads();


  for (int64_t fr = blockIdx.x; fr < total_frames; fr += gridDim.x) {
    const int64_t stripe = fr / frames_per_shard;
    const int64_t f = fr - stripe * frames_per_shard;
    const int64_t p0 = f * payload_full;
    const int64_t payload = i64min(payload_full, int64_t(shard_len) - p0);
    const uint8_t *sbase = as_global(base + stripe * stripe_stride);

    /* per-frame CRC partials live in the LDS red slab (4 waves x 16
     * shard slots): no runtime-indexed per-lane array -> no scratch */
    for (int j = threadIdx.x; j < 64; j += CRC_BLOCKT) red[j] = 0;
    uint4 acc[GM][NI];
    __syncthreads();

    /* Software pipeline over the k+GM shard units of each pass: unit u's
     * range is written into stage[u&1] while unit u-1's chunks are CRC'd
     * out of stage[(u-1)&1] — ONE barrier per unit, and the LDS/VALU CRC
     * work overlaps the next unit's global traffic. */
    for (int h = 0; h < EF_PASSES; h++) {
      const int64_t r0 = int64_t(h) * EF_PASS;
      const int64_t rbytes = i64min(int64_t(EF_PASS), payload - r0);
      if (rbytes <= 0) break;
#pragma unroll
      for (int r = 0; r < GM; r++)
#pragma unroll
        for (int i = 0; i < NI; i++) acc[r][i] = uint4{0, 0, 0, 0};

      const int64_t lane16 = int64_t(threadIdx.x) * 16;
      const int64_t c0b = int64_t(threadIdx.x) * EF_CHUNK;
      int clen = int(i64min(int64_t(EF_CHUNK), rbytes - c0b));
      if (clen < 0) clen = 0;
      uint32_t op = op_full[h];
      if (payload != payload_full) {
        const int64_t suffix = clen > 0 ? payload - (r0 + c0b + clen) : 0;
        op = x8n_d(uint64_t(suffix));
      }

      /* helper: CRC the previous unit's staged buffer, fold, reduce */
      auto crc_prev = [&](int unit) {
        if (ABL == 1) return;
        if (unit >= 0 && clen > 0) {
          const uint8_t *pstg =
              stage + (NBUF == 2 ? (unit & 1) : 0) * EF_STG_ONE;
          uint32_t part =
              gf2_mulmod_d(op,
                           crc_chunk16(pstg + threadIdx.x * EF_STRIDE, clen,
                                       tab));
#pragma unroll
          for (int sh = 32; sh > 0; sh >>= 1)
            part ^= __shfl_xor(part, sh, 64);
          if ((threadIdx.x & 63) == 0)
            red[(threadIdx.x >> 6) * 16 + unit] ^= part;
        }
      };

      for (int c = 0; c < k; c++) {
        uint8_t *stg = stage + (NBUF == 2 ? (c & 1) : 0) * EF_STG_ONE;
        const uint8_t *src = sbase + size_t(c) * shard_len + p0 + r0;
        uint8_t *fdst = dst + (stripe * (k + GM) + c) * dst_stride +
                        f * block_len + CRC_LEN + r0;
#pragma unroll
        for (int i = 0; i < NI; i++) {
          const int64_t off = int64_t(i) * 4096 + lane16;
          if (off + 16 <= rbytes) {
            const uint4 v = *reinterpret_cast<const uint4 *>(src + off);
            if (ABL != 2) {
              LinTab lt[GM];
#pragma unroll
              for (int r = 0; r < GM; r++)
                lt[r] = lintab_load(ctab, r * k + c);
#pragma unroll
              for (int d = 0; d < 4; d++)
                gfmac4_lin_rows_n<GM, NI>(acc, i, d, (&v.x)[d], lt);
            }
            if (ABL != 3) {
              uint32_t *dw = reinterpret_cast<uint32_t *>(fdst + off);
              dw[0] = v.x; dw[1] = v.y; dw[2] = v.z; dw[3] = v.w;
            }
            *reinterpret_cast<uint4 *>(
                &stg[(off / EF_CHUNK) * EF_STRIDE +
                     (off & (EF_CHUNK - 1))]) = v;
          }
        }
        if (rbytes < EF_PASS && threadIdx.x == 0) {
          const int64_t t0 = (rbytes / 16) * 16;
          for (int64_t p = t0; p < rbytes; p++) {
            const uint8_t x = src[p];
            fdst[p] = x;
            stg[(p / EF_CHUNK) * EF_STRIDE + (p & (EF_CHUNK - 1))] = x;
          }
        }
        if (NBUF == 2) {
          /* overlap: CRC unit c-1 (other buffer) before the reuse barrier */
          crc_prev(c - 1);
          __syncthreads();
        } else {
          __syncthreads();
          crc_prev(c);
          __syncthreads();
        }
      }
#pragma unroll
      for (int r = 0; r < GM; r++) {
        uint8_t *stg = stage + (NBUF == 2 ? ((k + r) & 1) : 0) * EF_STG_ONE;
        uint8_t *fdst = dst + (stripe * (k + GM) + k + r) * dst_stride +
                        f * block_len + CRC_LEN + r0;
#pragma unroll
        for (int i = 0; i < NI; i++) {
          const int64_t off = int64_t(i) * 4096 + lane16;
          if (off + 16 <= rbytes) {
            if (ABL != 3) {
              uint32_t *dw = reinterpret_cast<uint32_t *>(fdst + off);
              dw[0] = acc[r][i].x; dw[1] = acc[r][i].y;
              dw[2] = acc[r][i].z; dw[3] = acc[r][i].w;
            }
            *reinterpret_cast<uint4 *>(
                &stg[(off / EF_CHUNK) * EF_STRIDE +
                     (off & (EF_CHUNK - 1))]) = acc[r][i];
          }
        }
        if (rbytes < EF_PASS && threadIdx.x == 0) {
          const int64_t t0 = (rbytes / 16) * 16;
          for (int64_t p = t0; p < rbytes; p++) {
            uint8_t pv = 0;
            for (int c2 = 0; c2 < k; c2++) {
              const uint8_t b = sbase[size_t(c2) * shard_len + p0 + r0 + p];
              pv ^= gfmul1_lin(ctab + size_t(r * k + c2) * 32, b);
            }
            fdst[p] = pv;
            stg[(p / EF_CHUNK) * EF_STRIDE + (p & (EF_CHUNK - 1))] = pv;
          }
        }
        if (NBUF == 2) {
          crc_prev(k + r - 1);
          __syncthreads();
        } else {
          __syncthreads();
          crc_prev(k + r);
          __syncthreads();
        }
      }
      if (NBUF == 2) {
        crc_prev(k + GM - 1);
        __syncthreads();
      }
    }

    /* ---- combine wave partials, write the 4 B LE headers ---- */
    if (threadIdx.x == 0) {
      const uint32_t it = gf2_mulmod_d(x8n_d(uint64_t(payload)), 0xFFFFFFFFu);
      for (int j = 0; j < k + GM; j++) {
        const uint32_t crc =
            ~(it ^ red[j] ^ red[16 + j] ^ red[32 + j] ^ red[48 + j]);
        *reinterpret_cast<uint32_t *>(
            dst + (stripe * (k + GM) + j) * dst_stride + f * block_len) = crc;
      }
    }
    __syncthreads();
  }
}



/* Register-CRC variant of the fused encode+frame kernel: no LDS stage at
 * all.  Lane w's four uint4 pieces of a 16 KiB pass (subtile offsets
 * i*4096 + 16w) are CRC'd straight out of the registers the MAC/store
 * phase already holds, Horner-chained with the constant x^(8*4096) shift
 * (4 LDS gathers), then folded once by the lane's position operator and
 * wave-reduced — so the per-unit stage round-trip AND the two
 * __syncthreads per unit disappear (only the per-frame reduction-slab
 * barriers remain) and waves pipeline units/passes freely.  Same output
 * bytes as rs_encode_frame_k (oracle parity-tested). */
/* MAP: 0 = plain grid-stride over frames; 1 = each block owns a
 * contiguous run of frames (stream locality across its iterations);
 * 2 = run-per-block with the block ids permuted so the 8 XCDs (round-
 * robin dispatch) each own a contiguous 1/8 of the frame space and an
 * XCD's L2 sees only its own stripes' read/write streams. */
/* SKEL=1 compiles out MAC+CRC, leaving loads + framed stores with the
 * exact production addressing: the kernel's own empirical memory floor. */
/* PIPE=1: explicit one-unit lookahead - unit c+1's four piece loads are
 * issued before unit c's MAC/CRC/store consume their values, so the
 * compute of each unit overlaps the memory latency of the next.  Costs
 * ~32 VGPRs of double-buffer; pair with WPS=3. */
template <int GM, int WPS, int MAP = 0, int SKEL = 0, int PIPE = 0,
          int ST = 0>
__global__ __launch_bounds__(CRC_BLOCKT, WPS) void rs_encode_frame_reg_k(
    uint8_t *__restrict__ dst, size_t dst_stride, uint64_t base,
    uint64_t stripe_stride, size_t shard_len, int k,
    const uint8_t *__restrict__ tabs /* [GM*k][32] */, int64_t total_frames,
    int64_t frames_per_shard, int tiny_len /* folded last-frame payload:
    when a shard's last frame carries <= 64 payload bytes (64/128/256 KiB
    shards leave 4-16), the host drops it from the frame grid and the
    PRECEDING frame's workgroup emits it in its epilogue — at 64 KiB
    shards half of all workgroup iterations otherwise process ~nothing */) {
  constexpr int EF_PASS = 16384;
  constexpr int EF_PASSES = 4; /* ceil(65532 / 16384) */
  constexpr int64_t block_len = 65536;
  constexpr int64_t payload_full = block_len - CRC_LEN;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  /* crc tables 8 KB | shift4k 4 KB | red slab | coefficient tables */
  uint32_t(*tab)[256] = reinterpret_cast<uint32_t(*)[256]>(smem);
  uint32_t(*stab)[256] = reinterpret_cast<uint32_t(*)[256]>(smem + 8192);
  uint32_t *red = reinterpret_cast<uint32_t *>(smem + 12288);
  /* x^(8*j), j<16: position operators for the <16-byte pass tails */
  uint32_t *x8tab = reinterpret_cast<uint32_t *>(smem + 12288 + EF_RED);
  /* staged tail bytes of the (up to 16) input shards: the parity tails
   * read these from LDS instead of k dependent global loads per lane */
  uint8_t *tailb = smem + 12288 + EF_RED + 64;
  uint8_t *tinyb = smem + 12288 + EF_RED + 64 + 256; /* 16 x 64 */
  uint8_t *ctab = smem + 12288 + EF_RED + 64 + 256 + 1024;
  for (int i = threadIdx.x; i < 2048; i += CRC_BLOCKT)
    (&tab[0][0])[i] = (&g_crc_tab4[0][0])[i];
  for (int i = threadIdx.x; i < 1024; i += CRC_BLOCKT)
    (&stab[0][0])[i] = (&g_shift4k[0][0])[i];
  for (int i = threadIdx.x; i < GM * k * 2; i += CRC_BLOCKT)
    reinterpret_cast<uint4 *>(ctab)[i] =
        reinterpret_cast<const uint4 *>(tabs)[i];
  if (threadIdx.x == 0) {
    uint32_t v = 0x80000000u;
    for (int j = 0; j < 16; j++) {
      x8tab[j] = v;
      v = gf2_mulmod_d(v, g_pow8[0]);
    }
  }
  const int64_t lane16 = int64_t(threadIdx.x) * 16;
  const int lane16i = int(threadIdx.x) * 16;
  /* Full-frame fold operator, chained: op for pass h+1 = op for pass h
   * times x^(-8*16384) (constant 0x479933FC, precomputed inverse).  Only
   * lane 255 in the last pass has 3 pieces instead of 4; its operator is
   * the chained value times x^(8*4096), i.e. one shift4k.  One register
   * instead of an op_full[4] array. */
  constexpr uint32_t INV16K = 0x479933FCu;
  /* the chain is built from crc12u_reg pieces, each short of the raw CRC
   * by x^32: every operator that multiplies it carries 4 bytes more */
  const uint32_t op_first =
      x8n_d(uint64_t(payload_full - (3 * 4096 + lane16 + 16) + 4));
  /* full-frame per-pass operators are frame-independent: chain them once
   * here (a 3-select pick in the pass loop) instead of a ~96-VALU serial
   * mulmod per pass per frame */
  const uint32_t op_pA = op_first;
  const uint32_t op_pB = gf2_mulmod_d(op_pA, INV16K);
  const uint32_t op_pC = gf2_mulmod_d(op_pB, INV16K);
  const uint32_t op_pD = gf2_mulmod_d(op_pC, INV16K);
  const uint32_t it_full =
      gf2_mulmod_d(x8n_d(uint64_t(payload_full)), 0xFFFFFFFFu);
  __syncthreads();

  int64_t fr0 = blockIdx.x, frN = total_frames, frS = gridDim.x;
  if (MAP != 0) {
    const int64_t nper = (total_frames + gridDim.x - 1) / gridDim.x;
    const int64_t b = MAP == 2 ? int64_t(blockIdx.x & 7) * (gridDim.x >> 3) +
                                     (blockIdx.x >> 3)
                               : int64_t(blockIdx.x);
    fr0 = b * nper;
    frN = i64min(fr0 + nper, total_frames);
    frS = 1;
  }
  /* track (stripe, f) incrementally: one i64 division per block instead
   * of a ~100-instruction software divide per frame iteration */
  int64_t stripe = fr0 / frames_per_shard;
  int64_t f = fr0 - stripe * frames_per_shard;
  const int64_t dstripe = frS / frames_per_shard;
  const int64_t drem = frS - dstripe * frames_per_shard;
  for (int64_t fr = fr0; fr < frN; fr += frS,
               stripe += dstripe, f += drem,
               (f >= frames_per_shard ? (f -= frames_per_shard, ++stripe)
                                      : int64_t(0))) {
    const int64_t p0 = f * payload_full;
    const int64_t payload = i64min(payload_full, int64_t(shard_len) - p0);
    const uint8_t *sbase = as_global(base + stripe * stripe_stride);

    uint4 acc[GM][4];
    uint4 vnext[PIPE ? 4 : 1];
    uint4 vnext2[PIPE == 2 ? 4 : 1];
    if (PIPE && fr == fr0) { /* later frames are prefetched by the
                                previous frame's last pass */
      const int rb0 = int(i64min(int64_t(EF_PASS), payload));
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int off = i * 4096 + lane16i;
        vnext[PIPE ? i : 0] =
            off + 16 <= rb0
                ? *reinterpret_cast<const uint4 *>(sbase + p0 + off)
                : uint4{0, 0, 0, 0};
      }
      if (PIPE == 2) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int off = i * 4096 + lane16i;
          vnext2[PIPE == 2 ? i : 0] =
              off + 16 <= rb0 ? *reinterpret_cast<const uint4 *>(
                                    sbase + shard_len + p0 + off)
                              : uint4{0, 0, 0, 0};
        }
      }
    }
    for (int j = threadIdx.x; j < 64; j += CRC_BLOCKT) red[j] = 0;
    __syncthreads();

    for (int h = 0; h < EF_PASSES; h++) {
      const int64_t r0 = int64_t(h) * EF_PASS;
      const int64_t rbytes = i64min(int64_t(EF_PASS), payload - r0);
      if (rbytes <= 0) break;
#pragma unroll
      for (int r = 0; r < GM; r++)
#pragma unroll
        for (int i = 0; i < 4; i++) acc[r][i] = uint4{0, 0, 0, 0};

      uint32_t op = h == 0   ? op_pA
                    : h == 1 ? op_pB
                    : h == 2 ? op_pC
                             : op_pD;
      if (h == EF_PASSES - 1 && threadIdx.x == 255)
        op = shift4k(op, stab); /* lane 255's last pass has 3 pieces */
      if (payload != payload_full) {
        int np = 0;
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (int64_t(i) * 4096 + lane16 + 16 <= rbytes) np = i + 1;
        const int64_t end =
            np ? r0 + int64_t(np - 1) * 4096 + lane16 + 16 : r0;
        op = x8n_d(uint64_t(payload - end + 4));
      }

      const int rbi = int(rbytes);
      for (int c = 0; c < k; c++) {
        const uint8_t *src = sbase + size_t(c) * shard_len + p0 + r0;
        uint8_t *fdst = dst + (stripe * (k + GM) + c) * dst_stride +
                        f * block_len + CRC_LEN + r0;
        /* A|B|C tables for this unit's GM rows, hoisted to VGPRs for the
         * whole 64-B piece run (the nibble path re-read 2 ds_read_b128
         * per piece per row) */
        LinTab lt[GM];
        if (SKEL != 1 && SKEL != 4)
#pragma unroll
          for (int r = 0; r < GM; r++) lt[r] = lintab_load(ctab, r * k + c);
        uint4 vcur[PIPE ? 4 : 1];
        if (PIPE == 2) {
#pragma unroll
          for (int i = 0; i < 4; i++) {
            vcur[PIPE ? i : 0] = vnext[PIPE ? i : 0];
            vnext[PIPE ? i : 0] = vnext2[PIPE == 2 ? i : 0];
          }
          if (c + 2 < k) {
            const uint8_t *nsrc = sbase + size_t(c + 2) * shard_len + p0 + r0;
#pragma unroll
            for (int i = 0; i < 4; i++) {
              const int off = i * 4096 + lane16i;
              vnext2[PIPE == 2 ? i : 0] =
                  off + 16 <= rbi
                      ? *reinterpret_cast<const uint4 *>(nsrc + off)
                      : uint4{0, 0, 0, 0};
            }
          }
        } else if (PIPE) {
#pragma unroll
          for (int i = 0; i < 4; i++) vcur[PIPE ? i : 0] = vnext[PIPE ? i : 0];
          if (c + 1 < k) {
            const uint8_t *nsrc = sbase + size_t(c + 1) * shard_len + p0 + r0;
#pragma unroll
            for (int i = 0; i < 4; i++) {
              const int off = i * 4096 + lane16i;
              vnext[PIPE ? i : 0] =
                  off + 16 <= rbi
                      ? *reinterpret_cast<const uint4 *>(nsrc + off)
                      : uint4{0, 0, 0, 0};
            }
          }
        }
        /* shift4k(0) == 0, so the Horner chain can start from t = 0 and
         * run unconditionally: no 'any' tracking, less register state,
         * and the 4 piece loads stay in flight together. */
        uint32_t t = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int off = i * 4096 + lane16i;
          if (off + 16 <= rbi) {
            const uint4 v =
                PIPE ? vcur[PIPE ? i : 0]
                     : *reinterpret_cast<const uint4 *>(src + off);
            if (SKEL != 1 && SKEL != 4) {
#pragma unroll
              for (int d = 0; d < 4; d++)
                gfmac4_lin_rows<GM>(acc, i, d, (&v.x)[d], lt);
            }
            /* frame payload sits at +4 mod 16; the hardware takes
             * dword-aligned dwordx4 (the loads at p0 = f*65532 already
             * run that way), so one store instead of four */
            fstore16<ST>(fdst + off, v);
            if (SKEL != 1 && SKEL != 3) t = shift4k(t, stab) ^ crc12u_reg(v, tab);
          }
        }
        uint32_t part = SKEL == 2 ? t : (t ? gf2_mulmod_d(op, t) : 0);
        if (rbytes < EF_PASS) {
          /* lane-parallel tail: one byte per lane, folded by its own
           * position operator (the serial thread-0 loop dominated tiny
           * last frames: 9 units of dependent global loads) */
          const int t0 = (rbi / 16) * 16;
          const int p = t0 + int(threadIdx.x);
          if (p < rbi) {
            const uint8_t x = src[p];
            fdst[p] = x;
            tailb[c * 16 + (p - t0)] = x;
            if (SKEL != 1)
              part ^= gf2_mulmod_d(x8tab[rbi - 1 - p], tab[0][x]);
          }
        }
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1)
          part ^= __shfl_xor(part, sh, 64);
        if ((threadIdx.x & 63) == 0)
          red[(threadIdx.x >> 6) * 16 + c] ^= part;
      }
      if (rbytes < EF_PASS) __syncthreads(); /* tailb visible to all */
      if (PIPE) { /* next pass's (or next frame's) unit-0 loads fly
                     during the parity rows and the frame epilogue */
        int64_t r0n = r0 + EF_PASS;
        int64_t rbn = i64min(int64_t(EF_PASS), payload - r0n);
        const uint8_t *nbase = sbase + p0;
        if (rbn <= 0 && fr + frS < frN) {
          const int64_t fr2 = fr + frS;
          const int64_t st2 = fr2 / frames_per_shard;
          const int64_t p02 = (fr2 - st2 * frames_per_shard) * payload_full;
          rbn = i64min(int64_t(EF_PASS), int64_t(shard_len) - p02);
          nbase = as_global(base + st2 * stripe_stride) + p02;
          r0n = 0;
        }
        if (rbn > 0) {
          const int rbni = int(rbn);
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const int off = i * 4096 + lane16i;
            vnext[PIPE ? i : 0] =
                off + 16 <= rbni
                    ? *reinterpret_cast<const uint4 *>(nbase + r0n + off)
                    : uint4{0, 0, 0, 0};
          }
          if (PIPE == 2) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
              const int off = i * 4096 + lane16i;
              vnext2[PIPE == 2 ? i : 0] =
                  off + 16 <= rbni ? *reinterpret_cast<const uint4 *>(
                                         nbase + shard_len + r0n + off)
                                   : uint4{0, 0, 0, 0};
            }
          }
        }
      }
#pragma unroll
      for (int r = 0; r < GM; r++) {
        uint8_t *fdst = dst + (stripe * (k + GM) + k + r) * dst_stride +
                        f * block_len + CRC_LEN + r0;
        uint32_t t = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int off = i * 4096 + lane16i;
          if (off + 16 <= rbi) {
            fstore16<ST>(fdst + off, acc[r][i]);
            if (SKEL != 1 && SKEL != 3)
              t = shift4k(t, stab) ^ crc12u_reg(acc[r][i], tab);
          }
        }
        uint32_t part = SKEL == 2 ? t : (t ? gf2_mulmod_d(op, t) : 0);
        if (SKEL != 1 && rbytes < EF_PASS) {
          const int t0 = (rbi / 16) * 16;
          const int p = t0 + int(threadIdx.x);
          if (p < rbi) {
            uint8_t pv = 0;
            for (int c2 = 0; c2 < k; c2++) {
              const uint8_t b = tailb[c2 * 16 + (p - t0)];
              pv ^= gfmul1_lin(ctab + size_t(r * k + c2) * 32, b);
            }
            fdst[p] = pv;
            part ^= gf2_mulmod_d(x8tab[rbi - 1 - p], tab[0][pv]);
          }
        }
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1)
          part ^= __shfl_xor(part, sh, 64);
        if ((threadIdx.x & 63) == 0)
          red[(threadIdx.x >> 6) * 16 + k + r] ^= part;
      }
    }

    __syncthreads();
    { /* one frame-header lane per shard (j < k+GM <= 16, all in wave 0) */
      const int j = int(threadIdx.x);
      if (j < k + GM) {
        const uint32_t it =
            payload == payload_full
                ? it_full
                : gf2_mulmod_d(x8n_d(uint64_t(payload)), 0xFFFFFFFFu);
        const uint32_t crc =
            ~(it ^ red[j] ^ red[16 + j] ^ red[32 + j] ^ red[48 + j]);
        *reinterpret_cast<uint32_t *>(
            dst + (stripe * (k + GM) + j) * dst_stride + f * block_len) = crc;
      }
    }
    if (tiny_len && f == frames_per_shard - 1) {
      /* emit the folded tiny last frame: one lane per shard computes
       * (or copies) its <= 64 payload bytes, CRCs them bytewise, and
       * writes header + payload.  No private arrays (runtime-indexed
       * locals land in scratch). */
      const int j = int(threadIdx.x);
      const int64_t tp0 = (f + 1) * payload_full;
      if (j < k) {
        const uint8_t *sp = sbase + size_t(j) * shard_len + tp0;
        for (int b = 0; b < tiny_len; b++) tinyb[j * 64 + b] = sp[b];
      }
      __syncthreads();
      if (j < k + GM) {
        uint8_t *tb =
            dst + (stripe * (k + GM) + j) * dst_stride + (f + 1) * block_len;
        uint32_t cr = 0;
        for (int b = 0; b < tiny_len; b++) {
          uint8_t x;
          if (j < k) {
            x = tinyb[j * 64 + b];
          } else {
            x = 0;
            for (int c2 = 0; c2 < k; c2++)
              x ^= gfmul1_lin(ctab + size_t((j - k) * k + c2) * 32,
                              tinyb[c2 * 64 + b]);
          }
          tb[CRC_LEN + b] = x;
          cr = tab[0][(cr ^ x) & 0xFF] ^ (cr >> 8);
        }
        *reinterpret_cast<uint32_t *>(tb) =
            ~(gf2_mulmod_d(x8n_d(uint64_t(tiny_len)), 0xFFFFFFFFu) ^ cr);
      }
    }
    __syncthreads();
  }
}


/* ------------------------------------------------------------------ */
/* aligned fused encode+frame: destination-space chunks, DPP rotation   */
/* ------------------------------------------------------------------ */

/* A 65536-B frame image is 4096 aligned 16-B chunks: chunk 0 is
 * [crc | first 12 payload bytes], chunks 1..4095 are payload.  This kernel
 * lays the lane-piece map out in DESTINATION space, so every lane-piece is
 * one aligned uint4 store, and loads one ALIGNED source uint4 per piece:
 * image chunk q of frame f holds shard bytes [p0 + 16q - 4, +16), p0 =
 * f*65532, which start r = (3f - 1) mod 4 dwords into the aligned source
 * chunk L_q at shard offset p0 - 4 - 4r + 16q.  The image chunk is the
 * upper 4-r dwords of L_q followed by the lower r dwords of L_{q+1}, and
 * L_{q+1} is what the NEXT lane loaded: the rotation is r neighbour-lane
 * DPP moves (wave_shl:1, VALU rate, no LDS), done once straight after the
 * load so MAC, CRC and stores all run in destination space (the GF MAC is
 * bytewise: parity accumulators come out destination-aligned).
 *
 * Piece map (wave-contiguous): in pass h (1024 chunks) wave w owns chunks
 * [1024h + 256w, +256), piece i of lane l is chunk 1024h + 256w + 64i + l.
 * Lane 63's donor for pieces 0..2 is lane 0 of the same wave's next piece,
 * already in registers (one wave_rol:1 move feeds it in as the DPP `old`
 * operand); only piece 3 needs one extra ONE-LANE load per unit (lane 63,
 * 12 B).  The lane's pieces are 1024 B apart: Horner chain via g_shift1k.
 *
 * Eligibility (host): dst, dst_stride, base, stripe_stride and shard_len
 * all multiples of 16.  Then every L_q is 16-B aligned in memory and shard
 * ends are 16-B aligned too, so an aligned chunk that holds at least one
 * needed byte lies wholly inside its shard: loads are masked by exactly
 * that rule and never leave the caller's buffer (the one chunk before
 * frame 0 only carries the header slot and is masked).
 *
 * CRC: the header dword of chunk 0 is zeroed in registers; leading zeros
 * do not change the raw zero-init CRC, so the message is the image bytes
 * [0, 4 + payload) and the position operators are image-relative.
 * C0: 0 = chunk 0's 12 payload bytes are stored early (dwordx3 at +4) and
 * the header dword in the epilogue; 1 = they wait in LDS and the epilogue
 * writes [crc | 12 B] as one aligned uint4. */
typedef uint32_t u32x3a __attribute__((ext_vector_type(3)));
struct AlLd {
  uint4 v[4];
  u32x3a e; /* lane 63: low dwords of the chunk after its piece 3 */
};

/* aligned piece loads of one unit; sp = shard + p0 - 4 - 4r (chunk 0).
 * FULL = a whole 65532-B frame: only chunk 0 under r = 3 is masked. */
template <bool FULL>
GFRS_DEV AlLd al_load(const uint8_t *sp, int r, int P, int nfull, int q0) {
  AlLd o;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const int q = q0 + 64 * i;
    const bool lm = FULL ? (i > 0 || q > 0 || r < 3)
                         : (q <= nfull && 16 * q - 4 - 4 * r < P &&
                            16 * q + 12 - 4 * r > 0);
    o.v[i] = lm ? *reinterpret_cast<const uint4 *>(sp + 16 * q)
                : uint4{0, 0, 0, 0};
  }
  const int qe = q0 + 193; /* lane 63: the chunk after its piece 3 */
  const bool em = (q0 & 63) == 63 /* lane 63: q0 = lane (mod 64) */ && r > 0 &&
                  (FULL || (qe <= nfull && 16 * qe - 4 - 4 * r < P));
  o.e = em ? *reinterpret_cast<const u32x3a *>(sp + 16 * qe)
           : u32x3a{0, 0, 0};
  return o;
}

/* lane l <- lane l+1 of `own`; lane 63 <- `edge` */
GFRS_DEV uint32_t al_shl1(uint32_t edge, uint32_t own) {
  return uint32_t(__builtin_amdgcn_update_dpp(int(edge), int(own),
                                              0x130 /* wave_shl:1 */, 0xF,
                                              0xF, false));
}
/* lane 63 <- lane 0 (other lanes unused) */
GFRS_DEV uint32_t al_rol1(uint32_t v) {
  return uint32_t(__builtin_amdgcn_update_dpp(0, int(v),
                                              0x134 /* wave_rol:1 */, 0xF,
                                              0xF, false));
}

/* gf2_mulmod_d, branch-free and fully unrolled: the per-unit fold by the
 * lane's position operator is ~40% of a unit's VALU work in the looped
 * compare/select form; as sign-extended bit masks it is ~6 VALU per bit */
GFRS_DEV uint32_t al_mulmod(uint32_t a, uint32_t b) {
  /* the operator is loop-invariant at every call site: without this the 32
   * bit masks of `a` are hoisted out of the frame loop, where they hold 32
   * VGPRs and 64 SGPRs for the whole kernel and spill */
  asm volatile("" : "+v"(a));
  uint32_t prod = 0;
#pragma unroll
  for (int i = 31; i >= 0; i--) {
    const uint32_t ma = uint32_t(int32_t(a << (31 - i)) >> 31);
    prod ^= b & ma;
    const uint32_t mb = uint32_t(int32_t(b << 31) >> 31);
    b = (b >> 1) ^ (CRC_POLY & mb);
  }
  return prod;
}

/* XOR over the 64 lanes without LDS: two quad swaps and the two row
 * mirrors leave every lane with its 16-lane row's total; the four rows
 * meet in scalar registers.  All lanes must be active. */
GFRS_DEV uint32_t al_wave_xor(uint32_t x) {
  x ^= uint32_t(__builtin_amdgcn_update_dpp(0, int(x), 0xB1 /* quad_perm:
      [1,0,3,2] */, 0xF, 0xF, true));
  x ^= uint32_t(__builtin_amdgcn_update_dpp(0, int(x), 0x4E /* quad_perm:
      [2,3,0,1] */, 0xF, 0xF, true));
  x ^= uint32_t(__builtin_amdgcn_update_dpp(0, int(x),
                                            0x141 /* row_half_mirror */, 0xF,
                                            0xF, true));
  x ^= uint32_t(__builtin_amdgcn_update_dpp(0, int(x), 0x140 /* row_mirror */,
                                            0xF, 0xF, true));
  return uint32_t(__builtin_amdgcn_readlane(int(x), 0) ^
                  __builtin_amdgcn_readlane(int(x), 16) ^
                  __builtin_amdgcn_readlane(int(x), 32) ^
                  __builtin_amdgcn_readlane(int(x), 48));
}

/* piece I of a unit rotated into destination space.  It needs only v[I]
 * and lane 0 of v[I+1], so each loaded piece dies as it is consumed. */
template <int R, int I>
GFRS_DEV uint4 al_rot1(const AlLd &c) {
  const uint4 own = c.v[I];
  uint32_t n[3] = {0, 0, 0};
#pragma unroll
  for (int j = 0; j < R; j++) {
    const uint32_t ownj = j == 0 ? own.x : j == 1 ? own.y : own.z;
    uint32_t edge;
    if (I < 3) {
      const uint4 nx = c.v[I < 3 ? I + 1 : 3];
      edge = al_rol1(j == 0 ? nx.x : j == 1 ? nx.y : nx.z);
    } else {
      edge = j == 0 ? c.e.x : j == 1 ? c.e.y : c.e.z;
    }
    n[j] = al_shl1(edge, ownj);
  }
  return R == 0   ? own
         : R == 1 ? uint4{own.y, own.z, own.w, n[0]}
         : R == 2 ? uint4{own.z, own.w, n[0], n[1]}
                  : uint4{own.w, n[0], n[1], n[2]};
}

/* the frame's rotation r is wave-uniform: one scalar branch per piece */
template <int I>
GFRS_DEV uint4 al_rot_piece(const AlLd &c, int r) {
  switch (r) {
    case 0: return al_rot1<0, I>(c);
    case 1: return al_rot1<1, I>(c);
    case 2: return al_rot1<2, I>(c);
    default: return al_rot1<3, I>(c);
  }
}

/* pins a rotated piece in registers where the switch joins: left free, the
 * compiler turns "dword r of the loaded piece" into an r-indexed read of a
 * private array, and the loaded pieces go through scratch */
GFRS_DEV void al_pin(uint4 &v) {
  asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w));
}

/* LDS bytes ahead of the running-CRC slab (the launch adds (k+m+1) KB for
 * the slab and the coefficient tables) */
constexpr int AL_LDS_FIXED = 12288 + EF_RED + 64 + 256 + 1024 + 256 + 4096;

template <int GM, int WPS, int SKEL = 0, int ST = 0, int C0 = 0, int CRC16 = 0>
__global__ __launch_bounds__(CRC_BLOCKT, WPS) void rs_encode_frame_al_k(
    uint8_t *__restrict__ dst, size_t dst_stride, uint64_t base,
    uint64_t stripe_stride, size_t shard_len, int k,
    const uint8_t *__restrict__ tabs /* [GM*k][32] */, int64_t total_frames,
    int64_t frames_per_shard, int tiny_len /* as rs_encode_frame_reg_k */) {
  constexpr int64_t block_len = 65536;
  constexpr int payload_full = 65532;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  /* crc tables 8 KB | shift1k 4 KB | red slab | x8tab | tailb | tinyb |
   * chunk-0 slab (16 x 16 B) | shift13k 4 KB | running-CRC slab
   * [k+GM][256] dwords and one more row, the lanes' fold operators |
   * coefficient tables */
  uint32_t(*tab)[256] = reinterpret_cast<uint32_t(*)[256]>(smem);
  uint32_t(*stab)[256] = reinterpret_cast<uint32_t(*)[256]>(smem + 8192);
  uint32_t *red = reinterpret_cast<uint32_t *>(smem + 12288);
  uint32_t *x8tab = reinterpret_cast<uint32_t *>(smem + 12288 + EF_RED);
  uint8_t *tailb = smem + 12288 + EF_RED + 64;
  uint8_t *tinyb = smem + 12288 + EF_RED + 64 + 256; /* 16 x 64 */
  uint32_t *c0b =
      reinterpret_cast<uint32_t *>(smem + 12288 + EF_RED + 64 + 256 + 1024);
  uint32_t(*stab13)[256] = reinterpret_cast<uint32_t(*)[256]>(
      smem + 12288 + EF_RED + 64 + 256 + 1024 + 256);
  /* a full frame's running CRC per shard and lane, carried from pass to
   * pass; lane-contiguous, so every access is conflict-free */
  uint32_t *run0 = reinterpret_cast<uint32_t *>(smem + AL_LDS_FIXED);
  uint8_t *ctab = smem + AL_LDS_FIXED + (k + GM + 1) * 1024;
  for (int i = threadIdx.x; i < 2048; i += CRC_BLOCKT)
    (&tab[0][0])[i] = (&g_crc_tab4[0][0])[i];
  for (int i = threadIdx.x; i < 1024; i += CRC_BLOCKT)
    (&stab[0][0])[i] = (&g_shift1k[0][0])[i];
  for (int i = threadIdx.x; i < 1024; i += CRC_BLOCKT)
    (&stab13[0][0])[i] = (&g_shift13k[0][0])[i];
  for (int i = threadIdx.x; i < GM * k * 2; i += CRC_BLOCKT)
    reinterpret_cast<uint4 *>(ctab)[i] =
        reinterpret_cast<const uint4 *>(tabs)[i];
  if (threadIdx.x == 0) {
    uint32_t v = 0x80000000u;
    for (int j = 0; j < 16; j++) {
      x8tab[j] = v;
      v = gf2_mulmod_d(v, g_pow8[0]);
    }
  }
  const int tid = int(threadIdx.x);
  /* lane's piece-0 chunk within a pass: wave-contiguous map */
  const int ql0 = (tid >> 6) * 256 + (tid & 63);
  /* full-frame fold operator: a full frame's CRC is one Horner chain per
   * lane and shard over all 16 pieces (1024 B apart within a pass, 13312 B
   * from piece 3 of a pass to piece 0 of the next), folded once by the
   * suffix after the lane's last piece of pass 3, 16384 - 16*(ql0+193).
   * The chain is built from crc12u_reg pieces, each short of crc16_reg by
   * a factor x^32, which commutes through the chain into the operator: 4
   * bytes more (CRC16 = 1 keeps crc16_reg and the plain suffix).
   * The operator waits in LDS: it is needed once per shard per frame */
  run0[(k + GM) * 256 + tid] =
      x8n_d(uint64_t(16384 - 16 * (ql0 + 192 + 1) + (CRC16 ? 0 : 4)));
  const uint32_t it_full =
      gf2_mulmod_d(x8n_d(uint64_t(payload_full)), 0xFFFFFFFFu);
  __syncthreads();

  const int64_t fr0 = blockIdx.x, frS = gridDim.x;
  int64_t stripe = fr0 / frames_per_shard;
  int64_t f = fr0 - stripe * frames_per_shard;
  const int64_t dstripe = frS / frames_per_shard;
  const int64_t drem = frS - dstripe * frames_per_shard;
  AlLd nx = {};
  if (fr0 < total_frames) { /* later frames are prefetched by the previous
                               frame's last pass */
    const int64_t p0 = f * payload_full;
    const int r = int((3 * f + 3) & 3);
    const int P = int(i64min(payload_full, int64_t(shard_len) - p0));
    nx = al_load<false>(
        as_global(base + stripe * stripe_stride) + (p0 - 4 - 4 * r), r, P,
        (P + 4) >> 4, ql0);
  }
  for (int64_t fr = fr0; fr < total_frames; fr += frS) {
    /* (stripe, f) of this block's next frame, tracked incrementally */
    int64_t stripe2 = stripe + dstripe, f2 = f + drem;
    if (f2 >= frames_per_shard) {
      f2 -= frames_per_shard;
      ++stripe2;
    }
    const int64_t p0 = f * payload_full;
    const int r = int((3 * f + 3) & 3); /* (3f - 1) mod 4 */
    const int P = int(i64min(payload_full, int64_t(shard_len) - p0));
    const int T = P + 4;          /* image bytes of this frame */
    const int nfull = T >> 4;     /* whole chunks */
    const int tb = T & 15;        /* trailing bytes (0, 4, 8 or 12) */
    const int ntot = (T + 15) >> 4;
    const int64_t abase = p0 - 4 - 4 * r; /* shard offset of L_0 */
    const uint8_t *sbase = as_global(base + stripe * stripe_stride);

    /* the lane ids are re-derived per frame behind an opaque copy: without
     * it every lane mask and per-piece offset derived from them is hoisted
     * out of the frame loop and held, mostly spilled, for the whole kernel */
    int tidf = int(threadIdx.x);
    asm volatile("" : "+v"(tidf));
    const int tid = tidf;
    const int ql0 = (tid >> 6) * 256 + (tid & 63);
    uint32_t *run = run0 + tid;

    if (tid < 64) red[tid] = 0;
    __syncthreads();

    /* the four passes; FULL (a whole 65532-B frame, the common case) drops
     * every per-piece validity branch and the tail, so the four pieces of
     * a unit are one straight-line block the scheduler can interleave */
    auto passes = [&](auto fullc) {
    constexpr bool FULL = decltype(fullc)::value;
    uint4 acc[GM][4];
#pragma unroll 1
    for (int h = 0; h < 4; h++) {
      if (!FULL && 1024 * h >= ntot) break;
      int qp = 1024 * h + ql0; /* lane's piece-0 chunk */
      /* ragged frames: keep the per-piece addresses and masks of this
       * rare path from being set up, and spilled, at the top of every frame */
      if (!FULL) asm volatile("" : "+v"(qp));
      const bool tail = !FULL && tb != 0 && (nfull >> 10) == h;
#pragma unroll
      for (int rr = 0; rr < GM; rr++)
#pragma unroll
        for (int i = 0; i < 4; i++) acc[rr][i] = uint4{0, 0, 0, 0};

      uint32_t op = 0; /* ragged and short frames fold every pass */
      if (!FULL) {
        int np = 0;
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (qp + 64 * i < nfull) np = i + 1;
        const int end = np ? 16 * (qp + 64 * (np - 1) + 1) : 0;
        op = x8n_d(uint64_t(T - end));
      }

      for (int c = 0; c < k; c++) {
        const uint8_t *src = sbase + size_t(c) * shard_len;
        uint8_t *fdst =
            dst + (stripe * (k + GM) + c) * dst_stride + f * block_len;
        LinTab lt[GM];
        if (SKEL != 1)
#pragma unroll
          for (int rr = 0; rr < GM; rr++)
            lt[rr] = lintab_load(ctab, rr * k + c);
        const AlLd cur = nx;
        if (c + 1 < k)
          nx = al_load<FULL>(src + shard_len + abase, r, P, nfull, qp);
        /* a full frame continues the shard's chain from the previous pass
         * (pass 0 starts it: a shifted zero is zero) */
        uint32_t t = 0;
        if (FULL && SKEL != 1) t = shift4k(h ? run[c * 256] : 0u, stab13);
        /* one piece at a time: rotate into destination space (all lanes
         * active here, DPP reads neighbour lanes; masked pieces carry
         * zeros), then MAC, store and CRC it */
        auto piece = [&](auto ic) {
          constexpr int i = decltype(ic)::value;
          uint4 v = al_rot_piece<i>(cur, r);
          al_pin(v);
          if (i == 0 && qp == 0) v.x = 0; /* header slot of chunk 0 */
          const int q = qp + 64 * i;
          if (FULL || q < nfull) {
            if (SKEL != 1) {
#pragma unroll
              for (int dd = 0; dd < 4; dd++)
                gfmac4_lin_rows<GM>(acc, i, dd, (&v.x)[dd], lt);
            }
            if (i == 0 && q == 0) {
              if (C0 == 0) {
                *reinterpret_cast<u32x3a *>(fdst + 4) =
                    u32x3a{v.y, v.z, v.w};
              } else {
                c0b[c * 4 + 1] = v.y;
                c0b[c * 4 + 2] = v.z;
                c0b[c * 4 + 3] = v.w;
              }
            } else {
              fstore16<ST>(fdst + 16 * q, v);
            }
            if (SKEL != 1)
              t = (FULL && i == 0 ? t : shift4k(t, stab)) ^
                  (FULL && !CRC16 ? crc12u_reg(v, tab) : crc16_reg(v, tab));
          }
        };
        piece(std::integral_constant<int, 0>{});
        piece(std::integral_constant<int, 1>{});
        piece(std::integral_constant<int, 2>{});
        piece(std::integral_constant<int, 3>{});
        if (FULL) {
          if (SKEL != 1) run[c * 256] = t;
          continue;
        }
        uint32_t part = al_mulmod(op, t);
        if (tail) {
          /* lane-parallel tail: one byte per lane at image offset p */
          const int p = 16 * nfull + tid;
          if (p < T) {
            const uint8_t x = src[p0 + p - 4];
            fdst[p] = x;
            tailb[c * 16 + tid] = x;
            if (SKEL != 1)
              part ^= gf2_mulmod_d(x8tab[T - 1 - p], tab[0][x]);
          }
        }
        part = al_wave_xor(part);
        if ((tid & 63) == 0) red[(tid >> 6) * 16 + c] ^= part;
      }
      if (tail) __syncthreads(); /* tailb visible to all */
      { /* next pass's (or next frame's) unit-0 loads fly during the
           parity rows and the frame epilogue */
        if (FULL ? h < 3 : 1024 * (h + 1) < ntot) {
          nx = al_load<FULL>(sbase + abase, r, P, nfull, qp + 1024);
        } else if (fr + frS < total_frames) {
          const int64_t p02 = f2 * payload_full;
          const int r2 = int((3 * f2 + 3) & 3);
          const int P2 = int(i64min(payload_full, int64_t(shard_len) - p02));
          nx = al_load<false>(as_global(base + stripe2 * stripe_stride) +
                                  (p02 - 4 - 4 * r2),
                              r2, P2, (P2 + 4) >> 4, ql0);
        }
      }
#pragma unroll
      for (int rr = 0; rr < GM; rr++) {
        uint8_t *fdst =
            dst + (stripe * (k + GM) + k + rr) * dst_stride + f * block_len;
        uint32_t t = 0;
        if (FULL && SKEL != 1)
          t = shift4k(h ? run[(k + rr) * 256] : 0u, stab13);
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int q = qp + 64 * i;
          if (FULL || q < nfull) {
            const uint4 v = acc[rr][i];
            if (i == 0 && q == 0) {
              if (C0 == 0) {
                *reinterpret_cast<u32x3a *>(fdst + 4) =
                    u32x3a{v.y, v.z, v.w};
              } else {
                c0b[(k + rr) * 4 + 1] = v.y;
                c0b[(k + rr) * 4 + 2] = v.z;
                c0b[(k + rr) * 4 + 3] = v.w;
              }
            } else {
              fstore16<ST>(fdst + 16 * q, v);
            }
            if (SKEL != 1)
              t = (FULL && i == 0 ? t : shift4k(t, stab)) ^
                  (FULL && !CRC16 ? crc12u_reg(v, tab) : crc16_reg(v, tab));
          }
        }
        if (FULL) {
          if (SKEL != 1) run[(k + rr) * 256] = t;
          continue;
        }
        uint32_t part = al_mulmod(op, t);
        if (SKEL != 1 && tail) {
          const int p = 16 * nfull + tid;
          if (p < T) {
            uint8_t pv = 0;
            for (int c2 = 0; c2 < k; c2++) {
              const uint8_t b = tailb[c2 * 16 + tid];
              pv ^= gfmul1_lin(ctab + size_t(rr * k + c2) * 32, b);
            }
            fdst[p] = pv;
            part ^= gf2_mulmod_d(x8tab[T - 1 - p], tab[0][pv]);
          }
        }
        part = al_wave_xor(part);
        if ((tid & 63) == 0) red[(tid >> 6) * 16 + k + rr] ^= part;
      }
    }
    if (FULL && SKEL != 1) {
      /* one position fold per shard: each lane reads back its own chain */
      const uint32_t op_pD = run[(k + GM) * 256];
      for (int j = 0; j < k + GM; j++) {
        const uint32_t part = al_wave_xor(al_mulmod(op_pD, run[j * 256]));
        if ((tid & 63) == 0) red[(tid >> 6) * 16 + j] ^= part;
      }
    }
    };
    if (P == payload_full)
      passes(std::true_type{});
    else
      passes(std::false_type{});

    __syncthreads();
    { /* one frame-header lane per shard (j < k+GM <= 16, all in wave 0) */
      const int j = tid;
      if (j < k + GM) {
        const uint32_t it =
            P == payload_full
                ? it_full
                : gf2_mulmod_d(x8n_d(uint64_t(P)), 0xFFFFFFFFu);
        const uint32_t crc =
            ~(it ^ red[j] ^ red[16 + j] ^ red[32 + j] ^ red[48 + j]);
        uint8_t *fb0 =
            dst + (stripe * (k + GM) + j) * dst_stride + f * block_len;
        if (C0 == 1 && nfull > 0)
          *reinterpret_cast<uint4 *>(fb0) =
              uint4{crc, c0b[j * 4 + 1], c0b[j * 4 + 2], c0b[j * 4 + 3]};
        else
          *reinterpret_cast<uint32_t *>(fb0) = crc;
      }
    }
    if (tiny_len && f == frames_per_shard - 1) {
      /* folded tiny last frame, as in rs_encode_frame_reg_k */
      const int j = tid;
      const int64_t tp0 = (f + 1) * payload_full;
      if (j < k) {
        const uint8_t *sp = sbase + size_t(j) * shard_len + tp0;
#pragma clang loop vectorize(disable) unroll(disable)
        for (int b = 0; b < tiny_len; b++) tinyb[j * 64 + b] = sp[b];
      }
      __syncthreads();
      if (j < k + GM) {
        uint8_t *tb2 =
            dst + (stripe * (k + GM) + j) * dst_stride + (f + 1) * block_len;
        uint32_t cr = 0;
#pragma clang loop vectorize(disable) unroll(disable)
        for (int b = 0; b < tiny_len; b++) {
          uint8_t x;
          if (j < k) {
            x = tinyb[j * 64 + b];
          } else {
            x = 0;
#pragma clang loop vectorize(disable) unroll(disable)
            for (int c2 = 0; c2 < k; c2++)
              x ^= gfmul1_lin(ctab + size_t((j - k) * k + c2) * 32,
                              tinyb[c2 * 64 + b]);
          }
          tb2[CRC_LEN + b] = x;
          cr = tab[0][(cr ^ x) & 0xFF] ^ (cr >> 8);
        }
        *reinterpret_cast<uint32_t *>(tb2) =
            ~(gf2_mulmod_d(x8n_d(uint64_t(tiny_len)), 0xFFFFFFFFu) ^ cr);
      }
    }
    __syncthreads();
    stripe = stripe2;
    f = f2;
  }
}


/* ------------------------------------------------------------------ */
/* dual-aligned fused encode+frame: 32-B lane pieces, window rotation   */
/* ------------------------------------------------------------------ */

/* The frame format forces a 4 (mod 16) relative shift between a frame's
 * source bytes (shard offset f*65532) and its framed payload (image
 * offset f*65536+4), so one side of the straightforward piece map is
 * always misaligned; measured on the per-block 6r:9w stream mix that
 * costs 14-17% of the ceiling (profiles/: aligned 5.02 TB/s, either side
 * misaligned 4.16-4.33, the production both-misaligned 4.25).  This
 * kernel aligns BOTH sides:
 *  - stores: payload = 28-B prologue + 2047 x 32-B pieces (65532 - 28 =
 *    2047*32).  header(4) + prologue(28) = 32, so piece p stores at
 *    image offset f*65536 + 32 + 32p — 16-B aligned when the image
 *    stride is 16-B aligned; [crc | prologue] is written as two aligned
 *    uint4 in the epilogue.
 *  - loads: a lane's 32-B piece needs the source window
 *    [W + d, W + 32 + d), d = (28 + p0) mod 16 — frame-constant and
 *    always a dword multiple.  The lane loads three ALIGNED uint4
 *    (a 48-B private window) and selects the 8 piece dwords statically
 *    under a per-frame uniform branch on D0 = d/4.  No cross-lane
 *    traffic; the trailing over-read (<= 16 B) stays inside the stripe
 *    (a data shard is always followed by more shard space, m >= 1).
 * CRC bookkeeping follows rs_encode_frame_reg_k with lane-piece stride
 * 8192 (x^(8*8192) Horner tables g_shift8k) and a 32-entry x8tab for
 * sub-32-B byte tails. */

/* one slice-by-4 CRC step over a dword */
GFRS_DEV uint32_t crc_dw(uint32_t c, uint32_t w, const uint32_t (*tab)[256]) {
  c ^= w;
  return tab[3][c & 0xFF] ^ tab[2][(c >> 8) & 0xFF] ^
         tab[1][(c >> 16) & 0xFF] ^ tab[0][c >> 24];
}

GFRS_DEV uint32_t shift8k(uint32_t c, const uint32_t (*stab)[256]) {
  return xor3(stab[0][c & 0xFF], stab[1][(c >> 8) & 0xFF],
              stab[2][(c >> 16) & 0xFF]) ^
         stab[3][c >> 24];
}

/* raw CRC of 32 B held in two uint4 (slice-by-8, 4 steps) */
GFRS_DEV uint32_t crc32_reg(const uint4 qa, const uint4 qb,
                            const uint32_t (*tab)[256]) {
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const uint32_t w0 =
        (j == 0 ? qa.x : j == 1 ? qa.z : j == 2 ? qb.x : qb.z) ^ c;
    const uint32_t w1 = (j == 0 ? qa.y : j == 1 ? qa.w : j == 2 ? qb.y : qb.w);
    c = xor3(xor3(tab[7][w0 & 0xFF], tab[6][(w0 >> 8) & 0xFF],
                  tab[5][(w0 >> 16) & 0xFF]),
             xor3(tab[4][w0 >> 24], tab[3][w1 & 0xFF],
                  tab[2][(w1 >> 8) & 0xFF]),
             tab[1][(w1 >> 16) & 0xFF] ^ tab[0][w1 >> 24]);
  }
  return c;
}

/* load only the D0 dwords of the window tail that the rotation consumes
 * (unused uint4 components are DCE'd, so this trims both registers and
 * line requests) */
typedef uint32_t u32x3_t __attribute__((ext_vector_type(3)));
template <int D0>
GFRS_DEV void rot_tail_load(uint4 &w2, const uint8_t *p) {
  if (D0 == 1) {
    w2.x = *reinterpret_cast<const uint32_t *>(p);
  } else if (D0 == 2) {
    const uint2 t = *reinterpret_cast<const uint2 *>(p);
    w2.x = t.x;
    w2.y = t.y;
  } else if (D0 == 3) {
    const u32x3_t t = *reinterpret_cast<const u32x3_t *>(p);
    w2.x = t.x;
    w2.y = t.y;
    w2.z = t.z;
  }
}

/* statically select the 8 piece dwords out of the lane's 12-dword
 * aligned window (D0 = frame shift / 4) */
template <int D0>
GFRS_DEV void rot_pick(uint4 &h0, uint4 &h1, const uint4 w0, const uint4 w1,
                       const uint4 w2) {
  const uint32_t a[12] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y,
                          w1.z, w1.w, w2.x, w2.y, w2.z, w2.w};
  h0 = uint4{a[D0], a[D0 + 1], a[D0 + 2], a[D0 + 3]};
  h1 = uint4{a[D0 + 4], a[D0 + 5], a[D0 + 6], a[D0 + 7]};
}

struct RotArgs {
  uint8_t *dst;
  const uint8_t *sbase;
  size_t dst_stride, shard_len;
  int64_t stripe, f, p0, payload, payload_eff;
  int k;
  const uint8_t *ctab;
  const uint32_t (*tab)[256];
  const uint32_t (*stab)[256]; /* g_shift8k */
  uint32_t *red;
  const uint32_t *x8tab;
  uint8_t *tailb;
  uint32_t op_first;
};

template <int D0, int GM, int ST>
GFRS_DEV void rot_passes(const RotArgs A) {
  /* NOTE: args by VALUE and every acc[]/window[] index a compile-time
   * constant — a by-ref struct or a runtime-indexed accumulator array
   * is materialized in scratch and the piece loop serializes behind
   * vmcnt(0) drains (measured 3x slower). */
  constexpr int EF_PASS = 16384;
  constexpr int EF_PASSES = 4;
  constexpr int64_t block_len = 65536;
  constexpr int64_t payload_full = block_len - CRC_LEN;
  constexpr uint32_t INV16K = 0x479933FCu;
  const int tid = int(threadIdx.x);
  const int64_t lane32 = int64_t(tid) * 32;
  const int lane32i = tid * 32;
  const int k = A.k;

  uint4 acc[GM][4]; /* [row][piece*2 + half], constant-indexed */
  uint32_t op_chain = A.op_first;

  for (int h = 0; h < EF_PASSES; h++) {
    const int64_t r0 = int64_t(h) * EF_PASS;
    const int64_t rbytes = i64min(int64_t(EF_PASS), A.payload_eff - r0);
    if (rbytes <= 0) break;
#pragma unroll
    for (int r = 0; r < GM; r++)
#pragma unroll
      for (int q = 0; q < 4; q++) acc[r][q] = uint4{0, 0, 0, 0};

    uint32_t op = op_chain;
    if (h == EF_PASSES - 1 && tid == 255)
      op = shift8k(op, A.stab); /* lane 255's last pass has 1 piece */
    op_chain = gf2_mulmod_d(op_chain, INV16K);
    if (A.payload != payload_full) {
      int np = 0;
#pragma unroll
      for (int i = 0; i < 2; i++)
        if (int64_t(i) * 8192 + lane32 + 32 <= rbytes) np = i + 1;
      const int64_t end = np ? r0 + int64_t(np - 1) * 8192 + lane32 + 32 : r0;
      op = x8n_d(uint64_t(A.payload_eff - end));
    }

    const int rbi = int(rbytes);
    /* aligned window base of this pass (D0*4 = the frame shift) */
    const int64_t wbase = A.p0 + 28 - int64_t(D0) * 4 + r0;
    const bool v0 = lane32i + 32 <= rbi;
    const bool v1 = 8192 + lane32i + 32 <= rbi;

    /* two rolling window buffers (one per piece half), each refilled for
     * the next unit right after its consume: ~6 loads in flight, and
     * both the buffers and the accumulator halves keep constant
     * register indices */
    uint4 wA[3], wB[3];
    {
      const uint8_t *wp = A.sbase + wbase;
      wA[0] = v0 ? *reinterpret_cast<const uint4 *>(wp + lane32i)
                 : uint4{0, 0, 0, 0};
      wA[1] = v0 ? *reinterpret_cast<const uint4 *>(wp + lane32i + 16)
                 : uint4{0, 0, 0, 0};
      wA[2] = uint4{0, 0, 0, 0};
      if (v0 && D0 != 0) rot_tail_load<D0>(wA[2], wp + lane32i + 32);
      const int offb = 8192 + lane32i;
      wB[0] = v1 ? *reinterpret_cast<const uint4 *>(wp + offb)
                 : uint4{0, 0, 0, 0};
      wB[1] = v1 ? *reinterpret_cast<const uint4 *>(wp + offb + 16)
                 : uint4{0, 0, 0, 0};
      wB[2] = uint4{0, 0, 0, 0};
      if (v1 && D0 != 0) rot_tail_load<D0>(wB[2], wp + offb + 32);
    }

    for (int c = 0; c < k; c++) {
      LinTab lt[GM];
#pragma unroll
      for (int r = 0; r < GM; r++) lt[r] = lintab_load(A.ctab, r * k + c);
      uint8_t *fdst = A.dst + (A.stripe * (k + GM) + c) * A.dst_stride +
                      A.f * block_len + 32 + r0;
      const uint8_t *wnext =
          c + 1 < k ? A.sbase + size_t(c + 1) * A.shard_len + wbase : nullptr;
      uint32_t t = 0;
      { /* piece half 0 */
        uint4 cw0 = wA[0], cw1 = wA[1], cw2 = wA[2];
        if (wnext) {
          wA[0] = v0 ? *reinterpret_cast<const uint4 *>(wnext + lane32i)
                     : uint4{0, 0, 0, 0};
          wA[1] = v0 ? *reinterpret_cast<const uint4 *>(wnext + lane32i + 16)
                     : uint4{0, 0, 0, 0};
          if (v0 && D0 != 0) rot_tail_load<D0>(wA[2], wnext + lane32i + 32);
        }
        if (v0) {
          uint4 h0, h1;
          rot_pick<D0>(h0, h1, cw0, cw1, cw2);
#pragma unroll
          for (int d = 0; d < 4; d++)
            gfmac4_lin_rows<GM>(acc, 0, d, (&h0.x)[d], lt);
#pragma unroll
          for (int d = 0; d < 4; d++)
            gfmac4_lin_rows<GM>(acc, 1, d, (&h1.x)[d], lt);
          fstore16<ST>(fdst + lane32i, h0);
          fstore16<ST>(fdst + lane32i + 16, h1);
          t = crc32_reg(h0, h1, A.tab);
        }
      }
      { /* piece half 1 */
        uint4 cw0 = wB[0], cw1 = wB[1], cw2 = wB[2];
        const int offb = 8192 + lane32i;
        if (wnext) {
          wB[0] = v1 ? *reinterpret_cast<const uint4 *>(wnext + offb)
                     : uint4{0, 0, 0, 0};
          wB[1] = v1 ? *reinterpret_cast<const uint4 *>(wnext + offb + 16)
                     : uint4{0, 0, 0, 0};
          if (v1 && D0 != 0) rot_tail_load<D0>(wB[2], wnext + offb + 32);
        }
        if (v1) {
          uint4 h0, h1;
          rot_pick<D0>(h0, h1, cw0, cw1, cw2);
#pragma unroll
          for (int d = 0; d < 4; d++)
            gfmac4_lin_rows<GM>(acc, 2, d, (&h0.x)[d], lt);
#pragma unroll
          for (int d = 0; d < 4; d++)
            gfmac4_lin_rows<GM>(acc, 3, d, (&h1.x)[d], lt);
          fstore16<ST>(fdst + offb, h0);
          fstore16<ST>(fdst + offb + 16, h1);
          t = shift8k(t, A.stab) ^ crc32_reg(h0, h1, A.tab);
        }
      }
      uint32_t part = t ? gf2_mulmod_d(op, t) : 0;
      if (rbi & 31) {
        const uint8_t *src = A.sbase + size_t(c) * A.shard_len + A.p0 + 28 + r0;
        const int t0 = rbi & ~31;
        const int p = t0 + tid;
        if (p < rbi) {
          const uint8_t x = src[p];
          fdst[p] = x;
          A.tailb[c * 32 + (p - t0)] = x;
          part ^= gf2_mulmod_d(A.x8tab[rbi - 1 - p], A.tab[0][x]);
        }
      }
#pragma unroll
      for (int sh = 32; sh > 0; sh >>= 1) part ^= __shfl_xor(part, sh, 64);
      if ((tid & 63) == 0) A.red[(tid >> 6) * 16 + c] ^= part;
    }
    if (rbi & 31) __syncthreads(); /* tailb visible to the parity rows */
#pragma unroll
    for (int r = 0; r < GM; r++) {
      uint8_t *fdst = A.dst + (A.stripe * (k + GM) + k + r) * A.dst_stride +
                      A.f * block_len + 32 + r0;
      uint32_t tr = 0;
      if (v0) {
        fstore16<ST>(fdst + lane32i, acc[r][0]);
        fstore16<ST>(fdst + lane32i + 16, acc[r][1]);
        tr = crc32_reg(acc[r][0], acc[r][1], A.tab);
      }
      if (v1) {
        fstore16<ST>(fdst + 8192 + lane32i, acc[r][2]);
        fstore16<ST>(fdst + 8192 + lane32i + 16, acc[r][3]);
        tr = shift8k(tr, A.stab) ^ crc32_reg(acc[r][2], acc[r][3], A.tab);
      }
      uint32_t part = tr ? gf2_mulmod_d(op, tr) : 0;
      if (rbi & 31) {
        const int t0 = rbi & ~31;
        const int p = t0 + tid;
        if (p < rbi) {
          uint8_t pv = 0;
          for (int c2 = 0; c2 < k; c2++)
            pv ^= gfmul1_lin(A.ctab + size_t(r * k + c2) * 32,
                             A.tailb[c2 * 32 + (p - t0)]);
          fdst[p] = pv;
          part ^= gf2_mulmod_d(A.x8tab[rbi - 1 - p], A.tab[0][pv]);
        }
      }
#pragma unroll
      for (int sh = 32; sh > 0; sh >>= 1) part ^= __shfl_xor(part, sh, 64);
      if ((tid & 63) == 0) A.red[(tid >> 6) * 16 + k + r] ^= part;
    }
  }
}

template <int GM, int WPS, int ST>
__global__ __launch_bounds__(CRC_BLOCKT, WPS) void rs_encode_frame_rot_k(
    uint8_t *__restrict__ dst, size_t dst_stride, uint64_t base,
    uint64_t stripe_stride, size_t shard_len, int k,
    const uint8_t *__restrict__ tabs /* linear A|B|C region */,
    int64_t total_frames, int64_t frames_per_shard) {
  constexpr int64_t block_len = 65536;
  constexpr int64_t payload_full = block_len - CRC_LEN;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  /* crc tabs 8K | shift8k 4K | red | x8tab(32) | tailb(16x32) | ctab */
  uint32_t(*tab)[256] = reinterpret_cast<uint32_t(*)[256]>(smem);
  uint32_t(*stab)[256] = reinterpret_cast<uint32_t(*)[256]>(smem + 8192);
  uint32_t *red = reinterpret_cast<uint32_t *>(smem + 12288);
  uint32_t *x8tab = reinterpret_cast<uint32_t *>(smem + 12288 + EF_RED);
  uint8_t *tailb = smem + 12288 + EF_RED + 128;
  uint8_t *ctab = smem + 12288 + EF_RED + 128 + 512;
  for (int i = threadIdx.x; i < 2048; i += CRC_BLOCKT)
    (&tab[0][0])[i] = (&g_crc_tab4[0][0])[i];
  for (int i = threadIdx.x; i < 1024; i += CRC_BLOCKT)
    (&stab[0][0])[i] = (&g_shift8k[0][0])[i];
  for (int i = threadIdx.x; i < GM * k * 2; i += CRC_BLOCKT)
    reinterpret_cast<uint4 *>(ctab)[i] =
        reinterpret_cast<const uint4 *>(tabs)[i];
  if (threadIdx.x == 0) {
    uint32_t v = 0x80000000u;
    for (int j = 0; j < 32; j++) {
      x8tab[j] = v;
      v = gf2_mulmod_d(v, g_pow8[0]);
    }
  }
  const uint32_t op_first = x8n_d(
      uint64_t(payload_full - 28 - (8192 + int64_t(threadIdx.x) * 32 + 32)));
  const uint32_t it_full =
      gf2_mulmod_d(x8n_d(uint64_t(payload_full)), 0xFFFFFFFFu);
  const uint32_t p28_full = x8n_d(uint64_t(payload_full - 28));
  __syncthreads();

  int64_t stripe = int64_t(blockIdx.x) / frames_per_shard;
  int64_t f = int64_t(blockIdx.x) - stripe * frames_per_shard;
  const int64_t frS = gridDim.x;
  const int64_t dstripe = frS / frames_per_shard;
  const int64_t drem = frS - dstripe * frames_per_shard;
  for (int64_t fr = blockIdx.x; fr < total_frames; fr += frS,
               stripe += dstripe, f += drem,
               (f >= frames_per_shard ? (f -= frames_per_shard, ++stripe)
                                      : int64_t(0))) {
    RotArgs A;
    A.dst = dst;
    A.sbase = as_global(base + stripe * stripe_stride);
    A.dst_stride = dst_stride;
    A.shard_len = shard_len;
    A.stripe = stripe;
    A.f = f;
    A.p0 = f * payload_full;
    A.payload = i64min(payload_full, int64_t(shard_len) - A.p0);
    const int64_t pfx = i64min(int64_t(28), A.payload);
    A.payload_eff = A.payload - pfx;
    A.k = k;
    A.ctab = ctab;
    A.tab = tab;
    A.stab = stab;
    A.red = red;
    A.x8tab = x8tab;
    A.tailb = tailb;
    A.op_first = op_first;

    for (int j = threadIdx.x; j < 64; j += CRC_BLOCKT) red[j] = 0;
    __syncthreads();

    /* frame-constant source shift: (28 + p0) mod 16, always a multiple
     * of 4; one uniform branch selects the static rotation */
    switch (int((28 + A.p0) & 15) >> 2) {
      case 0: rot_passes<0, GM, ST>(A); break;
      case 1: rot_passes<1, GM, ST>(A); break;
      case 2: rot_passes<2, GM, ST>(A); break;
      default: rot_passes<3, GM, ST>(A); break;
    }

    __syncthreads();
    { /* header + 28-B payload prologue, one lane per shard */
      const int j = int(threadIdx.x);
      const int pfxi = int(pfx);
      uint32_t pw[7] = {0, 0, 0, 0, 0, 0, 0};
      if (j < k && pfxi) {
        const uint8_t *sp = A.sbase + size_t(j) * shard_len + A.p0;
        if (pfxi == 28) {
#pragma unroll
          for (int w = 0; w < 7; w++)
            pw[w] = *reinterpret_cast<const uint32_t *>(sp + 4 * w);
        } else {
          for (int b = 0; b < pfxi; b++)
            reinterpret_cast<uint8_t *>(pw)[b] = sp[b];
        }
        for (int b = 0; b < pfxi; b++)
          tailb[j * 32 + b] = reinterpret_cast<const uint8_t *>(pw)[b];
      }
      __syncthreads();
      if (j < k + GM) {
        if (j >= k && pfxi) {
          for (int b = 0; b < pfxi; b++) {
            uint8_t pv = 0;
            for (int c2 = 0; c2 < k; c2++)
              pv ^= gfmul1_lin(ctab + size_t((j - k) * k + c2) * 32,
                               tailb[c2 * 32 + b]);
            reinterpret_cast<uint8_t *>(pw)[b] = pv;
          }
        }
        uint32_t pcon = 0;
        if (pfxi) {
          uint32_t cp = 0;
          if (pfxi == 28) {
#pragma unroll
            for (int w = 0; w < 7; w++) cp = crc_dw(cp, pw[w], tab);
          } else {
            for (int b = 0; b < pfxi; b++)
              cp = tab[0][(cp ^ reinterpret_cast<const uint8_t *>(pw)[b]) &
                          0xFF] ^
                   (cp >> 8);
          }
          pcon = A.payload == payload_full ? gf2_mulmod_d(p28_full, cp)
                 : A.payload_eff
                     ? gf2_mulmod_d(x8n_d(uint64_t(A.payload_eff)), cp)
                     : cp;
        }
        const uint32_t it =
            A.payload == payload_full
                ? it_full
                : gf2_mulmod_d(x8n_d(uint64_t(A.payload)), 0xFFFFFFFFu);
        const uint32_t crc =
            ~(it ^ pcon ^ red[j] ^ red[16 + j] ^ red[32 + j] ^ red[48 + j]);
        uint8_t *fb0 =
            dst + (stripe * (k + GM) + j) * dst_stride + f * block_len;
        if (pfxi == 28) {
          fstore16<ST>(fb0, uint4{crc, pw[0], pw[1], pw[2]});
          fstore16<ST>(fb0 + 16, uint4{pw[3], pw[4], pw[5], pw[6]});
        } else {
          *reinterpret_cast<uint32_t *>(fb0) = crc;
          for (int b = 0; b < pfxi; b++)
            fb0[CRC_LEN + b] = reinterpret_cast<const uint8_t *>(pw)[b];
        }
      }
    }
    __syncthreads();
  }
}

/* ------------------------------------------------------------------ */
/* fused repair: reconstruct + verify + crc32block-framed images        */
/* ------------------------------------------------------------------ */

/* The blobnode repair tasklet (worker_slice_recover.go) reconstructs the
 * lost shards from k survivors, verifies parity consistency, and writes
 * the repaired shards as framed disk images.  As three passes that is
 * read k+ncmp, write nbad raw, read nbad, write nbad framed.  Fused:
 * the k inputs and ncmp check shards are read ONCE and only the nbad
 * framed bodies are written - the raw reconstruction never exists in
 * HBM.  Rows 0..nw-1 rebuild lost shards (framed output; image column
 * from colpack, 4 bits per row); rows nw.. are surviving-parity checks
 * (compared against the shard itself, mismatch -> fail[stripe]).
 * Same op-chain CRC machinery as rs_encode_frame_reg_k. */
template <int GM, int WPS = 4>
__global__ __launch_bounds__(CRC_BLOCKT, WPS) void rs_repair_frame_k(
    uint8_t *__restrict__ dst /* first image body (+32 into the image) */,
    size_t dst_stride /* whole-image stride */, uint64_t base,
    uint64_t stripe_stride, size_t shard_len, int k,
    const int32_t *__restrict__ imap /* k inputs then GM-nw cmp shards */,
    const uint8_t *__restrict__ tabs /* [GM*k][32] */, int nw,
    uint32_t colpack, uint32_t *__restrict__ fail, int64_t total_frames,
    int64_t frames_per_shard) {
  constexpr int EF_PASS = 16384;
  constexpr int EF_PASSES = 4;
  constexpr int64_t block_len = 65536;
  constexpr int64_t payload_full = block_len - CRC_LEN;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t(*tab)[256] = reinterpret_cast<uint32_t(*)[256]>(smem);
  uint32_t(*stab)[256] = reinterpret_cast<uint32_t(*)[256]>(smem + 8192);
  uint32_t *red = reinterpret_cast<uint32_t *>(smem + 12288);
  /* x^(8*j), j<16: position operators for the <16-byte pass tails */
  uint32_t *x8tab = reinterpret_cast<uint32_t *>(smem + 12288 + EF_RED);
  /* staged tail bytes of the (up to 16) input shards: the parity tails
   * read these from LDS instead of k dependent global loads per lane */
  uint8_t *tailb = smem + 12288 + EF_RED + 64;
  uint8_t *ctab = smem + 12288 + EF_RED + 64 + 256;
  for (int i = threadIdx.x; i < 2048; i += CRC_BLOCKT)
    (&tab[0][0])[i] = (&g_crc_tab4[0][0])[i];
  for (int i = threadIdx.x; i < 1024; i += CRC_BLOCKT)
    (&stab[0][0])[i] = (&g_shift4k[0][0])[i];
  for (int i = threadIdx.x; i < GM * k * 2; i += CRC_BLOCKT)
    reinterpret_cast<uint4 *>(ctab)[i] =
        reinterpret_cast<const uint4 *>(tabs)[i];
  if (threadIdx.x == 0) {
    uint32_t v = 0x80000000u;
    for (int j = 0; j < 16; j++) {
      x8tab[j] = v;
      v = gf2_mulmod_d(v, g_pow8[0]);
    }
  }
  const int64_t lane16 = int64_t(threadIdx.x) * 16;
  const int lane16i = int(threadIdx.x) * 16;
  constexpr uint32_t INV16K = 0x479933FCu;
  const uint32_t op_first =
      x8n_d(uint64_t(payload_full - (3 * 4096 + lane16 + 16)));
  const uint32_t op_pA = op_first;
  const uint32_t op_pB = gf2_mulmod_d(op_pA, INV16K);
  const uint32_t op_pC = gf2_mulmod_d(op_pB, INV16K);
  const uint32_t op_pD = gf2_mulmod_d(op_pC, INV16K);
  const uint32_t it_full =
      gf2_mulmod_d(x8n_d(uint64_t(payload_full)), 0xFFFFFFFFu);
  __syncthreads();


  int64_t stripe = int64_t(blockIdx.x) / frames_per_shard;
  int64_t f = int64_t(blockIdx.x) - stripe * frames_per_shard;
  const int64_t dstripe = int64_t(gridDim.x) / frames_per_shard;
  const int64_t drem = int64_t(gridDim.x) - dstripe * frames_per_shard;
  for (int64_t fr = blockIdx.x; fr < total_frames; fr += gridDim.x,
               stripe += dstripe, f += drem,
               (f >= frames_per_shard ? (f -= frames_per_shard, ++stripe)
                                      : int64_t(0))) {
    const int64_t p0 = f * payload_full;
    const int64_t payload = i64min(payload_full, int64_t(shard_len) - p0);
    const uint8_t *sbase = as_global(base + stripe * stripe_stride);

    uint4 acc[GM][4];
    uint4 vnext[4];
    { /* prefetch pass 0, unit 0 */
      const int rb0 = int(i64min(int64_t(EF_PASS), payload));
      const uint8_t *src0 = sbase + size_t(imap[0]) * shard_len + p0;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int off = i * 4096 + lane16i;
        vnext[i] = off + 16 <= rb0
                       ? *reinterpret_cast<const uint4 *>(src0 + off)
                       : uint4{0, 0, 0, 0};
      }
    }
    for (int j = threadIdx.x; j < 64; j += CRC_BLOCKT) red[j] = 0;
    __syncthreads();

    uint32_t mismatch = 0;
    for (int h = 0; h < EF_PASSES; h++) {
      const int64_t r0 = int64_t(h) * EF_PASS;
      const int64_t rbytes = i64min(int64_t(EF_PASS), payload - r0);
      if (rbytes <= 0) break;
#pragma unroll
      for (int r = 0; r < GM; r++)
#pragma unroll
        for (int i = 0; i < 4; i++) acc[r][i] = uint4{0, 0, 0, 0};

      uint32_t op = h == 0   ? op_pA
                    : h == 1 ? op_pB
                    : h == 2 ? op_pC
                             : op_pD;
      if (h == EF_PASSES - 1 && threadIdx.x == 255)
        op = shift4k(op, stab);
      if (payload != payload_full) {
        int np = 0;
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (int64_t(i) * 4096 + lane16 + 16 <= rbytes) np = i + 1;
        const int64_t end =
            np ? r0 + int64_t(np - 1) * 4096 + lane16 + 16 : r0;
        op = x8n_d(uint64_t(payload - end));
      }

      const int rbi = int(rbytes);
      for (int c = 0; c < k; c++) {
        uint4 vcur[4];
#pragma unroll
        for (int i = 0; i < 4; i++) vcur[i] = vnext[i];
        if (c + 1 < k) { /* next input's loads fly over this MAC */
          const uint8_t *nsrc =
              sbase + size_t(imap[c + 1]) * shard_len + p0 + r0;
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const int off = i * 4096 + lane16i;
            vnext[i] = off + 16 <= rbi
                           ? *reinterpret_cast<const uint4 *>(nsrc + off)
                           : uint4{0, 0, 0, 0};
          }
        }
        LinTab lt[GM];
#pragma unroll
        for (int r = 0; r < GM; r++) lt[r] = lintab_load(ctab, r * k + c);
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int off = i * 4096 + lane16i;
          if (off + 16 <= rbi) {
#pragma unroll
            for (int d = 0; d < 4; d++)
              gfmac4_lin_rows<GM>(acc, i, d, (&vcur[i].x)[d], lt);
          }
        }
      }
      { /* prefetch next pass's (or frame's) unit-0 loads */
        int64_t r0n = r0 + EF_PASS;
        int64_t rbn = i64min(int64_t(EF_PASS), payload - r0n);
        const uint8_t *nbase = sbase + size_t(imap[0]) * shard_len + p0;
        if (rbn <= 0 && fr + gridDim.x < total_frames) {
          const int64_t fr2 = fr + gridDim.x;
          const int64_t st2 = fr2 / frames_per_shard;
          const int64_t p02 = (fr2 - st2 * frames_per_shard) * payload_full;
          rbn = i64min(int64_t(EF_PASS), int64_t(shard_len) - p02);
          nbase = as_global(base + st2 * stripe_stride) +
                  size_t(imap[0]) * shard_len + p02;
          r0n = 0;
        }
        if (rbn > 0) {
          const int rbni = int(rbn);
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const int off = i * 4096 + lane16i;
            vnext[i] = off + 16 <= rbni
                           ? *reinterpret_cast<const uint4 *>(nbase + r0n + off)
                           : uint4{0, 0, 0, 0};
          }
        }
      }
      if (rbytes < EF_PASS) { /* stage input tail bytes: lane (c,j) */
        const int tt0 = (rbi / 16) * 16;
        const int c2 = int(threadIdx.x) >> 4, j = int(threadIdx.x) & 15;
        if (c2 < k && tt0 + j < rbi)
          tailb[c2 * 16 + j] =
              sbase[size_t(imap[c2]) * shard_len + p0 + r0 + tt0 + j];
        __syncthreads();
      }
#pragma unroll
      for (int r = 0; r < GM; r++) {
        if (r < nw) { /* rebuild row: framed image output */
          const int col = int((colpack >> (4 * r)) & 0xF);
          uint8_t *fdst = dst + (stripe * nw + col) * dst_stride +
                          f * block_len + CRC_LEN + r0;
          uint32_t t = 0;
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const int off = i * 4096 + lane16i;
            if (off + 16 <= rbi) {
              uint32_t *dw = reinterpret_cast<uint32_t *>(fdst + off);
              dw[0] = acc[r][i].x; dw[1] = acc[r][i].y;
              dw[2] = acc[r][i].z; dw[3] = acc[r][i].w;
              t = shift4k(t, stab) ^ crc16_reg(acc[r][i], tab);
            }
          }
          uint32_t part = t ? gf2_mulmod_d(op, t) : 0;
          if (rbytes < EF_PASS) { /* lane-parallel tail (see encode) */
            const int t0 = (rbi / 16) * 16;
            const int p = t0 + int(threadIdx.x);
            if (p < rbi) {
              uint8_t pv = 0;
              for (int c2 = 0; c2 < k; c2++) {
                const uint8_t b2 = tailb[c2 * 16 + (p - t0)];
                pv ^= gfmul1_lin(ctab + size_t(r * k + c2) * 32, b2);
              }
              fdst[p] = pv;
              part ^= gf2_mulmod_d(x8tab[rbi - 1 - p], tab[0][pv]);
            }
          }
#pragma unroll
          for (int sh = 32; sh > 0; sh >>= 1)
            part ^= __shfl_xor(part, sh, 64);
          if ((threadIdx.x & 63) == 0)
            red[(threadIdx.x >> 6) * 16 + r] ^= part;
        } else { /* check row: compare against the surviving parity */
          const uint8_t *cshard =
              sbase + size_t(imap[k + (r - nw)]) * shard_len + p0 + r0;
          uint32_t d = 0;
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const int off = i * 4096 + lane16i;
            if (off + 16 <= rbi) {
              const uint4 w =
                  *reinterpret_cast<const uint4 *>(cshard + off);
              d |= (w.x ^ acc[r][i].x) | (w.y ^ acc[r][i].y) |
                   (w.z ^ acc[r][i].z) | (w.w ^ acc[r][i].w);
            }
          }
          if (rbytes < EF_PASS) {
            const int t0 = (rbi / 16) * 16;
            const int p = t0 + int(threadIdx.x);
            if (p < rbi) {
              uint8_t pv = 0;
              for (int c2 = 0; c2 < k; c2++) {
                const uint8_t b2 = tailb[c2 * 16 + (p - t0)];
                pv ^= gfmul1_lin(ctab + size_t(r * k + c2) * 32, b2);
              }
              d |= uint32_t(pv ^ cshard[p]);
            }
          }
          mismatch |= d;
        }
      }
    }

    /* fail flag + the 4 B LE frame headers of the rebuilt images */
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1)
      mismatch |= __shfl_xor(mismatch, sh, 64);
    __syncthreads();
    {
      const int r = int(threadIdx.x);
      if (r < nw) {
        const uint32_t it =
            payload == payload_full
                ? it_full
                : gf2_mulmod_d(x8n_d(uint64_t(payload)), 0xFFFFFFFFu);
        const int col = int((colpack >> (4 * r)) & 0xF);
        const uint32_t crc =
            ~(it ^ red[r] ^ red[16 + r] ^ red[32 + r] ^ red[48 + r]);
        *reinterpret_cast<uint32_t *>(
            dst + (stripe * nw + col) * dst_stride + f * block_len) = crc;
      }
    }
    if ((threadIdx.x & 63) == 0 && mismatch)
      atomicOr(&fail[stripe], 1u);
    __syncthreads();
  }
}

/* Small-shard fused repair: wave-per-stripe variant of rs_repair_frame_k
 * for shards <= 4096 B (one short frame).  Same plan/imap/colpack
 * contract; inputs MAC-only, rebuild rows become framed image bodies,
 * check rows compare against the surviving shard; input tail bytes are
 * staged in a wave-local LDS slab (same-wave visibility, no barriers). */
template <int GM, int NI>
__global__ __launch_bounds__(CRC_BLOCKT, 4) void rs_repair_frame_small_k(
    uint8_t *__restrict__ dst, size_t dst_stride, uint64_t base,
    uint64_t stripe_stride, size_t shard_len, int k,
    const int32_t *__restrict__ imap, const uint8_t *__restrict__ tabs,
    int nw, uint32_t colpack, uint32_t *__restrict__ fail,
    int64_t nstripes) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t(*tab)[256] = reinterpret_cast<uint32_t(*)[256]>(smem);
  uint32_t(*stab)[256] = reinterpret_cast<uint32_t(*)[256]>(smem + 8192);
  uint32_t *x8tab = reinterpret_cast<uint32_t *>(smem + 12288);
  uint8_t *tailb = smem + 12288 + 64;
  uint8_t *ctab = smem + 12288 + 64 + 4 * 256;
  for (int i = threadIdx.x; i < 2048; i += CRC_BLOCKT)
    (&tab[0][0])[i] = (&g_crc_tab4[0][0])[i];
  for (int i = threadIdx.x; i < 1024; i += CRC_BLOCKT)
    (&stab[0][0])[i] = (&g_shift1k[0][0])[i];
  for (int i = threadIdx.x; i < GM * k * 2; i += CRC_BLOCKT)
    reinterpret_cast<uint4 *>(ctab)[i] =
        reinterpret_cast<const uint4 *>(tabs)[i];
  if (threadIdx.x == 0) {
    uint32_t v = 0x80000000u;
    for (int j = 0; j < 16; j++) {
      x8tab[j] = v;
      v = gf2_mulmod_d(v, g_pow8[0]);
    }
  }
  __syncthreads();

  const int wv = int(threadIdx.x) >> 6, lane = int(threadIdx.x) & 63;
  const int lane16i = lane * 16;
  uint8_t *wtail = tailb + wv * 256;
  const int pli = int(shard_len);
  int np = 0;
#pragma unroll
  for (int i = 0; i < NI; i++)
    if (i * 1024 + lane16i + 16 <= pli) np = i + 1;
  const uint32_t op =
      np ? x8n_d(uint64_t(pli - ((np - 1) * 1024 + lane16i + 16))) : 0;
  const uint32_t it = gf2_mulmod_d(x8n_d(uint64_t(pli)), 0xFFFFFFFFu);
  const int t0 = (pli / 16) * 16;

  for (int64_t stripe = int64_t(blockIdx.x) * 4 + wv; stripe < nstripes;
       stripe += int64_t(gridDim.x) * 4) {
    const uint8_t *sbase = as_global(base + stripe * stripe_stride);
    uint4 acc[GM][NI];
#pragma unroll
    for (int r = 0; r < GM; r++)
#pragma unroll
      for (int i = 0; i < NI; i++) acc[r][i] = uint4{0, 0, 0, 0};

    for (int c = 0; c < k; c++) {
      const uint8_t *src = sbase + size_t(imap[c]) * shard_len;
      LinTab lt[GM];
#pragma unroll
      for (int r = 0; r < GM; r++) lt[r] = lintab_load(ctab, r * k + c);
#pragma unroll
      for (int i = 0; i < NI; i++) {
        const int off = i * 1024 + lane16i;
        if (off + 16 <= pli) {
          const uint4 v = *reinterpret_cast<const uint4 *>(src + off);
#pragma unroll
          for (int d = 0; d < 4; d++)
            gfmac4_lin_rows_n<GM, NI>(acc, i, d, (&v.x)[d], lt);
        }
      }
    }
    if (t0 < pli) { /* stage input tail bytes, 4 shards per sweep */
      for (int cb = 0; cb < k; cb += 4) {
        const int c2 = cb + (lane >> 4), j = lane & 15;
        if (c2 < k && t0 + j < pli)
          wtail[c2 * 16 + j] =
              sbase[size_t(imap[c2]) * shard_len + t0 + j];
      }
    }

    uint32_t mismatch = 0;
#pragma unroll
    for (int r = 0; r < GM; r++) {
      if (r < nw) {
        const int col = int((colpack >> (4 * r)) & 0xF);
        uint8_t *fdst =
            dst + (stripe * nw + col) * dst_stride + CRC_LEN;
        uint32_t t = 0;
#pragma unroll
        for (int i = 0; i < NI; i++) {
          const int off = i * 1024 + lane16i;
          if (off + 16 <= pli) {
            uint32_t *dw = reinterpret_cast<uint32_t *>(fdst + off);
            dw[0] = acc[r][i].x; dw[1] = acc[r][i].y;
            dw[2] = acc[r][i].z; dw[3] = acc[r][i].w;
            t = shift4k(t, stab) ^ crc16_reg(acc[r][i], tab);
          }
        }
        uint32_t part = t ? gf2_mulmod_d(op, t) : 0;
        {
          const int p = t0 + lane;
          if (p < pli) {
            uint8_t pv = 0;
            for (int c2 = 0; c2 < k; c2++) {
              const uint8_t b = wtail[c2 * 16 + (p - t0)];
              pv ^= gfmul1_lin(ctab + size_t(r * k + c2) * 32, b);
            }
            fdst[p] = pv;
            part ^= gf2_mulmod_d(x8tab[pli - 1 - p], tab[0][pv]);
          }
        }
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1)
          part ^= __shfl_xor(part, sh, 64);
        if (lane == 0)
          *reinterpret_cast<uint32_t *>(
              dst + (stripe * nw + col) * dst_stride) = ~(it ^ part);
      } else {
        const uint8_t *cshard =
            sbase + size_t(imap[k + (r - nw)]) * shard_len;
        uint32_t d2 = 0;
#pragma unroll
        for (int i = 0; i < NI; i++) {
          const int off = i * 1024 + lane16i;
          if (off + 16 <= pli) {
            const uint4 w = *reinterpret_cast<const uint4 *>(cshard + off);
            d2 |= (w.x ^ acc[r][i].x) | (w.y ^ acc[r][i].y) |
                  (w.z ^ acc[r][i].z) | (w.w ^ acc[r][i].w);
          }
        }
        {
          const int p = t0 + lane;
          if (p < pli) {
            uint8_t pv = 0;
            for (int c2 = 0; c2 < k; c2++) {
              const uint8_t b = wtail[c2 * 16 + (p - t0)];
              pv ^= gfmul1_lin(ctab + size_t(r * k + c2) * 32, b);
            }
            d2 |= uint32_t(pv ^ cshard[p]);
          }
        }
        mismatch |= d2;
      }
    }
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1)
      mismatch |= __shfl_xor(mismatch, sh, 64);
    if (lane == 0 && mismatch) atomicOr(&fail[stripe], 1u);
  }
}

void launch_rs_repair_frame_small(uint8_t *dst, size_t dst_stride,
                                  uint64_t base, uint64_t stripe_stride,
                                  size_t shard_len, int k, int gm, int nw,
                                  const int32_t *imap, const uint8_t *tabs,
                                  uint32_t colpack, uint32_t *fail,
                                  int nstripes, hipStream_t s) {
  const int64_t groups = (int64_t(nstripes) + 3) / 4;
  const int64_t cap = env_grid("GFRS_CRC_GRID", 16384);
  int grid = int(groups < cap ? groups : cap);
  if (grid < 1) grid = 1;
  const int ni = int((shard_len + 1023) / 1024);
  const int lds = 12288 + 64 + 1024 + gm * k * 32;
#define GFRS_RPS_GO(G, I)                                                 \
  hipLaunchKernelGGL((rs_repair_frame_small_k<G, I>), dim3(grid),         \
                     dim3(CRC_BLOCKT), lds, s, dst, dst_stride, base,     \
                     stripe_stride, shard_len, k, imap, tabs, nw,         \
                     colpack, fail, nstripes)
#define GFRS_RPS_NI(G)                                                    \
  switch (ni) {                                                           \
    case 1: GFRS_RPS_GO(G, 1); break;                                     \
    case 2: GFRS_RPS_GO(G, 2); break;                                     \
    case 3: GFRS_RPS_GO(G, 3); break;                                     \
    default: GFRS_RPS_GO(G, 4);                                           \
  }
  switch (gm) {
    case 1: GFRS_RPS_NI(1); break;
    case 2: GFRS_RPS_NI(2); break;
    case 3: GFRS_RPS_NI(3); break;
    default: GFRS_RPS_NI(4);
  }
#undef GFRS_RPS_NI
#undef GFRS_RPS_GO
}

void launch_rs_repair_frame(uint8_t *dst, size_t dst_stride, uint64_t base,
                            uint64_t stripe_stride, size_t shard_len, int k,
                            int gm, int nw, const int32_t *imap,
                            const uint8_t *tabs, uint32_t colpack,
                            uint32_t *fail, int nstripes, hipStream_t s) {
  const int64_t fps = (int64_t(shard_len) + 65531) / 65532;
  const int64_t total = fps * nstripes;
  const int grid = fused_grid(total, fps);
  const int lds = 12288 + EF_RED + 64 + 256 + gm * k * 32;
  /* GFRS_RP_WAVES: 3 or 4 waves/SIMD (0/unset = size policy).  Measured
   * @512x4MiB bad=[2,6]: 3-wave 5.565 ms vs 4-wave 5.649; @256x8MiB
   * 6.457 vs 6.515 (gpurun_out/r3_rpw.log) — same direction as the
   * encode kernel's traffic-exact 3-wave form, so >=1 MiB shards
   * default to 3 waves. */
  static const int waves_env = []() {
    const char *e = getenv("GFRS_RP_WAVES");
    const int v = e ? atoi(e) : 0;
    return (v == 3 || v == 4) ? v : 0;
  }();
  const int waves =
      waves_env ? waves_env : (shard_len >= size_t(1) << 20 ? 3 : 4);
#define GFRS_RP_GO(G, W)                                                    hipLaunchKernelGGL((rs_repair_frame_k<G, W>), dim3(grid),                                    dim3(CRC_BLOCKT), lds, s, dst, dst_stride, base,                          stripe_stride, shard_len, k, imap, tabs, nw,                              colpack, fail, total, fps)
#define GFRS_RP_SEL(G)                                                      do {                                                                        if (waves == 3) GFRS_RP_GO(G, 3);                                         else GFRS_RP_GO(G, 4);                                                  } while (0)
  switch (gm) {
    case 1: GFRS_RP_SEL(1); break;
    case 2: GFRS_RP_SEL(2); break;
    case 3: GFRS_RP_SEL(3); break;
    default: GFRS_RP_SEL(4);
  }
#undef GFRS_RP_SEL
#undef GFRS_RP_GO
}

/* Repair-image queue: rs_repair_frame_k over the work items of one bucket of
 * the repair schedule (gfrs_plan.h).  The math of a frame - the 16 KiB
 * passes, the op-chain register CRC, the LDS-staged tail bytes, the per-row
 * write or compare, the ballot fail flag, the frame header store - is the
 * batch kernel's; what differs is where a frame comes from:
 *  - the grid is capped and block b walks the CONTIGUOUS frame range
 *    [b*per_blk, (b+1)*per_blk) of the bucket.  frame -> work item: one
 *    binary search over the frame prefix sums at the block's first frame,
 *    then a forward walk (every item has >= 1 frame).  All of it depends on
 *    blockIdx and kernel arguments only, so the search, the item and its
 *    descriptor are scalar loads, as in rs_apply_queue_k;
 *  - the tables (ctab) are restaged into LDS, and imap, k, nw and colpack
 *    reloaded, only when the descriptor of the next frame differs from what
 *    is loaded, between two barriers.  The test is block-uniform and no lane
 *    leaves the loop body early, so every lane reaches every barrier;
 *  - every pointer is rebuilt from base + item.off; a block works on one job
 *    at a time, so the fail flag goes to fail[item.job];
 *  - cross-frame prefetch: the batch kernel computes the next frame's unit 0
 *    from the CURRENT imap[0], shard_len and stripe arithmetic.  Here the
 *    next frame may belong to another job or descriptor, so its address and
 *    length come from the NEXT item's own values (its off, shard_len and its
 *    descriptor's imap[0]); `pref` says that vnext holds exactly the loads
 *    the top of the next frame would issue, otherwise the top reloads.  No
 *    load ever leaves the shards of the job it belongs to;
 *  - jobs of at most 4096 bytes run here too, one short frame per block (no
 *    wave-per-stripe packing). */
template <int GM, int WPS = 4>
__global__ __launch_bounds__(CRC_BLOCKT, WPS) void rs_repair_frame_queue_k(
    uint8_t *__restrict__ dst /* disk_dst */, uint64_t base,
    const gfrs_ritem *__restrict__ items,
    const uint64_t *__restrict__ frame_prefix, uint32_t nitems,
    uint64_t total_frames, const RepairDesc *__restrict__ descs,
    uint32_t *__restrict__ fail) {
  constexpr int EF_PASS = 16384;
  constexpr int EF_PASSES = 4;
  constexpr int64_t block_len = 65536;
  constexpr int64_t payload_full = block_len - CRC_LEN;

  const uint64_t per_blk = (total_frames + gridDim.x - 1) / gridDim.x;
  const uint64_t f_lo = uint64_t(blockIdx.x) * per_blk;
  const uint64_t f_hi =
      f_lo + per_blk < total_frames ? f_lo + per_blk : total_frames;
  if (f_lo >= f_hi) return; /* whole block, before any barrier */

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t(*tab)[256] = reinterpret_cast<uint32_t(*)[256]>(smem);
  uint32_t(*stab)[256] = reinterpret_cast<uint32_t(*)[256]>(smem + 8192);
  uint32_t *red = reinterpret_cast<uint32_t *>(smem + 12288);
  uint32_t *x8tab = reinterpret_cast<uint32_t *>(smem + 12288 + EF_RED);
  uint8_t *tailb = smem + 12288 + EF_RED + 64;
  uint8_t *ctab = smem + 12288 + EF_RED + 64 + 256;
  for (int i = threadIdx.x; i < 2048; i += CRC_BLOCKT)
    (&tab[0][0])[i] = (&g_crc_tab4[0][0])[i];
  for (int i = threadIdx.x; i < 1024; i += CRC_BLOCKT)
    (&stab[0][0])[i] = (&g_shift4k[0][0])[i];
  if (threadIdx.x == 0) {
    uint32_t v = 0x80000000u;
    for (int j = 0; j < 16; j++) {
      x8tab[j] = v;
      v = gf2_mulmod_d(v, g_pow8[0]);
    }
  }
  const int64_t lane16 = int64_t(threadIdx.x) * 16;
  const int lane16i = int(threadIdx.x) * 16;
  constexpr uint32_t INV16K = 0x479933FCu;
  const uint32_t op_pA =
      x8n_d(uint64_t(payload_full - (3 * 4096 + lane16 + 16)));
  const uint32_t op_pB = gf2_mulmod_d(op_pA, INV16K);
  const uint32_t op_pC = gf2_mulmod_d(op_pB, INV16K);
  const uint32_t op_pD = gf2_mulmod_d(op_pC, INV16K);
  const uint32_t it_full =
      gf2_mulmod_d(x8n_d(uint64_t(payload_full)), 0xFFFFFFFFu);
  __syncthreads();

  /* largest it with frame_prefix[it] <= f_lo (frame_prefix[0] == 0) */
  uint32_t it = 0;
  for (uint32_t hi = nitems; hi - it > 1;) {
    const uint32_t mid = it + (hi - it) / 2;
    if (frame_prefix[mid] <= f_lo)
      it = mid;
    else
      hi = mid;
  }

  /* imap arrives as a pointer read from the descriptor table: the constant
   * address space keeps its (block-uniform) reads scalar, as they are in
   * rs_repair_frame_k where imap is a kernel argument */
  typedef const __attribute__((address_space(4))) int32_t *IdxList;
  int cur_desc = -1;
  IdxList imap = nullptr;
  int k = 0, nw = 0;
  uint32_t colpack = 0;
  uint4 vnext[4] = {uint4{0, 0, 0, 0}, uint4{0, 0, 0, 0}, uint4{0, 0, 0, 0},
                    uint4{0, 0, 0, 0}};
  bool pref = false; /* vnext = pass 0, unit 0 of the frame about to start */

  for (uint64_t fr = f_lo; fr < f_hi; fr++) {
    while (frame_prefix[it + 1] <= fr) it++; /* it + 1 <= nitems */
    const gfrs_ritem item = items[it];
    const size_t shard_len = item.shard_len;
    const int64_t f = int64_t(fr - frame_prefix[it]);
    if (item.desc != cur_desc) {
      const RepairDesc d = descs[item.desc];
      __syncthreads(); /* all lanes are done with the old tables */
      const uint4 *src =
          reinterpret_cast<const uint4 *>(as_global(uint64_t(d.tabs)));
      for (int i = threadIdx.x; i < GM * d.k * 2; i += CRC_BLOCKT)
        reinterpret_cast<uint4 *>(ctab)[i] = src[i];
      __syncthreads();
      cur_desc = item.desc;
      imap = (IdxList)(uint64_t)d.imap;
      k = d.k;
      nw = d.nw;
      colpack = d.colpack;
    }
    const int64_t p0 = f * payload_full;
    const int64_t payload = i64min(payload_full, int64_t(shard_len) - p0);
    const uint8_t *sbase = as_global(base + item.off);
    /* body of the item's image column 0; column c at + c * img_stride */
    uint8_t *ibody = dst + item.img + 32;

    uint4 acc[GM][4];
    if (!pref) { /* pass 0, unit 0 */
      const int rb0 = int(i64min(int64_t(EF_PASS), payload));
      const uint8_t *src0 = sbase + size_t(imap[0]) * shard_len + p0;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int off = i * 4096 + lane16i;
        vnext[i] = off + 16 <= rb0
                       ? *reinterpret_cast<const uint4 *>(src0 + off)
                       : uint4{0, 0, 0, 0};
      }
    }
    pref = false;
    for (int j = threadIdx.x; j < 64; j += CRC_BLOCKT) red[j] = 0;
    __syncthreads();

    uint32_t mismatch = 0;
    for (int h = 0; h < EF_PASSES; h++) {
      const int64_t r0 = int64_t(h) * EF_PASS;
      const int64_t rbytes = i64min(int64_t(EF_PASS), payload - r0);
      if (rbytes <= 0) break;
#pragma unroll
      for (int r = 0; r < GM; r++)
#pragma unroll
        for (int i = 0; i < 4; i++) acc[r][i] = uint4{0, 0, 0, 0};

      uint32_t op = h == 0   ? op_pA
                    : h == 1 ? op_pB
                    : h == 2 ? op_pC
                             : op_pD;
      if (h == EF_PASSES - 1 && threadIdx.x == 255)
        op = shift4k(op, stab);
      if (payload != payload_full) {
        int np = 0;
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (int64_t(i) * 4096 + lane16 + 16 <= rbytes) np = i + 1;
        const int64_t end =
            np ? r0 + int64_t(np - 1) * 4096 + lane16 + 16 : r0;
        op = x8n_d(uint64_t(payload - end));
      }

      const int rbi = int(rbytes);
      for (int c = 0; c < k; c++) {
        uint4 vcur[4];
#pragma unroll
        for (int i = 0; i < 4; i++) vcur[i] = vnext[i];
        if (c + 1 < k) { /* next input's loads fly over this MAC */
          const uint8_t *nsrc =
              sbase + size_t(imap[c + 1]) * shard_len + p0 + r0;
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const int off = i * 4096 + lane16i;
            vnext[i] = off + 16 <= rbi
                           ? *reinterpret_cast<const uint4 *>(nsrc + off)
                           : uint4{0, 0, 0, 0};
          }
        }
        LinTab lt[GM];
#pragma unroll
        for (int r = 0; r < GM; r++) lt[r] = lintab_load(ctab, r * k + c);
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int off = i * 4096 + lane16i;
          if (off + 16 <= rbi) {
#pragma unroll
            for (int d = 0; d < 4; d++)
              gfmac4_lin_rows<GM>(acc, i, d, (&vcur[i].x)[d], lt);
          }
        }
      }
      { /* prefetch unit 0 of the next pass, or of the next frame */
        int64_t r0n = r0 + EF_PASS;
        int64_t rbn = i64min(int64_t(EF_PASS), payload - r0n);
        const uint8_t *nbase = sbase + size_t(imap[0]) * shard_len + p0 + r0n;
        if (rbn <= 0 && fr + 1 < f_hi) {
          /* the frame after this one, from ITS item: the same job's next
           * frame, or frame 0 of the next item (its own off, shard_len and
           * its descriptor's first input) */
          if (frame_prefix[it + 1] <= fr + 1) {
            const gfrs_ritem nx = items[it + 1];
            const IdxList nmap = (IdxList)(uint64_t)descs[nx.desc].imap;
            rbn = i64min(int64_t(EF_PASS), int64_t(nx.shard_len));
            nbase = as_global(base + nx.off) +
                    size_t(nmap[0]) * size_t(nx.shard_len);
          } else {
            const int64_t p0n = p0 + payload_full;
            rbn = i64min(int64_t(EF_PASS), int64_t(shard_len) - p0n);
            nbase = sbase + size_t(imap[0]) * shard_len + p0n;
          }
          pref = true;
        }
        if (rbn > 0) {
          const int rbni = int(rbn);
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const int off = i * 4096 + lane16i;
            vnext[i] = off + 16 <= rbni
                           ? *reinterpret_cast<const uint4 *>(nbase + off)
                           : uint4{0, 0, 0, 0};
          }
        }
      }
      if (rbytes < EF_PASS) { /* stage input tail bytes: lane (c,j) */
        const int tt0 = (rbi / 16) * 16;
        const int c2 = int(threadIdx.x) >> 4, j = int(threadIdx.x) & 15;
        if (c2 < k && tt0 + j < rbi)
          tailb[c2 * 16 + j] =
              sbase[size_t(imap[c2]) * shard_len + p0 + r0 + tt0 + j];
        __syncthreads();
      }
#pragma unroll
      for (int r = 0; r < GM; r++) {
        if (r < nw) { /* rebuild row: framed image output */
          const int col = int((colpack >> (4 * r)) & 0xF);
          uint8_t *fdst = ibody + size_t(col) * item.img_stride +
                          f * block_len + CRC_LEN + r0;
          uint32_t t = 0;
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const int off = i * 4096 + lane16i;
            if (off + 16 <= rbi) {
              uint32_t *dw = reinterpret_cast<uint32_t *>(fdst + off);
              dw[0] = acc[r][i].x; dw[1] = acc[r][i].y;
              dw[2] = acc[r][i].z; dw[3] = acc[r][i].w;
              t = shift4k(t, stab) ^ crc16_reg(acc[r][i], tab);
            }
          }
          uint32_t part = t ? gf2_mulmod_d(op, t) : 0;
          if (rbytes < EF_PASS) { /* lane-parallel tail (see encode) */
            const int t0 = (rbi / 16) * 16;
            const int p = t0 + int(threadIdx.x);
            if (p < rbi) {
              uint8_t pv = 0;
              for (int c2 = 0; c2 < k; c2++) {
                const uint8_t b2 = tailb[c2 * 16 + (p - t0)];
                pv ^= gfmul1_lin(ctab + size_t(r * k + c2) * 32, b2);
              }
              fdst[p] = pv;
              part ^= gf2_mulmod_d(x8tab[rbi - 1 - p], tab[0][pv]);
            }
          }
#pragma unroll
          for (int sh = 32; sh > 0; sh >>= 1)
            part ^= __shfl_xor(part, sh, 64);
          if ((threadIdx.x & 63) == 0)
            red[(threadIdx.x >> 6) * 16 + r] ^= part;
        } else { /* check row: compare against the surviving parity */
          const uint8_t *cshard =
              sbase + size_t(imap[k + (r - nw)]) * shard_len + p0 + r0;
          uint32_t d = 0;
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const int off = i * 4096 + lane16i;
            if (off + 16 <= rbi) {
              const uint4 w =
                  *reinterpret_cast<const uint4 *>(cshard + off);
              d |= (w.x ^ acc[r][i].x) | (w.y ^ acc[r][i].y) |
                   (w.z ^ acc[r][i].z) | (w.w ^ acc[r][i].w);
            }
          }
          if (rbytes < EF_PASS) {
            const int t0 = (rbi / 16) * 16;
            const int p = t0 + int(threadIdx.x);
            if (p < rbi) {
              uint8_t pv = 0;
              for (int c2 = 0; c2 < k; c2++) {
                const uint8_t b2 = tailb[c2 * 16 + (p - t0)];
                pv ^= gfmul1_lin(ctab + size_t(r * k + c2) * 32, b2);
              }
              d |= uint32_t(pv ^ cshard[p]);
            }
          }
          mismatch |= d;
        }
      }
    }

    /* fail flag + the 4 B LE frame headers of the rebuilt images */
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1)
      mismatch |= __shfl_xor(mismatch, sh, 64);
    __syncthreads();
    {
      const int r = int(threadIdx.x);
      if (r < nw) {
        const uint32_t itv =
            payload == payload_full
                ? it_full
                : gf2_mulmod_d(x8n_d(uint64_t(payload)), 0xFFFFFFFFu);
        const int col = int((colpack >> (4 * r)) & 0xF);
        const uint32_t crc =
            ~(itv ^ red[r] ^ red[16 + r] ^ red[32 + r] ^ red[48 + r]);
        *reinterpret_cast<uint32_t *>(ibody + size_t(col) * item.img_stride +
                                      f * block_len) = crc;
      }
    }
    if ((threadIdx.x & 63) == 0 && mismatch)
      atomicOr(&fail[item.job], 1u);
    __syncthreads();
  }
}

void launch_rs_repair_frame_queue(uint8_t *dst, uint64_t base,
                                  const gfrs_ritem *items,
                                  const uint64_t *frame_prefix,
                                  uint32_t nitems, uint64_t total_frames,
                                  const RepairDesc *descs, int kmax, int gm,
                                  uint32_t *fail, hipStream_t s) {
  if (nitems == 0 || total_frames == 0) return;
  /* the cap of fused_grid, read on every launch: GFRS_CRC_GRID forces the
   * multi-frame walk, the restage and the cross-item prefetch at tiny
   * shapes */
  const uint64_t cap = uint64_t(env_grid("GFRS_CRC_GRID", 16384));
  const int grid = int(total_frames < cap ? total_frames : cap);
  const int lds = 12288 + EF_RED + 64 + 256 + gm * kmax * 32;
  /* the wave policy of launch_rs_repair_frame, on the bucket's mean job:
   * 3 waves/SIMD from about 1 MiB (16 frames) per shard */
  static const int waves_env = []() {
    const char *e = getenv("GFRS_RP_WAVES");
    const int v = e ? atoi(e) : 0;
    return (v == 3 || v == 4) ? v : 0;
  }();
  const int waves =
      waves_env ? waves_env : (total_frames >= uint64_t(16) * nitems ? 3 : 4);
#define GFRS_RQ_GO(G, W)                                                   \
  hipLaunchKernelGGL((rs_repair_frame_queue_k<G, W>), dim3(grid),          \
                     dim3(CRC_BLOCKT), lds, s, dst, base, items,           \
                     frame_prefix, nitems, total_frames, descs, fail)
#define GFRS_RQ_SEL(G)                                                     \
  do {                                                                     \
    if (waves == 3) GFRS_RQ_GO(G, 3);                                      \
    else GFRS_RQ_GO(G, 4);                                                 \
  } while (0)
  switch (gm) {
    case 1: GFRS_RQ_SEL(1); break;
    case 2: GFRS_RQ_SEL(2); break;
    case 3: GFRS_RQ_SEL(3); break;
    default: GFRS_RQ_SEL(4);
  }
#undef GFRS_RQ_SEL
#undef GFRS_RQ_GO
}

/* ---- read queue: verify + rebuild + unframe in one pass ---- */

/* Store the 16-byte piece at frame position x (a multiple of 4) through
 * `rowf`, the address frame position 0 of the row would have, clipped to the
 * frame positions [lo, hi) the segment covers (lo a multiple of 4): the whole
 * dwords inside, nothing outside.  `inside` (block-uniform) says the whole
 * pass lies in [lo, hi).  The last dword of a segment with hi % 4 != 0 is
 * store_clip_tail's. */
GFRS_DEV void store_clip16(uint8_t *rowf, int x, int lo, int hi, bool inside,
                           const uint4 v) {
  uint32_t *dw = reinterpret_cast<uint32_t *>(rowf + x);
  if (inside) {
    dw[0] = v.x; dw[1] = v.y; dw[2] = v.z; dw[3] = v.w;
  } else {
    if (x >= lo && x + 4 <= hi) dw[0] = v.x;
    if (x + 4 >= lo && x + 8 <= hi) dw[1] = v.y;
    if (x + 8 >= lo && x + 12 <= hi) dw[2] = v.z;
    if (x + 12 >= lo && x + 16 <= hi) dw[3] = v.w;
  }
}

/* The partial last dword of the segment (hi % 4 != 0), byte by byte, when it
 * lies in the nv = rbi & ~15 bytes of the pass at r0 that lanes hold as
 * 16-byte pieces v[0..3] (lane l: pass offsets i * 4096 + 16 * l); in the
 * ragged tail behind them it is the byte path's.  The test is block-uniform;
 * one lane stores at most 3 bytes. */
GFRS_DEV void store_clip_tail(uint8_t *rowf, int r0, int nv, int hi,
                              const uint4 (&v)[4]) {
  const int hq = hi & ~3, pr = hq - r0;
  if ((hi & 3) && pr >= 0 && pr < nv &&
      int(threadIdx.x) == ((pr & 4095) >> 4)) {
    /* constant indices only, so that v stays in registers */
    const int sel = pr >> 12 << 2 | (pr & 15) >> 2;
    uint32_t w = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      if (sel == 4 * i) w = v[i].x;
      if (sel == 4 * i + 1) w = v[i].y;
      if (sel == 4 * i + 2) w = v[i].z;
      if (sel == 4 * i + 3) w = v[i].w;
    }
#pragma unroll
    for (int b = 0; b < 3; b++)
      if (b < (hi & 3)) rowf[hq + b] = uint8_t(w >> (8 * b));
  }
}

/* The read direction of the fused frame kernels (the degraded GET): frames
 * in, raw segment out.  The walk is rs_repair_frame_queue_k's - a contiguous
 * frame range per block, one binary search then a forward walk over the
 * prefix sums, block-uniform descriptor restage between two barriers, scalar
 * item loads, every pointer rebuilt from the item - but the prefix sums count
 * the frames an item's segment TOUCHES, and frame f of the walk is frame
 * seg_off / 65532 + f of the shard.  The data flow is inverted: for each
 * 16 KiB pass and each input c of the descriptor a lane
 *   1. takes its four 16-byte pieces of the input's PAYLOAD (image offset
 *      f * 65536 + 4 + pass offset), prefetched under the previous input,
 *   2. Horner-chains them through the register CRC (crc16_reg / shift4k) and
 *      folds by its position operator - the operators of crc32b_verify_reg_k,
 *   3. stores them to the input's own row when the input is a data shard,
 *   4. MACs them into the R accumulators (R > 0),
 * then stores the R rebuilt rows.  Every store is clipped to the segment
 * (store_clip16: dword granular at the head, where seg_off % 4 == 0 keeps
 * raw positions and addresses congruent; store_clip_tail: byte granular at
 * the tail).  The CRC of input c is reduced per wave into red[wave][c];
 * the ragged tail bytes of a frame (12 of a full frame's last pass) go
 * through the (input, byte) lane mapping of the repair kernel's tailb stage
 * and XOR their CRC terms into red[4][c].  At the end of a frame lane c
 * compares input c's CRC with the stored 4-byte LE header and ORs
 * 1 << shard into fail[item.job].
 * Frame f of every shard of a stripe covers the same raw range, so one lane
 * mapping serves all inputs and outputs.  No lane leaves the frame loop
 * early; no load leaves the touched frames of the item's input images; no
 * store leaves the item's declared rows.  There is no cross-frame prefetch:
 * the first input of a frame is loaded at its top. */
constexpr int RD_RED = 5 * 16 * 4; /* red[4 waves + tail][16 inputs] */
constexpr int RD_LDS = 12288 + RD_RED + 64 + 256; /* ctab follows */

template <int R, int WPS>
__global__ __launch_bounds__(CRC_BLOCKT, WPS) void rs_read_frame_queue_k(
    uint8_t *__restrict__ out, uint64_t framed,
    const gfrs_gitem *__restrict__ items,
    const uint64_t *__restrict__ frame_prefix, uint32_t nitems,
    uint64_t total_frames, const ReadDesc *__restrict__ descs,
    uint32_t *__restrict__ fail) {
  constexpr int EF_PASS = 16384;
  constexpr int EF_PASSES = 4;
  constexpr int64_t block_len = 65536;
  constexpr int64_t payload_full = block_len - CRC_LEN;
  constexpr int RR = R > 0 ? R : 1;

  const uint64_t per_blk = (total_frames + gridDim.x - 1) / gridDim.x;
  const uint64_t f_lo = uint64_t(blockIdx.x) * per_blk;
  const uint64_t f_hi =
      f_lo + per_blk < total_frames ? f_lo + per_blk : total_frames;
  if (f_lo >= f_hi) return; /* whole block, before any barrier */

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t(*tab)[256] = reinterpret_cast<uint32_t(*)[256]>(smem);
  uint32_t(*stab)[256] = reinterpret_cast<uint32_t(*)[256]>(smem + 8192);
  uint32_t *red = reinterpret_cast<uint32_t *>(smem + 12288);
  uint32_t *x8tab = reinterpret_cast<uint32_t *>(smem + 12288 + RD_RED);
  uint8_t *tailb = smem + 12288 + RD_RED + 64;
  uint8_t *ctab = smem + RD_LDS;
  for (int i = threadIdx.x; i < 2048; i += CRC_BLOCKT)
    (&tab[0][0])[i] = (&g_crc_tab4[0][0])[i];
  for (int i = threadIdx.x; i < 1024; i += CRC_BLOCKT)
    (&stab[0][0])[i] = (&g_shift4k[0][0])[i];
  if (threadIdx.x == 0) {
    uint32_t v = 0x80000000u;
    for (int j = 0; j < 16; j++) {
      x8tab[j] = v;
      v = gf2_mulmod_d(v, g_pow8[0]);
    }
  }
  const int64_t lane16 = int64_t(threadIdx.x) * 16;
  const int lane16i = int(threadIdx.x) * 16;
  constexpr uint32_t INV16K = 0x479933FCu;
  const uint32_t op_pA =
      x8n_d(uint64_t(payload_full - (3 * 4096 + lane16 + 16)));
  const uint32_t op_pB = gf2_mulmod_d(op_pA, INV16K);
  const uint32_t op_pC = gf2_mulmod_d(op_pB, INV16K);
  const uint32_t op_pD = gf2_mulmod_d(op_pC, INV16K);
  const uint32_t it_full =
      gf2_mulmod_d(x8n_d(uint64_t(payload_full)), 0xFFFFFFFFu);
  __syncthreads();

  /* largest it with frame_prefix[it] <= f_lo (frame_prefix[0] == 0) */
  uint32_t it = 0;
  for (uint32_t hi = nitems; hi - it > 1;) {
    const uint32_t mid = it + (hi - it) / 2;
    if (frame_prefix[mid] <= f_lo)
      it = mid;
    else
      hi = mid;
  }

  typedef const __attribute__((address_space(4))) int32_t *IdxList;
  int cur_desc = -1;
  IdxList imap = nullptr, omap = nullptr;
  int k = 0;
  uint32_t pass = 0;

  for (uint64_t fr = f_lo; fr < f_hi; fr++) {
    while (frame_prefix[it + 1] <= fr) it++; /* it + 1 <= nitems */
    const gfrs_gitem item = items[it];
    if (item.desc != cur_desc) {
      const ReadDesc d = descs[item.desc];
      if (R > 0) {
        __syncthreads(); /* all lanes are done with the old tables */
        const uint4 *src =
            reinterpret_cast<const uint4 *>(as_global(uint64_t(d.tabs)));
        for (int i = threadIdx.x; i < R * d.k * 2; i += CRC_BLOCKT)
          reinterpret_cast<uint4 *>(ctab)[i] = src[i];
        __syncthreads();
      }
      cur_desc = item.desc;
      imap = (IdxList)(uint64_t)d.imap;
      omap = (IdxList)(uint64_t)d.omap;
      k = d.k;
      pass = d.pass_mask;
    }
    /* frame f of the shard: the item's first touched frame + its walk index.
     * Everything below is 32-bit and relative to the frame: payload bytes,
     * and [lo, hi), the frame positions the segment covers (lo % 4 == 0) */
    const int64_t f = int64_t(item.seg_off / uint64_t(payload_full)) +
                      int64_t(fr - frame_prefix[it]);
    const int64_t p0 = f * payload_full;
    const int payload =
        int(i64min(payload_full, int64_t(item.shard_len) - p0));
    const int64_t slo = int64_t(item.seg_off) - p0;
    const int64_t shi = slo + int64_t(item.seg_len);
    const int lo = slo > 0 ? int(slo) : 0;
    const int hi = shi < int64_t(payload) ? int(shi) : payload;
    /* frame f of image 0 (image i at + i * img_stride), and the address
     * frame position 0 of row 0 would have (row i at + i * out_stride); a row
     * is dereferenced inside [lo, hi) only */
    const uint8_t *ibase = as_global(framed + item.img) + f * block_len;
    uint8_t *obase = reinterpret_cast<uint8_t *>(
        uint64_t(out) + item.out + uint64_t(p0) - item.seg_off);

    uint4 vnext[4];
    { /* pass 0, input 0 */
      const int rb0 = payload < EF_PASS ? payload : EF_PASS;
      const uint8_t *src0 =
          ibase + size_t(imap[0]) * item.img_stride + CRC_LEN;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int off = i * 4096 + lane16i;
        vnext[i] = off + 16 <= rb0
                       ? *reinterpret_cast<const uint4 *>(src0 + off)
                       : uint4{0, 0, 0, 0};
      }
    }
    for (int j = threadIdx.x; j < RD_RED / 4; j += CRC_BLOCKT) red[j] = 0;
    __syncthreads();

#pragma unroll 1
    for (int h = 0; h < EF_PASSES; h++) {
      const int r0 = h * EF_PASS;
      const int rbi = payload - r0 < EF_PASS ? payload - r0 : EF_PASS;
      if (rbi <= 0) break; /* block-uniform */
      const int rbn =
          payload - r0 - EF_PASS < EF_PASS ? payload - r0 - EF_PASS : EF_PASS;
      const bool inside = lo <= r0 && r0 + rbi <= hi; /* block-uniform */

      uint4 acc[RR][4];
#pragma unroll
      for (int r = 0; r < RR; r++)
#pragma unroll
        for (int i = 0; i < 4; i++) acc[r][i] = uint4{0, 0, 0, 0};

      uint32_t op = h == 0   ? op_pA
                    : h == 1 ? op_pB
                    : h == 2 ? op_pC
                             : op_pD;
      if (h == EF_PASSES - 1 && threadIdx.x == 255)
        op = shift4k(op, stab); /* lane 255's last pass has 3 pieces */
      if (payload != int(payload_full)) {
        int np = 0;
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (i * 4096 + lane16i + 16 <= rbi) np = i + 1;
        const int end = np ? r0 + (np - 1) * 4096 + lane16i + 16 : r0;
        op = x8n_d(uint64_t(payload - end));
      }

      for (int c = 0; c < k; c++) {
        uint4 vcur[4];
#pragma unroll
        for (int i = 0; i < 4; i++) vcur[i] = vnext[i];
        { /* the next input's loads, or the next pass's first input's, fly
             over this input's CRC and MAC */
          const bool more = c + 1 < k;
          const int nb = more ? rbi : rbn;
          const uint8_t *nsrc =
              ibase + size_t(imap[more ? c + 1 : 0]) * item.img_stride +
              CRC_LEN + r0 + (more ? 0 : EF_PASS);
          if (nb > 0) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
              const int off = i * 4096 + lane16i;
              vnext[i] = off + 16 <= nb
                             ? *reinterpret_cast<const uint4 *>(nsrc + off)
                             : uint4{0, 0, 0, 0};
            }
          }
        }
        uint32_t t = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int off = i * 4096 + lane16i;
          if (off + 16 <= rbi) t = shift4k(t, stab) ^ crc16_reg(vcur[i], tab);
        }
        uint32_t part = t ? gf2_mulmod_d(op, t) : 0;
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) part ^= __shfl_xor(part, sh, 64);
        if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * 16 + c] ^= part;

        if ((pass >> c) & 1) { /* a surviving data shard: its own row */
          uint8_t *rowf = obase + size_t(imap[c]) * item.out_stride;
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const int off = i * 4096 + lane16i;
            if (off + 16 <= rbi)
              store_clip16(rowf, r0 + off, lo, hi, inside, vcur[i]);
          }
          if (!inside) store_clip_tail(rowf, r0, rbi & ~15, hi, vcur);
        }
        if (R > 0) {
          LinTab lt[RR];
#pragma unroll
          for (int r = 0; r < RR; r++) lt[r] = lintab_load(ctab, r * k + c);
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const int off = i * 4096 + lane16i;
            if (off + 16 <= rbi) {
#pragma unroll
              for (int d = 0; d < 4; d++)
                gfmac4_lin_rows<RR>(acc, i, d, (&vcur[i].x)[d], lt);
            }
          }
        }
      }
      if (R > 0) { /* the rebuilt rows */
#pragma unroll
        for (int r = 0; r < RR; r++) {
          uint8_t *rowf = obase + size_t(omap[r]) * item.out_stride;
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const int off = i * 4096 + lane16i;
            if (off + 16 <= rbi)
              store_clip16(rowf, r0 + off, lo, hi, inside, acc[r][i]);
          }
          if (!inside) store_clip_tail(rowf, r0, rbi & ~15, hi, acc[r]);
        }
      }
      if (rbi & 15) { /* ragged tail of the frame: lane (input c2, byte j) */
        const int tt0 = rbi & ~15;
        const int c2 = int(threadIdx.x) >> 4, j = int(threadIdx.x) & 15;
        if (c2 < k && tt0 + j < rbi) {
          const int sh = imap[c2];
          const uint8_t x =
              ibase[size_t(sh) * item.img_stride + CRC_LEN + r0 + tt0 + j];
          tailb[c2 * 16 + j] = x;
          atomicXor(&red[64 + c2],
                    gf2_mulmod_d(x8tab[rbi - 1 - (tt0 + j)], tab[0][x]));
          const int q = r0 + tt0 + j;
          if (((pass >> c2) & 1) && q >= lo && q < hi)
            obase[size_t(sh) * item.out_stride + q] = x;
        }
        if (R > 0) {
          __syncthreads(); /* block-uniform: rbi is */
          const int p = tt0 + int(threadIdx.x);
          const int q = r0 + p;
          if (p < rbi && q >= lo && q < hi) {
#pragma unroll
            for (int r = 0; r < RR; r++) {
              uint8_t pv = 0;
              for (int c3 = 0; c3 < k; c3++)
                pv ^= gfmul1_lin(ctab + size_t(r * k + c3) * 32,
                                 tailb[c3 * 16 + (p - tt0)]);
              obase[size_t(omap[r]) * item.out_stride + q] = pv;
            }
          }
        }
      }
    }

    __syncthreads();
    if (int(threadIdx.x) < k) { /* lane c: input c's CRC against its header */
      const int c = int(threadIdx.x);
      const int sh = imap[c];
      const uint32_t itv =
          payload == int(payload_full)
              ? it_full
              : gf2_mulmod_d(x8n_d(uint64_t(payload)), 0xFFFFFFFFu);
      const uint32_t crc = ~(itv ^ red[c] ^ red[16 + c] ^ red[32 + c] ^
                             red[48 + c] ^ red[64 + c]);
      const uint8_t *hp = ibase + size_t(sh) * item.img_stride;
      const uint32_t want = uint32_t(hp[0]) | (uint32_t(hp[1]) << 8) |
                            (uint32_t(hp[2]) << 16) | (uint32_t(hp[3]) << 24);
      if (want != crc) atomicOr(&fail[item.job], 1u << sh);
    }
    __syncthreads();
  }
}

void launch_rs_read_frame_queue(uint8_t *out, uint64_t framed,
                                const gfrs_gitem *items,
                                const uint64_t *frame_prefix, uint32_t nitems,
                                uint64_t total_frames, const ReadDesc *descs,
                                int kmax, int r, uint32_t *fail,
                                hipStream_t s) {
  if (nitems == 0 || total_frames == 0) return;
  /* the cap of the other frame queues, read on every launch: GFRS_CRC_GRID
   * forces the multi-frame walk and the restage at tiny shapes */
  const uint64_t cap = uint64_t(env_grid("GFRS_CRC_GRID", 16384));
  const int grid = int(total_frames < cap ? total_frames : cap);
  const int lds = RD_LDS + r * kmax * 32;
  /* waves per SIMD: 4 for R = 0; 3 for R >= 1 - measured for R = 1 (1 % ahead
   * of 4 on 128 x 4 MiB), and the only build without spills for R >= 2
   * (DESIGN.md, section 15).  GFRS_RD_WAVES = 3 or 4 overrides it; like
   * GFRS_CRC_GRID it is read on every launch, so a test can run both builds
   * of every R. */
  const char *we = getenv("GFRS_RD_WAVES");
  const int wv = we ? atoi(we) : 0;
#define GFRS_RD_GO(G, W)                                                   \
  hipLaunchKernelGGL((rs_read_frame_queue_k<G, W>), dim3(grid),            \
                     dim3(CRC_BLOCKT), lds, s, out, framed, items,         \
                     frame_prefix, nitems, total_frames, descs, fail)
#define GFRS_RD_SEL(G, DFLT)                                               \
  do {                                                                     \
    if ((wv == 3 || wv == 4 ? wv : DFLT) == 3) GFRS_RD_GO(G, 3);           \
    else GFRS_RD_GO(G, 4);                                                 \
  } while (0)
  switch (r) {
    case 0: GFRS_RD_SEL(0, 4); break;
    case 1: GFRS_RD_SEL(1, 3); break;
    case 2: GFRS_RD_SEL(2, 3); break;
    case 3: GFRS_RD_SEL(3, 3); break;
    default: GFRS_RD_SEL(4, 3);
  }
#undef GFRS_RD_SEL
#undef GFRS_RD_GO
}

/* Small-shard fused encode+frame: one 64-lane WAVE per stripe, no LDS
 * staging, no barriers (everything wave-local).  Shard <= 4096 B is one
 * short crc32block frame; lane w owns pieces {i*1024 + 16w : i < NI}
 * (64 lanes x 16 B = 1 KiB per subtile) Horner-chained by the constant
 * x^(8*1024) byte-sliced tables.  Four independent waves per block.
 * Covers the reference's 2 KiB MinShardSize PUT shapes in one launch. */
template <int GM, int NI, int WPS = 4>
__global__ __launch_bounds__(CRC_BLOCKT, WPS) void rs_encode_frame_small_k(
    uint8_t *__restrict__ dst, size_t dst_stride, uint64_t base,
    uint64_t stripe_stride, size_t shard_len, int k,
    const uint8_t *__restrict__ tabs /* [GM*k][32] */, int64_t nstripes) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t(*tab)[256] = reinterpret_cast<uint32_t(*)[256]>(smem);
  uint32_t(*stab)[256] = reinterpret_cast<uint32_t(*)[256]>(smem + 8192);
  uint32_t *x8tab = reinterpret_cast<uint32_t *>(smem + 12288);
  uint8_t *tailb = smem + 12288 + 64; /* per-wave 16x16 tail bytes */
  uint8_t *ctab = smem + 12288 + 64 + 4 * 256;
  for (int i = threadIdx.x; i < 2048; i += CRC_BLOCKT)
    (&tab[0][0])[i] = (&g_crc_tab4[0][0])[i];
  for (int i = threadIdx.x; i < 1024; i += CRC_BLOCKT)
    (&stab[0][0])[i] = (&g_shift1k[0][0])[i];
  for (int i = threadIdx.x; i < GM * k * 2; i += CRC_BLOCKT)
    reinterpret_cast<uint4 *>(ctab)[i] =
        reinterpret_cast<const uint4 *>(tabs)[i];
  if (threadIdx.x == 0) {
    uint32_t v = 0x80000000u;
    for (int j = 0; j < 16; j++) {
      x8tab[j] = v;
      v = gf2_mulmod_d(v, g_pow8[0]);
    }
  }
  __syncthreads();

  const int wv = int(threadIdx.x) >> 6, lane = int(threadIdx.x) & 63;
  const int lane16i = lane * 16;
  uint8_t *wtail = tailb + wv * 256;
  const int64_t payload = int64_t(shard_len);
  const int pli = int(payload);
  /* lane's fold operator: suffix after its LAST present piece */
  int np = 0;
#pragma unroll
  for (int i = 0; i < NI; i++)
    if (i * 1024 + lane16i + 16 <= pli) np = i + 1;
  const uint32_t op =
      np ? x8n_d(uint64_t(pli - ((np - 1) * 1024 + lane16i + 16))) : 0;
  const uint32_t it = gf2_mulmod_d(x8n_d(uint64_t(payload)), 0xFFFFFFFFu);
  const int t0 = (pli / 16) * 16;

  for (int64_t stripe = int64_t(blockIdx.x) * 4 + wv; stripe < nstripes;
       stripe += int64_t(gridDim.x) * 4) {
    const uint8_t *sbase = as_global(base + stripe * stripe_stride);
    uint4 acc[GM][NI];
#pragma unroll
    for (int r = 0; r < GM; r++)
#pragma unroll
      for (int i = 0; i < NI; i++) acc[r][i] = uint4{0, 0, 0, 0};

    for (int c = 0; c < k; c++) {
      const uint8_t *src = sbase + size_t(c) * shard_len;
      uint8_t *fdst =
          dst + (stripe * (k + GM) + c) * dst_stride + CRC_LEN;
      uint32_t t = 0;
      LinTab lt[GM];
#pragma unroll
      for (int r = 0; r < GM; r++) lt[r] = lintab_load(ctab, r * k + c);
#pragma unroll
      for (int i = 0; i < NI; i++) {
        const int off = i * 1024 + lane16i;
        if (off + 16 <= pli) {
          const uint4 v = *reinterpret_cast<const uint4 *>(src + off);
#pragma unroll
          for (int d = 0; d < 4; d++)
            gfmac4_lin_rows_n<GM, NI>(acc, i, d, (&v.x)[d], lt);
          *reinterpret_cast<uint4 *>(fdst + off) = v;
          t = shift4k(t, stab) ^ crc16_reg(v, tab); /* stab = x^(8*1024) */
        }
      }
      uint32_t part = t ? gf2_mulmod_d(op, t) : 0;
      { /* tail bytes, one per lane; stage for the parity tails */
        const int p = t0 + lane;
        if (p < pli) {
          const uint8_t x = src[p];
          fdst[p] = x;
          wtail[c * 16 + (p - t0)] = x;
          part ^= gf2_mulmod_d(x8tab[pli - 1 - p], tab[0][x]);
        }
      }
#pragma unroll
      for (int sh = 32; sh > 0; sh >>= 1)
        part ^= __shfl_xor(part, sh, 64);
      if (lane == 0)
        *reinterpret_cast<uint32_t *>(
            dst + (stripe * (k + GM) + c) * dst_stride) = ~(it ^ part);
    }
#pragma unroll
    for (int r = 0; r < GM; r++) {
      uint8_t *fdst =
          dst + (stripe * (k + GM) + k + r) * dst_stride + CRC_LEN;
      uint32_t t = 0;
#pragma unroll
      for (int i = 0; i < NI; i++) {
        const int off = i * 1024 + lane16i;
        if (off + 16 <= pli) {
          *reinterpret_cast<uint4 *>(fdst + off) = acc[r][i];
          t = shift4k(t, stab) ^ crc16_reg(acc[r][i], tab);
        }
      }
      uint32_t part = t ? gf2_mulmod_d(op, t) : 0;
      {
        const int p = t0 + lane;
        if (p < pli) { /* same-wave LDS visibility: no barrier needed */
          uint8_t pv = 0;
          for (int c2 = 0; c2 < k; c2++) {
            const uint8_t b = wtail[c2 * 16 + (p - t0)];
            pv ^= gfmul1_lin(ctab + size_t(r * k + c2) * 32, b);
          }
          fdst[p] = pv;
          part ^= gf2_mulmod_d(x8tab[pli - 1 - p], tab[0][pv]);
        }
      }
#pragma unroll
      for (int sh = 32; sh > 0; sh >>= 1)
        part ^= __shfl_xor(part, sh, 64);
      if (lane == 0)
        *reinterpret_cast<uint32_t *>(
            dst + (stripe * (k + GM) + k + r) * dst_stride) = ~(it ^ part);
    }
  }
}

void launch_rs_encode_frame_small(uint8_t *dst, size_t dst_stride,
                                  uint64_t base, uint64_t stripe_stride,
                                  size_t shard_len, int k, int m,
                                  const uint8_t *tabs, int nstripes,
                                  hipStream_t s) {
  const int64_t groups = (int64_t(nstripes) + 3) / 4;
  const int64_t cap = env_grid("GFRS_CRC_GRID", 16384);
  int grid = int(groups < cap ? groups : cap);
  if (grid < 1) grid = 1;
  const int ni = int((shard_len + 1023) / 1024);
  const int lds = 12288 + 64 + 1024 + m * k * 32;
  const uint8_t *ltabs = tabs; /* linear A|B|C layout */
#define GFRS_SM_GO(G, I)                                                  \
  hipLaunchKernelGGL((rs_encode_frame_small_k<G, I>), dim3(grid),         \
                     dim3(CRC_BLOCKT), lds, s, dst, dst_stride, base,     \
                     stripe_stride, shard_len, k, ltabs, nstripes)
#define GFRS_SM_NI(G)                                                     \
  switch (ni) {                                                           \
    case 1: GFRS_SM_GO(G, 1); break;                                      \
    case 2: GFRS_SM_GO(G, 2); break;                                      \
    case 3: GFRS_SM_GO(G, 3); break;                                      \
    default: GFRS_SM_GO(G, 4);                                            \
  }
/* 4-8 KiB shards (the old fused-kernel gap: a 256-lane workgroup gets
 * only ~5 KiB of frame): extend the wave-per-stripe form to NI<=8 for
 * gm<=3 (acc registers stay within the 4-wave budget) */
/* NI >= 6 instantiates at 3 waves/SIMD: the 4-wave register budget
 * (128) spills 6-63 VGPRs for GM=3 accumulators at those widths */
#define GFRS_SM_GO3(G, I)                                                 \
  hipLaunchKernelGGL((rs_encode_frame_small_k<G, I, 3>), dim3(grid),      \
                     dim3(CRC_BLOCKT), lds, s, dst, dst_stride, base,     \
                     stripe_stride, shard_len, k, ltabs, nstripes)
#define GFRS_SM_NI8(G)                                                    \
  switch (ni) {                                                           \
    case 1: GFRS_SM_GO(G, 1); break;                                      \
    case 2: GFRS_SM_GO(G, 2); break;                                      \
    case 3: GFRS_SM_GO(G, 3); break;                                      \
    case 4: GFRS_SM_GO(G, 4); break;                                      \
    case 5: GFRS_SM_GO(G, 5); break;                                      \
    case 6: GFRS_SM_GO3(G, 6); break;                                     \
    case 7: GFRS_SM_GO3(G, 7); break;                                     \
    default: GFRS_SM_GO3(G, 8);                                           \
  }
  switch (m) {
    case 1: GFRS_SM_NI8(1); break;
    case 2: GFRS_SM_NI8(2); break;
    case 3: GFRS_SM_NI8(3); break;
    default: GFRS_SM_NI(4);
  }
#undef GFRS_SM_NI8
#undef GFRS_SM_GO3
#undef GFRS_SM_NI
#undef GFRS_SM_GO
}

/* auto policy for eligible >= 1 MiB launches: the aligned kernel (79)
 * instead of the register-CRC pipeline (76) - 29.0 vs 30.9 ms on the
 * headline shape, profiles/r03_aligned_frame.txt */
constexpr bool kAlAuto = true;

void launch_rs_encode_frame(uint8_t *dst, size_t dst_stride, uint64_t base,
                            uint64_t stripe_stride, size_t shard_len, int k,
                            int m, const uint8_t *tabs, int nstripes,
                            hipStream_t s) {
  const int64_t fps = (int64_t(shard_len) + 65531) / 65532;
  const int64_t total = fps * nstripes;
  const int grid = fused_grid(total, fps);
  const uint8_t *ltabs = tabs; /* linear A|B|C layout (DevPlan::upload) */
  /* tiny-last-frame fold (reg_k family only): a trailing frame with
   * <= 64 payload bytes is emitted by the previous frame's workgroup */
  const int64_t tiny0 =
      fps >= 2 ? int64_t(shard_len) - (fps - 1) * 65532 : int64_t(0);
  const int tinyi = (tiny0 > 0 && tiny0 <= 64) ? int(tiny0) : 0;
  const int64_t fps2 = tinyi ? fps - 1 : fps;
  const int64_t total2 = fps2 * nstripes;
  const int grid2 = tinyi ? fused_grid(total2, fps2) : grid;
  /* occupancy variant: GFRS_EF = NBUF*10 + waves-per-SIMD bound (16 KiB
   * pass), or a 3-digit NBUF*100 + WPS*10 + NI form for the 8 KiB-pass
   * (NI=2) geometry.  Measured @256 stripes RS(6+3): 14 -> 13.7 ms
   * (single 20 KB stage, 4 blocks/CU) beats 23 (15.3), 13 (15.4),
   * 24 (16.5); NI=2 variants (142/152/162) target 5-6 blocks/CU. */
  static const int var_env = []() {
    const char *e = getenv("GFRS_EF");
    const int v = e ? atoi(e) : -1; /* -1 = auto by shard size */
    switch (v) {
      case 13: case 14: case 23: case 24:
      case 72: case 73:
      case 74: case 75: case 76: case 77: case 78: case 79:
      case 86: case 87: case 96: case 97:
      case 103: case 104: case 113: case 114:
      case 142: case 152: case 162: return v;
      default: return -1;
    }
  }();
  /* auto policy (measured r02): >= 1 MiB shards run the 3-wave
   * register-CRC pipeline (76) whose PMC traffic is algorithmic-exact at
   * the HBM-bound operating point - or, where the layout is 16-B aligned
   * throughout, its aligned sibling (79); smaller shards run the 4-wave
   * nontemporal form (87), whose extra latency hiding is worth more than
   * its ~10% L2-thrash traffic there (64 KiB: 1010 vs 910 GiB/s) */
  const int var_old = shard_len >= (size_t(1) << 20) ? 76 : 87;
  /* 79 = aligned destination-space kernel (rs_encode_frame_al_k, 3 waves,
   * plain stores).  Eligible only when every address the kernel forms is a
   * multiple of 16; any other launch goes where it went before. */
  const bool al_ok = ((uint64_t(reinterpret_cast<uintptr_t>(dst)) |
                       uint64_t(dst_stride) | base | stripe_stride |
                       uint64_t(shard_len)) & 15) == 0;
  const int var = var_env == 79 ? (al_ok ? 79 : var_old)
                  : var_env >= 0 ? var_env
                  : (kAlAuto && al_ok && var_old == 76) ? 79
                                                        : var_old;
  if (var == 79) {
    const int lds =
        AL_LDS_FIXED + (k + (m < 4 ? m : 4) + 1) * 1024 + m * k * 32;
#define GFRS_AL_GO(G, SK, C, R)                                           \
  hipLaunchKernelGGL((rs_encode_frame_al_k<G, 3, SK, 0, C, R>),           \
                     dim3(grid2), dim3(CRC_BLOCKT), lds, s, dst,          \
                     dst_stride, base, stripe_stride, shard_len, k, ltabs, \
                     total2, fps2, tinyi)
    /* diagnostics (GM=3 only): GFRS_EF_ABL=4 = memory skeleton (loads,
     * rotation, stores; MAC and CRC compiled out), GFRS_EF_C0=1 = chunk 0
     * held in LDS and written as one aligned uint4 in the epilogue,
     * GFRS_EF_CRC16=1 = full frames keep the 16+4-gather piece form
     * (crc16_reg, operator without the 4 bytes) for a same-build A/B */
    static const int al_crc16 = []() {
      const char *e = getenv("GFRS_EF_CRC16");
      return e ? atoi(e) : 0;
    }();
    static const int al_abl = []() {
      const char *e = getenv("GFRS_EF_ABL");
      return e ? atoi(e) : 0;
    }();
    static const int al_c0 = []() {
      const char *e = getenv("GFRS_EF_C0");
      return e ? atoi(e) : 0;
    }();
    if (m == 3 && var_env == 79 && al_abl == 4) { GFRS_AL_GO(3, 1, 0, 0); return; }
    if (m == 3 && var_env == 79 && al_c0 == 1) { GFRS_AL_GO(3, 0, 1, 0); return; }
    if (m == 3 && var_env == 79 && al_crc16 == 1) { GFRS_AL_GO(3, 0, 0, 1); return; }
    switch (m) {
      case 1: GFRS_AL_GO(1, 0, 0, 0); break;
      case 2: GFRS_AL_GO(2, 0, 0, 0); break;
      case 3: GFRS_AL_GO(3, 0, 0, 0); break;
      default: GFRS_AL_GO(4, 0, 0, 0);
    }
#undef GFRS_AL_GO
    return;
  }
  /* 1xy = dual-aligned 32-B-piece rotation kernel: 103/104 plain stores
   * @3/4 waves, 113/114 nontemporal @3/4 waves */
  if (var == 103 || var == 104 || var == 113 || var == 114) {
    const int lds = 12288 + EF_RED + 128 + 512 + m * k * 32;
#define GFRS_ROT_GO(G, W, S)                                                hipLaunchKernelGGL((rs_encode_frame_rot_k<G, W, S>), dim3(grid),                             dim3(CRC_BLOCKT), lds, s, dst, dst_stride, base,                          stripe_stride, shard_len, k, ltabs, total, fps)
#define GFRS_ROT_SW(W, S)                                                   switch (m) {                                                                case 1: GFRS_ROT_GO(1, W, S); break;                                      case 2: GFRS_ROT_GO(2, W, S); break;                                      case 3: GFRS_ROT_GO(3, W, S); break;                                      default: GFRS_ROT_GO(4, W, S);                                          }
    if (var == 103) { GFRS_ROT_SW(3, 0) }
    else if (var == 104) { GFRS_ROT_SW(4, 0) }
    else if (var == 113) { GFRS_ROT_SW(3, 1) }
    else { GFRS_ROT_SW(4, 1) }
#undef GFRS_ROT_SW
#undef GFRS_ROT_GO
    return;
  }
  /* 72/73 = low-occupancy forms: 2 blocks/CU (512 resident WGs chip-wide,
   * halving the number of concurrently-touched DRAM streams) with deep
   * (72) or single (73) load lookahead */
  if (var == 72 || var == 73) {
    const int lds = 12288 + EF_RED + 64 + 256 + 1024 + m * k * 32;
#define GFRS_LO_GO(G, P)                                                    hipLaunchKernelGGL((rs_encode_frame_reg_k<G, 2, 0, 0, P>),                                   dim3(grid2), dim3(CRC_BLOCKT), lds, s, dst,                                dst_stride, base, stripe_stride, shard_len, k,                            ltabs, total2, fps2, tinyi)
#define GFRS_LO_SW(P)                                                       switch (m) {                                                                case 1: GFRS_LO_GO(1, P); break;                                          case 2: GFRS_LO_GO(2, P); break;                                          case 3: GFRS_LO_GO(3, P); break;                                          default: GFRS_LO_GO(4, P);                                              }
    if (var == 72) { GFRS_LO_SW(2) } else { GFRS_LO_SW(1) }
#undef GFRS_LO_SW
#undef GFRS_LO_GO
    return;
  }
  /* 8x/9x = store-policy variants of the lookahead pipeline:
   * 86/87 nontemporal @3/4 waves, 96/97 sc1 write-through @3/4 waves */
  if (var == 86 || var == 87 || var == 96 || var == 97) {
    const int lds = 12288 + EF_RED + 64 + 256 + 1024 + m * k * 32;
#define GFRS_STP_GO(G, W, S)                                                hipLaunchKernelGGL((rs_encode_frame_reg_k<G, W, 0, 0, 1, S>),                                dim3(grid2), dim3(CRC_BLOCKT), lds, s, dst,                                dst_stride, base, stripe_stride, shard_len, k,                            ltabs, total2, fps2, tinyi)
#define GFRS_STP_SW(W, S)                                                   switch (m) {                                                                case 1: GFRS_STP_GO(1, W, S); break;                                      case 2: GFRS_STP_GO(2, W, S); break;                                      case 3: GFRS_STP_GO(3, W, S); break;                                      default: GFRS_STP_GO(4, W, S);                                          }
    if (var == 86) { GFRS_STP_SW(3, 1) }
    else if (var == 87) { GFRS_STP_SW(4, 1) }
    else if (var == 96) { GFRS_STP_SW(3, 2) }
    else { GFRS_STP_SW(4, 2) }
#undef GFRS_STP_SW
#undef GFRS_STP_GO
    return;
  }
  /* frame->block mapping experiment on the 4-wave lookahead pipeline
   * (GFRS_EF=77 + GFRS_EF_MAP=1/2, GM=3 instantiations only) */
  if (var == 77 && m == 3) {
    static const int map77 = []() {
      const char *e = getenv("GFRS_EF_MAP");
      return e ? atoi(e) : 0;
    }();
    if (map77 == 1 || map77 == 2) {
      const int lds = 12288 + EF_RED + 64 + 256 + 1024 + m * k * 32;
      if (map77 == 1)
        hipLaunchKernelGGL((rs_encode_frame_reg_k<3, 4, 1, 0, 1>),
                           dim3(grid2), dim3(CRC_BLOCKT), lds, s, dst,
                           dst_stride, base, stripe_stride, shard_len, k,
                           ltabs, total2, fps2, tinyi);
      else
        hipLaunchKernelGGL((rs_encode_frame_reg_k<3, 4, 2, 0, 1>),
                           dim3(grid2), dim3(CRC_BLOCKT), lds, s, dst,
                           dst_stride, base, stripe_stride, shard_len, k,
                           ltabs, total2, fps2, tinyi);
      return;
    }
  }
  /* 7x = register-CRC kernel (no stage): crc tabs + shift tabs + red */
  if (var == 78) { /* two-unit-deep lookahead at 3 waves/SIMD */
    const int lds = 12288 + EF_RED + 64 + 256 + 1024 + m * k * 32;
    switch (m) {
      case 1: hipLaunchKernelGGL((rs_encode_frame_reg_k<1, 3, 0, 0, 2>),
          dim3(grid2), dim3(CRC_BLOCKT), lds, s, dst, dst_stride, base,
          stripe_stride, shard_len, k, ltabs, total2, fps2, tinyi); break;
      case 2: hipLaunchKernelGGL((rs_encode_frame_reg_k<2, 3, 0, 0, 2>),
          dim3(grid2), dim3(CRC_BLOCKT), lds, s, dst, dst_stride, base,
          stripe_stride, shard_len, k, ltabs, total2, fps2, tinyi); break;
      case 3: hipLaunchKernelGGL((rs_encode_frame_reg_k<3, 3, 0, 0, 2>),
          dim3(grid2), dim3(CRC_BLOCKT), lds, s, dst, dst_stride, base,
          stripe_stride, shard_len, k, ltabs, total2, fps2, tinyi); break;
      default: hipLaunchKernelGGL((rs_encode_frame_reg_k<4, 3, 0, 0, 2>),
          dim3(grid2), dim3(CRC_BLOCKT), lds, s, dst, dst_stride, base,
          stripe_stride, shard_len, k, ltabs, total2, fps2, tinyi);
    }
    return;
  }
  if (var == 77) { /* lookahead pipeline squeezed to 4 waves/SIMD */
    const int lds = 12288 + EF_RED + 64 + 256 + 1024 + m * k * 32;
    switch (m) {
      case 1: hipLaunchKernelGGL((rs_encode_frame_reg_k<1, 4, 0, 0, 1>),
          dim3(grid2), dim3(CRC_BLOCKT), lds, s, dst, dst_stride, base,
          stripe_stride, shard_len, k, ltabs, total2, fps2, tinyi); break;
      case 2: hipLaunchKernelGGL((rs_encode_frame_reg_k<2, 4, 0, 0, 1>),
          dim3(grid2), dim3(CRC_BLOCKT), lds, s, dst, dst_stride, base,
          stripe_stride, shard_len, k, ltabs, total2, fps2, tinyi); break;
      case 3: hipLaunchKernelGGL((rs_encode_frame_reg_k<3, 4, 0, 0, 1>),
          dim3(grid2), dim3(CRC_BLOCKT), lds, s, dst, dst_stride, base,
          stripe_stride, shard_len, k, ltabs, total2, fps2, tinyi); break;
      default: hipLaunchKernelGGL((rs_encode_frame_reg_k<4, 4, 0, 0, 1>),
          dim3(grid2), dim3(CRC_BLOCKT), lds, s, dst, dst_stride, base,
          stripe_stride, shard_len, k, ltabs, total2, fps2, tinyi);
    }
    return;
  }
  if (var == 76) { /* one-unit-lookahead pipeline at 3 waves/SIMD */
    const int lds = 12288 + EF_RED + 64 + 256 + 1024 + m * k * 32;
    switch (m) {
      case 1: hipLaunchKernelGGL((rs_encode_frame_reg_k<1, 3, 0, 0, 1>),
          dim3(grid2), dim3(CRC_BLOCKT), lds, s, dst, dst_stride, base,
          stripe_stride, shard_len, k, ltabs, total2, fps2, tinyi); break;
      case 2: hipLaunchKernelGGL((rs_encode_frame_reg_k<2, 3, 0, 0, 1>),
          dim3(grid2), dim3(CRC_BLOCKT), lds, s, dst, dst_stride, base,
          stripe_stride, shard_len, k, ltabs, total2, fps2, tinyi); break;
      case 3: hipLaunchKernelGGL((rs_encode_frame_reg_k<3, 3, 0, 0, 1>),
          dim3(grid2), dim3(CRC_BLOCKT), lds, s, dst, dst_stride, base,
          stripe_stride, shard_len, k, ltabs, total2, fps2, tinyi); break;
      default: hipLaunchKernelGGL((rs_encode_frame_reg_k<4, 3, 0, 0, 1>),
          dim3(grid2), dim3(CRC_BLOCKT), lds, s, dst, dst_stride, base,
          stripe_stride, shard_len, k, ltabs, total2, fps2, tinyi);
    }
    return;
  }
  if (var == 74 || var == 75) {
    const int lds = 12288 + EF_RED + 64 + 256 + 1024 + m * k * 32;
#define GFRS_EFR_GO(G, W, P) hipLaunchKernelGGL((rs_encode_frame_reg_k<G, W, P>), dim3(grid2), dim3(CRC_BLOCKT), lds, s, dst, dst_stride, base, stripe_stride, shard_len, k, ltabs, total2, fps2, tinyi)
#define GFRS_EFR_SW(W, P) switch (m) { case 1: GFRS_EFR_GO(1, W, P); break; case 2: GFRS_EFR_GO(2, W, P); break; case 3: GFRS_EFR_GO(3, W, P); break; default: GFRS_EFR_GO(4, W, P); }
    static const int map = []() {
      const char *e = getenv("GFRS_EF_MAP");
      const int v = e ? atoi(e) : 0;
      return (v >= 0 && v <= 2) ? v : 0;
    }();
    static const int rabl = []() {
      const char *e = getenv("GFRS_EF_ABL");
      const int v = e ? atoi(e) : 0;
      return (v >= 4 && v <= 7) ? v : 0;
    }();
    if (rabl >= 5 && var == 76 && m == 3) { /* phase diagnostics */
      const int lds5 = 12288 + EF_RED + 64 + 256 + 1024 + m * k * 32;
      if (rabl == 5) { hipLaunchKernelGGL((rs_encode_frame_reg_k<3, 3, 0, 2, 1>),
          dim3(grid2), dim3(CRC_BLOCKT), lds5, s, dst, dst_stride, base,
          stripe_stride, shard_len, k, ltabs, total2, fps2, tinyi); return; }
      if (rabl == 6) { hipLaunchKernelGGL((rs_encode_frame_reg_k<3, 3, 0, 3, 1>),
          dim3(grid2), dim3(CRC_BLOCKT), lds5, s, dst, dst_stride, base,
          stripe_stride, shard_len, k, ltabs, total2, fps2, tinyi); return; }
      if (rabl == 7) { hipLaunchKernelGGL((rs_encode_frame_reg_k<3, 3, 0, 4, 1>),
          dim3(grid2), dim3(CRC_BLOCKT), lds5, s, dst, dst_stride, base,
          stripe_stride, shard_len, k, ltabs, total2, fps2, tinyi); return; }
    }
    if (rabl == 4) { /* memory-floor skeleton (diagnostic only) */
      switch (m) {
        case 1: hipLaunchKernelGGL((rs_encode_frame_reg_k<1, 4, 1, 1>),
            dim3(grid2), dim3(CRC_BLOCKT), lds, s, dst, dst_stride, base,
            stripe_stride, shard_len, k, ltabs, total2, fps2, tinyi); break;
        case 3: hipLaunchKernelGGL((rs_encode_frame_reg_k<3, 4, 1, 1>),
            dim3(grid2), dim3(CRC_BLOCKT), lds, s, dst, dst_stride, base,
            stripe_stride, shard_len, k, ltabs, total2, fps2, tinyi); break;
        default: hipLaunchKernelGGL((rs_encode_frame_reg_k<4, 4, 1, 1>),
            dim3(grid2), dim3(CRC_BLOCKT), lds, s, dst, dst_stride, base,
            stripe_stride, shard_len, k, ltabs, total2, fps2, tinyi);
      }
      return;
    }
    if (map == 0) {
      if (var == 74) { GFRS_EFR_SW(4, 0) } else { GFRS_EFR_SW(5, 0) }
    } else if (map == 1 || (grid & 7) != 0) { /* XCD split needs grid%8==0 */
      if (var == 74) { GFRS_EFR_SW(4, 1) } else { GFRS_EFR_SW(5, 1) }
    } else {
      if (var == 74) { GFRS_EFR_SW(4, 2) } else { GFRS_EFR_SW(5, 2) }
    }
#undef GFRS_EFR_SW
#undef GFRS_EFR_GO
    return;
  }
  const int nbuf = (var >= 100 ? var / 100 : var / 10);
  const int ni = (var >= 100 ? var % 10 : 4);
  const int stg_one = 256 * (16 * ni + 16);
  const int lds = 8192 + EF_RED + nbuf * stg_one + m * k * 32;
#define GFRS_EF_GO(G, NB, W, I)                                           \
  hipLaunchKernelGGL((rs_encode_frame_k<G, NB, W, 0, I>), dim3(grid),     \
                     dim3(CRC_BLOCKT), lds, s, dst, dst_stride, base,     \
                     stripe_stride, shard_len, k, tabs, total, fps)
#define GFRS_EF_SW(NB, W, I)                                              \
  switch (m) {                                                            \
    case 1: GFRS_EF_GO(1, NB, W, I); break;                               \
    case 2: GFRS_EF_GO(2, NB, W, I); break;                               \
    case 3: GFRS_EF_GO(3, NB, W, I); break;                               \
    default: GFRS_EF_GO(4, NB, W, I);                                     \
  }
  static const int abl = []() {
    const char *e = getenv("GFRS_EF_ABL");
    return e ? atoi(e) : 0;
  }();
  if (abl == 1) {
    switch (m) { case 3: hipLaunchKernelGGL((rs_encode_frame_k<3, 1, 4, 1>),
        dim3(grid), dim3(CRC_BLOCKT), lds, s, dst, dst_stride, base,
        stripe_stride, shard_len, k, tabs, total, fps); return;
      default: break; }
  } else if (abl == 2) {
    switch (m) { case 3: hipLaunchKernelGGL((rs_encode_frame_k<3, 1, 4, 2>),
        dim3(grid), dim3(CRC_BLOCKT), lds, s, dst, dst_stride, base,
        stripe_stride, shard_len, k, tabs, total, fps); return;
      default: break; }
  } else if (abl == 3) {
    switch (m) { case 3: hipLaunchKernelGGL((rs_encode_frame_k<3, 1, 4, 3>),
        dim3(grid), dim3(CRC_BLOCKT), lds, s, dst, dst_stride, base,
        stripe_stride, shard_len, k, tabs, total, fps); return;
      default: break; }
  }
  if (var == 13) { GFRS_EF_SW(1, 3, 4) }
  else if (var == 14) { GFRS_EF_SW(1, 4, 4) }
  else if (var == 24) { GFRS_EF_SW(2, 4, 4) }
  else if (var == 142) { GFRS_EF_SW(1, 4, 2) }
  else if (var == 152) { GFRS_EF_SW(1, 5, 2) }
  else if (var == 162) { GFRS_EF_SW(1, 6, 2) }
  else { GFRS_EF_SW(2, 3, 4) }
#undef GFRS_EF_SW
#undef GFRS_EF_GO
}

/* Encode+frame queue, frame class: rs_encode_frame_reg_k<GM, WPS, 0, 0, 1,
 * ST> over the work items of one frame bucket of the encode schedule
 * (gfrs_plan.h).  The math of a frame - the 16 KiB passes, the register CRC
 * with the chained per-pass operators, the one-unit lookahead, the
 * LDS-staged tail bytes, the frame header store - is the batch kernel's;
 * what differs is where a frame comes from, which is rs_repair_frame_queue_k's
 * way:
 *  - the grid is capped and block b walks frames b, b + grid, b + 2*grid, ...
 *    of the bucket: the batch kernel's grid-stride walk, which keeps
 *    co-resident blocks on neighbouring frames.  (rs_repair_frame_queue_k's
 *    CONTIGUOUS ranges [b*per_blk, (b+1)*per_blk) measured 23 % slower here
 *    on the headline shape)  frame -> work item:
 *    one binary search over the frame prefix sums at the block's first
 *    frame, then a forward gallop + bisection from the current item (one
 *    compare while the frame stays inside it).  All of it depends on
 *    blockIdx and kernel arguments only, so the search and the item are
 *    scalar loads;
 *  - there is one encode plan per context: ctab is staged once, before the
 *    loop, and never restaged;
 *  - every pointer is rebuilt from base + item.off; the image row of shard j
 *    is dst + item.img + j*item.img_stride + f*65536;
 *  - cross-frame prefetch: the batch kernel computes the next frame's unit 0
 *    from the CURRENT shard_len and stripe arithmetic.  Here the next frame
 *    may belong to another job, so after a frame's last pass the address,
 *    length and mask come from the NEXT item's own off and shard_len; `pref`
 *    (block-uniform) says that vnext holds exactly the loads the top of the
 *    next frame would issue, otherwise the top issues them.  No load ever
 *    leaves the data shards of the job it belongs to;
 *  - no tiny-last-frame fold: a trailing frame of <= 64 payload bytes is a
 *    frame of the prefix sums like any other and gets its own workgroup
 *    iteration. */
template <int GM, int WPS, int ST>
__global__ __launch_bounds__(CRC_BLOCKT, WPS) void rs_encode_frame_queue_k(
    uint8_t *__restrict__ dst /* framed */, uint64_t base,
    const gfrs_eitem *__restrict__ items,
    const uint64_t *__restrict__ frame_prefix, uint32_t nitems,
    uint64_t total_frames, int k,
    const uint8_t *__restrict__ tabs /* [GM*k][32] */) {
  constexpr int EF_PASS = 16384;
  constexpr int EF_PASSES = 4;
  constexpr int64_t block_len = 65536;
  constexpr int64_t payload_full = block_len - CRC_LEN;

  /* block b walks frames b, b + grid, b + 2*grid, ... */
  const uint64_t f_step = uint64_t(gridDim.x);
  const uint64_t f_lo = uint64_t(blockIdx.x);
  const uint64_t f_hi = total_frames;
  if (f_lo >= f_hi) return; /* whole block, before any barrier */

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t(*tab)[256] = reinterpret_cast<uint32_t(*)[256]>(smem);
  uint32_t(*stab)[256] = reinterpret_cast<uint32_t(*)[256]>(smem + 8192);
  uint32_t *red = reinterpret_cast<uint32_t *>(smem + 12288);
  uint32_t *x8tab = reinterpret_cast<uint32_t *>(smem + 12288 + EF_RED);
  uint8_t *tailb = smem + 12288 + EF_RED + 64;
  uint8_t *ctab = smem + 12288 + EF_RED + 64 + 256;
  for (int i = threadIdx.x; i < 2048; i += CRC_BLOCKT)
    (&tab[0][0])[i] = (&g_crc_tab4[0][0])[i];
  for (int i = threadIdx.x; i < 1024; i += CRC_BLOCKT)
    (&stab[0][0])[i] = (&g_shift4k[0][0])[i];
  for (int i = threadIdx.x; i < GM * k * 2; i += CRC_BLOCKT)
    reinterpret_cast<uint4 *>(ctab)[i] =
        reinterpret_cast<const uint4 *>(tabs)[i];
  if (threadIdx.x == 0) {
    uint32_t v = 0x80000000u;
    for (int j = 0; j < 16; j++) {
      x8tab[j] = v;
      v = gf2_mulmod_d(v, g_pow8[0]);
    }
  }
  const int64_t lane16 = int64_t(threadIdx.x) * 16;
  const int lane16i = int(threadIdx.x) * 16;
  constexpr uint32_t INV16K = 0x479933FCu;
  const uint32_t op_pA =
      x8n_d(uint64_t(payload_full - (3 * 4096 + lane16 + 16)));
  const uint32_t op_pB = gf2_mulmod_d(op_pA, INV16K);
  const uint32_t op_pC = gf2_mulmod_d(op_pB, INV16K);
  const uint32_t op_pD = gf2_mulmod_d(op_pC, INV16K);
  const uint32_t it_full =
      gf2_mulmod_d(x8n_d(uint64_t(payload_full)), 0xFFFFFFFFu);
  __syncthreads();

  /* largest it with frame_prefix[it] <= f_lo (frame_prefix[0] == 0) */
  uint32_t it = 0;
  for (uint32_t hi = nitems; hi - it > 1;) {
    const uint32_t mid = it + (hi - it) / 2;
    if (frame_prefix[mid] <= f_lo)
      it = mid;
    else
      hi = mid;
  }

  uint4 vnext[4] = {uint4{0, 0, 0, 0}, uint4{0, 0, 0, 0}, uint4{0, 0, 0, 0},
                    uint4{0, 0, 0, 0}};
  bool pref = false; /* vnext = pass 0, unit 0 of the frame about to start */

  /* `it` -> the item of frame `to` (>= the frame `it` stands for): gallop,
   * then bisect; one compare when the frame belongs to the same item */
  auto advance = [&](uint32_t from, uint64_t to) {
    if (frame_prefix[from + 1] > to) return from; /* from + 1 <= nitems */
    uint32_t lo = from + 1, step = 1;
    while (lo + step < nitems && frame_prefix[lo + step] <= to) {
      lo += step;
      step <<= 1;
    }
    uint32_t hi = lo + step < nitems ? lo + step : nitems;
    while (hi - lo > 1) { /* frame_prefix[lo] <= to < frame_prefix[hi] */
      const uint32_t mid = lo + (hi - lo) / 2;
      if (frame_prefix[mid] <= to)
        lo = mid;
      else
        hi = mid;
    }
    return lo;
  };

  for (uint64_t fr = f_lo; fr < f_hi; fr += f_step) {
    it = advance(it, fr); /* a no-op after a prefetch */
    const gfrs_eitem item = items[it];
    const size_t shard_len = item.shard_len;
    const int64_t f = int64_t(fr - frame_prefix[it]);
    const int64_t p0 = f * payload_full;
    const int64_t payload = i64min(payload_full, int64_t(shard_len) - p0);
    const uint8_t *sbase = as_global(base + item.off);
    /* frame f of the image of shard 0; shard j at + j * img_stride */
    uint8_t *irow = dst + item.img + f * block_len;

    uint4 acc[GM][4];
    if (!pref) { /* pass 0, unit 0 */
      const int rb0 = int(i64min(int64_t(EF_PASS), payload));
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int off = i * 4096 + lane16i;
        vnext[i] = off + 16 <= rb0
                       ? *reinterpret_cast<const uint4 *>(sbase + p0 + off)
                       : uint4{0, 0, 0, 0};
      }
    }
    pref = false;
    for (int j = threadIdx.x; j < 64; j += CRC_BLOCKT) red[j] = 0;
    __syncthreads();

    for (int h = 0; h < EF_PASSES; h++) {
      const int64_t r0 = int64_t(h) * EF_PASS;
      const int64_t rbytes = i64min(int64_t(EF_PASS), payload - r0);
      if (rbytes <= 0) break;
#pragma unroll
      for (int r = 0; r < GM; r++)
#pragma unroll
        for (int i = 0; i < 4; i++) acc[r][i] = uint4{0, 0, 0, 0};

      uint32_t op = h == 0   ? op_pA
                    : h == 1 ? op_pB
                    : h == 2 ? op_pC
                             : op_pD;
      if (h == EF_PASSES - 1 && threadIdx.x == 255)
        op = shift4k(op, stab); /* lane 255's last pass has 3 pieces */
      if (payload != payload_full) {
        int np = 0;
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (int64_t(i) * 4096 + lane16 + 16 <= rbytes) np = i + 1;
        const int64_t end =
            np ? r0 + int64_t(np - 1) * 4096 + lane16 + 16 : r0;
        op = x8n_d(uint64_t(payload - end));
      }

      const int rbi = int(rbytes);
      for (int c = 0; c < k; c++) {
        const uint8_t *src = sbase + size_t(c) * shard_len + p0 + r0;
        uint8_t *fdst = irow + size_t(c) * item.img_stride + CRC_LEN + r0;
        LinTab lt[GM];
#pragma unroll
        for (int r = 0; r < GM; r++) lt[r] = lintab_load(ctab, r * k + c);
        uint4 vcur[4];
#pragma unroll
        for (int i = 0; i < 4; i++) vcur[i] = vnext[i];
        if (c + 1 < k) { /* next input's loads fly over this MAC */
          const uint8_t *nsrc = sbase + size_t(c + 1) * shard_len + p0 + r0;
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const int off = i * 4096 + lane16i;
            vnext[i] = off + 16 <= rbi
                           ? *reinterpret_cast<const uint4 *>(nsrc + off)
                           : uint4{0, 0, 0, 0};
          }
        }
        uint32_t t = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int off = i * 4096 + lane16i;
          if (off + 16 <= rbi) {
            const uint4 v = vcur[i];
#pragma unroll
            for (int d = 0; d < 4; d++)
              gfmac4_lin_rows<GM>(acc, i, d, (&v.x)[d], lt);
            fstore16<ST>(fdst + off, v);
            t = shift4k(t, stab) ^ crc16_reg(v, tab);
          }
        }
        uint32_t part = t ? gf2_mulmod_d(op, t) : 0;
        if (rbytes < EF_PASS) { /* lane-parallel tail, one byte per lane */
          const int t0 = (rbi / 16) * 16;
          const int p = t0 + int(threadIdx.x);
          if (p < rbi) {
            const uint8_t x = src[p];
            fdst[p] = x;
            tailb[c * 16 + (p - t0)] = x;
            part ^= gf2_mulmod_d(x8tab[rbi - 1 - p], tab[0][x]);
          }
        }
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1)
          part ^= __shfl_xor(part, sh, 64);
        if ((threadIdx.x & 63) == 0)
          red[(threadIdx.x >> 6) * 16 + c] ^= part;
      }
      if (rbytes < EF_PASS) __syncthreads(); /* tailb visible to all */
      { /* unit 0 of the next pass, or of the next frame, flies during the
           parity rows and the frame epilogue */
        const int64_t r0n = r0 + EF_PASS;
        int64_t rbn = i64min(int64_t(EF_PASS), payload - r0n);
        const uint8_t *nbase = sbase + p0 + r0n;
        if (rbn <= 0 && fr + f_step < f_hi) {
          /* this block's next frame, from ITS item (the same job or a later
           * one: its own off and shard_len); `it` moves on with it - the
           * rest of this frame works on `item` */
          it = advance(it, fr + f_step);
          const gfrs_eitem nx = items[it];
          const int64_t p0n =
              int64_t(fr + f_step - frame_prefix[it]) * payload_full;
          rbn = i64min(int64_t(EF_PASS), int64_t(nx.shard_len) - p0n);
          nbase = as_global(base + nx.off) + p0n;
          pref = true;
        }
        if (rbn > 0) {
          const int rbni = int(rbn);
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const int off = i * 4096 + lane16i;
            vnext[i] = off + 16 <= rbni
                           ? *reinterpret_cast<const uint4 *>(nbase + off)
                           : uint4{0, 0, 0, 0};
          }
        }
      }
#pragma unroll
      for (int r = 0; r < GM; r++) {
        uint8_t *fdst = irow + size_t(k + r) * item.img_stride + CRC_LEN + r0;
        uint32_t t = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int off = i * 4096 + lane16i;
          if (off + 16 <= rbi) {
            fstore16<ST>(fdst + off, acc[r][i]);
            t = shift4k(t, stab) ^ crc16_reg(acc[r][i], tab);
          }
        }
        uint32_t part = t ? gf2_mulmod_d(op, t) : 0;
        if (rbytes < EF_PASS) {
          const int t0 = (rbi / 16) * 16;
          const int p = t0 + int(threadIdx.x);
          if (p < rbi) {
            uint8_t pv = 0;
            for (int c2 = 0; c2 < k; c2++) {
              const uint8_t b = tailb[c2 * 16 + (p - t0)];
              pv ^= gfmul1_lin(ctab + size_t(r * k + c2) * 32, b);
            }
            fdst[p] = pv;
            part ^= gf2_mulmod_d(x8tab[rbi - 1 - p], tab[0][pv]);
          }
        }
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1)
          part ^= __shfl_xor(part, sh, 64);
        if ((threadIdx.x & 63) == 0)
          red[(threadIdx.x >> 6) * 16 + k + r] ^= part;
      }
    }

    __syncthreads();
    { /* one frame-header lane per shard (j < k+GM <= 16, all in wave 0) */
      const int j = int(threadIdx.x);
      if (j < k + GM) {
        const uint32_t itv =
            payload == payload_full
                ? it_full
                : gf2_mulmod_d(x8n_d(uint64_t(payload)), 0xFFFFFFFFu);
        const uint32_t crc =
            ~(itv ^ red[j] ^ red[16 + j] ^ red[32 + j] ^ red[48 + j]);
        *reinterpret_cast<uint32_t *>(irow + size_t(j) * item.img_stride) =
            crc;
      }
    }
    __syncthreads();
  }
}

void launch_rs_encode_frame_queue(uint8_t *dst, uint64_t base,
                                  const gfrs_eitem *items,
                                  const uint64_t *frame_prefix,
                                  uint32_t nitems, uint64_t total_frames,
                                  int k, int m, const uint8_t *tabs, int var,
                                  hipStream_t s) {
  if (nitems == 0 || total_frames == 0) return;
  /* the cap of fused_grid, read on every launch: GFRS_CRC_GRID forces the
   * multi-frame walk and the cross-item prefetch at tiny shapes */
  const uint64_t cap = uint64_t(env_grid("GFRS_CRC_GRID", 16384));
  int grid = int(total_frames < cap ? total_frames : cap);
  const int lds = 12288 + EF_RED + 64 + 256 + m * k * 32;
  /* fused_grid's rule: the stride must not alias the frame position inside
   * a shard, or whole blocks get only the short last frames.  A bucket has
   * no single frames-per-shard, so keep the stride coprime with every count
   * up to 13 (shards below 852 KiB); a forced small grid is left alone */
  if (uint64_t(grid) < total_frames && grid >= 1024) {
    auto gcd = [](int a, int b) {
      while (b) { const int t2 = a % b; a = b; b = t2; }
      return a;
    };
    while (gcd(grid, 2 * 3 * 5 * 7 * 11 * 13) != 1) grid--;
  }
#define GFRS_EQ_GO(G, W, S)                                                \
  hipLaunchKernelGGL((rs_encode_frame_queue_k<G, W, S>), dim3(grid),       \
                     dim3(CRC_BLOCKT), lds, s, dst, base, items,           \
                     frame_prefix, nitems, total_frames, k, tabs)
#define GFRS_EQ_SW(W, S)                                                   \
  switch (m) {                                                             \
    case 1: GFRS_EQ_GO(1, W, S); break;                                    \
    case 2: GFRS_EQ_GO(2, W, S); break;                                    \
    case 3: GFRS_EQ_GO(3, W, S); break;                                    \
    default: GFRS_EQ_GO(4, W, S);                                          \
  }
  /* the two variants launch_rs_encode_frame picks by shard size: 76 = 3
   * waves/SIMD, plain stores; 87 = 4 waves/SIMD, nontemporal stores */
  if (var == 76) { GFRS_EQ_SW(3, 0) } else { GFRS_EQ_SW(4, 1) }
#undef GFRS_EQ_SW
#undef GFRS_EQ_GO
}

/* Put queue, wide tactics: rs_encode_frame_queue_k's frame - the grid-stride
 * walk, the advance map, the cross-item prefetch rule, the 16 KiB passes, the
 * register CRC, the LDS tail bytes, the header lanes - for one ROW GROUP of a
 * tactic whose m+l parity rows do not fit one launch, with three changes:
 *  - k up to PUT_MAX_N = 32: red has PF_SLOTS = 36 words per wave (k data
 *    slots + 4 parity slots), tailb 16 bytes for each of 32 inputs, ctab up
 *    to 4*32 coefficients; the header lanes j < k + GM <= 36 still sit in
 *    wave 0;
 *  - row0: the GM parity rows of the launch are image columns k + row0 + r,
 *    and tabs points at the group's slice of the plan;
 *  - DATA = true is group 0 and stores the data frames and their CRCs as the
 *    sibling does.  DATA = false is a later group: the data is loaded and
 *    multiplied only - no data store, no data CRC, no data header word, no
 *    tail-byte store to the data images (tailb is still filled: the parity
 *    tail bytes are computed from it).
 * No lane leaves the frame loop early, no load leaves the data shards of the
 * item it belongs to, no store leaves the declared images. */
constexpr int PF_SLOTS = 36;                /* red words per wave */
constexpr int PF_RED = 4 * PF_SLOTS * 4;    /* bytes */
constexpr int PF_TAILB = 32 * 16;
constexpr int PF_LDS_FIXED = 12288 + PF_RED + 64 + PF_TAILB;

template <int GM, int WPS, int ST, bool DATA>
__global__ __launch_bounds__(CRC_BLOCKT, WPS) void rs_put_frame_queue_k(
    uint8_t *__restrict__ dst /* disk images */, uint64_t base,
    const gfrs_eitem *__restrict__ items,
    const uint64_t *__restrict__ frame_prefix, uint32_t nitems,
    uint64_t total_frames, int k, int row0,
    const uint8_t *__restrict__ tabs /* [GM*k][32], the group's slice */) {
  /* DATA launches are group 0: row0 == 0 (launch_rs_put_frame_queue) */
  constexpr int EF_PASS = 16384;
  constexpr int EF_PASSES = 4;
  constexpr int64_t block_len = 65536;
  constexpr int64_t payload_full = block_len - CRC_LEN;

  /* block b walks frames b, b + grid, b + 2*grid, ... */
  const uint64_t f_step = uint64_t(gridDim.x);
  const uint64_t f_lo = uint64_t(blockIdx.x);
  const uint64_t f_hi = total_frames;
  if (f_lo >= f_hi) return; /* whole block, before any barrier */
  /* group 0 is the DATA launch: its rows start at 0 by construction, and
   * with the constant the parity image rows continue the data loop's pointer
   * as in the sibling (a runtime row0 costs the DATA forms two more spilled
   * VGPRs) */
  const int prow0 = DATA ? 0 : row0;

  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t(*tab)[256] = reinterpret_cast<uint32_t(*)[256]>(smem);
  uint32_t(*stab)[256] = reinterpret_cast<uint32_t(*)[256]>(smem + 8192);
  uint32_t *red = reinterpret_cast<uint32_t *>(smem + 12288);
  uint32_t *x8tab = reinterpret_cast<uint32_t *>(smem + 12288 + PF_RED);
  uint8_t *tailb = smem + 12288 + PF_RED + 64;
  uint8_t *ctab = smem + PF_LDS_FIXED;
  for (int i = threadIdx.x; i < 2048; i += CRC_BLOCKT)
    (&tab[0][0])[i] = (&g_crc_tab4[0][0])[i];
  for (int i = threadIdx.x; i < 1024; i += CRC_BLOCKT)
    (&stab[0][0])[i] = (&g_shift4k[0][0])[i];
  for (int i = threadIdx.x; i < GM * k * 2; i += CRC_BLOCKT)
    reinterpret_cast<uint4 *>(ctab)[i] =
        reinterpret_cast<const uint4 *>(tabs)[i];
  if (threadIdx.x == 0) {
    uint32_t v = 0x80000000u;
    for (int j = 0; j < 16; j++) {
      x8tab[j] = v;
      v = gf2_mulmod_d(v, g_pow8[0]);
    }
  }
  const int64_t lane16 = int64_t(threadIdx.x) * 16;
  const int lane16i = int(threadIdx.x) * 16;
  constexpr uint32_t INV16K = 0x479933FCu;
  const uint32_t op_pA =
      x8n_d(uint64_t(payload_full - (3 * 4096 + lane16 + 16)));
  const uint32_t op_pB = gf2_mulmod_d(op_pA, INV16K);
  const uint32_t op_pC = gf2_mulmod_d(op_pB, INV16K);
  const uint32_t op_pD = gf2_mulmod_d(op_pC, INV16K);
  const uint32_t it_full =
      gf2_mulmod_d(x8n_d(uint64_t(payload_full)), 0xFFFFFFFFu);
  __syncthreads();

  /* largest it with frame_prefix[it] <= f_lo (frame_prefix[0] == 0) */
  uint32_t it = 0;
  for (uint32_t hi = nitems; hi - it > 1;) {
    const uint32_t mid = it + (hi - it) / 2;
    if (frame_prefix[mid] <= f_lo)
      it = mid;
    else
      hi = mid;
  }

  uint4 vnext[4] = {uint4{0, 0, 0, 0}, uint4{0, 0, 0, 0}, uint4{0, 0, 0, 0},
                    uint4{0, 0, 0, 0}};
  bool pref = false; /* vnext = pass 0, unit 0 of the frame about to start */

  /* `it` -> the item of frame `to` (>= the frame `it` stands for): gallop,
   * then bisect; one compare when the frame belongs to the same item */
  auto advance = [&](uint32_t from, uint64_t to) {
    if (frame_prefix[from + 1] > to) return from; /* from + 1 <= nitems */
    uint32_t lo = from + 1, step = 1;
    while (lo + step < nitems && frame_prefix[lo + step] <= to) {
      lo += step;
      step <<= 1;
    }
    uint32_t hi = lo + step < nitems ? lo + step : nitems;
    while (hi - lo > 1) { /* frame_prefix[lo] <= to < frame_prefix[hi] */
      const uint32_t mid = lo + (hi - lo) / 2;
      if (frame_prefix[mid] <= to)
        lo = mid;
      else
        hi = mid;
    }
    return lo;
  };

  for (uint64_t fr = f_lo; fr < f_hi; fr += f_step) {
    it = advance(it, fr); /* a no-op after a prefetch */
    const gfrs_eitem item = items[it];
    const size_t shard_len = item.shard_len;
    const int64_t f = int64_t(fr - frame_prefix[it]);
    const int64_t p0 = f * payload_full;
    const int64_t payload = i64min(payload_full, int64_t(shard_len) - p0);
    const uint8_t *sbase = as_global(base + item.off);
    /* frame f of the body of shard 0's image; column j at + j * img_stride */
    uint8_t *irow = dst + item.img + f * block_len;

    uint4 acc[GM][4];
    if (!pref) { /* pass 0, unit 0 */
      const int rb0 = int(i64min(int64_t(EF_PASS), payload));
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int off = i * 4096 + lane16i;
        vnext[i] = off + 16 <= rb0
                       ? *reinterpret_cast<const uint4 *>(sbase + p0 + off)
                       : uint4{0, 0, 0, 0};
      }
    }
    pref = false;
    for (int j = threadIdx.x; j < 4 * PF_SLOTS; j += CRC_BLOCKT) red[j] = 0;
    __syncthreads();

    for (int h = 0; h < EF_PASSES; h++) {
      const int64_t r0 = int64_t(h) * EF_PASS;
      const int64_t rbytes = i64min(int64_t(EF_PASS), payload - r0);
      if (rbytes <= 0) break;
#pragma unroll
      for (int r = 0; r < GM; r++)
#pragma unroll
        for (int i = 0; i < 4; i++) acc[r][i] = uint4{0, 0, 0, 0};

      uint32_t op = h == 0   ? op_pA
                    : h == 1 ? op_pB
                    : h == 2 ? op_pC
                             : op_pD;
      if (h == EF_PASSES - 1 && threadIdx.x == 255)
        op = shift4k(op, stab); /* lane 255's last pass has 3 pieces */
      if (payload != payload_full) {
        int np = 0;
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (int64_t(i) * 4096 + lane16 + 16 <= rbytes) np = i + 1;
        const int64_t end =
            np ? r0 + int64_t(np - 1) * 4096 + lane16 + 16 : r0;
        op = x8n_d(uint64_t(payload - end));
      }

      const int rbi = int(rbytes);
      for (int c = 0; c < k; c++) {
        const uint8_t *src = sbase + size_t(c) * shard_len + p0 + r0;
        uint8_t *fdst = irow + size_t(c) * item.img_stride + CRC_LEN + r0;
        LinTab lt[GM];
#pragma unroll
        for (int r = 0; r < GM; r++) lt[r] = lintab_load(ctab, r * k + c);
        uint4 vcur[4];
#pragma unroll
        for (int i = 0; i < 4; i++) vcur[i] = vnext[i];
        if (c + 1 < k) { /* next input's loads fly over this MAC */
          const uint8_t *nsrc = sbase + size_t(c + 1) * shard_len + p0 + r0;
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const int off = i * 4096 + lane16i;
            vnext[i] = off + 16 <= rbi
                           ? *reinterpret_cast<const uint4 *>(nsrc + off)
                           : uint4{0, 0, 0, 0};
          }
        }
        uint32_t t = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int off = i * 4096 + lane16i;
          if (off + 16 <= rbi) {
            const uint4 v = vcur[i];
#pragma unroll
            for (int d = 0; d < 4; d++)
              gfmac4_lin_rows<GM>(acc, i, d, (&v.x)[d], lt);
            if (DATA) {
              fstore16<ST>(fdst + off, v);
              t = shift4k(t, stab) ^ crc16_reg(v, tab);
            }
          }
        }
        uint32_t part = 0;
        if (DATA) part = t ? gf2_mulmod_d(op, t) : 0;
        if (rbytes < EF_PASS) { /* lane-parallel tail, one byte per lane */
          const int t0 = (rbi / 16) * 16;
          const int p = t0 + int(threadIdx.x);
          if (p < rbi) {
            const uint8_t x = src[p];
            tailb[c * 16 + (p - t0)] = x;
            if (DATA) {
              fdst[p] = x;
              part ^= gf2_mulmod_d(x8tab[rbi - 1 - p], tab[0][x]);
            }
          }
        }
        if (DATA) {
#pragma unroll
          for (int sh = 32; sh > 0; sh >>= 1)
            part ^= __shfl_xor(part, sh, 64);
          if ((threadIdx.x & 63) == 0)
            red[(threadIdx.x >> 6) * PF_SLOTS + c] ^= part;
        }
      }
      if (rbytes < EF_PASS) __syncthreads(); /* tailb visible to all */
      { /* unit 0 of the next pass, or of the next frame, flies during the
           parity rows and the frame epilogue */
        const int64_t r0n = r0 + EF_PASS;
        int64_t rbn = i64min(int64_t(EF_PASS), payload - r0n);
        const uint8_t *nbase = sbase + p0 + r0n;
        if (rbn <= 0 && fr + f_step < f_hi) {
          /* this block's next frame, from ITS item (the same job or a later
           * one: its own off and shard_len); `it` moves on with it - the
           * rest of this frame works on `item` */
          it = advance(it, fr + f_step);
          const gfrs_eitem nx = items[it];
          const int64_t p0n =
              int64_t(fr + f_step - frame_prefix[it]) * payload_full;
          rbn = i64min(int64_t(EF_PASS), int64_t(nx.shard_len) - p0n);
          nbase = as_global(base + nx.off) + p0n;
          pref = true;
        }
        if (rbn > 0) {
          const int rbni = int(rbn);
#pragma unroll
          for (int i = 0; i < 4; i++) {
            const int off = i * 4096 + lane16i;
            vnext[i] = off + 16 <= rbni
                           ? *reinterpret_cast<const uint4 *>(nbase + off)
                           : uint4{0, 0, 0, 0};
          }
        }
      }
#pragma unroll
      for (int r = 0; r < GM; r++) {
        uint8_t *fdst =
            irow + size_t(k + prow0 + r) * item.img_stride + CRC_LEN + r0;
        uint32_t t = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int off = i * 4096 + lane16i;
          if (off + 16 <= rbi) {
            fstore16<ST>(fdst + off, acc[r][i]);
            t = shift4k(t, stab) ^ crc16_reg(acc[r][i], tab);
          }
        }
        uint32_t part = t ? gf2_mulmod_d(op, t) : 0;
        if (rbytes < EF_PASS) {
          const int t0 = (rbi / 16) * 16;
          const int p = t0 + int(threadIdx.x);
          if (p < rbi) {
            uint8_t pv = 0;
            for (int c2 = 0; c2 < k; c2++) {
              const uint8_t b = tailb[c2 * 16 + (p - t0)];
              pv ^= gfmul1_lin(ctab + size_t(r * k + c2) * 32, b);
            }
            fdst[p] = pv;
            part ^= gf2_mulmod_d(x8tab[rbi - 1 - p], tab[0][pv]);
          }
        }
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1)
          part ^= __shfl_xor(part, sh, 64);
        if ((threadIdx.x & 63) == 0)
          red[(threadIdx.x >> 6) * PF_SLOTS + k + r] ^= part;
      }
    }

    __syncthreads();
    { /* one frame-header lane per image column of the launch: the k data
         columns (DATA only) and the GM parity columns; j < k + GM <= 36, all
         in wave 0 */
      const int j = int(threadIdx.x);
      if (j < k + GM && (DATA || j >= k)) {
        const uint32_t itv =
            payload == payload_full
                ? it_full
                : gf2_mulmod_d(x8n_d(uint64_t(payload)), 0xFFFFFFFFu);
        const uint32_t crc =
            ~(itv ^ red[j] ^ red[PF_SLOTS + j] ^ red[2 * PF_SLOTS + j] ^
              red[3 * PF_SLOTS + j]);
        const int col = j < k ? j : j + prow0;
        *reinterpret_cast<uint32_t *>(irow + size_t(col) * item.img_stride) =
            crc;
      }
    }
    __syncthreads();
  }
}

void launch_rs_put_frame_queue(uint8_t *dst, uint64_t base,
                               const gfrs_eitem *items,
                               const uint64_t *frame_prefix, uint32_t nitems,
                               uint64_t total_frames, int k, int gm, int row0,
                               const uint8_t *tabs, int var, bool data,
                               hipStream_t s) {
  if (nitems == 0 || total_frames == 0) return;
  assert(!data || row0 == 0); /* the DATA build takes row0 as the constant 0 */
  /* the grid rule of launch_rs_encode_frame_queue */
  const uint64_t cap = uint64_t(env_grid("GFRS_CRC_GRID", 16384));
  int grid = int(total_frames < cap ? total_frames : cap);
  const int lds = PF_LDS_FIXED + gm * k * 32;
  if (uint64_t(grid) < total_frames && grid >= 1024) {
    auto gcd = [](int a, int b) {
      while (b) { const int t2 = a % b; a = b; b = t2; }
      return a;
    };
    while (gcd(grid, 2 * 3 * 5 * 7 * 11 * 13) != 1) grid--;
  }
#define GFRS_PQ_GO(G, W, S, D)                                             \
  hipLaunchKernelGGL((rs_put_frame_queue_k<G, W, S, D>), dim3(grid),       \
                     dim3(CRC_BLOCKT), lds, s, dst, base, items,           \
                     frame_prefix, nitems, total_frames, k, row0, tabs)
#define GFRS_PQ_SW(W, S, D)                                                \
  switch (gm) {                                                            \
    case 1: GFRS_PQ_GO(1, W, S, D); break;                                 \
    case 2: GFRS_PQ_GO(2, W, S, D); break;                                 \
    case 3: GFRS_PQ_GO(3, W, S, D); break;                                 \
    default: GFRS_PQ_GO(4, W, S, D);                                       \
  }
  if (var == 76) {
    if (data) { GFRS_PQ_SW(3, 0, true) } else { GFRS_PQ_SW(3, 0, false) }
  } else {
    if (data) { GFRS_PQ_SW(4, 1, true) } else { GFRS_PQ_SW(4, 1, false) }
  }
#undef GFRS_PQ_SW
#undef GFRS_PQ_GO
}

/* Encode+frame queue, small class: rs_encode_frame_small_k with the stripe
 * loop turned into a loop over the items of one small bucket, wave
 * 4*blockIdx + wv, grid-stride.  Every item of the bucket has
 * ceil(shard_len / 1024) == NI, so the NI-long loops stay compile-time, but
 * shard_len itself is per job: what the batch kernel hoists out of its loop
 * is computed per job here.  A lane's fold operator is x^(8*s), s = the bytes
 * after its last present piece; s < 1024 and s mod 16 == shard_len mod 16, so
 * it is one multiply of two LDS table entries, x^(128*(s/16)) and
 * x^(8*(s%16)), instead of a binary expansion per job; the frame's init term
 * x^(8*shard_len) * 0xFFFFFFFF likewise (shard_len / 16 <= 256).  The wave
 * index goes through readfirstlane so the item is a scalar load.  No barrier
 * after the prologue: a wave with no item left simply leaves the loop. */
template <int GM, int NI>
__global__ __launch_bounds__(CRC_BLOCKT, 4) void rs_encode_frame_small_queue_k(
    uint8_t *__restrict__ dst /* framed */, uint64_t base,
    const gfrs_eitem *__restrict__ items, uint32_t nitems, int k,
    const uint8_t *__restrict__ tabs /* [GM*k][32] */) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t(*tab)[256] = reinterpret_cast<uint32_t(*)[256]>(smem);
  uint32_t(*stab)[256] = reinterpret_cast<uint32_t(*)[256]>(smem + 8192);
  uint32_t *x8tab = reinterpret_cast<uint32_t *>(smem + 12288);
  /* x^(8*j) * 0xFFFFFFFF, j < 16 */
  uint32_t *x8init = reinterpret_cast<uint32_t *>(smem + 12288 + 64);
  /* x^(128*a), a <= 256 */
  uint32_t *x128tab = reinterpret_cast<uint32_t *>(smem + 12288 + 128);
  uint8_t *tailb = smem + 12288 + 128 + 1040; /* per-wave 16x16 tail bytes */
  uint8_t *ctab = smem + 12288 + 128 + 1040 + 4 * 256;
  for (int i = threadIdx.x; i < 2048; i += CRC_BLOCKT)
    (&tab[0][0])[i] = (&g_crc_tab4[0][0])[i];
  for (int i = threadIdx.x; i < 1024; i += CRC_BLOCKT)
    (&stab[0][0])[i] = (&g_shift1k[0][0])[i];
  for (int i = threadIdx.x; i < GM * k * 2; i += CRC_BLOCKT)
    reinterpret_cast<uint4 *>(ctab)[i] =
        reinterpret_cast<const uint4 *>(tabs)[i];
  { /* the operator tables, one entry per lane: no serial thread-0 chain */
    const uint32_t v = x8n_d(uint64_t(threadIdx.x) * 16);
    x128tab[threadIdx.x] = v;
    if (threadIdx.x == 255)
      x128tab[256] = gf2_mulmod_d(v, g_pow8[4]); /* times x^(8*16) */
    if (threadIdx.x < 16) {
      const uint32_t w = x8n_d(uint64_t(threadIdx.x));
      x8tab[threadIdx.x] = w;
      x8init[threadIdx.x] = gf2_mulmod_d(w, 0xFFFFFFFFu);
    }
  }
  __syncthreads();

  const int wv = __builtin_amdgcn_readfirstlane(int(threadIdx.x) >> 6);
  const int lane = int(threadIdx.x) & 63;
  const int lane16i = lane * 16;
  uint8_t *wtail = tailb + wv * 256;

  for (uint32_t w = blockIdx.x * 4 + uint32_t(wv); w < nitems;
       w += gridDim.x * 4) {
    const gfrs_eitem item = items[w];
    const size_t shard_len = item.shard_len;
    const int pli = int(shard_len); /* <= 4096 */
    const uint8_t *sbase = as_global(base + item.off);
    uint8_t *img0 = dst + item.img; /* image of shard j at + j*img_stride */
    /* lane's fold operator: suffix after its LAST present piece */
    int np = 0;
#pragma unroll
    for (int i = 0; i < NI; i++)
      if (i * 1024 + lane16i + 16 <= pli) np = i + 1;
    const int sfx = np ? pli - ((np - 1) * 1024 + lane16i + 16) : 0;
    const uint32_t op =
        np ? gf2_mulmod_d(x128tab[sfx >> 4], x8tab[sfx & 15]) : 0;
    const uint32_t it = gf2_mulmod_d(x128tab[pli >> 4], x8init[pli & 15]);
    const int t0 = (pli / 16) * 16;

    uint4 acc[GM][NI];
#pragma unroll
    for (int r = 0; r < GM; r++)
#pragma unroll
      for (int i = 0; i < NI; i++) acc[r][i] = uint4{0, 0, 0, 0};

    for (int c = 0; c < k; c++) {
      const uint8_t *src = sbase + size_t(c) * shard_len;
      uint8_t *fdst = img0 + size_t(c) * item.img_stride + CRC_LEN;
      uint32_t t = 0;
      LinTab lt[GM];
#pragma unroll
      for (int r = 0; r < GM; r++) lt[r] = lintab_load(ctab, r * k + c);
#pragma unroll
      for (int i = 0; i < NI; i++) {
        const int off = i * 1024 + lane16i;
        if (off + 16 <= pli) {
          const uint4 v = *reinterpret_cast<const uint4 *>(src + off);
#pragma unroll
          for (int d = 0; d < 4; d++)
            gfmac4_lin_rows_n<GM, NI>(acc, i, d, (&v.x)[d], lt);
          *reinterpret_cast<uint4 *>(fdst + off) = v;
          t = shift4k(t, stab) ^ crc16_reg(v, tab); /* stab = x^(8*1024) */
        }
      }
      uint32_t part = t ? gf2_mulmod_d(op, t) : 0;
      { /* tail bytes, one per lane; stage for the parity tails */
        const int p = t0 + lane;
        if (p < pli) {
          const uint8_t x = src[p];
          fdst[p] = x;
          wtail[c * 16 + (p - t0)] = x;
          part ^= gf2_mulmod_d(x8tab[pli - 1 - p], tab[0][x]);
        }
      }
#pragma unroll
      for (int sh = 32; sh > 0; sh >>= 1)
        part ^= __shfl_xor(part, sh, 64);
      if (lane == 0)
        *reinterpret_cast<uint32_t *>(img0 + size_t(c) * item.img_stride) =
            ~(it ^ part);
    }
#pragma unroll
    for (int r = 0; r < GM; r++) {
      uint8_t *fdst = img0 + size_t(k + r) * item.img_stride + CRC_LEN;
      uint32_t t = 0;
#pragma unroll
      for (int i = 0; i < NI; i++) {
        const int off = i * 1024 + lane16i;
        if (off + 16 <= pli) {
          *reinterpret_cast<uint4 *>(fdst + off) = acc[r][i];
          t = shift4k(t, stab) ^ crc16_reg(acc[r][i], tab);
        }
      }
      uint32_t part = t ? gf2_mulmod_d(op, t) : 0;
      {
        const int p = t0 + lane;
        if (p < pli) { /* same-wave LDS visibility: no barrier needed */
          uint8_t pv = 0;
          for (int c2 = 0; c2 < k; c2++) {
            const uint8_t b = wtail[c2 * 16 + (p - t0)];
            pv ^= gfmul1_lin(ctab + size_t(r * k + c2) * 32, b);
          }
          fdst[p] = pv;
          part ^= gf2_mulmod_d(x8tab[pli - 1 - p], tab[0][pv]);
        }
      }
#pragma unroll
      for (int sh = 32; sh > 0; sh >>= 1)
        part ^= __shfl_xor(part, sh, 64);
      if (lane == 0)
        *reinterpret_cast<uint32_t *>(img0 + size_t(k + r) * item.img_stride) =
            ~(it ^ part);
    }
  }
}

void launch_rs_encode_frame_small_queue(uint8_t *dst, uint64_t base,
                                        const gfrs_eitem *items,
                                        uint32_t nitems, int k, int m, int ni,
                                        const uint8_t *tabs, hipStream_t s) {
  if (nitems == 0) return;
  const int64_t groups = (int64_t(nitems) + 3) / 4;
  const int64_t cap = env_grid("GFRS_CRC_GRID", 16384);
  const int grid = int(groups < cap ? groups : cap);
  const int lds = 12288 + 128 + 1040 + 1024 + m * k * 32;
#define GFRS_SQ_GO(G, I)                                                  \
  hipLaunchKernelGGL((rs_encode_frame_small_queue_k<G, I>), dim3(grid),   \
                     dim3(CRC_BLOCKT), lds, s, dst, base, items, nitems,  \
                     k, tabs)
#define GFRS_SQ_NI(G)                                                     \
  switch (ni) {                                                           \
    case 1: GFRS_SQ_GO(G, 1); break;                                      \
    case 2: GFRS_SQ_GO(G, 2); break;                                      \
    case 3: GFRS_SQ_GO(G, 3); break;                                      \
    default: GFRS_SQ_GO(G, 4);                                            \
  }
  switch (m) {
    case 1: GFRS_SQ_NI(1); break;
    case 2: GFRS_SQ_NI(2); break;
    case 3: GFRS_SQ_NI(3); break;
    default: GFRS_SQ_NI(4);
  }
#undef GFRS_SQ_NI
#undef GFRS_SQ_GO
}

/* ------------------------------------------------------------------ */
/* blobnode on-disk shard codec (core/shard.go:42-111, datafile.go:342)  */
/* ------------------------------------------------------------------ */

/* disk image = header(32B) | crc32block body | footer(8B).
 * header: crc32(BE, bytes 4..32) | magic ab cd ef cc | bid u64 BE |
 *         vuid u64 BE | size u32 BE | reserved u32 0   (shard.go:42-58)
 * footer: magic cc ef cd ab | crc32(raw data) u32 BE   (shard.go:66-73)
 * The footer CRC is the finalized CRC of the UNFRAMED payload
 * (datafile.go:338,381 io.TeeReader into crc32.NewIEEE).  Instead of a
 * second pass over the data we GF(2)-combine the per-frame header CRCs the
 * framing kernel just wrote: crc(A‖B) = x^(8|B|)·crc(A) ^ crc(B) on
 * finalized values (proven against the oracle in tests). */

/* One wave per shard: write the 32-B header (prebuilt on host), fold the
 * frame CRCs into the footer. */
__global__ void shard_finalize_k(uint8_t *__restrict__ dst, size_t dst_stride,
                                 const uint64_t *__restrict__ bids,
                                 const uint64_t *__restrict__ vuids,
                                 int64_t raw_size, int64_t block_len,
                                 int nshards) {
  const int sh = blockIdx.x * (blockDim.x / 64) + (threadIdx.x / 64);
  const int lane = threadIdx.x & 63;
  if (sh >= nshards) return;
  uint8_t *img = dst + size_t(sh) * dst_stride;
  if (lane != 0) return;
  /* build the 32 B header on device (shard.go:241-261): host-side
   * construction was the bottleneck at millions of shards per call.
   * Memory is LE; the format stores bid/vuid/size/crc big-endian. */
  {
    const uint64_t bid = bids[sh], vuid = vuids[sh];
    uint32_t w[8];
    w[1] = 0xccefcdabu; /* ab cd ef cc */
    w[2] = __builtin_bswap32(uint32_t(bid >> 32));
    w[3] = __builtin_bswap32(uint32_t(bid));
    w[4] = __builtin_bswap32(uint32_t(vuid >> 32));
    w[5] = __builtin_bswap32(uint32_t(vuid));
    w[6] = __builtin_bswap32(uint32_t(raw_size));
    w[7] = 0;
    uint32_t c = 0xFFFFFFFFu;
#pragma unroll
    for (int i = 1; i < 8; i++) {
      const uint32_t x = w[i];
#pragma unroll
      for (int b = 0; b < 4; b++)
        c = g_crc_tab4[0][(c ^ (x >> (8 * b))) & 0xFF] ^ (c >> 8);
    }
    w[0] = __builtin_bswap32(~c);
    uint32_t *d32 = reinterpret_cast<uint32_t *>(img);
#pragma unroll
    for (int i = 0; i < 8; i++) d32[i] = w[i];
  }
  const int64_t payload_full = block_len - CRC_LEN;
  const int64_t nframes = (raw_size + payload_full - 1) / payload_full;
  uint32_t crc = 0;
  int64_t remain = raw_size;
  for (int64_t f = 0; f < nframes; f++) {
    uint32_t fc;
    __builtin_memcpy(&fc, img + 32 + f * block_len, 4); /* LE header */
    const int64_t plen = remain < payload_full ? remain : payload_full;
    crc = f == 0 ? fc : gf2_mulmod_d(x8n_d(uint64_t(plen)), crc) ^ fc;
    remain -= plen;
  }
  uint8_t *ftr = img + 32 + (raw_size + CRC_LEN * nframes);
  ftr[0] = 0xcc; ftr[1] = 0xef; ftr[2] = 0xcd; ftr[3] = 0xab;
  ftr[4] = uint8_t(crc >> 24); ftr[5] = uint8_t(crc >> 16); /* BE */
  ftr[6] = uint8_t(crc >> 8); ftr[7] = uint8_t(crc);
}

/* One wave per shard: parse+verify header and footer; body CRCs are
 * checked separately by the crc verify kernel.  out layout per shard:
 * {bid u64, vuid u64, size u64, err i64} (err: 0 ok, negative =
 * GFRS_ERR_* from gfrs.h). */
__global__ void shard_parse_k(const uint8_t *__restrict__ img0,
                              size_t stride, int64_t raw_size,
                              int64_t block_len, int nshards,
                              uint64_t *__restrict__ out) {
  const int sh = blockIdx.x * (blockDim.x / 64) + (threadIdx.x / 64);
  const int lane = threadIdx.x & 63;
  if (sh >= nshards || lane != 0) return;
  const uint8_t *img = img0 + size_t(sh) * stride;
  uint64_t *o = out + sh * 4;
  int64_t err = 0;
  /* header: magic + crc over bytes 4..32 (shard.go:278-305) */
  if (!(img[4] == 0xab && img[5] == 0xcd && img[6] == 0xef && img[7] == 0xcc))
    err = -9;
  uint32_t hcrc = 0xFFFFFFFFu;
  for (int i = 4; i < 32; i++) {
    hcrc ^= img[i];
    for (int b = 0; b < 8; b++)
      hcrc = (hcrc & 1) ? (hcrc >> 1) ^ CRC_POLY : hcrc >> 1;
  }
  hcrc = ~hcrc;
  const uint32_t want_h = (uint32_t(img[0]) << 24) | (uint32_t(img[1]) << 16) |
                          (uint32_t(img[2]) << 8) | uint32_t(img[3]);
  if (err == 0 && want_h != hcrc) err = -9;
  uint64_t bid = 0, vuid = 0;
  for (int i = 0; i < 8; i++) bid = (bid << 8) | img[8 + i];
  for (int i = 0; i < 8; i++) vuid = (vuid << 8) | img[16 + i];
  uint32_t size = (uint32_t(img[24]) << 24) | (uint32_t(img[25]) << 16) |
                  (uint32_t(img[26]) << 8) | uint32_t(img[27]);
  /* footer: magic + combined body CRC */
  const int64_t payload_full = block_len - CRC_LEN;
  const int64_t nframes = (raw_size + payload_full - 1) / payload_full;
  const uint8_t *ftr = img + 32 + raw_size + CRC_LEN * nframes;
  if (err == 0 && !(ftr[0] == 0xcc && ftr[1] == 0xef && ftr[2] == 0xcd &&
                    ftr[3] == 0xab))
    err = -9;
  uint32_t crc = 0;
  int64_t remain = raw_size;
  for (int64_t f = 0; f < nframes; f++) {
    uint32_t fc;
    __builtin_memcpy(&fc, img + 32 + f * block_len, 4);
    const int64_t plen = remain < payload_full ? remain : payload_full;
    crc = f == 0 ? fc : gf2_mulmod_d(x8n_d(uint64_t(plen)), crc) ^ fc;
    remain -= plen;
  }
  const uint32_t want_f = (uint32_t(ftr[4]) << 24) | (uint32_t(ftr[5]) << 16) |
                          (uint32_t(ftr[6]) << 8) | uint32_t(ftr[7]);
  if (err == 0 && want_f != crc) err = -9;
  o[0] = bid;
  o[1] = vuid;
  o[2] = size;
  o[3] = uint64_t(err);
}

void launch_shard_finalize(uint8_t *dst, size_t dst_stride,
                           const uint64_t *bids, const uint64_t *vuids,
                           int64_t raw_size, int64_t block_len, int nshards,
                           hipStream_t s) {
  const int wps = 4; /* waves per block */
  const int blocks = (nshards + wps - 1) / wps;
  hipLaunchKernelGGL(shard_finalize_k, dim3(blocks), dim3(wps * 64), 0, s,
                     dst, dst_stride, bids, vuids, raw_size, block_len,
                     nshards);
}

/* shard_finalize_k for a repair queue: one wave per image, its place, raw
 * size and ids read from the image table (block_len 65536).  crcs (the put
 * queue's; NULL for the repair queue) also gets the footer's value of image
 * sh at crcs[sh]. */
__global__ void shard_finalize_queue_k(uint8_t *__restrict__ dst,
                                       const gfrs_rimage *__restrict__ imgs,
                                       int nimg, uint32_t *__restrict__ crcs) {
  constexpr int64_t block_len = 65536;
  const int sh = blockIdx.x * (blockDim.x / 64) + (threadIdx.x / 64);
  const int lane = threadIdx.x & 63;
  if (sh >= nimg || lane != 0) return;
  const gfrs_rimage im = imgs[sh];
  uint8_t *img = dst + im.off;
  const int64_t raw_size = int64_t(im.size);
  { /* the 32 B header (shard.go:241-261), big-endian fields */
    uint32_t w[8];
    w[1] = 0xccefcdabu; /* ab cd ef cc */
    w[2] = __builtin_bswap32(uint32_t(im.bid >> 32));
    w[3] = __builtin_bswap32(uint32_t(im.bid));
    w[4] = __builtin_bswap32(uint32_t(im.vuid >> 32));
    w[5] = __builtin_bswap32(uint32_t(im.vuid));
    w[6] = __builtin_bswap32(uint32_t(raw_size));
    w[7] = 0;
    uint32_t c = 0xFFFFFFFFu;
#pragma unroll
    for (int i = 1; i < 8; i++) {
      const uint32_t x = w[i];
#pragma unroll
      for (int b = 0; b < 4; b++)
        c = g_crc_tab4[0][(c ^ (x >> (8 * b))) & 0xFF] ^ (c >> 8);
    }
    w[0] = __builtin_bswap32(~c);
    uint32_t *d32 = reinterpret_cast<uint32_t *>(img);
#pragma unroll
    for (int i = 0; i < 8; i++) d32[i] = w[i];
  }
  /* footer CRC: GF(2)-combine the frame CRCs the frame kernel wrote.  The
   * raw size is per image here, not a kernel argument, so x^(8*plen) would
   * be a per-lane computation in every iteration: the operator of a full
   * frame is computed once, only the last frame can need another */
  const int64_t payload_full = block_len - CRC_LEN;
  const int64_t nframes = (raw_size + payload_full - 1) / payload_full;
  const uint32_t op_full = x8n_d(uint64_t(payload_full));
  uint32_t crc = 0;
  int64_t remain = raw_size;
  for (int64_t f = 0; f < nframes; f++) {
    uint32_t fc;
    __builtin_memcpy(&fc, img + 32 + f * block_len, 4); /* LE header */
    const int64_t plen = remain < payload_full ? remain : payload_full;
    if (f == 0) {
      crc = fc;
    } else {
      const uint32_t op =
          plen == payload_full ? op_full : x8n_d(uint64_t(plen));
      crc = gf2_mulmod_d(op, crc) ^ fc;
    }
    remain -= plen;
  }
  uint8_t *ftr = img + 32 + (raw_size + CRC_LEN * nframes);
  ftr[0] = 0xcc; ftr[1] = 0xef; ftr[2] = 0xcd; ftr[3] = 0xab;
  ftr[4] = uint8_t(crc >> 24); ftr[5] = uint8_t(crc >> 16); /* BE */
  ftr[6] = uint8_t(crc >> 8); ftr[7] = uint8_t(crc);
  if (crcs) crcs[sh] = crc;
}

void launch_shard_finalize_queue(uint8_t *dst, const gfrs_rimage *imgs,
                                 int nimg, uint32_t *crcs, hipStream_t s) {
  if (nimg <= 0) return;
  const int wps = 4; /* waves per block */
  const int blocks = (nimg + wps - 1) / wps;
  hipLaunchKernelGGL(shard_finalize_queue_k, dim3(blocks), dim3(wps * 64), 0,
                     s, dst, imgs, nimg, crcs);
}

void launch_shard_parse(const uint8_t *img, size_t stride, int64_t raw_size,
                        int64_t block_len, int nshards, uint64_t *out,
                        hipStream_t s) {
  const int wps = 4;
  const int blocks = (nshards + wps - 1) / wps;
  hipLaunchKernelGGL(shard_parse_k, dim3(blocks), dim3(wps * 64), 0, s, img,
                     stride, raw_size, block_len, nshards, out);
}

/* ---- shard read queue: verify and unframe the disk images of a chunk ---- */

/* The read direction over disk images.  The walk is rs_read_frame_queue_k's:
 * a contiguous frame range per block, one binary search then a forward walk
 * over the prefix sums of TOUCHED frames, scalar item loads, every pointer
 * rebuilt from the item; frame f of the walk is frame from / 65532 + f of the
 * image, whose body starts 32 bytes in.  The frame is crc32b_verify_reg_k's:
 * per 16 KiB pass a lane Horner-chains its four 16-byte pieces through the
 * register CRC (crc16_reg / shift4k) and folds by its position operator - the
 * same operators, the same partial-frame rule - and the ragged tail bytes
 * take one lane each.  The pass terms stay in a register, so a frame costs
 * one wave reduction.  No GF tables, no descriptor, no MAC.
 * Lane 0 writes the computed CRC to fcrc[walk index] and lowers
 * bad[item.job] to f when the stored 4-byte LE word differs.
 * STORE adds the read kernel's clipped stores (store_clip16 / store_clip_tail
 * and the byte path of the ragged tail): what was loaded is what is stored,
 * only inside [from, to).  The STORE = false build has no global store but
 * the fcrc word and the atomic.
 * No lane leaves the frame loop early; no load leaves the touched frames of
 * the item's image; no store leaves the item's declared bytes. */
template <bool STORE, int WPS>
__global__ __launch_bounds__(CRC_BLOCKT, WPS) void shard_read_frame_queue_k(
    uint8_t *__restrict__ out, uint64_t chunk,
    const gfrs_sitem *__restrict__ items,
    const uint64_t *__restrict__ frame_prefix, uint32_t nitems,
    uint64_t total_frames, uint32_t *__restrict__ fcrc,
    unsigned long long *__restrict__ bad) {
  constexpr int EF_PASS = 16384;
  constexpr int EF_PASSES = 4;
  constexpr int64_t block_len = 65536;
  constexpr int64_t payload_full = block_len - CRC_LEN;
  constexpr uint32_t INV16K = 0x479933FCu;

  const uint64_t per_blk = (total_frames + gridDim.x - 1) / gridDim.x;
  const uint64_t f_lo = uint64_t(blockIdx.x) * per_blk;
  const uint64_t f_hi =
      f_lo + per_blk < total_frames ? f_lo + per_blk : total_frames;
  if (f_lo >= f_hi) return; /* whole block, before any barrier */

  __shared__ __attribute__((aligned(16))) uint32_t tab[8][256];
  __shared__ uint32_t stab[4][256];
  __shared__ uint32_t red[4];
  __shared__ uint32_t x8tab[16];
  for (int i = threadIdx.x; i < 2048; i += CRC_BLOCKT)
    (&tab[0][0])[i] = (&g_crc_tab4[0][0])[i];
  for (int i = threadIdx.x; i < 1024; i += CRC_BLOCKT)
    (&stab[0][0])[i] = (&g_shift4k[0][0])[i];
  if (threadIdx.x == 0) {
    uint32_t v = 0x80000000u;
    for (int j = 0; j < 16; j++) {
      x8tab[j] = v;
      v = gf2_mulmod_d(v, g_pow8[0]);
    }
  }
  const int lane16i = int(threadIdx.x) * 16;
  const uint32_t op_pA =
      x8n_d(uint64_t(payload_full - (3 * 4096 + lane16i + 16)));
  const uint32_t op_pB = gf2_mulmod_d(op_pA, INV16K);
  const uint32_t op_pC = gf2_mulmod_d(op_pB, INV16K);
  const uint32_t op_pD = gf2_mulmod_d(op_pC, INV16K);
  const uint32_t it_full =
      gf2_mulmod_d(x8n_d(uint64_t(payload_full)), 0xFFFFFFFFu);
  __syncthreads();

  /* largest it with frame_prefix[it] <= f_lo (frame_prefix[0] == 0) */
  uint32_t it = 0;
  for (uint32_t hi = nitems; hi - it > 1;) {
    const uint32_t mid = it + (hi - it) / 2;
    if (frame_prefix[mid] <= f_lo)
      it = mid;
    else
      hi = mid;
  }

  for (uint64_t fr = f_lo; fr < f_hi; fr++) {
    while (frame_prefix[it + 1] <= fr) it++; /* it + 1 <= nitems */
    const gfrs_sitem item = items[it];
    /* frame f of the image: the item's first touched frame + its walk index.
     * Everything below is 32-bit and relative to the frame: payload bytes,
     * and [lo, hi), the frame positions the range covers (lo % 4 == 0) */
    const int64_t f = int64_t(item.from / uint64_t(payload_full)) +
                      int64_t(fr - frame_prefix[it]);
    const int64_t p0 = f * payload_full;
    const int payload = int(i64min(payload_full, int64_t(item.size) - p0));
    const int64_t slo = int64_t(item.from) - p0;
    const int64_t shi = int64_t(item.to) - p0;
    const int lo = slo > 0 ? int(slo) : 0;
    const int hi = shi < int64_t(payload) ? int(shi) : payload;
    const uint8_t *fb = as_global(chunk + item.img + 32) + f * block_len;
    const uint8_t *pb = fb + CRC_LEN;
    /* the address frame position 0 would have; dereferenced inside [lo, hi)
     * only, and only by the STORE build */
    uint8_t *rowf = reinterpret_cast<uint8_t *>(uint64_t(out) + item.out +
                                                uint64_t(p0) - item.from);

    uint32_t part = 0;
#pragma unroll 1
    for (int h = 0; h < EF_PASSES; h++) {
      const int r0 = h * EF_PASS;
      const int rbi = payload - r0 < EF_PASS ? payload - r0 : EF_PASS;
      if (rbi <= 0) break; /* block-uniform */
      const bool inside = lo <= r0 && r0 + rbi <= hi; /* block-uniform */

      uint4 v[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int off = i * 4096 + lane16i;
        v[i] = off + 16 <= rbi
                   ? *reinterpret_cast<const uint4 *>(pb + r0 + off)
                   : uint4{0, 0, 0, 0};
      }

      uint32_t op = h == 0   ? op_pA
                    : h == 1 ? op_pB
                    : h == 2 ? op_pC
                             : op_pD;
      if (h == EF_PASSES - 1 && threadIdx.x == 255)
        op = shift4k(op, stab); /* lane 255's last pass has 3 pieces */
      if (payload != int(payload_full)) {
        int np = 0;
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (i * 4096 + lane16i + 16 <= rbi) np = i + 1;
        const int end = np ? r0 + (np - 1) * 4096 + lane16i + 16 : r0;
        op = x8n_d(uint64_t(payload - end));
      }

      uint32_t t = 0;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int off = i * 4096 + lane16i;
        if (off + 16 <= rbi) t = shift4k(t, stab) ^ crc16_reg(v[i], tab);
      }
      part ^= t ? gf2_mulmod_d(op, t) : 0;

      if (STORE) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int off = i * 4096 + lane16i;
          if (off + 16 <= rbi)
            store_clip16(rowf, r0 + off, lo, hi, inside, v[i]);
        }
        if (!inside) store_clip_tail(rowf, r0, rbi & ~15, hi, v);
      }
      if (rbi & 15) { /* ragged tail of the frame: one lane per byte */
        const int p = (rbi & ~15) + int(threadIdx.x);
        if (p < rbi) {
          const uint8_t x = pb[r0 + p];
          part ^= gf2_mulmod_d(x8tab[rbi - 1 - p], tab[0][x]);
          const int q = r0 + p;
          if (STORE && q >= lo && q < hi) rowf[q] = x;
        }
      }
    }
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) part ^= __shfl_xor(part, sh, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint32_t itv =
          payload == int(payload_full)
              ? it_full
              : gf2_mulmod_d(x8n_d(uint64_t(payload)), 0xFFFFFFFFu);
      const uint32_t crc = ~(itv ^ red[0] ^ red[1] ^ red[2] ^ red[3]);
      fcrc[fr] = crc;
      const uint32_t want = uint32_t(fb[0]) | (uint32_t(fb[1]) << 8) |
                            (uint32_t(fb[2]) << 16) | (uint32_t(fb[3]) << 24);
      if (want != crc)
        atomicMin(&bad[item.job], static_cast<unsigned long long>(f));
    }
    __syncthreads(); /* red is the next frame's too */
  }
}

void launch_shard_read_frame_queue(uint8_t *out, uint64_t chunk,
                                   const gfrs_sitem *items,
                                   const uint64_t *frame_prefix,
                                   uint32_t nitems, uint64_t total_frames,
                                   bool store, uint32_t *fcrc, int64_t *bad,
                                   hipStream_t s) {
  if (nitems == 0 || total_frames == 0) return;
  /* the cap of the other frame queues, read on every launch: GFRS_CRC_GRID
   * forces the multi-frame walk at tiny shapes */
  const uint64_t cap = uint64_t(env_grid("GFRS_CRC_GRID", 16384));
  const int grid = int(total_frames < cap ? total_frames : cap);
  /* waves per SIMD: 8, the verify kernel's; GFRS_SRD_WAVES = 4 or 8 overrides
   * it and, like GFRS_RD_WAVES, is read on every launch, so a test can run
   * both builds */
  const char *we = getenv("GFRS_SRD_WAVES");
  const int wv = we ? atoi(we) : 0;
  unsigned long long *ubad = reinterpret_cast<unsigned long long *>(bad);
#define GFRS_SRD_GO(ST, W)                                                  \
  hipLaunchKernelGGL((shard_read_frame_queue_k<ST, W>), dim3(grid),         \
                     dim3(CRC_BLOCKT), 0, s, out, chunk, items,             \
                     frame_prefix, nitems, total_frames, fcrc, ubad)
  if (store) {
    if (wv == 4) GFRS_SRD_GO(true, 4);
    else GFRS_SRD_GO(true, 8);
  } else {
    if (wv == 4) GFRS_SRD_GO(false, 4);
    else GFRS_SRD_GO(false, 8);
  }
#undef GFRS_SRD_GO
}

/* One wave per job, after the frame buckets on the same stream: parse the
 * 32-byte header (shard.go:278-305) into the three header bits and the stored
 * fields, take BODY_CRC from bad[j], and for FOOTER jobs fold the job's
 * computed frame CRCs into the CRC of the whole payload by
 * shard_finalize_queue_k's rule - the operator of a full frame once, another
 * only for the last frame - and compare the footer.  Geometry follows the
 * job's size, never the header's. */
__global__ void shard_head_queue_k(uint64_t chunk,
                                   const gfrs_sjob *__restrict__ jobs,
                                   const uint64_t *__restrict__ job_frame,
                                   const uint32_t *__restrict__ fcrc,
                                   const int64_t *__restrict__ bad,
                                   gfrs_sresult *__restrict__ results,
                                   int njobs) {
  constexpr int64_t block_len = 65536;
  constexpr int64_t payload_full = block_len - CRC_LEN;
  const int j = blockIdx.x * (blockDim.x / 64) + (threadIdx.x / 64);
  const int lane = threadIdx.x & 63;
  if (j >= njobs) return; /* whole wave */
  /* every lane does the wave-uniform work below; lane 0 writes the result */
  const gfrs_sjob jb = jobs[j];
  const uint8_t *img = as_global(chunk + jb.img_off);
  uint32_t status = 0;
  if (!(img[4] == 0xab && img[5] == 0xcd && img[6] == 0xef && img[7] == 0xcc))
    status |= GFRS_SHARD_HDR_MAGIC;
  uint32_t hcrc = 0xFFFFFFFFu;
  for (int i = 4; i < 32; i++)
    hcrc = g_crc_tab4[0][(hcrc ^ img[i]) & 0xFF] ^ (hcrc >> 8);
  hcrc = ~hcrc;
  const uint32_t want_h = (uint32_t(img[0]) << 24) | (uint32_t(img[1]) << 16) |
                          (uint32_t(img[2]) << 8) | uint32_t(img[3]);
  if (want_h != hcrc) status |= GFRS_SHARD_HDR_CRC;
  uint64_t bid = 0, vuid = 0;
  for (int i = 0; i < 8; i++) bid = (bid << 8) | img[8 + i];
  for (int i = 0; i < 8; i++) vuid = (vuid << 8) | img[16 + i];
  const uint64_t size = (uint64_t(img[24]) << 24) | (uint64_t(img[25]) << 16) |
                        (uint64_t(img[26]) << 8) | uint64_t(img[27]);
  if (bid != jb.bid || vuid != jb.vuid || size != jb.size)
    status |= GFRS_SHARD_HDR_MISMATCH;
  const int64_t bb = bad[j];
  if (bb != -1) status |= GFRS_SHARD_BODY_CRC;
  uint32_t crc = 0;
  if (jb.flags & GFRS_SJOB_FOOTER) {
    const int64_t raw_size = int64_t(jb.size);
    const int64_t nframes = (raw_size + payload_full - 1) / payload_full;
    const uint32_t *fc = fcrc + job_frame[j];
    const uint32_t op_full = x8n_d(uint64_t(payload_full));
    int64_t remain = raw_size;
    /* the fold is serial, its loads are not: 64 words per wave load */
    for (int64_t f0 = 0; f0 < nframes; f0 += 64) {
      const uint32_t mine = f0 + lane < nframes ? fc[f0 + lane] : 0;
      const int nf = int(nframes - f0 < 64 ? nframes - f0 : 64);
      for (int i = 0; i < nf; i++) {
        const uint32_t fcv = __shfl(mine, i, 64);
        const int64_t plen = remain < payload_full ? remain : payload_full;
        if (f0 + i == 0) {
          crc = fcv;
        } else {
          const uint32_t op =
              plen == payload_full ? op_full : x8n_d(uint64_t(plen));
          crc = gf2_mulmod_d(op, crc) ^ fcv;
        }
        remain -= plen;
      }
    }
    const uint8_t *ftr = img + 32 + (raw_size + CRC_LEN * nframes);
    if (!(ftr[0] == 0xcc && ftr[1] == 0xef && ftr[2] == 0xcd &&
          ftr[3] == 0xab))
      status |= GFRS_SHARD_FTR_MAGIC;
    const uint32_t want_f = (uint32_t(ftr[4]) << 24) |
                            (uint32_t(ftr[5]) << 16) |
                            (uint32_t(ftr[6]) << 8) | uint32_t(ftr[7]);
    if (want_f != crc) status |= GFRS_SHARD_FTR_CRC;
  }
  gfrs_sresult r;
  r.status = status;
  r.crc = crc;
  r.bad_block = bb;
  r.bid = bid;
  r.vuid = vuid;
  r.size = size;
  if (lane == 0) results[j] = r;
}

void launch_shard_head_queue(uint64_t chunk, const gfrs_sjob *jobs,
                             const uint64_t *job_frame, const uint32_t *fcrc,
                             const int64_t *bad, gfrs_sresult *results,
                             int njobs, hipStream_t s) {
  if (njobs <= 0) return;
  const int wps = 4; /* waves per block */
  const int blocks = (njobs + wps - 1) / wps;
  hipLaunchKernelGGL(shard_head_queue_k, dim3(blocks), dim3(wps * 64), 0, s,
                     chunk, jobs, job_frame, fcrc, bad, results, njobs);
}

/* ---- shard write queue: frame payloads into new disk images ---- */

/* The write direction over disk images: a payload in, a new image body out.
 * The walk is shard_read_frame_queue_k's - a contiguous frame range per
 * block, one binary search then a forward walk over the prefix sums, scalar
 * item loads, every pointer rebuilt from the item - over ALL frames of an
 * item, so frame f of the walk is frame f of both images.  The frame is that
 * kernel's too: per 16 KiB pass a lane Horner-chains its four 16-byte pieces
 * through the register CRC (crc16_reg / shift4k) and folds by its position
 * operator - the same operators, the same partial-frame rule - and the ragged
 * tail bytes take one lane each; a frame costs one wave reduction.  No GF
 * tables, no descriptor, no MAC.
 * IMG = false reads raw bytes (frame f at item.src + f * 65532), IMG = true
 * the body of a source image (item.src + 32 + f * 65536 + 4); either may sit
 * at any byte address.  What was loaded is stored at
 * dst + item.img + 32 + f * 65536 + 4, which is 4-aligned: a 16-byte piece
 * goes out as one 16-byte store when the frame's payload address is a
 * multiple of 16 (block-uniform), as four dwords otherwise; the ragged tail
 * bytes are gathered four lanes to a dword, and only the partial last dword
 * of a shard is stored by bytes.
 * Lane 0 stores the computed CRC as the frame's 4-byte LE word, writes it to
 * fcrc[walk index] and - IMG only - lowers bad[item.job] to f when the
 * source's stored word differs.
 * No lane leaves the frame loop early; no load leaves the item's source
 * bytes; no store leaves the new image's body. */
template <bool IMG, int WPS>
__global__ __launch_bounds__(CRC_BLOCKT, WPS) void shard_write_frame_queue_k(
    uint8_t *__restrict__ dst, uint64_t src,
    const gfrs_witem *__restrict__ items,
    const uint64_t *__restrict__ frame_prefix, uint32_t nitems,
    uint64_t total_frames, uint32_t *__restrict__ fcrc,
    unsigned long long *__restrict__ bad) {
  constexpr int EF_PASS = 16384;
  constexpr int EF_PASSES = 4;
  constexpr int64_t block_len = 65536;
  constexpr int64_t payload_full = block_len - CRC_LEN;
  constexpr uint32_t INV16K = 0x479933FCu;

  const uint64_t per_blk = (total_frames + gridDim.x - 1) / gridDim.x;
  const uint64_t f_lo = uint64_t(blockIdx.x) * per_blk;
  const uint64_t f_hi =
      f_lo + per_blk < total_frames ? f_lo + per_blk : total_frames;
  if (f_lo >= f_hi) return; /* whole block, before any barrier */

  __shared__ __attribute__((aligned(16))) uint32_t tab[8][256];
  __shared__ uint32_t stab[4][256];
  __shared__ uint32_t red[4];
  __shared__ uint32_t x8tab[16];
  for (int i = threadIdx.x; i < 2048; i += CRC_BLOCKT)
    (&tab[0][0])[i] = (&g_crc_tab4[0][0])[i];
  for (int i = threadIdx.x; i < 1024; i += CRC_BLOCKT)
    (&stab[0][0])[i] = (&g_shift4k[0][0])[i];
  if (threadIdx.x == 0) {
    uint32_t v = 0x80000000u;
    for (int j = 0; j < 16; j++) {
      x8tab[j] = v;
      v = gf2_mulmod_d(v, g_pow8[0]);
    }
  }
  const int lane16i = int(threadIdx.x) * 16;
  const uint32_t op_pA =
      x8n_d(uint64_t(payload_full - (3 * 4096 + lane16i + 16)));
  const uint32_t op_pB = gf2_mulmod_d(op_pA, INV16K);
  const uint32_t op_pC = gf2_mulmod_d(op_pB, INV16K);
  const uint32_t op_pD = gf2_mulmod_d(op_pC, INV16K);
  const uint32_t it_full =
      gf2_mulmod_d(x8n_d(uint64_t(payload_full)), 0xFFFFFFFFu);
  __syncthreads();

  /* largest it with frame_prefix[it] <= f_lo (frame_prefix[0] == 0) */
  uint32_t it = 0;
  for (uint32_t hi = nitems; hi - it > 1;) {
    const uint32_t mid = it + (hi - it) / 2;
    if (frame_prefix[mid] <= f_lo)
      it = mid;
    else
      hi = mid;
  }

  for (uint64_t fr = f_lo; fr < f_hi; fr++) {
    while (frame_prefix[it + 1] <= fr) it++; /* it + 1 <= nitems */
    const gfrs_witem item = items[it];
    const int64_t f = int64_t(fr - frame_prefix[it]);
    const int payload =
        int(i64min(payload_full, int64_t(item.size) - f * payload_full));
    /* pb: the frame's payload in the source; db: the frame in the new image,
     * its CRC word first */
    const uint8_t *pb =
        IMG ? as_global(src + item.src + 32) + f * block_len + CRC_LEN
            : as_global(src + item.src) + f * payload_full;
    uint8_t *db = reinterpret_cast<uint8_t *>(uint64_t(dst) + item.img + 32) +
                  f * block_len;
    uint8_t *dp = db + CRC_LEN;
    const bool al16 = (uint64_t(dp) & 15) == 0; /* block-uniform */

    uint32_t part = 0;
#pragma unroll 1
    for (int h = 0; h < EF_PASSES; h++) {
      const int r0 = h * EF_PASS;
      const int rbi = payload - r0 < EF_PASS ? payload - r0 : EF_PASS;
      if (rbi <= 0) break; /* block-uniform */

      uint4 v[4];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int off = i * 4096 + lane16i;
        v[i] = off + 16 <= rbi
                   ? *reinterpret_cast<const uint4 *>(pb + r0 + off)
                   : uint4{0, 0, 0, 0};
      }

      uint32_t op = h == 0   ? op_pA
                    : h == 1 ? op_pB
                    : h == 2 ? op_pC
                             : op_pD;
      if (h == EF_PASSES - 1 && threadIdx.x == 255)
        op = shift4k(op, stab); /* lane 255's last pass has 3 pieces */
      if (payload != int(payload_full)) {
        int np = 0;
#pragma unroll
        for (int i = 0; i < 4; i++)
          if (i * 4096 + lane16i + 16 <= rbi) np = i + 1;
        const int end = np ? r0 + (np - 1) * 4096 + lane16i + 16 : r0;
        op = x8n_d(uint64_t(payload - end));
      }

      uint32_t t = 0;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int off = i * 4096 + lane16i;
        if (off + 16 <= rbi) t = shift4k(t, stab) ^ crc16_reg(v[i], tab);
      }
      part ^= t ? gf2_mulmod_d(op, t) : 0;

#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int off = i * 4096 + lane16i;
        if (off + 16 <= rbi) {
          uint8_t *q = dp + r0 + off;
          if (al16) {
            *reinterpret_cast<uint4 *>(q) = v[i];
          } else {
            uint32_t *dw = reinterpret_cast<uint32_t *>(q);
            dw[0] = v[i].x; dw[1] = v[i].y; dw[2] = v[i].z; dw[3] = v[i].w;
          }
        }
      }
      if (rbi & 15) { /* ragged tail of the frame: one lane per byte */
        const int nt = rbi & 15;
        const int tl = int(threadIdx.x);
        const int p = (rbi & ~15) + tl;
        uint32_t x = 0;
        if (tl < nt) {
          x = pb[r0 + p];
          part ^= gf2_mulmod_d(x8tab[rbi - 1 - p], tab[0][x]);
        }
        /* four lanes' bytes as one LE dword in the lowest of them; lanes
         * behind the tail hold 0.  The branch is block-uniform, so every
         * lane takes part in the shuffles */
        const uint32_t w = x | (__shfl_down(x, 1, 64) << 8) |
                           (__shfl_down(x, 2, 64) << 16) |
                           (__shfl_down(x, 3, 64) << 24);
        if (tl < nt && (tl & 3) == 0) {
          uint8_t *q = dp + r0 + p; /* r0 + p is a multiple of 4 */
          if (tl + 4 <= nt) {
            *reinterpret_cast<uint32_t *>(q) = w;
          } else { /* the partial last dword of the shard */
#pragma unroll
            for (int b = 0; b < 3; b++)
              if (tl + b < nt) q[b] = uint8_t(w >> (8 * b));
          }
        }
      }
    }
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) part ^= __shfl_xor(part, sh, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
      const uint32_t itv =
          payload == int(payload_full)
              ? it_full
              : gf2_mulmod_d(x8n_d(uint64_t(payload)), 0xFFFFFFFFu);
      const uint32_t crc = ~(itv ^ red[0] ^ red[1] ^ red[2] ^ red[3]);
      *reinterpret_cast<uint32_t *>(db) = crc; /* the LE frame word */
      fcrc[fr] = crc;
      if (IMG) {
        const uint8_t *sb = pb - CRC_LEN;
        const uint32_t want = uint32_t(sb[0]) | (uint32_t(sb[1]) << 8) |
                              (uint32_t(sb[2]) << 16) |
                              (uint32_t(sb[3]) << 24);
        if (want != crc)
          atomicMin(&bad[item.job], static_cast<unsigned long long>(f));
      }
    }
    __syncthreads(); /* red is the next frame's too */
  }
}

void launch_shard_write_frame_queue(uint8_t *dst, uint64_t src,
                                    const gfrs_witem *items,
                                    const uint64_t *frame_prefix,
                                    uint32_t nitems, uint64_t total_frames,
                                    bool img, uint32_t *fcrc, int64_t *bad,
                                    hipStream_t s) {
  if (nitems == 0 || total_frames == 0) return;
  /* the cap of the other frame queues, read on every launch: GFRS_CRC_GRID
   * forces the multi-frame walk at tiny shapes */
  const uint64_t cap = uint64_t(env_grid("GFRS_CRC_GRID", 16384));
  const int grid = int(total_frames < cap ? total_frames : cap);
  /* waves per SIMD: 8; GFRS_SWR_WAVES = 4 or 8
   * overrides it and, like GFRS_SRD_WAVES, is read on every launch, so a test
   * can run both builds */
  const char *we = getenv("GFRS_SWR_WAVES");
  const int wv = we ? atoi(we) : 0;
  unsigned long long *ubad = reinterpret_cast<unsigned long long *>(bad);
#define GFRS_SWR_GO(IM, W)                                                  \
  hipLaunchKernelGGL((shard_write_frame_queue_k<IM, W>), dim3(grid),        \
                     dim3(CRC_BLOCKT), 0, s, dst, src, items, frame_prefix, \
                     nitems, total_frames, fcrc, ubad)
  if (img) {
    if (wv == 4) GFRS_SWR_GO(true, 4);
    else GFRS_SWR_GO(true, 8);
  } else {
    if (wv == 4) GFRS_SWR_GO(false, 4);
    else GFRS_SWR_GO(false, 8);
  }
#undef GFRS_SWR_GO
}

/* One wave per job, after the frame buckets on the same stream: write the new
 * 32-byte header (shard_finalize_queue_k's code, from the job), fold the job's
 * computed frame CRCs into the CRC of the whole payload - the operator of a
 * full frame once, another only for the last frame, the words loaded 64 to a
 * wave as in shard_head_queue_k - and write the footer.  For a SRC_IMAGE job
 * parse the source's header and footer by shard_head_queue_k's rules into the
 * status bits and the stored fields; a raw job reports its own ids and
 * status 0.  Geometry follows the job's size, never the source header's. */
__global__ void shard_write_head_queue_k(uint8_t *__restrict__ dst,
                                         uint64_t src,
                                         const gfrs_wjob *__restrict__ jobs,
                                         const uint64_t *__restrict__ job_frame,
                                         const uint32_t *__restrict__ fcrc,
                                         const int64_t *__restrict__ bad,
                                         gfrs_sresult *__restrict__ results,
                                         int njobs) {
  constexpr int64_t block_len = 65536;
  constexpr int64_t payload_full = block_len - CRC_LEN;
  const int j = blockIdx.x * (blockDim.x / 64) + (threadIdx.x / 64);
  const int lane = threadIdx.x & 63;
  if (j >= njobs) return; /* whole wave */
  /* every lane does the wave-uniform work below; lane 0 does the stores */
  const gfrs_wjob jb = jobs[j];
  uint8_t *img = dst + jb.img_off;
  const int64_t raw_size = int64_t(jb.size);
  const int64_t nframes = (raw_size + payload_full - 1) / payload_full;
  { /* the 32 B header (shard.go:241-261), big-endian fields */
    uint32_t w[8];
    w[1] = 0xccefcdabu; /* ab cd ef cc */
    w[2] = __builtin_bswap32(uint32_t(jb.bid >> 32));
    w[3] = __builtin_bswap32(uint32_t(jb.bid));
    w[4] = __builtin_bswap32(uint32_t(jb.vuid >> 32));
    w[5] = __builtin_bswap32(uint32_t(jb.vuid));
    w[6] = __builtin_bswap32(uint32_t(raw_size));
    w[7] = 0;
    uint32_t c = 0xFFFFFFFFu;
#pragma unroll
    for (int i = 1; i < 8; i++) {
      const uint32_t x = w[i];
#pragma unroll
      for (int b = 0; b < 4; b++)
        c = g_crc_tab4[0][(c ^ (x >> (8 * b))) & 0xFF] ^ (c >> 8);
    }
    w[0] = __builtin_bswap32(~c);
    uint32_t *d32 = reinterpret_cast<uint32_t *>(img);
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < 8; i++) d32[i] = w[i];
    }
  }
  uint32_t crc = 0;
  {
    const uint32_t *fc = fcrc + job_frame[j];
    const uint32_t op_full = x8n_d(uint64_t(payload_full));
    int64_t remain = raw_size;
    /* the fold is serial, its loads are not: 64 words per wave load */
    for (int64_t f0 = 0; f0 < nframes; f0 += 64) {
      const uint32_t mine = f0 + lane < nframes ? fc[f0 + lane] : 0;
      const int nf = int(nframes - f0 < 64 ? nframes - f0 : 64);
      for (int i = 0; i < nf; i++) {
        const uint32_t fcv = __shfl(mine, i, 64);
        const int64_t plen = remain < payload_full ? remain : payload_full;
        if (f0 + i == 0) {
          crc = fcv;
        } else {
          const uint32_t op =
              plen == payload_full ? op_full : x8n_d(uint64_t(plen));
          crc = gf2_mulmod_d(op, crc) ^ fcv;
        }
        remain -= plen;
      }
    }
  }
  const int64_t ftr_off = 32 + (raw_size + CRC_LEN * nframes);
  if (lane == 0) {
    uint8_t *ftr = img + ftr_off;
    ftr[0] = 0xcc; ftr[1] = 0xef; ftr[2] = 0xcd; ftr[3] = 0xab;
    ftr[4] = uint8_t(crc >> 24); ftr[5] = uint8_t(crc >> 16); /* BE */
    ftr[6] = uint8_t(crc >> 8); ftr[7] = uint8_t(crc);
  }
  gfrs_sresult r;
  r.status = 0;
  r.crc = crc;
  r.bad_block = -1;
  r.bid = jb.bid;
  r.vuid = jb.vuid;
  r.size = jb.size;
  if (jb.flags & GFRS_WJOB_SRC_IMAGE) { /* wave-uniform */
    const uint8_t *si = as_global(src + jb.src_off);
    uint32_t status = 0;
    if (!(si[4] == 0xab && si[5] == 0xcd && si[6] == 0xef && si[7] == 0xcc))
      status |= GFRS_SHARD_HDR_MAGIC;
    uint32_t hcrc = 0xFFFFFFFFu;
    for (int i = 4; i < 32; i++)
      hcrc = g_crc_tab4[0][(hcrc ^ si[i]) & 0xFF] ^ (hcrc >> 8);
    hcrc = ~hcrc;
    const uint32_t want_h = (uint32_t(si[0]) << 24) | (uint32_t(si[1]) << 16) |
                            (uint32_t(si[2]) << 8) | uint32_t(si[3]);
    if (want_h != hcrc) status |= GFRS_SHARD_HDR_CRC;
    uint64_t bid = 0, vuid = 0;
    for (int i = 0; i < 8; i++) bid = (bid << 8) | si[8 + i];
    for (int i = 0; i < 8; i++) vuid = (vuid << 8) | si[16 + i];
    const uint64_t size = (uint64_t(si[24]) << 24) | (uint64_t(si[25]) << 16) |
                          (uint64_t(si[26]) << 8) | uint64_t(si[27]);
    if (bid != jb.src_bid || vuid != jb.src_vuid || size != jb.size)
      status |= GFRS_SHARD_HDR_MISMATCH;
    const int64_t bb = bad[j];
    if (bb != -1) status |= GFRS_SHARD_BODY_CRC;
    const uint8_t *ftr = si + ftr_off;
    if (!(ftr[0] == 0xcc && ftr[1] == 0xef && ftr[2] == 0xcd &&
          ftr[3] == 0xab))
      status |= GFRS_SHARD_FTR_MAGIC;
    const uint32_t want_f = (uint32_t(ftr[4]) << 24) |
                            (uint32_t(ftr[5]) << 16) |
                            (uint32_t(ftr[6]) << 8) | uint32_t(ftr[7]);
    if (want_f != crc) status |= GFRS_SHARD_FTR_CRC;
    r.status = status;
    r.bad_block = bb;
    r.bid = bid;
    r.vuid = vuid;
    r.size = size;
  }
  if (lane == 0) results[j] = r;
}

void launch_shard_write_head_queue(uint8_t *dst, uint64_t src,
                                   const gfrs_wjob *jobs,
                                   const uint64_t *job_frame,
                                   const uint32_t *fcrc, const int64_t *bad,
                                   gfrs_sresult *results, int njobs,
                                   hipStream_t s) {
  if (njobs <= 0) return;
  const int wps = 4; /* waves per block */
  const int blocks = (njobs + wps - 1) / wps;
  hipLaunchKernelGGL(shard_write_head_queue_k, dim3(blocks), dim3(wps * 64), 0,
                     s, dst, src, jobs, job_frame, fcrc, bad, results, njobs);
}

/* Host-side one-time init of the device CRC tables (g_crc_tab4, g_pow8)
 * for the CURRENT device.  Called by gfrs_host.cpp under its device mutex. */
int crc_device_init_current(void) {
  uint32_t tab[8][256];
  for (uint32_t i = 0; i < 256; i++) {
    uint32_t c = i;
    for (int j = 0; j < 8; j++) c = (c & 1) ? (c >> 1) ^ CRC_POLY : c >> 1;
    tab[0][i] = c;
  }
  for (int t = 1; t < 8; t++)
    for (int i = 0; i < 256; i++)
      tab[t][i] = tab[0][tab[t - 1][i] & 0xFF] ^ (tab[t - 1][i] >> 8);
  /* x^(8*2^j) mod P, reflected (identity = 0x80000000) */
  auto mulmod = [](uint32_t a, uint32_t b) {
    uint32_t prod = 0;
    for (int i = 31; i >= 0; i--) {
      if ((a >> i) & 1) prod ^= b;
      b = (b & 1) ? (b >> 1) ^ CRC_POLY : (b >> 1);
    }
    return prod;
  };
  uint32_t pow8[40];
  uint32_t p = 0x00800000u; /* x^8 reflected */
  for (int j = 0; j < 40; j++) {
    pow8[j] = p;
    p = mulmod(p, p);
  }
  /* g_shift4k[j][b] = x^(8*4096) * (b << 8j): mulmod is GF(2)-linear in
   * its second argument, so XORing the four byte-slice lookups of a value
   * multiplies the whole value by x^(8*4096).  pow8[12] = x^(8*2^12). */
  uint32_t s4k[4][256];
  for (int j = 0; j < 4; j++)
    for (uint32_t b = 0; b < 256; b++)
      s4k[j][b] = mulmod(pow8[12], b << (8 * j));
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_shift4k), s4k, sizeof(s4k)) != hipSuccess)
    return -100;
  for (int j = 0; j < 4; j++)
    for (uint32_t b = 0; b < 256; b++)
      s4k[j][b] = mulmod(pow8[10], b << (8 * j)); /* x^(8*2^10) */
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_shift1k), s4k, sizeof(s4k)) != hipSuccess)
    return -100;
  for (int j = 0; j < 4; j++)
    for (uint32_t b = 0; b < 256; b++)
      s4k[j][b] = mulmod(pow8[13], b << (8 * j)); /* x^(8*2^13) */
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_shift8k), s4k, sizeof(s4k)) != hipSuccess)
    return -100;
  /* 13312 = 2^13 + 2^12 + 2^10 */
  const uint32_t x13k = mulmod(mulmod(pow8[13], pow8[12]), pow8[10]);
  for (int j = 0; j < 4; j++)
    for (uint32_t b = 0; b < 256; b++)
      s4k[j][b] = mulmod(x13k, b << (8 * j));
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_shift13k), s4k, sizeof(s4k)) != hipSuccess)
    return -100;
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_crc_tab4), tab, sizeof(tab)) != hipSuccess)
    return -100;
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_pow8), pow8, sizeof(pow8)) != hipSuccess)
    return -100;
  return 0;
}

void launch_crc_encode(uint8_t *dst, size_t dst_stride, const uint8_t *src,
                       size_t src_stride, int64_t n, int64_t block_len,
                       int nshards, hipStream_t s) {
  const int64_t payload = block_len - CRC_LEN;
  const int64_t fps = (n + payload - 1) / payload;
  crc_dispatch<0>(dst, dst_stride, src, src_stride, n, block_len, fps,
                  fps * nshards, nullptr, s);
}

void launch_crc_verify(const uint8_t *framed, size_t stride,
                       int64_t framed_len, int64_t block_len, int nshards,
                       int64_t *bad, hipStream_t s) {
  const int64_t fps = (framed_len + block_len - 1) / block_len;
  const int64_t n = framed_len - CRC_LEN * fps; /* raw payload total */
  crc_dispatch<1>(nullptr, 0, framed, stride, n, block_len, fps,
                  fps * nshards, bad, s);
}

void launch_crc_decode(uint8_t *dst, size_t dst_stride, const uint8_t *framed,
                       size_t src_stride, int64_t framed_len,
                       int64_t block_len, int nshards, int64_t *bad,
                       hipStream_t s) {
  const int64_t fps = (framed_len + block_len - 1) / block_len;
  const int64_t n = framed_len - CRC_LEN * fps;
  crc_dispatch<2>(dst, dst_stride, framed, src_stride, n, block_len, fps,
                  fps * nshards, bad, s);
}

}  // namespace gfrs
