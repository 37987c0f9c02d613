/* cubefs_amd/csrc/gfrs_host.cpp — C-ABI host runtime of the MI355X EC/CRC
 * engine (include/gfrs.h).
 *
 * Mirrors the blobstore/common/ec host semantics:
 *   ec.NewEncoder / encoder / lrcEncoder     (encoder.go:78-112, lrcencoder.go)
 *   Encode / Verify / Reconstruct[Data]      (encoder.go:114-151)
 *   LRC layering: global RS(n,m) + per-AZ RS((n+m)/az, l/az)
 *                                            (lrcencoder.go:35-82,133-207)
 *   inversionTree decode-matrix cache keyed by the missing-index set
 *                                            (inversion_tree.go:16-164) —
 *                                            here a bitmask-keyed map
 *   codemode local stripe layout             (codemode.go:301-318)
 *
 * Which coefficients multiply which shards is decided in gfrs_plan.cpp
 * (host-only, testable without a device); this file caches and uploads
 * those plans, stages memory, picks the kernel for a shape and launches.
 *
 * GPU-only by design: no CPU compute fallback exists.  When no HIP device
 * is visible every compute call fails with GFRS_ERR_NO_GPU.
 */
#include "../../include/gfrs.h"
#include "gfrs_internal.h"

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <algorithm>
#include <array>
#include <atomic>
#include <memory>
#include <vector>

namespace gfrs {

/* 256-bit shard bitmask + tag: collision-free plan-cache key for every
 * engine tactic_valid admits (n+m <= 256). */
typedef std::array<uint64_t, 5> PlanKey;

static inline PlanKey plan_key_tag(uint64_t tag) {
  PlanKey k{};
  k[4] = tag;
  return k;
}

static inline void plan_key_set(PlanKey &k, int i) {
  k[size_t(i) >> 6] |= 1ull << (unsigned(i) & 63u);
}

static inline bool plan_key_test(const PlanKey &k, int i) {
  return (k[size_t(i) >> 6] >> (unsigned(i) & 63u)) & 1u;
}

static thread_local std::string g_err;

static void seterr(const char *fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
}

static int hip_fail(const char *what, hipError_t e) {
  seterr("%s: %s", what, hipGetErrorString(e));
  return GFRS_ERR_HIP;
}

#define HIP_TRY(call)                                    \
  do {                                                   \
    hipError_t e_ = (call);                              \
    if (e_ != hipSuccess) return hip_fail(#call, e_);    \
  } while (0)

/* per-device one-time CRC table init */
static std::mutex g_dev_mu;
static std::set<int> g_dev_inited;

static int ensure_device_init(int device) {
  std::lock_guard<std::mutex> lk(g_dev_mu);
  if (g_dev_inited.count(device)) return GFRS_OK;
  HIP_TRY(hipSetDevice(device));
  int rc = crc_device_init_current();
  if (rc != 0) {
    seterr("crc_device_init_current failed");
    return GFRS_ERR_HIP;
  }
  g_dev_inited.insert(device);
  return GFRS_OK;
}

/* Grow-only device buffer. */
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  int ensure(size_t n) {
    if (n <= cap) return GFRS_OK;
    if (p) hipFree(p);
    p = nullptr;
    cap = 0;
    HIP_TRY(hipMalloc(&p, n));
    cap = n;
    return GFRS_OK;
  }
  ~DevBuf() {
    if (p) hipFree(p);
  }
};

struct PinBuf {
  void *p = nullptr;
  size_t cap = 0;
  int ensure(size_t n) {
    if (n <= cap) return GFRS_OK;
    if (p) hipHostFree(p);
    p = nullptr;
    cap = 0;
    HIP_TRY(hipHostMalloc(&p, n));
    cap = n;
    return GFRS_OK;
  }
  ~PinBuf() {
    if (p) hipHostFree(p);
  }
};

/* An uploaded coding plan: index lists + per-coefficient tables. */
struct DevPlan {
  DevBuf in_idx, out_idx, tabs;
  int k = 0, nout = 0; /* row width (in_idx may carry extra cmp indices
                          after the first k inputs), output rows */
  uint32_t cmp_mask = 0;
  const int32_t *in() const { return (const int32_t *)in_idx.p; }
  const int32_t *out() const { return (const int32_t *)out_idx.p; }
  const uint8_t *tab() const { return (const uint8_t *)tabs.p; }
  int upload(const Plan &pl, hipStream_t s) {
    const GfTables &t = gft();
    k = pl.rowk;
    nout = int(pl.out.size());
    cmp_mask = pl.cmp_mask;
    /* 3-way linear-split tables, 32 B per coefficient (A8|B8|C4|pad):
     * GF(2^8) multiply-by-constant is GF(2)-linear, so mul_c(b) =
     * A[b&7] ^ B[(b>>3)&7] ^ C[b>>6] with A[i]=mul(c,i), B[i]=mul(c,8i),
     * C[i]=mul(c,64i).  Every kernel looks a packed dword up as
     * 3 v_perm + xor3 (+xor into acc) with selectors shared across
     * output rows — measured ~25% fewer VALU than the lo|hi nibble
     * form's 4 v_perm + 2 blends + 2 mask broadcasts. */
    std::vector<uint8_t> tb(size_t(nout) * k * 32, 0);
    for (int r = 0; r < nout; r++)
      for (int c = 0; c < k; c++) {
        uint8_t coef = pl.rows[size_t(r) * k + c];
        uint8_t *lt = &tb[(size_t(r) * k + c) * 32];
        for (int i = 0; i < 8; i++) {
          lt[i] = t.mul[coef][i];
          lt[8 + i] = t.mul[coef][8 * i];
        }
        for (int i = 0; i < 4; i++) lt[16 + i] = t.mul[coef][64 * i];
      }
    int rc;
    if ((rc = in_idx.ensure(pl.in.size() * 4)) != GFRS_OK) return rc;
    if ((rc = out_idx.ensure(pl.out.size() * 4)) != GFRS_OK) return rc;
    if ((rc = tabs.ensure(tb.size())) != GFRS_OK) return rc;
    HIP_TRY(hipMemcpyAsync(in_idx.p, pl.in.data(), pl.in.size() * 4,
                           hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(out_idx.p, pl.out.data(), pl.out.size() * 4,
                           hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(tabs.p, tb.data(), tb.size(),
                           hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s)); /* plans are built once, reused many times */
    return GFRS_OK;
  }
};

typedef std::map<PlanKey, DevPlan *> PlanCache;

/* One independent execution lane: own stream + own scratch, so
 * concurrent single-stripe callers on one context (the reference shares
 * one ec.Encoder across ~100 goroutines behind a counting semaphore,
 * encoder.go:29,115) issue to the GPU in parallel instead of
 * serializing on one stream. */
struct Lane {
  hipStream_t stream = nullptr;
  DevBuf ptr_buf, fail_buf, stage_dev;
  PinBuf stage_pin;
  std::mutex mu;
  ~Lane() {
    if (stream) hipStreamDestroy(stream);
  }
};

struct gfrs_ctx_impl;

/* view over either a lane's or the context's stream+scratch; owner is the
 * context when the scratch is the context's own (pin_for_write), nullptr
 * for a lane */
struct LaneView {
  hipStream_t stream;
  DevBuf *ptr_buf, *fail_buf, *stage_dev;
  PinBuf *stage_pin;
  gfrs_ctx_impl *owner;
};

struct gfrs_ctx_impl {
  Code code; /* tactic + encode matrices (gfrs_plan.h) */
  int device = 0;
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  std::mutex mu;

  DevPlan enc_plan;                  /* global encode */
  std::vector<DevPlan *> local_enc;  /* per-AZ local encode (global idx) */
  DevPlan local_plan;                /* local engine, identity idx (one
                                        local-stripe set, lrcencoder.go:94) */
  DevPlan fused_lrc;                 /* m+l output rows composed over the
                                        n data shards (locals are linear in
                                        the data through the parity rows) */
  bool fused_lrc_ok = false;
  /* Plan-cache key: full 256-bit missing/present bitmask (words 0..3) plus
   * an engine/namespace tag (word 4).  tactic_valid admits engines up to
   * n+m=256 shards, so a packed-u64 key would silently collide distinct
   * missing sets above 58 shards (and 1ull<<i is UB at i>=64); the wide
   * key makes every reachable engine collision-free. */
  PlanCache dec_cache; /* missing-bitmask → data decode (engine tags 1,
                          2+az, 50) and the bad-set namespaces 60-63 */
  PlanCache par_cache; /* missing-bitmask → parity rows */

  DevBuf ptr_buf;   /* pointer tables for pointer-mode launches */
  DevBuf fail_buf;  /* verify flags / crc bad blocks */
  DevBuf stage_dev; /* host-mode staging */
  PinBuf stage_pin;
  DevBuf queue_buf; /* repair queue: pattern descriptors, work items, tile
                       prefix sums of one call */
  DevBuf repair_buf; /* repair-image queue: descriptors, work items, frame
                        prefix sums, image table of one call */
  DevBuf encq_buf; /* encode+frame queue: work items, frame prefix sums of
                      one call */
  PinBuf encq_pin; /* ... and the pinned host copy it is uploaded from */
  DevBuf readq_buf; /* read queue: descriptors, identity indices, work items,
                       frame prefix sums of one call */
  PinBuf readq_pin; /* ... and the pinned host copy it is uploaded from */
  DevBuf shardq_buf; /* shard read queue: work items, frame prefix sums, jobs,
                        their first-frame places and bad blocks of one call
                        (the uploaded blob), then the computed frame CRCs and
                        the results */
  DevBuf shardwq_buf; /* shard write queue: the same, with the write queue's
                         items and jobs */
  DevBuf putq_buf; /* put queue: work items, frame prefix sums and image table
                      of one call (the uploaded blob), then the image CRCs */
  DevPlan put_lrc; /* put queue, LRC tactics outside lrc_single_pass: the
                      plan_fused_lrc rows, uploaded by the first put call
                      (fused_lrc, and every gate that reads fused_lrc_ok, stay
                      as they are) */
  bool put_lrc_ok = false;
  DevBuf read_scratch; /* read queue, slow jobs: one decoded stripe of the
                          touched frames; grown on demand, freed with the
                          context */

  /* finalize-pipeline resources (repair path): shard_finalize of chunk i
   * runs on aux_stream behind an event while chunk i+1's repair kernel
   * streams on the main stream */
  hipStream_t aux_stream = nullptr;
  hipEvent_t aux_ev[2] = {nullptr, nullptr};
  hipEvent_t aux_done = nullptr;
  int ensure_aux() {
    if (aux_stream) return GFRS_OK;
    if (hipStreamCreateWithFlags(&aux_stream, hipStreamNonBlocking) !=
        hipSuccess)
      return GFRS_ERR_HIP;
    for (int i = 0; i < 2; i++)
      if (hipEventCreateWithFlags(&aux_ev[i], hipEventDisableTiming) !=
          hipSuccess)
        return GFRS_ERR_HIP;
    if (hipEventCreateWithFlags(&aux_done, hipEventDisableTiming) !=
        hipSuccess)
      return GFRS_ERR_HIP;
    return GFRS_OK;
  }

  /* gfrs_shard_write_batch returns with its id upload out of stage_pin
   * still queued; no later call may write stage_pin (or free it to grow
   * it) before that copy ran.  pin_ev is recorded behind the copy and
   * pin_for_write waits it out.  Every other call that uploads from
   * stage_pin synchronizes its stream before it returns. */
  hipEvent_t pin_ev = nullptr;
  bool pin_pending = false;

  /* stream-lane pool for concurrent foreground (single-stripe) calls;
   * empty when GFRS_LANES=0 or after gfrs_set_stream pins a caller
   * stream (user_stream) */
  std::vector<std::unique_ptr<Lane>> lanes;
  std::atomic<uint32_t> lane_rr{0};
  bool user_stream = false;
  std::mutex cache_mu; /* plan caches (dec/par) — lanes bypass this->mu */

  Lane *pick_lane() {
    if (user_stream || lanes.empty()) return nullptr;
    return lanes[lane_rr.fetch_add(1) % lanes.size()].get();
  }

  ~gfrs_ctx_impl() {
    for (auto *p : local_enc) delete p;
    for (auto &kv : dec_cache) delete kv.second;
    for (auto &kv : par_cache) delete kv.second;
    if (own_stream) hipStreamDestroy(own_stream);
    if (aux_stream) hipStreamDestroy(aux_stream);
    for (int i = 0; i < 2; i++)
      if (aux_ev[i]) hipEventDestroy(aux_ev[i]);
    if (aux_done) hipEventDestroy(aux_done);
    if (pin_ev) hipEventDestroy(pin_ev);
  }
};

struct StreamGuard {
  int prev = -1;
  explicit StreamGuard(const gfrs_ctx_impl *c) {
    hipGetDevice(&prev);
    hipSetDevice(c->device);
  }
  ~StreamGuard() {
    if (prev >= 0) hipSetDevice(prev);
  }
};

static inline LaneView view_of(gfrs_ctx_impl *c) {
  return LaneView{c->stream, &c->ptr_buf, &c->fail_buf, &c->stage_dev,
                  &c->stage_pin, c};
}
static inline LaneView view_of(Lane *L) {
  return LaneView{L->stream, &L->ptr_buf, &L->fail_buf, &L->stage_dev,
                  &L->stage_pin, nullptr};
}

/* The plans a context keeps for its lifetime: global encode, per-AZ local
 * encode, the local engine with identity indices, and (where the fused
 * kernels serve the tactic) the composed LRC encode. */
static bool upload_fixed_plans(gfrs_ctx_impl *c) {
  const Code &cd = c->code;
  const gfrs_tactic &t = cd.t;
  bool ok = true;
  /* an engine's encode plan is its parity plan with every parity missing */
  auto encode_plan = [&](int k, int m, const std::vector<uint8_t> &matrix,
                         const std::vector<int32_t> &idx, DevPlan *dp) {
    std::vector<uint8_t> present(k + m, 0);
    std::fill_n(present.begin(), k, 1);
    Plan pl;
    plan_parity(Engine{k, m, matrix.data(), idx.data()}, present.data(), &pl);
    return dp->upload(pl, c->stream) == GFRS_OK;
  };
  std::vector<int32_t> ident(256);
  for (int i = 0; i < 256; i++) ident[i] = i;
  if (ok && t.m > 0)
    ok = encode_plan(t.n, t.m, cd.enc_matrix, ident, &c->enc_plan);
  if (ok && t.l > 0) {
    for (int az = 0; az < t.az_count && ok; az++) {
      c->local_enc.push_back(new DevPlan());
      ok = encode_plan(cd.local_n, cd.local_m, cd.local_matrix,
                       local_stripe(t, az), c->local_enc.back());
    }
    if (ok) /* one local-stripe set, identity indices */
      ok = encode_plan(cd.local_n, cd.local_m, cd.local_matrix, ident,
                       &c->local_plan);
    if (ok && lrc_single_pass(cd)) {
      Plan pl;
      plan_fused_lrc(cd, &pl);
      ok = c->fused_lrc.upload(pl, c->stream) == GFRS_OK;
      c->fused_lrc_ok = ok;
    }
  }
  return ok;
}

}  // namespace gfrs

using namespace gfrs;

/* unlocked bodies of the public batch entry points (defined below);
 * already-locked callers reuse these instead of re-locking */
static int encode_batch_impl(gfrs_ctx_impl *c, void *base, size_t shard_len,
                             size_t stripe_stride, int nstripes,
                             hipStream_t st);
static int verify_batch_impl(gfrs_ctx_impl *c, const void *base,
                             size_t shard_len, size_t stripe_stride,
                             int nstripes, uint64_t *fail_bitmap,
                             hipStream_t st, DevBuf *fail);
static int crc32b_encode_batch_impl(gfrs_ctx_impl *c, void *dst,
                                    size_t dst_stride, const void *src,
                                    size_t src_stride, int64_t n,
                                    int64_t block_len, int nshards);

extern "C" {

const char *gfrs_last_error(void) { return g_err.c_str(); }
const char *gfrs_version(void) { return "gfrs 0.1.0 (gfx950)"; }

int gfrs_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int gfrs_buffer_sizes(const gfrs_tactic *t, int64_t data_size,
                      int64_t *shard_size, int64_t *ec_data_size,
                      int64_t *ec_size) {
  /* buf.go:67-133 */
  if (!t || t->n <= 0) return GFRS_ERR_INVALID_CODEMODE;
  if (data_size <= 0) return GFRS_ERR_SHORT_DATA;
  int64_t ss = (data_size + t->n - 1) / t->n;
  if (ss < t->min_shard_size) ss = t->min_shard_size;
  *shard_size = ss;
  *ec_data_size = ss * t->n;
  *ec_size = ss * (t->n + t->m + t->l);
  return GFRS_OK;
}

gfrs_ctx *gfrs_create(const gfrs_tactic *t, int device) {
  if (!tactic_valid(t)) {
    seterr("invalid code mode tactic");
    return nullptr;
  }
  int ndev = gfrs_device_count();
  if (ndev == 0) {
    seterr("no HIP device visible (the gfrs engine has no CPU fallback)");
    return nullptr;
  }
  if (device < 0) hipGetDevice(&device);
  if (device >= ndev) {
    seterr("device %d out of range (%d visible)", device, ndev);
    return nullptr;
  }
  if (ensure_device_init(device) != GFRS_OK) return nullptr;

  auto *c = new gfrs_ctx_impl();
  c->device = device;

  int prev = -1;
  hipGetDevice(&prev);
  hipSetDevice(device);
  bool ok = hipStreamCreate(&c->own_stream) == hipSuccess;
  c->stream = c->own_stream;
  if (ok) {
    const char *le = getenv("GFRS_LANES");
    int nl = le ? atoi(le) : 4;
    if (nl < 0) nl = 0;
    if (nl > 16) nl = 16;
    for (int i = 0; i < nl && ok; i++) {
      auto L = std::make_unique<Lane>();
      ok = hipStreamCreate(&L->stream) == hipSuccess;
      if (ok) c->lanes.push_back(std::move(L));
    }
  }

  ok = ok && code_build(*t, &c->code) && upload_fixed_plans(c);
  if (prev >= 0) hipSetDevice(prev);
  if (!ok) {
    seterr("gfrs_create: init failed (%s)", g_err.c_str());
    delete c;
    return nullptr;
  }
  return reinterpret_cast<gfrs_ctx *>(c);
}

void gfrs_destroy(gfrs_ctx *ctx) { delete reinterpret_cast<gfrs_ctx_impl *>(ctx); }

int gfrs_set_stream(gfrs_ctx *ctx, void *hip_stream) {
  auto *c = reinterpret_cast<gfrs_ctx_impl *>(ctx);
  std::lock_guard<std::mutex> lk(c->mu);
  hipStream_t next = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream)
                                : c->own_stream;
  if (next != c->stream) {
    /* the async batch calls leave work queued that reads the context's
     * scratch (ptr_buf, the plans); the next stream is not ordered against
     * it, so drain it here - this is not a hot call.  A caller stream that
     * has been destroyed meanwhile has nothing queued: its error is
     * dropped. */
    StreamGuard g(c);
    if (hipStreamSynchronize(c->stream) != hipSuccess) (void)hipGetLastError();
    c->pin_pending = false;
  }
  c->stream = next;
  /* a caller-pinned stream implies caller-managed ordering: foreground
   * calls then issue on that one stream instead of fanning out */
  c->user_stream = hip_stream != nullptr;
  return GFRS_OK;
}

int gfrs_synchronize(gfrs_ctx *ctx) {
  auto *c = reinterpret_cast<gfrs_ctx_impl *>(ctx);
  StreamGuard g(c);
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (auto &L : c->lanes) HIP_TRY(hipStreamSynchronize(L->stream));
  return GFRS_OK;
}

int gfrs_encode_matrix(gfrs_ctx *ctx, uint8_t *out) {
  auto *c = reinterpret_cast<gfrs_ctx_impl *>(ctx);
  memcpy(out, c->code.enc_matrix.data(), c->code.enc_matrix.size());
  return GFRS_OK;
}

int gfrs_compute_encode_matrix(int k, int total, uint8_t *out) {
  if (!gf_build_matrix(k, total, out)) {
    seterr("encode matrix build failed (k=%d total=%d)", k, total);
    return GFRS_ERR_SINGULAR;
  }
  return GFRS_OK;
}

int gfrs_probe_perm(void) {
  if (gfrs_device_count() == 0) return GFRS_ERR_NO_GPU;
  return probe_perm_device();
}

}  /* extern "C" (continued in this file below) */

/* ---------------- internal helpers for the compute entry points ------- */

namespace gfrs {

/* The one way the host gets to write a view's pinned staging: n bytes of
 * it, after any upload out of it that an earlier call left queued has run.
 * Device-side scratch reuse is ordered by the stream; the host's writes to
 * the staging are ordered by nothing but this wait (it also precedes the
 * free that grows the buffer).  Nothing pending - the usual case - costs
 * one flag test; a lane's staging is never left pending (owner == nullptr),
 * every lane call syncs its stream under the lane mutex. */
static int pin_for_write(const LaneView &lv, size_t n, uint8_t **pin) {
  gfrs_ctx_impl *c = lv.owner;
  if (c && c->pin_pending) {
    HIP_TRY(hipEventSynchronize(c->pin_ev));
    c->pin_pending = false;
  }
  int rc = lv.stage_pin->ensure(n);
  if (rc != GFRS_OK) return rc;
  *pin = (uint8_t *)lv.stage_pin->p;
  return GFRS_OK;
}

/* Upload a pointer table for pointer-mode launches (stream-ordered, so
 * reuse of the scratch buffer is safe across calls on one stream). */
static int upload_ptrs(const LaneView &lv, void *const *shards, int nshards) {
  int rc = lv.ptr_buf->ensure(size_t(nshards) * 8);
  if (rc != GFRS_OK) return rc;
  /* small, use pinned staging for async copy */
  uint8_t *pin;
  if ((rc = pin_for_write(lv, size_t(nshards) * 8, &pin)) != GFRS_OK) return rc;
  memcpy(pin, shards, size_t(nshards) * 8);
  HIP_TRY(hipMemcpyAsync(lv.ptr_buf->p, lv.stage_pin->p, size_t(nshards) * 8,
                         hipMemcpyHostToDevice, lv.stream));
  return GFRS_OK;
}

/* Stage a host stripe: pin, gather the first ncopy shards that are present
 * (present == nullptr: all), H2D those ncopy shards.  The device and pinned
 * images hold nshards shards (+ dev_slack device bytes); what is copied
 * back, and when, is the caller's rule. */
static int stage_host_stripe(const LaneView &lv, void *const *shards,
                             int nshards, int ncopy, const uint8_t *present,
                             size_t shard_len, size_t dev_slack = 0) {
  const size_t tot = size_t(nshards) * shard_len;
  int rc;
  if ((rc = lv.stage_dev->ensure(tot + dev_slack)) != GFRS_OK) return rc;
  uint8_t *pin;
  if ((rc = pin_for_write(lv, tot, &pin)) != GFRS_OK) return rc;
  for (int i = 0; i < ncopy; i++)
    if (!present || present[i])
      memcpy(pin + size_t(i) * shard_len, shards[i], shard_len);
  HIP_TRY(hipMemcpyAsync(lv.stage_dev->p, pin, size_t(ncopy) * shard_len,
                         hipMemcpyHostToDevice, lv.stream));
  return GFRS_OK;
}

/* Stage n bids then n vuids into c->ptr_buf (stream-ordered scratch reuse)
 * through the pinned staging.  gfrs_shard_write_batch returns with this
 * upload still queued (pin_pending). */
static int stage_ids(gfrs_ctx_impl *c, const uint64_t *bids,
                     const uint64_t *vuids, size_t n) {
  const size_t idbytes = n * 8;
  int rc;
  uint8_t *pin;
  if ((rc = pin_for_write(view_of(c), idbytes * 2, &pin)) != GFRS_OK) return rc;
  memcpy(pin, bids, idbytes);
  memcpy(pin + idbytes, vuids, idbytes);
  if ((rc = c->ptr_buf.ensure(idbytes * 2)) != GFRS_OK) return rc;
  HIP_TRY(hipMemcpyAsync(c->ptr_buf.p, c->stage_pin.p, idbytes * 2,
                         hipMemcpyHostToDevice, c->stream));
  return GFRS_OK;
}

/* Per-stripe fail words: begin clears them ahead of the launches ... */
static int fail_begin(DevBuf *fail, int nstripes, hipStream_t s) {
  int rc = fail->ensure(size_t(nstripes) * 4);
  if (rc != GFRS_OK) return rc;
  HIP_TRY(hipMemsetAsync(fail->p, 0, size_t(nstripes) * 4, s));
  return GFRS_OK;
}

/* ... finish reads them back, syncs the stream and packs them: one bit per
 * stripe into fail_bitmap and/or one flag for the whole call into ok. */
static int fail_finish(DevBuf *fail, int nstripes, hipStream_t s,
                       uint64_t *fail_bitmap, int *ok = nullptr) {
  uint32_t one = 0; /* the single-stripe calls stay off the heap */
  std::vector<uint32_t> many(nstripes > 1 ? nstripes : 0);
  uint32_t *fails = nstripes > 1 ? many.data() : &one;
  HIP_TRY(hipMemcpyAsync(fails, fail->p, size_t(nstripes) * 4,
                         hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (fail_bitmap) memset(fail_bitmap, 0, ((nstripes + 63) / 64) * 8);
  if (ok) *ok = 1;
  for (int i = 0; i < nstripes; i++)
    if (fails[i]) {
      if (fail_bitmap) fail_bitmap[i / 64] |= 1ull << (i % 64);
      if (ok) *ok = 0;
    }
  return GFRS_OK;
}

/* Where a launch finds its shards: a pointer table (nptr > 0: nptr
 * pointers per stripe) or a strided batch (stripe s shard i at
 * base + s*stride + i*shard_len). */
struct Shards {
  const uint64_t *ptrs;
  int nptr;
  uint64_t base, stride;
};
static inline Shards table_of(const LaneView &lv, int nptr) {
  return Shards{(const uint64_t *)lv.ptr_buf->p, nptr, 0, 0};
}
static inline Shards strided(const void *base, size_t stride) {
  return Shards{nullptr, 0, (uint64_t)base, stride};
}

enum PlanOp {
  OP_APPLY,  /* out = rows x in */
  OP_VERIFY, /* compare every row, OR into fail[s] */
  OP_XOR,    /* out ^= rows x in (pointer tables only) */
  OP_MIXED,  /* write or compare per p.cmp_mask (strided only) */
};

/* The one way a plan reaches a kernel. */
static void run_plan(PlanOp op, const DevPlan &p, const Shards &sh,
                     size_t shard_len, int nstripes, hipStream_t s,
                     uint32_t *fail = nullptr) {
  const bool tab = sh.nptr > 0;
  switch (op) {
    case OP_APPLY:
      if (tab)
        launch_rs_apply(sh.ptrs, sh.nptr, p.in(), p.k, p.out(), p.nout,
                        p.tab(), shard_len, nstripes, s);
      else
        launch_rs_apply_strided(sh.base, sh.stride, p.in(), p.k, p.out(),
                                p.nout, p.tab(), shard_len, nstripes, s);
      break;
    case OP_VERIFY:
      if (tab)
        launch_rs_verify(sh.ptrs, sh.nptr, p.in(), p.k, p.out(), p.nout,
                         p.tab(), shard_len, nstripes, fail, s);
      else
        launch_rs_verify_strided(sh.base, sh.stride, p.in(), p.k, p.out(),
                                 p.nout, p.tab(), shard_len, nstripes, fail,
                                 s);
      break;
    case OP_XOR:
      launch_rs_apply_xor(sh.ptrs, sh.nptr, p.in(), p.k, p.out(), p.nout,
                          p.tab(), shard_len, nstripes, s);
      break;
    case OP_MIXED:
      launch_rs_apply_mixed_strided(sh.base, sh.stride, p.in(), p.k, p.out(),
                                    p.nout, p.tab(), p.cmp_mask, shard_len,
                                    nstripes, fail, s);
      break;
  }
}

/* global encode / verify: the global plan, then every AZ's local plan */
static void run_encode_plans(PlanOp op, const gfrs_ctx_impl *c,
                             const Shards &sh, size_t shard_len, int nstripes,
                             hipStream_t s, uint32_t *fail = nullptr) {
  run_plan(op, c->enc_plan, sh, shard_len, nstripes, s, fail);
  for (auto *lp : c->local_enc)
    run_plan(op, *lp, sh, shard_len, nstripes, s, fail);
}

/* Find the plan cached under `key`, or build, upload and insert it.
 * cache_mu is held throughout (lanes look plans up concurrently and bypass
 * c->mu); the build itself runs under the context or lane mutex the caller
 * already holds.  A hit costs the one lock and the map lookup.  A builder
 * that leaves `out` empty has nothing to do: *out = nullptr, not cached.
 * Pass the builder as std::ref(lambda) so that no closure is copied. */
static int cached_plan(gfrs_ctx_impl *c, PlanCache &cache, const PlanKey &key,
                       hipStream_t s,
                       const std::function<int(Plan *)> &build,
                       DevPlan **out) {
  std::lock_guard<std::mutex> cache_lk(c->cache_mu);
  auto it = cache.find(key);
  if (it != cache.end()) {
    *out = it->second;
    return GFRS_OK;
  }
  Plan pl;
  int rc = build(&pl);
  if (rc != GFRS_OK) return rc;
  *out = nullptr;
  if (pl.out.empty()) return GFRS_OK;
  auto p = std::make_unique<DevPlan>();
  if ((rc = p->upload(pl, s)) != GFRS_OK) return rc;
  *out = cache[key] = p.release();
  return GFRS_OK;
}

/* Key of a bad list in namespace `tag`; refuses out-of-range indices and,
 * unless dup_ok, duplicates (a duplicate would alias the key of the set
 * without it, whose plan has fewer write rows). */
static int bad_list_key(uint64_t tag, const int32_t *bad, int nbad, int total,
                        bool dup_ok, PlanKey *key) {
  *key = plan_key_tag(tag);
  for (int i = 0; i < nbad; i++) {
    if (bad[i] < 0 || bad[i] >= total) return GFRS_ERR_INVALID_SHARDS;
    if (!dup_ok && plan_key_test(*key, bad[i])) return GFRS_ERR_INVALID_SHARDS;
    plan_key_set(*key, bad[i]);
  }
  return GFRS_OK;
}

/* Run one engine's reconstruct: decode plan for the missing data (mirrors
 * the inversion_tree cache), then parity plan for the missing parities.
 * present covers the engine's k+m shards. */
static int reconstruct_engine(gfrs_ctx_impl *c, const LaneView &lv,
                              const Engine &e,
                              const std::vector<uint8_t> &present,
                              size_t shard_len, int nstripes, int data_only,
                              const Shards &sh, int tag) {
  const int k = e.k, m = e.m;
  int npresent = 0, dpresent = 0;
  for (int i = 0; i < k + m; i++)
    if (present[i]) {
      npresent++;
      if (i < k) dpresent++;
    }
  if (npresent == k + m || (data_only && dpresent == k)) return GFRS_OK;
  if (npresent < k) return GFRS_ERR_TOO_FEW_SHARDS;

  /* key = missing bitmask + engine tag (global=1, az-local=2+az, ...):
   * global and local engines can share k, first index AND mask, so the
   * tag is load-bearing (a collision here once wrote a local parity row
   * over a global one — caught by the randomized fuzz test) */
  PlanKey key = plan_key_tag(uint64_t(tag));
  for (int i = 0; i < k + m; i++)
    if (!present[i]) plan_key_set(key, i);
  const uint8_t *pr = present.data();
  DevPlan *p = nullptr;
  int rc;
  if (dpresent < k) { /* missing data */
    auto build = [&](Plan *pl) { return plan_decode(e, pr, pl); };
    rc = cached_plan(c, c->dec_cache, key, lv.stream, std::ref(build), &p);
    if (rc != GFRS_OK) return rc;
    run_plan(OP_APPLY, *p, sh, shard_len, nstripes, lv.stream);
  }
  if (!data_only) {
    auto build = [&](Plan *pl) { return plan_parity(e, pr, pl); };
    rc = cached_plan(c, c->par_cache, key, lv.stream, std::ref(build), &p);
    if (rc != GFRS_OK) return rc;
    if (p) run_plan(OP_APPLY, *p, sh, shard_len, nstripes, lv.stream);
  }
  return GFRS_OK;
}

/* one local stripe set given on its own (lrcencoder.go:94-99,147-153) */
static int reconstruct_local_form(gfrs_ctx_impl *c, const LaneView &lv,
                                  const std::vector<uint8_t> &present,
                                  size_t shard_len, int data_only,
                                  const Shards &sh) {
  const Code &cd = c->code;
  std::vector<int32_t> li(present.size());
  for (size_t i = 0; i < li.size(); i++) li[i] = int32_t(i);
  const Engine e{cd.local_n, cd.local_m, cd.local_matrix.data(), li.data()};
  return reconstruct_engine(c, lv, e, present, shard_len, 1, data_only, sh,
                            /*tag=*/50);
}

/* Core reconstruct across global + local engines.  present covers all
 * n+m+l global slots. */
static int reconstruct_all(gfrs_ctx_impl *c, const LaneView &lv,
                           std::vector<uint8_t> &present, size_t shard_len,
                           int nstripes, int data_only, const Shards &sh) {
  const Code &cd = c->code;
  const gfrs_tactic &t = cd.t;
  std::vector<int32_t> gidx(t.n + t.m);
  for (int i = 0; i < t.n + t.m; i++) gidx[i] = i;
  std::vector<uint8_t> gpresent(present.begin(), present.begin() + t.n + t.m);
  const Engine g{t.n, t.m, cd.enc_matrix.data(), gidx.data()};
  int rc = reconstruct_engine(c, lv, g, gpresent, shard_len, nstripes,
                              data_only, sh, /*tag=*/1);
  if (rc != GFRS_OK) return rc;
  if (t.l == 0 || data_only) return GFRS_OK;
  /* regenerate bad local parities per AZ (lrcencoder.go:160-184); after
   * the global pass everything below n+m is intact */
  for (int az = 0; az < t.az_count; az++) {
    auto idx = local_stripe(t, az);
    bool need = false;
    std::vector<uint8_t> lp(idx.size());
    for (size_t i = 0; i < idx.size(); i++) {
      lp[i] = idx[i] < t.n + t.m ? 1 : present[idx[i]];
      if (!lp[i]) need = true;
    }
    if (!need) continue;
    const Engine e{cd.local_n, cd.local_m, cd.local_matrix.data(),
                   idx.data()};
    rc = reconstruct_engine(c, lv, e, lp, shard_len, nstripes,
                            /*data_only=*/0, sh, /*tag=*/2 + az);
    if (rc != GFRS_OK) return rc;
  }
  return GFRS_OK;
}

}  // namespace gfrs

/* ---------------- compute entry points ---------------- */

extern "C" {

int gfrs_encode(gfrs_ctx *ctx, void *const *shards, size_t shard_len,
                int nshards, int memloc) {
  auto *c = reinterpret_cast<gfrs_ctx_impl *>(ctx);
  const gfrs_tactic &t = c->code.t;
  const int total = c->code.total;
  if (t.m == 0) return nshards == total ? GFRS_OK : GFRS_ERR_INVALID_SHARDS;
  if (nshards != total) {
    seterr("encode: want %d shards, got %d", total, nshards);
    return GFRS_ERR_INVALID_SHARDS;
  }
  /* checkShards (reedsolomon.go:1314-1318) */
  if (shard_len == 0) return GFRS_ERR_SHARD_NO_DATA;
  /* foreground call: fan out over the stream-lane pool so concurrent
   * callers on one context overlap on the GPU (the reference shares one
   * encoder across ~100 goroutines, encoder.go:29) */
  Lane *L = c->pick_lane();
  std::unique_lock<std::mutex> lk(L ? L->mu : c->mu);
  StreamGuard g(c);
  const LaneView lv = L ? view_of(L) : view_of(c);
  int rc;
  if (memloc == GFRS_MEM_HOST) {
    /* stage contiguous stripe, run strided, copy parity back */
    const size_t tot = size_t(total) * shard_len;
    if ((rc = stage_host_stripe(lv, shards, total, t.n, nullptr,
                                shard_len)) != GFRS_OK)
      return rc;
    uint8_t *pin = (uint8_t *)lv.stage_pin->p;
    uint8_t *dev = (uint8_t *)lv.stage_dev->p;
    rc = encode_batch_impl(c, dev, shard_len, tot, 1, lv.stream);
    if (rc != GFRS_OK) return rc;
    HIP_TRY(hipMemcpyAsync(pin + size_t(t.n) * shard_len,
                           dev + size_t(t.n) * shard_len,
                           size_t(t.m + t.l) * shard_len,
                           hipMemcpyDeviceToHost, lv.stream));
    HIP_TRY(hipStreamSynchronize(lv.stream));
    for (int i = t.n; i < total; i++)
      memcpy(shards[i], pin + size_t(i) * shard_len, shard_len);
    return GFRS_OK;
  }
  /* ec.Buffer lays shards out contiguously (buf.go:24-35): detect that
   * and take the strided path — no pointer-table upload, one less
   * dependency on the foreground latency path */
  bool contig = true;
  for (int i = 1; i < nshards && contig; i++)
    contig = (const uint8_t *)shards[i] ==
             (const uint8_t *)shards[0] + size_t(i) * shard_len;
  if (contig) {
    rc = encode_batch_impl(c, shards[0], shard_len,
                           size_t(nshards) * shard_len, 1, lv.stream);
    if (rc != GFRS_OK) return rc;
    HIP_TRY(hipStreamSynchronize(lv.stream));
    return GFRS_OK;
  }
  if ((rc = upload_ptrs(lv, shards, nshards)) != GFRS_OK) return rc;
  run_encode_plans(OP_APPLY, c, table_of(lv, total), shard_len, 1, lv.stream);
  HIP_TRY(hipStreamSynchronize(lv.stream));
  return GFRS_OK;
}

/* unlocked bodies: public entry points take c->mu (the reference encoder
 * is share-safe behind its limiter, encoder.go:29,115) */
static int encode_batch_impl(gfrs_ctx_impl *c, void *base, size_t shard_len,
                             size_t stripe_stride, int nstripes,
                             hipStream_t st) {
  StreamGuard g(c);
  run_encode_plans(OP_APPLY, c, strided(base, stripe_stride), shard_len,
                   nstripes, st);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail("encode_batch launch", e);
  return GFRS_OK;
}

int gfrs_encode_batch(gfrs_ctx *ctx, void *base, size_t shard_len,
                      size_t stripe_stride, int nstripes) {
  auto *c = reinterpret_cast<gfrs_ctx_impl *>(ctx);
  std::lock_guard<std::mutex> lk(c->mu);
  return encode_batch_impl(c, base, shard_len, stripe_stride, nstripes,
                           c->stream);
}

int gfrs_verify(gfrs_ctx *ctx, void *const *shards, size_t shard_len,
                int nshards, int memloc, int *ok) {
  auto *c = reinterpret_cast<gfrs_ctx_impl *>(ctx);
  const int total = c->code.total;
  if (c->code.t.m == 0) { /* zero parity rows: vacuously true (reedsolomon.go:784) */
    *ok = 1;
    return nshards == total ? GFRS_OK : GFRS_ERR_INVALID_SHARDS;
  }
  /* full set or one local stripe set (lrcencoder.go:94-99) */
  bool local_form = c->code.t.l > 0 && nshards == total / c->code.t.az_count;
  if (nshards != total && !local_form) return GFRS_ERR_INVALID_SHARDS;
  if (shard_len == 0) return GFRS_ERR_SHARD_NO_DATA;
  Lane *L = c->pick_lane();
  std::unique_lock<std::mutex> lk(L ? L->mu : c->mu);
  StreamGuard g(c);
  const LaneView lv = L ? view_of(L) : view_of(c);
  int rc;
  Shards sh;
  if (memloc == GFRS_MEM_HOST) {
    if ((rc = stage_host_stripe(lv, shards, nshards, nshards, nullptr,
                                shard_len, local_form ? 0 : 64)) != GFRS_OK)
      return rc;
    sh = strided(lv.stage_dev->p, size_t(nshards) * shard_len);
  } else {
    if ((rc = upload_ptrs(lv, shards, nshards)) != GFRS_OK) return rc;
    sh = table_of(lv, nshards);
  }
  if ((rc = fail_begin(lv.fail_buf, 1, lv.stream)) != GFRS_OK) return rc;
  uint32_t *fail = (uint32_t *)lv.fail_buf->p;
  if (local_form)
    run_plan(OP_VERIFY, c->local_plan, sh, shard_len, 1, lv.stream, fail);
  else
    run_encode_plans(OP_VERIFY, c, sh, shard_len, 1, lv.stream, fail);
  return fail_finish(lv.fail_buf, 1, lv.stream, nullptr, ok);
}

static int verify_batch_impl(gfrs_ctx_impl *c, const void *base,
                             size_t shard_len, size_t stripe_stride,
                             int nstripes, uint64_t *fail_bitmap,
                             hipStream_t st, DevBuf *fail) {
  StreamGuard g(c);
  int rc;
  if ((rc = fail_begin(fail, nstripes, st)) != GFRS_OK) return rc;
  run_encode_plans(OP_VERIFY, c, strided(base, stripe_stride), shard_len,
                   nstripes, st, (uint32_t *)fail->p);
  return fail_finish(fail, nstripes, st, fail_bitmap);
}

int gfrs_verify_batch(gfrs_ctx *ctx, const void *base, size_t shard_len,
                      size_t stripe_stride, int nstripes,
                      uint64_t *fail_bitmap) {
  auto *c = reinterpret_cast<gfrs_ctx_impl *>(ctx);
  std::lock_guard<std::mutex> lk(c->mu);
  return verify_batch_impl(c, base, shard_len, stripe_stride, nstripes,
                           fail_bitmap, c->stream, &c->fail_buf);
}

int gfrs_reconstruct(gfrs_ctx *ctx, void *const *shards, size_t shard_len,
                     int nshards, int memloc, const int32_t *bad_idx,
                     int nbad, int data_only) {
  auto *c = reinterpret_cast<gfrs_ctx_impl *>(ctx);
  const gfrs_tactic &t = c->code.t;
  int rc;

  if (t.m == 0) /* no parity: any missing shard is unrecoverable */
    return nbad == 0 ? GFRS_OK : GFRS_ERR_TOO_FEW_SHARDS;
  /* full set or, for LRC, a single local stripe (lrcencoder.go:147-153) */
  bool local_form = t.l > 0 && nshards == c->code.total / t.az_count;
  if (nshards != c->code.total && !local_form) return GFRS_ERR_INVALID_SHARDS;
  if (shard_len == 0) return GFRS_ERR_SHARD_NO_DATA;

  std::vector<uint8_t> present(nshards, 1);
  for (int i = 0; i < nbad; i++) {
    if (bad_idx[i] < 0 || bad_idx[i] >= nshards) return GFRS_ERR_INVALID_SHARDS;
    present[bad_idx[i]] = 0;
  }
  Lane *L = c->pick_lane();
  std::unique_lock<std::mutex> lk(L ? L->mu : c->mu);
  StreamGuard g(c);
  const LaneView lv = L ? view_of(L) : view_of(c);

  /* host memory: stage the whole stripe contiguously, run strided */
  const bool host = memloc == GFRS_MEM_HOST;
  const size_t tot = size_t(nshards) * shard_len;
  if (host)
    rc = stage_host_stripe(lv, shards, nshards, nshards, present.data(),
                           shard_len);
  else
    rc = upload_ptrs(lv, shards, nshards);
  if (rc != GFRS_OK) return rc;
  const Shards sh = host ? strided(lv.stage_dev->p, tot) : table_of(lv, nshards);
  if (local_form)
    rc = reconstruct_local_form(c, lv, present, shard_len, data_only, sh);
  else
    rc = reconstruct_all(c, lv, present, shard_len, 1, data_only, sh);
  if (rc != GFRS_OK) return rc;
  uint8_t *pin = (uint8_t *)lv.stage_pin->p;
  if (host)
    HIP_TRY(hipMemcpyAsync(pin, lv.stage_dev->p, tot, hipMemcpyDeviceToHost,
                           lv.stream));
  HIP_TRY(hipStreamSynchronize(lv.stream));
  if (host) {
    /* copy back only shards actually rebuilt: with data_only the engine
     * leaves missing parity untouched (ReconstructData semantics,
     * reedsolomon.go:1441-1444) — overwriting the caller's buffer with
     * stale staging bytes would be wrong */
    const int ndata = local_form ? c->code.local_n : t.n;
    for (int i = 0; i < nshards; i++)
      if (!present[i] && (!data_only || i < ndata))
        memcpy(shards[i], pin + size_t(i) * shard_len, shard_len);
  }
  return GFRS_OK;
}

int gfrs_reconstruct_batch(gfrs_ctx *ctx, void *base, size_t shard_len,
                           size_t stripe_stride, int nstripes,
                           const int32_t *bad_idx, int nbad, int data_only) {
  auto *c = reinterpret_cast<gfrs_ctx_impl *>(ctx);
  std::lock_guard<std::mutex> lk(c->mu);
  StreamGuard g(c);
  std::vector<uint8_t> present(c->code.total, 1);
  for (int i = 0; i < nbad; i++) {
    if (bad_idx[i] < 0 || bad_idx[i] >= c->code.total)
      return GFRS_ERR_INVALID_SHARDS;
    present[bad_idx[i]] = 0;
  }
  int rc = reconstruct_all(c, view_of(c), present, shard_len, nstripes,
                           data_only, strided(base, stripe_stride));
  if (rc != GFRS_OK) return rc;
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail("reconstruct_batch launch", e);
  return GFRS_OK;
}

int gfrs_encode_frame_batch(gfrs_ctx *ctx, void *framed,
                            size_t framed_stride, void *base,
                            size_t shard_len, size_t stripe_stride,
                            int nstripes, int64_t block_len) {
  auto *c = reinterpret_cast<gfrs_ctx_impl *>(ctx);
  const gfrs_tactic &t = c->code.t;
  if (block_len <= 0 || block_len % 4096) return GFRS_ERR_INVALID_BLOCK;
  if (nstripes <= 0 || shard_len == 0) return GFRS_ERR_INVALID_SHARDS;
  std::lock_guard<std::mutex> lk(c->mu);
  StreamGuard g(c);
  /* the fused kernel gives a workgroup a whole 64 KiB frame; below a few
   * frames per shard the two-kernel composition (whose rs_apply packs
   * small stripes per tile) is the faster shape.  LRC runs fused through
   * the composed plan: every global AND local parity is a row over the n
   * data shards. */
  const int gm_all = t.m + t.l;
  /* Measured crossover (pipelined fused kernel, RS(6+3), fixed 4 GiB
   * source): fused wins from 8 KiB shards up (837 vs 306 GiB/s at 8 KiB,
   * ~1180 vs ~780 at 16 KiB-8 MiB); the two-kernel path with rs_apply
   * stripe packing wins at 2-4 KiB (684 vs 320 at 2 KiB).
   * GFRS_FUSED_MIN overrides the threshold (bytes); shards
   * <= 4096 take the wave-per-stripe small kernel, and at
   * 5 KiB the big fused kernel beats two-kernel 622 vs 392. */
  static const size_t fused_min = []() {
    const char *e = getenv("GFRS_FUSED_MIN");
    const long v = e ? atol(e) : 0;
    return v > 0 ? size_t(v) : size_t(4097);
  }();
  const bool shapes_ok = block_len == 65536 && t.m >= 1 && gm_all <= 4 &&
                         t.n + gm_all <= 16 && framed_stride % 4 == 0 &&
                         (t.l == 0 || c->fused_lrc_ok);
  /* wave-per-stripe crossover (measured r02): the small kernel wins the
   * whole 4-8 KiB band (5K 1353 / 6K 1427 / 7K 1056 / 8K 863 vs
   * 514-833 GiB/s for the workgroup-per-frame form) */
  static const size_t small_max = []() {
    const char *e = getenv("GFRS_SMALL_MAX");
    const long v = e ? atol(e) : 0;
    return v > 0 ? size_t(v) : size_t(8192);
  }();
  const bool small_ok =
      shard_len <= 4096 || (shard_len <= small_max && gm_all <= 3);
  if (shapes_ok && small_ok) {
    /* MinShardSize-class shapes: wave-per-stripe fused kernel */
    const DevPlan &pl = t.l == 0 ? c->enc_plan : c->fused_lrc;
    launch_rs_encode_frame_small((uint8_t *)framed, framed_stride,
                                 (uint64_t)base, stripe_stride, shard_len,
                                 t.n, gm_all, pl.tab(), nstripes, c->stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail("encode_frame_small launch", e);
    return GFRS_OK;
  }
  const bool fused = shapes_ok && shard_len >= fused_min;
  if (fused) {
    const DevPlan &pl = t.l == 0 ? c->enc_plan : c->fused_lrc;
    launch_rs_encode_frame((uint8_t *)framed, framed_stride, (uint64_t)base,
                           stripe_stride, shard_len, t.n, gm_all,
                           pl.tab(), nstripes, c->stream);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail("encode_frame launch", e);
    return GFRS_OK;
  }
  /* fallback composition: needs the contiguous ec.Buffer batch layout */
  if (stripe_stride != size_t(c->code.total) * shard_len)
    return GFRS_ERR_UNSUPPORTED;
  int rc = encode_batch_impl(c, base, shard_len, stripe_stride, nstripes,
                             c->stream);
  if (rc != GFRS_OK) return rc;
  return crc32b_encode_batch_impl(c, framed, framed_stride, base, shard_len,
                                  int64_t(shard_len), block_len,
                                  nstripes * c->code.total);
}

/* ---------------- sized coder (rpc2 body framing) ---------------- */

int gfrs_sized_encode_size(int64_t actual_size, int64_t block_len,
                           int64_t *size, int64_t *tail) {
  /* PartialEncodeSizeWith with stableSize == 0 (util.go:73-80),
   * _alignment = 512 (rpc2/transport/allocator.go:12-15) */
  int64_t enc = gfrs_crc32b_encode_size(actual_size, block_len);
  if (enc < 0) return int(enc);
  int64_t t = (512 - (enc & 511)) & 511;
  *size = enc + t;
  *tail = t;
  return GFRS_OK;
}

int64_t gfrs_sized_decode_size(int64_t total, int64_t tail,
                               int64_t block_len) {
  /* PartialDecodeSizeWith, stableSize == 0 (util.go:86-94) */
  return gfrs_crc32b_decode_size(total - tail, block_len);
}

int64_t gfrs_sized_encode(gfrs_ctx *ctx, void *dst, const void *src,
                          int64_t n, int64_t block_len) {
  auto *c = reinterpret_cast<gfrs_ctx_impl *>(ctx);
  if (block_len <= 0 || block_len % 4096) return GFRS_ERR_INVALID_BLOCK;
  if (n <= 0) return GFRS_ERR_INVALID_SHARDS;
  int64_t size = 0, tail = 0;
  int rc = gfrs_sized_encode_size(n, block_len, &size, &tail);
  if (rc != GFRS_OK) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  StreamGuard g(c);
  launch_sized_encode((uint8_t *)dst, 0, (const uint8_t *)src, 0, n,
                      block_len, 1, c->stream);
  if (tail)
    HIP_TRY(hipMemsetAsync((uint8_t *)dst + size - tail, 0, size_t(tail),
                           c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return size;
}

int gfrs_sized_verify(gfrs_ctx *ctx, const void *framed, int64_t total,
                      int64_t tail, int64_t block_len, int64_t *bad_block) {
  auto *c = reinterpret_cast<gfrs_ctx_impl *>(ctx);
  if (block_len <= 0 || block_len % 4096) return GFRS_ERR_INVALID_BLOCK;
  std::lock_guard<std::mutex> lk(c->mu);
  StreamGuard g(c);
  int rc;
  if ((rc = c->fail_buf.ensure(8)) != GFRS_OK) return rc;
  int64_t bad = INT64_MAX;
  HIP_TRY(hipMemcpyAsync(c->fail_buf.p, &bad, 8, hipMemcpyHostToDevice,
                         c->stream));
  launch_sized_verify((const uint8_t *)framed, 0, total - tail, block_len, 1,
                      (int64_t *)c->fail_buf.p, c->stream);
  HIP_TRY(hipMemcpyAsync(&bad, c->fail_buf.p, 8, hipMemcpyDeviceToHost,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  *bad_block = bad == INT64_MAX ? -1 : bad;
  return GFRS_OK;
}

int64_t gfrs_sized_decode(gfrs_ctx *ctx, void *dst, const void *framed,
                          int64_t total, int64_t tail, int64_t block_len) {
  auto *c = reinterpret_cast<gfrs_ctx_impl *>(ctx);
  if (block_len <= 0 || block_len % 4096) return GFRS_ERR_INVALID_BLOCK;
  std::lock_guard<std::mutex> lk(c->mu);
  StreamGuard g(c);
  int rc;
  if ((rc = c->fail_buf.ensure(8)) != GFRS_OK) return rc;
  int64_t bad = INT64_MAX;
  HIP_TRY(hipMemcpyAsync(c->fail_buf.p, &bad, 8, hipMemcpyHostToDevice,
                         c->stream));
  launch_sized_decode((uint8_t *)dst, 0, (const uint8_t *)framed, 0,
                      total - tail, block_len, 1, (int64_t *)c->fail_buf.p,
                      c->stream);
  HIP_TRY(hipMemcpyAsync(&bad, c->fail_buf.p, 8, hipMemcpyDeviceToHost,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (bad != INT64_MAX) return GFRS_ERR_MISMATCHED_CRC;
  return gfrs_sized_decode_size(total, tail, block_len);
}

/* ---------------- blobnode shard images ---------------- */

/* (the 32 B headers - magic, BE ids, CRC - are built on device by
 * shard_finalize_k; see shard.go:241-261 for the format) */

int64_t gfrs_shard_disk_size(int64_t size, int64_t block_len) {
  int64_t body = gfrs_crc32b_encode_size(size, block_len);
  if (body < 0) return body;
  return 32 + body + 8; /* header + framed body + footer */
}

int gfrs_shard_write_batch(gfrs_ctx *ctx, void *dst, size_t dst_stride,
                           const void *src, size_t src_stride, int64_t size,
                           int64_t block_len, const uint64_t *bids,
                           const uint64_t *vuids, int nshards) {
  auto *c = reinterpret_cast<gfrs_ctx_impl *>(ctx);
  if (block_len <= 0 || block_len % 4096) return GFRS_ERR_INVALID_BLOCK;
  if (size <= 0 || nshards <= 0) return GFRS_ERR_INVALID_SHARDS;
  std::lock_guard<std::mutex> lk(c->mu);
  StreamGuard g(c);
  int rc;
  /* ship the raw id arrays; the finalize kernel builds the 32 B headers
   * (shard.go:241-261) on device - host-side construction was the
   * bottleneck at millions of shards per call */
  /* this call is async, so no later call may refill the staging before
   * this upload ran (the legacy repair path issues one call per lost
   * column back to back: column b then got column b+1's ids; a pointer
   * table or a host stripe of the next call would do the same):
   * pin_for_write waits for the event recorded here */
  if (!c->pin_ev)
    HIP_TRY(hipEventCreateWithFlags(&c->pin_ev, hipEventDisableTiming));
  if ((rc = stage_ids(c, bids, vuids, size_t(nshards))) != GFRS_OK) return rc;
  HIP_TRY(hipEventRecord(c->pin_ev, c->stream));
  c->pin_pending = true;
  const uint64_t *ids = (const uint64_t *)c->ptr_buf.p;
  /* framed body at +32 */
  launch_crc_encode((uint8_t *)dst + 32, dst_stride, (const uint8_t *)src,
                    src_stride, size, block_len, nshards, c->stream);
  launch_shard_finalize((uint8_t *)dst, dst_stride, ids, ids + nshards, size,
                        block_len, nshards, c->stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail("shard_write launch", e);
  return GFRS_OK;
}

int gfrs_shard_parse_batch(gfrs_ctx *ctx, const void *img, size_t stride,
                           int64_t size, int64_t block_len,
                           uint64_t *out_meta, int64_t *bad_block_per_shard,
                           int nshards) {
  auto *c = reinterpret_cast<gfrs_ctx_impl *>(ctx);
  if (block_len <= 0 || block_len % 4096) return GFRS_ERR_INVALID_BLOCK;
  if (size <= 0 || nshards <= 0) return GFRS_ERR_INVALID_SHARDS;
  int64_t body = gfrs_crc32b_encode_size(size, block_len);
  std::lock_guard<std::mutex> lk(c->mu);
  StreamGuard g(c);
  int rc;
  if ((rc = c->fail_buf.ensure(size_t(nshards) * (8 + 32))) != GFRS_OK)
    return rc;
  int64_t *bad_dev = (int64_t *)c->fail_buf.p;
  uint64_t *meta_dev = (uint64_t *)((uint8_t *)c->fail_buf.p + 8 * nshards);
  std::vector<int64_t> bad(nshards, INT64_MAX);
  HIP_TRY(hipMemcpyAsync(bad_dev, bad.data(), 8 * size_t(nshards),
                         hipMemcpyHostToDevice, c->stream));
  /* body block CRCs */
  launch_crc_verify((const uint8_t *)img + 32, stride, body, block_len,
                    nshards, bad_dev, c->stream);
  /* header/footer */
  launch_shard_parse((const uint8_t *)img, stride, size, block_len, nshards,
                     meta_dev, c->stream);
  HIP_TRY(hipMemcpyAsync(bad.data(), bad_dev, 8 * size_t(nshards),
                         hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(out_meta, meta_dev, 32 * size_t(nshards),
                         hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int j = 0; j < nshards; j++) {
    bad_block_per_shard[j] = bad[j] == INT64_MAX ? -1 : bad[j];
    /* body corruption (caught by the block-CRC recompute) must surface in
     * err too: the frame-header fold in the footer check cannot see
     * payload flips that keep the stored header */
    if (bad_block_per_shard[j] >= 0 && int64_t(out_meta[4 * j + 3]) == 0)
      out_meta[4 * j + 3] = uint64_t(int64_t(GFRS_ERR_MISMATCHED_CRC));
  }
  return GFRS_OK;
}

int gfrs_encode_idx(gfrs_ctx *ctx, const void *data_shard, int idx,
                    void *const *parity, size_t shard_len, int nparity) {
  auto *c = reinterpret_cast<gfrs_ctx_impl *>(ctx);
  /* the reference's order (reedsolomon.go:632-647) */
  if (nparity != c->code.t.m) return GFRS_ERR_TOO_FEW_SHARDS;
  if (nparity == 0) return GFRS_OK; /* replicate: no parity rows, :635-637 */
  if (idx < 0 || idx >= c->code.t.n) return GFRS_ERR_INVALID_SHARDS;
  if (shard_len == 0) return GFRS_ERR_SHARD_NO_DATA;
  std::lock_guard<std::mutex> lk(c->mu);
  StreamGuard g(c);
  int rc;
  /* pointer table: [data, parity...]; plan: k=1 input col idx */
  std::vector<void *> ptrs(1 + nparity);
  ptrs[0] = const_cast<void *>(data_shard);
  for (int r = 0; r < nparity; r++) ptrs[1 + r] = parity[r];
  const LaneView lv = view_of(c);
  if ((rc = upload_ptrs(lv, ptrs.data(), int(ptrs.size()))) != GFRS_OK)
    return rc;
  /* per-idx plan cached in dec_cache keyed off a synthetic mask */
  PlanKey key = plan_key_tag(62); /* EncodeIdx namespace */
  plan_key_set(key, idx);
  DevPlan *p;
  auto build = [&](Plan *pl) { return plan_encode_idx(c->code, idx, pl); };
  rc = cached_plan(c, c->dec_cache, key, c->stream, std::ref(build), &p);
  if (rc != GFRS_OK) return rc;
  run_plan(OP_XOR, *p, table_of(lv, 1 + nparity), shard_len, 1, c->stream);
  HIP_TRY(hipStreamSynchronize(c->stream));
  return GFRS_OK;
}

/* Reconstruct + verify in ONE rs_apply_mixed pass over a plan that writes
 * the bad shards and compares surviving parities (gfrs_plan.h has the row
 * conventions of both builders):
 *   plain RS (tag 63): duplicates in the bad list are tolerated;
 *   LRC (tag 60): every bad shard - data, global or local parity - is a
 *     write row composed over the k global decode inputs.  Requires the bad
 *     set to be globally decodable; returns GFRS_ERR_UNSUPPORTED otherwise
 *     so the caller can fall back to local-stripe decode + full verify. */
static int reconstruct_verify_mixed(gfrs_ctx_impl *c, void *base,
                                    size_t shard_len, size_t stripe_stride,
                                    int nstripes, const int32_t *bad_idx,
                                    int nbad, uint64_t *fail_bitmap) {
  const bool lrc = c->code.t.l != 0;
  PlanKey key;
  int rc = bad_list_key(lrc ? 60 : 63, bad_idx, nbad, c->code.total,
                        /*dup_ok=*/!lrc, &key);
  if (rc != GFRS_OK) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  StreamGuard g(c);
  DevPlan *plan;
  auto build = [&](Plan *pl) {
    return (lrc ? plan_lrc_reconstruct_verify
                : plan_rs_reconstruct_verify)(c->code, bad_idx, nbad, pl);
  };
  rc = cached_plan(c, c->dec_cache, key, c->stream, std::ref(build), &plan);
  if (rc != GFRS_OK) return rc;
  if ((rc = fail_begin(&c->fail_buf, nstripes, c->stream)) != GFRS_OK)
    return rc;
  run_plan(OP_MIXED, *plan, strided(base, stripe_stride), shard_len, nstripes,
           c->stream, (uint32_t *)c->fail_buf.p);
  return fail_finish(&c->fail_buf, nstripes, c->stream, fail_bitmap);
}

int gfrs_reconstruct_verify_batch(gfrs_ctx *ctx, void *base,
                                  size_t shard_len, size_t stripe_stride,
                                  int nstripes, const int32_t *bad_idx,
                                  int nbad, uint64_t *fail_bitmap) {
  auto *c = reinterpret_cast<gfrs_ctx_impl *>(ctx);
  const gfrs_tactic &t = c->code.t;
  if (nstripes <= 0) return GFRS_ERR_INVALID_SHARDS;
  if (t.l == 0)
    return reconstruct_verify_mixed(c, base, shard_len, stripe_stride,
                                    nstripes, bad_idx, nbad, fail_bitmap);
  /* LRC single pass: ONE rs_apply_mixed pass instead of reconstruct + full
   * re-read verify.  Falls back to two passes only when the bad set needs
   * local-stripe decode (globally undecodable). */
  int nglobad = 0;
  for (int i = 0; i < nbad; i++) {
    if (bad_idx[i] < 0 || bad_idx[i] >= c->code.total)
      return GFRS_ERR_INVALID_SHARDS;
    if (bad_idx[i] < t.n + t.m) nglobad++;
  }
  if (nglobad <= t.m && c->fused_lrc_ok) {
    int rc = reconstruct_verify_mixed(c, base, shard_len, stripe_stride,
                                      nstripes, bad_idx, nbad, fail_bitmap);
    if (rc != GFRS_ERR_UNSUPPORTED) return rc;
  }
  int rc = gfrs_reconstruct_batch(ctx, base, shard_len, stripe_stride,
                                  nstripes, bad_idx, nbad, 0);
  if (rc != GFRS_OK) return rc;
  return gfrs_verify_batch(ctx, base, shard_len, stripe_stride, nstripes,
                           fail_bitmap);
}

/* The repair queue: per-job erasure pattern and shard length, a bounded
 * number of launches, one sync.  gfrs_plan.cpp validates the patterns,
 * builds their plans (cached here like the batch call's, same namespaces)
 * and decides which job runs in which launch; rv_queue_prepare collects
 * that and rv_queue_issue uploads the schedule and issues it, both with the
 * context lock held.  Jobs of slow patterns follow as the two passes
 * gfrs_reconstruct_verify_batch falls back to, without its locks and sync. */
struct RvQueue {
  QueueSchedule sched;
  std::vector<uint8_t> blob; /* [npat descriptors | work items | tile prefix
                                sums]; alive until the stream is synced */
  size_t o_items = 0, o_prefix = 0;
};

/* Everything that can refuse: nothing is launched, nothing written. */
static int rv_queue_prepare(gfrs_ctx_impl *c, const gfrs_qjob *jobs, int njobs,
                            const int32_t *bad_idx, const int32_t *bad_off,
                            int npat, RvQueue *q) {
  const Code &cd = c->code;
  const bool lrc = cd.t.l != 0;
  int rc;
  /* every pattern, used or not: validate, then find or build its plan */
  std::vector<QueuePattern> pats(npat);
  std::vector<DevPlan *> plans(npat, nullptr);
  for (int p = 0; p < npat; p++) {
    const int32_t *bad = bad_idx + bad_off[p];
    const int nbad = bad_off[p + 1] - bad_off[p];
    if ((rc = queue_pattern_check(cd, bad, nbad, &pats[p].slow)) != GFRS_OK)
      return rc;
    if (pats[p].slow) continue;
    PlanKey key;
    rc = bad_list_key(lrc ? 60 : 63, bad, nbad, cd.total, /*dup_ok=*/!lrc,
                      &key);
    if (rc != GFRS_OK) return rc;
    auto build = [&](Plan *pl) {
      QueuePattern qp;
      int brc = queue_pattern(cd, bad, nbad, pl, &qp);
      /* the batch call's fallback signal; cached_plan caches no failure */
      return brc == GFRS_OK && qp.slow ? int(GFRS_ERR_UNSUPPORTED) : brc;
    };
    rc = cached_plan(c, c->dec_cache, key, c->stream, std::ref(build),
                     &plans[p]);
    if (rc == GFRS_ERR_UNSUPPORTED) {
      pats[p].slow = true;
      continue;
    }
    if (rc != GFRS_OK) return rc;
    pats[p].nout = plans[p]->nout;
  }
  QueueSchedule &sched = q->sched;
  if ((rc = queue_schedule(jobs, njobs, pats.data(), npat, &sched)) != GFRS_OK)
    return rc;

  /* one upload: [npat descriptors | work items | tile prefix sums] */
  q->o_items = size_t(npat) * sizeof(QueuePat);
  q->o_prefix = q->o_items + sched.items.size() * sizeof(gfrs_qitem);
  const size_t nbytes = q->o_prefix + sched.tile_prefix.size() * 8;
  q->blob.assign(nbytes, 0);
  for (int p = 0; p < npat; p++) {
    QueuePat d{};
    if (plans[p])
      d = QueuePat{plans[p]->in(), plans[p]->out(), plans[p]->tab(),
                   plans[p]->cmp_mask, plans[p]->nout};
    memcpy(&q->blob[size_t(p) * sizeof(QueuePat)], &d, sizeof(d));
  }
  if (!sched.items.empty()) {
    memcpy(&q->blob[q->o_items], sched.items.data(), q->o_prefix - q->o_items);
    memcpy(&q->blob[q->o_prefix], sched.tile_prefix.data(),
           nbytes - q->o_prefix);
  }
  return c->queue_buf.ensure(nbytes);
}

/* Upload and launch a prepared queue.  Job j reports to fail[j], or to
 * fail[fail_slot[j]] when the queue is a part of a larger one (q's items are
 * rewritten for that).  A failure may leave work in flight that still reads
 * q->blob: the caller synchronizes the stream before it lets go of q. */
static int rv_queue_issue(gfrs_ctx_impl *c, void *base, RvQueue *q,
                          const gfrs_qjob *jobs, const int32_t *bad_idx,
                          const int32_t *bad_off, uint32_t *fail,
                          const int32_t *fail_slot) {
  const Code &cd = c->code;
  const QueueSchedule &sched = q->sched;
  if (fail_slot) {
    gfrs_qitem *hi = reinterpret_cast<gfrs_qitem *>(&q->blob[q->o_items]);
    for (size_t i = 0; i < sched.items.size(); i++)
      hi[i].job = fail_slot[sched.items[i].job];
  }
  HIP_TRY(hipMemcpyAsync(c->queue_buf.p, q->blob.data(), q->blob.size(),
                         hipMemcpyHostToDevice, c->stream));
  const uint8_t *dq = (const uint8_t *)c->queue_buf.p;
  for (const QueueBucket &b : sched.buckets)
    launch_rs_apply_queue(
        (uint64_t)base, (const gfrs_qitem *)(dq + q->o_items) + b.first,
        (const uint64_t *)(dq + q->o_prefix) + b.prefix, uint32_t(b.count),
        sched.tile_prefix[b.prefix + b.count], (const QueuePat *)dq, cd.t.n,
        b.gm, fail, c->stream);
  for (int32_t j : sched.slow_jobs) {
    const gfrs_qjob &jb = jobs[j];
    const int32_t *bad = bad_idx + bad_off[jb.pattern];
    const int nbad = bad_off[jb.pattern + 1] - bad_off[jb.pattern];
    std::vector<uint8_t> present(cd.total, 1);
    for (int i = 0; i < nbad; i++) present[bad[i]] = 0;
    const Shards sh = strided((const uint8_t *)base + jb.off, 0);
    int rc = reconstruct_all(c, view_of(c), present, jb.shard_len, 1,
                             /*data_only=*/0, sh);
    if (rc != GFRS_OK) return rc;
    run_encode_plans(OP_VERIFY, c, sh, jb.shard_len, 1, c->stream,
                     fail + (fail_slot ? fail_slot[j] : j));
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail("reconstruct_verify_queue launch", e);
  return GFRS_OK;
}

int gfrs_reconstruct_verify_queue(gfrs_ctx *ctx, void *base,
                                  const gfrs_qjob *jobs, int njobs,
                                  const int32_t *bad_idx,
                                  const int32_t *bad_off, int npat,
                                  uint64_t *fail_bitmap) {
  auto *c = reinterpret_cast<gfrs_ctx_impl *>(ctx);
  if (njobs <= 0 || npat <= 0 || !jobs) return GFRS_ERR_INVALID_SHARDS;
  int rc = queue_offsets_check(bad_off, npat);
  if (rc != GFRS_OK) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  StreamGuard g(c);
  RvQueue q; /* alive until fail_finish has synchronized the stream */
  if ((rc = rv_queue_prepare(c, jobs, njobs, bad_idx, bad_off, npat, &q)) !=
      GFRS_OK)
    return rc;
  if ((rc = fail_begin(&c->fail_buf, njobs, c->stream)) != GFRS_OK) return rc;
  rc = rv_queue_issue(c, base, &q, jobs, bad_idx, bad_off,
                      (uint32_t *)c->fail_buf.p, nullptr);
  if (rc != GFRS_OK) {
    hipStreamSynchronize(c->stream); /* the blob is still being read */
    return rc;
  }
  return fail_finish(&c->fail_buf, njobs, c->stream, fail_bitmap);
}

/* The repair-image queue: gfrs_repair_batch per job, as one call.  Fused
 * patterns run the fused frame kernel over their cached plan (namespace 61,
 * shared with gfrs_repair_batch); in-place patterns are reconstructed and
 * verified in `base` by the reconstruct queue above (its plans, its
 * schedule), then framed from `base` by identity work items.  gfrs_plan.cpp
 * classes the patterns and builds the schedule; this function validates,
 * uploads one blob and issues: in-place work, the <= 4 frame buckets, the
 * finalize launch, one fail_finish. */
int gfrs_repair_queue(gfrs_ctx *ctx, void *base, const gfrs_rjob *jobs,
                      int njobs, const int32_t *bad_idx,
                      const int32_t *bad_off, int npat, void *disk_dst,
                      int64_t block_len, const uint64_t *bids,
                      const uint64_t *vuids, uint64_t *fail_bitmap) {
  auto *c = reinterpret_cast<gfrs_ctx_impl *>(ctx);
  const Code &cd = c->code;
  if (njobs <= 0 || npat <= 0 || !jobs) return GFRS_ERR_INVALID_SHARDS;
  int rc = queue_offsets_check(bad_off, npat);
  if (rc != GFRS_OK) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  StreamGuard g(c);

  /* every pattern, used or not: validate and class it; fused ones find or
   * build their plan */
  std::vector<RepairPattern> pats(npat);
  std::vector<DevPlan *> plans(npat, nullptr);
  for (int p = 0; p < npat; p++) {
    const int32_t *bad = bad_idx + bad_off[p];
    const int nbad = bad_off[p + 1] - bad_off[p];
    if ((rc = repair_pattern_check(cd, bad, nbad, &pats[p])) != GFRS_OK)
      return rc;
    if (pats[p].cls != GFRS_RPAT_FUSED) continue;
    PlanKey key;
    rc = bad_list_key(61, bad, nbad, cd.total, /*dup_ok=*/false, &key);
    if (rc != GFRS_OK) return rc;
    auto build = [&](Plan *pl) { return plan_fused_repair(cd, bad, nbad, pl); };
    rc = cached_plan(c, c->dec_cache, key, c->stream, std::ref(build),
                     &plans[p]);
    if (rc != GFRS_OK) return rc;
    pats[p].gm = plans[p]->nout;
  }
  if (block_len != REPAIR_BLOCK) return GFRS_ERR_UNSUPPORTED;
  RepairSchedule sched;
  rc = repair_schedule(jobs, njobs, pats.data(), npat, bad_idx, bad_off,
                       (uint64_t)disk_dst, bids, vuids, &sched);
  if (rc != GFRS_OK) return rc;

  /* the in-place jobs as a reconstruct queue of their own: their patterns
   * compacted, each job reporting to its caller index */
  RvQueue rvq;
  std::vector<gfrs_qjob> ijobs;
  std::vector<int32_t> ibad, ioff(1, 0), ipat(npat, -1);
  if (!sched.inplace_jobs.empty()) {
    for (int p = 0; p < npat; p++) {
      if (pats[p].cls == GFRS_RPAT_FUSED) continue;
      ipat[p] = int32_t(ioff.size()) - 1;
      ibad.insert(ibad.end(), bad_idx + bad_off[p], bad_idx + bad_off[p + 1]);
      ioff.push_back(int32_t(ibad.size()));
    }
    for (int32_t j : sched.inplace_jobs)
      ijobs.push_back(
          gfrs_qjob{jobs[j].off, jobs[j].shard_len, ipat[jobs[j].pattern], 0});
    rc = rv_queue_prepare(c, ijobs.data(), int(ijobs.size()), ibad.data(),
                          ioff.data(), int(ioff.size()) - 1, &rvq);
    if (rc != GFRS_OK) return rc;
  }

  /* ONE blob: [npat + total descriptors | identity indices | identity table
   * | work items | frame prefix sums | image table]; identity descriptors
   * point into the blob itself */
  const int ndesc = npat + cd.total;
  const size_t o_ident = size_t(ndesc) * sizeof(RepairDesc);
  const size_t o_tab = (o_ident + size_t(cd.total) * 4 + 15) / 16 * 16;
  const size_t o_items = o_tab + 32;
  const size_t o_prefix = o_items + sched.items.size() * sizeof(gfrs_ritem);
  const size_t o_imgs = o_prefix + sched.frame_prefix.size() * 8;
  const size_t nbytes = o_imgs + sched.images.size() * sizeof(gfrs_rimage);
  if ((rc = c->repair_buf.ensure(nbytes)) != GFRS_OK) return rc;
  const uint8_t *dq = (const uint8_t *)c->repair_buf.p;
  std::vector<uint8_t> blob(nbytes, 0);
  for (int p = 0; p < npat; p++) {
    if (!plans[p]) continue;
    const RepairDesc d{plans[p]->in(), plans[p]->tab(), plans[p]->k,
                       pats[p].nw, pats[p].colpack, 0};
    memcpy(&blob[size_t(p) * sizeof(RepairDesc)], &d, sizeof(d));
  }
  for (int s = 0; s < cd.total; s++) {
    const RepairDesc d{(const int32_t *)(dq + o_ident) + s, dq + o_tab, 1, 1,
                       0, 0};
    memcpy(&blob[size_t(npat + s) * sizeof(RepairDesc)], &d, sizeof(d));
    const int32_t idx = s;
    memcpy(&blob[o_ident + size_t(s) * 4], &idx, 4);
  }
  { /* coefficient 1 in the A|B|C split of DevPlan::upload */
    uint8_t *lt = &blob[o_tab];
    for (int i = 0; i < 8; i++) {
      lt[i] = uint8_t(i);
      lt[8 + i] = uint8_t(8 * i);
    }
    for (int i = 0; i < 4; i++) lt[16 + i] = uint8_t(64 * i);
  }
  memcpy(&blob[o_items], sched.items.data(), o_prefix - o_items);
  memcpy(&blob[o_prefix], sched.frame_prefix.data(), o_imgs - o_prefix);
  memcpy(&blob[o_imgs], sched.images.data(), nbytes - o_imgs);

  if ((rc = fail_begin(&c->fail_buf, njobs, c->stream)) != GFRS_OK) return rc;
  uint32_t *fail = (uint32_t *)c->fail_buf.p;
  /* both blobs stay alive until the stream has been synchronized */
  if (!ijobs.empty())
    rc = rv_queue_issue(c, base, &rvq, ijobs.data(), ibad.data(), ioff.data(),
                        fail, sched.inplace_jobs.data());
  hipError_t e = hipSuccess;
  if (rc == GFRS_OK)
    e = hipMemcpyAsync(c->repair_buf.p, blob.data(), nbytes,
                       hipMemcpyHostToDevice, c->stream);
  if (rc == GFRS_OK && e == hipSuccess) {
    for (const RepairBucket &b : sched.buckets)
      launch_rs_repair_frame_queue(
          (uint8_t *)disk_dst, (uint64_t)base,
          (const gfrs_ritem *)(dq + o_items) + b.first,
          (const uint64_t *)(dq + o_prefix) + b.prefix, uint32_t(b.count),
          sched.frame_prefix[b.prefix + b.count], (const RepairDesc *)dq,
          cd.t.n, b.gm, fail, c->stream);
    launch_shard_finalize_queue((uint8_t *)disk_dst,
                                (const gfrs_rimage *)(dq + o_imgs),
                                int(sched.images.size()), nullptr, c->stream);
    e = hipGetLastError();
  }
  if (rc != GFRS_OK || e != hipSuccess) {
    hipStreamSynchronize(c->stream); /* the blobs are still being read */
    return rc != GFRS_OK ? rc : hip_fail("repair_queue launch", e);
  }
  return fail_finish(&c->fail_buf, njobs, c->stream, fail_bitmap);
}

/* The encode+frame queue: gfrs_encode_frame_batch per job, as one call.
 * gfrs_plan.cpp validates the jobs and sorts them into at most 6 buckets;
 * this function uploads one blob [work items | frame prefix sums], issues the
 * small buckets, then the frame buckets, and syncs once.  Tactics outside the
 * gate of the fused kernels run their jobs one at a time as the composition
 * the batch call falls back to. */
int gfrs_encode_frame_queue(gfrs_ctx *ctx, void *framed, void *base,
                            const gfrs_ejob *jobs, int njobs,
                            int64_t block_len) {
  auto *c = reinterpret_cast<gfrs_ctx_impl *>(ctx);
  const Code &cd = c->code;
  const gfrs_tactic &t = cd.t;
  int rc = encode_queue_block_check(block_len);
  if (rc != GFRS_OK) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  StreamGuard g(c);
  EncSchedule sched;
  rc = encode_queue_schedule(jobs, njobs, (uint64_t)framed, &sched);
  if (rc != GFRS_OK) return rc;
  const bool fused =
      encode_frame_fused(cd) && (t.l == 0 || c->fused_lrc_ok);
  hipError_t e = hipSuccess;
  if (fused) {
    /* the blob goes through pinned memory (a 65536-job queue uploads 2.6 MB);
     * the buffer is the context's, reused under its mutex, and the call
     * syncs before it returns */
    const size_t o_prefix = sched.items.size() * sizeof(gfrs_eitem);
    const size_t nbytes = o_prefix + sched.frame_prefix.size() * 8;
    if ((rc = c->encq_buf.ensure(nbytes)) != GFRS_OK) return rc;
    if ((rc = c->encq_pin.ensure(nbytes)) != GFRS_OK) return rc;
    uint8_t *blob = (uint8_t *)c->encq_pin.p;
    memcpy(blob, sched.items.data(), o_prefix);
    if (nbytes > o_prefix)
      memcpy(blob + o_prefix, sched.frame_prefix.data(), nbytes - o_prefix);
    e = hipMemcpyAsync(c->encq_buf.p, blob, nbytes, hipMemcpyHostToDevice,
                       c->stream);
    if (e == hipSuccess) {
      const uint8_t *dq = (const uint8_t *)c->encq_buf.p;
      const DevPlan &pl = t.l == 0 ? c->enc_plan : c->fused_lrc;
      const int gm = t.m + t.l;
      for (const EncBucket &b : sched.buckets) {
        const gfrs_eitem *items = (const gfrs_eitem *)dq + b.first;
        if (b.kind == GFRS_EQ_SMALL)
          launch_rs_encode_frame_small_queue((uint8_t *)framed,
                                             (uint64_t)base, items,
                                             uint32_t(b.count), t.n, gm,
                                             b.param, pl.tab(), c->stream);
        else
          launch_rs_encode_frame_queue(
              (uint8_t *)framed, (uint64_t)base, items,
              (const uint64_t *)(dq + o_prefix) + b.prefix, uint32_t(b.count),
              sched.frame_prefix[b.prefix + b.count], t.n, gm, pl.tab(),
              b.param, c->stream);
      }
      e = hipGetLastError();
    }
  } else {
    for (int j = 0; j < njobs && rc == GFRS_OK; j++) {
      const gfrs_ejob &jb = jobs[j];
      uint8_t *src = (uint8_t *)base + jb.off;
      rc = encode_batch_impl(c, src, jb.shard_len,
                             size_t(cd.total) * jb.shard_len, 1, c->stream);
      if (rc == GFRS_OK)
        rc = crc32b_encode_batch_impl(c, (uint8_t *)framed + jb.img_off,
                                      jb.img_stride, src, jb.shard_len,
                                      int64_t(jb.shard_len), block_len,
                                      cd.total);
    }
  }
  hipError_t se = hipStreamSynchronize(c->stream); /* the one sync; the blob
                                                      is read until here */
  if (rc != GFRS_OK) return rc;
  if (e != hipSuccess) return hip_fail("encode_frame_queue launch", e);
  if (se != hipSuccess) return hip_fail("encode_frame_queue sync", se);
  return GFRS_OK;
}

/* The read queue: crc32block decode + ReconstructData of a segment per job,
 * as one call.  gfrs_plan.cpp validates and classes the patterns and builds
 * the schedule; this function finds or builds the plans of the fused
 * patterns (namespace 64), uploads one blob [npat + n descriptors | identity
 * indices | work items | frame prefix sums], issues the <= 5 buckets, then
 * the slow jobs one at a time, and syncs once.  Words of fused jobs come
 * from the kernel; a slow job's word is assembled from the bad-block answers
 * of its inputs' decodes, which sit behind the words in fail_buf. */
int gfrs_read_queue(gfrs_ctx *ctx, void *out, const void *framed,
                    const gfrs_gjob *jobs, int njobs, const int32_t *bad_idx,
                    const int32_t *bad_off, int npat, int64_t block_len,
                    uint32_t *bad_shards) {
  auto *c = reinterpret_cast<gfrs_ctx_impl *>(ctx);
  const Code &cd = c->code;
  const int n = cd.t.n, nm = cd.t.n + cd.t.m;
  int rc = read_queue_gate(cd, block_len);
  if (rc != GFRS_OK) return rc;
  if (njobs <= 0 || npat <= 0 || !jobs || !bad_shards)
    return GFRS_ERR_INVALID_SHARDS;
  if ((rc = queue_offsets_check(bad_off, npat)) != GFRS_OK) return rc;
  std::lock_guard<std::mutex> lk(c->mu);
  StreamGuard g(c);

  /* every pattern, used or not: validate and class it; its inputs are the
   * first n present of the n+m; fused rebuilds find or build their plan */
  std::vector<ReadPattern> pats(npat);
  std::vector<DevPlan *> plans(npat, nullptr);
  std::vector<std::vector<uint8_t>> present(npat);
  std::vector<uint32_t> pass(npat, 0);
  for (int p = 0; p < npat; p++) {
    const int32_t *bad = bad_idx + bad_off[p];
    const int nbad = bad_off[p + 1] - bad_off[p];
    if ((rc = read_pattern_check(cd, bad, nbad, &pats[p])) != GFRS_OK)
      return rc;
    present[p].assign(nm, 1);
    PlanKey key = plan_key_tag(64);
    for (int i = 0; i < nbad; i++)
      if (bad[i] < nm) {
        present[p][bad[i]] = 0;
        plan_key_set(key, bad[i]);
      }
    for (int i = 0, ci = 0; i < nm && ci < n; i++)
      if (present[p][i]) {
        if (i < n) pass[p] |= 1u << ci;
        ci++;
      }
    if (pats[p].cls != GFRS_GPAT_FUSED || pats[p].r == 0) continue;
    auto build = [&](Plan *pl) { return plan_read(cd, bad, nbad, pl); };
    rc = cached_plan(c, c->dec_cache, key, c->stream, std::ref(build),
                     &plans[p]);
    if (rc != GFRS_OK) return rc;
  }
  ReadSchedule sched;
  rc = read_schedule(cd, jobs, njobs, pats.data(), npat, (uint64_t)out,
                     &sched);
  if (rc != GFRS_OK) return rc;

  /* the slow jobs share one scratch stripe, sized for the largest */
  const int nslow = int(sched.slow_jobs.size());
  size_t scratch = 0;
  for (int32_t j : sched.slow_jobs) {
    const uint64_t raw0 = read_first_frame(jobs[j]) * REPAIR_PAYLOAD;
    const uint64_t raw1 = std::min<uint64_t>(
        (read_last_frame(jobs[j]) + 1) * REPAIR_PAYLOAD, jobs[j].shard_len);
    scratch = std::max(scratch, size_t(nm) * size_t(raw1 - raw0));
  }
  if (scratch && (rc = c->read_scratch.ensure(scratch)) != GFRS_OK) return rc;

  /* ONE blob; identity descriptors and R = 0 patterns point into it */
  const int ndesc = npat + n;
  const size_t o_ident = size_t(ndesc) * sizeof(ReadDesc);
  const size_t o_items = (o_ident + size_t(n) * 4 + 15) / 16 * 16;
  const size_t o_prefix = o_items + sched.items.size() * sizeof(gfrs_gitem);
  const size_t nbytes = o_prefix + sched.frame_prefix.size() * 8;
  if ((rc = c->readq_buf.ensure(nbytes)) != GFRS_OK) return rc;
  if ((rc = c->readq_pin.ensure(nbytes)) != GFRS_OK) return rc;
  const uint8_t *dq = (const uint8_t *)c->readq_buf.p;
  const int32_t *d_ident = (const int32_t *)(dq + o_ident);
  uint8_t *blob = (uint8_t *)c->readq_pin.p;
  memset(blob, 0, o_items);
  for (int p = 0; p < npat; p++) {
    if (pats[p].cls != GFRS_GPAT_FUSED) continue;
    const ReadDesc d =
        plans[p] ? ReadDesc{plans[p]->in(), plans[p]->out(), plans[p]->tab(),
                            plans[p]->k, pass[p]}
                 : ReadDesc{d_ident, nullptr, nullptr, n, pass[p]};
    memcpy(blob + size_t(p) * sizeof(ReadDesc), &d, sizeof(d));
  }
  for (int s = 0; s < n; s++) {
    const ReadDesc d{d_ident + s, nullptr, nullptr, 1, 1u};
    memcpy(blob + size_t(npat + s) * sizeof(ReadDesc), &d, sizeof(d));
    const int32_t idx = s;
    memcpy(blob + o_ident + size_t(s) * 4, &idx, 4);
  }
  if (!sched.items.empty()) {
    memcpy(blob + o_items, sched.items.data(), o_prefix - o_items);
    memcpy(blob + o_prefix, sched.frame_prefix.data(), nbytes - o_prefix);
  }

  /* fail_buf: njobs words, then one bad-block answer per slow-job input */
  const size_t o_bad = (size_t(njobs) * 4 + 7) / 8 * 8;
  const size_t nfail = o_bad + size_t(nslow) * n * 8;
  if ((rc = c->fail_buf.ensure(nfail)) != GFRS_OK) return rc;
  uint32_t *fail = (uint32_t *)c->fail_buf.p;
  int64_t *dbad = (int64_t *)((uint8_t *)c->fail_buf.p + o_bad);
  hipError_t e = hipMemsetAsync(fail, 0, o_bad, c->stream);
  if (e == hipSuccess && nslow)
    e = hipMemsetAsync(dbad, 0xFF, nfail - o_bad, c->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(c->readq_buf.p, blob, nbytes, hipMemcpyHostToDevice,
                       c->stream);
  if (e == hipSuccess) {
    for (const ReadBucket &b : sched.buckets)
      launch_rs_read_frame_queue(
          (uint8_t *)out, (uint64_t)framed,
          (const gfrs_gitem *)(dq + o_items) + b.first,
          (const uint64_t *)(dq + o_prefix) + b.prefix, uint32_t(b.count),
          sched.frame_prefix[b.prefix + b.count], (const ReadDesc *)dq, n, b.r,
          fail, c->stream);
    e = hipGetLastError();
  }
  /* slow jobs: decode the touched frames of the inputs into the scratch
   * stripe, rebuild the missing data there, copy the segment out */
  std::vector<int32_t> gidx(nm);
  for (int i = 0; i < nm; i++) gidx[i] = i;
  const Engine ge{n, cd.t.m, cd.enc_matrix.data(), gidx.data()};
  for (int q = 0; q < nslow && rc == GFRS_OK && e == hipSuccess; q++) {
    const gfrs_gjob &jb = jobs[sched.slow_jobs[q]];
    const uint64_t f0 = read_first_frame(jb), f1 = read_last_frame(jb);
    const uint64_t raw0 = f0 * REPAIR_PAYLOAD;
    const uint64_t flen =
        std::min<uint64_t>((f1 + 1) * REPAIR_PAYLOAD, jb.shard_len) - raw0;
    uint8_t *sc = (uint8_t *)c->read_scratch.p;
    const std::vector<uint8_t> &pr = present[jb.pattern];
    for (int i = 0, ci = 0; i < nm && ci < n; i++) {
      if (!pr[i]) continue;
      launch_crc_decode(sc + size_t(i) * flen, 0,
                        (const uint8_t *)framed + jb.img_off +
                            size_t(i) * jb.img_stride + f0 * REPAIR_BLOCK,
                        0, int64_t(flen + 4 * (f1 - f0 + 1)), REPAIR_BLOCK, 1,
                        dbad + size_t(q) * n + ci, c->stream);
      ci++;
    }
    rc = reconstruct_engine(c, view_of(c), ge, pr, flen, 1, /*data_only=*/1,
                            strided(sc, 0), /*tag=*/1);
    if (rc == GFRS_OK)
      e = hipMemcpy2DAsync((uint8_t *)out + jb.out_off, jb.out_stride,
                           sc + (jb.seg_off - raw0), flen, jb.seg_len, n,
                           hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipGetLastError();
  }
  std::vector<uint8_t> back(nfail);
  if (rc == GFRS_OK && e == hipSuccess)
    e = hipMemcpyAsync(back.data(), c->fail_buf.p, nfail,
                       hipMemcpyDeviceToHost, c->stream);
  hipError_t se = hipStreamSynchronize(c->stream); /* the one sync; the blob
                                                      is read until here */
  if (rc != GFRS_OK) return rc;
  if (e != hipSuccess) return hip_fail("read_queue launch", e);
  if (se != hipSuccess) return hip_fail("read_queue sync", se);
  memcpy(bad_shards, back.data(), size_t(njobs) * 4);
  for (int q = 0; q < nslow; q++) {
    const std::vector<uint8_t> &pr = present[jobs[sched.slow_jobs[q]].pattern];
    uint32_t word = 0;
    for (int i = 0, ci = 0; i < nm && ci < n; i++) {
      if (!pr[i]) continue;
      int64_t b;
      memcpy(&b, &back[o_bad + (size_t(q) * n + ci) * 8], 8);
      if (b != -1) word |= 1u << i;
      ci++;
    }
    bad_shards[sched.slow_jobs[q]] = word;
  }
  return GFRS_OK;
}

/* The shard read queue: gfrs_shard_parse_batch + gfrs_crc32b_decode per job,
 * over images of any size anywhere in one chunk, as one call.  gfrs_plan.cpp
 * validates the jobs and splits them into the storing and the NO_OUT bucket;
 * this function uploads one blob [work items | frame prefix sums | jobs |
 * first-frame places | bad blocks preset to -1] through the pinned staging,
 * issues the <= 2 frame buckets and the header launch, reads the results
 * back and syncs once.  The computed frame CRCs and the results follow the
 * blob in the same grow-only scratch. */
int gfrs_shard_read_queue(gfrs_ctx *ctx, void *out, const void *chunk,
                          const gfrs_sjob *jobs, int njobs, int64_t block_len,
                          gfrs_sresult *results) {
  auto *c = reinterpret_cast<gfrs_ctx_impl *>(ctx);
  int rc = encode_queue_block_check(block_len);
  if (rc != GFRS_OK) return rc;
  if (njobs <= 0 || !jobs || !results) return GFRS_ERR_INVALID_SHARDS;
  std::lock_guard<std::mutex> lk(c->mu);
  StreamGuard g(c);
  ShardReadSchedule sched;
  rc = shard_read_schedule(jobs, njobs, (uint64_t)out, out != nullptr, &sched);
  if (rc != GFRS_OK) return rc;

  const size_t nj = size_t(njobs);
  const size_t o_prefix = nj * sizeof(gfrs_sitem);
  const size_t o_jobs = o_prefix + sched.frame_prefix.size() * 8;
  const size_t o_place = o_jobs + nj * sizeof(gfrs_sjob);
  const size_t o_bad = o_place + nj * 8;
  const size_t nblob = o_bad + nj * 8;
  const size_t o_fcrc = nblob;
  const size_t o_res = (o_fcrc + size_t(sched.total_frames) * 4 + 7) / 8 * 8;
  const size_t nres = nj * sizeof(gfrs_sresult);
  if ((rc = c->shardq_buf.ensure(o_res + nres)) != GFRS_OK) return rc;
  uint8_t *dq = (uint8_t *)c->shardq_buf.p;
  /* the staging an async gfrs_shard_write_batch may still upload its ids
   * from: pin_for_write waits that copy out */
  uint8_t *blob;
  if ((rc = pin_for_write(view_of(c), nblob, &blob)) != GFRS_OK) return rc;
  memcpy(blob, sched.items.data(), o_prefix);
  memcpy(blob + o_prefix, sched.frame_prefix.data(), o_jobs - o_prefix);
  memcpy(blob + o_jobs, jobs, o_place - o_jobs);
  memcpy(blob + o_place, sched.job_frame.data(), o_bad - o_place);
  memset(blob + o_bad, 0xFF, nblob - o_bad);

  uint32_t *fcrc = (uint32_t *)(dq + o_fcrc);
  int64_t *bad = (int64_t *)(dq + o_bad);
  hipError_t e =
      hipMemcpyAsync(dq, blob, nblob, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    for (const ShardReadBucket &b : sched.buckets)
      launch_shard_read_frame_queue(
          (uint8_t *)out, (uint64_t)chunk, (const gfrs_sitem *)dq + b.first,
          (const uint64_t *)(dq + o_prefix) + b.prefix, uint32_t(b.count),
          sched.frame_prefix[b.prefix + b.count], !b.no_out,
          fcrc + b.frame_base, bad, c->stream);
    launch_shard_head_queue((uint64_t)chunk, (const gfrs_sjob *)(dq + o_jobs),
                            (const uint64_t *)(dq + o_place), fcrc, bad,
                            (gfrs_sresult *)(dq + o_res), njobs, c->stream);
    e = hipGetLastError();
  }
  std::vector<gfrs_sresult> back(nj);
  if (e == hipSuccess)
    e = hipMemcpyAsync(back.data(), dq + o_res, nres, hipMemcpyDeviceToHost,
                       c->stream);
  hipError_t se = hipStreamSynchronize(c->stream); /* the one sync; the blob
                                                      is read until here */
  if (e != hipSuccess) return hip_fail("shard_read_queue launch", e);
  if (se != hipSuccess) return hip_fail("shard_read_queue sync", se);
  memcpy(results, back.data(), nres);
  return GFRS_OK;
}

/* The shard write queue: gfrs_shard_write_batch per job, over payloads of any
 * size that are raw bytes or the body of an existing image, as one call.
 * gfrs_plan.cpp validates the jobs and splits them into the raw and the
 * SRC_IMAGE bucket; this function uploads one blob [work items | frame prefix
 * sums | jobs | first-frame places | bad blocks preset to -1] through the
 * pinned staging, issues the <= 2 frame buckets and the head launch, reads
 * the results back and syncs once.  The computed frame CRCs and the results
 * follow the blob in the same grow-only scratch. */
int gfrs_shard_write_queue(gfrs_ctx *ctx, void *dst, const void *src,
                           const gfrs_wjob *jobs, int njobs, int64_t block_len,
                           gfrs_sresult *results) {
  auto *c = reinterpret_cast<gfrs_ctx_impl *>(ctx);
  int rc = encode_queue_block_check(block_len);
  if (rc != GFRS_OK) return rc;
  if (njobs <= 0 || !jobs || !results || !dst || !src)
    return GFRS_ERR_INVALID_SHARDS;
  std::lock_guard<std::mutex> lk(c->mu);
  StreamGuard g(c);
  ShardWriteSchedule sched;
  rc = shard_write_schedule(jobs, njobs, (uint64_t)dst, &sched);
  if (rc != GFRS_OK) return rc;

  const size_t nj = size_t(njobs);
  const size_t o_prefix = nj * sizeof(gfrs_witem);
  const size_t o_jobs = o_prefix + sched.frame_prefix.size() * 8;
  const size_t o_place = o_jobs + nj * sizeof(gfrs_wjob);
  const size_t o_bad = o_place + nj * 8;
  const size_t nblob = o_bad + nj * 8;
  const size_t o_fcrc = nblob;
  const size_t o_res = (o_fcrc + size_t(sched.total_frames) * 4 + 7) / 8 * 8;
  const size_t nres = nj * sizeof(gfrs_sresult);
  if ((rc = c->shardwq_buf.ensure(o_res + nres)) != GFRS_OK) return rc;
  uint8_t *dq = (uint8_t *)c->shardwq_buf.p;
  /* the staging an async gfrs_shard_write_batch may still upload its ids
   * from: pin_for_write waits that copy out */
  uint8_t *blob;
  if ((rc = pin_for_write(view_of(c), nblob, &blob)) != GFRS_OK) return rc;
  memcpy(blob, sched.items.data(), o_prefix);
  memcpy(blob + o_prefix, sched.frame_prefix.data(), o_jobs - o_prefix);
  memcpy(blob + o_jobs, jobs, o_place - o_jobs);
  memcpy(blob + o_place, sched.job_frame.data(), o_bad - o_place);
  memset(blob + o_bad, 0xFF, nblob - o_bad);

  uint32_t *fcrc = (uint32_t *)(dq + o_fcrc);
  int64_t *bad = (int64_t *)(dq + o_bad);
  hipError_t e =
      hipMemcpyAsync(dq, blob, nblob, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    for (const ShardWriteBucket &b : sched.buckets)
      launch_shard_write_frame_queue(
          (uint8_t *)dst, (uint64_t)src, (const gfrs_witem *)dq + b.first,
          (const uint64_t *)(dq + o_prefix) + b.prefix, uint32_t(b.count),
          sched.frame_prefix[b.prefix + b.count], b.src_image != 0,
          fcrc + b.frame_base, bad, c->stream);
    launch_shard_write_head_queue(
        (uint8_t *)dst, (uint64_t)src, (const gfrs_wjob *)(dq + o_jobs),
        (const uint64_t *)(dq + o_place), fcrc, bad,
        (gfrs_sresult *)(dq + o_res), njobs, c->stream);
    e = hipGetLastError();
  }
  std::vector<gfrs_sresult> back(nj);
  if (e == hipSuccess)
    e = hipMemcpyAsync(back.data(), dq + o_res, nres, hipMemcpyDeviceToHost,
                       c->stream);
  hipError_t se = hipStreamSynchronize(c->stream); /* the one sync; the blob
                                                      is read until here */
  if (e != hipSuccess) return hip_fail("shard_write_queue launch", e);
  if (se != hipSuccess) return hip_fail("shard_write_queue sync", se);
  memcpy(results, back.data(), nres);
  return GFRS_OK;
}

/* The put queue: encode + frame + header/footer per job, as one call, for every
 * tactic up to 32 data shards.  gfrs_plan.cpp validates the jobs and builds
 * the schedule; this function uploads one blob [work items | frame prefix
 * sums | image table] through the pinned staging, issues the encode queue's
 * buckets (narrow tactics) or the two frame buckets once per row group (wide
 * ones), then the head launch, reads the image CRCs back and syncs once. */
int gfrs_put_queue(gfrs_ctx *ctx, void *disk_dst, const void *base,
                   const gfrs_pjob *jobs, int njobs, const uint64_t *vuids,
                   int nvol, int64_t block_len, uint32_t *crcs) {
  auto *c = reinterpret_cast<gfrs_ctx_impl *>(ctx);
  const Code &cd = c->code;
  const gfrs_tactic &t = cd.t;
  int rc = put_queue_gate(cd, block_len);
  if (rc != GFRS_OK) return rc;
  if (!disk_dst || !base) return GFRS_ERR_INVALID_SHARDS;
  std::lock_guard<std::mutex> lk(c->mu);
  StreamGuard g(c);
  PutSchedule sched;
  rc = put_queue_schedule(cd, jobs, njobs, vuids, nvol, (uint64_t)disk_dst,
                          &sched);
  if (rc != GFRS_OK) return rc;

  /* the parity rows over the n data shards, row-major [rows*n][32] */
  const DevPlan *pl = &c->enc_plan;
  if (t.l > 0) {
    if (c->fused_lrc_ok) {
      pl = &c->fused_lrc;
    } else {
      if (!c->put_lrc_ok) {
        Plan p;
        if ((rc = plan_fused_lrc(cd, &p)) != GFRS_OK) return rc;
        if ((rc = c->put_lrc.upload(p, c->stream)) != GFRS_OK) return rc;
        c->put_lrc_ok = true;
      }
      pl = &c->put_lrc;
    }
  }

  const EncSchedule &es = sched.enc;
  const size_t nimg = sched.images.size();
  const size_t o_prefix = es.items.size() * sizeof(gfrs_eitem);
  const size_t o_imgs = o_prefix + es.frame_prefix.size() * 8;
  const size_t nblob = o_imgs + nimg * sizeof(gfrs_rimage);
  const size_t o_crc = nblob;
  if ((rc = c->putq_buf.ensure(o_crc + nimg * 4)) != GFRS_OK) return rc;
  uint8_t *dq = (uint8_t *)c->putq_buf.p;
  /* the staging an async gfrs_shard_write_batch may still upload its ids
   * from: pin_for_write waits that copy out */
  uint8_t *blob;
  if ((rc = pin_for_write(view_of(c), nblob, &blob)) != GFRS_OK) return rc;
  memcpy(blob, es.items.data(), o_prefix);
  if (o_imgs > o_prefix)
    memcpy(blob + o_prefix, es.frame_prefix.data(), o_imgs - o_prefix);
  memcpy(blob + o_imgs, sched.images.data(), nblob - o_imgs);

  uint8_t *dst = (uint8_t *)disk_dst;
  const int k = t.n;
  hipError_t e =
      hipMemcpyAsync(dq, blob, nblob, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    const uint64_t *dprefix = (const uint64_t *)(dq + o_prefix);
    if (!sched.wide) {
      const int gm = t.m + t.l;
      for (const EncBucket &b : es.buckets) {
        const gfrs_eitem *items = (const gfrs_eitem *)dq + b.first;
        if (b.kind == GFRS_EQ_SMALL)
          launch_rs_encode_frame_small_queue(dst, (uint64_t)base, items,
                                             uint32_t(b.count), k, gm, b.param,
                                             pl->tab(), c->stream);
        else
          launch_rs_encode_frame_queue(
              dst, (uint64_t)base, items, dprefix + b.prefix,
              uint32_t(b.count), es.frame_prefix[b.prefix + b.count], k, gm,
              pl->tab(), b.param, c->stream);
      }
    } else {
      for (size_t gi = 0; gi < sched.group_rows.size(); gi++) {
        const int row0 = int(gi) * PUT_ROWS;
        for (const EncBucket &b : es.buckets)
          launch_rs_put_frame_queue(
              dst, (uint64_t)base, (const gfrs_eitem *)dq + b.first,
              dprefix + b.prefix, uint32_t(b.count),
              es.frame_prefix[b.prefix + b.count], k, sched.group_rows[gi],
              row0, pl->tab() + size_t(row0) * k * 32, b.param, gi == 0,
              c->stream);
      }
    }
    launch_shard_finalize_queue(dst, (const gfrs_rimage *)(dq + o_imgs),
                                int(nimg), (uint32_t *)(dq + o_crc),
                                c->stream);
    e = hipGetLastError();
  }
  std::vector<uint32_t> back(crcs ? nimg : 0);
  if (e == hipSuccess && crcs)
    e = hipMemcpyAsync(back.data(), dq + o_crc, nimg * 4,
                       hipMemcpyDeviceToHost, c->stream);
  hipError_t se = hipStreamSynchronize(c->stream); /* the one sync; the blob
                                                      is read until here */
  if (e != hipSuccess) return hip_fail("put_queue launch", e);
  if (se != hipSuccess) return hip_fail("put_queue sync", se);
  if (crcs) memcpy(crcs, back.data(), nimg * 4);
  return GFRS_OK;
}

int gfrs_update_idx(gfrs_ctx *ctx, const void *old_shard,
                    const void *new_shard, int idx, void *const *parity,
                    size_t shard_len, int nparity) {
  /* the first pass validates for both: its checks depend on nothing the
   * second pass is given differently, so a refused call has run neither */
  int rc = gfrs_encode_idx(ctx, old_shard, idx, parity, shard_len, nparity);
  if (rc != GFRS_OK) return rc;
  return gfrs_encode_idx(ctx, new_shard, idx, parity, shard_len, nparity);
}

/* Chunked finalize pipeline (GFRS_REPAIR_CHUNK=N, DEFAULT OFF): stripes
 * per chunk, nstripes = one launch.  The header/footer pass of chunk c only
 * needs chunk c's images (the footer CRC is GF(2)-combined from the frame
 * CRCs the repair kernel just wrote), so it can run on an aux stream behind
 * an event while chunk c+1's repair kernel streams on the main stream.
 * Measured @512x4MiB RS(6+3) bad=[2,6]: the single launch wins — 5.66 ms
 * serial vs 6.48-7.71 chunked (CH=64/128/256): each repair sub-launch pays
 * a fill/drain ramp and the finalize competes for bandwidth, costing more
 * than the ~0.9 ms finalize pass hides.  Kept as a measured variant;
 * parity-tested (test_repair_batch_chunk_pipeline). */
static int repair_chunk(size_t shard_len, int nstripes) {
  if (shard_len <= 4096) return nstripes;
  const char *e = getenv("GFRS_REPAIR_CHUNK");
  const long v = e ? atol(e) : 0;
  return v > 0 && v < (long)nstripes ? (int)v : nstripes;
}

/* Fused repair: one kernel reads the k inputs + surviving-parity check
 * shards and writes ONLY the repaired shards' framed bodies - the raw
 * reconstruction never touches HBM and `base` is NOT mutated (the legacy
 * path of gfrs_repair_batch reconstructs in place). */
static int repair_fused(gfrs_ctx_impl *cc, void *base, size_t shard_len,
                        size_t stripe_stride, int nstripes,
                        const int32_t *bad_idx, int nbad, void *disk_dst,
                        size_t dst_stride, int64_t block_len,
                        const uint64_t *bids, const uint64_t *vuids,
                        uint64_t *fail_bitmap) {
  /* the image column of each rebuild row follows the caller's order, which
   * the cached plan (keyed by the bad SET, local-parity bads included)
   * does not know */
  uint32_t colpack = 0;
  PlanKey key; /* 61 = fused-repair namespace */
  int rc = bad_list_key(61, bad_idx, nbad, cc->code.total, /*dup_ok=*/false,
                        &key);
  if (rc == GFRS_OK)
    rc = repair_colpack(cc->code.total, bad_idx, nbad, &colpack);
  if (rc != GFRS_OK) return rc;
  std::lock_guard<std::mutex> lk(cc->mu);
  StreamGuard g(cc);
  DevPlan *plan;
  auto build = [&](Plan *pl) {
    return plan_fused_repair(cc->code, bad_idx, nbad, pl);
  };
  rc = cached_plan(cc, cc->dec_cache, key, cc->stream, std::ref(build), &plan);
  if (rc != GFRS_OK) return rc;
  if ((rc = fail_begin(&cc->fail_buf, nstripes, cc->stream)) != GFRS_OK)
    return rc;
  uint32_t *fail = (uint32_t *)cc->fail_buf.p;
  /* id arrays for every (stripe, bad) image, caller's column order;
   * headers themselves are built by the finalize kernel */
  const size_t nimg = size_t(nstripes) * nbad;
  if ((rc = stage_ids(cc, bids, vuids, nimg)) != GFRS_OK) return rc;
  const uint64_t *ids = (const uint64_t *)cc->ptr_buf.p;
  /* stripes [lo, lo+cn): repair kernel on the main stream, then the
   * header/footer pass on `fin` */
  auto repair = [&](int lo, int cn, hipStream_t fin, hipEvent_t ev) {
    uint8_t *cd = (uint8_t *)disk_dst + size_t(lo) * nbad * dst_stride;
    (shard_len <= 4096 ? launch_rs_repair_frame_small
                       : launch_rs_repair_frame)(
        cd + 32, dst_stride, (uint64_t)base + (uint64_t)lo * stripe_stride,
        stripe_stride, shard_len, plan->k, plan->nout, nbad, plan->in(),
        plan->tab(), colpack, fail + lo, cn, cc->stream);
    if (ev) {
      HIP_TRY(hipEventRecord(ev, cc->stream));
      HIP_TRY(hipStreamWaitEvent(fin, ev, 0));
    }
    launch_shard_finalize(cd, dst_stride, ids + size_t(lo) * nbad,
                          ids + nimg + size_t(lo) * nbad, int64_t(shard_len),
                          block_len, cn * nbad, fin);
    return int(GFRS_OK);
  };
  const int chunk = repair_chunk(shard_len, nstripes);
  const bool pipe = chunk < nstripes && cc->ensure_aux() == GFRS_OK;
  if (!pipe) {
    repair(0, nstripes, cc->stream, nullptr);
  } else {
    int ci = 0;
    for (int lo = 0; lo < nstripes; lo += chunk, ci++)
      if ((rc = repair(lo, std::min(chunk, nstripes - lo), cc->aux_stream,
                       cc->aux_ev[ci & 1])) != GFRS_OK)
        return rc;
    HIP_TRY(hipEventRecord(cc->aux_done, cc->aux_stream));
    HIP_TRY(hipStreamWaitEvent(cc->stream, cc->aux_done, 0));
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail("repair_frame launch", e);
  return fail_finish(&cc->fail_buf, nstripes, cc->stream, fail_bitmap);
}

int gfrs_repair_batch(gfrs_ctx *ctx, void *base, size_t shard_len,
                      size_t stripe_stride, int nstripes,
                      const int32_t *bad_idx, int nbad, void *disk_dst,
                      size_t dst_stride, int64_t block_len,
                      const uint64_t *bids, const uint64_t *vuids,
                      uint64_t *fail_bitmap) {
  if (nbad <= 0) return GFRS_ERR_INVALID_SHARDS;
  auto *cc = reinterpret_cast<gfrs_ctx_impl *>(ctx);
  const gfrs_tactic &t = cc->code.t;
  static const size_t fmin = []() {
    const char *e = getenv("GFRS_FUSED_MIN");
    const long v = e ? atol(e) : 0;
    return v > 0 ? size_t(v) : size_t(4097);
  }();
  int nglobad = 0;
  for (int i = 0; i < nbad; i++)
    if (bad_idx[i] < t.n + t.m) nglobad++;
  /* The kernel carries 4 rows: nbad rebuild rows plus one check row per
   * surviving parity that is not an input, m + l rows in all.  A tactic
   * with m + l > 4 (RS(6+6)) would drop check rows and pass stripes the
   * reference Verify fails, so it takes the legacy path. */
  if ((t.l == 0 || cc->fused_lrc_ok) && block_len == 65536 && t.m >= 1 &&
      t.m + t.l <= 4 && t.n + t.m + t.l <= 16 && nglobad <= t.m &&
      nbad <= 4 && (shard_len >= fmin || shard_len <= 4096) &&
      dst_stride % 4 == 0 && nstripes > 0)
    return repair_fused(cc, base, shard_len, stripe_stride, nstripes, bad_idx,
                        nbad, disk_dst, dst_stride, block_len, bids, vuids,
                        fail_bitmap);
  /* legacy path: reconstruct + the mandatory verify in one data pass */
  int rc = gfrs_reconstruct_verify_batch(ctx, base, shard_len, stripe_stride,
                                         nstripes, bad_idx, nbad,
                                         fail_bitmap);
  if (rc != GFRS_OK) return rc;
  /* frame each repaired shard; images laid out (stripe, bad) row-major.
   * For bad shard b the raw source is strided across stripes.  The
   * sub-calls take the ctx lock themselves; stream ordering serializes
   * the kernels. */
  std::vector<uint64_t> bb(nstripes), vv(nstripes);
  for (int b = 0; b < nbad; b++) {
    /* headers differ per stripe: gather this bad-shard column's ids */
    for (int s2 = 0; s2 < nstripes; s2++) {
      bb[s2] = bids[size_t(s2) * nbad + b];
      vv[s2] = vuids[size_t(s2) * nbad + b];
    }
    /* write images for column b: dst row stride = nbad*dst_stride */
    rc = gfrs_shard_write_batch(
        ctx, (uint8_t *)disk_dst + size_t(b) * dst_stride,
        size_t(nbad) * dst_stride,
        (const uint8_t *)base + size_t(bad_idx[b]) * shard_len,
        stripe_stride, int64_t(shard_len), block_len, bb.data(), vv.data(),
        nstripes);
    if (rc != GFRS_OK) return rc;
  }
  return GFRS_OK;
}

/* ---------------- crc32block ---------------- */

/* Host CRC32-IEEE (reflected 0xEDB88320), slice-by-8, Update semantics
 * like hash/crc32.Update (util.go:22 ChecksumIEEE call sites).  Host-side
 * on purpose: it backs the per-block streaming request-body wrapper
 * (request_body.go:57-127), which the reference also runs on host CPUs;
 * all bulk framing goes through the device kernels. */
static uint32_t g_crc8tab[8][256];
static std::once_flag g_crc8_once;

static void crc8tab_init() {
  for (uint32_t i = 0; i < 256; i++) {
    uint32_t c = i;
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1)));
    g_crc8tab[0][i] = c;
  }
  for (int t = 1; t < 8; t++)
    for (uint32_t i = 0; i < 256; i++)
      g_crc8tab[t][i] =
          (g_crc8tab[t - 1][i] >> 8) ^ g_crc8tab[0][g_crc8tab[t - 1][i] & 0xFF];
}

uint32_t gfrs_crc32_host(uint32_t crc, const void *data, int64_t n) {
  std::call_once(g_crc8_once, crc8tab_init);
  const uint8_t *p = (const uint8_t *)data;
  uint32_t c = ~crc;
  while (n >= 8) {
    uint32_t lo, hi;
    memcpy(&lo, p, 4);
    memcpy(&hi, p + 4, 4);
    lo ^= c;
    c = g_crc8tab[7][lo & 0xFF] ^ g_crc8tab[6][(lo >> 8) & 0xFF] ^
        g_crc8tab[5][(lo >> 16) & 0xFF] ^ g_crc8tab[4][lo >> 24] ^
        g_crc8tab[3][hi & 0xFF] ^ g_crc8tab[2][(hi >> 8) & 0xFF] ^
        g_crc8tab[1][(hi >> 16) & 0xFF] ^ g_crc8tab[0][hi >> 24];
    p += 8;
    n -= 8;
  }
  while (n-- > 0) c = (c >> 8) ^ g_crc8tab[0][(c ^ *p++) & 0xFF];
  return ~c;
}

int64_t gfrs_crc32b_encode_size(int64_t size, int64_t block_len) {
  if (block_len <= 0 || block_len % 4096) return GFRS_ERR_INVALID_BLOCK;
  int64_t payload = block_len - 4;
  return size + 4 * ((size + payload - 1) / payload);
}

int64_t gfrs_crc32b_decode_size(int64_t size, int64_t block_len) {
  if (block_len <= 0 || block_len % 4096) return GFRS_ERR_INVALID_BLOCK;
  return size - 4 * ((size + block_len - 1) / block_len);
}

static int crc32b_encode_batch_impl(gfrs_ctx_impl *c, void *dst,
                                    size_t dst_stride, const void *src,
                                    size_t src_stride, int64_t n,
                                    int64_t block_len, int nshards) {
  if (block_len <= 0 || block_len % 4096) return GFRS_ERR_INVALID_BLOCK;
  if (n <= 0 || nshards <= 0) return GFRS_ERR_INVALID_SHARDS;
  StreamGuard g(c);
  launch_crc_encode((uint8_t *)dst, dst_stride, (const uint8_t *)src,
                    src_stride, n, block_len, nshards, c->stream);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail("crc encode launch", e);
  return GFRS_OK;
}

int gfrs_crc32b_encode_batch(gfrs_ctx *ctx, void *dst, size_t dst_stride,
                             const void *src, size_t src_stride, int64_t n,
                             int64_t block_len, int nshards) {
  auto *c = reinterpret_cast<gfrs_ctx_impl *>(ctx);
  std::lock_guard<std::mutex> lk(c->mu);
  return crc32b_encode_batch_impl(c, dst, dst_stride, src, src_stride, n,
                                  block_len, nshards);
}

int64_t gfrs_crc32b_encode(gfrs_ctx *ctx, void *dst, const void *src,
                           int64_t n, int64_t block_len) {
  auto *c = reinterpret_cast<gfrs_ctx_impl *>(ctx);
  std::lock_guard<std::mutex> lk(c->mu);
  int rc = crc32b_encode_batch_impl(c, dst, 0, src, 0, n, block_len, 1);
  if (rc != GFRS_OK) return rc;
  StreamGuard g(c);
  HIP_TRY(hipStreamSynchronize(c->stream));
  return gfrs_crc32b_encode_size(n, block_len);
}

int gfrs_crc32b_verify_batch(gfrs_ctx *ctx, const void *framed, size_t stride,
                             int64_t framed_len, int64_t block_len,
                             int nshards, int64_t *bad_block_per_shard) {
  auto *c = reinterpret_cast<gfrs_ctx_impl *>(ctx);
  if (block_len <= 0 || block_len % 4096) return GFRS_ERR_INVALID_BLOCK;
  if (framed_len <= 0 || nshards <= 0) return GFRS_ERR_INVALID_SHARDS;
  std::lock_guard<std::mutex> lk(c->mu);
  StreamGuard g(c);
  int rc;
  if ((rc = c->fail_buf.ensure(size_t(nshards) * 8)) != GFRS_OK) return rc;
  std::vector<int64_t> bad(nshards, INT64_MAX);
  HIP_TRY(hipMemcpyAsync(c->fail_buf.p, bad.data(), size_t(nshards) * 8,
                         hipMemcpyHostToDevice, c->stream));
  launch_crc_verify((const uint8_t *)framed, stride, framed_len, block_len,
                    nshards, (int64_t *)c->fail_buf.p, c->stream);
  HIP_TRY(hipMemcpyAsync(bad.data(), c->fail_buf.p, size_t(nshards) * 8,
                         hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int i = 0; i < nshards; i++)
    bad_block_per_shard[i] = bad[i] == INT64_MAX ? -1 : bad[i];
  return GFRS_OK;
}

int gfrs_crc32b_verify(gfrs_ctx *ctx, const void *framed, int64_t framed_len,
                       int64_t block_len, int64_t *bad_block) {
  return gfrs_crc32b_verify_batch(ctx, framed, 0, framed_len, block_len, 1,
                                  bad_block);
}

int64_t gfrs_crc32b_decode(gfrs_ctx *ctx, void *dst, const void *framed,
                           int64_t framed_len, int64_t block_len) {
  auto *c = reinterpret_cast<gfrs_ctx_impl *>(ctx);
  if (block_len <= 0 || block_len % 4096) return GFRS_ERR_INVALID_BLOCK;
  std::lock_guard<std::mutex> lk(c->mu);
  StreamGuard g(c);
  int rc;
  if ((rc = c->fail_buf.ensure(8)) != GFRS_OK) return rc;
  int64_t bad = INT64_MAX;
  HIP_TRY(hipMemcpyAsync(c->fail_buf.p, &bad, 8, hipMemcpyHostToDevice,
                         c->stream));
  launch_crc_decode((uint8_t *)dst, 0, (const uint8_t *)framed, 0, framed_len,
                    block_len, 1, (int64_t *)c->fail_buf.p, c->stream);
  HIP_TRY(hipMemcpyAsync(&bad, c->fail_buf.p, 8, hipMemcpyDeviceToHost,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (bad != INT64_MAX) return GFRS_ERR_MISMATCHED_CRC;
  return gfrs_crc32b_decode_size(framed_len, block_len);
}

} /* extern "C" */
