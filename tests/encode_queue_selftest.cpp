/* tests/encode_queue_selftest.cpp — stand-alone host check of the
 * encode+frame schedule builder (cubefs_amd/csrc/gfrs_plan.cpp), meant to be
 * built with -fsanitize=address,undefined by a plain host compiler together
 * with gfrs_plan.cpp and gfrs_gf.cpp (tests/test_encode_queue_cpu.py does
 * that).
 *
 * Generated queues - the lengths of tests/_encq.py interleaved, one class
 * only, one job, a large queue, huge shards, pseudo-random ones - go through
 * encode_queue_schedule and through the C export.  Every schedule must hold
 * each job in exactly one bucket, of the class and param its length demands,
 * in caller order, with at most 6 buckets in the fixed order and the frame
 * prefix sums of ceil(shard_len / 65532).  Bad arguments must return their
 * codes.  Exit status 0 and "encode queue selftest OK" on success.
 */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../cubefs_amd/csrc/gfrs_plan.h"

using namespace gfrs;

#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      fprintf(stderr, "FAIL %s:%d: %s\n  ", __FILE__, __LINE__, #cond); \
      fprintf(stderr, __VA_ARGS__);               \
      fprintf(stderr, "\n");                      \
      exit(1);                                    \
    }                                             \
  } while (0)

static long g_items = 0;

static uint64_t round4(uint64_t n) { return (n + 3) / 4 * 4; }
static uint64_t frames(uint64_t len) { return (len + 65531) / 65532; }

/* odd gaps between jobs; images back to back at 4-aligned offsets, tight
 * stride for odd jobs, padded for even ones */
static std::vector<gfrs_ejob> layout(int total,
                                     const std::vector<uint64_t> &lens) {
  static const int gaps[11] = {1, 3, 7, 5, 11, 1, 9, 3, 13, 7, 5};
  std::vector<gfrs_ejob> jobs;
  uint64_t off = 0, img = 0;
  for (size_t j = 0; j < lens.size(); j++) {
    const uint64_t stride =
        round4(encode_image_size(lens[j])) + (j % 2 ? 0 : 4 * (1 + j % 3));
    jobs.push_back(gfrs_ejob{off, lens[j], img, stride, 0});
    off += uint64_t(total) * lens[j] + gaps[j % 11];
    img += stride * total + 4 * ((5 * j) % 4);
  }
  return jobs;
}

static void class_of(uint64_t len, int *kind, int *param) {
  if (len <= 4096) {
    *kind = GFRS_EQ_SMALL;
    *param = int((len + 1023) / 1024);
  } else {
    *kind = GFRS_EQ_FRAME;
    *param = len < (uint64_t(1) << 20) ? 87 : 76;
  }
}

static int rank_of(int kind, int param) {
  return kind == GFRS_EQ_SMALL ? param - 1 : (param == 87 ? 4 : 5);
}

static void check_schedule(const char *name,
                           const std::vector<gfrs_ejob> &jobs,
                           const EncSchedule &s) {
  CHECK(s.buckets.size() <= size_t(ENCQ_BUCKETS), "%s: %zu buckets", name,
        s.buckets.size());
  std::vector<int> hits(jobs.size(), 0);
  size_t at = 0, pre = 0;
  int last_rank = -1;
  for (size_t b = 0; b < s.buckets.size(); b++) {
    const EncBucket &bk = s.buckets[b];
    CHECK(bk.first == at && bk.count > 0, "%s: bucket %zu placement", name, b);
    const int rank = rank_of(bk.kind, bk.param);
    CHECK(rank > last_rank, "%s: bucket order", name);
    last_rank = rank;
    if (bk.kind == GFRS_EQ_FRAME) {
      CHECK(bk.prefix == pre && pre + bk.count + 1 <= s.frame_prefix.size(),
            "%s: prefix place of bucket %zu", name, b);
      CHECK(s.frame_prefix[pre] == 0, "%s: prefix start", name);
    }
    int last_job = -1;
    for (size_t i = 0; i < bk.count; i++) {
      const gfrs_eitem &it = s.items[bk.first + i];
      CHECK(it.job > last_job && it.job < int(jobs.size()),
            "%s: caller order in bucket %zu", name, b);
      last_job = it.job;
      const gfrs_ejob &jb = jobs[it.job];
      CHECK(it.off == jb.off && it.shard_len == jb.shard_len &&
                it.img == jb.img_off && it.img_stride == jb.img_stride &&
                it.reserved == 0,
            "%s: item %zu does not carry its job", name, bk.first + i);
      int kind, param;
      class_of(jb.shard_len, &kind, &param);
      CHECK(kind == bk.kind && param == bk.param, "%s: class of job %d", name,
            it.job);
      hits[it.job]++;
      if (bk.kind == GFRS_EQ_FRAME)
        CHECK(s.frame_prefix[pre + i + 1] - s.frame_prefix[pre + i] ==
                  frames(jb.shard_len),
              "%s: frames of job %d", name, it.job);
    }
    if (bk.kind == GFRS_EQ_FRAME) pre += bk.count + 1;
    at += bk.count;
  }
  CHECK(at == s.items.size() && at == jobs.size() &&
            pre == s.frame_prefix.size(),
        "%s: items outside buckets", name);
  for (size_t j = 0; j < jobs.size(); j++)
    CHECK(hits[j] == 1, "%s: job %zu in %d buckets", name, j, hits[j]);
  g_items += long(s.items.size());
}

static void run_case(const char *name, const gfrs_tactic &t,
                     const std::vector<uint64_t> &lens, int want_fused) {
  const int total = t.n + t.m + t.l;
  const std::vector<gfrs_ejob> jobs = layout(total, lens);
  EncSchedule s;
  int rc = encode_queue_schedule(jobs.data(), int(jobs.size()), 0, &s);
  CHECK(rc == GFRS_OK, "%s: schedule rc %d", name, rc);
  check_schedule(name, jobs, s);
  /* a misaligned framed refuses what an aligned one accepts; +4 passes */
  EncSchedule s2;
  CHECK(encode_queue_schedule(jobs.data(), int(jobs.size()), 2, &s2) ==
            GFRS_ERR_INVALID_SHARDS,
        "%s: misaligned framed", name);
  CHECK(encode_queue_schedule(jobs.data(), int(jobs.size()), 0x7000004, &s2) ==
            GFRS_OK,
        "%s: framed at 4", name);

  /* the C export: exact capacity passes, one less refuses */
  const int ni = int(s.items.size());
  for (int shorter = 0; shorter < 2; shorter++) {
    const int cap = ni - shorter;
    std::vector<gfrs_eitem> items(cap);
    std::vector<uint64_t> prefix(size_t(cap) + 2);
    std::vector<gfrs_ebucket> buckets(ENCQ_BUCKETS);
    int gi = -1, gb = -1, fused = -1;
    rc = gfrs_compute_encode_queue_schedule(
        &t, jobs.data(), int(jobs.size()), REPAIR_BLOCK, cap, items.data(),
        prefix.data(), &gi, buckets.data(), &gb, &fused);
    if (shorter) {
      CHECK(rc == GFRS_ERR_NOMEM, "%s: cap %d rc %d", name, cap, rc);
      continue;
    }
    CHECK(rc == GFRS_OK && gi == ni && gb == int(s.buckets.size()) &&
              fused == want_fused,
          "%s: export rc %d fused %d", name, rc, fused);
    size_t nsmall = 0;
    int q = 0;
    for (int b = 0; b < gb; b++) {
      CHECK(buckets[b].kind == s.buckets[b].kind &&
                buckets[b].param == s.buckets[b].param &&
                size_t(buckets[b].first) == s.buckets[b].first &&
                size_t(buckets[b].count) == s.buckets[b].count,
            "%s: export bucket %d", name, b);
      if (buckets[b].kind == GFRS_EQ_SMALL) {
        nsmall += size_t(buckets[b].count);
      } else { /* where the header says the sums are */
        CHECK(size_t(buckets[b].first) - nsmall + q == s.buckets[b].prefix,
              "%s: export prefix place %d", name, b);
        q++;
      }
    }
    for (int i = 0; i < ni; i++)
      CHECK(items[i].job == s.items[i].job && items[i].img == s.items[i].img,
            "%s: export item %d", name, i);
    prefix.resize(s.frame_prefix.size());
    CHECK(prefix == s.frame_prefix, "%s: export prefix", name);
  }
}

static void expect_rc(const gfrs_tactic &t, std::vector<gfrs_ejob> jobs,
                      int64_t block_len, int want, const char *what) {
  std::vector<gfrs_eitem> items(64);
  std::vector<uint64_t> prefix(66);
  std::vector<gfrs_ebucket> buckets(ENCQ_BUCKETS);
  int gi, gb, fused;
  int rc = gfrs_compute_encode_queue_schedule(
      &t, jobs.data(), int(jobs.size()), block_len, 64, items.data(),
      prefix.data(), &gi, buckets.data(), &gb, &fused);
  CHECK(rc == want, "%s: rc %d, want %d", what, rc, want);
}

int main() {
  const gfrs_tactic ec41{4, 1, 0, 1, 4, 0, 2048};
  const gfrs_tactic ec42{4, 2, 0, 1, 5, 0, 2048};
  const gfrs_tactic ec63{6, 3, 0, 1, 8, 0, 2048};
  const gfrs_tactic ec66{6, 6, 0, 3, 11, 0, 2048};
  const gfrs_tactic ec124{12, 4, 0, 1, 15, 0, 2048};
  const gfrs_tactic ec134{13, 4, 0, 1, 16, 0, 2048};
  const gfrs_tactic lrc{12, 2, 2, 2, 14, 0, 2048};
  const gfrs_tactic ec633{6, 3, 3, 3, 9, 0, 2048};
  const std::vector<uint64_t> small{1,    15,   16,   17,   1023, 1024, 1025,
                                    2048, 2049, 3072, 3073, 4095, 4096};
  const std::vector<uint64_t> frame{4097,  8209,  16383, 16385,  49153, 65531,
                                    65532, 65533, 65596, 65597, 131064, 131065};
  const std::vector<uint64_t> large{1048576, 1048577};
  std::vector<uint64_t> mixed;
  for (size_t i = 0; i < small.size() || i < frame.size(); i++) {
    if (i < small.size()) mixed.push_back(small[i]);
    if (i < frame.size()) mixed.push_back(frame[frame.size() - 1 - i]);
    if (i < large.size()) mixed.push_back(large[i]);
  }
  int ncases = 0;
  auto go = [&](const char *name, const gfrs_tactic &t,
                const std::vector<uint64_t> &lens, int fused) {
    run_case(name, t, lens, fused);
    ncases++;
  };
  go("rs63_mixed", ec63, mixed, 1);
  {
    std::vector<uint64_t> lens;
    for (int j = 0; j < 91; j++) lens.push_back(small[(5 * j) % small.size()]);
    go("rs63_small", ec63, lens, 1);
  }
  go("rs42", ec42, mixed, 1);
  go("rs41", ec41, frame, 1);
  go("rs124_k12", ec124, mixed, 1);
  go("lrc_fused", lrc, mixed, 1);
  go("rs66_slow", ec66, mixed, 0);
  go("rs134_w17", ec134, frame, 0);
  go("lrc_slow", ec633, small, 0);
  go("large only", ec63, large, 1);
  go("one job", ec63, {70005}, 1);
  go("one small job", ec63, {1}, 1);
  go("huge shards", ec63, {uint64_t(1) << 40, 1, (uint64_t(1) << 40) + 1}, 1);
  {
    std::vector<uint64_t> lens;
    for (int j = 0; j < 20000; j++) lens.push_back(mixed[(7 * j) % mixed.size()]);
    go("large queue", ec124, lens, 1);
  }
  { /* pseudo-random lengths around every edge */
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (int q = 0; q < 200; q++) {
      std::vector<uint64_t> lens;
      x = x * 6364136223846793005ull + 1442695040888963407ull;
      const int nj = 1 + int((x >> 33) % 50);
      for (int j = 0; j < nj; j++) {
        x = x * 6364136223846793005ull + 1442695040888963407ull;
        const uint64_t r = x >> 20;
        const uint64_t edges[6] = {1024, 4096, 16384, 65532, 131064, 1u << 20};
        lens.push_back(r % 3 ? edges[(r >> 8) % 6] + (r >> 16) % 5 - 2
                             : 1 + (r >> 8) % 300000);
      }
      go("random", ec63, lens, 1);
    }
  }

  /* validation codes */
  CHECK(encode_image_size(100) == 104 && encode_image_size(65532) == 65536 &&
            encode_image_size(65533) == 65541,
        "image size");
  const std::vector<gfrs_ejob> ok{{0, 100, 0, 104, 0}};
  const int64_t B = REPAIR_BLOCK;
  expect_rc(ec63, ok, B, GFRS_OK, "ok");
  expect_rc(ec63, ok, 0, GFRS_ERR_INVALID_BLOCK, "block_len 0");
  expect_rc(ec63, ok, -4096, GFRS_ERR_INVALID_BLOCK, "block_len < 0");
  expect_rc(ec63, ok, 65540, GFRS_ERR_INVALID_BLOCK, "block_len % 4096");
  expect_rc(ec63, ok, 4096, GFRS_ERR_UNSUPPORTED, "block_len 4096");
  expect_rc(ec63, ok, 131072, GFRS_ERR_UNSUPPORTED, "block_len 128K");
  expect_rc(ec63, {}, B, GFRS_ERR_INVALID_SHARDS, "no jobs");
  expect_rc(ec63, {{0, 100, 0, 104, 1}}, B, GFRS_ERR_INVALID_SHARDS,
            "reserved");
  expect_rc(ec63, {{0, 0, 0, 104, 0}}, B, GFRS_ERR_SHARD_NO_DATA, "length 0");
  expect_rc(ec63, {{0, 100, 2, 104, 0}}, B, GFRS_ERR_INVALID_SHARDS,
            "img_off alignment");
  expect_rc(ec63, {{0, 100, 0, 106, 0}}, B, GFRS_ERR_INVALID_SHARDS,
            "img_stride alignment");
  expect_rc(ec63, {{0, 100, 0, 100, 0}}, B, GFRS_ERR_INVALID_SHARDS,
            "img_stride below the image size");
  expect_rc(ec63, {{0, 65533, 0, 65540, 0}}, B, GFRS_ERR_INVALID_SHARDS,
            "second frame's CRC");
  expect_rc(ec63, {{0, 65533, 0, 65544, 0}}, B, GFRS_OK, "two frames");
  expect_rc(ec66, {{0, 0, 0, 104, 0}}, B, GFRS_ERR_SHARD_NO_DATA,
            "slow tactic, length 0");
  expect_rc(ec66, ok, 4096, GFRS_ERR_UNSUPPORTED, "slow tactic, block_len");
  printf("encode queue selftest OK: %d queues, %ld work items\n", ncases,
         g_items);
  return 0;
}
