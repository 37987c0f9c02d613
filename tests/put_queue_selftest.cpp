/* tests/put_queue_selftest.cpp — stand-alone host check of the put-queue
 * schedule builder (cubefs_amd/csrc/gfrs_plan.cpp), meant to be built with
 * -fsanitize=address,undefined by a plain host compiler together with
 * gfrs_plan.cpp and gfrs_gf.cpp (tests/test_put_queue_cpu.py does that).
 *
 * Generated queues - the lengths of tests/_putq.py interleaved, one job, a
 * large queue, pseudo-random ones - over narrow and wide tactics go through
 * put_queue_schedule and through the C export.  Every schedule must hold each
 * job in exactly one bucket, of the class and param its length and the
 * tactic's width demand, in caller order, with img = img_off + 32, the frame
 * prefix sums of ceil(shard_len / 65532), the row groups of the tactic and
 * the job-major image table.  Bad arguments must return their codes.  Exit
 * status 0 and "put queue selftest OK" on success.
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
static const int NVOL = 3;

static uint64_t round4(uint64_t n) { return (n + 3) / 4 * 4; }
static uint64_t frames(uint64_t len) { return (len + 65531) / 65532; }
static uint64_t disk_size(uint64_t len) {
  return 32 + len + 4 * frames(len) + 8;
}

static std::vector<uint64_t> vuids_of(int total) {
  std::vector<uint64_t> v;
  for (int i = 0; i < NVOL * total; i++)
    v.push_back((uint64_t(7) << 40) + 131u * unsigned(i));
  return v;
}

/* odd gaps between jobs (data shards only); images back to back at 4-aligned
 * offsets, tight stride for odd jobs, padded for even ones */
static std::vector<gfrs_pjob> layout(int n, int total,
                                     const std::vector<uint64_t> &lens) {
  static const int gaps[11] = {1, 3, 7, 5, 11, 1, 9, 3, 13, 7, 5};
  std::vector<gfrs_pjob> jobs;
  uint64_t off = 0, img = 0;
  for (size_t j = 0; j < lens.size(); j++) {
    const uint64_t stride =
        round4(disk_size(lens[j])) + (j % 2 ? 0 : 4 * (1 + j % 3));
    jobs.push_back(gfrs_pjob{off, lens[j], img, stride,
                             (uint64_t(1) << 40) | (j + 1),
                             int32_t(j % NVOL), 0});
    off += uint64_t(n) * lens[j] + gaps[j % 11];
    img += stride * total + 4 * ((5 * j) % 4);
  }
  return jobs;
}

static void class_of(bool wide, uint64_t len, int *kind, int *param) {
  if (len <= 4096 && !wide) {
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

static void check_schedule(const char *name, const gfrs_tactic &t,
                           const std::vector<gfrs_pjob> &jobs,
                           const std::vector<uint64_t> &vuids,
                           const PutSchedule &ps, bool want_wide) {
  const EncSchedule &s = ps.enc;
  const int total = t.n + t.m + t.l, rows = t.m + t.l;
  CHECK(ps.wide == want_wide, "%s: wide %d", name, int(ps.wide));
  CHECK(int(ps.group_rows.size()) == (rows + 3) / 4, "%s: groups", name);
  int sum = 0;
  for (size_t g = 0; g < ps.group_rows.size(); g++) {
    const int want = g + 1 < ps.group_rows.size() ? 4 : rows - 4 * int(g);
    CHECK(ps.group_rows[g] == want, "%s: rows of group %zu", name, g);
    sum += ps.group_rows[g];
  }
  CHECK(sum == rows, "%s: group rows sum", name);
  CHECK(s.buckets.size() <= size_t(want_wide ? 2 : ENCQ_BUCKETS),
        "%s: %zu buckets", name, s.buckets.size());
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
      const gfrs_pjob &jb = jobs[it.job];
      CHECK(it.off == jb.off && it.shard_len == jb.shard_len &&
                it.img == jb.img_off + 32 && it.img_stride == jb.img_stride &&
                it.reserved == 0,
            "%s: item %zu does not carry its job", name, bk.first + i);
      int kind, param;
      class_of(want_wide, jb.shard_len, &kind, &param);
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
  CHECK(ps.images.size() == jobs.size() * size_t(total), "%s: images", name);
  for (size_t j = 0; j < jobs.size(); j++)
    for (int i = 0; i < total; i++) {
      const gfrs_rimage &im = ps.images[j * total + i];
      CHECK(im.off == jobs[j].img_off + uint64_t(i) * jobs[j].img_stride &&
                im.size == jobs[j].shard_len && im.bid == jobs[j].bid &&
                im.vuid == vuids[size_t(jobs[j].vol) * total + i],
            "%s: image %d of job %zu", name, i, j);
    }
  g_items += long(s.items.size());
}

static void run_case(const char *name, const gfrs_tactic &t,
                     const std::vector<uint64_t> &lens, bool want_wide) {
  const int total = t.n + t.m + t.l;
  Code c;
  CHECK(code_build(t, &c), "%s: code_build", name);
  const std::vector<gfrs_pjob> jobs = layout(t.n, total, lens);
  const std::vector<uint64_t> vuids = vuids_of(total);
  PutSchedule s;
  int rc = put_queue_schedule(c, jobs.data(), int(jobs.size()), vuids.data(),
                              NVOL, 0, &s);
  CHECK(rc == GFRS_OK, "%s: schedule rc %d", name, rc);
  check_schedule(name, t, jobs, vuids, s, want_wide);
  /* a misaligned disk_dst refuses what an aligned one accepts; +4 passes */
  PutSchedule s2;
  CHECK(put_queue_schedule(c, jobs.data(), int(jobs.size()), vuids.data(),
                           NVOL, 2, &s2) == GFRS_ERR_INVALID_SHARDS,
        "%s: misaligned disk_dst", name);
  CHECK(put_queue_schedule(c, jobs.data(), int(jobs.size()), vuids.data(),
                           NVOL, 0x7000004, &s2) == GFRS_OK,
        "%s: disk_dst at 4", name);

  /* the C export: exact capacities pass, one less of either refuses */
  const int ni = int(s.enc.items.size()), nimg = int(s.images.size());
  for (int shorter = 0; shorter < 3; shorter++) {
    const int cap = ni - (shorter == 1), icap = nimg - (shorter == 2);
    std::vector<gfrs_eitem> items(cap);
    std::vector<uint64_t> prefix(size_t(cap) + 2);
    std::vector<gfrs_ebucket> buckets(ENCQ_BUCKETS);
    std::vector<gfrs_rimage> images(icap);
    std::vector<int32_t> grows(64, -1);
    int gi = -1, gb = -1, gimg = -1, wide = -1, ng = -1;
    rc = gfrs_compute_put_queue_schedule(
        &t, jobs.data(), int(jobs.size()), vuids.data(), NVOL, REPAIR_BLOCK,
        cap, icap, items.data(), prefix.data(), &gi, buckets.data(), &gb,
        images.data(), &gimg, &wide, &ng, grows.data());
    if (shorter) {
      CHECK(rc == GFRS_ERR_NOMEM, "%s: caps %d %d rc %d", name, cap, icap, rc);
      continue;
    }
    CHECK(rc == GFRS_OK && gi == ni && gb == int(s.enc.buckets.size()) &&
              gimg == nimg && wide == int(want_wide) &&
              ng == int(s.group_rows.size()),
          "%s: export rc %d wide %d", name, rc, wide);
    for (int g = 0; g < ng; g++)
      CHECK(grows[g] == s.group_rows[g], "%s: export group %d", name, g);
    CHECK(grows[ng] == -1, "%s: export wrote past the groups", name);
    for (int b = 0; b < gb; b++)
      CHECK(buckets[b].kind == s.enc.buckets[b].kind &&
                buckets[b].param == s.enc.buckets[b].param &&
                size_t(buckets[b].first) == s.enc.buckets[b].first &&
                size_t(buckets[b].count) == s.enc.buckets[b].count,
            "%s: export bucket %d", name, b);
    for (int i = 0; i < ni; i++)
      CHECK(items[i].job == s.enc.items[i].job &&
                items[i].img == s.enc.items[i].img,
            "%s: export item %d", name, i);
    for (int i = 0; i < nimg; i++)
      CHECK(images[i].off == s.images[i].off &&
                images[i].vuid == s.images[i].vuid,
            "%s: export image %d", name, i);
    prefix.resize(s.enc.frame_prefix.size());
    CHECK(prefix == s.enc.frame_prefix, "%s: export prefix", name);
  }
}

static void expect_rc(const gfrs_tactic &t, std::vector<gfrs_pjob> jobs,
                      int nvol, int64_t block_len, int want,
                      const char *what) {
  const int total = t.n + t.m + t.l;
  const std::vector<uint64_t> vuids = vuids_of(total);
  std::vector<gfrs_eitem> items(64);
  std::vector<uint64_t> prefix(66);
  std::vector<gfrs_ebucket> buckets(ENCQ_BUCKETS);
  std::vector<gfrs_rimage> images(64 * size_t(total));
  std::vector<int32_t> grows(64);
  int gi, gb, gimg, wide, ng;
  int rc = gfrs_compute_put_queue_schedule(
      &t, jobs.data(), int(jobs.size()), vuids.data(), nvol, block_len, 64,
      64 * total, items.data(), prefix.data(), &gi, buckets.data(), &gb,
      images.data(), &gimg, &wide, &ng, grows.data());
  CHECK(rc == want, "%s: rc %d, want %d", what, rc, want);
}

int main() {
  const gfrs_tactic ec63{6, 3, 0, 1, 8, 0, 2048};
  const gfrs_tactic ec124{12, 4, 0, 1, 15, 0, 2048};
  const gfrs_tactic lrc{12, 2, 2, 2, 14, 0, 2048};
  const gfrs_tactic ec66{6, 6, 0, 3, 11, 0, 2048};
  const gfrs_tactic ec1512{15, 12, 0, 3, 24, 0, 2048};
  const gfrs_tactic ec164{16, 4, 0, 1, 19, 0, 2048};
  const gfrs_tactic ec248{24, 8, 0, 1, 30, 0, 2048};
  const gfrs_tactic ec442{4, 4, 2, 2, 6, 0, 2048};
  const gfrs_tactic ec16202{16, 20, 2, 2, 34, 0, 2048};
  const gfrs_tactic ec324{32, 4, 0, 1, 35, 0, 2048};
  const gfrs_tactic ec334{33, 4, 0, 1, 36, 0, 2048};
  const gfrs_tactic rep3{3, 0, 0, 3, 3, 0, 0};
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
                const std::vector<uint64_t> &lens, bool wide) {
    run_case(name, t, lens, wide);
    ncases++;
  };
  go("rs63", ec63, mixed, false);
  go("rs124", ec124, mixed, false);
  go("lrc narrow", lrc, mixed, false);
  go("rs66", ec66, mixed, true);
  go("rs1512", ec1512, mixed, true);
  go("rs164", ec164, frame, true);
  go("rs248", ec248, {17, 4097, 16385, 65533, 131065}, true);
  go("lrc442", ec442, mixed, true);
  go("lrc16202", ec16202, {17, 65533, 65597}, true);
  go("rs324", ec324, {1, 4097, 65533}, true);
  go("wide, small only", ec66, small, true);
  go("wide, large only", ec66, large, true);
  go("one job", ec1512, {70005}, true);
  go("one small job", ec63, {1}, false);
  go("longest shards", ec66, {0xFFFFFFFFull, 1, 0xFFFFFFFEull}, true);
  {
    std::vector<uint64_t> lens;
    for (int j = 0; j < 5000; j++) lens.push_back(mixed[(7 * j) % mixed.size()]);
    go("large queue", ec1512, lens, true);
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
      go("random", q % 2 ? ec63 : ec66, lens, q % 2 == 0);
    }
  }

  /* validation codes */
  CHECK(disk_size(100) == 144 && repair_image_size(100) == 144 &&
            repair_image_size(65533) == 65533 + 48,
        "disk size");
  const gfrs_pjob good{0, 100, 0, 144, 5, 0, 0};
  const std::vector<gfrs_pjob> ok{good};
  const int64_t B = REPAIR_BLOCK;
  auto with = [&](auto edit) {
    gfrs_pjob j = good;
    edit(j);
    return std::vector<gfrs_pjob>{good, j};
  };
  expect_rc(ec63, ok, NVOL, B, GFRS_OK, "ok");
  expect_rc(ec66, ok, NVOL, B, GFRS_OK, "ok, wide");
  expect_rc(ec324, ok, NVOL, B, GFRS_OK, "ok, n = 32");
  expect_rc(ec63, ok, NVOL, 0, GFRS_ERR_INVALID_BLOCK, "block_len 0");
  expect_rc(ec63, ok, NVOL, -4096, GFRS_ERR_INVALID_BLOCK, "block_len < 0");
  expect_rc(ec63, ok, NVOL, 65540, GFRS_ERR_INVALID_BLOCK, "block_len % 4096");
  expect_rc(ec63, ok, NVOL, 4096, GFRS_ERR_UNSUPPORTED, "block_len 4096");
  expect_rc(ec66, ok, NVOL, 131072, GFRS_ERR_UNSUPPORTED, "block_len 128K");
  expect_rc(ec334, ok, NVOL, B, GFRS_ERR_UNSUPPORTED, "n = 33");
  expect_rc(rep3, ok, NVOL, B, GFRS_ERR_UNSUPPORTED, "replicate");
  expect_rc(ec334, ok, NVOL, 0, GFRS_ERR_INVALID_BLOCK,
            "block_len before the width");
  expect_rc(ec63, {}, NVOL, B, GFRS_ERR_INVALID_SHARDS, "no jobs");
  expect_rc(ec63, ok, 0, B, GFRS_ERR_INVALID_SHARDS, "nvol 0");
  expect_rc(ec63, ok, -1, B, GFRS_ERR_INVALID_SHARDS, "nvol < 0");
  expect_rc(ec63, with([](gfrs_pjob &j) { j.vol = NVOL; }), NVOL, B,
            GFRS_ERR_INVALID_SHARDS, "vol == nvol");
  expect_rc(ec63, with([](gfrs_pjob &j) { j.vol = -1; }), NVOL, B,
            GFRS_ERR_INVALID_SHARDS, "vol < 0");
  expect_rc(ec63, with([](gfrs_pjob &j) { j.vol = NVOL - 1; }), NVOL, B,
            GFRS_OK, "last vol");
  expect_rc(ec63, with([](gfrs_pjob &j) { j.reserved = 1; }), NVOL, B,
            GFRS_ERR_INVALID_SHARDS, "reserved");
  expect_rc(ec66, with([](gfrs_pjob &j) { j.shard_len = 0; }), NVOL, B,
            GFRS_ERR_SHARD_NO_DATA, "length 0");
  expect_rc(ec66, with([](gfrs_pjob &j) {
              j.shard_len = uint64_t(1) << 32;
              j.img_stride = uint64_t(1) << 33;
            }),
            NVOL, B, GFRS_ERR_INVALID_SHARDS, "length 2^32");
  expect_rc(ec63, with([](gfrs_pjob &j) { j.img_off = 2; }), NVOL, B,
            GFRS_ERR_INVALID_SHARDS, "img_off alignment");
  expect_rc(ec63, with([](gfrs_pjob &j) { j.img_stride = 146; }), NVOL, B,
            GFRS_ERR_INVALID_SHARDS, "img_stride alignment");
  expect_rc(ec63, with([](gfrs_pjob &j) { j.img_stride = 140; }), NVOL, B,
            GFRS_ERR_INVALID_SHARDS, "img_stride below the disk size");
  expect_rc(ec63, with([](gfrs_pjob &j) {
              j.shard_len = 65533;
              j.img_stride = 65533 + 47;
            }),
            NVOL, B, GFRS_ERR_INVALID_SHARDS, "second frame's CRC");
  expect_rc(ec63, with([](gfrs_pjob &j) {
              j.shard_len = 65533;
              j.img_stride = 65533 + 51;
            }),
            NVOL, B, GFRS_OK, "two frames");
  printf("put queue selftest OK: %d queues, %ld work items\n", ncases, g_items);
  return 0;
}
