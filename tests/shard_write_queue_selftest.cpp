/* tests/shard_write_queue_selftest.cpp — stand-alone host check of the shard
 * write schedule builder (cubefs_amd/csrc/gfrs_plan.cpp), meant to be built
 * with -fsanitize=address,undefined by a plain host compiler together with
 * gfrs_plan.cpp and gfrs_gf.cpp (tests/test_shard_write_queue_cpu.py does
 * that).
 *
 * Pseudo-random queues go through shard_write_schedule and the C export:
 * every job must sit once in the bucket of its SRC_IMAGE flag, raw bucket
 * first, items in caller order, prefix sums counting ceil(size / 65532)
 * frames, frame bases and per-job frame places partitioning
 * [0, total_frames).  Bad arguments must return their codes and leave the
 * schedule empty.  Exit status 0 and "shard write queue selftest OK" on
 * success.
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

static long g_queues = 0, g_items = 0, g_refused = 0;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd(uint64_t n) {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return g_rng % n;
}

static uint64_t frames_of(const gfrs_wjob &j) { return (j.size - 1) / 65532 + 1; }

static gfrs_wjob random_job(uint64_t *src, uint64_t *img) {
  static const uint64_t pick[] = {1,     3,     4,      5,      17,    4096,
                                  65531, 65532, 65533,  65597,  131064,
                                  131065, 200000, 1 << 20, 0xFFFFFFFFull};
  gfrs_wjob j{};
  j.size = rnd(3) ? pick[rnd(sizeof(pick) / sizeof(pick[0]))]
                  : 1 + rnd(300000);
  j.src_off = *src;
  j.bid = rnd(~0ull);
  j.vuid = rnd(~0ull);
  j.src_bid = rnd(~0ull);
  j.src_vuid = rnd(~0ull);
  j.flags = uint32_t(rnd(2));
  j.img_off = *img;
  const uint64_t disk = 40 + j.size + 4 * frames_of(j);
  *src += ((j.flags & GFRS_WJOB_SRC_IMAGE) ? disk : j.size) + rnd(7);
  *img += (disk + 3) / 4 * 4 + 4 * rnd(4);
  return j;
}

static void check_queue(const std::vector<gfrs_wjob> &jobs) {
  const int nj = int(jobs.size());
  ShardWriteSchedule s;
  int rc = shard_write_schedule(jobs.data(), nj, 0x1000, &s);
  CHECK(rc == GFRS_OK, "rc %d", rc);
  size_t count[2] = {0, 0};
  for (const gfrs_wjob &j : jobs) count[j.flags & GFRS_WJOB_SRC_IMAGE]++;
  CHECK(s.buckets.size() == size_t((count[0] != 0) + (count[1] != 0)),
        "%zu buckets", s.buckets.size());
  CHECK(s.items.size() == size_t(nj), "%zu items", s.items.size());
  CHECK(s.frame_prefix.size() == size_t(nj) + s.buckets.size(), "prefix size");
  CHECK(s.job_frame.size() == size_t(nj), "job_frame size");
  size_t at = 0;
  uint64_t frames = 0;
  int last_kind = -1;
  std::vector<int> seen(nj, 0);
  for (size_t b = 0; b < s.buckets.size(); b++) {
    const ShardWriteBucket &bk = s.buckets[b];
    CHECK(bk.src_image > last_kind, "bucket order");
    last_kind = bk.src_image;
    CHECK(bk.first == at && bk.count == count[bk.src_image], "bucket extent");
    CHECK(bk.prefix == at + b, "prefix place");
    CHECK(bk.frame_base == frames, "frame base");
    CHECK(s.frame_prefix[bk.prefix] == 0, "prefix start");
    int prev = -1;
    for (size_t i = 0; i < bk.count; i++) {
      const gfrs_witem &it = s.items[at + i];
      CHECK(it.job > prev && it.job < nj, "caller order");
      prev = it.job;
      const gfrs_wjob &j = jobs[it.job];
      CHECK(!seen[it.job]++, "job twice");
      CHECK(int(j.flags & GFRS_WJOB_SRC_IMAGE) == bk.src_image,
            "wrong bucket");
      CHECK(it.src == j.src_off && it.size == j.size && it.img == j.img_off &&
                it.flags == j.flags,
            "item fields");
      CHECK(s.frame_prefix[bk.prefix + i + 1] - s.frame_prefix[bk.prefix + i] ==
                frames_of(j),
            "frames of job %d", it.job);
      CHECK(s.job_frame[it.job] == frames + s.frame_prefix[bk.prefix + i],
            "frame place of job %d", it.job);
      g_items++;
    }
    frames += s.frame_prefix[bk.prefix + bk.count];
    at += bk.count;
  }
  CHECK(frames == s.total_frames, "total frames");

  /* the C export tells the same */
  std::vector<gfrs_witem> items(nj);
  std::vector<uint64_t> prefix(nj + 2);
  gfrs_wbucket bks[2];
  int ni = -1, nb = -1;
  uint64_t tot = ~0ull;
  rc = gfrs_compute_shard_write_queue_schedule(jobs.data(), nj, 65536, nj,
                                               items.data(), prefix.data(),
                                               &ni, bks, &nb, &tot);
  CHECK(rc == GFRS_OK && ni == nj && nb == int(s.buckets.size()) &&
            tot == s.total_frames,
        "export rc %d", rc);
  for (int i = 0; i < ni; i++)
    CHECK(items[i].job == s.items[i].job && items[i].img == s.items[i].img &&
              items[i].src == s.items[i].src,
          "export item %d", i);
  for (size_t i = 0; i < s.frame_prefix.size(); i++)
    CHECK(prefix[i] == s.frame_prefix[i], "export prefix %zu", i);
  for (int b = 0; b < nb; b++)
    CHECK(bks[b].src_image == s.buckets[b].src_image &&
              bks[b].first == int(s.buckets[b].first) &&
              bks[b].count == int(s.buckets[b].count) && bks[b].reserved == 0,
          "export bucket %d", b);
  if (nj > 1) {
    rc = gfrs_compute_shard_write_queue_schedule(jobs.data(), nj, 65536,
                                                 nj - 1, items.data(),
                                                 prefix.data(), &ni, bks, &nb,
                                                 &tot);
    CHECK(rc == GFRS_ERR_NOMEM, "capacity rc %d", rc);
  }
  g_queues++;
}

static void refuse(gfrs_wjob j, int want, uint64_t dst_addr = 0) {
  ShardWriteSchedule s;
  gfrs_wjob ok{};
  ok.size = 100;
  ok.img_off = (4 - dst_addr % 4) % 4;
  const gfrs_wjob two[2] = {ok, j};
  const int rc = shard_write_schedule(two, 2, dst_addr, &s);
  CHECK(rc == want, "rc %d want %d", rc, want);
  if (want != GFRS_OK)
    CHECK(s.items.empty() && s.buckets.empty() && s.total_frames == 0,
          "schedule left behind");
  g_refused += want != GFRS_OK;
}

int main() {
  for (int q = 0; q < 400; q++) {
    std::vector<gfrs_wjob> jobs;
    uint64_t src = rnd(64), img = 4 * rnd(9);
    const int nj = 1 + int(rnd(q % 4 == 0 ? 300 : 12));
    const int force = q % 5; /* 1: all SRC_IMAGE, 2: all raw */
    for (int i = 0; i < nj; i++) {
      gfrs_wjob j = random_job(&src, &img);
      if (force == 1) j.flags |= GFRS_WJOB_SRC_IMAGE;
      if (force == 2) j.flags = 0;
      jobs.push_back(j);
    }
    check_queue(jobs);
  }

  gfrs_wjob ok{};
  ok.size = 131065;
  ok.src_off = 3;
  ok.img_off = 8;
  refuse(ok, GFRS_OK);
  gfrs_wjob j = ok;
  j.size = 0; refuse(j, GFRS_ERR_SHARD_NO_DATA);
  j = ok; j.size = 1ull << 32; refuse(j, GFRS_ERR_INVALID_SHARDS);
  j = ok; j.size = 0xFFFFFFFFull; refuse(j, GFRS_OK);
  j = ok; j.reserved = 1; refuse(j, GFRS_ERR_INVALID_SHARDS);
  j = ok; j.flags = 2; refuse(j, GFRS_ERR_INVALID_SHARDS);
  j = ok; j.flags = 0x80000001u; refuse(j, GFRS_ERR_INVALID_SHARDS);
  j = ok; j.flags = GFRS_WJOB_SRC_IMAGE; refuse(j, GFRS_OK);
  j = ok; j.img_off = 6; refuse(j, GFRS_ERR_INVALID_SHARDS);
  j = ok; j.img_off = 1; refuse(j, GFRS_ERR_INVALID_SHARDS);
  j = ok; j.img_off = 6; refuse(j, GFRS_OK, 2);
  j = ok; refuse(j, GFRS_ERR_INVALID_SHARDS, 2);
  j = ok; j.img_off = 7; j.flags = GFRS_WJOB_SRC_IMAGE;
  refuse(j, GFRS_ERR_INVALID_SHARDS);
  j = ok; j.src_off = ~0ull; refuse(j, GFRS_OK); /* not the builder's matter */
  {
    ShardWriteSchedule s;
    j = ok;
    j.flags = GFRS_WJOB_SRC_IMAGE;
    CHECK(shard_write_schedule(&j, 1, 0, &s) == GFRS_OK, "one job");
    CHECK(s.buckets.size() == 1 && s.buckets[0].src_image == 1 &&
              s.total_frames == 3 && s.job_frame[0] == 0,
          "one job schedule");
    CHECK(shard_write_schedule(&j, 0, 0, &s) == GFRS_ERR_INVALID_SHARDS,
          "njobs 0");
    CHECK(shard_write_schedule(&j, -1, 0, &s) == GFRS_ERR_INVALID_SHARDS,
          "njobs -1");
    CHECK(shard_write_schedule(nullptr, 1, 0, &s) == GFRS_ERR_INVALID_SHARDS,
          "null jobs");
  }
  {
    gfrs_witem it;
    uint64_t pre[3], tot;
    gfrs_wbucket bk[2];
    int ni, nb;
    const int64_t bad_bl[] = {0, -65536, 100, 65540};
    for (int64_t bl : bad_bl)
      CHECK(gfrs_compute_shard_write_queue_schedule(&ok, 1, bl, 1, &it, pre,
                                                    &ni, bk, &nb, &tot) ==
                GFRS_ERR_INVALID_BLOCK,
            "block %lld", (long long)bl);
    const int64_t uns_bl[] = {4096, 131072, 3 * 65536};
    for (int64_t bl : uns_bl)
      CHECK(gfrs_compute_shard_write_queue_schedule(&ok, 1, bl, 1, &it, pre,
                                                    &ni, bk, &nb, &tot) ==
                GFRS_ERR_UNSUPPORTED,
            "block %lld", (long long)bl);
  }
  CHECK(g_queues == 400 && g_items > 5000 && g_refused >= 8,
        "coverage %ld %ld %ld", g_queues, g_items, g_refused);
  printf("shard write queue selftest OK: %ld queues, %ld items, %ld refusals\n",
         g_queues, g_items, g_refused);
  return 0;
}
