/* tests/shard_read_queue_selftest.cpp — stand-alone host check of the shard
 * read schedule builder (cubefs_amd/csrc/gfrs_plan.cpp), meant to be built
 * with -fsanitize=address,undefined by a plain host compiler together with
 * gfrs_plan.cpp and gfrs_gf.cpp (tests/test_shard_read_queue_cpu.py does
 * that).
 *
 * Pseudo-random queues go through shard_read_schedule and the C export: every
 * job must sit once in the bucket of its NO_OUT flag, storing bucket first,
 * items in caller order, prefix sums counting touched frames, frame bases
 * and per-job frame places partitioning [0, total_frames).  Bad arguments must
 * return their codes and leave the schedule empty.  Exit status 0 and
 * "shard read queue selftest OK" on success.
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

static uint64_t g_rng = 0xD1B54A32D192ED03ull;
static uint64_t rnd(uint64_t n) {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return g_rng % n;
}

static uint64_t touched(const gfrs_sjob &j) {
  return (j.to - 1) / 65532 - j.from / 65532 + 1;
}

static gfrs_sjob random_job(uint64_t *img, uint64_t *out) {
  static const uint64_t pick[] = {1,     3,     4,      5,      17,    4096,
                                  65531, 65532, 65533,  65597,  131064,
                                  131065, 200000, 1 << 20, 0xFFFFFFFFull};
  gfrs_sjob j{};
  j.size = rnd(3) ? pick[rnd(sizeof(pick) / sizeof(pick[0]))]
                  : 1 + rnd(300000);
  j.img_off = *img;
  j.bid = rnd(~0ull);
  j.vuid = rnd(~0ull);
  j.flags = uint32_t(rnd(4));
  if (j.flags & GFRS_SJOB_FOOTER) {
    j.from = 0;
    j.to = j.size;
  } else {
    j.from = 4 * rnd((j.size + 3) / 4);
    j.to = j.from + 1 + rnd(j.size - j.from);
  }
  j.out_off = (j.flags & GFRS_SJOB_NO_OUT) ? rnd(1000) : *out;
  *img += 40 + j.size + 4 * ((j.size - 1) / 65532 + 1) + rnd(7);
  *out += (j.to - j.from + 3) / 4 * 4 + 4 * rnd(4);
  return j;
}

static void check_queue(const std::vector<gfrs_sjob> &jobs) {
  const int nj = int(jobs.size());
  ShardReadSchedule s;
  int rc = shard_read_schedule(jobs.data(), nj, 0x1000, true, &s);
  CHECK(rc == GFRS_OK, "rc %d", rc);
  size_t count[2] = {0, 0};
  for (const gfrs_sjob &j : jobs) count[j.flags & GFRS_SJOB_NO_OUT]++;
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
    const ShardReadBucket &bk = s.buckets[b];
    CHECK(bk.no_out > last_kind, "bucket order");
    last_kind = bk.no_out;
    CHECK(bk.first == at && bk.count == count[bk.no_out], "bucket extent");
    CHECK(bk.prefix == at + b, "prefix place");
    CHECK(bk.frame_base == frames, "frame base");
    CHECK(s.frame_prefix[bk.prefix] == 0, "prefix start");
    int prev = -1;
    for (size_t i = 0; i < bk.count; i++) {
      const gfrs_sitem &it = s.items[at + i];
      CHECK(it.job > prev && it.job < nj, "caller order");
      prev = it.job;
      const gfrs_sjob &j = jobs[it.job];
      CHECK(!seen[it.job]++, "job twice");
      CHECK(int(j.flags & GFRS_SJOB_NO_OUT) == bk.no_out, "wrong bucket");
      CHECK(it.img == j.img_off && it.size == j.size && it.from == j.from &&
                it.to == j.to && it.out == j.out_off && it.flags == j.flags,
            "item fields");
      CHECK(s.frame_prefix[bk.prefix + i + 1] - s.frame_prefix[bk.prefix + i] ==
                touched(j),
            "touched frames of job %d", it.job);
      CHECK(s.job_frame[it.job] == frames + s.frame_prefix[bk.prefix + i],
            "frame place of job %d", it.job);
      CHECK(shard_last_frame(j) - shard_first_frame(j) + 1 == touched(j),
            "frame helpers");
      g_items++;
    }
    frames += s.frame_prefix[bk.prefix + bk.count];
    at += bk.count;
  }
  CHECK(frames == s.total_frames, "total frames");

  /* the C export tells the same */
  std::vector<gfrs_sitem> items(nj);
  std::vector<uint64_t> prefix(nj + 2);
  gfrs_sbucket bks[2];
  int ni = -1, nb = -1;
  uint64_t tot = ~0ull;
  rc = gfrs_compute_shard_read_queue_schedule(jobs.data(), nj, 65536, nj,
                                              items.data(), prefix.data(), &ni,
                                              bks, &nb, &tot);
  CHECK(rc == GFRS_OK && ni == nj && nb == int(s.buckets.size()) &&
            tot == s.total_frames,
        "export rc %d", rc);
  for (int i = 0; i < ni; i++)
    CHECK(items[i].job == s.items[i].job && items[i].out == s.items[i].out,
          "export item %d", i);
  for (size_t i = 0; i < s.frame_prefix.size(); i++)
    CHECK(prefix[i] == s.frame_prefix[i], "export prefix %zu", i);
  for (int b = 0; b < nb; b++)
    CHECK(bks[b].no_out == s.buckets[b].no_out &&
              bks[b].first == int(s.buckets[b].first) &&
              bks[b].count == int(s.buckets[b].count) && bks[b].reserved == 0,
          "export bucket %d", b);
  if (nj > 1) {
    rc = gfrs_compute_shard_read_queue_schedule(jobs.data(), nj, 65536, nj - 1,
                                                items.data(), prefix.data(),
                                                &ni, bks, &nb, &tot);
    CHECK(rc == GFRS_ERR_NOMEM, "capacity rc %d", rc);
  }
  g_queues++;
}

static void refuse(gfrs_sjob j, int want, uint64_t out_addr = 0,
                   bool have_out = true) {
  ShardReadSchedule s;
  gfrs_sjob ok{};
  ok.size = 100;
  ok.to = 100;
  ok.flags = GFRS_SJOB_NO_OUT;
  const gfrs_sjob two[2] = {ok, j};
  const int rc = shard_read_schedule(two, 2, out_addr, have_out, &s);
  CHECK(rc == want, "rc %d want %d", rc, want);
  if (want != GFRS_OK)
    CHECK(s.items.empty() && s.buckets.empty() && s.total_frames == 0,
          "schedule left behind");
  g_refused += want != GFRS_OK;
}

int main() {
  for (int q = 0; q < 400; q++) {
    std::vector<gfrs_sjob> jobs;
    uint64_t img = rnd(64), out = 4 * rnd(9);
    const int nj = 1 + int(rnd(q % 4 == 0 ? 300 : 12));
    const int force = q % 5; /* 1: all NO_OUT, 2: none */
    for (int i = 0; i < nj; i++) {
      gfrs_sjob j = random_job(&img, &out);
      if (force == 1) j.flags |= GFRS_SJOB_NO_OUT;
      if (force == 2 && (j.flags & GFRS_SJOB_NO_OUT)) {
        j.flags &= ~uint32_t(GFRS_SJOB_NO_OUT);
        j.out_off = 4 * rnd(1000);
      }
      jobs.push_back(j);
    }
    check_queue(jobs);
  }

  gfrs_sjob ok{};
  ok.size = 131065;
  ok.from = 4;
  ok.to = 131065;
  ok.out_off = 8;
  refuse(ok, GFRS_OK);
  gfrs_sjob j = ok;
  j.size = 0; refuse(j, GFRS_ERR_SHARD_NO_DATA);
  j = ok; j.size = 1ull << 32; j.to = j.size; refuse(j, GFRS_ERR_INVALID_SHARDS);
  j = ok; j.size = 0xFFFFFFFFull; j.to = j.size; refuse(j, GFRS_OK);
  j = ok; j.reserved = 1; refuse(j, GFRS_ERR_INVALID_SHARDS);
  j = ok; j.flags = 4; refuse(j, GFRS_ERR_INVALID_SHARDS);
  j = ok; j.flags = 0x80000001u; refuse(j, GFRS_ERR_INVALID_SHARDS);
  j = ok; j.from = j.to; refuse(j, GFRS_ERR_INVALID_SHARDS);
  j = ok; j.from = 8; j.to = 4; refuse(j, GFRS_ERR_INVALID_SHARDS);
  j = ok; j.to = j.size + 1; refuse(j, GFRS_ERR_INVALID_SHARDS);
  j = ok; j.from = 2; refuse(j, GFRS_ERR_INVALID_SHARDS);
  j = ok; j.from = ~0ull - 3; j.to = ~0ull; refuse(j, GFRS_ERR_INVALID_SHARDS);
  j = ok; j.flags = GFRS_SJOB_FOOTER; refuse(j, GFRS_ERR_INVALID_SHARDS);
  j = ok; j.flags = GFRS_SJOB_FOOTER; j.from = 0; j.to = 8;
  refuse(j, GFRS_ERR_INVALID_SHARDS);
  j = ok; j.flags = GFRS_SJOB_FOOTER; j.from = 0; refuse(j, GFRS_OK);
  j = ok; j.out_off = 6; refuse(j, GFRS_ERR_INVALID_SHARDS);
  j = ok; j.out_off = 6; refuse(j, GFRS_OK, 2);
  j = ok; refuse(j, GFRS_ERR_INVALID_SHARDS, 2);
  j = ok; j.out_off = 7; j.flags = GFRS_SJOB_NO_OUT; refuse(j, GFRS_OK);
  /* a NULL out: only when nobody stores */
  j = ok; refuse(j, GFRS_ERR_INVALID_SHARDS, 0, false);
  j = ok; j.flags = GFRS_SJOB_NO_OUT; refuse(j, GFRS_OK, 0, false);
  {
    ShardReadSchedule s;
    j = ok;
    j.flags = GFRS_SJOB_NO_OUT;
    CHECK(shard_read_schedule(&j, 1, 0, false, &s) == GFRS_OK, "null out");
    CHECK(s.buckets.size() == 1 && s.buckets[0].no_out == 1 &&
              s.total_frames == 3,
          "null out schedule");
    CHECK(shard_read_schedule(&j, 0, 0, true, &s) == GFRS_ERR_INVALID_SHARDS,
          "njobs 0");
    CHECK(shard_read_schedule(&j, -1, 0, true, &s) == GFRS_ERR_INVALID_SHARDS,
          "njobs -1");
    CHECK(shard_read_schedule(nullptr, 1, 0, true, &s) ==
              GFRS_ERR_INVALID_SHARDS,
          "null jobs");
  }
  {
    gfrs_sitem it;
    uint64_t pre[3], tot;
    gfrs_sbucket bk[2];
    int ni, nb;
    const int64_t bad_bl[] = {0, -65536, 100, 65540};
    for (int64_t bl : bad_bl)
      CHECK(gfrs_compute_shard_read_queue_schedule(&ok, 1, bl, 1, &it, pre, &ni,
                                                   bk, &nb, &tot) ==
                GFRS_ERR_INVALID_BLOCK,
            "block %lld", (long long)bl);
    const int64_t uns_bl[] = {4096, 131072, 3 * 65536};
    for (int64_t bl : uns_bl)
      CHECK(gfrs_compute_shard_read_queue_schedule(&ok, 1, bl, 1, &it, pre, &ni,
                                                   bk, &nb, &tot) ==
                GFRS_ERR_UNSUPPORTED,
            "block %lld", (long long)bl);
  }
  CHECK(g_queues == 400 && g_items > 5000 && g_refused >= 14,
        "coverage %ld %ld %ld", g_queues, g_items, g_refused);
  printf("shard read queue selftest OK: %ld queues, %ld items, %ld refusals\n",
         g_queues, g_items, g_refused);
  return 0;
}
