/* tests/queue_selftest.cpp — stand-alone host check of the repair-queue
 * schedule builder (cubefs_amd/csrc/gfrs_plan.cpp), meant to be built with
 * -fsanitize=address,undefined by a plain host compiler together with
 * gfrs_plan.cpp and gfrs_gf.cpp (tests/test_queue_cpu.py does that).
 *
 * The queues of tests/_repairq.py (same tactics, patterns, lengths and job
 * interleave) plus degenerate ones - one job, all jobs one pattern, every
 * job its own pattern, all jobs slow, a large queue, capacity too small -
 * go through queue_pattern + queue_schedule and through the C export.
 * Every schedule must cover each (job, plan row) exactly once, in a bucket
 * of the right row count, with the items of a bucket grouped by pattern and
 * the tile prefix sums of ceil(shard_len / 4096).
 * Exit status 0 and "queue selftest OK" on success.
 */
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
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

typedef std::vector<std::vector<int32_t>> Patterns;

struct Case {
  const char *name;
  gfrs_tactic t;
  Patterns pats;
  std::vector<gfrs_qjob> jobs;
};

static long g_items = 0, g_buckets = 0;

/* job j: length j mod |lens|, the pattern advancing by one more every
 * |lens| jobs; odd gaps between jobs (tests/_repairq.py) */
static std::vector<gfrs_qjob> interleaved(int total,
                                          const std::vector<uint64_t> &lens,
                                          int npat, int njobs) {
  static const int gaps[11] = {1, 3, 7, 5, 11, 1, 9, 3, 13, 7, 5};
  std::vector<gfrs_qjob> jobs;
  uint64_t off = 0;
  const int nl = int(lens.size());
  for (int j = 0; j < njobs; j++) {
    const uint64_t slen = lens[j % nl];
    jobs.push_back(gfrs_qjob{off, slen, int32_t((j + j / nl) % npat), 0});
    off += uint64_t(total) * slen + gaps[j % 11];
  }
  return jobs;
}

static void flatten(const Patterns &pats, std::vector<int32_t> *bad,
                    std::vector<int32_t> *off) {
  off->assign(1, 0);
  for (const auto &p : pats) {
    bad->insert(bad->end(), p.begin(), p.end());
    off->push_back(int32_t(bad->size()));
  }
}

static void check_schedule(const Case &cs, const std::vector<QueuePattern> &qp,
                           const QueueSchedule &s) {
  const int njobs = int(cs.jobs.size());
  int max_nout = 0;
  for (const auto &q : qp) max_nout = std::max(max_nout, q.nout);
  CHECK(s.buckets.size() <=
            size_t(QUEUE_ROWS) * ((max_nout + QUEUE_ROWS - 1) / QUEUE_ROWS),
        "%s: %zu buckets", cs.name, s.buckets.size());
  CHECK(s.tile_prefix.size() == s.items.size() + s.buckets.size(),
        "%s: prefix size", cs.name);
  std::set<std::pair<int, int>> covered;
  size_t at = 0;
  int last_slot = -1;
  for (size_t b = 0; b < s.buckets.size(); b++) {
    const QueueBucket &bk = s.buckets[b];
    CHECK(bk.first == at && bk.count > 0 && bk.prefix == at + b,
          "%s: bucket %zu placement", cs.name, b);
    CHECK(bk.gm >= 1 && bk.gm <= QUEUE_ROWS && bk.g >= 0, "%s: gm", cs.name);
    CHECK(bk.g * QUEUE_ROWS + bk.gm > last_slot, "%s: bucket order", cs.name);
    last_slot = bk.g * QUEUE_ROWS + bk.gm;
    CHECK(s.tile_prefix[bk.prefix] == 0, "%s: prefix start", cs.name);
    std::set<int> closed;
    int cur = -1;
    for (size_t i = 0; i < bk.count; i++) {
      const gfrs_qitem &it = s.items[bk.first + i];
      CHECK(it.job >= 0 && it.job < njobs, "%s: job index", cs.name);
      const gfrs_qjob &jb = cs.jobs[it.job];
      CHECK(it.off == jb.off && it.shard_len == jb.shard_len &&
                it.pattern == jb.pattern && it.reserved == 0,
            "%s: item %zu does not carry its job", cs.name, bk.first + i);
      CHECK(it.row_off == QUEUE_ROWS * bk.g, "%s: row_off", cs.name);
      CHECK(!qp[it.pattern].slow, "%s: slow job scheduled", cs.name);
      CHECK(bk.gm == std::min(QUEUE_ROWS, qp[it.pattern].nout - it.row_off),
            "%s: gm of job %d step %d", cs.name, it.job, bk.g);
      CHECK(s.tile_prefix[bk.prefix + i + 1] - s.tile_prefix[bk.prefix + i] ==
                (jb.shard_len + QUEUE_TILE - 1) / QUEUE_TILE,
            "%s: tiles of job %d", cs.name, it.job);
      if (it.pattern != cur) {
        CHECK(!closed.count(it.pattern), "%s: pattern %d split", cs.name,
              it.pattern);
        if (cur >= 0) closed.insert(cur);
        cur = it.pattern;
      }
      for (int r = it.row_off; r < it.row_off + bk.gm; r++)
        CHECK(covered.insert({it.job, r}).second, "%s: (%d,%d) twice",
              cs.name, it.job, r);
    }
    at += bk.count;
  }
  CHECK(at == s.items.size(), "%s: items outside buckets", cs.name);
  size_t want = 0, nslow = 0;
  for (int j = 0; j < njobs; j++) {
    const QueuePattern &q = qp[cs.jobs[j].pattern];
    if (q.slow) {
      CHECK(nslow < s.slow_jobs.size() && s.slow_jobs[nslow] == j,
            "%s: slow job %d", cs.name, j);
      nslow++;
    } else {
      want += size_t(q.nout);
    }
  }
  CHECK(nslow == s.slow_jobs.size(), "%s: slow count", cs.name);
  CHECK(covered.size() == want, "%s: covered %zu of %zu rows", cs.name,
        covered.size(), want);
  g_items += long(s.items.size());
  g_buckets += long(s.buckets.size());
}

static void run_case(const Case &cs) {
  Code c;
  CHECK(tactic_valid(&cs.t) && code_build(cs.t, &c), "%s: tactic", cs.name);
  std::vector<QueuePattern> qp(cs.pats.size());
  for (size_t p = 0; p < cs.pats.size(); p++) {
    Plan pl;
    int rc = queue_pattern(c, cs.pats[p].data(), int(cs.pats[p].size()), &pl,
                           &qp[p]);
    CHECK(rc == GFRS_OK, "%s: pattern %zu rc %d", cs.name, p, rc);
    CHECK(qp[p].slow ? pl.out.empty() && qp[p].nout == 0
                     : int(pl.out.size()) == qp[p].nout && qp[p].nout > 0,
          "%s: pattern %zu rows", cs.name, p);
    if (cs.t.l > 0)
      CHECK(qp[p].slow == !lrc_single_pass(c), "%s: slow mark", cs.name);
  }
  QueueSchedule s;
  int rc = queue_schedule(cs.jobs.data(), int(cs.jobs.size()), qp.data(),
                          int(qp.size()), &s);
  CHECK(rc == GFRS_OK, "%s: schedule rc %d", cs.name, rc);
  check_schedule(cs, qp, s);

  /* the C export: exact capacity passes, one less of either refuses */
  std::vector<int32_t> bad, boff;
  flatten(cs.pats, &bad, &boff);
  bad.push_back(0); /* never read */
  const int ni = int(s.items.size()), nb = int(s.buckets.size());
  for (int short_items = 0; short_items < 2; short_items++)
    for (int short_buckets = 0; short_buckets < 2; short_buckets++) {
      const int icap = ni - short_items, bcap = nb - short_buckets;
      if (icap < 0 || bcap < 0) continue;
      std::vector<gfrs_qitem> items(icap);
      std::vector<uint64_t> prefix(size_t(icap) + bcap);
      std::vector<gfrs_qbucket> buckets(bcap);
      std::vector<int32_t> nout(cs.pats.size()), slow_jobs(cs.jobs.size());
      std::vector<uint8_t> slow(cs.pats.size());
      int gi = -1, gb = -1, gs = -1;
      rc = gfrs_compute_queue_schedule(
          &cs.t, cs.jobs.data(), int(cs.jobs.size()), bad.data(), boff.data(),
          int(cs.pats.size()), icap, bcap, items.data(), prefix.data(), &gi,
          buckets.data(), &gb, nout.data(), slow.data(), slow_jobs.data(),
          &gs);
      if (short_items || short_buckets) {
        CHECK(rc == GFRS_ERR_NOMEM, "%s: cap %d/%d rc %d", cs.name, icap,
              bcap, rc);
        continue;
      }
      CHECK(rc == GFRS_OK && gi == ni && gb == nb &&
                gs == int(s.slow_jobs.size()),
            "%s: export rc %d", cs.name, rc);
      for (int i = 0; i < ni; i++)
        CHECK(items[i].job == s.items[i].job &&
                  items[i].row_off == s.items[i].row_off,
              "%s: export item %d", cs.name, i);
      CHECK(prefix == s.tile_prefix, "%s: export prefix", cs.name);
    }
}

static void expect_rc(const gfrs_tactic &t, const Patterns &pats,
                      std::vector<gfrs_qjob> jobs, int want, const char *what) {
  std::vector<int32_t> bad, boff;
  flatten(pats, &bad, &boff);
  bad.push_back(0);
  std::vector<gfrs_qitem> items(64);
  std::vector<uint64_t> prefix(128);
  std::vector<gfrs_qbucket> buckets(64);
  std::vector<int32_t> nout(pats.size() + 1), slow_jobs(jobs.size() + 1);
  std::vector<uint8_t> slow(pats.size() + 1);
  int gi, gb, gs;
  int rc = gfrs_compute_queue_schedule(
      &t, jobs.data(), int(jobs.size()), bad.data(), boff.data(),
      int(pats.size()), 64, 64, items.data(), prefix.data(), &gi,
      buckets.data(), &gb, nout.data(), slow.data(), slow_jobs.data(), &gs);
  CHECK(rc == want, "%s: rc %d, want %d", what, rc, want);
}

int main() {
  const gfrs_tactic ec63{6, 3, 0, 1, 8, 0, 2048};
  const gfrs_tactic ec66{6, 6, 0, 3, 11, 0, 2048};
  const gfrs_tactic ec124{12, 4, 0, 1, 15, 0, 2048};
  const gfrs_tactic ec134{13, 4, 0, 1, 16, 0, 2048};
  const gfrs_tactic lrc{12, 2, 2, 2, 14, 0, 2048};
  const gfrs_tactic ec633{6, 3, 3, 3, 9, 0, 2048};
  const std::vector<uint64_t> lens{1, 15, 16, 17, 33, 4095, 4096, 4097, 8209};

  std::vector<Case> cases;
  cases.push_back({"rs63_mixed", ec63,
                   {{}, {1}, {0, 5}, {0, 2, 4}, {7}, {1, 8}},
                   interleaved(9, lens, 6, 54)});
  cases.push_back({"rs63_uniform", ec63, {{1, 7}},
                   interleaved(9, {4097}, 1, 7)});
  cases.push_back({"rs66_depth", ec66,
                   {{0, 1, 2}, {1, 3, 5, 8}, {0, 1, 2, 3, 4},
                    {0, 1, 2, 3, 4, 5}, {4, 9, 10, 11}},
                   interleaved(12, {17, 4097, 33, 8209, 16}, 5, 20)});
  cases.push_back({"rs124_k12", ec124, {{}, {1}, {0, 13}, {2, 5, 11, 15}},
                   interleaved(16, {4095, 33, 8209, 1, 4096}, 4, 15)});
  cases.push_back({"rs134_w17", ec134, {{16}, {0, 12}, {3}, {1, 2, 14}},
                   interleaved(17, {4097, 15, 8209, 16, 33}, 4, 15)});
  cases.push_back({"lrc_single", lrc,
                   {{}, {0}, {12}, {14}, {3, 15}, {0, 13}},
                   interleaved(16, {33, 4097, 17, 8209}, 6, 24)});
  cases.push_back({"lrc_slow", ec633,
                   {{9}, {11, 0}, {6, 9}, {0, 9, 6}, {}},
                   interleaved(12, {33, 4097, 17}, 5, 10)});
  /* degenerate */
  cases.push_back({"one job", ec63, {{0, 5}}, interleaved(9, {5000}, 1, 1)});
  cases.push_back({"one pattern of two", ec63, {{8}, {2}},
                   interleaved(9, lens, 1, 40)});
  {
    Patterns own;
    for (int i = 0; i < 9; i++) own.push_back({i});
    std::vector<gfrs_qjob> jobs = interleaved(9, {4096, 100}, 9, 9);
    for (int j = 0; j < 9; j++) jobs[j].pattern = 8 - j;
    cases.push_back({"own patterns", ec63, own, jobs});
  }
  cases.push_back({"large", ec66, {{0}, {0, 1, 2, 3, 4, 5}, {7}, {}},
                   interleaved(12, {1, 1u << 20, 4097, 65536}, 4, 5000)});
  cases.push_back({"huge shards", ec63, {{0}},
                   interleaved(9, {uint64_t(1) << 40, 1}, 1, 4)});
  for (const Case &cs : cases) run_case(cs);

  /* validation codes */
  const std::vector<gfrs_qjob> ok{{0, 100, 0, 0}};
  expect_rc(ec63, {{1}}, ok, GFRS_OK, "ok");
  expect_rc(ec63, {{1}}, {}, GFRS_ERR_INVALID_SHARDS, "no jobs");
  expect_rc(ec63, {}, ok, GFRS_ERR_INVALID_SHARDS, "no patterns");
  expect_rc(ec63, {{1}}, {{0, 100, 1, 0}}, GFRS_ERR_INVALID_SHARDS, "pattern");
  expect_rc(ec63, {{1}}, {{0, 100, -1, 0}}, GFRS_ERR_INVALID_SHARDS,
            "negative pattern");
  expect_rc(ec63, {{1}}, {{0, 0, 0, 0}}, GFRS_ERR_SHARD_NO_DATA, "length 0");
  expect_rc(ec63, {{1}}, {{0, 100, 0, 1}}, GFRS_ERR_INVALID_SHARDS, "reserved");
  expect_rc(ec63, {{1}, {9}}, ok, GFRS_ERR_INVALID_SHARDS, "unused pattern");
  expect_rc(ec63, {{1}, {0, 1, 2, 3}}, ok, GFRS_ERR_TOO_FEW_SHARDS, "m+1 bad");
  expect_rc(ec63, {{1, 1}}, ok, GFRS_OK, "RS repeat");
  expect_rc(lrc, {{0, 0}}, ok, GFRS_ERR_INVALID_SHARDS, "LRC repeat");
  expect_rc(lrc, {{0, 1, 2}}, ok, GFRS_ERR_TOO_FEW_SHARDS, "LRC 3 global");
  expect_rc(lrc, {{0, 14, 15}}, ok, GFRS_OK, "LRC locals");
  {
    const int32_t bad[1] = {1}, off_bad[2] = {1, 1}, off_dec[3] = {0, 1, 0};
    CHECK(queue_offsets_check(off_bad, 1) == GFRS_ERR_INVALID_SHARDS, "off0");
    CHECK(queue_offsets_check(off_dec, 2) == GFRS_ERR_INVALID_SHARDS, "dec");
    CHECK(queue_offsets_check(nullptr, 1) == GFRS_ERR_INVALID_SHARDS, "null");
    (void)bad;
  }
  printf("queue selftest OK: %zu queues, %ld work items, %ld buckets\n",
         cases.size(), g_items, g_buckets);
  return 0;
}
