/* tests/repair_queue_selftest.cpp — stand-alone host check of the
 * repair-image schedule builder (cubefs_amd/csrc/gfrs_plan.cpp), meant to be
 * built with -fsanitize=address,undefined by a plain host compiler together
 * with gfrs_plan.cpp and gfrs_gf.cpp (tests/test_repair_queue_cpu.py does
 * that).
 *
 * The queues of tests/_repairimgq.py (same tactics, patterns, lengths and job
 * interleave; the images packed back to back here) plus degenerate ones - one
 * job, all jobs one pattern, every job its own pattern, a large queue,
 * capacity too small - go through repair_pattern + repair_schedule and
 * through the C export.  Every schedule must cover each (job, bad shard)
 * exactly once, by a fused item of its pattern's row count or by an identity
 * item in the 1-row bucket, with at most one bucket per row count, items
 * ordered by descriptor then caller index, the frame prefix sums of
 * ceil(shard_len / 65532) and an image table in id order.
 * Exit status 0 and "repair queue selftest OK" on success.
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
  std::vector<gfrs_rjob> jobs;
};

static long g_items = 0, g_images = 0;

static uint64_t round4(uint64_t n) { return (n + 3) / 4 * 4; }

/* job j: length j mod |lens|, the pattern advancing by one more every |lens|
 * jobs, odd gaps between jobs (tests/_repairq.py); images back to back at
 * 4-aligned offsets, tight stride for odd jobs, padded for even ones */
static std::vector<gfrs_rjob> interleaved(int total, const Patterns &pats,
                                          const std::vector<uint64_t> &lens,
                                          int njobs) {
  static const int gaps[11] = {1, 3, 7, 5, 11, 1, 9, 3, 13, 7, 5};
  std::vector<gfrs_rjob> jobs;
  uint64_t off = 0, img = 0;
  const int nl = int(lens.size()), npat = int(pats.size());
  for (int j = 0; j < njobs; j++) {
    const uint64_t slen = lens[j % nl];
    const int pat = (j + j / nl) % npat;
    const uint64_t stride =
        round4(repair_image_size(slen)) + (j % 2 ? 0 : 4 * (1 + j % 3));
    jobs.push_back(gfrs_rjob{off, slen, img, stride, int32_t(pat), 0});
    off += uint64_t(total) * slen + gaps[j % 11];
    img += stride * pats[pat].size() + 4 * ((5 * j) % 4);
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

static void check_schedule(const Case &cs, const std::vector<RepairPattern> &rp,
                           const std::vector<uint64_t> &bids,
                           const RepairSchedule &s) {
  const int njobs = int(cs.jobs.size()), npat = int(cs.pats.size());
  const int total = cs.t.n + cs.t.m + cs.t.l;
  CHECK(s.buckets.size() <= size_t(REPAIR_ROWS), "%s: %zu buckets", cs.name,
        s.buckets.size());
  CHECK(s.frame_prefix.size() == s.items.size() + s.buckets.size(),
        "%s: prefix size", cs.name);
  std::set<std::pair<int, int>> covered;
  size_t at = 0;
  int last_gm = 0;
  for (size_t b = 0; b < s.buckets.size(); b++) {
    const RepairBucket &bk = s.buckets[b];
    CHECK(bk.first == at && bk.count > 0 && bk.prefix == at + b,
          "%s: bucket %zu placement", cs.name, b);
    CHECK(bk.gm > last_gm && bk.gm <= REPAIR_ROWS, "%s: bucket order", cs.name);
    last_gm = bk.gm;
    CHECK(s.frame_prefix[bk.prefix] == 0, "%s: prefix start", cs.name);
    std::pair<int, int> last_key{-1, -1};
    for (size_t i = 0; i < bk.count; i++) {
      const gfrs_ritem &it = s.items[bk.first + i];
      CHECK(it.job >= 0 && it.job < njobs, "%s: job index", cs.name);
      const gfrs_rjob &jb = cs.jobs[it.job];
      const std::vector<int32_t> &bad = cs.pats[jb.pattern];
      CHECK(it.off == jb.off && it.shard_len == jb.shard_len &&
                it.img_stride == jb.img_stride,
            "%s: item %zu does not carry its job", cs.name, bk.first + i);
      CHECK(s.frame_prefix[bk.prefix + i + 1] - s.frame_prefix[bk.prefix + i] ==
                (jb.shard_len + REPAIR_PAYLOAD - 1) / REPAIR_PAYLOAD,
            "%s: frames of job %d", cs.name, it.job);
      const std::pair<int, int> key{it.desc, it.job};
      CHECK(key > last_key, "%s: item order in bucket %zu", cs.name, b);
      last_key = key;
      if (it.desc < npat) {
        CHECK(it.desc == jb.pattern && rp[jb.pattern].cls == GFRS_RPAT_FUSED &&
                  bk.gm == rp[jb.pattern].gm && it.img == jb.img_off,
              "%s: fused item of job %d", cs.name, it.job);
        for (int32_t idx : bad)
          CHECK(covered.insert({it.job, idx}).second, "%s: (%d,%d) twice",
                cs.name, it.job, idx);
      } else {
        const int idx = it.desc - npat;
        const auto pos = std::find(bad.begin(), bad.end(), idx);
        CHECK(idx < total && pos != bad.end() && bk.gm == 1 &&
                  rp[jb.pattern].cls != GFRS_RPAT_FUSED,
              "%s: identity item of job %d", cs.name, it.job);
        CHECK(it.img == jb.img_off + uint64_t(pos - bad.begin()) * jb.img_stride,
              "%s: identity image of job %d", cs.name, it.job);
        CHECK(covered.insert({it.job, idx}).second, "%s: (%d,%d) twice",
              cs.name, it.job, idx);
      }
    }
    at += bk.count;
  }
  CHECK(at == s.items.size(), "%s: items outside buckets", cs.name);
  size_t want = 0, nin = 0;
  for (int j = 0; j < njobs; j++) {
    const gfrs_rjob &jb = cs.jobs[j];
    const RepairPattern &r = rp[jb.pattern];
    for (int b = 0; b < r.nbad; b++) {
      CHECK(want < s.images.size(), "%s: image table short", cs.name);
      const gfrs_rimage &im = s.images[want];
      CHECK(im.off == jb.img_off + uint64_t(b) * jb.img_stride &&
                im.size == jb.shard_len && im.bid == bids[want] &&
                im.vuid == bids[want] + 7,
            "%s: image %zu", cs.name, want);
      want++;
    }
    if (r.cls != GFRS_RPAT_FUSED) {
      CHECK(nin < s.inplace_jobs.size() && s.inplace_jobs[nin] == j,
            "%s: in-place job %d", cs.name, j);
      nin++;
    }
  }
  CHECK(want == s.images.size() && nin == s.inplace_jobs.size() &&
            covered.size() == want,
        "%s: covered %zu of %zu", cs.name, covered.size(), want);
  g_items += long(s.items.size());
  g_images += long(s.images.size());
}

static void run_case(const Case &cs) {
  Code c;
  CHECK(tactic_valid(&cs.t) && code_build(cs.t, &c), "%s: tactic", cs.name);
  std::vector<RepairPattern> rp(cs.pats.size());
  for (size_t p = 0; p < cs.pats.size(); p++) {
    Plan pl;
    const int nbad = int(cs.pats[p].size());
    int rc = repair_pattern(c, cs.pats[p].data(), nbad, &pl, &rp[p]);
    CHECK(rc == GFRS_OK && rp[p].nbad == nbad, "%s: pattern %zu rc %d",
          cs.name, p, rc);
    if (rp[p].cls == GFRS_RPAT_FUSED) {
      uint32_t colpack = 0;
      CHECK(repair_colpack(c.total, cs.pats[p].data(), nbad, &colpack) ==
                    GFRS_OK &&
                colpack == rp[p].colpack && colpack == pl.colpack,
            "%s: colpack of pattern %zu", cs.name, p);
      CHECK(int(pl.out.size()) == rp[p].gm && rp[p].gm >= nbad &&
                rp[p].gm <= REPAIR_ROWS && rp[p].nw == nbad &&
                rp[p].gm == cs.t.m + cs.t.l,
            "%s: rows of pattern %zu", cs.name, p);
    } else {
      CHECK(pl.out.empty() && rp[p].gm == 0, "%s: in-place pattern %zu",
            cs.name, p);
      CHECK((rp[p].cls == GFRS_RPAT_INPLACE_SLOW) == (cs.t.l > 0),
            "%s: slow mark", cs.name);
    }
  }
  std::vector<int32_t> bad, boff;
  flatten(cs.pats, &bad, &boff);
  bad.push_back(0); /* never read */
  size_t nimg = 0;
  for (const auto &jb : cs.jobs) nimg += cs.pats[jb.pattern].size();
  std::vector<uint64_t> bids(nimg), vuids(nimg);
  for (size_t i = 0; i < nimg; i++) {
    bids[i] = 9000 + 3 * i;
    vuids[i] = bids[i] + 7;
  }
  RepairSchedule s;
  int rc = repair_schedule(cs.jobs.data(), int(cs.jobs.size()), rp.data(),
                           int(rp.size()), bad.data(), boff.data(), 0,
                           bids.data(), vuids.data(), &s);
  CHECK(rc == GFRS_OK, "%s: schedule rc %d", cs.name, rc);
  check_schedule(cs, rp, bids, s);
  /* a misaligned disk_dst refuses what an aligned one accepts */
  RepairSchedule s2;
  CHECK(repair_schedule(cs.jobs.data(), int(cs.jobs.size()), rp.data(),
                        int(rp.size()), bad.data(), boff.data(), 2,
                        bids.data(), vuids.data(), &s2) ==
            GFRS_ERR_INVALID_SHARDS,
        "%s: misaligned disk_dst", cs.name);

  /* the C export: exact capacity passes, one less of either refuses */
  const int ni = int(s.items.size()), nim = int(s.images.size());
  for (int short_items = 0; short_items < 2; short_items++)
    for (int short_images = 0; short_images < 2; short_images++) {
      const int icap = ni - short_items, mcap = nim - short_images;
      std::vector<gfrs_ritem> items(icap);
      std::vector<uint64_t> prefix(size_t(icap) + REPAIR_ROWS);
      std::vector<gfrs_rbucket> buckets(REPAIR_ROWS);
      std::vector<gfrs_rimage> images(mcap);
      std::vector<int32_t> cls(cs.pats.size()), gm(cs.pats.size()),
          nw(cs.pats.size()), inplace(cs.jobs.size());
      std::vector<uint32_t> colpack(cs.pats.size());
      int gi = -1, gb = -1, gim = -1, gin = -1;
      rc = gfrs_compute_repair_queue_schedule(
          &cs.t, cs.jobs.data(), int(cs.jobs.size()), bad.data(), boff.data(),
          int(cs.pats.size()), REPAIR_BLOCK, bids.data(), vuids.data(), icap,
          mcap, items.data(), prefix.data(), &gi, buckets.data(), &gb,
          images.data(), &gim, cls.data(), gm.data(), nw.data(),
          colpack.data(), inplace.data(), &gin);
      if (short_items || short_images) {
        CHECK(rc == GFRS_ERR_NOMEM, "%s: cap %d/%d rc %d", cs.name, icap, mcap,
              rc);
        continue;
      }
      CHECK(rc == GFRS_OK && gi == ni && gim == nim &&
                gb == int(s.buckets.size()) &&
                gin == int(s.inplace_jobs.size()),
            "%s: export rc %d", cs.name, rc);
      for (int i = 0; i < ni; i++)
        CHECK(items[i].job == s.items[i].job &&
                  items[i].desc == s.items[i].desc &&
                  items[i].img == s.items[i].img,
              "%s: export item %d", cs.name, i);
      for (size_t p = 0; p < cs.pats.size(); p++)
        CHECK(cls[p] == rp[p].cls && gm[p] == rp[p].gm && nw[p] == rp[p].nw &&
                  colpack[p] == rp[p].colpack,
              "%s: export pattern %zu", cs.name, p);
      prefix.resize(s.frame_prefix.size());
      CHECK(prefix == s.frame_prefix, "%s: export prefix", cs.name);
    }
}

static void expect_rc(const gfrs_tactic &t, const Patterns &pats,
                      std::vector<gfrs_rjob> jobs, int64_t block_len, int want,
                      const char *what) {
  std::vector<int32_t> bad, boff;
  flatten(pats, &bad, &boff);
  bad.push_back(0);
  std::vector<gfrs_ritem> items(64);
  std::vector<uint64_t> prefix(64 + REPAIR_ROWS);
  std::vector<gfrs_rbucket> buckets(REPAIR_ROWS);
  std::vector<gfrs_rimage> images(64);
  std::vector<int32_t> cls(pats.size() + 1), gm(pats.size() + 1),
      nw(pats.size() + 1), inplace(jobs.size() + 1);
  std::vector<uint32_t> colpack(pats.size() + 1);
  int gi, gb, gim, gin;
  int rc = gfrs_compute_repair_queue_schedule(
      &t, jobs.data(), int(jobs.size()), bad.data(), boff.data(),
      int(pats.size()), block_len, nullptr, nullptr, 64, 64, items.data(),
      prefix.data(), &gi, buckets.data(), &gb, images.data(), &gim,
      cls.data(), gm.data(), nw.data(), colpack.data(), inplace.data(), &gin);
  CHECK(rc == want, "%s: rc %d, want %d", what, rc, want);
}

int main() {
  const gfrs_tactic ec41{4, 1, 0, 1, 4, 0, 2048};
  const gfrs_tactic ec63{6, 3, 0, 1, 8, 0, 2048};
  const gfrs_tactic ec66{6, 6, 0, 3, 11, 0, 2048};
  const gfrs_tactic ec124{12, 4, 0, 1, 15, 0, 2048};
  const gfrs_tactic ec134{13, 4, 0, 1, 16, 0, 2048};
  const gfrs_tactic lrc{12, 2, 2, 2, 14, 0, 2048};
  const gfrs_tactic ec633{6, 3, 3, 3, 9, 0, 2048};
  const std::vector<uint64_t> lens{1,     15,    16,    17,    33,     4095,
                                   4096,  4097,  8209,  16383, 16385,  49153,
                                   65531, 65532, 65533, 70005, 131064, 131065};

  std::vector<Case> cases;
  auto add = [&](const char *name, const gfrs_tactic &t, const Patterns &pats,
                 const std::vector<uint64_t> &ls, int njobs) {
    cases.push_back(
        {name, t, pats, interleaved(t.n + t.m + t.l, pats, ls, njobs)});
  };
  add("rs63_mixed", ec63, {{1}, {0, 5}, {0, 2, 4}, {7}, {1, 8}, {8, 1}}, lens,
      36);
  add("rs63_uniform", ec63, {{1, 7}}, {65533}, 7);
  add("rs124_k12", ec124, {{1}, {0, 13}, {2, 5, 11, 15}, {14, 3}},
      {70005, 33, 4097, 65533, 16385, 1, 131065, 4096, 49153, 15}, 12);
  add("lrc_single", lrc, {{0}, {12}, {14}, {3, 15}, {0, 13}},
      {33, 65533, 4097, 17, 70005, 8209, 16383}, 15);
  add("rs66_inplace", ec66,
      {{0, 1, 2}, {8, 1, 5, 3}, {0, 1, 2, 3, 4}, {5, 4, 3, 2, 1, 0},
       {4, 9, 10, 11}},
      {17, 4097, 65533, 8209, 16, 70005, 1, 131064, 16383, 33}, 20);
  add("rs134_w17", ec134, {{16}, {0, 12}, {3}, {14, 1, 2}},
      {4097, 15, 65533, 16, 33, 8209, 131065}, 14);
  add("lrc_slow", ec633, {{9}, {11, 0}, {6, 9}, {0, 9, 6}},
      {33, 4097, 17, 65533, 16}, 14);
  /* degenerate */
  add("one job", ec63, {{5, 0}}, {70005}, 1);
  add("one row", ec41, {{0}, {4}, {3}}, lens, 20);
  add("one pattern of two", ec63, {{8}, {2}}, lens, 40);
  {
    Patterns own;
    for (int i = 0; i < 9; i++) own.push_back({i});
    cases.push_back({"own patterns", ec63, own,
                     interleaved(9, own, {4096, 100}, 9)});
    for (int j = 0; j < 9; j++) cases.back().jobs[j].pattern = 8 - j;
  }
  add("large", ec66, {{0}, {0, 1, 2, 3, 4, 5}, {7}, {11, 10}},
      {1, 1u << 20, 4097, 65536}, 5000);
  add("large fused", ec124, {{0}, {15, 0, 7, 3}, {7}},
      {1, 1u << 20, 4097, 65536}, 5000);
  add("huge shards", ec63, {{0}}, {uint64_t(1) << 40, 1}, 4);
  for (const Case &cs : cases) run_case(cs);

  /* validation codes */
  const uint64_t sz = repair_image_size(100);
  CHECK(sz == 144 && repair_image_size(65532) == 65532 + 44 &&
            repair_image_size(65533) == 65533 + 48,
        "image size");
  const std::vector<gfrs_rjob> ok{{0, 100, 0, sz, 0, 0}};
  const int64_t B = REPAIR_BLOCK;
  expect_rc(ec63, {{1}}, ok, B, GFRS_OK, "ok");
  expect_rc(ec63, {{1}}, {}, B, GFRS_ERR_INVALID_SHARDS, "no jobs");
  expect_rc(ec63, {}, ok, B, GFRS_ERR_INVALID_SHARDS, "no patterns");
  expect_rc(ec63, {{1}}, {{0, 100, 0, sz, 1, 0}}, B, GFRS_ERR_INVALID_SHARDS,
            "pattern");
  expect_rc(ec63, {{1}}, {{0, 100, 0, sz, -1, 0}}, B, GFRS_ERR_INVALID_SHARDS,
            "negative pattern");
  expect_rc(ec63, {{1}}, {{0, 0, 0, sz, 0, 0}}, B, GFRS_ERR_SHARD_NO_DATA,
            "length 0");
  expect_rc(ec63, {{1}}, {{0, 100, 0, sz, 0, 1}}, B, GFRS_ERR_INVALID_SHARDS,
            "reserved");
  expect_rc(ec63, {{1}}, {{0, 100, 2, sz, 0, 0}}, B, GFRS_ERR_INVALID_SHARDS,
            "img_off alignment");
  expect_rc(ec63, {{1}}, {{0, 100, 0, sz + 2, 0, 0}}, B,
            GFRS_ERR_INVALID_SHARDS, "img_stride alignment");
  expect_rc(ec63, {{1}}, {{0, 100, 0, sz - 4, 0, 0}}, B,
            GFRS_ERR_INVALID_SHARDS, "img_stride below the image size");
  expect_rc(ec63, {{1}}, ok, 4096, GFRS_ERR_UNSUPPORTED, "block_len 4096");
  expect_rc(ec63, {{1}}, ok, 131072, GFRS_ERR_UNSUPPORTED, "block_len 128K");
  expect_rc(ec63, {{1}, {9}}, ok, B, GFRS_ERR_INVALID_SHARDS,
            "unused pattern");
  expect_rc(ec63, {{1}, {0, 1, 2, 3}}, ok, B, GFRS_ERR_TOO_FEW_SHARDS,
            "m+1 bad");
  expect_rc(ec63, {{1}, {}}, ok, B, GFRS_ERR_INVALID_SHARDS, "empty pattern");
  expect_rc(ec63, {{1, 1}}, ok, B, GFRS_ERR_INVALID_SHARDS, "RS repeat");
  expect_rc(ec66, {{2, 3, 2}}, ok, B, GFRS_ERR_INVALID_SHARDS,
            "RS(6+6) repeat");
  expect_rc(ec66, {{1}, {}}, ok, B, GFRS_ERR_INVALID_SHARDS,
            "RS(6+6) empty pattern");
  expect_rc(lrc, {{0, 0}}, ok, B, GFRS_ERR_INVALID_SHARDS, "LRC repeat");
  expect_rc(lrc, {{0, 1, 2}}, ok, B, GFRS_ERR_TOO_FEW_SHARDS, "LRC 3 global");
  expect_rc(lrc, {{0, 14, 15}}, ok, B, GFRS_OK, "LRC locals");
  printf("repair queue selftest OK: %zu queues, %ld work items, %ld images\n",
         cases.size(), g_items, g_images);
  return 0;
}
