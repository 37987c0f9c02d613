/* tests/read_queue_selftest.cpp — stand-alone host check of the read plan,
 * the pattern classes and the read schedule builder
 * (cubefs_amd/csrc/gfrs_plan.cpp), meant to be built with
 * -fsanitize=address,undefined by a plain host compiler together with
 * gfrs_plan.cpp and gfrs_gf.cpp (tests/test_read_queue_cpu.py does that).
 *
 * For RS(6+3), RS(6+6), RS(13+4) and LRC(12+2+2): every bad set of size <= 3
 * (out-of-range, repeated and undecodable ones included) goes through
 * read_pattern; every plan is checked by matrix identity (each row, applied
 * to the encode-matrix rows of its inputs, must give the unit row of the
 * missing data shard).  Pseudo-random queues go through read_schedule and the
 * C export: every fused job must sit once in the bucket of its R, every
 * identity job n times in the R = 0 bucket, items ordered by descriptor then
 * caller index, prefix sums counting touched frames, slow jobs in caller
 * order.  Bad arguments must return their codes.  Exit status 0 and
 * "read queue selftest OK" on success.
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

static long g_plans = 0, g_refused = 0, g_items = 0;

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd(uint64_t n) {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return g_rng % n;
}

static uint64_t round4(uint64_t n) { return (n + 3) / 4 * 4; }

/* one pattern: codes, class, plan */
static void check_pattern(const Code &c, const std::vector<int32_t> &bad) {
  const int n = c.t.n, nm = c.t.n + c.t.m;
  int want = GFRS_OK, nglobal = 0, ndata = 0;
  std::vector<int> seen(c.total, 0);
  for (int32_t b : bad) {
    if (b < 0 || b >= c.total || seen[b]) {
      want = GFRS_ERR_INVALID_SHARDS;
      break;
    }
    seen[b] = 1;
    nglobal += b < nm;
    ndata += b < n;
  }
  if (want == GFRS_OK && nglobal > c.t.m) want = GFRS_ERR_TOO_FEW_SHARDS;
  Plan p;
  ReadPattern rp;
  const int rc = read_pattern(c, bad.data(), int(bad.size()), &p, &rp);
  CHECK(rc == want, "rc %d want %d (nbad %zu)", rc, want, bad.size());
  ReadPattern rp2;
  CHECK(read_pattern_check(c, bad.data(), int(bad.size()), &rp2) == want,
        "check disagrees");
  if (rc != GFRS_OK) {
    g_refused++;
    return;
  }
  g_plans++;
  CHECK(rp.r == ndata && rp2.r == ndata && rp.cls == rp2.cls, "class");
  const int cls = c.total <= 16
                      ? (ndata <= READ_ROWS ? GFRS_GPAT_FUSED : GFRS_GPAT_SLOW)
                      : (ndata == 0 ? GFRS_GPAT_IDENTITY : GFRS_GPAT_SLOW);
  CHECK(rp.cls == cls, "class %d want %d", rp.cls, cls);
  /* inputs: first n present of the n+m, ascending */
  CHECK(int(p.in.size()) == n && p.rowk == n, "inputs");
  int at = 0;
  uint32_t pass = 0;
  for (int i = 0; i < nm && at < n; i++)
    if (!seen[i]) {
      CHECK(p.in[at] == i, "input %d is %d want %d", at, p.in[at], i);
      if (i < n) pass |= 1u << at;
      at++;
    }
  CHECK(at == n && p.pass_mask == pass, "pass mask %x want %x", p.pass_mask,
        pass);
  /* rows: the missing data shards ascending, write rows only */
  CHECK(int(p.out.size()) == ndata && p.cmp_mask == 0, "rows");
  CHECK(p.rows.size() == size_t(ndata) * n, "row bytes");
  const GfTables &gt = gft();
  int r = 0;
  for (int d = 0; d < n; d++) {
    if (!seen[d]) continue;
    CHECK(p.out[r] == d, "row %d is %d want %d", r, p.out[r], d);
    /* sum_c rows[r][c] * enc_matrix[in[c]] == unit row d */
    for (int col = 0; col < n; col++) {
      uint8_t v = 0;
      for (int ci = 0; ci < n; ci++)
        v ^= gt.mul[p.rows[size_t(r) * n + ci]]
                   [c.enc_matrix[size_t(p.in[ci]) * n + col]];
      CHECK(v == (col == d ? 1 : 0), "row %d column %d", r, col);
    }
    r++;
  }
}

static void all_patterns(const Code &c) {
  const int lo = -1, hi = c.total; /* one index out of range at each end */
  check_pattern(c, {});
  for (int a = lo; a <= hi; a++) {
    check_pattern(c, {a});
    for (int b = lo; b <= hi; b++) {
      check_pattern(c, {a, b});
      if ((a + b) % 3 == 0) /* a third of the triples is plenty */
        for (int d = 0; d < hi; d++) check_pattern(c, {a, b, d});
    }
  }
  /* larger sets: every data shard, and more than m */
  std::vector<int32_t> bad;
  for (int i = 0; i < c.t.m && i < c.t.n; i++) bad.push_back(i);
  check_pattern(c, bad);
  bad.push_back(c.t.n);
  check_pattern(c, bad);
}

static void check_schedule(const char *name, const Code &c,
                           const std::vector<gfrs_gjob> &jobs,
                           const std::vector<ReadPattern> &pats,
                           const ReadSchedule &s) {
  const int n = c.t.n, npat = int(pats.size());
  CHECK(s.buckets.size() <= size_t(READ_ROWS + 1), "%s: buckets", name);
  std::vector<int> hits(jobs.size(), 0);
  size_t at = 0;
  int last_r = -1;
  for (size_t b = 0; b < s.buckets.size(); b++) {
    const ReadBucket &bk = s.buckets[b];
    CHECK(bk.first == at && bk.count > 0 && bk.r > last_r &&
              bk.prefix == at + b,
          "%s: bucket %zu placement", name, b);
    last_r = bk.r;
    CHECK(bk.prefix + bk.count + 1 <= s.frame_prefix.size() &&
              s.frame_prefix[bk.prefix] == 0,
          "%s: prefix of bucket %zu", name, b);
    long last_key = -1;
    for (size_t i = 0; i < bk.count; i++) {
      const gfrs_gitem &it = s.items[bk.first + i];
      CHECK(it.job >= 0 && it.job < int(jobs.size()), "%s: job index", name);
      const gfrs_gjob &jb = jobs[it.job];
      const ReadPattern &rp = pats[jb.pattern];
      CHECK(it.img == jb.img_off && it.img_stride == jb.img_stride &&
                it.shard_len == jb.shard_len && it.seg_off == jb.seg_off &&
                it.seg_len == jb.seg_len && it.out == jb.out_off &&
                it.out_stride == jb.out_stride,
            "%s: item %zu does not carry its job", name, bk.first + i);
      if (rp.cls == GFRS_GPAT_FUSED)
        CHECK(it.desc == jb.pattern && bk.r == rp.r, "%s: fused item", name);
      else
        CHECK(rp.cls == GFRS_GPAT_IDENTITY && bk.r == 0 && it.desc >= npat &&
                  it.desc < npat + n,
              "%s: identity item", name);
      const long key = long(it.desc) * long(jobs.size()) + it.job;
      CHECK(key > last_key, "%s: item order in bucket %zu", name, b);
      last_key = key;
      const uint64_t nf = (jb.seg_off + jb.seg_len - 1) / 65532 -
                          jb.seg_off / 65532 + 1;
      CHECK(s.frame_prefix[bk.prefix + i + 1] -
                    s.frame_prefix[bk.prefix + i] == nf,
            "%s: touched frames of job %d", name, it.job);
      hits[it.job]++;
      g_items++;
    }
    at += bk.count;
  }
  CHECK(at == s.items.size() &&
            s.frame_prefix.size() == at + s.buckets.size(),
        "%s: totals", name);
  size_t ns = 0;
  for (size_t j = 0; j < jobs.size(); j++) {
    const int cls = pats[jobs[j].pattern].cls;
    const int want = cls == GFRS_GPAT_FUSED ? 1 : cls == GFRS_GPAT_IDENTITY
                                                      ? n : 0;
    CHECK(hits[j] == want, "%s: job %zu appears %d times", name, j, hits[j]);
    if (cls == GFRS_GPAT_SLOW) {
      CHECK(ns < s.slow_jobs.size() && s.slow_jobs[ns] == int(j),
            "%s: slow job %zu", name, j);
      ns++;
    }
  }
  CHECK(ns == s.slow_jobs.size(), "%s: slow jobs", name);
}

static void random_queues(const char *name, const Code &c, int rounds) {
  const int nm = c.t.n + c.t.m;
  static const uint64_t pick[] = {1, 3, 4, 17, 4096, 65531, 65532, 65533,
                                  65597, 131064, 131065, 1 << 20};
  for (int round = 0; round < rounds; round++) {
    const int npat = 1 + int(rnd(6));
    std::vector<int32_t> bad_idx, bad_off(1, 0);
    for (int p = 0; p < npat; p++) {
      const int nb = int(rnd(uint64_t(c.t.m) + 1));
      std::vector<int> used(c.total, 0);
      for (int i = 0; i < nb; i++) {
        int b = int(rnd(uint64_t(nm)));
        while (used[b]) b = (b + 1) % nm;
        used[b] = 1;
        bad_idx.push_back(b);
      }
      if (c.t.l > 0 && rnd(2)) bad_idx.push_back(nm + int(rnd(c.t.l)));
      bad_off.push_back(int32_t(bad_idx.size()));
    }
    std::vector<ReadPattern> pats(npat);
    for (int p = 0; p < npat; p++)
      CHECK(read_pattern_check(c, bad_idx.data() + bad_off[p],
                               bad_off[p + 1] - bad_off[p],
                               &pats[p]) == GFRS_OK,
            "%s: pattern %d", name, p);
    const int njobs = 1 + int(rnd(40));
    std::vector<gfrs_gjob> jobs;
    uint64_t img = rnd(64), out = 4 * rnd(9);
    for (int j = 0; j < njobs; j++) {
      const uint64_t len = rnd(3) ? pick[rnd(12)] : 1 + rnd(300000);
      const uint64_t so = 4 * rnd((len + 3) / 4);
      const uint64_t sl = 1 + rnd(len - so);
      const uint64_t stride = encode_image_size(len) + rnd(5);
      const uint64_t ostride = round4(sl) + 4 * rnd(3);
      jobs.push_back(gfrs_gjob{img, stride, len, so, sl, out, ostride,
                               int32_t(rnd(uint64_t(npat))), 0});
      img += stride * c.total + rnd(7);
      out += ostride * c.t.n + 4 * rnd(5);
    }
    ReadSchedule s;
    CHECK(read_schedule(c, jobs.data(), njobs, pats.data(), npat, 0, &s) ==
              GFRS_OK,
          "%s: schedule", name);
    check_schedule(name, c, jobs, pats, s);

    /* the C export agrees */
    const int cap = njobs * c.t.n;
    std::vector<gfrs_gitem> items(cap);
    std::vector<uint64_t> prefix(cap + 5);
    gfrs_gbucket buckets[5];
    std::vector<int32_t> pcls(npat), pr(npat), slow(njobs);
    int ni = 0, nb = 0, ns = 0;
    CHECK(gfrs_compute_read_queue_schedule(
              &c.t, jobs.data(), njobs, bad_idx.data(), bad_off.data(), npat,
              65536, cap, items.data(), prefix.data(), &ni, buckets, &nb,
              pcls.data(), pr.data(), slow.data(), &ns) == GFRS_OK,
          "%s: export", name);
    CHECK(ni == int(s.items.size()) && nb == int(s.buckets.size()) &&
              ns == int(s.slow_jobs.size()),
          "%s: export counts", name);
    for (int i = 0; i < ni; i++)
      CHECK(items[i].job == s.items[i].job && items[i].desc == s.items[i].desc,
            "%s: export item %d", name, i);
    for (int i = 0; i < ni + nb; i++)
      CHECK(prefix[i] == s.frame_prefix[i], "%s: export prefix %d", name, i);
    for (int p = 0; p < npat; p++)
      CHECK(pcls[p] == pats[p].cls && pr[p] == pats[p].r,
            "%s: export pattern %d", name, p);
    if (ni > 0) {
      int ni2, nb2, ns2;
      CHECK(gfrs_compute_read_queue_schedule(
                &c.t, jobs.data(), njobs, bad_idx.data(), bad_off.data(), npat,
                65536, ni - 1, items.data(), prefix.data(), &ni2, buckets,
                &nb2, pcls.data(), pr.data(), slow.data(), &ns2) ==
                GFRS_ERR_NOMEM,
            "%s: export capacity", name);
    }
  }
}

static void validation(const Code &c) {
  const ReadPattern pats[2] = {ReadPattern(), ReadPattern()};
  const uint64_t sz = encode_image_size(100);
  const gfrs_gjob ok{0, sz, 100, 0, 100, 0, 100, 0, 0};
  ReadSchedule s;
  auto rc = [&](gfrs_gjob j, uint64_t out_addr = 0) {
    return read_schedule(c, &j, 1, pats, 2, out_addr, &s);
  };
  CHECK(rc(ok) == GFRS_OK, "ok job");
  gfrs_gjob j = ok;
  j.pattern = 2;
  CHECK(rc(j) == GFRS_ERR_INVALID_SHARDS, "pattern range");
  j = ok; j.reserved = 1;
  CHECK(rc(j) == GFRS_ERR_INVALID_SHARDS, "reserved");
  j = ok; j.shard_len = 0;
  CHECK(rc(j) == GFRS_ERR_SHARD_NO_DATA, "shard_len 0");
  j = ok; j.seg_len = 0;
  CHECK(rc(j) == GFRS_ERR_SHARD_NO_DATA, "seg_len 0");
  j = ok; j.seg_off = 2; j.seg_len = 4;
  CHECK(rc(j) == GFRS_ERR_INVALID_SHARDS, "seg_off alignment");
  j = ok; j.out_off = 2;
  CHECK(rc(j) == GFRS_ERR_INVALID_SHARDS, "out_off alignment");
  CHECK(rc(ok, 2) == GFRS_ERR_INVALID_SHARDS, "out alignment");
  j = ok; j.out_stride = 102;
  CHECK(rc(j) == GFRS_ERR_INVALID_SHARDS, "out_stride alignment");
  j = ok; j.out_stride = 96;
  CHECK(rc(j) == GFRS_ERR_INVALID_SHARDS, "out_stride below seg_len");
  j = ok; j.img_stride = sz - 1;
  CHECK(rc(j) == GFRS_ERR_INVALID_SHARDS, "img_stride below the image");
  j = ok; j.seg_off = 4; j.seg_len = 97;
  CHECK(rc(j) == GFRS_ERR_INVALID_SHARDS, "segment past the shard");
  j = ok; j.seg_off = uint64_t(1) << 63; j.seg_len = uint64_t(1) << 63;
  CHECK(rc(j) == GFRS_ERR_INVALID_SHARDS, "segment overflow");
  CHECK(read_schedule(c, &ok, 0, pats, 2, 0, &s) == GFRS_ERR_INVALID_SHARDS,
        "njobs 0");
  CHECK(read_schedule(c, &ok, 1, pats, 0, 0, &s) == GFRS_ERR_INVALID_SHARDS,
        "npat 0");
  CHECK(read_queue_gate(c, 0) == GFRS_ERR_INVALID_BLOCK &&
            read_queue_gate(c, 65540) == GFRS_ERR_INVALID_BLOCK &&
            read_queue_gate(c, 4096) == GFRS_ERR_UNSUPPORTED &&
            read_queue_gate(c, 65536) == GFRS_OK,
        "block_len");
}

int main() {
  const gfrs_tactic tactics[] = {
      {6, 3, 0, 1, 0, 0, 2048},  {6, 6, 0, 1, 0, 0, 2048},
      {13, 4, 0, 1, 0, 0, 2048}, {12, 2, 2, 2, 0, 0, 2048}};
  const char *names[] = {"rs63", "rs66", "rs134", "lrc12p2l2"};
  for (int i = 0; i < 4; i++) {
    Code c;
    CHECK(tactic_valid(&tactics[i]) && code_build(tactics[i], &c), "%s",
          names[i]);
    all_patterns(c);
    random_queues(names[i], c, 60);
    validation(c);
  }
  /* a tactic wider than a verdict word */
  const gfrs_tactic wide{30, 3, 0, 1, 0, 0, 2048};
  Code cw;
  CHECK(code_build(wide, &cw), "wide");
  CHECK(read_queue_gate(cw, 65536) == GFRS_ERR_UNSUPPORTED, "33 shards");
  printf("read queue selftest OK: %ld plans, %ld refused, %ld items\n",
         g_plans, g_refused, g_items);
  return 0;
}
