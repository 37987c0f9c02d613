/* tests/plan_selftest.cpp — stand-alone host check of the plan builders
 * (cubefs_amd/csrc/gfrs_plan.cpp), meant to be built with
 * -fsanitize=address,undefined by a plain host compiler together with
 * gfrs_plan.cpp and gfrs_gf.cpp (tests/test_plan_cpu.py does that).
 *
 * For each tactic of the verdict sweeps: every bad multiset of size 1..4
 * over the indices -1..total (so out-of-range, duplicate and undecodable
 * lists are met), ascending and descending, through every builder.  The
 * return code must be the documented one, and every returned plan must
 * satisfy   rows x dspace(in) == dspace(out)   where dspace(s) is the row
 * of shard s over the n data shards, computed here independently.
 * Exit status 0 and "plan selftest OK" on success.
 */
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../cubefs_amd/csrc/gfrs_plan.h"

using namespace gfrs;

static long g_plans = 0, g_refused = 0;

#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      fprintf(stderr, "FAIL %s:%d: %s\n  ", __FILE__, __LINE__, #cond); \
      fprintf(stderr, __VA_ARGS__);               \
      fprintf(stderr, "\n");                      \
      exit(1);                                    \
    }                                             \
  } while (0)

typedef std::vector<uint8_t> Row;

/* row of every shard over the n data shards, from the two matrices */
static std::vector<Row> dspace(const Code &c) {
  const GfTables &gt = gft();
  const int k = c.t.n, m = c.t.m;
  std::vector<Row> d(c.total, Row(k, 0));
  for (int s = 0; s < k + m; s++)
    d[s].assign(&c.enc_matrix[size_t(s) * k], &c.enc_matrix[size_t(s) * k] + k);
  for (int s = k + m; s < c.total; s++) {
    const int az = (s - k - m) / c.local_m, lp = (s - k - m) % c.local_m;
    const std::vector<int32_t> idx = local_stripe(c.t, az);
    for (int j = 0; j < c.local_n; j++) {
      const uint8_t coef =
          c.local_matrix[size_t(c.local_n + lp) * c.local_n + j];
      for (int col = 0; col < k; col++)
        d[s][col] ^= gt.mul[coef][d[idx[j]][col]];
    }
  }
  return d;
}

/* rows x space(in) == space(out), space[] given per plan index */
static void check_identity(const Plan &p, const std::vector<Row> &space,
                           const char *what) {
  const GfTables &gt = gft();
  CHECK(p.rows.size() == p.out.size() * size_t(p.rowk), "%s: rows size", what);
  CHECK(int(p.in.size()) >= p.rowk, "%s: in shorter than rowk", what);
  const size_t w = space[0].size();
  for (size_t r = 0; r < p.out.size(); r++) {
    Row acc(w, 0);
    for (int c = 0; c < p.rowk; c++)
      for (size_t col = 0; col < w; col++)
        acc[col] ^= gt.mul[p.rows[r * p.rowk + c]][space[p.in[c]][col]];
    CHECK(acc == space[p.out[r]], "%s: row %zu (shard %d)", what, r, p.out[r]);
  }
  g_plans++;
}

static std::vector<int> first_k_present(const Code &c,
                                        const std::vector<uint8_t> &missing) {
  std::vector<int> v;
  for (int i = 0; i < c.t.n + c.t.m && int(v.size()) < c.t.n; i++)
    if (!missing[i]) v.push_back(i);
  return v;
}

static void walk_bad(const Code &c, const std::vector<Row> &ds,
                     const std::vector<int32_t> &bad) {
  const int k = c.t.n, m = c.t.m, nbad = int(bad.size());
  bool range_ok = true, dup = false;
  std::vector<uint8_t> missing(c.total, 0);
  for (int b : bad) {
    if (b < 0 || b >= c.total) {
      range_ok = false;
      continue;
    }
    dup |= missing[b] != 0;
    missing[b] = 1;
  }
  const bool enough = int(first_k_present(c, missing).size()) == k;
  char what[96];
  snprintf(what, sizeof(what), "n=%d m=%d l=%d bad=[%d %d %d %d]/%d", k, m,
           c.t.l, bad[0], nbad > 1 ? bad[1] : -9, nbad > 2 ? bad[2] : -9,
           nbad > 3 ? bad[3] : -9, nbad);

  Plan rs, lrc, rep;
  int rc = plan_rs_reconstruct_verify(c, bad.data(), nbad, &rs);
  int want = !range_ok ? GFRS_ERR_INVALID_SHARDS
             : !enough ? GFRS_ERR_TOO_FEW_SHARDS : GFRS_OK;
  CHECK(rc == want, "%s rs rc=%d want=%d", what, rc, want);
  if (rc == GFRS_OK) {
    check_identity(rs, ds, what);
    int nparity = 0;
    for (size_t r = 0; r < rs.out.size(); r++) {
      const bool cmp = rs.cmp_mask >> r & 1;
      CHECK(cmp == !missing[rs.out[r]], "%s rs cmp bit %zu", what, r);
      nparity += rs.out[r] >= k;
    }
    CHECK(nparity == m, "%s rs carries %d parity rows", what, nparity);
  } else {
    g_refused++;
  }

  rc = plan_lrc_reconstruct_verify(c, bad.data(), nbad, &lrc);
  want = !range_ok || dup ? GFRS_ERR_INVALID_SHARDS
         : !enough        ? GFRS_ERR_UNSUPPORTED : GFRS_OK;
  CHECK(rc == want, "%s lrc rc=%d want=%d", what, rc, want);
  if (rc == GFRS_OK) {
    check_identity(lrc, ds, what);
    CHECK(std::equal(bad.begin(), bad.end(), lrc.out.begin()),
          "%s lrc write rows follow the caller", what);
    for (size_t r = 0; r < lrc.out.size(); r++)
      CHECK((lrc.cmp_mask >> r & 1) == (r >= size_t(nbad)) &&
                missing[lrc.out[r]] == (r < size_t(nbad)),
            "%s lrc row %zu", what, r);
  } else {
    g_refused++;
  }

  rc = plan_fused_repair(c, bad.data(), nbad, &rep);
  want = !range_ok || dup ? GFRS_ERR_INVALID_SHARDS
         : !enough        ? GFRS_ERR_TOO_FEW_SHARDS : GFRS_OK;
  CHECK(rc == want, "%s repair rc=%d want=%d", what, rc, want);
  uint32_t colpack = 0;
  CHECK(repair_colpack(c.total, bad.data(), nbad, &colpack) ==
            (!range_ok || dup ? GFRS_ERR_INVALID_SHARDS : GFRS_OK),
        "%s colpack rc", what);
  if (rc == GFRS_OK) {
    check_identity(rep, ds, what);
    CHECK(rep.out.size() <= 4 && rep.colpack == colpack, "%s budget", what);
    CHECK(rep.in.size() == size_t(k) + rep.out.size() - nbad, "%s in", what);
    for (int r = 0; r < nbad; r++) {
      CHECK(r == 0 || rep.out[r - 1] < rep.out[r], "%s repair order", what);
      CHECK(bad[(rep.colpack >> (4 * r)) & 15] == rep.out[r], "%s col", what);
    }
    for (size_t r = nbad; r < rep.out.size(); r++)
      CHECK(rep.in[k + r - nbad] == rep.out[r] && !missing[rep.out[r]],
            "%s check row %zu", what, r);
  } else {
    g_refused++;
  }
  if (!range_ok) return;

  /* the per-engine builders: global engine, then each AZ's local engine */
  std::vector<int32_t> gidx(k + m);
  for (int i = 0; i < k + m; i++) gidx[i] = i;
  std::vector<uint8_t> present(k + m);
  for (int i = 0; i < k + m; i++) present[i] = !missing[i];
  const Engine g{k, m, c.enc_matrix.data(), gidx.data()};
  Plan dec, par;
  rc = plan_decode(g, present.data(), &dec);
  CHECK(rc == (enough ? GFRS_OK : GFRS_ERR_TOO_FEW_SHARDS), "%s decode", what);
  if (rc == GFRS_OK && !dec.out.empty()) check_identity(dec, ds, what);
  CHECK(plan_parity(g, present.data(), &par) == GFRS_OK, "%s parity", what);
  if (!par.out.empty()) check_identity(par, ds, what);
  for (int az = 0; c.t.l > 0 && az < c.t.az_count; az++) {
    const std::vector<int32_t> idx = local_stripe(c.t, az);
    const int lk = c.local_n, lm = c.local_m;
    std::vector<uint8_t> lp(lk + lm);
    int np = 0;
    for (int i = 0; i < lk + lm; i++) np += lp[i] = !missing[idx[i]];
    /* engine-space identity: shard idx[i] is row i of the local matrix */
    std::vector<Row> space(c.total, Row(lk, 0));
    for (int i = 0; i < lk + lm; i++)
      space[idx[i]].assign(&c.local_matrix[size_t(i) * lk],
                           &c.local_matrix[size_t(i) * lk] + lk);
    const Engine e{lk, lm, c.local_matrix.data(), idx.data()};
    Plan ld, lpar;
    rc = plan_decode(e, lp.data(), &ld);
    CHECK(rc == (np >= lk ? GFRS_OK : GFRS_ERR_TOO_FEW_SHARDS), "%s local",
          what);
    if (rc == GFRS_OK && !ld.out.empty()) check_identity(ld, space, what);
    CHECK(plan_parity(e, lp.data(), &lpar) == GFRS_OK, "%s lparity", what);
    if (!lpar.out.empty()) check_identity(lpar, space, what);
  }
}

static void walk_tactic(int n, int m, int l, int az) {
  gfrs_tactic t{};
  t.n = n, t.m = m, t.l = l, t.az_count = az;
  CHECK(tactic_valid(&t), "tactic %d+%d+%d", n, m, l);
  Code c;
  CHECK(code_build(t, &c), "code %d+%d+%d", n, m, l);
  const std::vector<Row> ds = dspace(c);

  Plan enc;
  CHECK(plan_fused_lrc(c, &enc) == GFRS_OK, "fused encode");
  CHECK(int(enc.out.size()) == m + l && int(enc.in.size()) == n, "encode");
  check_identity(enc, ds, "fused encode");
  for (int idx = -1; idx <= n; idx++) {
    Plan p;
    int rc = plan_encode_idx(c, idx, &p);
    CHECK(rc == (idx < 0 || idx >= n ? GFRS_ERR_INVALID_SHARDS : GFRS_OK),
          "encode_idx %d", idx);
    for (int r = 0; rc == GFRS_OK && r < m; r++)
      CHECK(p.rows[r] == ds[n + r][idx] && p.out[r] == 1 + r, "encode_idx");
  }

  /* multisets of size 1..4 over -1..total, ascending then descending */
  const int lo = -1, hi = c.total;
  for (int nb = 1; nb <= 4; nb++) {
    std::vector<int32_t> bad(nb, lo);
    for (;;) {
      walk_bad(c, ds, bad);
      std::vector<int32_t> rev(bad.rbegin(), bad.rend());
      if (rev != bad) walk_bad(c, ds, rev);
      int i = nb - 1;
      while (i >= 0 && bad[i] == hi) i--;
      if (i < 0) break;
      const int v = bad[i] + 1;
      for (int j = i; j < nb; j++) bad[j] = v;
    }
  }
}

int main() {
  walk_tactic(6, 3, 0, 1);   /* EC6P3 */
  walk_tactic(4, 2, 0, 1);   /* EC4P2 */
  walk_tactic(3, 3, 0, 1);   /* EC3P3 */
  walk_tactic(12, 4, 0, 1);  /* EC12P4 */
  walk_tactic(13, 4, 0, 1);  /* EC13P4 */
  walk_tactic(6, 6, 0, 3);   /* EC6P6 */
  walk_tactic(12, 2, 2, 2);  /* LRC12P2L2 */
  walk_tactic(6, 3, 3, 3);   /* EC6P3L3 */
  walk_tactic(4, 4, 2, 2);   /* EC4P4L2 */
  printf("plan selftest OK: %ld plans checked, %ld lists refused\n", g_plans,
         g_refused);
  return 0;
}
