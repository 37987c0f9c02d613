/* cubefs_amd/csrc/gfrs_plan.cpp — coding-plan construction (see
 * gfrs_plan.h).  One copy of each piece of algebra:
 *   dspace_row   shard index -> its row over the n data shards
 *   Basis        the first k present shards, inverted
 *   over_inputs  data-space row -> row over the k chosen inputs
 * Every builder is a few lines on top of them.  A row that expresses
 * out[r] over k independent inputs is unique, so the builders only have to
 * agree on `in` and `out`.
 */
#include "gfrs_plan.h"

#include <algorithm>
#include <cstring>

namespace gfrs {

bool tactic_valid(const gfrs_tactic *t) {
  /* codemode.go:291-299 IsValid; replicate modes (m==0, l==0) are legal —
   * ec.NewEncoder accepts them and Encode is a no-op (reedsolomon.go:442) */
  if (!t) return false;
  if (t->m == 0 && t->l == 0)
    return t->n > 0 && t->az_count > 0 && t->n % t->az_count == 0;
  if (t->n <= 0 || t->m <= 0 || t->l < 0 || t->az_count <= 0) return false;
  if (t->n % t->az_count || t->m % t->az_count || t->l % t->az_count)
    return false;
  if (t->n + t->m > 256) return false;
  if (t->l > 0 && (t->n + t->m) / t->az_count + t->l / t->az_count > 256)
    return false;
  return true;
}

bool code_build(const gfrs_tactic &t, Code *c) {
  c->t = t;
  c->total = t.n + t.m + t.l;
  /* global encode matrix (reedsolomon.go:220-244); replicate modes have
   * no parity engine (reedsolomon.go:442 parityShards==0 early return) */
  if (t.m > 0) {
    c->enc_matrix.resize(size_t(t.n + t.m) * t.n);
    if (!gf_build_matrix(t.n, t.n + t.m, c->enc_matrix.data())) return false;
  }
  /* local engines (encoder.go:92-104) */
  if (t.l > 0) {
    c->local_n = (t.n + t.m) / t.az_count;
    c->local_m = t.l / t.az_count;
    c->local_matrix.resize(size_t(c->local_n + c->local_m) * c->local_n);
    if (!gf_build_matrix(c->local_n, c->local_n + c->local_m,
                         c->local_matrix.data()))
      return false;
  }
  return true;
}

std::vector<int32_t> local_stripe(const gfrs_tactic &t, int az_idx) {
  int ln = t.n / t.az_count, lm = t.m / t.az_count, ll = t.l / t.az_count;
  std::vector<int32_t> idx;
  idx.reserve(ln + lm + ll);
  for (int i = 0; i < ln; i++) idx.push_back(az_idx * ln + i);
  for (int i = 0; i < lm; i++) idx.push_back(t.n + az_idx * lm + i);
  for (int i = 0; i < ll; i++) idx.push_back(t.n + t.m + az_idx * ll + i);
  return idx;
}

/* Shard index -> its row over the n data shards.  Data and global parity
 * shards are rows of the encode matrix (whose top is the identity).  A
 * local parity is linear in its local stripe: an input that is a data
 * shard contributes its coefficient directly; one that is a global parity
 * contributes localcoef x its parity row (GF linearity). */
static void dspace_row(const Code &c, int sh, uint8_t *drow) {
  const int k = c.t.n, m = c.t.m;
  if (sh < k + m) {
    memcpy(drow, &c.enc_matrix[size_t(sh) * k], k);
    return;
  }
  const GfTables &gt = gft();
  const int az = (sh - k - m) / c.local_m, lp = (sh - k - m) % c.local_m;
  const std::vector<int32_t> idx = local_stripe(c.t, az);
  const uint8_t *lr = &c.local_matrix[size_t(c.local_n + lp) * c.local_n];
  memset(drow, 0, k);
  for (int j = 0; j < c.local_n; j++) {
    const uint8_t *er = &c.enc_matrix[size_t(idx[j]) * k];
    for (int d = 0; d < k; d++) drow[d] ^= gt.mul[lr[j]][er[d]];
  }
}

/* The decoding basis of one engine for one erasure set. */
struct Basis {
  int k = 0;
  std::vector<int> valid;        /* the k inputs, engine indices */
  std::vector<int> slot;         /* data column -> input slot, -1 = missing */
  std::vector<uint8_t> is_input; /* per engine shard */
  std::vector<uint8_t> dec;      /* k×k: data column d over the inputs */
};

/* first k present rows in index order (reedsolomon.go:1453-1466), inverted */
static int basis_build(int k, int m, const uint8_t *matrix,
                       const uint8_t *present, Basis *b) {
  b->k = k;
  b->slot.assign(k, -1);
  b->is_input.assign(k + m, 0);
  for (int i = 0; i < k + m && int(b->valid.size()) < k; i++)
    if (present[i]) {
      if (i < k) b->slot[i] = int(b->valid.size());
      b->is_input[i] = 1;
      b->valid.push_back(i);
    }
  if (int(b->valid.size()) < k) return GFRS_ERR_TOO_FEW_SHARDS;
  std::vector<uint8_t> sub(size_t(k) * k);
  b->dec.resize(size_t(k) * k);
  for (int r = 0; r < k; r++)
    memcpy(&sub[size_t(r) * k], &matrix[size_t(b->valid[r]) * k], k);
  return gf_invert(sub.data(), k, b->dec.data()) ? GFRS_OK
                                                  : GFRS_ERR_SINGULAR;
}

/* data-space row -> row over the k chosen inputs: a present data column is
 * its own input slot, a missing one is substituted through dec
 *   row[j] = drow[d]·1[slot(d)==j] (+) Σ_missing drow[d]·dec[d][j] */
static void over_inputs(const Basis &b, const uint8_t *drow, uint8_t *row) {
  const GfTables &gt = gft();
  const int k = b.k;
  memset(row, 0, k);
  for (int d = 0; d < k; d++) {
    const uint8_t coef = drow[d];
    if (!coef) continue;
    if (b.slot[d] >= 0)
      row[b.slot[d]] ^= coef;
    else
      for (int j = 0; j < k; j++)
        row[j] ^= gt.mul[coef][b.dec[size_t(d) * k + j]];
  }
}

/* append shard `sh` as an output row, given its data-space row */
static void add_row(Plan *p, const Basis &b, const uint8_t *drow, int sh) {
  p->out.push_back(sh);
  p->rows.resize(p->rows.size() + b.k);
  over_inputs(b, drow, &p->rows[p->rows.size() - b.k]);
}

int plan_decode(const Engine &e, const uint8_t *present, Plan *p) {
  Basis b;
  int rc = basis_build(e.k, e.m, e.matrix, present, &b);
  if (rc != GFRS_OK) return rc;
  p->rowk = e.k;
  for (int v : b.valid) p->in.push_back(e.idx[v]);
  for (int i = 0; i < e.k; i++)
    if (!present[i]) add_row(p, b, &e.matrix[size_t(i) * e.k], e.idx[i]);
  return GFRS_OK;
}

int plan_parity(const Engine &e, const uint8_t *present, Plan *p) {
  p->rowk = e.k;
  for (int i = 0; i < e.k; i++) p->in.push_back(e.idx[i]);
  for (int i = e.k; i < e.k + e.m; i++)
    if (!present[i]) {
      p->out.push_back(e.idx[i]);
      p->rows.insert(p->rows.end(), &e.matrix[size_t(i) * e.k],
                     &e.matrix[size_t(i) * e.k + e.k]);
    }
  return GFRS_OK;
}

int plan_encode_idx(const Code &c, int idx, Plan *p) {
  if (idx < 0 || idx >= c.t.n) return GFRS_ERR_INVALID_SHARDS;
  p->rowk = 1;
  p->in.push_back(0);
  for (int r = 0; r < c.t.m; r++) {
    p->out.push_back(1 + r);
    p->rows.push_back(c.enc_matrix[size_t(c.t.n + r) * c.t.n + idx]);
  }
  return GFRS_OK;
}

int plan_fused_lrc(const Code &c, Plan *p) {
  const int k = c.t.n;
  p->rowk = k;
  for (int i = 0; i < k; i++) p->in.push_back(i);
  for (int sh = k; sh < c.total; sh++) {
    p->out.push_back(sh);
    p->rows.resize(p->rows.size() + k);
    dspace_row(c, sh, &p->rows[p->rows.size() - k]);
  }
  return GFRS_OK;
}

/* ---- reconstruct + verify / repair over the global engine ---- */

/* bad list -> missing[] over all shards; the global basis for it */
struct Erasure {
  std::vector<uint8_t> missing; /* total */
  Basis b;
};

static int erasure_build(const Code &c, const int32_t *bad, int nbad,
                         bool dup_ok, Erasure *e) {
  if (c.t.m <= 0) return GFRS_ERR_TOO_FEW_SHARDS;
  e->missing.assign(c.total, 0);
  for (int i = 0; i < nbad; i++) {
    if (bad[i] < 0 || bad[i] >= c.total) return GFRS_ERR_INVALID_SHARDS;
    if (e->missing[bad[i]] && !dup_ok) return GFRS_ERR_INVALID_SHARDS;
    e->missing[bad[i]] = 1;
  }
  const int k = c.t.n, m = c.t.m;
  std::vector<uint8_t> present(k + m);
  for (int i = 0; i < k + m; i++) present[i] = !e->missing[i];
  return basis_build(k, m, c.enc_matrix.data(), present.data(), &e->b);
}

static void add_shard(Plan *p, const Code &c, const Erasure &e, int sh) {
  std::vector<uint8_t> drow(c.t.n);
  dspace_row(c, sh, drow.data());
  add_row(p, e.b, drow.data(), sh);
}

/* The check sequence of the single-pass paths: surviving global parities
 * that are not inputs (an input parity's check is the identity), then
 * surviving local parities (they restore detection when exactly k globals
 * survive).  Stops once `out` holds max_rows; a check shard is appended to
 * `in` when cmp_in is set. */
static void add_checks(Plan *p, const Code &c, const Erasure &e,
                       size_t max_rows, bool cmp_in) {
  for (int sh = c.t.n; sh < c.total && p->out.size() < max_rows; sh++) {
    if (e.missing[sh]) continue;
    if (sh < c.t.n + c.t.m && e.b.is_input[sh]) continue;
    add_shard(p, c, e, sh);
    if (cmp_in) p->in.push_back(sh);
  }
}

int plan_rs_reconstruct_verify(const Code &c, const int32_t *bad, int nbad,
                               Plan *p) {
  Erasure e;
  int rc = erasure_build(c, bad, nbad, /*dup_ok=*/true, &e);
  if (rc != GFRS_OK) return rc;
  const int k = c.t.n, m = c.t.m;
  p->rowk = k;
  p->in.assign(e.b.valid.begin(), e.b.valid.end());
  for (int i = 0; i < k; i++)
    if (e.missing[i]) add_shard(p, c, e, i);
  /* every parity row, inputs included: a missing one is written, a present
   * one compared */
  for (int sh = k; sh < k + m; sh++) {
    if (!e.missing[sh]) p->cmp_mask |= 1u << p->out.size();
    add_shard(p, c, e, sh);
  }
  return GFRS_OK;
}

int plan_lrc_reconstruct_verify(const Code &c, const int32_t *bad, int nbad,
                                Plan *p) {
  Erasure e;
  int rc = erasure_build(c, bad, nbad, /*dup_ok=*/false, &e);
  if (rc == GFRS_ERR_TOO_FEW_SHARDS) return GFRS_ERR_UNSUPPORTED;
  if (rc != GFRS_OK) return rc;
  p->rowk = c.t.n;
  p->in.assign(e.b.valid.begin(), e.b.valid.end());
  for (int i = 0; i < nbad; i++) add_shard(p, c, e, bad[i]);
  add_checks(p, c, e, size_t(-1), /*cmp_in=*/false);
  if (p->out.size() > 32) return GFRS_ERR_UNSUPPORTED; /* cmp_mask width */
  for (size_t r = size_t(nbad); r < p->out.size(); r++)
    p->cmp_mask |= 1u << r;
  return GFRS_OK;
}

int repair_colpack(int total, const int32_t *bad, int nbad,
                   uint32_t *colpack) {
  if (nbad <= 0 || nbad > 4) return GFRS_ERR_UNSUPPORTED; /* 4-row budget */
  *colpack = 0;
  for (int i = 0; i < nbad; i++) {
    if (bad[i] < 0 || bad[i] >= total) return GFRS_ERR_INVALID_SHARDS;
    int rank = 0; /* row of bad[i] = its rank in ascending order */
    for (int j = 0; j < nbad; j++) {
      if (j != i && bad[j] == bad[i]) return GFRS_ERR_INVALID_SHARDS;
      rank += bad[j] < bad[i];
    }
    *colpack |= uint32_t(i) << (4 * rank);
  }
  return GFRS_OK;
}

int plan_fused_repair(const Code &c, const int32_t *bad, int nbad, Plan *p) {
  int rc = repair_colpack(c.total, bad, nbad, &p->colpack);
  if (rc != GFRS_OK) return rc;
  Erasure e;
  if ((rc = erasure_build(c, bad, nbad, /*dup_ok=*/false, &e)) != GFRS_OK)
    return rc;
  p->rowk = c.t.n;
  p->in.assign(e.b.valid.begin(), e.b.valid.end());
  for (int sh = 0; sh < c.total; sh++) /* rebuild rows, ascending */
    if (e.missing[sh]) add_shard(p, c, e, sh);
  add_checks(p, c, e, 4, /*cmp_in=*/true);
  for (size_t r = size_t(nbad); r < p->out.size(); r++)
    p->cmp_mask |= 1u << r;
  return GFRS_OK;
}

bool lrc_single_pass(const Code &c) {
  return c.t.l > 0 && c.t.m + c.t.l <= 4 && c.total <= 16;
}

/* ---- the repair queue ---- */

int queue_offsets_check(const int32_t *bad_off, int npat) {
  if (npat <= 0 || !bad_off || bad_off[0] != 0) return GFRS_ERR_INVALID_SHARDS;
  for (int p = 0; p < npat; p++)
    if (bad_off[p + 1] < bad_off[p]) return GFRS_ERR_INVALID_SHARDS;
  return GFRS_OK;
}

int queue_pattern_check(const Code &c, const int32_t *bad, int nbad,
                        bool *slow) {
  *slow = false;
  if (nbad < 0) return GFRS_ERR_INVALID_SHARDS;
  const bool lrc = c.t.l > 0;
  std::vector<uint8_t> seen(c.total, 0);
  int nglobal = 0;
  for (int i = 0; i < nbad; i++) {
    if (bad[i] < 0 || bad[i] >= c.total) return GFRS_ERR_INVALID_SHARDS;
    if (seen[bad[i]]) {
      /* plain RS tolerates a repeated index, the LRC plans do not */
      if (lrc) return GFRS_ERR_INVALID_SHARDS;
      continue;
    }
    seen[bad[i]] = 1;
    nglobal += bad[i] < c.t.n + c.t.m;
  }
  /* the full-width Reconstruct decodes the global stripe first
   * (lrcencoder.go:155-186): more than m global losses fail whatever the
   * local parities could have restored */
  if (nglobal > c.t.m) return GFRS_ERR_TOO_FEW_SHARDS;
  if (lrc && !lrc_single_pass(c)) *slow = true;
  return GFRS_OK;
}

int queue_pattern(const Code &c, const int32_t *bad, int nbad, Plan *p,
                  QueuePattern *q) {
  *q = QueuePattern();
  int rc = queue_pattern_check(c, bad, nbad, &q->slow);
  if (rc != GFRS_OK || q->slow) return rc;
  if (c.t.l > 0) {
    rc = plan_lrc_reconstruct_verify(c, bad, nbad, p);
    if (rc == GFRS_ERR_UNSUPPORTED) { /* more rows than cmp_mask has bits */
      *p = Plan();
      q->slow = true;
      return GFRS_OK;
    }
  } else {
    rc = plan_rs_reconstruct_verify(c, bad, nbad, p);
  }
  if (rc == GFRS_OK) q->nout = int(p->out.size());
  return rc;
}

int queue_schedule(const gfrs_qjob *jobs, int njobs, const QueuePattern *pats,
                   int npat, QueueSchedule *out) {
  *out = QueueSchedule();
  if (njobs <= 0 || npat <= 0 || !jobs || !pats) return GFRS_ERR_INVALID_SHARDS;
  int max_steps = 0;
  for (int j = 0; j < njobs; j++) {
    const gfrs_qjob &jb = jobs[j];
    if (jb.pattern < 0 || jb.pattern >= npat || jb.reserved != 0)
      return GFRS_ERR_INVALID_SHARDS;
    if (jb.shard_len == 0) return GFRS_ERR_SHARD_NO_DATA;
    const int steps = (pats[jb.pattern].nout + QUEUE_ROWS - 1) / QUEUE_ROWS;
    max_steps = std::max(max_steps, steps);
  }
  /* jobs by pattern, caller order inside one pattern (counting sort) */
  std::vector<size_t> pstart(size_t(npat) + 1, 0);
  for (int j = 0; j < njobs; j++) pstart[size_t(jobs[j].pattern) + 1]++;
  for (int p = 0; p < npat; p++) pstart[p + 1] += pstart[p];
  std::vector<int32_t> order(njobs);
  for (int j = 0; j < njobs; j++) order[pstart[jobs[j].pattern]++] = j;

  /* bucket slot of step g with gm rows: ascending g, then gm */
  auto slot = [](int g, int gm) { return size_t(g) * QUEUE_ROWS + (gm - 1); };
  auto rows_of = [&](int nout, int g) {
    return std::min(QUEUE_ROWS, nout - QUEUE_ROWS * g);
  };
  std::vector<size_t> count(size_t(max_steps) * QUEUE_ROWS, 0);
  for (int j = 0; j < njobs; j++) {
    const QueuePattern &qp = pats[jobs[j].pattern];
    if (qp.slow) {
      out->slow_jobs.push_back(j);
      continue;
    }
    for (int g = 0; QUEUE_ROWS * g < qp.nout; g++)
      count[slot(g, rows_of(qp.nout, g))]++;
  }
  std::vector<size_t> bucket_of(count.size(), size_t(-1)), fill(count.size());
  size_t nitems = 0;
  for (size_t s = 0; s < count.size(); s++) {
    if (!count[s]) continue;
    QueueBucket b;
    b.g = int(s / QUEUE_ROWS);
    b.gm = int(s % QUEUE_ROWS) + 1;
    b.first = nitems;
    b.count = count[s];
    b.prefix = nitems + out->buckets.size();
    bucket_of[s] = out->buckets.size();
    fill[s] = nitems;
    nitems += count[s];
    out->buckets.push_back(b);
  }
  out->items.resize(nitems);
  out->tile_prefix.assign(nitems + out->buckets.size(), 0);
  for (int32_t j : order) {
    const gfrs_qjob &jb = jobs[j];
    const QueuePattern &qp = pats[jb.pattern];
    if (qp.slow) continue;
    for (int g = 0; QUEUE_ROWS * g < qp.nout; g++) {
      const size_t s = slot(g, rows_of(qp.nout, g));
      const QueueBucket &b = out->buckets[bucket_of[s]];
      const size_t at = fill[s]++;
      gfrs_qitem &it = out->items[at];
      it.off = jb.off;
      it.shard_len = jb.shard_len;
      it.job = j;
      it.pattern = jb.pattern;
      it.row_off = QUEUE_ROWS * g;
      it.reserved = 0;
      const size_t pi = b.prefix + (at - b.first);
      out->tile_prefix[pi + 1] =
          out->tile_prefix[pi] + (jb.shard_len - 1) / QUEUE_TILE + 1;
    }
  }
  return GFRS_OK;
}

/* ---- the repair-image queue ---- */

int repair_pattern_check(const Code &c, const int32_t *bad, int nbad,
                         RepairPattern *r) {
  *r = RepairPattern();
  if (nbad <= 0 || !bad) return GFRS_ERR_INVALID_SHARDS;
  std::vector<uint8_t> seen(c.total, 0);
  int nglobal = 0;
  for (int i = 0; i < nbad; i++) {
    if (bad[i] < 0 || bad[i] >= c.total || seen[bad[i]])
      return GFRS_ERR_INVALID_SHARDS; /* strict for every tactic */
    seen[bad[i]] = 1;
    nglobal += bad[i] < c.t.n + c.t.m;
  }
  bool slow = false;
  int rc = queue_pattern_check(c, bad, nbad, &slow);
  if (rc != GFRS_OK) return rc;
  r->nbad = nbad;
  /* the gate of gfrs_repair_batch's fused path */
  const gfrs_tactic &t = c.t;
  const bool fused = (t.l == 0 || lrc_single_pass(c)) && t.m >= 1 &&
                     t.m + t.l <= REPAIR_ROWS && c.total <= 16 &&
                     nglobal <= t.m && nbad <= REPAIR_ROWS;
  if (!fused) {
    r->cls = slow ? GFRS_RPAT_INPLACE_SLOW : GFRS_RPAT_INPLACE;
    return GFRS_OK;
  }
  r->cls = GFRS_RPAT_FUSED;
  r->nw = nbad;
  return repair_colpack(c.total, bad, nbad, &r->colpack);
}

int repair_pattern(const Code &c, const int32_t *bad, int nbad, Plan *p,
                   RepairPattern *r) {
  int rc = repair_pattern_check(c, bad, nbad, r);
  if (rc != GFRS_OK || r->cls != GFRS_RPAT_FUSED) return rc;
  if ((rc = plan_fused_repair(c, bad, nbad, p)) != GFRS_OK) return rc;
  r->gm = int(p->out.size());
  return GFRS_OK;
}

uint64_t repair_image_size(uint64_t shard_len) {
  const uint64_t frames = (shard_len - 1) / REPAIR_PAYLOAD + 1;
  return 32 + shard_len + 4 * frames + 8;
}

int repair_schedule(const gfrs_rjob *jobs, int njobs,
                    const RepairPattern *pats, int npat,
                    const int32_t *bad_idx, const int32_t *bad_off,
                    uint64_t dst_addr, const uint64_t *bids,
                    const uint64_t *vuids, RepairSchedule *out) {
  *out = RepairSchedule();
  if (njobs <= 0 || npat <= 0 || !jobs || !pats) return GFRS_ERR_INVALID_SHARDS;
  size_t count[REPAIR_ROWS + 1] = {0}, nimg = 0;
  for (int j = 0; j < njobs; j++) {
    const gfrs_rjob &jb = jobs[j];
    if (jb.pattern < 0 || jb.pattern >= npat || jb.reserved != 0)
      return GFRS_ERR_INVALID_SHARDS;
    if (jb.shard_len == 0) return GFRS_ERR_SHARD_NO_DATA;
    if ((dst_addr + jb.img_off) % 4 || jb.img_stride % 4 ||
        jb.img_stride < repair_image_size(jb.shard_len))
      return GFRS_ERR_INVALID_SHARDS;
    const RepairPattern &rp = pats[jb.pattern];
    if (rp.cls == GFRS_RPAT_FUSED) {
      if (rp.gm < rp.nbad || rp.gm > REPAIR_ROWS) return GFRS_ERR_UNSUPPORTED;
      count[rp.gm]++;
    } else {
      count[1] += size_t(rp.nbad);
    }
    nimg += size_t(rp.nbad);
  }
  size_t bucket_of[REPAIR_ROWS + 1], nitems = 0;
  for (int gm = 1; gm <= REPAIR_ROWS; gm++) {
    if (!count[gm]) continue;
    RepairBucket b;
    b.gm = gm;
    b.first = nitems;
    b.count = count[gm];
    b.prefix = nitems + out->buckets.size();
    bucket_of[gm] = out->buckets.size();
    nitems += count[gm];
    out->buckets.push_back(b);
  }
  out->items.reserve(nitems);
  out->images.reserve(nimg);
  /* caller order first: bucket by bucket below, a stable sort by descriptor
   * then leaves the items of one descriptor in caller order */
  std::vector<std::vector<gfrs_ritem>> per(REPAIR_ROWS + 1);
  for (int j = 0; j < njobs; j++) {
    const gfrs_rjob &jb = jobs[j];
    const RepairPattern &rp = pats[jb.pattern];
    const int32_t *bad = bad_idx + bad_off[jb.pattern];
    for (int b = 0; b < rp.nbad; b++) {
      const size_t id = out->images.size();
      out->images.push_back(gfrs_rimage{jb.img_off + uint64_t(b) * jb.img_stride,
                                        jb.shard_len, bids ? bids[id] : 0,
                                        vuids ? vuids[id] : 0});
      if (rp.cls != GFRS_RPAT_FUSED)
        per[1].push_back(gfrs_ritem{jb.off, jb.shard_len,
                                    jb.img_off + uint64_t(b) * jb.img_stride,
                                    jb.img_stride, j, npat + bad[b]});
    }
    if (rp.cls == GFRS_RPAT_FUSED)
      per[rp.gm].push_back(gfrs_ritem{jb.off, jb.shard_len, jb.img_off,
                                      jb.img_stride, j, jb.pattern});
    else
      out->inplace_jobs.push_back(j);
  }
  out->frame_prefix.assign(nitems + out->buckets.size(), 0);
  for (int gm = 1; gm <= REPAIR_ROWS; gm++) {
    if (!count[gm]) continue;
    std::stable_sort(per[gm].begin(), per[gm].end(),
                     [](const gfrs_ritem &a, const gfrs_ritem &b) {
                       return a.desc < b.desc;
                     });
    const RepairBucket &bk = out->buckets[bucket_of[gm]];
    for (size_t i = 0; i < per[gm].size(); i++) {
      out->items.push_back(per[gm][i]);
      out->frame_prefix[bk.prefix + i + 1] =
          out->frame_prefix[bk.prefix + i] +
          (per[gm][i].shard_len - 1) / REPAIR_PAYLOAD + 1;
    }
  }
  return GFRS_OK;
}

/* ---- the encode+frame queue ---- */

bool encode_frame_fused(const Code &c) {
  const gfrs_tactic &t = c.t;
  return t.m >= 1 && t.m + t.l <= 4 && c.total <= 16 &&
         (t.l == 0 || lrc_single_pass(c));
}

uint64_t encode_image_size(uint64_t shard_len) {
  return shard_len + 4 * ((shard_len - 1) / REPAIR_PAYLOAD + 1);
}

int encode_queue_block_check(int64_t block_len) {
  if (block_len <= 0 || block_len % 4096) return GFRS_ERR_INVALID_BLOCK;
  return block_len == REPAIR_BLOCK ? GFRS_OK : GFRS_ERR_UNSUPPORTED;
}

/* the buckets, items and prefix sums of validated jobs; frame_only puts the
 * jobs of the small class into the frame bucket below ENCQ_LARGE_MIN (the put
 * queue's wide tactics) */
static void encode_queue_fill(const gfrs_ejob *jobs, int njobs,
                              bool frame_only, EncSchedule *out) {
  /* slots 0..3: small NI 1..4; 4: frame below ENCQ_LARGE_MIN; 5: from it up */
  auto slot_of = [frame_only](uint64_t len) {
    if (len <= ENCQ_SMALL_MAX && !frame_only) return int((len - 1) / 1024);
    return len < ENCQ_LARGE_MIN ? 4 : 5;
  };
  size_t count[ENCQ_BUCKETS] = {0};
  for (int j = 0; j < njobs; j++) count[slot_of(jobs[j].shard_len)]++;
  size_t fill[ENCQ_BUCKETS], pre[ENCQ_BUCKETS] = {0}, nitems = 0, npre = 0;
  for (int s = 0; s < ENCQ_BUCKETS; s++) {
    fill[s] = nitems;
    if (!count[s]) continue;
    EncBucket b;
    b.kind = s < 4 ? GFRS_EQ_SMALL : GFRS_EQ_FRAME;
    b.param = s < 4 ? s + 1
                    : (s == 4 ? ENCQ_VAR_SMALL_SHARDS : ENCQ_VAR_LARGE_SHARDS);
    b.first = nitems;
    b.count = count[s];
    if (s >= 4) {
      b.prefix = pre[s] = npre;
      npre += count[s] + 1;
    }
    nitems += count[s];
    out->buckets.push_back(b);
  }
  out->items.resize(nitems);
  out->frame_prefix.assign(npre, 0);
  for (int j = 0; j < njobs; j++) {
    const gfrs_ejob &jb = jobs[j];
    const int s = slot_of(jb.shard_len);
    const size_t at = fill[s]++;
    out->items[at] =
        gfrs_eitem{jb.off, jb.shard_len, jb.img_off, jb.img_stride, j, 0};
    if (s >= 4) {
      const size_t pi = pre[s]++;
      out->frame_prefix[pi + 1] =
          out->frame_prefix[pi] + (jb.shard_len - 1) / REPAIR_PAYLOAD + 1;
    }
  }
}

int encode_queue_schedule(const gfrs_ejob *jobs, int njobs,
                          uint64_t framed_addr, EncSchedule *out) {
  *out = EncSchedule();
  if (njobs <= 0 || !jobs) return GFRS_ERR_INVALID_SHARDS;
  for (int j = 0; j < njobs; j++) {
    const gfrs_ejob &jb = jobs[j];
    if (jb.reserved != 0) return GFRS_ERR_INVALID_SHARDS;
    if (jb.shard_len == 0) return GFRS_ERR_SHARD_NO_DATA;
    if ((framed_addr + jb.img_off) % 4 || jb.img_stride % 4 ||
        jb.img_stride < encode_image_size(jb.shard_len))
      return GFRS_ERR_INVALID_SHARDS;
  }
  encode_queue_fill(jobs, njobs, false, out);
  return GFRS_OK;
}

/* ---- the read queue ---- */

int plan_read(const Code &c, const int32_t *bad, int nbad, Plan *p) {
  const int k = c.t.n, m = c.t.m;
  std::vector<uint8_t> present(k + m, 1);
  for (int i = 0; i < nbad; i++) {
    if (bad[i] < 0 || bad[i] >= c.total) return GFRS_ERR_INVALID_SHARDS;
    if (bad[i] < k + m) present[bad[i]] = 0; /* local parities: ignored */
  }
  std::vector<int32_t> gidx(k + m);
  for (int i = 0; i < k + m; i++) gidx[i] = i;
  const Engine g{k, m, c.enc_matrix.data(), gidx.data()};
  int rc = plan_decode(g, present.data(), p);
  if (rc != GFRS_OK) return rc;
  for (size_t ci = 0; ci < p->in.size() && ci < 32; ci++)
    if (p->in[ci] < k) p->pass_mask |= 1u << ci;
  return GFRS_OK;
}

int read_pattern_check(const Code &c, const int32_t *bad, int nbad,
                       ReadPattern *r) {
  *r = ReadPattern();
  if (nbad < 0 || (nbad > 0 && !bad)) return GFRS_ERR_INVALID_SHARDS;
  std::vector<uint8_t> seen(c.total, 0);
  int nglobal = 0, ndata = 0;
  for (int i = 0; i < nbad; i++) {
    if (bad[i] < 0 || bad[i] >= c.total || seen[bad[i]])
      return GFRS_ERR_INVALID_SHARDS;
    seen[bad[i]] = 1;
    nglobal += bad[i] < c.t.n + c.t.m;
    ndata += bad[i] < c.t.n;
  }
  if (nglobal > c.t.m) return GFRS_ERR_TOO_FEW_SHARDS;
  r->r = ndata;
  if (c.total <= 16)
    r->cls = ndata <= READ_ROWS ? GFRS_GPAT_FUSED : GFRS_GPAT_SLOW;
  else
    r->cls = ndata == 0 ? GFRS_GPAT_IDENTITY : GFRS_GPAT_SLOW;
  return GFRS_OK;
}

int read_pattern(const Code &c, const int32_t *bad, int nbad, Plan *p,
                 ReadPattern *r) {
  int rc = read_pattern_check(c, bad, nbad, r);
  if (rc != GFRS_OK) return rc;
  return plan_read(c, bad, nbad, p);
}

int read_queue_gate(const Code &c, int64_t block_len) {
  int rc = encode_queue_block_check(block_len);
  if (rc != GFRS_OK) return rc;
  return c.t.n + c.t.m <= READ_WORD_BITS ? GFRS_OK : GFRS_ERR_UNSUPPORTED;
}

int read_schedule(const Code &c, const gfrs_gjob *jobs, int njobs,
                  const ReadPattern *pats, int npat, uint64_t out_addr,
                  ReadSchedule *out) {
  *out = ReadSchedule();
  if (njobs <= 0 || npat <= 0 || !jobs || !pats) return GFRS_ERR_INVALID_SHARDS;
  const int n = c.t.n;
  size_t count[READ_ROWS + 1] = {0};
  for (int j = 0; j < njobs; j++) {
    const gfrs_gjob &jb = jobs[j];
    if (jb.pattern < 0 || jb.pattern >= npat || jb.reserved != 0)
      return GFRS_ERR_INVALID_SHARDS;
    if (jb.shard_len == 0 || jb.seg_len == 0) return GFRS_ERR_SHARD_NO_DATA;
    if (jb.seg_off % 4 || (out_addr + jb.out_off) % 4 || jb.out_stride % 4)
      return GFRS_ERR_INVALID_SHARDS;
    if (jb.out_stride < jb.seg_len ||
        jb.img_stride < encode_image_size(jb.shard_len) ||
        jb.seg_off > jb.shard_len || jb.seg_len > jb.shard_len - jb.seg_off)
      return GFRS_ERR_INVALID_SHARDS;
    const ReadPattern &rp = pats[jb.pattern];
    if (rp.cls == GFRS_GPAT_FUSED)
      count[rp.r]++;
    else if (rp.cls == GFRS_GPAT_IDENTITY)
      count[0] += size_t(n);
  }
  size_t bucket_of[READ_ROWS + 1], nitems = 0;
  for (int r = 0; r <= READ_ROWS; r++) {
    if (!count[r]) continue;
    ReadBucket b;
    b.r = r;
    b.first = nitems;
    b.count = count[r];
    b.prefix = nitems + out->buckets.size();
    bucket_of[r] = out->buckets.size();
    nitems += count[r];
    out->buckets.push_back(b);
  }
  out->items.reserve(nitems);
  /* caller order first; a stable sort by descriptor then leaves the items of
   * one descriptor in caller order */
  std::vector<std::vector<gfrs_gitem>> per(READ_ROWS + 1);
  for (int j = 0; j < njobs; j++) {
    const gfrs_gjob &jb = jobs[j];
    const ReadPattern &rp = pats[jb.pattern];
    gfrs_gitem it{jb.img_off, jb.img_stride, jb.shard_len, jb.seg_off,
                  jb.seg_len, jb.out_off,    jb.out_stride, j, jb.pattern};
    if (rp.cls == GFRS_GPAT_FUSED) {
      per[rp.r].push_back(it);
    } else if (rp.cls == GFRS_GPAT_IDENTITY) {
      for (int s = 0; s < n; s++) {
        it.desc = npat + s;
        per[0].push_back(it);
      }
    } else {
      out->slow_jobs.push_back(j);
    }
  }
  out->frame_prefix.assign(nitems + out->buckets.size(), 0);
  for (int r = 0; r <= READ_ROWS; r++) {
    if (!count[r]) continue;
    std::stable_sort(per[r].begin(), per[r].end(),
                     [](const gfrs_gitem &a, const gfrs_gitem &b) {
                       return a.desc < b.desc;
                     });
    const ReadBucket &bk = out->buckets[bucket_of[r]];
    for (size_t i = 0; i < per[r].size(); i++) {
      const gfrs_gitem &it = per[r][i];
      out->items.push_back(it);
      out->frame_prefix[bk.prefix + i + 1] =
          out->frame_prefix[bk.prefix + i] +
          (it.seg_off + it.seg_len - 1) / REPAIR_PAYLOAD -
          it.seg_off / REPAIR_PAYLOAD + 1;
    }
  }
  return GFRS_OK;
}

/* ---- the shard read queue ---- */

int shard_read_schedule(const gfrs_sjob *jobs, int njobs, uint64_t out_addr,
                        bool have_out, ShardReadSchedule *out) {
  *out = ShardReadSchedule();
  if (njobs <= 0 || !jobs) return GFRS_ERR_INVALID_SHARDS;
  constexpr uint32_t known = GFRS_SJOB_NO_OUT | GFRS_SJOB_FOOTER;
  size_t count[2] = {0, 0};
  for (int j = 0; j < njobs; j++) {
    const gfrs_sjob &jb = jobs[j];
    if (jb.reserved != 0 || (jb.flags & ~known)) return GFRS_ERR_INVALID_SHARDS;
    if (jb.size == 0) return GFRS_ERR_SHARD_NO_DATA;
    if (jb.size >> 32) return GFRS_ERR_INVALID_SHARDS;
    if (jb.from >= jb.to || jb.to > jb.size || jb.from % 4)
      return GFRS_ERR_INVALID_SHARDS;
    if ((jb.flags & GFRS_SJOB_FOOTER) && (jb.from != 0 || jb.to != jb.size))
      return GFRS_ERR_INVALID_SHARDS;
    const bool no_out = jb.flags & GFRS_SJOB_NO_OUT;
    if (!no_out && (!have_out || (out_addr + jb.out_off) % 4))
      return GFRS_ERR_INVALID_SHARDS;
    count[no_out]++;
  }
  size_t fill[2] = {0, 0}, pre[2] = {0, 0};
  for (int b = 0, nitems = 0; b < 2; b++) {
    if (!count[b]) continue;
    ShardReadBucket bk;
    bk.no_out = b;
    bk.first = fill[b] = size_t(nitems);
    bk.count = count[b];
    bk.prefix = pre[b] = size_t(nitems) + out->buckets.size();
    nitems += int(count[b]);
    out->buckets.push_back(bk);
  }
  out->items.resize(size_t(njobs));
  out->frame_prefix.assign(size_t(njobs) + out->buckets.size(), 0);
  out->job_frame.assign(size_t(njobs), 0);
  for (int j = 0; j < njobs; j++) {
    const gfrs_sjob &jb = jobs[j];
    const int b = (jb.flags & GFRS_SJOB_NO_OUT) ? 1 : 0;
    out->items[fill[b]++] = gfrs_sitem{jb.img_off, jb.size, jb.from, jb.to,
                                       jb.out_off, j,       jb.flags};
    const size_t pi = pre[b]++;
    out->job_frame[j] = out->frame_prefix[pi]; /* + frame_base, below */
    out->frame_prefix[pi + 1] = out->frame_prefix[pi] + shard_last_frame(jb) -
                                shard_first_frame(jb) + 1;
  }
  for (ShardReadBucket &bk : out->buckets) {
    bk.frame_base = out->total_frames;
    out->total_frames += out->frame_prefix[bk.prefix + bk.count];
  }
  if (out->buckets.size() == 2)
    for (int j = 0; j < njobs; j++)
      if (jobs[j].flags & GFRS_SJOB_NO_OUT)
        out->job_frame[j] += out->buckets[1].frame_base;
  return GFRS_OK;
}

/* ---- the shard write queue ---- */

int shard_write_schedule(const gfrs_wjob *jobs, int njobs, uint64_t dst_addr,
                         ShardWriteSchedule *out) {
  *out = ShardWriteSchedule();
  if (njobs <= 0 || !jobs) return GFRS_ERR_INVALID_SHARDS;
  constexpr uint32_t known = GFRS_WJOB_SRC_IMAGE;
  size_t count[2] = {0, 0};
  for (int j = 0; j < njobs; j++) {
    const gfrs_wjob &jb = jobs[j];
    if (jb.reserved != 0 || (jb.flags & ~known)) return GFRS_ERR_INVALID_SHARDS;
    if (jb.size == 0) return GFRS_ERR_SHARD_NO_DATA;
    if (jb.size >> 32) return GFRS_ERR_INVALID_SHARDS;
    if ((dst_addr + jb.img_off) % 4) return GFRS_ERR_INVALID_SHARDS;
    count[(jb.flags & GFRS_WJOB_SRC_IMAGE) ? 1 : 0]++;
  }
  size_t fill[2] = {0, 0}, pre[2] = {0, 0};
  for (int b = 0, nitems = 0; b < 2; b++) {
    if (!count[b]) continue;
    ShardWriteBucket bk;
    bk.src_image = b;
    bk.first = fill[b] = size_t(nitems);
    bk.count = count[b];
    bk.prefix = pre[b] = size_t(nitems) + out->buckets.size();
    nitems += int(count[b]);
    out->buckets.push_back(bk);
  }
  out->items.resize(size_t(njobs));
  out->frame_prefix.assign(size_t(njobs) + out->buckets.size(), 0);
  out->job_frame.assign(size_t(njobs), 0);
  for (int j = 0; j < njobs; j++) {
    const gfrs_wjob &jb = jobs[j];
    const int b = (jb.flags & GFRS_WJOB_SRC_IMAGE) ? 1 : 0;
    out->items[fill[b]++] =
        gfrs_witem{jb.src_off, jb.size, jb.img_off, j, jb.flags};
    const size_t pi = pre[b]++;
    out->job_frame[j] = out->frame_prefix[pi]; /* + frame_base, below */
    out->frame_prefix[pi + 1] =
        out->frame_prefix[pi] + (jb.size + REPAIR_PAYLOAD - 1) / REPAIR_PAYLOAD;
  }
  for (ShardWriteBucket &bk : out->buckets) {
    bk.frame_base = out->total_frames;
    out->total_frames += out->frame_prefix[bk.prefix + bk.count];
  }
  if (out->buckets.size() == 2)
    for (int j = 0; j < njobs; j++)
      if (jobs[j].flags & GFRS_WJOB_SRC_IMAGE)
        out->job_frame[j] += out->buckets[1].frame_base;
  return GFRS_OK;
}

/* ---- the put queue ---- */

int put_queue_gate(const Code &c, int64_t block_len) {
  int rc = encode_queue_block_check(block_len);
  if (rc != GFRS_OK) return rc;
  return c.t.m >= 1 && c.t.n <= PUT_MAX_N ? GFRS_OK : GFRS_ERR_UNSUPPORTED;
}

int put_queue_schedule(const Code &c, const gfrs_pjob *jobs, int njobs,
                       const uint64_t *vuids, int nvol, uint64_t dst_addr,
                       PutSchedule *out) {
  *out = PutSchedule();
  if (njobs <= 0 || nvol <= 0 || !jobs || !vuids)
    return GFRS_ERR_INVALID_SHARDS;
  for (int j = 0; j < njobs; j++) {
    const gfrs_pjob &jb = jobs[j];
    if (jb.reserved != 0 || jb.vol < 0 || jb.vol >= nvol)
      return GFRS_ERR_INVALID_SHARDS;
    if (jb.shard_len == 0) return GFRS_ERR_SHARD_NO_DATA;
    if (jb.shard_len >> 32) return GFRS_ERR_INVALID_SHARDS;
    if ((dst_addr + jb.img_off) % 4 || jb.img_stride % 4 ||
        jb.img_stride < repair_image_size(jb.shard_len))
      return GFRS_ERR_INVALID_SHARDS;
  }
  const int rows = c.t.m + c.t.l;
  out->wide = !encode_frame_fused(c);
  for (int r = 0; r < rows; r += PUT_ROWS)
    out->group_rows.push_back(rows - r < PUT_ROWS ? rows - r : PUT_ROWS);
  /* the body of an image is an encode-queue image 32 bytes in */
  std::vector<gfrs_ejob> ej;
  ej.resize(size_t(njobs));
  out->images.reserve(size_t(njobs) * c.total);
  for (int j = 0; j < njobs; j++) {
    const gfrs_pjob &jb = jobs[j];
    ej[j] = gfrs_ejob{jb.off, jb.shard_len, jb.img_off + 32, jb.img_stride, 0};
    for (int i = 0; i < c.total; i++)
      out->images.push_back(
          gfrs_rimage{jb.img_off + uint64_t(i) * jb.img_stride, jb.shard_len,
                      jb.bid, vuids[size_t(jb.vol) * c.total + i]});
  }
  encode_queue_fill(ej.data(), njobs, out->wide, &out->enc);
  return GFRS_OK;
}

}  // namespace gfrs

/* ---- GPU-free diagnostic export (include/gfrs.h) ---- */

extern "C" int gfrs_compute_put_queue_schedule(
    const gfrs_tactic *t, const gfrs_pjob *jobs, int njobs,
    const uint64_t *vuids, int nvol, int64_t block_len, int item_cap,
    int image_cap, gfrs_eitem *items, uint64_t *frame_prefix, int *nitems,
    gfrs_ebucket *buckets, int *nbuckets, gfrs_rimage *images, int *nimages,
    int *wide, int *ngroups, int32_t *group_rows) {
  using namespace gfrs;
  if (!tactic_valid(t)) return GFRS_ERR_INVALID_CODEMODE;
  Code c;
  c.t = *t; /* the gate reads the tactic only */
  int rc = put_queue_gate(c, block_len);
  if (rc != GFRS_OK) return rc;
  if (!code_build(*t, &c)) return GFRS_ERR_SINGULAR;
  PutSchedule s;
  if ((rc = put_queue_schedule(c, jobs, njobs, vuids, nvol, 0, &s)) != GFRS_OK)
    return rc;
  if (s.enc.items.size() > size_t(item_cap < 0 ? 0 : item_cap) ||
      s.images.size() > size_t(image_cap < 0 ? 0 : image_cap))
    return GFRS_ERR_NOMEM;
  *nitems = int(s.enc.items.size());
  *nbuckets = int(s.enc.buckets.size());
  *nimages = int(s.images.size());
  *wide = s.wide ? 1 : 0;
  *ngroups = int(s.group_rows.size());
  std::copy(s.enc.items.begin(), s.enc.items.end(), items);
  std::copy(s.enc.frame_prefix.begin(), s.enc.frame_prefix.end(), frame_prefix);
  std::copy(s.images.begin(), s.images.end(), images);
  std::copy(s.group_rows.begin(), s.group_rows.end(), group_rows);
  for (size_t b = 0; b < s.enc.buckets.size(); b++)
    buckets[b] = gfrs_ebucket{s.enc.buckets[b].kind, s.enc.buckets[b].param,
                              int32_t(s.enc.buckets[b].first),
                              int32_t(s.enc.buckets[b].count)};
  return GFRS_OK;
}

extern "C" int gfrs_compute_shard_write_queue_schedule(
    const gfrs_wjob *jobs, int njobs, int64_t block_len, int item_cap,
    gfrs_witem *items, uint64_t *frame_prefix, int *nitems,
    gfrs_wbucket *buckets, int *nbuckets, uint64_t *total_frames) {
  using namespace gfrs;
  int rc = encode_queue_block_check(block_len);
  if (rc != GFRS_OK) return rc;
  ShardWriteSchedule s;
  if ((rc = shard_write_schedule(jobs, njobs, 0, &s)) != GFRS_OK) return rc;
  if (s.items.size() > size_t(item_cap < 0 ? 0 : item_cap))
    return GFRS_ERR_NOMEM;
  *nitems = int(s.items.size());
  *nbuckets = int(s.buckets.size());
  *total_frames = s.total_frames;
  std::copy(s.items.begin(), s.items.end(), items);
  std::copy(s.frame_prefix.begin(), s.frame_prefix.end(), frame_prefix);
  for (size_t b = 0; b < s.buckets.size(); b++)
    buckets[b] =
        gfrs_wbucket{s.buckets[b].src_image, int32_t(s.buckets[b].first),
                     int32_t(s.buckets[b].count), 0};
  return GFRS_OK;
}

extern "C" int gfrs_compute_shard_read_queue_schedule(
    const gfrs_sjob *jobs, int njobs, int64_t block_len, int item_cap,
    gfrs_sitem *items, uint64_t *frame_prefix, int *nitems,
    gfrs_sbucket *buckets, int *nbuckets, uint64_t *total_frames) {
  using namespace gfrs;
  int rc = encode_queue_block_check(block_len);
  if (rc != GFRS_OK) return rc;
  ShardReadSchedule s;
  if ((rc = shard_read_schedule(jobs, njobs, 0, true, &s)) != GFRS_OK)
    return rc;
  if (s.items.size() > size_t(item_cap < 0 ? 0 : item_cap))
    return GFRS_ERR_NOMEM;
  *nitems = int(s.items.size());
  *nbuckets = int(s.buckets.size());
  *total_frames = s.total_frames;
  std::copy(s.items.begin(), s.items.end(), items);
  std::copy(s.frame_prefix.begin(), s.frame_prefix.end(), frame_prefix);
  for (size_t b = 0; b < s.buckets.size(); b++)
    buckets[b] = gfrs_sbucket{s.buckets[b].no_out, int32_t(s.buckets[b].first),
                              int32_t(s.buckets[b].count), 0};
  return GFRS_OK;
}

extern "C" int gfrs_compute_read_queue_schedule(
    const gfrs_tactic *t, const gfrs_gjob *jobs, int njobs,
    const int32_t *bad_idx, const int32_t *bad_off, int npat,
    int64_t block_len, int item_cap, gfrs_gitem *items,
    uint64_t *frame_prefix, int *nitems, gfrs_gbucket *buckets, int *nbuckets,
    int32_t *pat_class, int32_t *pat_r, int32_t *slow_jobs, int *nslow) {
  using namespace gfrs;
  if (!tactic_valid(t) || t->m == 0) return GFRS_ERR_INVALID_CODEMODE;
  Code c;
  if (!code_build(*t, &c)) return GFRS_ERR_SINGULAR;
  int rc = read_queue_gate(c, block_len);
  if (rc != GFRS_OK) return rc;
  if (njobs <= 0 || npat <= 0) return GFRS_ERR_INVALID_SHARDS;
  if ((rc = queue_offsets_check(bad_off, npat)) != GFRS_OK) return rc;
  std::vector<ReadPattern> pats(npat);
  for (int p = 0; p < npat; p++) {
    Plan pl;
    rc = read_pattern(c, bad_idx + bad_off[p], bad_off[p + 1] - bad_off[p],
                      &pl, &pats[p]);
    if (rc != GFRS_OK) return rc;
  }
  ReadSchedule s;
  if ((rc = read_schedule(c, jobs, njobs, pats.data(), npat, 0, &s)) != GFRS_OK)
    return rc;
  if (s.items.size() > size_t(item_cap < 0 ? 0 : item_cap))
    return GFRS_ERR_NOMEM;
  *nitems = int(s.items.size());
  *nbuckets = int(s.buckets.size());
  *nslow = int(s.slow_jobs.size());
  std::copy(s.items.begin(), s.items.end(), items);
  std::copy(s.frame_prefix.begin(), s.frame_prefix.end(), frame_prefix);
  for (size_t b = 0; b < s.buckets.size(); b++)
    buckets[b] = gfrs_gbucket{s.buckets[b].r, int32_t(s.buckets[b].first),
                              int32_t(s.buckets[b].count), 0};
  for (int p = 0; p < npat; p++) {
    pat_class[p] = pats[p].cls;
    pat_r[p] = pats[p].r;
  }
  std::copy(s.slow_jobs.begin(), s.slow_jobs.end(), slow_jobs);
  return GFRS_OK;
}

extern "C" int gfrs_compute_encode_queue_schedule(
    const gfrs_tactic *t, const gfrs_ejob *jobs, int njobs, int64_t block_len,
    int item_cap, gfrs_eitem *items, uint64_t *frame_prefix, int *nitems,
    gfrs_ebucket *buckets, int *nbuckets, int *fused) {
  using namespace gfrs;
  if (!tactic_valid(t) || t->m == 0) return GFRS_ERR_INVALID_CODEMODE;
  int rc = encode_queue_block_check(block_len);
  if (rc != GFRS_OK) return rc;
  Code c;
  if (!code_build(*t, &c)) return GFRS_ERR_SINGULAR;
  EncSchedule s;
  if ((rc = encode_queue_schedule(jobs, njobs, 0, &s)) != GFRS_OK) return rc;
  if (s.items.size() > size_t(item_cap < 0 ? 0 : item_cap))
    return GFRS_ERR_NOMEM;
  *nitems = int(s.items.size());
  *nbuckets = int(s.buckets.size());
  *fused = encode_frame_fused(c) ? 1 : 0;
  std::copy(s.items.begin(), s.items.end(), items);
  std::copy(s.frame_prefix.begin(), s.frame_prefix.end(), frame_prefix);
  for (size_t b = 0; b < s.buckets.size(); b++)
    buckets[b] = gfrs_ebucket{s.buckets[b].kind, s.buckets[b].param,
                              int32_t(s.buckets[b].first),
                              int32_t(s.buckets[b].count)};
  return GFRS_OK;
}

extern "C" int gfrs_compute_repair_queue_schedule(
    const gfrs_tactic *t, const gfrs_rjob *jobs, int njobs,
    const int32_t *bad_idx, const int32_t *bad_off, int npat,
    int64_t block_len, const uint64_t *bids, const uint64_t *vuids,
    int item_cap, int image_cap, gfrs_ritem *items, uint64_t *frame_prefix,
    int *nitems, gfrs_rbucket *buckets, int *nbuckets, gfrs_rimage *images,
    int *nimages, int32_t *pat_class, int32_t *pat_gm, int32_t *pat_nw,
    uint32_t *pat_colpack, int32_t *inplace_jobs, int *ninplace) {
  using namespace gfrs;
  if (!tactic_valid(t) || t->m == 0) return GFRS_ERR_INVALID_CODEMODE;
  if (njobs <= 0 || npat <= 0) return GFRS_ERR_INVALID_SHARDS;
  int rc = queue_offsets_check(bad_off, npat);
  if (rc != GFRS_OK) return rc;
  Code c;
  if (!code_build(*t, &c)) return GFRS_ERR_SINGULAR;
  std::vector<RepairPattern> pats(npat);
  for (int p = 0; p < npat; p++) {
    Plan pl;
    rc = repair_pattern(c, bad_idx + bad_off[p], bad_off[p + 1] - bad_off[p],
                        &pl, &pats[p]);
    if (rc != GFRS_OK) return rc;
  }
  if (block_len != REPAIR_BLOCK) return GFRS_ERR_UNSUPPORTED;
  RepairSchedule s;
  rc = repair_schedule(jobs, njobs, pats.data(), npat, bad_idx, bad_off, 0,
                       bids, vuids, &s);
  if (rc != GFRS_OK) return rc;
  if (s.items.size() > size_t(item_cap < 0 ? 0 : item_cap) ||
      s.images.size() > size_t(image_cap < 0 ? 0 : image_cap))
    return GFRS_ERR_NOMEM;
  *nitems = int(s.items.size());
  *nbuckets = int(s.buckets.size());
  *nimages = int(s.images.size());
  *ninplace = int(s.inplace_jobs.size());
  std::copy(s.items.begin(), s.items.end(), items);
  std::copy(s.frame_prefix.begin(), s.frame_prefix.end(), frame_prefix);
  for (size_t b = 0; b < s.buckets.size(); b++)
    buckets[b] = gfrs_rbucket{s.buckets[b].gm, int32_t(s.buckets[b].first),
                              int32_t(s.buckets[b].count), 0};
  std::copy(s.images.begin(), s.images.end(), images);
  for (int p = 0; p < npat; p++) {
    pat_class[p] = pats[p].cls;
    pat_gm[p] = pats[p].gm;
    pat_nw[p] = pats[p].nw;
    pat_colpack[p] = pats[p].colpack;
  }
  std::copy(s.inplace_jobs.begin(), s.inplace_jobs.end(), inplace_jobs);
  return GFRS_OK;
}

extern "C" int gfrs_compute_queue_schedule(
    const gfrs_tactic *t, const gfrs_qjob *jobs, int njobs,
    const int32_t *bad_idx, const int32_t *bad_off, int npat, int item_cap,
    int bucket_cap, gfrs_qitem *items, uint64_t *tile_prefix, int *nitems,
    gfrs_qbucket *buckets, int *nbuckets, int32_t *pat_nout,
    uint8_t *pat_slow, int32_t *slow_jobs, int *nslow) {
  using namespace gfrs;
  if (!tactic_valid(t) || t->m == 0) return GFRS_ERR_INVALID_CODEMODE;
  if (njobs <= 0 || npat <= 0) return GFRS_ERR_INVALID_SHARDS;
  int rc = queue_offsets_check(bad_off, npat);
  if (rc != GFRS_OK) return rc;
  Code c;
  if (!code_build(*t, &c)) return GFRS_ERR_SINGULAR;
  std::vector<QueuePattern> pats(npat);
  for (int p = 0; p < npat; p++) {
    Plan pl;
    rc = queue_pattern(c, bad_idx + bad_off[p], bad_off[p + 1] - bad_off[p],
                       &pl, &pats[p]);
    if (rc != GFRS_OK) return rc;
  }
  QueueSchedule s;
  if ((rc = queue_schedule(jobs, njobs, pats.data(), npat, &s)) != GFRS_OK)
    return rc;
  if (s.items.size() > size_t(item_cap < 0 ? 0 : item_cap) ||
      s.buckets.size() > size_t(bucket_cap < 0 ? 0 : bucket_cap))
    return GFRS_ERR_NOMEM;
  *nitems = int(s.items.size());
  *nbuckets = int(s.buckets.size());
  *nslow = int(s.slow_jobs.size());
  std::copy(s.items.begin(), s.items.end(), items);
  std::copy(s.tile_prefix.begin(), s.tile_prefix.end(), tile_prefix);
  for (size_t b = 0; b < s.buckets.size(); b++)
    buckets[b] = gfrs_qbucket{s.buckets[b].g, s.buckets[b].gm,
                              int32_t(s.buckets[b].first),
                              int32_t(s.buckets[b].count)};
  for (int p = 0; p < npat; p++) {
    pat_nout[p] = pats[p].nout;
    pat_slow[p] = pats[p].slow;
  }
  std::copy(s.slow_jobs.begin(), s.slow_jobs.end(), slow_jobs);
  return GFRS_OK;
}

extern "C" int gfrs_compute_plan(const gfrs_tactic *t, int kind,
                                 const int32_t *bad, int nbad, int cap,
                                 int32_t *in, int *nin, int32_t *out,
                                 int *nout, uint8_t *rows, int *rowk,
                                 uint32_t *cmp_mask, uint32_t *colpack) {
  using namespace gfrs;
  if (!tactic_valid(t) || t->m == 0) return GFRS_ERR_INVALID_CODEMODE;
  Code c;
  if (!code_build(*t, &c)) return GFRS_ERR_SINGULAR;
  Plan p;
  int rc = GFRS_ERR_UNSUPPORTED;
  if (kind == GFRS_PLAN_FUSED_LRC_ENCODE) rc = plan_fused_lrc(c, &p);
  if (kind == GFRS_PLAN_RS_RECONSTRUCT_VERIFY)
    rc = plan_rs_reconstruct_verify(c, bad, nbad, &p);
  if (kind == GFRS_PLAN_LRC_RECONSTRUCT_VERIFY)
    rc = plan_lrc_reconstruct_verify(c, bad, nbad, &p);
  if (kind == GFRS_PLAN_FUSED_REPAIR) rc = plan_fused_repair(c, bad, nbad, &p);
  if (kind == GFRS_PLAN_READ) {
    ReadPattern rp;
    rc = read_pattern(c, bad, nbad, &p, &rp);
    p.colpack = p.pass_mask;
  }
  if (rc != GFRS_OK) return rc;
  if (int(p.in.size()) > cap || int(p.out.size()) > cap) return GFRS_ERR_NOMEM;
  *nin = int(p.in.size());
  *nout = int(p.out.size());
  *rowk = p.rowk;
  *cmp_mask = p.cmp_mask;
  *colpack = p.colpack;
  std::copy(p.in.begin(), p.in.end(), in);
  std::copy(p.out.begin(), p.out.end(), out);
  std::copy(p.rows.begin(), p.rows.end(), rows);
  return GFRS_OK;
}
