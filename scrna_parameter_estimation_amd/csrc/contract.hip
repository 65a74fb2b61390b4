// contract.hip -- K9+K10: per-test linear contraction over replicate groups and null statistics.
//
// Reference behaviour replaced (memento/hypothesis_test.py):
//   :249-251  valid_boostrap_iters -- drop replicate columns with any non-finite entry (mean OR var rows)
//   :262-271, :290-291  weighted mean / (residualise on covariates + _cross_coef): LINEAR in the response,
//             so the host folds it into one weight row W[t][:] per test (see memento/design.py)
//   :297-298  nanstd of the replicate coefficients -> standard error
//   :62-92    _compute_asl: all-equal check, null = coef[1:] - coef[0], two-sided extreme count
// One 256-thread workgroup per test; replicates across lanes (coalesced along b).
#include "mm_common.h"
#include <math.h>

#define K9_THREADS 256

// workgroup reduction: xor butterfly inside each wave, then the wave results in ascending order starting from ``init``
template <class Op>
__device__ __forceinline__ double wg_reduce(double x, double *red, double init, Op op) {
  for (int off = 32; off > 0; off >>= 1) x = op(x, __shfl_xor(x, off, 64));
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  double t = init;
  for (int i = 0; i < K9_THREADS / 64; i++) t = op(t, red[i]);
  return t;
}
__device__ __forceinline__ double wg_sum(double x, double *red) {
  return wg_reduce(x, red, 0.0, [](double a, double b) { return a + b; });
}
__device__ __forceinline__ double wg_min(double x, double *red) {
  return wg_reduce(x, red, INFINITY, [](double a, double b) { return fmin(a, b); });
}
__device__ __forceinline__ double wg_max(double x, double *red) {
  return wg_reduce(x, red, -INFINITY, [](double a, double b) { return fmax(a, b); });
}

// ------------------------------------------------------------------------------------------------
// THE TEST RECORD.  Every statistics kernel of this file writes, per test and response plane, the same 8 doubles
//   [0] coef0      the observed coefficient (replicate column 0)
//   [1] se         sqrt(mean squared deviation of coef[1:] about its mean) over the valid columns   (hypothesis_test.py:297-298)
//   [2] n_valid    number of valid columns among 1..B
//   [3] n_extreme  #{ |coef[c] - coef0| > |coef0| }   (_compute_asl, hypothesis_test.py:62-92)
//   [4] mean(coef[1:]) - coef0
//   [5] all_equal  1 when every valid coefficient, column 0 included, is the same number
//   [6] n_raw_extreme  #{ |coef[c]| > |coef0| }: the null NOT centred on the observed value (resampling != 'bootstrap')
//   [7] range      max - min over the valid columns, column 0 included
// and the kernels differ only in how the coefficient of a column is obtained.
__device__ __forceinline__ void write_nan_record(double *st) {   // a test with nothing to test
  if (threadIdx.x == 0)
    for (int i = 0; i < 8; i++) st[i] = (i == 2 || i == 3 || i == 5) ? 0.0 : NAN;
}

// Fill the records st[0..NP) of one test from ``coef_at(c, v)``: it puts the NP coefficients of replicate column c into v and
// returns whether the column is valid (one verdict for all planes) and leaves NaN in v where it is not: coef0 = v of column 0.  Called
// by all K9_THREADS threads of the workgroup.  Pass A: count / sum / min / max; pass B: squared deviations and the extreme
// counts.  STORED = false: pass B calls coef_at again (nothing per-replicate is stored; row is unused).  STORED = true
// (NP == 1): pass A stores the coefficient row in ``row``, which is also an output, and pass B reads it back; invalid
// columns are NaN in it.
template <int NP, bool STORED, class F>
__device__ __forceinline__ void fill_records(F coef_at, int n_cols, double *row, double *const (&st)[NP], double *red) {
  double v[NP], sum[NP], lo[NP], hi[NP], cnt = 0.0;
  for (int k = 0; k < NP; k++) { sum[k] = 0.0; lo[k] = INFINITY; hi[k] = -INFINITY; }
  for (int c = threadIdx.x; c < n_cols; c += K9_THREADS) {
    bool ok = coef_at(c, v);
    if (STORED) row[c] = v[0];
    if (ok) {
      for (int k = 0; k < NP; k++) { lo[k] = fmin(lo[k], v[k]); hi[k] = fmax(hi[k], v[k]); }
      if (c > 0) {
        for (int k = 0; k < NP; k++) sum[k] += v[k];
        cnt += 1.0;
      }
    }
  }
  double n = wg_sum(cnt, red);
  for (int k = 0; k < NP; k++) sum[k] = wg_sum(sum[k], red);
  for (int k = 0; k < NP; k++) { lo[k] = wg_min(lo[k], red); hi[k] = wg_max(hi[k], red); }
  double c0[NP], mean[NP], a0[NP], sq[NP], ext[NP], raw[NP];
  if (STORED) {
    __threadfence_block();
    __syncthreads();
    c0[0] = row[0];
  } else {
    coef_at(0, c0);
  }
  for (int k = 0; k < NP; k++) {
    mean[k] = n > 0 ? sum[k] / n : NAN;
    a0[k] = fabs(c0[k]);
    sq[k] = ext[k] = raw[k] = 0.0;
  }
  for (int c = 1 + threadIdx.x; c < n_cols; c += K9_THREADS) {
    bool ok;
    if (STORED) { v[0] = row[c]; ok = v[0] == v[0]; }
    else ok = coef_at(c, v);
    if (ok) {
      for (int k = 0; k < NP; k++) {
        double d = v[k] - mean[k];
        sq[k] += d * d;
        double nul = v[k] - c0[k];
        if (nul > a0[k] || nul < -a0[k]) ext[k] += 1.0;
        if (v[k] > a0[k] || v[k] < -a0[k]) raw[k] += 1.0;
      }
    }
  }
  for (int k = 0; k < NP; k++) sq[k] = wg_sum(sq[k], red);
  for (int k = 0; k < NP; k++) ext[k] = wg_sum(ext[k], red);
  for (int k = 0; k < NP; k++) raw[k] = wg_sum(raw[k], red);
  if (threadIdx.x == 0) {
    for (int k = 0; k < NP; k++) {
      double *s = st[k];
      s[0] = c0[k];
      s[1] = n > 0 ? sqrt(sq[k] / n) : NAN;
      s[2] = n;
      s[3] = ext[k];
      s[4] = mean[k] - c0[k];
      s[5] = (lo[k] == hi[k]) ? 1.0 : 0.0;
      s[6] = raw[k];
      s[7] = hi[k] - lo[k];
    }
  }
}

__global__ __launch_bounds__(K9_THREADS) void k_contract_stats(const double *__restrict__ ym, const double *__restrict__ yv, int64_t ld,
                                                               int32_t num_boot, int32_t n_groups, const int32_t *__restrict__ test_gene,
                                                               const double *__restrict__ W, const uint8_t *__restrict__ good,
                                                               int32_t which, double *__restrict__ coef, double *__restrict__ stats) {
  extern __shared__ double sm[];
  double *wrow = sm;                              // [n_groups]
  int32_t *glist = (int32_t *)(sm + n_groups);    // [n_groups] indices of good groups
  __shared__ double red[K9_THREADS / 64];
  __shared__ int n_good_s;
  int64_t t = blockIdx.x;
  int gene = test_gene[t];
  const uint8_t *gd = good + (int64_t)gene * n_groups;
  if (threadIdx.x == 0) {
    int ng = 0;
    for (int j = 0; j < n_groups; j++)
      if (gd[j]) glist[ng++] = j;
    n_good_s = ng;
  }
  for (int j = threadIdx.x; j < n_groups; j += K9_THREADS) wrow[j] = W[t * n_groups + j];
  __syncthreads();
  int n_good = n_good_s;
  double *crow = coef + t * ld;
  double *const st[1] = {stats + t * 8};
  int64_t row_base = (int64_t)gene * n_groups;
  int n_cols = num_boot + 1;
  if (n_good == 0) {
    for (int c = threadIdx.x; c < n_cols; c += K9_THREADS) crow[c] = NAN;
    write_nan_record(st[0]);
    return;
  }
  auto coef_at = [&](int c, double(&v)[1]) {
    double acc = 0.0;
    bool ok = true;
    for (int q = 0; q < n_good; q++) {
      int j = glist[q];
      int64_t o = (row_base + j) * ld + c;
      double a = ym[o], b = yv[o];
      ok = ok && isfinite(a) && isfinite(b);
      acc += wrow[j] * (which ? b : a);
    }
    v[0] = ok ? acc : NAN;   // dropped replicates are stored as NaN
    return ok;
  };
  fill_records<1, true>(coef_at, n_cols, crow, st, red);
}

// ------------------------------------------------------------------------------------------------
// resample_rep=True (hypothesis_test.py:273-286, :231-239): hierarchical resampling of the replicate groups.
// Step 0: which replicate columns survive hypothesis_test.py:249-251 (a column is dropped when ANY good group has a
// non-finite mean OR variance entry).  One workgroup per gene: col_map[gene][k] = k-th surviving column (ascending),
// n_valid[gene] = how many.  With nothing dropped col_map is the identity and n_valid = num_boot + 1.
__global__ __launch_bounds__(256) void k_valid_cols(const double *__restrict__ ym, const double *__restrict__ yv, int64_t ld,
                                                    int32_t num_boot, int32_t n_groups, const uint8_t *__restrict__ good,
                                                    int32_t *__restrict__ col_map, int32_t *__restrict__ n_valid) {
  extern __shared__ int32_t glist_v[];             // [n_groups] indices of good groups
  __shared__ int n_good_s, base_s;
  __shared__ int wave_cnt[4];
  int64_t gene = blockIdx.x;
  const uint8_t *gd = good + gene * n_groups;
  if (threadIdx.x == 0) {
    int ng = 0;
    for (int j = 0; j < n_groups; j++)
      if (gd[j]) glist_v[ng++] = j;
    n_good_s = ng;
    base_s = 0;
  }
  __syncthreads();
  int n_good = n_good_s;
  int n_cols = num_boot + 1;
  int32_t *cm = col_map + gene * (int64_t)n_cols;
  int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int c0 = 0; c0 < n_cols; c0 += 256) {
    int c = c0 + threadIdx.x;
    bool ok = c < n_cols;
    if (ok) {
      for (int q = 0; q < n_good; q++) {
        int64_t o = (gene * n_groups + glist_v[q]) * ld + c;
        ok = ok && isfinite(ym[o]) && isfinite(yv[o]);
      }
    }
    uint64_t bal = __ballot(ok);
    int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wave_cnt[wv] = __popcll(bal);
    __syncthreads();
    int off = base_s;
    for (int w = 0; w < wv; w++) off += wave_cnt[w];
    if (ok) cm[off + before] = c;
    __syncthreads();
    if (threadIdx.x == 0) base_s += wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    __syncthreads();
  }
  if (threadIdx.x == 0) n_valid[gene] = base_s;
}

// Step 1: residualise the rows of a gene on the covariates, dst = M src  (M = I - H of the weighted fit, zero on bad
// groups), column by column.  Any number of groups (one group per donor is the reference's real use of resample_rep,
// analysis/lupus/run_memento.py:31-52): row i of M is staged in LDS, the column entries come back from L1/L2.
// The sum runs over j in ascending order and skips exact zeros of M (rows that are all zero, i.e. bad groups, give NaN).
__global__ __launch_bounds__(256) void k_residualize(const double *__restrict__ src, double *__restrict__ dst, int64_t ld,
                                                     int32_t n_cols, int32_t n_groups, int32_t col_tiles,
                                                     const int32_t *__restrict__ gene_mask /* [n_genes] index into M */,
                                                     const double *__restrict__ M /* [n_masks][ng][ng] */) {
  extern __shared__ double mrow[];                 // [n_groups]
  int64_t gene = blockIdx.x / col_tiles;
  int tile = (int)(blockIdx.x % col_tiles);
  const double *Mg = M + (int64_t)gene_mask[gene] * n_groups * n_groups;
  int c = tile * 256 + threadIdx.x;
  bool mine = c < n_cols;
  const double *sb = src + gene * n_groups * ld + c;
  double *db = dst + gene * n_groups * ld + c;
  for (int i = 0; i < n_groups; i++) {
    __syncthreads();
    for (int j = threadIdx.x; j < n_groups; j += 256) mrow[j] = Mg[(int64_t)i * n_groups + j];
    __syncthreads();
    if (!mine) continue;
    double acc = 0.0;
    bool any = false;
    for (int j = 0; j < n_groups; j++) {
      double m = mrow[j];
      if (m != 0.0) {
        acc += m * sb[(int64_t)j * ld];
        any = true;
      }
    }
    db[(int64_t)i * ld] = any ? acc : NAN;
  }
}

__device__ __forceinline__ uint64_t rr_mix(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// Step 2: per test and resampled column c < nb (nb = surviving columns - 1, hypothesis_test.py:249-254): rows i = 0..n-1 take
// group rep[i][c] and the bcol[i][c]-th SURVIVING replicate column of the residualised response; coefficient = weighted slope
// on the residualised treatment of the drawn groups (_cross_coef_resampled).  rep/bcol NULL -> drawn on the fly from a
// counter-based RNG (column 0 is always the identity / observed column).  rep/bcol rows have stride num_boot.  Then the
// test record, read back from the stored row as in k_contract_stats.
__global__ __launch_bounds__(K9_THREADS) void k_cross_resampled(const double *__restrict__ yt, int64_t ld, int32_t num_boot,
                                                                int32_t n_groups, const int32_t *__restrict__ test_gene,
                                                                const double *__restrict__ tt /* [n_tests][ng] residualised treatment */,
                                                                const uint8_t *__restrict__ good, const double *__restrict__ Nc,
                                                                const int16_t *__restrict__ rep, const int32_t *__restrict__ bcol,
                                                                const int32_t *__restrict__ col_map, const int32_t *__restrict__ n_valid,
                                                                const int64_t *__restrict__ gene_key /* NULL: the gene's slot */,
                                                                uint64_t seed, double *__restrict__ coef, double *__restrict__ stats) {
  extern __shared__ double sm[];
  double *tts = sm;                               // [ng]
  double *ncs = sm + n_groups;                    // [ng]
  int32_t *glist = (int32_t *)(sm + 2 * n_groups);
  __shared__ double red[K9_THREADS / 64];
  __shared__ int n_good_s;
  int64_t t = blockIdx.x;
  int gene = test_gene[t];
  const uint8_t *gd = good + (int64_t)gene * n_groups;
  if (threadIdx.x == 0) {
    int ng = 0;
    for (int j = 0; j < n_groups; j++)
      if (gd[j]) glist[ng++] = j;
    n_good_s = ng;
  }
  for (int j = threadIdx.x; j < n_groups; j += K9_THREADS) {
    tts[j] = tt[t * n_groups + j];
    ncs[j] = Nc[j];
  }
  __syncthreads();
  int n = n_good_s;
  double *crow = coef + t * ld;
  double *const st[1] = {stats + t * 8};
  int64_t row_base = (int64_t)gene * n_groups;
  if (n == 0) {
    for (int c = threadIdx.x; c <= num_boot; c += K9_THREADS) crow[c] = NAN;
    write_nan_record(st[0]);
    return;
  }
  const int16_t *rg = rep ? rep + (int64_t)gene * n_groups * num_boot : nullptr;
  const int32_t *bg = bcol ? bcol + (int64_t)gene * n_groups * num_boot : nullptr;
  // surviving replicate columns (hypothesis_test.py:249-254): nb resampled columns, indices through col_map
  const int32_t *cm = col_map ? col_map + (int64_t)gene * (num_boot + 1) : nullptr;
  const int nb = n_valid ? n_valid[gene] - 1 : num_boot;
  const uint64_t gk = gene_key ? (uint64_t)gene_key[gene] : (uint64_t)gene;
  if (nb < 1) {    // nothing (or only one column) survives: the reference returns NaNs ("skipped") or has no null at all
    for (int c = threadIdx.x; c <= num_boot; c += K9_THREADS) crow[c] = NAN;
    write_nan_record(st[0]);
    return;
  }
  for (int c = nb + threadIdx.x; c <= num_boot; c += K9_THREADS) crow[c] = NAN;  // the resampled row uses nb <= num_boot slots
  auto coef_at = [&](int c, double(&v)[1]) {
    double sw = 0.0, swy = 0.0, swa = 0.0, amax = 0.0;
    // first pass: weighted means
    for (int i = 0; i < n; i++) {
      int r, bb;
      if (c == 0) { r = i; bb = 0; }
      else if (rg) { r = rg[(int64_t)i * num_boot + c]; bb = bg[(int64_t)i * num_boot + c]; }
      else {
        uint64_t h = rr_mix(seed ^ rr_mix((gk << 32) ^ ((uint64_t)i << 24) ^ (uint64_t)c));
        r = (int)(h % (uint64_t)n);
        bb = (int)(rr_mix(h) % (uint64_t)nb) + 1;
      }
      if (cm) bb = cm[bb];
      int j = glist[r];
      double y = yt[(row_base + j) * ld + bb];
      double w = ncs[j];
      sw += w; swy += w * y; swa += w * tts[j];
      amax = fmax(amax, fabs(tts[j]));
    }
    double mB = swy / sw, mA = swa / sw;
    double ss = 0.0, num = 0.0;
    for (int i = 0; i < n; i++) {
      int r, bb;
      if (c == 0) { r = i; bb = 0; }
      else if (rg) { r = rg[(int64_t)i * num_boot + c]; bb = bg[(int64_t)i * num_boot + c]; }
      else {
        uint64_t h = rr_mix(seed ^ rr_mix((gk << 32) ^ ((uint64_t)i << 24) ^ (uint64_t)c));
        r = (int)(h % (uint64_t)n);
        bb = (int)(rr_mix(h) % (uint64_t)nb) + 1;
      }
      if (cm) bb = cm[bb];
      int j = glist[r];
      double y = yt[(row_base + j) * ld + bb];
      double w = ncs[j], da = tts[j] - mA;
      ss += da * da * w;
      num += (da * w) * (y - mB);
    }
    // DELIBERATE DEVIATION: a degenerate column -- every drawn group has the same (residualised)
    // treatment, so the slope is 0/0.  The reference gets NaN there when its weighted mean happens to round to exactly that
    // value and O(1) noise otherwise (hypothesis_test.py:234-239: a ratio of two round-off residues, one of which comes out of
    // LAPACK's least-squares residuals and is not reproducible bit for bit); here such a column is always NaN, which np.nanstd
    // and the isfinite filter of _compute_asl ignore.  With >= 12 groups such columns do not occur (P < 1e-3 per column).
    double val = num / sw / (ss / sw);
    if (ss / sw <= 1e-24 * amax * amax) val = NAN;
    v[0] = val;
    return val == val;
  };
  fill_records<1, true>(coef_at, nb, crow, st, red);
}

// ------------------------------------------------------------------------------------------------
// Step 2, gene-major (ht_1d_eqtl: hundreds of cis SNPs per gene, analysis/lupus/run_memento.py:84-109): the tests arrive as a CSR
// gene_ptr over tt, and one workgroup takes a TILE of XB_TT consecutive tests of one gene.  The draws (rep, bcol) of a column
// depend on the gene, not on the test, so a thread obtains each draw of its column once per pass -- table or hash, col_map,
// glist, the yt read, the weight -- and applies it to all XB_TT tests, whose accumulators it keeps in registers; the tile's tt
// rows sit in LDS test-minor, so that a draw reads XB_TT consecutive doubles.  For every (test, column) the operations and their
// order over i are those of k_cross_resampled, so with the same key the coefficient is that kernel's bit for bit; the columns go
// to the threads and the partial sums through wg_reduce as in fill_records, so the whole record is.  Nothing per replicate is
// stored: pass B of the record computes the coefficients again, and mm_cross_resampled on a subset gives the rows of the few
// tests that need them.
// XB_TT = 8: the record's pass B keeps 3 doubles and 2 counts per test (c0, mean, sq; ext, raw) next to the 4 doubles of a
// coefficient's second pass (mA, ss, num, amax): 16 VGPRs per test, 128 for the tile, which with the operands in flight stays
// inside the 256 registers at which two waves share a SIMD; 16 tests would need the whole file for one wave.  LDS: (XB_TT + 1.5) * 8 B per group, 19 KB at 250 donors.
#define XB_TT 8

// fill_records with ONE VALIDITY PER PLANE: plane k of ``coef_at(c, v)`` is valid at column c when v[k] is not NaN (a column can
// be degenerate for one SNP and not for its neighbour).  Nothing is stored; the records of the first n_used planes are written.
// Column order per thread and reduction order are those of fill_records.
template <int NP, class F>
__device__ __forceinline__ void fill_records_each(F coef_at, int n_cols, double *(&st)[NP], int n_used, double *red) {
  double v[NP], sum[NP], lo[NP], hi[NP], cnt[NP];
  for (int k = 0; k < NP; k++) { sum[k] = 0.0; cnt[k] = 0.0; lo[k] = INFINITY; hi[k] = -INFINITY; }
  for (int c = threadIdx.x; c < n_cols; c += K9_THREADS) {
    coef_at(c, v);
    for (int k = 0; k < NP; k++) {
      if (v[k] == v[k]) {
        lo[k] = fmin(lo[k], v[k]); hi[k] = fmax(hi[k], v[k]);
        if (c > 0) { sum[k] += v[k]; cnt[k] += 1.0; }
      }
    }
  }
  for (int k = 0; k < NP; k++) cnt[k] = wg_sum(cnt[k], red);
  for (int k = 0; k < NP; k++) sum[k] = wg_sum(sum[k], red);
  for (int k = 0; k < NP; k++) { lo[k] = wg_min(lo[k], red); hi[k] = wg_max(hi[k], red); }
  double c0[NP], mean[NP], sq[NP];
  int ext[NP], raw[NP];      // (counts: exact either way, and half the registers)
  coef_at(0, c0);
  for (int k = 0; k < NP; k++) {
    mean[k] = cnt[k] > 0 ? sum[k] / cnt[k] : NAN;
    sq[k] = 0.0;
    ext[k] = raw[k] = 0;
  }
  for (int c = 1 + threadIdx.x; c < n_cols; c += K9_THREADS) {
    coef_at(c, v);
    for (int k = 0; k < NP; k++) {
      if (v[k] == v[k]) {
        double d = v[k] - mean[k];
        sq[k] += d * d;
        double nul = v[k] - c0[k], a0 = fabs(c0[k]);
        if (nul > a0 || nul < -a0) ext[k]++;
        if (v[k] > a0 || v[k] < -a0) raw[k]++;
      }
    }
  }
  for (int k = 0; k < NP; k++) sq[k] = wg_sum(sq[k], red);
  double n_ext[NP], n_raw[NP];
  for (int k = 0; k < NP; k++) n_ext[k] = wg_sum((double)ext[k], red);
  for (int k = 0; k < NP; k++) n_raw[k] = wg_sum((double)raw[k], red);
  if (threadIdx.x == 0) {
    for (int k = 0; k < NP; k++) {
      if (k >= n_used) break;
      double *s = st[k];
      s[0] = c0[k];
      s[1] = cnt[k] > 0 ? sqrt(sq[k] / cnt[k]) : NAN;
      s[2] = cnt[k];
      s[3] = n_ext[k];
      s[4] = mean[k] - c0[k];
      s[5] = (lo[k] == hi[k]) ? 1.0 : 0.0;
      s[6] = n_raw[k];
      s[7] = hi[k] - lo[k];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// A covariate PER TEST (ht_1d_eqtl(interaction=): the genotype main effect g_s beside the tested g_s * ctx).  With M the shared
// residual maker and z = M g_s, residualising on [shared | g_s] is M followed by a rank-one step (Frisch-Waugh):
//   y_t[j][c] = (M y)[j][c] - z[j] * beta[c],   beta[c] = sum_j Nc_j z_j (M y)[j][c] / sum_j Nc_j z_j^2   over the good groups.
// The three routines below are the only place where the weights, beta and y_t are formed: k_cross_cov_beta (beta of a tile into a
// scratch), k_cross_resampled_block_cov (reads that scratch) and k_residualize_rank1 (materialises y_t) share them, so under
// -ffp-contract=off the response a test sees is the same number on every route.
// cov_weights: IN PLACE, zs[j * NT + k] (z of test k at group j) becomes Nc_j z_j / sum Nc z^2; the sum runs over the good groups
// in ascending order, a zero sum gives zero weights (beta = 0: the host passes z = 0 for a covariate inside the shared span).
// Thread k < NT does test k; the caller puts a barrier on either side.
template <int NT>
__device__ __forceinline__ void cov_weights(double *zs, const double *__restrict__ Nc, const int32_t *glist, int n) {
  if (threadIdx.x < NT) {
    const int k = threadIdx.x;
    double den = 0.0;
    for (int q = 0; q < n; q++) {
      int j = glist[q];
      double z = zs[(size_t)j * NT + k];
      den += Nc[j] * z * z;
    }
    for (int q = 0; q < n; q++) {
      int j = glist[q];
      double z = zs[(size_t)j * NT + k];
      zs[(size_t)j * NT + k] = den > 0.0 ? Nc[j] * z / den : 0.0;
    }
  }
}
// cov_beta: beta of NT tests at replicate column c from the weights wz [ng][NT]: good groups in ascending order, one read of the
// residualised plane per group (columns across threads: coalesced).
template <int NT>
__device__ __forceinline__ void cov_beta(const double *__restrict__ yt, int64_t ld, int64_t row_base, const int32_t *glist, int n,
                                         const double *wz, int c, double (&b)[NT]) {
  for (int k = 0; k < NT; k++) b[k] = 0.0;
  for (int q = 0; q < n; q++) {
    int j = glist[q];
    double y = yt[(row_base + j) * ld + c];
    const double *w = wz + (size_t)j * NT;
    for (int k = 0; k < NT; k++) b[k] += w[k] * y;
  }
}
__device__ __forceinline__ double cov_residual(double y, double z, double beta) { return y - z * beta; }

// The coefficients of ONE TILE of XB_TT tests of a gene at replicate column c, shared by the record kernel
// (k_cross_resampled_block) and the family kernel (k_cross_family_max): for every (test, column) the operations of k_cross_resampled
// in its order.  tts [ng][XB_TT] test-minor, ncs [ng] and glist [n] are in LDS; rg / bg / cm (or NULL) are the gene's own tables.
// COV (k_cross_resampled_block_cov): every test has a covariate of its own, taken out of the shared response by a rank-one step:
// test k reads y - zts[j][k] * beta[bb][k] where the others read y (zts [ng][XB_TT] in LDS, beta [ld][XB_TT] of this tile from
// k_cross_cov_beta), so the response sums swy and mB are per test.
template <bool COV>
struct CrossTileT {
  const double *__restrict__ yt;
  int64_t ld;
  int32_t num_boot;
  const double *tts, *ncs;
  const int32_t *glist;
  int n, nb;
  int64_t row_base;
  const int16_t *__restrict__ rg;
  const int32_t *__restrict__ bg, *__restrict__ cm;
  uint64_t gk, seed;
  const double *zts = nullptr;
  const double *__restrict__ beta = nullptr;
  // row i of column c: the drawn group (index into yt / ncs / tts), the response there and the replicate column it came from
  __device__ __forceinline__ void draw(int i, int c, int &j, double &y, int &bb) const {
    int r;
    if (c == 0) { r = i; bb = 0; }
    else if (rg) { r = rg[(int64_t)i * num_boot + c]; bb = bg[(int64_t)i * num_boot + c]; }
    else {
      uint64_t h = rr_mix(seed ^ rr_mix((gk << 32) ^ ((uint64_t)i << 24) ^ (uint64_t)c));
      r = (int)(h % (uint64_t)n);
      bb = (int)(rr_mix(h) % (uint64_t)nb) + 1;
    }
    if (cm) bb = cm[bb];
    j = glist[r];
    y = yt[(row_base + j) * ld + bb];
  }
  __device__ __forceinline__ void coef_at(int c, double (&v)[XB_TT]) const {
    constexpr int NY = COV ? XB_TT : 1;      // response sums: one per test under COV, else one for the tile
    double sw = 0.0, swy[NY], swa[XB_TT], amax[XB_TT];
    for (int k = 0; k < NY; k++) swy[k] = 0.0;
    for (int k = 0; k < XB_TT; k++) swa[k] = amax[k] = 0.0;
    for (int i = 0; i < n; i++) {
      int j, bb;
      double y;
      draw(i, c, j, y, bb);
      double w = ncs[j];
      const double *a = tts + (size_t)j * XB_TT;
      sw += w;
      if (COV) {
        const double *z = zts + (size_t)j * XB_TT, *b = beta + (size_t)bb * XB_TT;
        for (int k = 0; k < NY; k++) swy[k] += w * cov_residual(y, z[k], b[k]);
      } else {
        swy[0] += w * y;
      }
      for (int k = 0; k < XB_TT; k++) {
        swa[k] += w * a[k];
        amax[k] = fmax(amax[k], fabs(a[k]));
      }
    }
    double ss[XB_TT], num[XB_TT];
    for (int k = 0; k < NY; k++) swy[k] = swy[k] / sw;                                     // swy is mB from here on
    for (int k = 0; k < XB_TT; k++) { swa[k] = swa[k] / sw; ss[k] = num[k] = 0.0; }      // swa is mA from here on
    for (int i = 0; i < n; i++) {
      int j, bb;
      double y;
      draw(i, c, j, y, bb);
      double w = ncs[j], dy = y - swy[0];
      const double *a = tts + (size_t)j * XB_TT;
      const double *z = COV ? zts + (size_t)j * XB_TT : nullptr, *b = COV ? beta + (size_t)bb * XB_TT : nullptr;
      for (int k = 0; k < XB_TT; k++) {
        double da = a[k] - swa[k];
        if (COV) dy = cov_residual(y, z[k], b[k]) - swy[k < NY ? k : 0];
        ss[k] += da * da * w;
        num[k] += (da * w) * dy;
      }
    }
    for (int k = 0; k < XB_TT; k++) {      // the degenerate-column rule of k_cross_resampled
      double val = num[k] / sw / (ss[k] / sw);
      if (ss[k] / sw <= 1e-24 * amax[k] * amax[k]) val = NAN;
      v[k] = val;
    }
  }
};
using CrossTile = CrossTileT<false>;

__global__ __launch_bounds__(K9_THREADS, 2) void k_cross_resampled_block(
    const double *__restrict__ yt, int64_t ld, int32_t num_boot, int32_t n_groups, int32_t tiles_per_gene,
    const int32_t *__restrict__ gene_ptr /* [n_genes + 1] CSR over the tests */,
    const double *__restrict__ tt /* [n_tests][ng] residualised treatment */, const uint8_t *__restrict__ good,
    const double *__restrict__ Nc, const int16_t *__restrict__ rep, const int32_t *__restrict__ bcol,
    const int32_t *__restrict__ col_map, const int32_t *__restrict__ n_valid, const int64_t *__restrict__ gene_key, uint64_t seed,
    double *__restrict__ stats) {
  extern __shared__ double sm[];
  double *tts = sm;                                        // [ng][XB_TT], test-minor
  double *ncs = sm + (size_t)XB_TT * n_groups;             // [ng]
  int32_t *glist = (int32_t *)(ncs + n_groups);            // [ng] indices of good groups
  __shared__ double red[K9_THREADS / 64];
  __shared__ int n_good_s;
  const int gene = (int)(blockIdx.x / (unsigned)tiles_per_gene);
  const int64_t t0 = (int64_t)gene_ptr[gene] + (int64_t)(blockIdx.x % (unsigned)tiles_per_gene) * XB_TT;
  const int64_t t1 = gene_ptr[gene + 1];
  if (t0 >= t1) return;                                    // (uniform over the workgroup) a gene without tests, or past its last tile
  const int nt = (int)(t1 - t0 < XB_TT ? t1 - t0 : XB_TT);  // the gene's last tile may be partial: its other slots compute on zeros
  const uint8_t *gd = good + (int64_t)gene * n_groups;
  if (threadIdx.x == 0) {
    int ng = 0;
    for (int j = 0; j < n_groups; j++)
      if (gd[j]) glist[ng++] = j;
    n_good_s = ng;
  }
  for (int j = threadIdx.x; j < n_groups; j += K9_THREADS) {
    for (int k = 0; k < XB_TT; k++) tts[(size_t)j * XB_TT + k] = k < nt ? tt[(t0 + k) * n_groups + j] : 0.0;
    ncs[j] = Nc[j];
  }
  __syncthreads();
  const int n = n_good_s;
  double *st[XB_TT];
  for (int k = 0; k < XB_TT; k++) st[k] = stats + (t0 + (k < nt ? k : 0)) * 8;
  const int64_t row_base = (int64_t)gene * n_groups;
  const int nb = n_valid ? n_valid[gene] - 1 : num_boot;
  if (n == 0 || nb < 1) {
    for (int k = 0; k < nt; k++) write_nan_record(st[k]);
    return;
  }
  const int16_t *rg = rep ? rep + (int64_t)gene * n_groups * num_boot : nullptr;
  const int32_t *bg = bcol ? bcol + (int64_t)gene * n_groups * num_boot : nullptr;
  const int32_t *cm = col_map ? col_map + (int64_t)gene * (num_boot + 1) : nullptr;
  const uint64_t gk = gene_key ? (uint64_t)gene_key[gene] : (uint64_t)gene;
  const CrossTile tile{yt, ld, num_boot, tts, ncs, glist, n, nb, row_base, rg, bg, cm, gk, seed};
  auto coef_at = [&](int c, double(&v)[XB_TT]) { tile.coef_at(c, v); };
  fill_records_each<XB_TT>(coef_at, nb, st, nt, red);
}

// beta of the tiles tile_lo + blockIdx.x / col_tiles: beta[(blockIdx.x / col_tiles)][c][k] for the columns c <= num_boot, 256 a
// workgroup.  A tile past its gene's last test writes nothing (nobody reads its block).
__global__ __launch_bounds__(K9_THREADS) void k_cross_cov_beta(
    const double *__restrict__ yt, int64_t ld, int32_t num_boot, int32_t n_groups, int32_t tiles_per_gene, int32_t tile_lo,
    int32_t col_tiles, const int32_t *__restrict__ gene_ptr, const double *__restrict__ zt /* [n_tests][ng] */,
    const uint8_t *__restrict__ good, const double *__restrict__ Nc, double *__restrict__ beta /* [tiles][ld][XB_TT] */) {
  extern __shared__ double sm[];
  double *wz = sm;                                         // [ng][XB_TT], test-minor: z, then the weights
  int32_t *glist = (int32_t *)(sm + (size_t)XB_TT * n_groups);
  __shared__ int n_good_s;
  const unsigned slot = blockIdx.x / (unsigned)col_tiles, tile = (unsigned)tile_lo + slot;
  const int c = (int)(blockIdx.x % (unsigned)col_tiles) * K9_THREADS + (int)threadIdx.x;
  const int gene = (int)(tile / (unsigned)tiles_per_gene);
  const int64_t t0 = (int64_t)gene_ptr[gene] + (int64_t)(tile % (unsigned)tiles_per_gene) * XB_TT;
  const int64_t t1 = gene_ptr[gene + 1];
  if (t0 >= t1) return;
  const int nt = (int)(t1 - t0 < XB_TT ? t1 - t0 : XB_TT);
  const uint8_t *gd = good + (int64_t)gene * n_groups;
  if (threadIdx.x == 0) {
    int ng = 0;
    for (int j = 0; j < n_groups; j++)
      if (gd[j]) glist[ng++] = j;
    n_good_s = ng;
  }
  for (int j = threadIdx.x; j < n_groups; j += K9_THREADS)
    for (int k = 0; k < XB_TT; k++) wz[(size_t)j * XB_TT + k] = k < nt ? zt[(t0 + k) * n_groups + j] : 0.0;
  __syncthreads();
  const int n = n_good_s;
  cov_weights<XB_TT>(wz, Nc, glist, n);
  __syncthreads();
  if (c > num_boot) return;
  double b[XB_TT];
  cov_beta<XB_TT>(yt, ld, (int64_t)gene * n_groups, glist, n, wz, c, b);
  double *out = beta + ((size_t)slot * ld + c) * XB_TT;
  for (int k = 0; k < XB_TT; k++) out[k] = b[k];
}

// k_cross_resampled_block with a covariate per test (zt [n_tests][ng] beside tt): the tiles tile_lo + blockIdx.x, whose beta blocks
// ([ld][XB_TT] each) a launch of k_cross_cov_beta over the same range wrote before this one on the same stream.  The set-up is
// k_cross_resampled_block's, kept apart from it so that that kernel's code does not move; the tile's zt rows sit in LDS beside tts.
__global__ __launch_bounds__(K9_THREADS, 2) void k_cross_resampled_block_cov(
    const double *__restrict__ yt, int64_t ld, int32_t num_boot, int32_t n_groups, int32_t tiles_per_gene, int32_t tile_lo,
    const int32_t *__restrict__ gene_ptr, const double *__restrict__ tt, const double *__restrict__ zt,
    const uint8_t *__restrict__ good, const double *__restrict__ Nc, const int16_t *__restrict__ rep, const int32_t *__restrict__ bcol,
    const int32_t *__restrict__ col_map, const int32_t *__restrict__ n_valid, const int64_t *__restrict__ gene_key, uint64_t seed,
    const double *__restrict__ beta, double *__restrict__ stats) {
  extern __shared__ double sm[];
  double *tts = sm;                                        // [ng][XB_TT], test-minor
  double *zts = sm + (size_t)XB_TT * n_groups;             // [ng][XB_TT], test-minor
  double *ncs = zts + (size_t)XB_TT * n_groups;            // [ng]
  int32_t *glist = (int32_t *)(ncs + n_groups);            // [ng] indices of good groups
  __shared__ double red[K9_THREADS / 64];
  __shared__ int n_good_s;
  const unsigned tile = (unsigned)tile_lo + blockIdx.x;
  const int gene = (int)(tile / (unsigned)tiles_per_gene);
  const int64_t t0 = (int64_t)gene_ptr[gene] + (int64_t)(tile % (unsigned)tiles_per_gene) * XB_TT;
  const int64_t t1 = gene_ptr[gene + 1];
  if (t0 >= t1) return;
  const int nt = (int)(t1 - t0 < XB_TT ? t1 - t0 : XB_TT);
  const uint8_t *gd = good + (int64_t)gene * n_groups;
  if (threadIdx.x == 0) {
    int ng = 0;
    for (int j = 0; j < n_groups; j++)
      if (gd[j]) glist[ng++] = j;
    n_good_s = ng;
  }
  for (int j = threadIdx.x; j < n_groups; j += K9_THREADS) {
    for (int k = 0; k < XB_TT; k++) {
      tts[(size_t)j * XB_TT + k] = k < nt ? tt[(t0 + k) * n_groups + j] : 0.0;
      zts[(size_t)j * XB_TT + k] = k < nt ? zt[(t0 + k) * n_groups + j] : 0.0;
    }
    ncs[j] = Nc[j];
  }
  __syncthreads();
  const int n = n_good_s;
  double *st[XB_TT];
  for (int k = 0; k < XB_TT; k++) st[k] = stats + (t0 + (k < nt ? k : 0)) * 8;
  const int64_t row_base = (int64_t)gene * n_groups;
  const int nb = n_valid ? n_valid[gene] - 1 : num_boot;
  if (n == 0 || nb < 1) {
    for (int k = 0; k < nt; k++) write_nan_record(st[k]);
    return;
  }
  const int16_t *rg = rep ? rep + (int64_t)gene * n_groups * num_boot : nullptr;
  const int32_t *bg = bcol ? bcol + (int64_t)gene * n_groups * num_boot : nullptr;
  const int32_t *cm = col_map ? col_map + (int64_t)gene * (num_boot + 1) : nullptr;
  const uint64_t gk = gene_key ? (uint64_t)gene_key[gene] : (uint64_t)gene;
  const CrossTileT<true> tile_c{yt, ld, num_boot, tts, ncs, glist, n, nb, row_base, rg, bg, cm, gk, seed, zts,
                                beta + (size_t)blockIdx.x * ld * XB_TT};
  auto coef_at = [&](int c, double(&v)[XB_TT]) { tile_c.coef_at(c, v); };
  fill_records_each<XB_TT>(coef_at, nb, st, nt, red);
}

// y_t of a short LIST of tests, materialised: out[l][j][c] = yt[gene_l][j][c] - z_l[j] * beta_l[c] on the good groups of
// gene_l = test_gene[l] and the columns c <= num_boot (NaN on the other groups), with the weights, beta and the subtraction of
// the routines above -- mm_cross_resampled_keyed on ``out`` with test l on row block l then gives, bit for bit, the coefficients
// that k_cross_resampled_block_cov forms for that test.  One workgroup per (l, 256 columns).
__global__ __launch_bounds__(K9_THREADS) void k_residualize_rank1(
    const double *__restrict__ yt, int64_t ld, int32_t num_boot, int32_t n_groups, int32_t col_tiles,
    const int32_t *__restrict__ test_gene /* [n_list] */, const double *__restrict__ zt /* [n_list][ng] */,
    const uint8_t *__restrict__ good, const double *__restrict__ Nc, double *__restrict__ out /* [n_list][ng][ld] */) {
  extern __shared__ double sm[];
  double *zs = sm;                                         // [ng] z
  double *wz = sm + n_groups;                              // [ng] the weights
  int32_t *glist = (int32_t *)(wz + n_groups);
  __shared__ int n_good_s;
  const int64_t l = blockIdx.x / (unsigned)col_tiles;
  const int c = (int)(blockIdx.x % (unsigned)col_tiles) * K9_THREADS + (int)threadIdx.x;
  const int gene = test_gene[l];
  const uint8_t *gd = good + (int64_t)gene * n_groups;
  if (threadIdx.x == 0) {
    int ng = 0;
    for (int j = 0; j < n_groups; j++)
      if (gd[j]) glist[ng++] = j;
    n_good_s = ng;
  }
  for (int j = threadIdx.x; j < n_groups; j += K9_THREADS) zs[j] = wz[j] = zt[l * n_groups + j];
  __syncthreads();
  const int n = n_good_s;
  cov_weights<1>(wz, Nc, glist, n);
  __syncthreads();
  if (c > num_boot) return;
  const int64_t row_base = (int64_t)gene * n_groups;
  double b[1];
  cov_beta<1>(yt, ld, row_base, glist, n, wz, c, b);
  for (int j = 0; j < n_groups; j++)
    out[(l * n_groups + j) * ld + c] = gd[j] ? cov_residual(yt[(row_base + j) * ld + c], zs[j], b[0]) : NAN;
}

// ------------------------------------------------------------------------------------------------
// Guide-vs-control contrasts (ht_1d_vs_control, ht_2d_vs_control): test t applies the sparse weight row of design
// d = test_design[t] to the replicate rows of row block test_row[t] (a gene slot, or a pair of Bootstrap2D) on NP response planes:
//   coef_c = sum_p design_w[p] * y[test_row[t] * n_groups + design_grp[p]][c]  for p in [design_ptr[d], design_ptr[d + 1]).
// With covariates (replicate / well / dose strata) the row is the per-guide weighted regression of _regress_1d
// (hypothesis_test.py:242-300) on the guide's and the control's stratum groups, folded into weights by memento/design.py.  The
// plain two-group test against a shared control (BASELINE config 5; the weighted slope of _cross_coef for two groups and a binary
// treatment, hypothesis_test.py:218-228) is the design {(guide, +1), (control, -1)}: the library is built with -ffp-contract=off,
// so design_coef forms (0.0 + 1.0 * a) + (-1.0 * b), which is a - b bit for bit except that an exact zero is always +0.0 -- and no
// count, flag or comparison of the record sees the sign of a zero.  The control's bootstrap rows are computed once and shared by
// every guide.
// Column c is valid only if every listed group is finite there in EVERY plane (:249-251, :372-373; groups with a ~0 weight
// included): one verdict for all planes.  An empty design (no good guide or control group, or no stratum holding both arms) gives
// the NaN record.  One workgroup per test; the coefficient is recomputed in the second pass instead of being stored (a test reads
// 2 x |design| rows; the control rows are shared by a row block's consecutive tests through L2 / MALL).  The routines take the
// number of planes NP as a template parameter: k_contrast_design_* is NP = 2 (ym, yv of Bootstrap1D), k_contrast_design1_* NP = 1
// (the replicate correlations of Bootstrap2D), which reads every byte once, tests it once and writes one record.
// design_coef<NP>: the coefficient of column c on NP response planes at once (each operand offset and weight read once);
// returns whether the column is valid and leaves NaN in v where it is not.
template <int NP>
__device__ __forceinline__ bool design_coef(const double *const (&y)[NP], int64_t ld, int64_t row_base, const int32_t *__restrict__ grp,
                                            const double *__restrict__ w, int p0, int p1, int c, double (&v)[NP]) {
  bool good = true;
  for (int k = 0; k < NP; k++) v[k] = 0.0;
  for (int p = p0; p < p1; p++) {
    int64_t o = (row_base + grp[p]) * ld + c;
    double wp = w[p];
    for (int k = 0; k < NP; k++) {
      double a = y[k][o];
      good = good && isfinite(a);
      v[k] += wp * a;
    }
  }
  if (!good)
    for (int k = 0; k < NP; k++) v[k] = NAN;
  return good;
}

// One workgroup = one test, on NP planes.  y[k]: plane k; st[k]: record k of this test.
template <int NP>
__device__ __forceinline__ void design_test(const double *const (&y)[NP], int64_t ld, int32_t num_boot, int32_t n_groups, int row, int d,
                                            const int32_t *__restrict__ design_ptr, const int32_t *__restrict__ design_grp,
                                            const double *__restrict__ design_w, double *const (&st)[NP], double *red) {
  int p0 = design_ptr[d], p1 = design_ptr[d + 1];
  if (p1 <= p0) {
    for (int k = 0; k < NP; k++) write_nan_record(st[k]);
    return;
  }
  int64_t row_base = (int64_t)row * n_groups;
  auto coef_at = [&](int c, double(&v)[NP]) { return design_coef<NP>(y, ld, row_base, design_grp, design_w, p0, p1, c, v); };
  fill_records<NP, false>(coef_at, num_boot + 1, nullptr, st, red);
}

// The coefficient row of one test on plane ``which`` (for the host-side tail fits); NaN in the columns that are not valid
template <int NP>
__device__ __forceinline__ void design_rows(const double *const (&y)[NP], int64_t ld, int32_t num_boot, int32_t n_groups, int row, int d,
                                            const int32_t *__restrict__ design_ptr, const int32_t *__restrict__ design_grp,
                                            const double *__restrict__ design_w, int32_t which, double *__restrict__ out_row) {
  int p0 = design_ptr[d], p1 = design_ptr[d + 1];
  int64_t row_base = (int64_t)row * n_groups;
  for (int c = threadIdx.x; c <= num_boot; c += 256) {
    double v[NP];
    bool ok = design_coef<NP>(y, ld, row_base, design_grp, design_w, p0, p1, c, v);
    out_row[c] = (ok && p1 > p0) ? (which ? v[NP - 1] : v[0]) : NAN;
  }
}

__global__ __launch_bounds__(K9_THREADS) void k_contrast_design_stats(const double *__restrict__ ym, const double *__restrict__ yv,
                                                                      int64_t ld, int32_t num_boot, int32_t n_groups,
                                                                      const int32_t *__restrict__ test_gene,
                                                                      const int32_t *__restrict__ test_design,
                                                                      const int32_t *__restrict__ design_ptr,
                                                                      const int32_t *__restrict__ design_grp,
                                                                      const double *__restrict__ design_w, double *__restrict__ stats_m,
                                                                      double *__restrict__ stats_v) {
  __shared__ double red[K9_THREADS / 64];
  int64_t t = blockIdx.x;
  const double *const y[2] = {ym, yv};
  double *const st[2] = {stats_m + t * 8, stats_v + t * 8};
  design_test<2>(y, ld, num_boot, n_groups, test_gene[t], test_design[t], design_ptr, design_grp, design_w, st, red);
}

__global__ __launch_bounds__(256) void k_contrast_design_rows(const double *__restrict__ ym, const double *__restrict__ yv, int64_t ld,
                                                              int32_t num_boot, int32_t n_groups, const int32_t *__restrict__ test_gene,
                                                              const int32_t *__restrict__ test_design,
                                                              const int32_t *__restrict__ design_ptr,
                                                              const int32_t *__restrict__ design_grp,
                                                              const double *__restrict__ design_w, int32_t which,
                                                              double *__restrict__ out) {
  int64_t t = blockIdx.x;
  const double *const y[2] = {ym, yv};
  design_rows<2>(y, ld, num_boot, n_groups, test_gene[t], test_design[t], design_ptr, design_grp, design_w, which, out + t * ld);
}

__global__ __launch_bounds__(K9_THREADS) void k_contrast_design1_stats(const double *__restrict__ y, int64_t ld, int32_t num_boot,
                                                                       int32_t n_groups, const int32_t *__restrict__ test_row,
                                                                       const int32_t *__restrict__ test_design,
                                                                       const int32_t *__restrict__ design_ptr,
                                                                       const int32_t *__restrict__ design_grp,
                                                                       const double *__restrict__ design_w, double *__restrict__ stats) {
  __shared__ double red[K9_THREADS / 64];
  int64_t t = blockIdx.x;
  const double *const yp[1] = {y};
  double *const st[1] = {stats + t * 8};
  design_test<1>(yp, ld, num_boot, n_groups, test_row[t], test_design[t], design_ptr, design_grp, design_w, st, red);
}

__global__ __launch_bounds__(256) void k_contrast_design1_rows(const double *__restrict__ y, int64_t ld, int32_t num_boot, int32_t n_groups,
                                                               const int32_t *__restrict__ test_row,
                                                               const int32_t *__restrict__ test_design,
                                                               const int32_t *__restrict__ design_ptr,
                                                               const int32_t *__restrict__ design_grp,
                                                               const double *__restrict__ design_w, double *__restrict__ out) {
  int64_t t = blockIdx.x;
  const double *const yp[1] = {y};
  design_rows<1>(yp, ld, num_boot, n_groups, test_row[t], test_design[t], design_ptr, design_grp, design_w, 0, out + t * ld);
}

// ------------------------------------------------------------------------------------------------
// Single-step max-T adjustment over a FAMILY of design contrasts (ht_1d_posthoc): the tests [family_ptr[f], family_ptr[f + 1]) are the
// m members of family f; they share the row block test_row and each has its design, as in k_contrast_design_stats.  Every (row,
// group) chain is bootstrapped once, so replicate column c of all members is one joint draw of the whole family, and
//   M[c] = max_j |coef_j[c] - coef_j[0]| * scale_j,   t0_j = |coef_j[0]| * scale_j,   n_adj_j = #{ family-valid c : M[c] > t0_j }
// per plane (Westfall-Young within the family; the host forms p_adj_j = (1 + n_adj_j) / (1 + n_valid_family)).  Member j is INCLUDED
// on a plane when its scale there is a finite number > 0 and its column 0 is valid (the host passes 1 / se, and 0 for a member
// without a test); the others get t0 = NaN, n_adj = 0 and do not enter the maximum.  Column c >= 1 is family-valid on a plane when
// every member included there is valid at c (design_coef's verdict: every listed group finite in EVERY plane), so the maximum
// runs over the same members in every column, j ascending.  One workgroup per family, in three steps:
//   1  threads over members: coef_j[0] through design_coef (the arithmetic of the records), t0 and the effective scale; the first
//      stage_cap members keep (coef0, scale) in LDS, every member keeps (t0, coef0) in its adj cells, which the members beyond
//      stage_cap are read back from: the same doubles, so the outputs do not depend on stage_cap;
//   2  threads over columns: the maximum row, stored (column 0 and the invalid columns NaN), and n_valid_family;
//   3  waves over blocks of FM_BLOCK members, lanes over columns: the counts from the stored row, FM_BLOCK comparisons per
//      element read, summed by ballots -- no reduction across waves; the count replaces coef0 in the adj cell.
#define FM_BLOCK 8
#define FM_MAX_STAGED 1024      // 32 KB of LDS at two planes: four workgroups a CU (a choice, not a measurement)

// y[k]: plane k; sm: LDS [2][NP][stage_cap] (coef0, then scale); maxrow [NP][ld], adj [m][NP][2] and fam [NP][2] of THIS family
template <int NP>
__device__ __forceinline__ void family_maxt(const double *const (&y)[NP], int64_t ld, int32_t num_boot, int32_t n_groups, int row, int t0,
                                            int m, const int32_t *__restrict__ test_design, const int32_t *__restrict__ design_ptr,
                                            const int32_t *__restrict__ design_grp, const double *__restrict__ design_w,
                                            const double *__restrict__ scale, int32_t stage_cap, double *__restrict__ maxrow,
                                            double *__restrict__ adj, double *__restrict__ fam, double *sm, double *red) {
  double *c0s = sm, *scs = sm + NP * (int64_t)stage_cap;
  const int64_t row_base = (int64_t)row * n_groups;
  // step 1
  double ninc[NP];
  for (int k = 0; k < NP; k++) ninc[k] = 0.0;
  for (int j = threadIdx.x; j < m; j += K9_THREADS) {
    int d = test_design[t0 + j];
    int p0 = design_ptr[d], p1 = design_ptr[d + 1];
    double v[NP];
    bool good = design_coef<NP>(y, ld, row_base, design_grp, design_w, p0, p1, 0, v) && p1 > p0;
    for (int k = 0; k < NP; k++) {
      double s = scale[(int64_t)(t0 + j) * NP + k];
      bool inc = good && isfinite(v[k]) && isfinite(s) && s > 0.0;
      double se = inc ? s : 0.0;
      adj[((int64_t)j * NP + k) * 2] = inc ? fabs(v[k]) * se : NAN;
      adj[((int64_t)j * NP + k) * 2 + 1] = v[k];
      if (j < stage_cap) { c0s[k * stage_cap + j] = v[k]; scs[k * stage_cap + j] = se; }
      if (inc) ninc[k] += 1.0;
    }
  }
  __threadfence_block();
  for (int k = 0; k < NP; k++) ninc[k] = wg_sum(ninc[k], red);      // (its barriers also publish the LDS and the adj cells)
  // step 2
  double nval[NP];
  for (int k = 0; k < NP; k++) nval[k] = 0.0;
  for (int c = threadIdx.x; c <= num_boot; c += K9_THREADS) {
    double mx[NP];
    bool ok[NP];
    for (int k = 0; k < NP; k++) { mx[k] = -INFINITY; ok[k] = c > 0 && ninc[k] > 0.0; }
    for (int j = 0; j < m && c > 0; j++) {
      double c0[NP], sc[NP];
      bool any = false;
      for (int k = 0; k < NP; k++) {
        if (j < stage_cap) { c0[k] = c0s[k * stage_cap + j]; sc[k] = scs[k * stage_cap + j]; }
        else {
          const double *a = adj + ((int64_t)j * NP + k) * 2;
          c0[k] = a[1];
          sc[k] = a[0] == a[0] ? scale[(int64_t)(t0 + j) * NP + k] : 0.0;
        }
        any = any || sc[k] > 0.0;
      }
      if (!any) continue;
      int d = test_design[t0 + j];
      double v[NP];
      bool good = design_coef<NP>(y, ld, row_base, design_grp, design_w, design_ptr[d], design_ptr[d + 1], c, v);
      for (int k = 0; k < NP; k++) {
        if (sc[k] > 0.0) {
          ok[k] = ok[k] && good;
          mx[k] = fmax(mx[k], fabs(v[k] - c0[k]) * sc[k]);
        }
      }
    }
    for (int k = 0; k < NP; k++) {
      maxrow[k * ld + c] = ok[k] ? mx[k] : NAN;
      if (ok[k]) nval[k] += 1.0;
    }
  }
  __threadfence_block();
  for (int k = 0; k < NP; k++) nval[k] = wg_sum(nval[k], red);      // (its barriers also publish the row)
  if (threadIdx.x == 0)
    for (int k = 0; k < NP; k++) { fam[k * 2] = nval[k]; fam[k * 2 + 1] = ninc[k]; }
  // step 3
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j0 = wave * FM_BLOCK; j0 < m; j0 += FM_BLOCK * (K9_THREADS / 64)) {
    for (int k = 0; k < NP; k++) {
      double t[FM_BLOCK];
      uint32_t cnt[FM_BLOCK];
#pragma unroll
      for (int i = 0; i < FM_BLOCK; i++) {
        t[i] = j0 + i < m ? adj[((int64_t)(j0 + i) * NP + k) * 2] : NAN;
        cnt[i] = 0;
      }
      const double *r = maxrow + k * ld;
      for (int cb = 1; cb <= num_boot; cb += 64) {
        int c = cb + lane;
        double x = c <= num_boot ? r[c] : NAN;
#pragma unroll
        for (int i = 0; i < FM_BLOCK; i++) cnt[i] += (uint32_t)__popcll(__ballot(x > t[i]));      // (NaN on either side: not counted)
      }
      if (lane == 0) {
#pragma unroll
        for (int i = 0; i < FM_BLOCK; i++)
          if (j0 + i < m) adj[((int64_t)(j0 + i) * NP + k) * 2 + 1] = (double)cnt[i];
      }
    }
  }
}

__global__ __launch_bounds__(K9_THREADS) void k_family_maxt(const double *__restrict__ ym, const double *__restrict__ yv, int64_t ld,
                                                            int32_t num_boot, int32_t n_groups, const int32_t *__restrict__ family_ptr,
                                                            const int32_t *__restrict__ test_row, const int32_t *__restrict__ test_design,
                                                            const int32_t *__restrict__ design_ptr, const int32_t *__restrict__ design_grp,
                                                            const double *__restrict__ design_w, const double *__restrict__ scale,
                                                            int32_t stage_cap, double *__restrict__ maxrow, double *__restrict__ adj,
                                                            double *__restrict__ fam) {
  extern __shared__ double sm[];
  __shared__ double red[K9_THREADS / 64];
  int64_t f = blockIdx.x;
  int t0 = family_ptr[f], m = family_ptr[f + 1] - t0;
  const double *const y[2] = {ym, yv};
  // (an empty family has no test to take its row block from: row 0 is never read, m == 0 leaves the NaN row and the zero counts)
  family_maxt<2>(y, ld, num_boot, n_groups, m > 0 ? test_row[t0] : 0, t0, m, test_design, design_ptr, design_grp, design_w, scale, stage_cap,
                 maxrow + f * 2 * ld, adj + (int64_t)t0 * 4, fam + f * 4, sm, red);
}

// The one-plane entry (ht_2d_posthoc: the replicate correlations of Bootstrap2D): scale [test][1], maxrow [family][ld],
// adj [test][1][2], fam [family][1][2]; a column is valid for a member when every listed group is finite in this plane.
__global__ __launch_bounds__(K9_THREADS) void k_family_maxt1(const double *__restrict__ y, int64_t ld, int32_t num_boot, int32_t n_groups,
                                                             const int32_t *__restrict__ family_ptr, const int32_t *__restrict__ test_row,
                                                             const int32_t *__restrict__ test_design,
                                                             const int32_t *__restrict__ design_ptr, const int32_t *__restrict__ design_grp,
                                                             const double *__restrict__ design_w, const double *__restrict__ scale,
                                                             int32_t stage_cap, double *__restrict__ maxrow, double *__restrict__ adj,
                                                             double *__restrict__ fam) {
  extern __shared__ double sm[];
  __shared__ double red[K9_THREADS / 64];
  int64_t f = blockIdx.x;
  int t0 = family_ptr[f], m = family_ptr[f + 1] - t0;
  const double *const yp[1] = {y};
  family_maxt<1>(yp, ld, num_boot, n_groups, m > 0 ? test_row[t0] : 0, t0, m, test_design, design_ptr, design_grp, design_w, scale, stage_cap,
                 maxrow + f * ld, adj + (int64_t)t0 * 2, fam + f * 2, sm, red);
}

// ------------------------------------------------------------------------------------------------
// Single-step max-T over the resampled tests of a GENE (ht_1d_eqtl(adjust=True)): family_maxt's rule on the resampled row, whose
// slots 0..nb - 1 are what fill_records sees in k_cross_resampled_block (slot 0 observed, 1..nb - 1 the replicates).  The draws of
// slot c are keyed by the gene, so slot c of all its tests is one joint draw.  With coef0_j = stats[j][0] (the block kernel's
// record: coef_at(0) bit for bit) and scale_j from the host (1 / se, 0 for no test), member j is INCLUDED when scale_j is finite and
// > 0 and coef0_j is finite; slot c >= 1 is family-valid when no included member is NaN there (the degenerate-column rule, member by
// member), and there  M[c] = max_j |coef_j[c] - coef0_j| * scale_j  over the included members, j ascending.
//
// k_cross_family_max: one workgroup per (gene, slab of ``slab`` slots).  A thread owns a slot and walks the gene's tiles of XB_TT
// tests: every tile is staged as in the block kernel, with (coef0, effective scale) beside it, and evaluated by CrossTile::coef_at
// ONCE per (test, slot); the running maximum and the verdict stay in registers.  A tile without an included member is skipped (the
// partial last tile's unused slots have scale 0: never members).  Writes maxrow[gene][c] for c <= num_boot: NaN at slot 0, at
// invalid slots and at nb..num_boot, and everywhere for a gene without tests, without a good group, with nb < 1 or without an
// included member.  Nothing depends on ``slab``.  LDS: 76 bytes per group + 128.
// XF_SLAB = one round of the workgroup: at 3000 replicates a gene is 12 workgroups, so that a chunk of 263 genes fills the 256 CUs
// several times over where one workgroup per gene would leave one each (a choice, not a measurement).
#define XF_SLAB K9_THREADS
__global__ __launch_bounds__(K9_THREADS) void k_cross_family_max(
    const double *__restrict__ yt, int64_t ld, int32_t num_boot, int32_t n_groups, int32_t slabs, int32_t slab,
    const int32_t *__restrict__ gene_ptr, const double *__restrict__ tt, const uint8_t *__restrict__ good, const double *__restrict__ Nc,
    const int16_t *__restrict__ rep, const int32_t *__restrict__ bcol, const int32_t *__restrict__ col_map,
    const int32_t *__restrict__ n_valid, const int64_t *__restrict__ gene_key, uint64_t seed, const double *__restrict__ stats,
    const double *__restrict__ scale, double *__restrict__ maxrow) {
  extern __shared__ double sm[];
  double *tts = sm;                                        // [ng][XB_TT], test-minor
  double *ncs = sm + (size_t)XB_TT * n_groups;             // [ng]
  double *c0s = ncs + n_groups, *scs = c0s + XB_TT;        // [XB_TT] coef0 and the effective scale (0: not a member) of the tile
  int32_t *glist = (int32_t *)(scs + XB_TT);               // [ng] indices of good groups
  __shared__ int n_good_s;
  const int gene = (int)(blockIdx.x / (unsigned)slabs);
  const int64_t c_lo = (int64_t)(blockIdx.x % (unsigned)slabs) * slab;
  const int64_t c_hi = c_lo + slab < (int64_t)num_boot + 1 ? c_lo + slab : (int64_t)num_boot + 1;
  const int64_t t_lo = gene_ptr[gene], t_hi = gene_ptr[gene + 1];
  const uint8_t *gd = good + (int64_t)gene * n_groups;
  if (threadIdx.x == 0) {
    int ng = 0;
    for (int j = 0; j < n_groups; j++)
      if (gd[j]) glist[ng++] = j;
    n_good_s = ng;
  }
  for (int j = threadIdx.x; j < n_groups; j += K9_THREADS) ncs[j] = Nc[j];
  __syncthreads();
  const int n = n_good_s;
  const int nb = n_valid ? n_valid[gene] - 1 : num_boot;
  const bool live = t_hi > t_lo && n > 0 && nb >= 1;
  const int64_t row_base = (int64_t)gene * n_groups;
  const int16_t *rg = rep ? rep + (int64_t)gene * n_groups * num_boot : nullptr;
  const int32_t *bg = bcol ? bcol + (int64_t)gene * n_groups * num_boot : nullptr;
  const int32_t *cm = col_map ? col_map + (int64_t)gene * (num_boot + 1) : nullptr;
  const uint64_t gk = gene_key ? (uint64_t)gene_key[gene] : (uint64_t)gene;
  const CrossTile tile{yt, ld, num_boot, tts, ncs, glist, n, nb, row_base, rg, bg, cm, gk, seed};
  double *out = maxrow + (int64_t)gene * ld;
  for (int64_t cb = c_lo; cb < c_hi; cb += K9_THREADS) {      // (uniform) K9_THREADS slots of the slab at a time
    const int64_t c = cb + threadIdx.x;
    const bool act = live && c < c_hi && c >= 1 && c < nb;   // a slot with replicates: the only ones coef_at is asked for
    const bool walk = live && cb < nb && cb + K9_THREADS > 1;   // (uniform) some slot of this round is one
    double mx = -INFINITY;
    bool ok = act, any = false;
    for (int64_t t0 = t_lo; walk && t0 < t_hi; t0 += XB_TT) {
      const int nt = (int)(t_hi - t0 < XB_TT ? t_hi - t0 : XB_TT);
      __syncthreads();                                       // the previous tile has been read
      for (int j = threadIdx.x; j < n_groups; j += K9_THREADS)
        for (int k = 0; k < XB_TT; k++) tts[(size_t)j * XB_TT + k] = k < nt ? tt[(t0 + k) * n_groups + j] : 0.0;
      if (threadIdx.x < XB_TT) {
        const int k = threadIdx.x;
        double c0 = k < nt ? stats[(t0 + k) * 8] : NAN, sc = k < nt ? scale[t0 + k] : 0.0;
        c0s[k] = c0;
        scs[k] = (isfinite(sc) && sc > 0.0 && isfinite(c0)) ? sc : 0.0;
      }
      __syncthreads();
      bool tile_any = false;
      for (int k = 0; k < XB_TT; k++) tile_any = tile_any || scs[k] > 0.0;
      if (!tile_any) continue;                               // (uniform: read from LDS)
      any = true;
      if (act) {
        double v[XB_TT];
        tile.coef_at((int)c, v);
        for (int k = 0; k < XB_TT; k++) {
          if (scs[k] > 0.0) {
            ok = ok && v[k] == v[k];
            mx = fmax(mx, fabs(v[k] - c0s[k]) * scs[k]);
          }
        }
      }
    }
    if (c < c_hi) out[c] = (ok && any) ? mx : NAN;
  }
}

// k_cross_family_count: one workgroup per gene, after k_cross_family_max.  adj[t] = (t0, n_adj) with t0_j = |coef0_j| * scale_j (NaN
// where the member is not included) and n_adj_j = #{c : M[c] > t0_j} (NaN on either side is not counted); fam[gene] =
// (n_valid_family = the non-NaN slots of the row, n_included).  The counts as in step 3 of family_maxt: waves over blocks of
// FM_BLOCK members, lanes over slots, ballots, no reduction across waves.
__global__ __launch_bounds__(K9_THREADS) void k_cross_family_count(int64_t ld, int32_t num_boot, int32_t n_groups,
                                                                   const int32_t *__restrict__ gene_ptr, const uint8_t *__restrict__ good,
                                                                   const int32_t *__restrict__ n_valid, const double *__restrict__ stats,
                                                                   const double *__restrict__ scale, const double *__restrict__ maxrow,
                                                                   double *__restrict__ adj, double *__restrict__ fam) {
  __shared__ double red[K9_THREADS / 64];
  const int gene = blockIdx.x;
  const int64_t t_lo = gene_ptr[gene];
  const int m = (int)(gene_ptr[gene + 1] - t_lo);
  const int nb = n_valid ? n_valid[gene] - 1 : num_boot;
  double n_good = 0.0;
  for (int j = threadIdx.x; j < n_groups; j += K9_THREADS) n_good += good[(int64_t)gene * n_groups + j] ? 1.0 : 0.0;
  n_good = wg_sum(n_good, red);
  const bool live = m > 0 && n_good > 0.0 && nb >= 1;
  double ninc = 0.0;
  for (int j = threadIdx.x; j < m; j += K9_THREADS) {
    double c0 = stats[(t_lo + j) * 8], sc = scale[t_lo + j];
    bool inc = live && isfinite(sc) && sc > 0.0 && isfinite(c0);
    adj[(t_lo + j) * 2] = inc ? fabs(c0) * sc : NAN;
    if (inc) ninc += 1.0;
  }
  __threadfence_block();
  ninc = wg_sum(ninc, red);                                  // (its barriers also publish the adj cells)
  const double *r = maxrow + (int64_t)gene * ld;
  double nval = 0.0;
  for (int c = 1 + threadIdx.x; c <= num_boot; c += K9_THREADS) {
    double x = r[c];
    if (x == x) nval += 1.0;
  }
  nval = wg_sum(nval, red);
  if (threadIdx.x == 0) { fam[(int64_t)gene * 2] = nval; fam[(int64_t)gene * 2 + 1] = ninc; }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j0 = wave * FM_BLOCK; j0 < m; j0 += FM_BLOCK * (K9_THREADS / 64)) {
    double t[FM_BLOCK];
    uint32_t cnt[FM_BLOCK];
#pragma unroll
    for (int i = 0; i < FM_BLOCK; i++) {
      t[i] = j0 + i < m ? adj[(t_lo + j0 + i) * 2] : NAN;
      cnt[i] = 0;
    }
    for (int cb = 1; cb <= num_boot; cb += 64) {
      int c = cb + lane;
      double x = c <= num_boot ? r[c] : NAN;
#pragma unroll
      for (int i = 0; i < FM_BLOCK; i++) cnt[i] += (uint32_t)__popcll(__ballot(x > t[i]));      // (NaN on either side: not counted)
    }
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < FM_BLOCK; i++)
        if (j0 + i < m) adj[(t_lo + j0 + i) * 2 + 1] = (double)cnt[i];
    }
  }
}

// ------------------------------------------------------------------------------------------------
// Joint test of a block of treatment columns (ht_1d_joint): test t applies the r linear forms of design d = test_design[t] --
// L [r][n_d] row-major at design_L + design_lofs[d], over the n_d groups design_grp[design_ptr[d] .. design_ptr[d + 1]) -- to
// every replicate column of gene test_gene[t] and reduces the quadratic statistic
//   Q_0 = ||L y_0||^2,   Q*_c = ||L y_c - L y_0||^2  (c >= 1: the centred bootstrap null),
// on the mean and the variability plane at once.  THE JOINT RECORD, 8 doubles per test and plane:
//   [0] Q_0   [1] population sd of Q* over the valid columns 1..B   [2] n_valid   [3] n_extreme = #{ Q*_c > Q_0 }
//   [4] mean of Q*   [5] all_equal: 1 when every valid Q*_c is exactly 0   [6] max of Q*   [7] r
// Column c is valid only if every listed group is finite there in BOTH planes (hypothesis_test.py:249-251); an invalid
// column 0, an empty design and r = 0 give the NaN record on both planes.  z_0 = L y_0 is formed first and kept in LDS.  A form
// sums p ascending, Q sums k ascending, and column 0 goes through the same routine as the others: a replicate column equal to
// column 0 has Q* == 0 exactly.  L is staged in LDS when r * n_d <= JOINT_LDS_DOUBLES (32 KB: a choice that leaves four
// workgroups per CU, not a measurement) and comes through the cache otherwise; both paths do the same arithmetic in the same
// order.  Two passes that recompute Q* (count / sum / max, then squared deviations and the extreme count): nothing
// per-replicate is stored.  Up to JOINT_REG_GROUPS groups a thread keeps its column's operands in registers (one read of the
// planes per pass; instantiated for JOINT_REG_SMALL and for JOINT_REG_GROUPS); beyond, the rows are read again for every form and come back
// from L1 / L2.  The routines take the number of planes NP as a template parameter: k_joint_stats is NP = 2, k_joint1_stats (the
// correlation plane of ht_2d_joint) NP = 1.
#define JOINT_LDS_DOUBLES 4096
#define JOINT_REG_GROUPS 32
#define JOINT_REG_SMALL 8      // the narrower tier: 86 VGPRs against 184, 2.5x the wider one's speed on designs it holds (profiles/joint_stats.txt, profiles/joint1_stats.txt)

// The NP response planes of a test (NP = 2: ym, yv of Bootstrap1D; NP = 1: the correlation rows of Bootstrap2D, mm_joint1_stats)
template <int NP>
struct joint_design {
  const double *y[NP];        // the planes, offset to the test's first row
  const int32_t *grp;         // [nd]
  int64_t ld;
  int nd, r;
};

// form k of column c on every plane: each L element and each operand offset is read once
template <int NP, class LP>
__device__ __forceinline__ void joint_form(const joint_design<NP> &D, LP Lk, int c, double (&a)[NP]) {
#pragma unroll
  for (int j = 0; j < NP; j++) a[j] = 0.0;
  for (int p = 0; p < D.nd; p++) {
    int64_t o = (int64_t)D.grp[p] * D.ld + c;
    double l = Lk[p];
#pragma unroll
    for (int j = 0; j < NP; j++) a[j] += l * D.y[j][o];
  }
}

template <int NP>
__device__ __forceinline__ bool joint_valid(const joint_design<NP> &D, int c) {
  bool ok = true;
  for (int p = 0; p < D.nd; p++) {
    int64_t o = (int64_t)D.grp[p] * D.ld + c;
#pragma unroll
    for (int j = 0; j < NP; j++) ok = ok && isfinite(D.y[j][o]);
  }
  return ok;
}

// Q* of column c on every plane into q; returns whether the column is valid.  NDR == 0: any n_d, the operands are read again for
// every form and come back from L1 / L2.  NDR > 0 (n_d <= NDR): the column's operands are read ONCE into registers, which also
// decides its validity, and the forms run on registers and the LDS copy of L.  The arithmetic and its order are those of
// joint_form either way.  LP: ``const double *`` into LDS (staged) or into global memory; z0 [NP][zs] in LDS, r <= zs.
template <int NDR, int NP, class LP>
__device__ __forceinline__ bool joint_q(const joint_design<NP> &D, LP L, const double *z0, int zs, int c, double (&q)[NP]) {
#pragma unroll
  for (int j = 0; j < NP; j++) q[j] = 0.0;
  if constexpr (NDR == 0) {
    if (!joint_valid(D, c)) return false;
    for (int k = 0; k < D.r; k++) {
      double a[NP];
      joint_form(D, L + (int64_t)k * D.nd, c, a);
#pragma unroll
      for (int j = 0; j < NP; j++) {
        double d = a[j] - z0[j * zs + k];
        q[j] += d * d;
      }
    }
  } else {
    double a[NP][NDR];
    bool ok = true;
#pragma unroll
    for (int p = 0; p < NDR; p++) {
#pragma unroll
      for (int j = 0; j < NP; j++) a[j][p] = 0.0;
      if (p < D.nd) {
        int64_t o = (int64_t)D.grp[p] * D.ld + c;
#pragma unroll
        for (int j = 0; j < NP; j++) a[j][p] = D.y[j][o];      // every plane's load is issued before the first value is looked at
#pragma unroll
        for (int j = 0; j < NP; j++) ok = ok && isfinite(a[j][p]);
      }
    }
    if (!ok) return false;
    for (int k = 0; k < D.r; k++) {
      LP Lk = L + (int64_t)k * D.nd;
      double s[NP];
#pragma unroll
      for (int j = 0; j < NP; j++) s[j] = 0.0;
#pragma unroll
      for (int p = 0; p < NDR; p++) {
        if (p < D.nd) {
          double l = Lk[p];
#pragma unroll
          for (int j = 0; j < NP; j++) s[j] += l * a[j][p];
        }
      }
#pragma unroll
      for (int j = 0; j < NP; j++) {
        double d = s[j] - z0[j * zs + k];
        q[j] += d * d;
      }
    }
  }
  return true;
}

// Called by all threads of the workgroup.  z0: LDS scratch [NP][zs]; st[j]: the record of plane j.
template <int NDR, int NP, class LP>
__device__ __forceinline__ void joint_records(const joint_design<NP> &D, LP L, double *z0, int zs, int num_boot, double *const (&st)[NP],
                                              double *red) {
  for (int k = threadIdx.x; k < D.r; k += K9_THREADS) {
    double a[NP];
    joint_form(D, L + (int64_t)k * D.nd, 0, a);
#pragma unroll
    for (int j = 0; j < NP; j++) z0[j * zs + k] = a[j];
  }
  __syncthreads();
  double q0[NP], q[NP], sum[NP], hi[NP], cnt = 0.0;
#pragma unroll
  for (int j = 0; j < NP; j++) { q0[j] = 0.0; sum[j] = 0.0; hi[j] = -INFINITY; }
  for (int k = 0; k < D.r; k++) {
#pragma unroll
    for (int j = 0; j < NP; j++) q0[j] += z0[j * zs + k] * z0[j * zs + k];
  }
  for (int c = 1 + threadIdx.x; c <= num_boot; c += K9_THREADS) {
    if (!joint_q<NDR>(D, L, z0, zs, c, q)) continue;
#pragma unroll
    for (int j = 0; j < NP; j++) { sum[j] += q[j]; hi[j] = fmax(hi[j], q[j]); }
    cnt += 1.0;
  }
  double n = wg_sum(cnt, red), mean[NP], sq[NP], ext[NP];
#pragma unroll
  for (int j = 0; j < NP; j++) {
    sum[j] = wg_sum(sum[j], red);
    hi[j] = wg_max(hi[j], red);
    mean[j] = n > 0 ? sum[j] / n : NAN;
    sq[j] = 0.0;
    ext[j] = 0.0;
  }
  for (int c = 1 + threadIdx.x; c <= num_boot; c += K9_THREADS) {
    if (!joint_q<NDR>(D, L, z0, zs, c, q)) continue;
#pragma unroll
    for (int j = 0; j < NP; j++) {
      double d = q[j] - mean[j];
      sq[j] += d * d;
      if (q[j] > q0[j]) ext[j] += 1.0;
    }
  }
#pragma unroll
  for (int j = 0; j < NP; j++) { sq[j] = wg_sum(sq[j], red); ext[j] = wg_sum(ext[j], red); }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < NP; j++) {
      double *s = st[j];
      s[0] = q0[j];
      s[1] = n > 0 ? sqrt(sq[j] / n) : NAN;
      s[2] = n;
      s[3] = ext[j];
      s[4] = mean[j];
      s[5] = (n > 0 && hi[j] == 0.0) ? 1.0 : 0.0;
      s[6] = n > 0 ? hi[j] : NAN;
      s[7] = (double)D.r;
    }
  }
}

// One workgroup = one test, on NP planes: the designs, the NaN records, the staging of L and the column-0 check that the
// two kernels below share.  y[j]: plane j; st[j]: record j of this test; sm: LDS [NP * n_groups + stage_cap].
template <int NDR, int NP>
__device__ __forceinline__ void joint_test(const double *const (&y)[NP], int64_t ld, int32_t num_boot, int32_t n_groups, int32_t stage_cap,
                                           int row, int d, const int32_t *__restrict__ design_ptr, const int32_t *__restrict__ design_rank,
                                           const int64_t *__restrict__ design_lofs, const int32_t *__restrict__ design_grp,
                                           const double *__restrict__ design_L, double *const (&st)[NP], double *sm, double *red) {
  double *z0 = sm, *Ls = sm + NP * (int64_t)n_groups;      // [NP][n_groups], [stage_cap]
  int p0 = design_ptr[d], p1 = design_ptr[d + 1];
  joint_design<NP> D;
  D.nd = p1 - p0;
  D.r = design_rank[d];
  if (D.nd <= 0 || D.r <= 0 || D.r > n_groups || (NDR > 0 && D.nd > NDR)) {
#pragma unroll
    for (int j = 0; j < NP; j++) write_nan_record(st[j]);
    return;
  }
  D.ld = ld;
  D.grp = design_grp + p0;
#pragma unroll
  for (int j = 0; j < NP; j++) D.y[j] = y[j] + (int64_t)row * n_groups * ld;
  const double *Lg = design_L + design_lofs[d];
  const int n_l = D.r * D.nd;                       // <= n_groups^2 < 2^31 (checked by the caller)
  const bool staged = n_l <= stage_cap;
  if (staged)
    for (int i = threadIdx.x; i < n_l; i += K9_THREADS) Ls[i] = Lg[i];
  double ok0 = 1.0;                                 // column 0: every listed group finite in every plane?
  for (int p = threadIdx.x; p < D.nd; p += K9_THREADS) {
    int64_t o = (int64_t)D.grp[p] * ld;
#pragma unroll
    for (int j = 0; j < NP; j++)
      if (!isfinite(D.y[j][o])) ok0 = 0.0;
  }
  ok0 = wg_min(ok0, red);                           // (its barriers also publish Ls)
  if (ok0 == 0.0) {
#pragma unroll
    for (int j = 0; j < NP; j++) write_nan_record(st[j]);
    return;
  }
  if (staged) joint_records<NDR>(D, (const double *)Ls, z0, n_groups, num_boot, st, red);
  else joint_records<NDR>(D, Lg, z0, n_groups, num_boot, st, red);
}

// NDR: 0, or a bound on n_groups (and so on every n_d) that lets a column's operands live in registers (joint_q)
template <int NDR>
__global__ __launch_bounds__(K9_THREADS) void k_joint_stats(const double *__restrict__ ym, const double *__restrict__ yv, int64_t ld,
                                                            int32_t num_boot, int32_t n_groups, int32_t stage_cap,
                                                            const int32_t *__restrict__ test_gene, const int32_t *__restrict__ test_design,
                                                            const int32_t *__restrict__ design_ptr, const int32_t *__restrict__ design_rank,
                                                            const int64_t *__restrict__ design_lofs, const int32_t *__restrict__ design_grp,
                                                            const double *__restrict__ design_L, double *__restrict__ stats_m,
                                                            double *__restrict__ stats_v) {
  extern __shared__ double sm[];
  __shared__ double red[K9_THREADS / 64];
  int64_t t = blockIdx.x;
  const double *const y[2] = {ym, yv};
  double *const st[2] = {stats_m + t * 8, stats_v + t * 8};
  joint_test<NDR, 2>(y, ld, num_boot, n_groups, stage_cap, test_gene[t], test_design[t], design_ptr, design_rank, design_lofs, design_grp,
                     design_L, st, sm, red);
}

// The joint test on ONE response plane (the replicate correlations of Bootstrap2D, ht_2d_joint): test t applies the forms of
// design test_design[t] to the rows of pair test_row[t] and writes one joint record.  The routines, the arithmetic and its
// order are those of k_joint_stats, instantiated for one plane: the record is, bit for bit, the mean-plane record of
// k_joint_stats given the plane twice, but every operand is read once, every form evaluated once and -- in the register tiers --
// one operand array is held, not two (profiles/joint1_stats.txt).
template <int NDR>
__global__ __launch_bounds__(K9_THREADS) void k_joint1_stats(const double *__restrict__ y, int64_t ld, int32_t num_boot, int32_t n_groups,
                                                             int32_t stage_cap, const int32_t *__restrict__ test_row,
                                                             const int32_t *__restrict__ test_design, const int32_t *__restrict__ design_ptr,
                                                             const int32_t *__restrict__ design_rank, const int64_t *__restrict__ design_lofs,
                                                             const int32_t *__restrict__ design_grp, const double *__restrict__ design_L,
                                                             double *__restrict__ stats) {
  extern __shared__ double sm[];
  __shared__ double red[K9_THREADS / 64];
  int64_t t = blockIdx.x;
  const double *const yp[1] = {y};
  double *const st[1] = {stats + t * 8};
  joint_test<NDR, 1>(yp, ld, num_boot, n_groups, stage_cap, test_row[t], test_design[t], design_ptr, design_rank, design_lofs, design_grp,
                     design_L, st, sm, red);
}

// ------------------------------------------------------------------------------------------------
// Order statistics of a replicate row (percentile intervals of the coefficients): np.nanquantile(row[1 : B + 1], probs),
// method 'linear', for up to RQ_MAX_PROBS probabilities per launch.  One workgroup per row.  Every double maps to a uint64 key
// of the same order (negatives: all bits flipped; others: sign bit flipped) and the two order statistics of every probability
// are found by an MSB-first radix select, 8 bits per pass: a pass builds one 256-bin LDS histogram per distinct key prefix
// among the wanted ranks (ranks inside one run of equal keys share their prefix, and so their histogram, to the end) over the
// keys that carry that prefix; a scan of the histogram gives the rank's next digit and its rank among the keys that share it.
// The first pass has the empty prefix, so its histogram also counts the non-NaN columns.  The row is read from global memory
// in every pass (8 reads of a row that stays in L2), so nothing depends on the row length: no LDS-resident variant.
#define RQ_THREADS 256
#define RQ_MAX_PROBS 8
#define RQ_MAX_RANKS (2 * RQ_MAX_PROBS)
struct rq_probs { double p[RQ_MAX_PROBS]; };

__device__ __forceinline__ uint64_t rq_key(double x) {
  uint64_t b = (uint64_t)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double rq_value(uint64_t k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}

__global__ __launch_bounds__(RQ_THREADS) void k_row_quantiles(const double *__restrict__ rows, int64_t ld, int32_t num_boot, rq_probs probs,
                                                              int32_t n_probs, double *__restrict__ out, int32_t *__restrict__ n_valid) {
  __shared__ uint32_t hist[RQ_MAX_RANKS][256];
  __shared__ uint64_t pre[RQ_MAX_RANKS];      // per wanted rank: the key digits found so far
  __shared__ uint32_t rnk[RQ_MAX_RANKS];      //                  its rank among the keys that share them
  __shared__ int slot[RQ_MAX_RANKS];          //                  the histogram of its prefix
  __shared__ uint64_t gpre[RQ_MAX_RANKS];     // per histogram: the prefix it counts
  __shared__ int n_hist_s;
  __shared__ uint32_t wave_n[RQ_THREADS / 64];
  const int tid = threadIdx.x;
  const int n_ranks = 2 * n_probs;
  const double *x = rows + (int64_t)blockIdx.x * ld + 1;     // replicate columns 1..num_boot
  int n_hist = 1;
  uint32_t n = 0;
  for (int pass = 0; pass < 8; pass++) {
    const int shift = 56 - 8 * pass;
    for (int i = tid; i < n_hist * 256; i += RQ_THREADS) (&hist[0][0])[i] = 0;
    __syncthreads();
    for (int c = tid; c < num_boot; c += RQ_THREADS) {
      double v = x[c];
      if (v != v) continue;
      uint64_t k = rq_key(v);
      uint32_t digit = (uint32_t)(k >> shift) & 255u;
      if (pass == 0) {
        atomicAdd(&hist[0][digit], 1u);
      } else {
        uint64_t hi = k >> (shift + 8);
        for (int g = 0; g < n_hist; g++)
          if (gpre[g] == hi) {      // the prefixes are distinct: at most one histogram takes the key
            atomicAdd(&hist[g][digit], 1u);
            break;
          }
      }
    }
    __syncthreads();
    if (pass == 0) {
      uint32_t cnt = hist[0][tid];
      for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
      if ((tid & 63) == 0) wave_n[tid >> 6] = cnt;
      __syncthreads();
      n = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
      if (n == 0) {
        if (tid < n_probs) out[(int64_t)blockIdx.x * n_probs + tid] = NAN;
        if (tid == 0) n_valid[blockIdx.x] = 0;
        return;
      }
      if (tid < n_ranks) {
        double h = (double)(n - 1) * probs.p[tid >> 1];
        uint32_t lo = (uint32_t)floor(h);
        lo = lo < n - 1 ? lo : n - 1;
        uint32_t hi = lo + 1 < n - 1 ? lo + 1 : n - 1;
        rnk[tid] = (tid & 1) ? hi : lo;
        pre[tid] = 0;
        slot[tid] = 0;
      }
      __syncthreads();
    }
    if (tid < n_ranks) {
      const uint32_t *hg = hist[slot[tid]];
      uint32_t r = rnk[tid], cum = 0, digit = 255;
      for (uint32_t d = 0; d < 256; d++) {
        uint32_t cnt = hg[d];
        if (r < cum + cnt) { digit = d; break; }
        cum += cnt;
      }
      rnk[tid] = r - cum;
      pre[tid] = (pre[tid] << 8) | digit;
    }
    __syncthreads();
    if (tid == 0) {      // one histogram per distinct prefix for the next pass
      int nh = 0;
      for (int j = 0; j < n_ranks; j++) {
        int g = 0;
        while (g < nh && gpre[g] != pre[j]) g++;
        if (g == nh) gpre[nh++] = pre[j];
        slot[j] = g;
      }
      n_hist_s = nh;
    }
    __syncthreads();
    n_hist = n_hist_s;
  }
  if (tid < n_probs) {
    // numpy's 'linear' method: virtual index h = (n - 1) p, weight t = h - floor(h), then _lerp(a, b, t).  t == 0 and a == b
    // return a itself, which is _lerp's value wherever that is finite and keeps +-inf where _lerp has inf - inf.
    double h = (double)(n - 1) * probs.p[tid];
    double t = h - floor(h);
    double a = rq_value(pre[2 * tid]), b = rq_value(pre[2 * tid + 1]);
    double d = b - a, q;
    if (t == 0.0 || a == b) q = a;
    else if (t < 0.5) q = a + d * t;
    else q = b - d * (1.0 - t);
    out[(int64_t)blockIdx.x * n_probs + tid] = q;
  }
  if (tid == 0) n_valid[blockIdx.x] = (int32_t)n;
}

extern "C" {

int mm_row_quantiles(const double *d_rows, int64_t n_rows, int64_t ld, int32_t num_boot, const double *probs, int32_t n_probs,
                     double *d_out, int32_t *d_n_valid, void *stream) {
  MM_ARG(n_rows >= 0 && n_rows < 2147483647LL && num_boot >= 1 && ld >= (int64_t)num_boot + 1);
  MM_ARG(probs && n_probs >= 1 && n_probs <= RQ_MAX_PROBS);
  rq_probs pr;
  for (int k = 0; k < RQ_MAX_PROBS; k++) pr.p[k] = k < n_probs ? probs[k] : 0.0;
  for (int k = 0; k < n_probs; k++) MM_ARG(pr.p[k] >= 0.0 && pr.p[k] <= 1.0);   // (NaN fails both comparisons)
  if (n_rows == 0) return MM_OK;
  MM_ARG(d_rows && d_out && d_n_valid);
  hipLaunchKernelGGL(k_row_quantiles, dim3((unsigned)n_rows), dim3(RQ_THREADS), 0, (hipStream_t)stream, d_rows, ld, num_boot, pr, n_probs,
                     d_out, d_n_valid);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_contract_stats(const double *d_ym, const double *d_yv, int64_t ld, int32_t num_boot, int32_t n_groups,
                      const int32_t *d_test_gene, const double *d_W, const uint8_t *d_good, int64_t n_tests, int32_t which,
                      double *d_coef, double *d_stats, void *stream) {
  MM_ARG(d_ym && d_yv && d_test_gene && d_W && d_good && d_coef && d_stats);
  MM_ARG(n_tests >= 0 && n_groups > 0 && num_boot > 0 && ld >= (int64_t)num_boot + 1 && (which == 0 || which == 1));
  if (n_tests == 0) return MM_OK;
  size_t shm = (size_t)n_groups * 12 + 8;
  hipLaunchKernelGGL(k_contract_stats, dim3((unsigned)n_tests), dim3(K9_THREADS), shm, (hipStream_t)stream, d_ym, d_yv, ld, num_boot,
                     n_groups, d_test_gene, d_W, d_good, which, d_coef, d_stats);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_valid_cols(const double *d_ym, const double *d_yv, int64_t ld, int32_t num_boot, int32_t n_groups, const uint8_t *d_good,
                  int64_t n_genes, int32_t *d_col_map, int32_t *d_n_valid, void *stream) {
  MM_ARG(d_ym && d_yv && d_good && d_col_map && d_n_valid && n_groups > 0 && num_boot >= 0 && ld >= (int64_t)num_boot + 1);
  MM_ARG(n_genes >= 0 && n_genes < 2147483647LL);
  if (n_genes == 0) return MM_OK;
  size_t shm = (size_t)n_groups * 4;
  hipLaunchKernelGGL(k_valid_cols, dim3((unsigned)n_genes), dim3(256), shm, (hipStream_t)stream, d_ym, d_yv, ld, num_boot, n_groups,
                     d_good, d_col_map, d_n_valid);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_residualize(const double *d_src, double *d_dst, int64_t ld, int32_t n_cols, int32_t n_groups, int64_t n_genes,
                   const int32_t *d_gene_mask, const double *d_M, void *stream) {
  MM_ARG(d_src && d_dst && d_src != d_dst && d_gene_mask && d_M && n_cols > 0 && n_groups > 0 && n_genes >= 0);
  MM_ARG((size_t)n_groups * 8 <= 64 * 1024);
  if (n_genes == 0) return MM_OK;
  int32_t col_tiles = (n_cols + 255) / 256;
  MM_ARG(n_genes * col_tiles < 2147483647LL);
  size_t shm = (size_t)n_groups * 8;
  hipLaunchKernelGGL(k_residualize, dim3((unsigned)(n_genes * col_tiles)), dim3(256), shm, (hipStream_t)stream, d_src, d_dst, ld, n_cols,
                     n_groups, col_tiles, d_gene_mask, d_M);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

static int cross_resampled_args(const double *d_yt, int64_t ld, int32_t num_boot, int32_t n_groups, const void *d_tests, const double *d_tt,
                                const uint8_t *d_good, const double *d_Nc, const int16_t *d_rep, const int32_t *d_bcol,
                                const int32_t *d_col_map, const int32_t *d_n_valid, int64_t n_tests, const double *d_stats) {
  MM_ARG(d_yt && d_tests && d_tt && d_good && d_Nc && d_stats);
  MM_ARG(n_tests >= 0 && n_tests < 2147483647LL && n_groups > 0 && n_groups <= 32767 && num_boot > 1 && ld >= (int64_t)num_boot + 1);
  MM_ARG(((d_rep == nullptr) == (d_bcol == nullptr)) && ((d_col_map == nullptr) == (d_n_valid == nullptr)));
  return MM_OK;
}

int mm_cross_resampled_keyed(const double *d_yt, int64_t ld, int32_t num_boot, int32_t n_groups, const int32_t *d_test_gene,
                             const double *d_tt, const uint8_t *d_good, const double *d_Nc, const int16_t *d_rep, const int32_t *d_bcol,
                             const int32_t *d_col_map, const int32_t *d_n_valid, const int64_t *d_gene_key, uint64_t seed,
                             int64_t n_tests, double *d_coef, double *d_stats, void *stream) {
  int rc = cross_resampled_args(d_yt, ld, num_boot, n_groups, d_test_gene, d_tt, d_good, d_Nc, d_rep, d_bcol, d_col_map, d_n_valid, n_tests,
                                d_stats);
  if (rc != MM_OK) return rc;
  MM_ARG(d_coef);
  if (n_tests == 0) return MM_OK;
  size_t shm = (size_t)n_groups * 20 + 8;
  hipLaunchKernelGGL(k_cross_resampled, dim3((unsigned)n_tests), dim3(K9_THREADS), shm, (hipStream_t)stream, d_yt, ld, num_boot, n_groups,
                     d_test_gene, d_tt, d_good, d_Nc, d_rep, d_bcol, d_col_map, d_n_valid, d_gene_key, seed, d_coef, d_stats);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_cross_resampled(const double *d_yt, int64_t ld, int32_t num_boot, int32_t n_groups, const int32_t *d_test_gene,
                       const double *d_tt, const uint8_t *d_good, const double *d_Nc, const int16_t *d_rep, const int32_t *d_bcol,
                       const int32_t *d_col_map, const int32_t *d_n_valid, uint64_t seed, int64_t n_tests, double *d_coef,
                       double *d_stats, void *stream) {
  return mm_cross_resampled_keyed(d_yt, ld, num_boot, n_groups, d_test_gene, d_tt, d_good, d_Nc, d_rep, d_bcol, d_col_map, d_n_valid,
                                  nullptr, seed, n_tests, d_coef, d_stats, stream);
}

int mm_cross_resampled_block(const double *d_yt, int64_t ld, int32_t num_boot, int32_t n_groups, const int32_t *d_gene_ptr,
                             int64_t n_genes, int32_t max_gene_tests, const double *d_tt, const uint8_t *d_good, const double *d_Nc,
                             const int16_t *d_rep, const int32_t *d_bcol, const int32_t *d_col_map, const int32_t *d_n_valid,
                             const int64_t *d_gene_key, uint64_t seed, int64_t n_tests, double *d_stats, void *stream) {
  int rc = cross_resampled_args(d_yt, ld, num_boot, n_groups, d_gene_ptr, d_tt, d_good, d_Nc, d_rep, d_bcol, d_col_map, d_n_valid, n_tests,
                                d_stats);
  if (rc != MM_OK) return rc;
  MM_ARG(n_genes >= 0 && max_gene_tests >= 0 && (int64_t)max_gene_tests <= n_tests);
  if (n_tests == 0 || n_genes == 0 || max_gene_tests == 0) return MM_OK;
  int32_t tiles = (max_gene_tests + XB_TT - 1) / XB_TT;
  MM_ARG(n_genes * tiles < 2147483647LL);
  size_t shm = (size_t)n_groups * (XB_TT * 8 + 12) + 8;
  MM_ARG(shm <= 64 * 1024);
  hipLaunchKernelGGL(k_cross_resampled_block, dim3((unsigned)(n_genes * tiles)), dim3(K9_THREADS), shm, (hipStream_t)stream, d_yt, ld,
                     num_boot, n_groups, tiles, d_gene_ptr, d_tt, d_good, d_Nc, d_rep, d_bcol, d_col_map, d_n_valid, d_gene_key, seed,
                     d_stats);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

// the tile range of the per-test-covariate entry points: [tile_lo, tile_hi) among the n_genes * ceil(max_gene_tests / XB_TT) tiles
static int cross_cov_tiles(int64_t n_genes, int32_t max_gene_tests, int64_t n_tests, int64_t tile_lo, int64_t tile_hi, int32_t *tiles) {
  MM_ARG(n_genes >= 0 && max_gene_tests >= 0 && (int64_t)max_gene_tests <= n_tests);
  *tiles = (max_gene_tests + XB_TT - 1) / XB_TT;
  MM_ARG(n_genes * *tiles < 2147483647LL && tile_lo >= 0 && tile_lo <= tile_hi && tile_hi <= n_genes * *tiles);
  return MM_OK;
}

int mm_cross_cov_beta(const double *d_yt, int64_t ld, int32_t num_boot, int32_t n_groups, const int32_t *d_gene_ptr, int64_t n_genes,
                      int32_t max_gene_tests, const double *d_zt, const uint8_t *d_good, const double *d_Nc, int64_t n_tests,
                      int64_t tile_lo, int64_t tile_hi, double *d_beta, void *stream) {
  MM_ARG(d_yt && d_gene_ptr && d_zt && d_good && d_Nc && d_beta);
  MM_ARG(n_tests >= 0 && n_tests < 2147483647LL && n_groups > 0 && n_groups <= 32767 && num_boot > 1 && ld >= (int64_t)num_boot + 1);
  int32_t tiles;
  int rc = cross_cov_tiles(n_genes, max_gene_tests, n_tests, tile_lo, tile_hi, &tiles);
  if (rc != MM_OK) return rc;
  if (tile_hi == tile_lo) return MM_OK;
  int32_t col_tiles = (num_boot + K9_THREADS) / K9_THREADS;      // ceil((num_boot + 1) / K9_THREADS)
  MM_ARG((tile_hi - tile_lo) * col_tiles < 2147483647LL);
  size_t shm = (size_t)n_groups * (XB_TT * 8 + 4) + 8;
  MM_ARG(shm <= 64 * 1024);
  hipLaunchKernelGGL(k_cross_cov_beta, dim3((unsigned)((tile_hi - tile_lo) * col_tiles)), dim3(K9_THREADS), shm, (hipStream_t)stream, d_yt,
                     ld, num_boot, n_groups, tiles, (int32_t)tile_lo, col_tiles, d_gene_ptr, d_zt, d_good, d_Nc, d_beta);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_cross_resampled_block_cov(const double *d_yt, int64_t ld, int32_t num_boot, int32_t n_groups, const int32_t *d_gene_ptr,
                                 int64_t n_genes, int32_t max_gene_tests, const double *d_tt, const double *d_zt, const uint8_t *d_good,
                                 const double *d_Nc, const int16_t *d_rep, const int32_t *d_bcol, const int32_t *d_col_map,
                                 const int32_t *d_n_valid, const int64_t *d_gene_key, uint64_t seed, int64_t n_tests, int64_t tile_lo,
                                 int64_t tile_hi, double *d_beta, double *d_stats, void *stream) {
  int rc = cross_resampled_args(d_yt, ld, num_boot, n_groups, d_gene_ptr, d_tt, d_good, d_Nc, d_rep, d_bcol, d_col_map, d_n_valid, n_tests,
                                d_stats);
  if (rc != MM_OK) return rc;
  MM_ARG(d_zt && d_beta);
  int32_t tiles;
  rc = cross_cov_tiles(n_genes, max_gene_tests, n_tests, tile_lo, tile_hi, &tiles);
  if (rc != MM_OK) return rc;
  if (tile_hi == tile_lo) return MM_OK;
  size_t shm = (size_t)n_groups * (2 * XB_TT * 8 + 12) + 8;
  MM_ARG(shm <= 64 * 1024);
  // beta first, by a launch of its own: the record kernel reads it through a const __restrict__ pointer
  rc = mm_cross_cov_beta(d_yt, ld, num_boot, n_groups, d_gene_ptr, n_genes, max_gene_tests, d_zt, d_good, d_Nc, n_tests, tile_lo, tile_hi,
                         d_beta, stream);
  if (rc != MM_OK) return rc;
  hipLaunchKernelGGL(k_cross_resampled_block_cov, dim3((unsigned)(tile_hi - tile_lo)), dim3(K9_THREADS), shm, (hipStream_t)stream, d_yt, ld,
                     num_boot, n_groups, tiles, (int32_t)tile_lo, d_gene_ptr, d_tt, d_zt, d_good, d_Nc, d_rep, d_bcol, d_col_map, d_n_valid,
                     d_gene_key, seed, d_beta, d_stats);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_residualize_rank1(const double *d_yt, int64_t ld, int32_t num_boot, int32_t n_groups, const int32_t *d_test_gene,
                         const double *d_zt, const uint8_t *d_good, const double *d_Nc, int64_t n_list, double *d_out, void *stream) {
  MM_ARG(d_yt && d_test_gene && d_zt && d_good && d_Nc && d_out && d_out != d_yt);
  MM_ARG(n_list >= 0 && n_groups > 0 && n_groups <= 32767 && num_boot > 1 && ld >= (int64_t)num_boot + 1);
  if (n_list == 0) return MM_OK;
  int32_t col_tiles = (num_boot + K9_THREADS) / K9_THREADS;
  MM_ARG(n_list * col_tiles < 2147483647LL);
  size_t shm = (size_t)n_groups * 20 + 8;
  MM_ARG(shm <= 64 * 1024);
  hipLaunchKernelGGL(k_residualize_rank1, dim3((unsigned)(n_list * col_tiles)), dim3(K9_THREADS), shm, (hipStream_t)stream, d_yt, ld, num_boot,
                     n_groups, col_tiles, d_test_gene, d_zt, d_good, d_Nc, d_out);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_cross_resampled_family(const double *d_yt, int64_t ld, int32_t num_boot, int32_t n_groups, const int32_t *d_gene_ptr,
                              int64_t n_genes, int32_t max_gene_tests, const double *d_tt, const uint8_t *d_good, const double *d_Nc,
                              const int16_t *d_rep, const int32_t *d_bcol, const int32_t *d_col_map, const int32_t *d_n_valid,
                              const int64_t *d_gene_key, uint64_t seed, int64_t n_tests, const double *d_stats, const double *d_scale,
                              int32_t slab, double *d_maxrow, double *d_adj, double *d_fam, void *stream) {
  int rc = cross_resampled_args(d_yt, ld, num_boot, n_groups, d_gene_ptr, d_tt, d_good, d_Nc, d_rep, d_bcol, d_col_map, d_n_valid, n_tests,
                                d_stats);
  if (rc != MM_OK) return rc;
  MM_ARG(d_scale && d_maxrow && d_adj && d_fam);
  MM_ARG(n_genes >= 0 && max_gene_tests >= 0 && (int64_t)max_gene_tests <= n_tests && slab >= 0);
  if (n_genes == 0) return MM_OK;
  if (slab == 0) slab = XF_SLAB;
  int64_t slabs = ((int64_t)num_boot + slab) / slab;      // ceil((num_boot + 1) / slab)
  MM_ARG(n_genes * slabs < 2147483647LL);
  size_t shm = (size_t)n_groups * (XB_TT * 8 + 12) + 2 * XB_TT * 8 + 8;
  MM_ARG(shm <= 64 * 1024);
  hipLaunchKernelGGL(k_cross_family_max, dim3((unsigned)(n_genes * slabs)), dim3(K9_THREADS), shm, (hipStream_t)stream, d_yt, ld, num_boot,
                     n_groups, (int32_t)slabs, slab, d_gene_ptr, d_tt, d_good, d_Nc, d_rep, d_bcol, d_col_map, d_n_valid, d_gene_key, seed,
                     d_stats, d_scale, d_maxrow);
  MM_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_cross_family_count, dim3((unsigned)n_genes), dim3(K9_THREADS), 0, (hipStream_t)stream, ld, num_boot, n_groups,
                     d_gene_ptr, d_good, d_n_valid, d_stats, d_scale, d_maxrow, d_adj, d_fam);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

// The checks the four design-contrast entry points share (the index tables themselves are trusted: engine._design_tables)
static int design_args(bool planes_and_outputs, int64_t ld, int32_t num_boot, int32_t n_groups, const int32_t *d_test_row,
                       const int32_t *d_test_design, const int32_t *d_design_ptr, const int32_t *d_design_grp, const double *d_design_w,
                       int64_t n_tests) {
  MM_ARG(planes_and_outputs && d_test_row && d_test_design && d_design_ptr && d_design_grp && d_design_w);
  MM_ARG(n_tests >= 0 && n_tests < 2147483647LL && n_groups > 0 && num_boot > 0 && ld >= (int64_t)num_boot + 1);
  return MM_OK;
}

int mm_contrast_design_stats(const double *d_ym, const double *d_yv, int64_t ld, int32_t num_boot, int32_t n_groups,
                             const int32_t *d_test_gene, const int32_t *d_test_design, const int32_t *d_design_ptr,
                             const int32_t *d_design_grp, const double *d_design_w, int64_t n_tests, double *d_stats_mean,
                             double *d_stats_var, void *stream) {
  int rc = design_args(d_ym && d_yv && d_stats_mean && d_stats_var, ld, num_boot, n_groups, d_test_gene, d_test_design, d_design_ptr,
                       d_design_grp, d_design_w, n_tests);
  if (rc != MM_OK || n_tests == 0) return rc;
  hipLaunchKernelGGL(k_contrast_design_stats, dim3((unsigned)n_tests), dim3(K9_THREADS), 0, (hipStream_t)stream, d_ym, d_yv, ld, num_boot,
                     n_groups, d_test_gene, d_test_design, d_design_ptr, d_design_grp, d_design_w, d_stats_mean, d_stats_var);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_contrast_design_rows(const double *d_ym, const double *d_yv, int64_t ld, int32_t num_boot, int32_t n_groups,
                            const int32_t *d_test_gene, const int32_t *d_test_design, const int32_t *d_design_ptr,
                            const int32_t *d_design_grp, const double *d_design_w, int64_t n_tests, int32_t which, double *d_out,
                            void *stream) {
  MM_ARG(which == 0 || which == 1);
  int rc = design_args(d_ym && d_yv && d_out, ld, num_boot, n_groups, d_test_gene, d_test_design, d_design_ptr, d_design_grp, d_design_w,
                       n_tests);
  if (rc != MM_OK || n_tests == 0) return rc;
  hipLaunchKernelGGL(k_contrast_design_rows, dim3((unsigned)n_tests), dim3(256), 0, (hipStream_t)stream, d_ym, d_yv, ld, num_boot, n_groups,
                     d_test_gene, d_test_design, d_design_ptr, d_design_grp, d_design_w, which, d_out);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_contrast_design1_stats(const double *d_y, int64_t ld, int32_t num_boot, int32_t n_groups, const int32_t *d_test_row,
                              const int32_t *d_test_design, const int32_t *d_design_ptr, const int32_t *d_design_grp,
                              const double *d_design_w, int64_t n_tests, double *d_stats, void *stream) {
  int rc = design_args(d_y && d_stats, ld, num_boot, n_groups, d_test_row, d_test_design, d_design_ptr, d_design_grp, d_design_w, n_tests);
  if (rc != MM_OK || n_tests == 0) return rc;
  hipLaunchKernelGGL(k_contrast_design1_stats, dim3((unsigned)n_tests), dim3(K9_THREADS), 0, (hipStream_t)stream, d_y, ld, num_boot, n_groups,
                     d_test_row, d_test_design, d_design_ptr, d_design_grp, d_design_w, d_stats);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_contrast_design1_rows(const double *d_y, int64_t ld, int32_t num_boot, int32_t n_groups, const int32_t *d_test_row,
                             const int32_t *d_test_design, const int32_t *d_design_ptr, const int32_t *d_design_grp,
                             const double *d_design_w, int64_t n_tests, double *d_out, void *stream) {
  int rc = design_args(d_y && d_out, ld, num_boot, n_groups, d_test_row, d_test_design, d_design_ptr, d_design_grp, d_design_w, n_tests);
  if (rc != MM_OK || n_tests == 0) return rc;
  hipLaunchKernelGGL(k_contrast_design1_rows, dim3((unsigned)n_tests), dim3(256), 0, (hipStream_t)stream, d_y, ld, num_boot, n_groups,
                     d_test_row, d_test_design, d_design_ptr, d_design_grp, d_design_w, d_out);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_family_maxt(const double *d_ym, const double *d_yv, int64_t ld, int32_t num_boot, int32_t n_groups, const int32_t *d_family_ptr,
                   const int32_t *d_test_gene, const int32_t *d_test_design, const int32_t *d_design_ptr, const int32_t *d_design_grp,
                   const double *d_design_w, const double *d_scale, int32_t stage_cap, int64_t n_fam, double *d_maxrow, double *d_adj,
                   double *d_fam, void *stream) {
  MM_ARG(n_fam >= 0 && n_fam < 2147483647LL && stage_cap >= 0 && stage_cap <= FM_MAX_STAGED);
  int rc = design_args(d_ym && d_yv && d_family_ptr && d_scale && d_maxrow && d_adj && d_fam, ld, num_boot, n_groups, d_test_gene,
                       d_test_design, d_design_ptr, d_design_grp, d_design_w, 0);
  if (rc != MM_OK || n_fam == 0) return rc;
  size_t shm = (size_t)stage_cap * 2 * 2 * 8;
  hipLaunchKernelGGL(k_family_maxt, dim3((unsigned)n_fam), dim3(K9_THREADS), shm, (hipStream_t)stream, d_ym, d_yv, ld, num_boot, n_groups,
                     d_family_ptr, d_test_gene, d_test_design, d_design_ptr, d_design_grp, d_design_w, d_scale, stage_cap, d_maxrow, d_adj,
                     d_fam);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_family_maxt1(const double *d_y, int64_t ld, int32_t num_boot, int32_t n_groups, const int32_t *d_family_ptr,
                    const int32_t *d_test_row, const int32_t *d_test_design, const int32_t *d_design_ptr, const int32_t *d_design_grp,
                    const double *d_design_w, const double *d_scale, int32_t stage_cap, int64_t n_fam, double *d_maxrow, double *d_adj,
                    double *d_fam, void *stream) {
  MM_ARG(n_fam >= 0 && n_fam < 2147483647LL && stage_cap >= 0 && stage_cap <= FM_MAX_STAGED);
  int rc = design_args(d_y && d_family_ptr && d_scale && d_maxrow && d_adj && d_fam, ld, num_boot, n_groups, d_test_row, d_test_design,
                       d_design_ptr, d_design_grp, d_design_w, 0);
  if (rc != MM_OK || n_fam == 0) return rc;
  size_t shm = (size_t)stage_cap * 1 * 2 * 8;
  hipLaunchKernelGGL(k_family_maxt1, dim3((unsigned)n_fam), dim3(K9_THREADS), shm, (hipStream_t)stream, d_y, ld, num_boot, n_groups,
                     d_family_ptr, d_test_row, d_test_design, d_design_ptr, d_design_grp, d_design_w, d_scale, stage_cap, d_maxrow, d_adj,
                     d_fam);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

// The checks and the launch shape mm_joint_stats (NP = 2) and mm_joint1_stats (NP = 1) share.  A design has r <= n_d <= n_groups:
// z_0 takes NP x n_groups doubles of LDS, the staged L at most JOINT_LDS_DOUBLES (*cap); *tier: 0, 1, 2 = the kernel's NDR
// JOINT_REG_SMALL, JOINT_REG_GROUPS, 0.
static int joint_args(int n_planes, bool planes_and_outputs, int64_t ld, int32_t num_boot, int32_t n_groups, const int32_t *d_test_row,
                      const int32_t *d_test_design, const int32_t *d_design_ptr, const int32_t *d_design_rank,
                      const int64_t *d_design_lofs, const int32_t *d_design_grp, const double *d_design_L, int64_t n_tests, int32_t *cap,
                      size_t *shm, int *tier) {
  MM_ARG(planes_and_outputs && d_test_row && d_test_design && d_design_ptr && d_design_rank && d_design_lofs && d_design_grp && d_design_L);
  MM_ARG(n_tests >= 0 && n_tests < 2147483647LL && n_groups > 0 && num_boot > 0 && ld >= (int64_t)num_boot + 1);
  int64_t c = (int64_t)n_groups * n_groups < JOINT_LDS_DOUBLES ? (int64_t)n_groups * n_groups : JOINT_LDS_DOUBLES;
  *cap = (int32_t)c;
  *shm = ((size_t)n_groups * n_planes + (size_t)c) * 8;
  MM_ARG(*shm <= 64 * 1024);
  *tier = n_groups <= JOINT_REG_SMALL ? 0 : n_groups <= JOINT_REG_GROUPS ? 1 : 2;
  return MM_OK;
}

int mm_joint_stats(const double *d_ym, const double *d_yv, int64_t ld, int32_t num_boot, int32_t n_groups,
                   const int32_t *d_test_gene, const int32_t *d_test_design, const int32_t *d_design_ptr,
                   const int32_t *d_design_rank, const int64_t *d_design_lofs, const int32_t *d_design_grp,
                   const double *d_design_L, int64_t n_tests, double *d_stats_mean, double *d_stats_var, void *stream) {
  int32_t cap;
  size_t shm;
  int tier;
  int rc = joint_args(2, d_ym && d_yv && d_stats_mean && d_stats_var, ld, num_boot, n_groups, d_test_gene, d_test_design, d_design_ptr,
                      d_design_rank, d_design_lofs, d_design_grp, d_design_L, n_tests, &cap, &shm, &tier);
  if (rc != MM_OK || n_tests == 0) return rc;
  auto kernel = tier == 0 ? k_joint_stats<JOINT_REG_SMALL> : tier == 1 ? k_joint_stats<JOINT_REG_GROUPS> : k_joint_stats<0>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)n_tests), dim3(K9_THREADS), shm, (hipStream_t)stream, d_ym, d_yv, ld, num_boot, n_groups, cap,
                     d_test_gene, d_test_design, d_design_ptr, d_design_rank, d_design_lofs, d_design_grp, d_design_L, d_stats_mean,
                     d_stats_var);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_joint1_stats(const double *d_y, int64_t ld, int32_t num_boot, int32_t n_groups, const int32_t *d_test_row,
                    const int32_t *d_test_design, const int32_t *d_design_ptr, const int32_t *d_design_rank,
                    const int64_t *d_design_lofs, const int32_t *d_design_grp, const double *d_design_L, int64_t n_tests,
                    double *d_stats, void *stream) {
  int32_t cap;
  size_t shm;
  int tier;
  int rc = joint_args(1, d_y && d_stats, ld, num_boot, n_groups, d_test_row, d_test_design, d_design_ptr, d_design_rank, d_design_lofs,
                      d_design_grp, d_design_L, n_tests, &cap, &shm, &tier);
  if (rc != MM_OK || n_tests == 0) return rc;
  auto kernel = tier == 0 ? k_joint1_stats<JOINT_REG_SMALL> : tier == 1 ? k_joint1_stats<JOINT_REG_GROUPS> : k_joint1_stats<0>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)n_tests), dim3(K9_THREADS), shm, (hipStream_t)stream, d_y, ld, num_boot, n_groups, cap,
                     d_test_row, d_test_design, d_design_ptr, d_design_rank, d_design_lofs, d_design_grp, d_design_L, d_stats);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

}  // extern "C"
