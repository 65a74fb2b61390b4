// boot.hip -- K6+K7+K8: the unique-value bootstrap, replayed draw-for-draw against numpy.
//
// Reference behaviour replaced:
//   bootstrap._bootstrap_1d            memento/bootstrap.py:97-110
//     gen = Generator(PCG64(5)); w = gen.multinomial(N_g, counts/counts.sum(), size=B).T
//   estimator._hyper_1d_relative tuple branch   memento/estimator.py:171-174, :182-183
//   estimator._residual_variance + hypothesis_test._fill + np.log
//                                      memento/estimator.py:103-111, hypothesis_test.py:23-33, :186-197
//
// One lane = one (gene, group) pair = one sequential PCG64 stream (the reference re-seeds PCG64(5) per
// pair).  The 64 pairs of a tile walk their bins in lock step so every operand load is a coalesced
// 512-B row; the multinomial weights never leave registers (the K x B matrix is never materialised).
// fp64, contraction OFF (-ffp-contract=off): replicate means/variances are bit-identical to numpy's.
// The three tile kernels (k_boot1d_replay, k_boot1d_free, k_boot2d_replay) are built from parts defined once, above k_boot1d_replay:
// tile_lane (the lane's chain, the unused-lane rule), a plane and a record cursor for Ops1D / Ops2D, draw_bin (the draw of one bin), Stat1D /
// Stat2D (the replicate statistic), tile_lockstep (the lock-step loop).  chain_body and k_boot1d_async draw in their own forms.
#include "mm_common.h"
#include "npy_rng.h"
#include <type_traits>

// Chains that run one per WAVE (below: chain_body, k_boot1d_chain).  The tile kernel takes them as well: a tile flagged in
// ``tile_chain`` is such a chain, so that the host can put chain waves at chosen places of ONE launch's dispatch order.
#define MM_CHAIN_CLOCK_OFF (1 << 18)   // engine.CHAIN_CLOCK_OFF: the chain waves' records in the mm_debug_wave_clock buffer
struct ChainArgs {
  const double *ops;           // 8-double operand records (mm_bins_order, MM_CHAIN_SLOT pairs)
  const int64_t *base;         // [chain] first record
  const int32_t *K;            // [chain] bins
  const double *nobs, *omq;    // [chain] N_g, 1 - q_g
  const int64_t *row;          // [chain] output row
  const uint64_t *jump;        // [64][4] PCG64 jump constants
  const int32_t *tile_chain;   // [tile] chain index or -1 (tile kernel only; may be NULL)
  int32_t *w_dump;             // optional weights [chain][k][b]
  int32_t kmax_dump;
};
template <bool FAST>
__device__ __forceinline__ void chain_body(const ChainArgs &ca, int64_t ch, int lane, uint64_t st0, uint64_t st1, int32_t num_boot,
                                           int32_t mean_only, int64_t ld, double *__restrict__ out_mean, double *__restrict__ out_var,
                                           int64_t *__restrict__ wave_clock);

// The uniforms of a stream as a table (engine.pcg64_stream_table; the tile kernel once read its uniforms from such a table:
// measured slower, a wave's lanes sit at 64 different places of it).
// out[i] = the (i + 1)-th uniform of the stream that starts at ``state`` (numpy: Generator(PCG64).random()): every thread jumps
// to the start of its run of 64 outputs (PCG's O(log n) advance) and steps through it.
__global__ __launch_bounds__(256) void k_pcg64_stream(double *__restrict__ out, int64_t n, uint64_t st0, uint64_t st1, uint64_t st2,
                                                      uint64_t st3) {
  typedef unsigned __int128 u128;
  const u128 MULT = ((u128)2549297995355413924ULL << 64) | 4865540595714422341ULL;
  int64_t first = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 64;
  if (first >= n) return;
  u128 state = ((u128)st0 << 64) | st1, inc = ((u128)st2 << 64) | st3;
  u128 acc_mult = 1, acc_plus = 0, cur_mult = MULT, cur_plus = inc;
  for (uint64_t delta = (uint64_t)first; delta > 0; delta >>= 1) {
    if (delta & 1) {
      acc_mult *= cur_mult;
      acc_plus = acc_plus * cur_mult + cur_plus;
    }
    cur_plus = (cur_mult + 1) * cur_plus;
    cur_mult *= cur_mult;
  }
  state = acc_mult * state + acc_plus;
  npyrng::Pcg64 g{(uint64_t)(state >> 64), (uint64_t)state, st2, st3};
  int64_t last = first + 64 < n ? first + 64 : n;
  for (int64_t i = first; i < last; i++) out[i] = npyrng::pcg64_next_double(g);
}

#ifndef BOOT_MIN_WAVES
#define BOOT_MIN_WAVES 2
#endif
#ifndef BOOT_SETPRIO
#define BOOT_SETPRIO 2
#endif
// MINW = waves per SIMD the register budget is set for: 2 when every tile is resident (<= 2048 tiles, the pairing order below
// assumes two per SIMD), 3 in the many-tile regime where a third resident wave adds a little issue throughput.
#ifndef BOOT_BTPE_CAP
#define BOOT_BTPE_CAP 1          // BTPE attempts a lane makes per bin step of its tile (0: as many as the draw takes, every lane waiting)
#endif
#ifndef BOOT_TAIL_LANES
#define BOOT_TAIL_LANES 4        // with at most this many lanes still inside the replicate, draws run to completion
#endif
// One bin's share of a replicate's two sums (estimator.py:171-174, :182-183) and the replicate's mean / variance from them.  Every 1D
// kernel below adds its bins in chain order through these two: the association of every product is numpy's, which is what makes
// the replicate moments of all of them the same bit for bit.
__device__ __forceinline__ void accumulate_1d(double &M1, double &M2, int32_t w, double v, double a, double b, double omq) {
  double wd = (double)w;
  M1 += (v * wd) * a;
  M2 += ((v * v) * wd) * b - ((omq * v) * wd) * b;
}
__device__ __forceinline__ void close_replicate(double M1, double M2, double nobs, int32_t mean_only, double *mean_out, double *var_out) {
  double mean = M1 / nobs;
  double var = M2 / nobs - mean * mean;
  if (mean_only) {  // estimator._mean_only_1p (estimator.py:188-204): [mean + 1, 10]
    mean = mean + 1;
    var = 10.0;
  }
  *mean_out = mean;
  *var_out = var;
}
// A wave of a tile kernel whose "tile" is flagged in ca.tile_chain runs that chain in the one-wave-per-chain form, at the tile's
// place (and priority) in the dispatch order.  True when it did: the wave is done.
template <bool FAST>
__device__ __forceinline__ bool run_tile_as_chain(const ChainArgs &ca, int64_t tile, int64_t n_tiles, int lane, uint64_t st0, uint64_t st1,
                                                  int32_t num_boot, int32_t mean_only, int64_t ld, double *__restrict__ out_mean,
                                                  double *__restrict__ out_var, int64_t *__restrict__ wave_clock) {
  if (ca.tile_chain) {
    int cidx = __builtin_amdgcn_readfirstlane(ca.tile_chain[tile]);
    if (cidx >= 0) {
      if (tile * 2 < n_tiles) __builtin_amdgcn_s_setprio(BOOT_SETPRIO);
      chain_body<FAST>(ca, (int64_t)cidx, lane, st0, st1, num_boot, mean_only, ld, out_mean, out_var,
                       wave_clock ? wave_clock + MM_CHAIN_CLOCK_OFF : nullptr);
      return true;
    }
  }
  return false;
}

// ------------------------------------------------------------------------------------------------
// The tile kernels' parts.  A lane's chain: K = 0 marks an unused lane (K <= 0 or row < 0 in the tables; where the chains are read as
// records, REC, slot_rec < 0 as well): such a lane draws nothing and stores nothing, so whether a lane runs is decided from this K alone.
// The loader also raises the wave's issue priority in the first half of the grid: two waves share a SIMD, the host puts the long tiles
// there (engine.pair_tiles) and pairs each with a short one from the second half; the long tile is the critical path and is served first.
struct TileLane {
  int64_t slot, row, rec;   // slot of the tables, output row, the chain's first record (REC; 0 otherwise)
  int K;
  double nobs, omq;         // N_g, 1 - q of the pair's group
  int32_t n;                // N_g < 2^31 (checked by the host)
  __device__ __forceinline__ double *out(double *plane, int64_t ld) const { return plane + row * ld + 1; }   // the replicates' cells
};
template <bool REC>
__device__ __forceinline__ TileLane tile_lane(int64_t tile, int64_t n_tiles, int lane, const int32_t *__restrict__ slot_K,
                                              const double *__restrict__ slot_nobs, const double *__restrict__ slot_omq,
                                              const int64_t *__restrict__ slot_row, const int64_t *__restrict__ slot_rec) {
  if (tile * 2 < n_tiles) __builtin_amdgcn_s_setprio(BOOT_SETPRIO);
  const int64_t slot = tile * 64 + lane;
  TileLane t{slot, slot_row[slot], REC ? slot_rec[slot] : 0, slot_K[slot], slot_nobs[slot], slot_omq[slot], 0};
  if (t.K <= 0 || t.row < 0 || t.rec < 0) t.K = 0;
  t.n = (int32_t)t.nobs;
  return t;
}
// The operands of one bin, and where a lane's chain keeps them: [row][64] planes (the 64 lanes of a tile read one coalesced 512-B row
// per plane and bin) or the chain's own 8-double records (mm_bins_order / mm_bins_order2d with MM_CHAIN_SLOT pairs: one 64-B half line
// per bin).  The kernels load bin k + 1 while bin k computes: one lane is one latency-bound sequential chain, so an exposed L2 / HBM
// round trip per step would be a large part of the step.
struct Ops1D { double pk, lq, v, a, b; };
struct Planes1D {
  const double *__restrict__ pk, *__restrict__ lq, *__restrict__ v, *__restrict__ a, *__restrict__ b;
  int64_t obase;   // first row of the tile * 64 + lane
  __device__ __forceinline__ Ops1D load(int k) const {
    int64_t o = obase + (int64_t)k * 64;
    return Ops1D{pk[o], lq[o], v[o], a[o], b[o]};
  }
};
struct Records1D {
  const double *__restrict__ rec;   // [K][8]: pk, lq, count, 1/sf, 1/sf^2, (3 spare)
  __device__ __forceinline__ Ops1D load(int k) const {
    const double *p = rec + (int64_t)k * 8;
    double2 t0 = *(const double2 *)(p), t1 = *(const double2 *)(p + 2);
    return Ops1D{t0.x, t0.y, t1.x, t1.y, p[4]};
  }
};

// The draw of one bin of a lane's chain: the weight of the bin.  Every bin but the last draws a binomial from what the replicate has
// left (``dn``; ``live`` goes off when nothing is left, and the later bins get 0 without a draw, as in numpy); the last bin takes the
// remainder.  The lanes share the instruction stream, not the bin index: with ``cap`` > 0 a BTPE draw makes that many attempt(s) per bin
// step, and a lane whose attempts were all rejected comes back ``pending``: it stays on its bin and tries again in the next step, beside
// its neighbours' next draws (npyrng::binomial_pre_capped) -- so a step costs the wave one attempt, not as many as its unluckiest lane
// needs.  The kernels' cap is a constant while more than BOOT_TAIL_LANES lanes are inside the replicate; then draws run to completion (0).
// dn and live go in and come back by value: taken by reference, k_boot2d_replay<., false, .> came out with other registers (180 VGPRs
// for 185 in the two-wave builds), and every kernel is to keep its resources (profiles/replay_shared_step_resources.txt).
struct BinDraw {
  int32_t w, dn;        // the bin's weight (meaningless when pending); what the replicate has left behind this bin
  bool live, pending;
};
template <bool FAST>
__device__ __forceinline__ BinDraw draw_bin(npyrng::Pcg64 &g, double pk, double lq, int32_t dn, bool live, bool last_bin, int cap) {
  int32_t w;
  bool pending = false;
  if (!last_bin) {
    w = 0;
    if (live) {
      if constexpr (FAST) w = npyrng::binomial_pre_capped<int32_t>(g, pk, lq, dn, cap, pending);
      else w = npyrng::binomial_pre<int32_t, false>(g, pk, lq, dn);
      if (!pending) {
        dn -= w;
        if (dn <= 0) live = false;
      }
    }
  } else {
    w = dn > 0 ? dn : 0;
  }
  return BinDraw{w, dn, live, pending};
}
// The replicate statistic of a 1D chain: the two sums of accumulate_1d, closed into the replicate's cell of the mean and the variance
// row.  Chains of fewer than MIN_K bins do not run; a single bin gives all-NaN replicates (bootstrap.py:97-98).
// w_dump (optional): int32 weights [slot][k < kmax_dump][r < num_boot].
struct Stat1D {
  static constexpr int MIN_K = 2;
  const TileLane &t;
  int32_t num_boot, mean_only;
  double *om, *ov;   // t.out() of the two planes
  int32_t *__restrict__ w_dump;
  int32_t kmax_dump;
  double M1, M2;
  __device__ __forceinline__ void short_chain() {
    if (t.K == 1) {
      for (int r = 0; r < num_boot; r++) om[r] = ov[r] = NAN;
    }
  }
  __device__ __forceinline__ void begin() { M1 = 0.0, M2 = 0.0; }
  __device__ __forceinline__ void dump(int k, int r, int32_t w) { if (w_dump) w_dump[((int64_t)t.slot * kmax_dump + k) * num_boot + r] = w; }
  __device__ __forceinline__ void add(int32_t w, const Ops1D &c) { accumulate_1d(M1, M2, w, c.v, c.a, c.b, t.omq); }
  __device__ __forceinline__ void close(int r) { close_replicate(M1, M2, t.nobs, mean_only, om + r, ov + r); }
};

// The lock-step tile body (k_boot1d_replay, k_boot2d_replay): one lane = one chain, every lane of the wave in the same replicate.
// Within a replicate each lane is on its own bin (draw_bin: a pending lane stays behind); the lanes meet again at the replicate's end.
// ``Stat`` is the replicate statistic (Stat1D, Stat2D), ``ops`` the lane's operand cursor, CAP the BTPE attempts per bin step.
template <bool FAST, int CAP, typename Stat, typename Cursor>
__device__ __forceinline__ void tile_lockstep(const TileLane &t, uint64_t st0, uint64_t st1, uint64_t st2, uint64_t st3, int32_t num_boot,
                                              Stat &stat, const Cursor &ops) {
  const int K = t.K;
  stat.short_chain();
  npyrng::Pcg64 g{st0, st1, st2, st3};
  const bool run = K >= Stat::MIN_K;
  auto c = ops.load(0);
  for (int r = 0; r < num_boot; r++) {
    stat.begin();
    int32_t dn = t.n;
    bool live = true;
    int kl = 0;
    for (;;) {
      const bool act = run && kl < K;
      const uint64_t act_mask = __ballot(act);
      if (act_mask == 0) break;
      const int cap = (CAP > 0 && __popcll(act_mask) > BOOT_TAIL_LANES) ? CAP : 0;
      const auto nx = ops.load(kl + 1 < K ? kl + 1 : 0);
      bool adv = false;
      if (act) {
        const BinDraw d = draw_bin<FAST>(g, c.pk, c.lq, dn, live, kl >= K - 1, cap);
        dn = d.dn;
        live = d.live;
        if (!d.pending) {
          stat.dump(kl, r, d.w);
          if (d.w != 0) stat.add(d.w, c);
          adv = true;
        }
      }
      if (adv) {
        kl++;
        c = nx;
      }
    }
    if (run) stat.close(r);
  }
}

// The strict 1D tile kernel: the lock-step body on [row][64] operand planes, the tile's rows from tile_ptr[tile].  A tile flagged in
// ca.tile_chain is a chain of the one-wave-per-chain form instead.
template <int MINW, bool FAST>
__global__ __launch_bounds__(256, MINW) void k_boot1d_replay(const double *__restrict__ pk_, const double *__restrict__ lq_,
                                                       const double *__restrict__ v, const double *__restrict__ a,
                                                       const double *__restrict__ b,
                                                       const int64_t *__restrict__ tile_ptr, int64_t n_tiles,
                                                       const int32_t *__restrict__ slot_K, const double *__restrict__ slot_nobs,
                                                       const double *__restrict__ slot_omq, const int64_t *__restrict__ slot_row, uint64_t st0, uint64_t st1,
                                                       uint64_t st2, uint64_t st3, int32_t num_boot, int32_t mean_only,
                                                       int64_t ld, double *__restrict__ out_mean, double *__restrict__ out_var,
                                                       int32_t *__restrict__ w_dump, int32_t kmax_dump,
                                                       int64_t *__restrict__ wave_clock, ChainArgs ca) {
  int lane = mm_lane();
  int64_t tile = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (tile >= n_tiles) return;
  if (run_tile_as_chain<FAST>(ca, tile, n_tiles, lane, st0, st1, num_boot, mean_only, ld, out_mean, out_var, wave_clock)) return;
  int64_t t_start = wave_clock ? (int64_t)wall_clock64() : 0;
  const TileLane t = tile_lane<false>(tile, n_tiles, lane, slot_K, slot_nobs, slot_omq, slot_row, nullptr);
  Stat1D stat{t, num_boot, mean_only, t.out(out_mean, ld), t.out(out_var, ld), w_dump, kmax_dump};
  const Planes1D ops{pk_, lq_, v, a, b, tile_ptr[tile] * 64 + lane};
  tile_lockstep<FAST, BOOT_BTPE_CAP>(t, st0, st1, st2, st3, num_boot, stat, ops);
  if (wave_clock && lane == 0) {  // profiling hook (mm_debug_wave_clock): when and where this wave ran
    wave_clock[tile * 4 + 0] = t_start;
    wave_clock[tile * 4 + 1] = (int64_t)wall_clock64();
    wave_clock[tile * 4 + 2] = (int64_t)__builtin_amdgcn_s_getreg((31 << 11) | 4);    // HW_REG_HW_ID: se / cu / simd / wave slot
    wave_clock[tile * 4 + 3] = (int64_t)__builtin_amdgcn_s_getreg((31 << 11) | 20);   // HW_REG_XCC_ID
  }
}

// ------------------------------------------------------------------------------------------------
// CHAIN kernel: one WAVE per (gene, group) chain.  A chain is one sequential PCG64 stream, so a chain that sits alone in a
// 64-wide tile of k_boot1d_replay leaves 63 lanes idle and still pays the per-lane (exec-masked) control flow of that kernel.
// Here every value of the chain is wave-uniform -- operands come in through scalar loads, the samplers' branches are scalar
// branches -- and the 64 lanes do the one thing that parallelises: the generator.  PCG64 is an LCG, so the state j steps on
// is A^j * s + C_j (mod 2^128): lane j holds (A^(j+1), C_(j+1)) and one 128-bit multiply-add per lane produces the next 64
// outputs of the stream at once; the samplers take them one by one with v_readlane.  Same draws, same replicate moments (bit
// for bit) as k_boot1d_replay; the host sends the long chains here and packs the rest into tiles (engine.Bootstrap1D.run).
namespace npyrng {
__device__ __forceinline__ uint64_t wave_read64(uint64_t x, int lane) {
  uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, lane);
  uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), lane);
  return ((uint64_t)hi << 32) | lo;
}

struct WaveRng {
  uint64_t s_hi, s_lo;              // per lane: the state (lane + 1) steps after the batch's base state
  double u;                         // per lane: the uniform that state yields
  uint64_t a_hi, a_lo, c_hi, c_lo;  // per lane: A^(lane+1), C_(lane+1)
  int pos;                          // wave-uniform: next lane to hand out
  typedef int Mark;
  __device__ __forceinline__ Mark mark() const { return pos; }
  __device__ __forceinline__ void rewind(Mark m) { pos = m; }
  __device__ __forceinline__ void fill(uint64_t b_hi, uint64_t b_lo) {   // b = wave-uniform base state
    uint64_t lo = a_lo * b_lo;
    uint64_t hi = __umul64hi(a_lo, b_lo) + a_hi * b_lo + a_lo * b_hi;
    uint64_t nlo = lo + c_lo;
    uint64_t nhi = hi + c_hi + (nlo < lo ? 1ULL : 0ULL);
    s_lo = nlo;
    s_hi = nhi;
    uint64_t x = nhi ^ nlo;
    unsigned rot = (unsigned)(nhi >> 58);
    uint64_t out = (x >> rot) | (x << ((64u - rot) & 63u));
    u = (double)(out >> 11) * (1.0 / 9007199254740992.0);
    pos = 0;
  }
  __device__ __forceinline__ void refill() {   // continue behind the last uniform handed out
    if (pos == 0) return;
    uint64_t b_hi = wave_read64(s_hi, pos - 1), b_lo = wave_read64(s_lo, pos - 1);
    fill(b_hi, b_lo);
  }
  __device__ __forceinline__ void reserve(int n) {
    if (pos > 64 - n) refill();
  }
  __device__ __forceinline__ int max_attempts() const { return 16; }
};

__device__ __forceinline__ double pcg64_next_double(WaveRng &g) {
  if (g.pos == 64) g.refill();
  uint64_t bits = wave_read64((uint64_t)__double_as_longlong(g.u), g.pos);
  g.pos++;
  return __longlong_as_double((long long)bits);
}
}  // namespace npyrng

#ifndef CHAIN_MIN_WAVES
#define CHAIN_MIN_WAVES 3
#endif
#ifndef CHAIN_PRIO
#define CHAIN_PRIO 3      // issue priority of a chain wave against the tile kernel's waves (first half of its grid: BOOT_SETPRIO = 2)
#endif
// Four chains (waves) per 256-thread workgroup and the register budget of the tile kernel's three-waves-per-SIMD build: a
// workgroup of either kernel then takes the same resources, so the chain waves and the tile waves of one bootstrap are all
// resident together however the dispatcher interleaves the two launches (64-thread workgroups with their own register / LDS
// footprint fragmented the CUs: tile workgroups waited for seconds, measured in profiles/README.md).
template <bool FAST>
__device__ __forceinline__ void chain_body(const ChainArgs &ca, int64_t ch, int lane, uint64_t st0, uint64_t st1, int32_t num_boot,
                                           int32_t mean_only, int64_t ld, double *__restrict__ out_mean, double *__restrict__ out_var,
                                           int64_t *__restrict__ wave_clock) {
  const double *__restrict__ ops = ca.ops;
  const int64_t *__restrict__ ch_base = ca.base;
  const uint64_t *__restrict__ jump = ca.jump;
  int32_t *__restrict__ w_dump = ca.w_dump;
  const int32_t kmax_dump = ca.kmax_dump;
  int64_t t_start = wave_clock ? (int64_t)wall_clock64() : 0;
  const int K = ca.K[ch];
  const int64_t row = ca.row[ch];
  const double nobs = ca.nobs[ch], omq = ca.omq[ch];
  const int32_t n = (int32_t)nobs;
  // wave-uniform addresses: the compiler reads the operand records with scalar loads, one bin ahead (staging them in LDS
  // instead measured the same step time: the scalar cache / L2 round trip is already hidden behind the step)
  const double *__restrict__ op = ops + ch_base[ch] * 8;      // [K][8]: pk, lq, v, a, b, (3 spare)
  double *om = out_mean + row * ld + 1;
  double *ov = out_var + row * ld + 1;
  npyrng::WaveRng g;
  g.a_hi = jump[lane * 4 + 0];
  g.a_lo = jump[lane * 4 + 1];
  g.c_hi = jump[lane * 4 + 2];
  g.c_lo = jump[lane * 4 + 3];
  g.fill(st0, st1);
  double keep_m = 0.0, keep_v = 0.0;     // lane (r & 63) keeps replicate r until 64 of them go out as one coalesced store
  for (int r = 0; r < num_boot; r++) {
    double M1 = 0.0, M2 = 0.0;
    int32_t dn = n;
    double c_pk = op[0], c_lq = op[1], c_v = op[2], c_a = op[3], c_b = op[4];
    for (int k = 0; k < K - 1; k++) {
      const double *nx = op + (int64_t)(k + 1) * 8;          // k + 1 <= K - 1: the last bin's v, a, b are read here
      double n_pk = nx[0], n_lq = nx[1], n_v = nx[2], n_a = nx[3], n_b = nx[4];
      int32_t w = npyrng::binomial_pre<int32_t, FAST, true>(g, c_pk, c_lq, dn);
      dn -= w;
      if (w_dump && lane == 0) w_dump[((int64_t)ch * kmax_dump + k) * num_boot + r] = w;
      if (w != 0) accumulate_1d(M1, M2, w, c_v, c_a, c_b, omq);
      c_pk = n_pk; c_lq = n_lq; c_v = n_v; c_a = n_a; c_b = n_b;
      if (dn <= 0) break;                                      // numpy stops the chain here; nothing is left for later bins
    }
    if (dn > 0) {                                              // the loop ran to its end: c_* hold the last bin, which takes the rest
      if (w_dump && lane == 0) w_dump[((int64_t)ch * kmax_dump + (K - 1)) * num_boot + r] = dn;
      accumulate_1d(M1, M2, dn, c_v, c_a, c_b, omq);
    }
    double mean, var;
    close_replicate(M1, M2, nobs, mean_only, &mean, &var);
    if (lane == (r & 63)) {
      keep_m = mean;
      keep_v = var;
    }
    if ((r & 63) == 63 || r == num_boot - 1) {
      int r0 = r & ~63;
      if (r0 + lane <= r) {
        om[r0 + lane] = keep_m;
        ov[r0 + lane] = keep_v;
      }
    }
  }
  if (wave_clock && lane == 0) {   // 8 int64 per chain: start, end (100 MHz); the rest spare
    wave_clock[ch * 8 + 0] = t_start;
    wave_clock[ch * 8 + 1] = (int64_t)wall_clock64();
  }
}

template <bool FAST>
__global__ __launch_bounds__(256, CHAIN_MIN_WAVES) void k_boot1d_chain(ChainArgs ca, int64_t n_chains, uint64_t st0, uint64_t st1,
                                                       int32_t num_boot, int32_t mean_only, int64_t ld, double *__restrict__ out_mean,
                                                       double *__restrict__ out_var, int64_t *__restrict__ wave_clock) {
  const int lane = threadIdx.x & 63;
  const int64_t ch = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wave-uniform
  if (ch >= n_chains) return;
  __builtin_amdgcn_s_setprio(CHAIN_PRIO);
  chain_body<FAST>(ca, ch, lane, st0, st1, num_boot, mean_only, ld, out_mean, out_var, wave_clock);
}

// ------------------------------------------------------------------------------------------------
// ASYNC tile kernel: one lane = one chain, like k_boot1d_replay, but the lanes of a wave are NOT in lock step.  Every lane
// carries the state of its own draw (npyrng::LaneDraw) and its own position (replicate r, bin k); one pass of the wave runs a
// fixed sequence of phases -- retire / start, <= 9 steps of the inversion search, one BTPE attempt, explicit product, squeeze,
// exact redo -- each for the lanes that are in it, and a lane whose draw is done goes on to ITS next bin in the next pass whatever
// its neighbours are doing.  No lane waits for the longest search, the unluckiest BTPE draw or the longest chain of its wave; a
// lane's operands are the 8-double records of its chain (the mm_boot1d_chain layout), read one bin ahead.  Draws and replicate
// moments are those of k_boot1d_replay bit for bit (same samplers, same arithmetic per draw, same accumulation order).
#ifndef ASYNC_MIN_WAVES
#define ASYNC_MIN_WAVES 2     // 64 chains per wave: the chains of a launch rarely fill two waves per SIMD; no register spills
#endif
// one record with five 8-byte loads, as this kernel has always read it (Records1D reads the same record with two 16-byte loads)
__device__ __forceinline__ Ops1D load_bin(const double *__restrict__ rec) { return Ops1D{rec[0], rec[1], rec[2], rec[3], rec[4]}; }

template <bool FAST>
__global__ __launch_bounds__(256, ASYNC_MIN_WAVES) void k_boot1d_async(const double *__restrict__ ops, const int64_t *__restrict__ ch_base,
                                                        const int32_t *__restrict__ ch_K, const double *__restrict__ ch_nobs,
                                                        const double *__restrict__ ch_omq, const int64_t *__restrict__ ch_row,
                                                        int64_t n_slots, uint64_t st0, uint64_t st1, uint64_t st2, uint64_t st3,
                                                        int32_t num_boot, int32_t mean_only, int64_t ld, double *__restrict__ out_mean,
                                                        double *__restrict__ out_var, int32_t *__restrict__ w_dump, int32_t kmax_dump,
                                                        int64_t *__restrict__ wave_clock) {
  using namespace npyrng;
  const int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t t_start = wave_clock ? (int64_t)wall_clock64() : 0;
  int K = slot < n_slots ? ch_K[slot] : 0;
  if (K < 2) K = 0;                                             // unused lane (K == 1 rows are NaN rows, written by the host)
  const int64_t sl = K ? slot : 0;
  const double nobs = ch_nobs[sl], omq = ch_omq[sl];
  const int32_t n = (int32_t)nobs;
  const double *__restrict__ rec = ops + ch_base[sl] * 8;      // [K][8]: pk, lq, v, a, b, (3 spare)
  const int64_t row = ch_row[sl];
  double *om = out_mean + row * ld + 1;
  double *ov = out_var + row * ld + 1;
  Pcg64 g{st0, st1, st2, st3};
  LaneDraw D = LaneDraw();
  int32_t state = K ? LS_RESTART : LS_IDLE;
  int32_t r = 0, k = 0, dn = n;
  double M1 = 0.0, M2 = 0.0;
  Ops1D cur = load_bin(rec), nxt = load_bin(rec + (K ? 8 : 0));
  int64_t passes = 0;
  while (__ballot(state != LS_IDLE)) {
    passes++;
    // ---- retire the finished draw; finish the replicate or move on to the next bin ----------------------------------------
    if (state == LS_DONE) {
      const int32_t w = D.w;
      if (w_dump) w_dump[((int64_t)slot * kmax_dump + k) * num_boot + r] = w;
      if (w != 0) accumulate_1d(M1, M2, w, cur.v, cur.a, cur.b, omq);
      dn -= w;
      k++;
      cur = nxt;                                                 // record k
      if (dn <= 0 || k == K - 1) {
        state = LS_FINISH;                                       // the replicate is complete: closed in one of the passes below
      } else {
        nxt = load_bin(rec + (int64_t)(k + 1) * 8);              // k + 1 <= K - 1
        state = LS_START;
      }
    } else if (state == LS_RESTART) {
      M1 = 0.0;
      M2 = 0.0;
      dn = n;
      k = 0;
      state = LS_START;
    }
    // closing a replicate (the last bin's remainder, two fp64 divisions, the stores, the next replicate's first operands) is ~100
    // dependent instructions that some lane of a 64-wide wave needs on nearly every pass: done every fourth pass, for all lanes
    // that wait for it (a lane loses 1.5 passes per replicate on average, every other lane saves the time on three passes in four)
    if ((passes & 3) == 0 && state == LS_FINISH) {
      if (dn > 0) {                                              // every bin but the last has drawn: the last one takes the rest
        if (w_dump) w_dump[((int64_t)slot * kmax_dump + k) * num_boot + r] = dn;
        accumulate_1d(M1, M2, dn, cur.v, cur.a, cur.b, omq);
      }
      double mean, var;
      close_replicate(M1, M2, nobs, mean_only, &mean, &var);
      om[r] = mean;
      ov[r] = var;
      r++;
      if (r < num_boot) {
        cur = load_bin(rec);                                     // in flight until the lane starts its next replicate (next pass)
        nxt = load_bin(rec + 8);
        state = LS_RESTART;
      } else {
        state = LS_IDLE;
      }
    }
    // ---- the draw of bin k, phase by phase (csrc/npy_rng.h) ------------------------------------------------------------------
    if (FAST) {
      // start + inversion segment + BTPE attempt in one straight line for every lane (csrc/npy_rng.h: the branch-free forms):
      // the independent dependency chains interleave instead of queueing behind three branches
      int32_t s0 = lane_begin_bf(D, g, cur.pk, cur.lq, dn > 0 ? dn : 1, state == LS_START);
      state = state == LS_START ? s0 : state;
      state = lane_inv_att_bf(D, g, state);
      if (state == LS_ATT2) state = lane_att_rest(D);
    } else if (state == LS_START) {                              // mm_debug_replay_arith(1): numpy's arithmetic, draw by draw
      D.w = binomial_pre<int32_t, false>(g, cur.pk, cur.lq, dn);
      state = LS_DONE;
    }
    if (state == LS_EXPL) state = lane_expl(D);
    // the rarer phases do not run on every pass: a lane in one of them waits a pass or a few, every other lane saves the time
    // (squeeze / Stirling: ~3 % of the lanes, every second pass; the exact redo: ~0.3 % of the draws, every 32nd pass)
    if ((passes & 1) == 0) {
      if (state == LS_SQZ) state = lane_sqz(D);
    }
    if ((passes & 31) == 0) {
      if (state == LS_XINV) state = lane_xinv(D, g);
      if (state == LS_XBT) state = lane_xbt(D, g);
    }
  }
  if (wave_clock && mm_lane() == 0) {
    int64_t wave = slot >> 6;
    wave_clock[wave * 4 + 0] = t_start;
    wave_clock[wave * 4 + 1] = (int64_t)wall_clock64();
    wave_clock[wave * 4 + 2] = passes;
    wave_clock[wave * 4 + 3] = 0;
  }
}

// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t mix64(uint64_t x) {  // splitmix64 finaliser (counter-based fill RNG)
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// rng='fast' (k_boot1d_fast, k_boot2d_fast): the PCG64 stream that replicate r of the chain with key ``key`` owns
__device__ __forceinline__ npyrng::Pcg64 fast_stream(uint64_t seed, uint64_t key, int r) {
  uint64_t h = mix64(seed ^ mix64(key * 0x100000001B3ull + (uint64_t)r));
  return npyrng::Pcg64{mix64(h), mix64(h + 1), mix64(h + 2), mix64(h + 3) | 1ull};
}

// counter of the refill draws of replicate r in plane ``which`` (0 mean, 1 res_var) of the row with key ``key``
__device__ __forceinline__ uint64_t fill_ctr(uint64_t seed, uint64_t key, int which, int r) {
  return mix64(seed ^ mix64(key * 2 + which) ^ ((uint64_t)r << 20));
}

// One wave per row.  Pass 1: res_var, validity, counts.  Pass 2 (fill_mode 0): each invalid entry takes
// a uniformly chosen VALID replicate (stored negated so later readers still see it as "not original"): up to FILL_ATTEMPTS
// rejection draws per lane, then, for what those left (rows with very few valid replicates), the wave resolves the entries
// one at a time: rank = hash mod V, found by a ballot / popcount scan over the row.  Valid entries are never written in pass 2,
// so the scan races with nothing.  The draw rule is part of the C-ABI contract (include/memento_hip.h).  Pass 3: log.
#define FILL_ATTEMPTS 4096
__global__ __launch_bounds__(256) void k_boot_fill_log(double *__restrict__ mean, double *__restrict__ var, int64_t n_rows,
                                                       int64_t ld, int32_t num_boot, double f0, double f1, double f2,
                                                       int32_t fill_mode, uint64_t seed, int32_t *__restrict__ n_invalid,
                                                       const int64_t *__restrict__ row_key) {
  int lane = mm_lane();
  int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (row >= n_rows) return;
  // the refill draws of a row are a function of (seed, key of the row, replicate): with the caller's keys (gene position in the
  // unsharded gene order x groups + group) they do not depend on how the genes were chunked or sharded over GPUs
  const uint64_t key = row_key ? (uint64_t)row_key[row] : (uint64_t)row;
  double *m = mean + row * ld + 1;
  double *s = var + row * ld + 1;
  int bad_m = 0, bad_v = 0;
  for (int r = lane; r < num_boot; r += 64) {
    double mm = m[r], vv = s[r];
    double rv = NAN;
    if (mm > 0.0 && vv > 0.0) {
      double lm = log(mm);
      double pred = ((0.0 * lm + f0) * lm + f1) * lm + f2;  // np.poly1d Horner order
      rv = exp(log(vv) - pred);
    }
    if (!(mm > 0.0)) {
      m[r] = NAN;
      bad_m++;
    }
    if (!(rv > 0.0)) {
      rv = NAN;
      bad_v++;
    }
    s[r] = rv;
  }
  for (int off = 32; off > 0; off >>= 1) {
    bad_m += __shfl_xor(bad_m, off, 64);
    bad_v += __shfl_xor(bad_v, off, 64);
  }
  bool none_m = bad_m == num_boot, none_v = bad_v == num_boot;
  if (lane == 0) {
    n_invalid[row * 2] = none_m ? -1 : bad_m;
    n_invalid[row * 2 + 1] = none_v ? -1 : bad_v;
  }
  __threadfence_block();
  if (fill_mode == 0) {
    for (int which = 0; which < 2; which++) {
      double *x = which ? s : m;
      int nb = which ? bad_v : bad_m;
      if (nb == 0 || nb == num_boot) continue;
      bool left = false;
      for (int r = lane; r < num_boot; r += 64) {
        double cur = x[r];
        if (!(cur > 0.0) && !(cur < 0.0)) {  // NaN => invalid and not yet filled
          uint64_t ctr = fill_ctr(seed, key, which, r);
          double pick = NAN;
          for (int attempt = 0; attempt < FILL_ATTEMPTS; attempt++) {
            ctr = mix64(ctr + attempt);
            int idx = (int)(ctr % (uint64_t)num_boot);
            double c = x[idx];
            if (c > 0.0) {
              pick = c;
              break;
            }
          }
          x[r] = -pick;
          left = left || !(pick > 0.0);
        }
      }
      __threadfence_block();
      if (!__any(left)) continue;
      // the entries the rejection draws left NaN (probability (1 - V / num_boot)^FILL_ATTEMPTS each, V = valid replicates): the
      // whole wave takes them in ascending order and gives each the rank-th valid entry of the row, rank = hash mod V
      const uint64_t n_ok = (uint64_t)(num_boot - nb);
      for (int r0 = 0; r0 < num_boot; r0 += 64) {
        double cur = r0 + lane < num_boot ? x[r0 + lane] : 1.0;
        uint64_t todo = __ballot(!(cur > 0.0) && !(cur < 0.0));
        while (todo) {
          int r = r0 + __ffsll((unsigned long long)todo) - 1;
          todo &= todo - 1;
          uint64_t rank = mix64(~fill_ctr(seed, key, which, r)) % n_ok;
          for (int c0 = 0; c0 < num_boot; c0 += 64) {
            double c = c0 + lane < num_boot ? x[c0 + lane] : NAN;
            uint64_t bal = __ballot(c > 0.0);
            uint64_t cnt = (uint64_t)__popcll(bal);
            if (rank < cnt) {
              if (c > 0.0 && (uint64_t)__popcll(bal & ((1ull << lane) - 1ull)) == rank) x[r] = -c;
              break;
            }
            rank -= cnt;
          }
        }
      }
      __threadfence_block();
    }
  }
  for (int r = lane; r < num_boot; r += 64) {
    double mm = m[r], vv = s[r];
    m[r] = log(fabs(mm));  // NaN stays NaN; filled entries were stored negated
    s[r] = log(fabs(vv));
  }
}

// ------------------------------------------------------------------------------------------------
// FAST mode (rng='fast'): the same multinomial chain and replicate moments, but one lane = one REPLICATE and
// one wave = 64 replicates of ONE (gene, group) pair.  Every lane of a wave walks the same bins, so the
// operands are wave-uniform, lanes take the same sampler (inversion or BTPE) at each step, and pairs x
// replicates give the chip millions of independent chains.  Replicate r of the chain with key ``slot_key[slot]`` owns the
// PCG64 stream derived from (seed, key, r) (fast_stream) -- NOT the reference's single stream: results are statistically equivalent
// to the reference, and draw for draw numpy's multinomial on that stream (tests/_fast_ref.py).  The caller's keys number the
// (gene, group) chains independently of gene chunking, of sharding and of the tile layout, so none of them changes a result;
// ``slot_row`` addresses the output row only.  The launch covers the ``num_boot`` replicates from global replicate ``rep_lo`` on
// (mm_boot1d_fast: rep_lo = 0): local replicate i draws from the stream of replicate rep_lo + i and is stored in column 1 + i, so a
// later launch on [rep_lo, rep_lo + n) continues a chain with the replicates a one-shot run would have made.  Lanes beyond
// num_boot walk along and store nothing.
// w_dump (optional): int32 weights [slot][k < kmax_dump][i < num_boot].
__global__ __launch_bounds__(256) void k_boot1d_fast(const double *__restrict__ pk_, const double *__restrict__ lq_,
                                                     const double *__restrict__ v, const double *__restrict__ a,
                                                     const double *__restrict__ b, const int64_t *__restrict__ tile_ptr,
                                                     int64_t n_slots, const int32_t *__restrict__ slot_K,
                                                     const double *__restrict__ slot_nobs, const double *__restrict__ slot_omq,
                                                     const int64_t *__restrict__ slot_row, const int64_t *__restrict__ slot_key,
                                                     uint64_t seed, int32_t rep_lo, int32_t num_boot, int32_t mean_only, int32_t chunks,
                                                     int64_t ld, double *__restrict__ out_mean, double *__restrict__ out_var,
                                                     int32_t *__restrict__ w_dump, int32_t kmax_dump) {
  int lane = mm_lane();
  // (a grid dimension holds fewer than 2^32 threads: the blocks beyond FAST_GRID_X go to gridDim.y)
  int64_t wid = (((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  int64_t slot = wid / chunks;
  int chunk = (int)(wid % chunks);
  if (slot >= n_slots) return;
  int K = slot_K[slot];
  int64_t row = slot_row[slot];
  if (K < 2 || row < 0) return;  // K == 1 rows stay NaN (bootstrap.py:97-98)
  int r = chunk * 64 + lane;
  bool mine = r < num_boot;
  int64_t obase = tile_ptr[slot >> 6] * 64 + (slot & 63);
  double nobs = slot_nobs[slot], omq = slot_omq[slot];
  int32_t n = (int32_t)nobs;
  // global replicate; unsigned, as only a lane beyond num_boot (it stores nothing) can pass 2^31 - 1
  npyrng::Pcg64 g = fast_stream(seed, (uint64_t)slot_key[slot], (int)((uint32_t)rep_lo + (uint32_t)r));
  int32_t *wd = (w_dump && mine) ? w_dump + (slot * kmax_dump) * (int64_t)num_boot + r : nullptr;
  double M1 = 0.0, M2 = 0.0;
  int32_t dn = n;
  for (int k = 0; k < K; k++) {
    int64_t o = obase + (int64_t)k * 64;   // wave-uniform address: one broadcast load
    int32_t w;
    if (k < K - 1) {
      w = dn > 0 ? npyrng::binomial_pre<int32_t, true>(g, pk_[o], lq_[o], dn) : 0;
      dn -= w;
    } else {
      w = dn > 0 ? dn : 0;
    }
    if (wd && k < kmax_dump) wd[(int64_t)k * num_boot] = w;
    accumulate_1d(M1, M2, w, v[o], a[o], b[o], omq);
  }
  if (mine) {
    double mean, var;
    close_replicate(M1, M2, nobs, mean_only, &mean, &var);
    out_mean[row * ld + 1 + r] = mean;
    out_var[row * ld + 1 + r] = var;
  }
}

// ------------------------------------------------------------------------------------------------
// FREE-RUNNING tile kernel: one lane = one chain, the lanes of a wave share the instruction stream and nothing else.  The lane, the
// draw of a bin (BOOT_BTPE_CAP attempt(s) per bin step, a rejected lane retries in the next step) and the replicate statistic are the
// shared parts above k_boot1d_replay (tile_lane, draw_bin, Stat1D); the loop is this kernel's own: a
// lane that finishes a replicate starts its next one at once instead of waiting for the slowest lane of its wave (in-kernel stamps of
// k_boot1d_replay: a 64-wide tile makes 1.23 bin steps per nominal step, 1.095 is the lanes' average), so every lane carries its own
// replicate index as well.  The lanes drift apart without bound, and operand ROWS shared by the wave (one coalesced 512-B row per plane
// and step) would turn into 64 separate lines per plane: the operands are therefore the chain's own 8-double RECORDS (mm_bins_order,
// MM_CHAIN_SLOT: pk, lq, count, 1/sf, 1/sf^2, one 64-B half line per bin, the form chain_body reads), fetched one bin ahead.
// Same samplers, same arithmetic per draw, same accumulation order per replicate: the replicate moments are those of
// k_boot1d_replay bit for bit.  A tile flagged in ca.tile_chain is a chain of the one-wave-per-chain form, as there.
template <int MINW, bool FAST>
__global__ __launch_bounds__(256, MINW) void k_boot1d_free(const double *__restrict__ recs, const int64_t *__restrict__ slot_rec,
                                                           int64_t n_tiles, const int32_t *__restrict__ slot_K,
                                                           const double *__restrict__ slot_nobs, const double *__restrict__ slot_omq,
                                                           const int64_t *__restrict__ slot_row, uint64_t st0, uint64_t st1, uint64_t st2,
                                                           uint64_t st3, int32_t num_boot, int32_t mean_only, int64_t ld,
                                                           double *__restrict__ out_mean, double *__restrict__ out_var,
                                                           int32_t *__restrict__ w_dump, int32_t kmax_dump,
                                                           int64_t *__restrict__ wave_clock, ChainArgs ca) {
  int lane = mm_lane();
  int64_t tile = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (tile >= n_tiles) return;
  if (run_tile_as_chain<FAST>(ca, tile, n_tiles, lane, st0, st1, num_boot, mean_only, ld, out_mean, out_var, wave_clock)) return;
  int64_t t_start = wave_clock ? (int64_t)wall_clock64() : 0;
  const TileLane t = tile_lane<true>(tile, n_tiles, lane, slot_K, slot_nobs, slot_omq, slot_row, slot_rec);
  const int K = t.K;
  Stat1D stat{t, num_boot, mean_only, t.out(out_mean, ld), t.out(out_var, ld), w_dump, kmax_dump};
  stat.short_chain();
  npyrng::Pcg64 g{st0, st1, st2, st3};
  bool more = K >= Stat1D::MIN_K;           // this lane still has replicates to draw
  const Records1D ops{recs + (more ? t.rec : 0) * 8};
  int rl = 0, kl = 0;                       // its replicate and its bin
  stat.begin();
  int32_t dn = t.n;
  bool live = true;
  Ops1D c = ops.load(0);
  int64_t steps = 0;
  for (;;) {
    const bool act = more;
    const uint64_t act_mask = __ballot(more);
    if (act_mask == 0) break;
    steps++;
    const int cap = (BOOT_BTPE_CAP > 0 && __popcll(act_mask) > BOOT_TAIL_LANES) ? BOOT_BTPE_CAP : 0;
    const Ops1D nx = ops.load(kl + 1 < K ? kl + 1 : 0);
    if (act) {
      const BinDraw d = draw_bin<FAST>(g, c.pk, c.lq, dn, live, kl >= K - 1, cap);
      dn = d.dn;
      live = d.live;
      if (!d.pending) {
        stat.dump(kl, rl, d.w);
        if (d.w != 0) stat.add(d.w, c);
        kl++;
        c = nx;
        if (kl == K) {                       // the replicate is complete (the operands just taken over are bin 0's again)
          stat.close(rl);
          rl++;
          kl = 0;
          stat.begin();
          dn = t.n;
          live = true;
          more = rl < num_boot;
        }
      }
    }
  }
  if (wave_clock && lane == 0) {  // profiling hook (mm_debug_wave_clock): when this wave ran, how many bin steps it made
    wave_clock[tile * 4 + 0] = t_start;
    wave_clock[tile * 4 + 1] = (int64_t)wall_clock64();
    wave_clock[tile * 4 + 2] = steps;
    wave_clock[tile * 4 + 3] = (int64_t)__builtin_amdgcn_s_getreg((31 << 11) | 20);   // HW_REG_XCC_ID
  }
}

// ------------------------------------------------------------------------------------------------
// 2D replay: same multinomial chain over the (x_i, x_j, sf_bin) bins of a gene pair; per replicate the
// covariance and the two variances (bootstrap.py:141-155, estimator.py:214-218, :171-174) are folded
// into the correlation exactly as estimator._corr_from_cov does (:281-292: 5.0 sentinel where a variance
// is <= 0, then clip to [-1, 1]).  Writes corr_b to out[row*ld + 1 + b].
#ifndef BOOT2D_BTPE_CAP
#define BOOT2D_BTPE_CAP 0
#endif
// One bin's share of a replicate's five sums and the replicate's correlation from them.  Both 2D kernels below add their bins in chain
// order through these two (the association of every product is numpy's), as the 1D kernels do through accumulate_1d / close_replicate.
struct Sums2D {
  double A1 = 0.0, A2 = 0.0, MX = 0.0, Q1 = 0.0, Q2 = 0.0;
};
__device__ __forceinline__ void accumulate_2d(Sums2D &s, int32_t w, double x1, double x2, double aa, double bb, double omq) {
  double wd = (double)w;
  s.A1 += (x1 * wd) * aa;
  s.A2 += (x2 * wd) * aa;
  s.MX += ((x1 * x2) * wd) * bb;
  s.Q1 += ((x1 * x1) * wd) * bb - ((omq * x1) * wd) * bb;
  s.Q2 += ((x2 * x2) * wd) * bb - ((omq * x2) * wd) * bb;
}
__device__ __forceinline__ double close_replicate_2d(const Sums2D &s, double nobs) {
  double m1 = s.A1 / nobs, m2 = s.A2 / nobs;
  double cov = s.MX / nobs - m1 * m2;
  double var1 = s.Q1 / nobs - m1 * m1;
  double var2 = s.Q2 / nobs - m2 * m2;
  double corr = 5.0;       // estimator._corr_from_cov: the sentinel where a variance is <= 0, clipped below like any other value
  if (var1 > 0.0 && var2 > 0.0) {
    double vp = sqrt(var1 * var2);
    if (isfinite(vp)) corr = cov / vp;
  }
  if (corr > 1.0) corr = 1.0;
  if (corr < -1.0) corr = -1.0;
  return corr;
}
#ifndef BOOT2D_REC_BTPE_CAP
#define BOOT2D_REC_BTPE_CAP 1    // attempts per bin step when the chains read their own operand records (REC): no shared rows to scatter
#endif
// A 2D bin's operands in the two layouts (the 1D forms: Ops1D, Planes1D, Records1D).
struct Ops2D { double pk, lq, x1, x2, a, b; };
struct Planes2D {
  const double *__restrict__ pk, *__restrict__ lq, *__restrict__ x1, *__restrict__ x2, *__restrict__ a, *__restrict__ b;
  int64_t obase;   // first row of the tile * 64 + lane
  __device__ __forceinline__ Ops2D load(int k) const {
    int64_t o = obase + (int64_t)k * 64;
    return Ops2D{pk[o], lq[o], x1[o], x2[o], a[o], b[o]};
  }
};
struct Records2D {
  const double *__restrict__ rec;   // [K][8]: pk, lq, x_i, x_j, 1/sf, 1/sf^2, (2 spare)
  __device__ __forceinline__ Ops2D load(int k) const {
    const double *p = rec + (int64_t)k * 8;
    double2 t0 = *(const double2 *)(p), t1 = *(const double2 *)(p + 2), t2 = *(const double2 *)(p + 4);
    return Ops2D{t0.x, t0.y, t1.x, t1.y, t2.x, t2.y};
  }
};
// The replicate statistic of a 2D chain: the five sums, closed into the replicate's cell of the one output row.  Every chain with a
// bin runs (K == 1: every replicate is the observed sample); there is no weight dump.
struct Stat2D {
  static constexpr int MIN_K = 1;
  const TileLane &t;
  double *oc;   // t.out() of the plane
  Sums2D sums;
  __device__ __forceinline__ void short_chain() {}
  __device__ __forceinline__ void begin() { sums = Sums2D(); }
  __device__ __forceinline__ void dump(int, int, int32_t) {}
  __device__ __forceinline__ void add(int32_t w, const Ops2D &c) { accumulate_2d(sums, w, c.x1, c.x2, c.a, c.b, t.omq); }
  __device__ __forceinline__ void close(int r) { oc[r] = close_replicate_2d(sums, t.nobs); }
};
// The lock-step body (tile_lockstep) with Stat2D.  REC: pk_ is the record buffer and the lane's chain starts at record slot_rec[slot];
// otherwise six [row][64] planes, the tile's rows from tile_ptr[tile].  BOOT2D_BTPE_CAP is 0: measured on configs[3]'s share (250 x 2000
// pairs, 335 bins per chain on average, 64-wide tiles in several rounds) one attempt per step takes 29.2 s against 16.8 s: the steps of
// this kernel are short (small inversion searches), and lanes that fall behind by different amounts turn the six coalesced 512-B operand
// rows of a step into up to 64 separate lines each.  (The load one bin ahead: the longest pair runs alone in its wave.)
template <int MINW, bool FAST, bool REC>
__global__ __launch_bounds__(256, MINW) void k_boot2d_replay(const double *__restrict__ pk_, const double *__restrict__ lq_,
                                                       const double *__restrict__ v1_, const double *__restrict__ v2_,
                                                       const double *__restrict__ a, const double *__restrict__ b,
                                                       const int64_t *__restrict__ tile_ptr, int64_t n_tiles,
                                                       const int32_t *__restrict__ slot_K, const double *__restrict__ slot_nobs,
                                                       const double *__restrict__ slot_omq, const int64_t *__restrict__ slot_row,
                                                       uint64_t st0, uint64_t st1, uint64_t st2, uint64_t st3, int32_t num_boot,
                                                       int64_t ld, double *__restrict__ out_corr, const int64_t *__restrict__ slot_rec) {
  int lane = mm_lane();
  int64_t tile = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (tile >= n_tiles) return;
  const TileLane t = tile_lane<REC>(tile, n_tiles, lane, slot_K, slot_nobs, slot_omq, slot_row, slot_rec);
  Stat2D stat{t, t.out(out_corr, ld)};
  if constexpr (REC) {
    const Records2D ops{pk_ + (t.K >= Stat2D::MIN_K ? t.rec : 0) * 8};
    tile_lockstep<FAST, BOOT2D_REC_BTPE_CAP>(t, st0, st1, st2, st3, num_boot, stat, ops);
  } else {
    const Planes2D ops{pk_, lq_, v1_, v2_, a, b, tile_ptr[tile] * 64 + lane};
    tile_lockstep<FAST, BOOT2D_BTPE_CAP>(t, st0, st1, st2, st3, num_boot, stat, ops);
  }
}

// ------------------------------------------------------------------------------------------------
// 2D FAST mode (rng='fast'): k_boot1d_fast's decomposition with k_boot2d_replay's arithmetic.  One lane = one REPLICATE, one wave
// = 64 replicates of ONE (pair, group) chain: wave wid = slot * chunks + chunk draws the local replicates chunk * 64 + lane.  The
// address of bin k in the six [row][64] planes is wave-uniform (one broadcast load per operand and step, fetched one bin ahead); the
// lanes hold different remainders, so they may take different samplers at a step.  A chain's critical path is its K draws instead of
// K x B, and the launch has chains x ceil(B / 64) independent waves.  Replicate r of the chain with key ``slot_key[slot]`` owns the
// PCG64 stream derived from (seed, key, r) -- the caller's keys number the (pair, group) chains independently of chunking, of the
// order the pairs are in and of the tile layout, so neither changes a result.  The launch covers the ``num_boot`` replicates from
// global replicate ``rep_lo`` on (mm_boot2d_fast: rep_lo = 0): local replicate i draws from the stream of replicate rep_lo + i and is
// stored in column 1 + i, so a later launch on [rep_lo, rep_lo + n) continues a chain with the replicates a one-shot run would have
// made.  Chains with K >= 1 run (K == 1: every replicate is the observed sample, as in the replay kernel); K <= 0 or row < 0 writes
// nothing.  Lanes beyond num_boot walk along and store nothing.  The grid is one row of blocks up to FAST_GRID_X of them and rows
// of FAST_GRID_X blocks in gridDim.y beyond (mm_boot2d_fast_range); the waves behind the last slot return at once.
// w_dump (optional): int32 weights [slot][k < kmax_dump][i < num_boot].
//
// LISTED (k_boot2d_fast_slots, mm_boot2d_fast_slots): the launch covers the ``n_list`` slots of ``slot_list`` instead of the whole
// tile layout -- wave wid takes slot_list[wid / chunks] -- and everything from there on is the same body, so a listed slot gets bit
// for bit the replicates that the launch over the layout gives it.  The list is trusted (a slot outside the layout is passed over).
template <bool LISTED>
__device__ __forceinline__ void boot2d_fast_body(const double *__restrict__ pk_, const double *__restrict__ lq_,
                                                 const double *__restrict__ v1_, const double *__restrict__ v2_,
                                                 const double *__restrict__ a, const double *__restrict__ b,
                                                 const int64_t *__restrict__ tile_ptr, int64_t n_slots,
                                                 const int32_t *__restrict__ slot_K, const double *__restrict__ slot_nobs,
                                                 const double *__restrict__ slot_omq, const int64_t *__restrict__ slot_row,
                                                 const int64_t *__restrict__ slot_key, uint64_t seed, int32_t rep_lo,
                                                 int32_t num_boot, int32_t chunks, int64_t ld, double *__restrict__ out_corr,
                                                 int32_t *__restrict__ w_dump, int32_t kmax_dump,
                                                 const int64_t *__restrict__ slot_list, int64_t n_list) {
  int lane = mm_lane();
  // (a grid dimension holds fewer than 2^32 threads: the blocks beyond FAST_GRID_X go to gridDim.y)
  int64_t wid = (((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
  int64_t slot = wid / chunks;
  int chunk = (int)(wid % chunks);
  if (LISTED) {
    if (slot >= n_list) return;
    slot = slot_list[slot];
    if (slot < 0) return;
  }
  if (slot >= n_slots) return;
  int K = slot_K[slot];
  int64_t row = slot_row[slot];
  if (K <= 0 || row < 0) return;
  int r = chunk * 64 + lane;
  bool mine = r < num_boot;
  int64_t obase = tile_ptr[slot >> 6] * 64 + (slot & 63);
  double nobs = slot_nobs[slot], omq = slot_omq[slot];
  // global replicate; unsigned, as only a lane beyond num_boot (it stores nothing) can pass 2^31 - 1
  npyrng::Pcg64 g = fast_stream(seed, (uint64_t)slot_key[slot], (int)((uint32_t)rep_lo + (uint32_t)r));
  int32_t *wd = (w_dump && mine) ? w_dump + (slot * kmax_dump) * (int64_t)num_boot + r : nullptr;
  Sums2D sums;
  int32_t dn = (int32_t)nobs;  // N_g < 2^31 (checked by the host)
  double c_pk = pk_[obase], c_lq = lq_[obase], c_x1 = v1_[obase], c_x2 = v2_[obase], c_a = a[obase], c_b = b[obase];
  for (int k = 0; k < K; k++) {
    int64_t on = obase + (int64_t)(k + 1 < K ? k + 1 : 0) * 64;   // wave-uniform address of the next bin's operands
    double n_pk = pk_[on], n_lq = lq_[on], n_x1 = v1_[on], n_x2 = v2_[on], n_a = a[on], n_b = b[on];
    int32_t w;
    if (k < K - 1) {
      w = dn > 0 ? npyrng::binomial_pre<int32_t, true>(g, c_pk, c_lq, dn) : 0;
      dn -= w;
    } else {
      w = dn > 0 ? dn : 0;
    }
    if (wd && k < kmax_dump) wd[(int64_t)k * num_boot] = w;
    accumulate_2d(sums, w, c_x1, c_x2, c_a, c_b, omq);
    c_pk = n_pk; c_lq = n_lq; c_x1 = n_x1; c_x2 = n_x2; c_a = n_a; c_b = n_b;
  }
  if (mine) out_corr[row * ld + 1 + r] = close_replicate_2d(sums, nobs);
}

__global__ __launch_bounds__(256) void k_boot2d_fast(const double *__restrict__ pk_, const double *__restrict__ lq_,
                                                     const double *__restrict__ v1_, const double *__restrict__ v2_,
                                                     const double *__restrict__ a, const double *__restrict__ b,
                                                     const int64_t *__restrict__ tile_ptr, int64_t n_slots,
                                                     const int32_t *__restrict__ slot_K, const double *__restrict__ slot_nobs,
                                                     const double *__restrict__ slot_omq, const int64_t *__restrict__ slot_row,
                                                     const int64_t *__restrict__ slot_key, uint64_t seed, int32_t rep_lo,
                                                     int32_t num_boot, int32_t chunks, int64_t ld, double *__restrict__ out_corr,
                                                     int32_t *__restrict__ w_dump, int32_t kmax_dump) {
  boot2d_fast_body<false>(pk_, lq_, v1_, v2_, a, b, tile_ptr, n_slots, slot_K, slot_nobs, slot_omq, slot_row, slot_key, seed, rep_lo,
                          num_boot, chunks, ld, out_corr, w_dump, kmax_dump, nullptr, 0);
}

// The body over a list of slots, without a weight dump (mm_boot2d_fast_slots).
__global__ __launch_bounds__(256) void k_boot2d_fast_slots(const double *__restrict__ pk_, const double *__restrict__ lq_,
                                                           const double *__restrict__ v1_, const double *__restrict__ v2_,
                                                           const double *__restrict__ a, const double *__restrict__ b,
                                                           const int64_t *__restrict__ tile_ptr, int64_t n_slots,
                                                           const int32_t *__restrict__ slot_K, const double *__restrict__ slot_nobs,
                                                           const double *__restrict__ slot_omq, const int64_t *__restrict__ slot_row,
                                                           const int64_t *__restrict__ slot_key, uint64_t seed, int32_t rep_lo,
                                                           int32_t num_boot, int32_t chunks, int64_t ld, double *__restrict__ out_corr,
                                                           const int64_t *__restrict__ slot_list, int64_t n_list) {
  boot2d_fast_body<true>(pk_, lq_, v1_, v2_, a, b, tile_ptr, n_slots, slot_K, slot_nobs, slot_omq, slot_row, slot_key, seed, rep_lo,
                         num_boot, chunks, ld, out_corr, nullptr, 0, slot_list, n_list);
}

// mm_debug_inversion_ladder: the guarded fp32 inversion search of thread i's (U, n, p) through both forms of its ladder -- form 0 the
// nested ifs, form 1 the one-mask asm statement (csrc/npy_rng.h) -- inside a branch that only the lanes of ``lane_mask`` take, so the
// asm statement is entered with partial EXEC.  out[(form * 4 + f) * count + i], f = 0..3: the return value (X or -1), the steps
// taken, the bits of Uf and of px where the search stopped.  They are stored behind the call, inside the branch: a lane the
// statement failed to switch back on would leave its cells untouched.  marker[i] = i + 1 from every thread, masked or not.
__global__ __launch_bounds__(256) void k_debug_inversion_ladder(const double *__restrict__ U, const int32_t *__restrict__ n,
                                                                const double *__restrict__ p, int64_t count, uint64_t lane_mask,
                                                                int32_t *__restrict__ out, int32_t *__restrict__ marker) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  if ((lane_mask >> (threadIdx.x & 63)) & 1) {
    const double Ui = U[i], pi = p[i];
    const int32_t ni = n[i];
    const double lq = npyrng::binomial_lq(pi);
    npyrng::InversionStop st;
    int32_t ret = npyrng::binomial_inversion_fast<int32_t, true, true>(Ui, ni, pi, lq, &st);
    out[0 * count + i] = ret;
    out[1 * count + i] = st.steps;
    out[2 * count + i] = (int32_t)__float_as_uint(st.Uf);
    out[3 * count + i] = (int32_t)__float_as_uint(st.px);
    ret = npyrng::binomial_inversion_fast<int32_t, false, true>(Ui, ni, pi, lq, &st);
    out[4 * count + i] = ret;
    out[5 * count + i] = st.steps;
    out[6 * count + i] = (int32_t)__float_as_uint(st.Uf);
    out[7 * count + i] = (int32_t)__float_as_uint(st.px);
  }
  marker[i] = (int32_t)(i + 1);
}

static int64_t *g_wave_clock = nullptr;  // set by mm_debug_wave_clock; nullptr = no profiling writes
static int g_exact_arith = 0;            // set by mm_debug_replay_arith: 1 = numpy's fp64 arithmetic in every search loop (A/B timing, tests)

// The chains a tile launch takes along (``chains`` may be NULL: none) as the kernels' ChainArgs.
static int chain_args_of(const mm_chain_tiles *chains, ChainArgs *ca) {
  *ca = ChainArgs{};
  if (!chains) return MM_OK;
  MM_ARG(chains->d_tile_chain && chains->d_ops && chains->d_ch_base && chains->d_ch_K && chains->d_ch_nobs && chains->d_ch_omq &&
         chains->d_ch_row && chains->d_jump);
  *ca = ChainArgs{chains->d_ops, chains->d_ch_base, chains->d_ch_K, chains->d_ch_nobs, chains->d_ch_omq, chains->d_ch_row, chains->d_jump,
                  chains->d_tile_chain, chains->d_w_dump, chains->kmax_dump};
  return MM_OK;
}

// The instantiation of a tile kernel for one launch.  ``three``: the 168-VGPR build (three waves per SIMD) instead of the
// BOOT_MIN_WAVES one; FAST is off under mm_debug_replay_arith(1).  ``pick(minw, fast)`` names the kernel: both arguments are
// std::integral_constant values (``minw()`` is a constant expression), every instantiation of one kernel has the same type.
template <typename Pick>
static auto tile_kernel(bool three, Pick pick) {
  std::integral_constant<int, 3> w3;
  std::integral_constant<int, BOOT_MIN_WAVES> w2;
  if (three) return g_exact_arith ? pick(w3, std::false_type()) : pick(w3, std::true_type());
  return g_exact_arith ? pick(w2, std::false_type()) : pick(w2, std::true_type());
}

// What the four tile entry points check alike (``ptrs``: every table, operand and output pointer of the entry point is there), and
// their grid (0: no tile, nothing to launch).  4 tiles per 256-thread workgroup: tiles t and t + 1024 (+-3) then meet on one SIMD,
// which engine.pair_tiles relies on (one tile per workgroup was measured too: worse when everything is resident, a wash otherwise).
static int tile_grid(bool ptrs, int64_t n_tiles, int32_t num_boot, int64_t ld, unsigned *blocks) {
  MM_ARG(ptrs && n_tiles >= 0 && n_tiles < 2147483647LL && num_boot > 0 && ld >= (int64_t)num_boot + 1);
  *blocks = (unsigned)((n_tiles + 3) / 4);
  return MM_OK;
}
extern "C" {

int mm_debug_wave_clock(int64_t *d_buf) {
  g_wave_clock = d_buf;
  return MM_OK;
}

int mm_debug_replay_arith(int32_t exact) {
  g_exact_arith = exact ? 1 : 0;
  return MM_OK;
}

int mm_debug_inversion_ladder(const double *d_U, const int32_t *d_n, const double *d_p, int64_t count, uint64_t lane_mask, int32_t *d_out,
                              int32_t *d_marker, void *stream) {
  MM_ARG(d_U && d_n && d_p && d_out && d_marker && count >= 0 && count < (1LL << 28));
  if (count == 0) return MM_OK;
  // exactly ``count`` threads while they fit one workgroup (a launch of 65 threads has a one-lane wave), 256-thread workgroups beyond
  const unsigned threads = count < 256 ? (unsigned)count : 256u;
  hipLaunchKernelGGL(k_debug_inversion_ladder, dim3((unsigned)((count + threads - 1) / threads)), dim3(threads), 0, (hipStream_t)stream,
                     d_U, d_n, d_p, count, lane_mask, d_out, d_marker);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_boot1d_replay(const double *d_pk, const double *d_lq, const double *d_v, const double *d_a, const double *d_b,
                     const int64_t *d_tile_ptr, int64_t n_tiles, const int32_t *d_slot_K, const double *d_slot_nobs,
                     const double *d_slot_omq, const int64_t *d_slot_row, const uint64_t pcg_state[4], int32_t num_boot,
                     int32_t mean_only, int64_t ld, double *d_out_mean, double *d_out_var, int32_t *d_w_dump, int32_t kmax_dump,
                     int64_t co_resident_waves, const mm_chain_tiles *chains, void *stream) {
  unsigned blocks;
  const bool ptrs = d_pk && d_lq && d_v && d_a && d_b && d_tile_ptr && d_slot_K && d_slot_nobs && d_slot_omq && d_slot_row && pcg_state;
  if (int rc = tile_grid(ptrs && d_out_mean && d_out_var, n_tiles, num_boot, ld, &blocks)) return rc;
  ChainArgs ca;
  if (int rc = chain_args_of(chains, &ca)) return rc;
  if (blocks == 0) return MM_OK;
  // the 168-VGPR build (three waves per SIMD) when this launch and the chain-kernel waves running beside it need more than two
  // wave slots per SIMD; the two-wave build otherwise
  const bool three = n_tiles + (co_resident_waves > 0 ? co_resident_waves : 0) > 2048;
  auto kern = tile_kernel(three, [](auto minw, auto fast) { return &k_boot1d_replay<minw(), fast()>; });
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, (hipStream_t)stream, d_pk, d_lq, d_v, d_a, d_b,
                     d_tile_ptr, n_tiles, d_slot_K, d_slot_nobs, d_slot_omq, d_slot_row, pcg_state[0], pcg_state[1], pcg_state[2],
                     pcg_state[3], num_boot, mean_only, ld, d_out_mean, d_out_var, d_w_dump, kmax_dump, g_wave_clock, ca);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_boot1d_free(const double *d_recs, const int64_t *d_slot_rec, int64_t n_tiles, const int32_t *d_slot_K, const double *d_slot_nobs,
                   const double *d_slot_omq, const int64_t *d_slot_row, const uint64_t pcg_state[4], int32_t num_boot, int32_t mean_only,
                   int64_t ld, double *d_out_mean, double *d_out_var, int32_t *d_w_dump, int32_t kmax_dump, const mm_chain_tiles *chains,
                   void *stream) {
  unsigned blocks;
  const bool ptrs = d_recs && d_slot_rec && d_slot_K && d_slot_nobs && d_slot_omq && d_slot_row && pcg_state;
  if (int rc = tile_grid(ptrs && d_out_mean && d_out_var, n_tiles, num_boot, ld, &blocks)) return rc;
  ChainArgs ca;
  if (int rc = chain_args_of(chains, &ca)) return rc;
  if (blocks == 0) return MM_OK;
  // the register budgets of mm_boot1d_replay: three waves per SIMD beyond 2,048 tiles
  auto kern = tile_kernel(n_tiles > 2048, [](auto minw, auto fast) { return &k_boot1d_free<minw(), fast()>; });
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, (hipStream_t)stream, d_recs, d_slot_rec, n_tiles, d_slot_K,
                     d_slot_nobs, d_slot_omq, d_slot_row, pcg_state[0], pcg_state[1], pcg_state[2], pcg_state[3], num_boot, mean_only, ld,
                     d_out_mean, d_out_var, d_w_dump, kmax_dump, g_wave_clock, ca);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_pcg64_stream(const uint64_t pcg_state[4], int64_t n, double *d_out, void *stream) {
  MM_ARG(pcg_state && d_out && n >= 0);
  if (n == 0) return MM_OK;
  int64_t threads = (n + 63) / 64;
  hipLaunchKernelGGL(k_pcg64_stream, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_out, n, pcg_state[0],
                     pcg_state[1], pcg_state[2], pcg_state[3]);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_boot1d_chain(const double *d_ops, const int64_t *d_ch_base, const int32_t *d_ch_K, const double *d_ch_nobs,
                    const double *d_ch_omq, const int64_t *d_ch_row, int64_t n_chains, const uint64_t *d_jump,
                    const uint64_t pcg_state[4], int32_t num_boot, int32_t mean_only, int64_t ld, double *d_out_mean,
                    double *d_out_var, int32_t *d_w_dump, int32_t kmax_dump, void *stream) {
  MM_ARG(d_ops && d_ch_base && d_ch_K && d_ch_nobs && d_ch_omq && d_ch_row && d_jump && pcg_state && d_out_mean && d_out_var);
  MM_ARG(n_chains >= 0 && n_chains < 2147483647LL && num_boot > 0 && ld >= (int64_t)num_boot + 1);
  if (n_chains == 0) return MM_OK;
  auto kern = g_exact_arith ? k_boot1d_chain<false> : k_boot1d_chain<true>;
  ChainArgs ca{d_ops, d_ch_base, d_ch_K, d_ch_nobs, d_ch_omq, d_ch_row, d_jump, nullptr, d_w_dump, kmax_dump};
  hipLaunchKernelGGL(kern, dim3((unsigned)((n_chains + 3) / 4)), dim3(256), 0, (hipStream_t)stream, ca, n_chains, pcg_state[0], pcg_state[1],
                     num_boot, mean_only, ld, d_out_mean, d_out_var, g_wave_clock ? g_wave_clock + MM_CHAIN_CLOCK_OFF : nullptr);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_boot1d_async(const double *d_ops, const int64_t *d_ch_base, const int32_t *d_ch_K, const double *d_ch_nobs,
                    const double *d_ch_omq, const int64_t *d_ch_row, int64_t n_slots, const uint64_t pcg_state[4], int32_t num_boot,
                    int32_t mean_only, int64_t ld, double *d_out_mean, double *d_out_var, int32_t *d_w_dump, int32_t kmax_dump,
                    void *stream) {
  MM_ARG(d_ops && d_ch_base && d_ch_K && d_ch_nobs && d_ch_omq && d_ch_row && pcg_state && d_out_mean && d_out_var);
  MM_ARG(n_slots >= 0 && n_slots < (1LL << 38) && num_boot > 0 && ld >= (int64_t)num_boot + 1);
  if (n_slots == 0) return MM_OK;
  auto kern = g_exact_arith ? k_boot1d_async<false> : k_boot1d_async<true>;
  hipLaunchKernelGGL(kern, dim3((unsigned)((n_slots + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_ops, d_ch_base, d_ch_K, d_ch_nobs,
                     d_ch_omq, d_ch_row, n_slots, pcg_state[0], pcg_state[1], pcg_state[2], pcg_state[3], num_boot, mean_only, ld,
                     d_out_mean, d_out_var, d_w_dump, kmax_dump, g_wave_clock);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_boot_fill_log(double *d_mean, double *d_var, int64_t n_rows, int64_t ld, int32_t num_boot, const double mv_fit[3],
                     int32_t fill_mode, uint64_t fill_seed, int32_t *d_n_invalid, const int64_t *d_row_key, void *stream) {
  MM_ARG(d_mean && d_var && mv_fit && d_n_invalid && n_rows >= 0 && num_boot > 0 && ld >= (int64_t)num_boot + 1);
  MM_ARG(fill_mode == 0 || fill_mode == 1);
  if (n_rows == 0) return MM_OK;
  int64_t blocks = (n_rows + 3) / 4;
  hipLaunchKernelGGL(k_boot_fill_log, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d_mean, d_var, n_rows, ld, num_boot,
                     mv_fit[0], mv_fit[1], mv_fit[2], fill_mode, fill_seed, d_n_invalid, d_row_key);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_boot2d_replay(const double *d_pk, const double *d_lq, const double *d_v1, const double *d_v2, const double *d_a,
                     const double *d_b, const int64_t *d_tile_ptr, int64_t n_tiles, const int32_t *d_slot_K,
                     const double *d_slot_nobs, const double *d_slot_omq, const int64_t *d_slot_row, const uint64_t pcg_state[4],
                     int32_t num_boot, int64_t ld, double *d_out_corr, void *stream) {
  unsigned blocks;
  const bool ptrs = d_pk && d_lq && d_v1 && d_v2 && d_a && d_b && d_tile_ptr && d_slot_K && d_slot_nobs && d_slot_omq && d_slot_row && pcg_state;
  if (int rc = tile_grid(ptrs && d_out_corr, n_tiles, num_boot, ld, &blocks)) return rc;
  if (blocks == 0) return MM_OK;
  auto kern = tile_kernel(n_tiles > 2048, [](auto minw, auto fast) { return &k_boot2d_replay<minw(), fast(), false>; });
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, (hipStream_t)stream, d_pk, d_lq, d_v1, d_v2, d_a, d_b,
                     d_tile_ptr, n_tiles, d_slot_K, d_slot_nobs, d_slot_omq, d_slot_row, pcg_state[0], pcg_state[1], pcg_state[2],
                     pcg_state[3], num_boot, ld, d_out_corr, (const int64_t *)nullptr);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_boot2d_replay_rec(const double *d_recs, const int64_t *d_slot_rec, int64_t n_tiles, const int32_t *d_slot_K,
                         const double *d_slot_nobs, const double *d_slot_omq, const int64_t *d_slot_row, const uint64_t pcg_state[4],
                         int32_t num_boot, int64_t ld, double *d_out_corr, void *stream) {
  unsigned blocks;
  const bool ptrs = d_recs && d_slot_rec && d_slot_K && d_slot_nobs && d_slot_omq && d_slot_row && pcg_state;
  if (int rc = tile_grid(ptrs && d_out_corr, n_tiles, num_boot, ld, &blocks)) return rc;
  if (blocks == 0) return MM_OK;
  auto kern = tile_kernel(n_tiles > 2048, [](auto minw, auto fast) { return &k_boot2d_replay<minw(), fast(), true>; });
  const double *nul = nullptr;
  hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, (hipStream_t)stream, d_recs, nul, nul, nul, nul, nul,
                     (const int64_t *)nullptr, n_tiles, d_slot_K, d_slot_nobs, d_slot_omq, d_slot_row, pcg_state[0], pcg_state[1],
                     pcg_state[2], pcg_state[3], num_boot, ld, d_out_corr, d_slot_rec);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_boot2d_fast(const double *d_pk, const double *d_lq, const double *d_v1, const double *d_v2, const double *d_a,
                   const double *d_b, const int64_t *d_tile_ptr, int64_t n_slots, const int32_t *d_slot_K, const double *d_slot_nobs,
                   const double *d_slot_omq, const int64_t *d_slot_row, const int64_t *d_slot_key, uint64_t seed, int32_t num_boot,
                   int64_t ld, double *d_out_corr, int32_t *d_w_dump, int32_t kmax_dump, void *stream) {
  return mm_boot2d_fast_range(d_pk, d_lq, d_v1, d_v2, d_a, d_b, d_tile_ptr, n_slots, d_slot_K, d_slot_nobs, d_slot_omq, d_slot_row,
                              d_slot_key, seed, 0, num_boot, ld, d_out_corr, d_w_dump, kmax_dump, stream);
}

// The grid of the two rng='fast' kernels for ``blocks`` workgroups.  gridDim.x * 256 threads must stay below 2^32 (a larger launch
// runs only part of its blocks): up to FAST_GRID_X blocks the grid is one row, as it always was; beyond, rows of FAST_GRID_X
// blocks, the last one ragged (its surplus waves return at once).
static int fast_grid(int64_t blocks, dim3 *grid) {
  const int64_t FAST_GRID_X = 1 << 22;
  int64_t grid_x = blocks < FAST_GRID_X ? blocks : FAST_GRID_X, grid_y = (blocks + grid_x - 1) / grid_x;
  MM_ARG(grid_y <= 65535);
  *grid = dim3((unsigned)grid_x, (unsigned)grid_y);
  return MM_OK;
}

int mm_boot2d_fast_range(const double *d_pk, const double *d_lq, const double *d_v1, const double *d_v2, const double *d_a,
                         const double *d_b, const int64_t *d_tile_ptr, int64_t n_slots, const int32_t *d_slot_K,
                         const double *d_slot_nobs, const double *d_slot_omq, const int64_t *d_slot_row, const int64_t *d_slot_key,
                         uint64_t seed, int32_t rep_lo, int32_t rep_n, int64_t ld, double *d_out_corr, int32_t *d_w_dump,
                         int32_t kmax_dump, void *stream) {
  MM_ARG(d_pk && d_lq && d_v1 && d_v2 && d_a && d_b && d_tile_ptr && d_slot_K && d_slot_nobs && d_slot_omq && d_slot_row && d_slot_key);
  MM_ARG(d_out_corr && n_slots >= 0 && n_slots % 64 == 0 && rep_n > 0 && ld >= (int64_t)rep_n + 1);
  MM_ARG(rep_lo >= 0 && (int64_t)rep_lo + rep_n <= 2147483647LL);
  MM_ARG(!d_w_dump || kmax_dump > 0);
  if (n_slots == 0) return MM_OK;
  int32_t chunks = (int32_t)(((int64_t)rep_n + 63) / 64);
  int64_t waves = n_slots * chunks;
  dim3 grid;
  if (int rc = fast_grid((waves + 3) / 4, &grid)) return rc;
  hipLaunchKernelGGL(k_boot2d_fast, grid, dim3(256), 0, (hipStream_t)stream, d_pk, d_lq, d_v1, d_v2, d_a, d_b, d_tile_ptr, n_slots, d_slot_K,
                     d_slot_nobs, d_slot_omq, d_slot_row, d_slot_key, seed, rep_lo, rep_n, chunks, ld, d_out_corr, d_w_dump, kmax_dump);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_boot2d_fast_slots(const double *d_pk, const double *d_lq, const double *d_v1, const double *d_v2, const double *d_a,
                         const double *d_b, const int64_t *d_tile_ptr, int64_t n_slots, const int32_t *d_slot_K,
                         const double *d_slot_nobs, const double *d_slot_omq, const int64_t *d_slot_row, const int64_t *d_slot_key,
                         uint64_t seed, int32_t rep_lo, int32_t rep_n, int64_t ld, double *d_out_corr, const int64_t *d_slot_list,
                         int64_t n_list, void *stream) {
  MM_ARG(d_pk && d_lq && d_v1 && d_v2 && d_a && d_b && d_tile_ptr && d_slot_K && d_slot_nobs && d_slot_omq && d_slot_row && d_slot_key);
  MM_ARG(d_out_corr && n_slots >= 0 && n_slots % 64 == 0 && rep_n > 0 && ld >= (int64_t)rep_n + 1);
  MM_ARG(rep_lo >= 0 && (int64_t)rep_lo + rep_n <= 2147483647LL);
  MM_ARG(n_list >= 0 && (d_slot_list || n_list == 0));
  if (n_list == 0 || n_slots == 0) return MM_OK;
  int32_t chunks = (int32_t)(((int64_t)rep_n + 63) / 64);
  MM_ARG(n_list <= INT64_MAX / chunks);
  int64_t waves = n_list * chunks;
  dim3 grid;
  if (int rc = fast_grid((waves + 3) / 4, &grid)) return rc;
  hipLaunchKernelGGL(k_boot2d_fast_slots, grid, dim3(256), 0, (hipStream_t)stream, d_pk, d_lq, d_v1, d_v2, d_a, d_b, d_tile_ptr, n_slots,
                     d_slot_K, d_slot_nobs, d_slot_omq, d_slot_row, d_slot_key, seed, rep_lo, rep_n, chunks, ld, d_out_corr, d_slot_list,
                     n_list);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

int mm_boot1d_fast(const double *d_pk, const double *d_lq, const double *d_v, const double *d_a, const double *d_b,
                   const int64_t *d_tile_ptr, int64_t n_slots, const int32_t *d_slot_K, const double *d_slot_nobs,
                   const double *d_slot_omq, const int64_t *d_slot_row, const int64_t *d_slot_key, uint64_t seed, int32_t num_boot,
                   int32_t mean_only, int64_t ld, double *d_out_mean, double *d_out_var, int32_t *d_w_dump, int32_t kmax_dump,
                   void *stream) {
  return mm_boot1d_fast_range(d_pk, d_lq, d_v, d_a, d_b, d_tile_ptr, n_slots, d_slot_K, d_slot_nobs, d_slot_omq, d_slot_row, d_slot_key,
                              seed, 0, num_boot, mean_only, ld, d_out_mean, d_out_var, d_w_dump, kmax_dump, stream);
}

int mm_boot1d_fast_range(const double *d_pk, const double *d_lq, const double *d_v, const double *d_a, const double *d_b,
                         const int64_t *d_tile_ptr, int64_t n_slots, const int32_t *d_slot_K, const double *d_slot_nobs,
                         const double *d_slot_omq, const int64_t *d_slot_row, const int64_t *d_slot_key, uint64_t seed, int32_t rep_lo,
                         int32_t rep_n, int32_t mean_only, int64_t ld, double *d_out_mean, double *d_out_var, int32_t *d_w_dump,
                         int32_t kmax_dump, void *stream) {
  MM_ARG(d_pk && d_lq && d_v && d_a && d_b && d_tile_ptr && d_slot_K && d_slot_nobs && d_slot_omq && d_slot_row && d_slot_key);
  MM_ARG(d_out_mean && d_out_var && n_slots >= 0 && rep_n > 0 && ld >= (int64_t)rep_n + 1);
  MM_ARG(rep_lo >= 0 && (int64_t)rep_lo + rep_n <= 2147483647LL);
  MM_ARG(!d_w_dump || kmax_dump > 0);
  if (n_slots == 0) return MM_OK;
  int32_t chunks = (int32_t)(((int64_t)rep_n + 63) / 64);
  int64_t waves = n_slots * chunks;
  dim3 grid;
  if (int rc = fast_grid((waves + 3) / 4, &grid)) return rc;
  hipLaunchKernelGGL(k_boot1d_fast, grid, dim3(256), 0, (hipStream_t)stream, d_pk, d_lq, d_v, d_a, d_b,
                     d_tile_ptr, n_slots, d_slot_K, d_slot_nobs, d_slot_omq, d_slot_row, d_slot_key, seed, rep_lo, rep_n, mean_only, chunks, ld,
                     d_out_mean, d_out_var, d_w_dump, kmax_dump);
  MM_LAUNCH_CHECK();
  return MM_OK;
}

}  // extern "C"
