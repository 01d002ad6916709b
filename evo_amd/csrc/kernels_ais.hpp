// Annealed importance sampling for EBSC (evoamd_ais_loglik; incomplete data under EVOAMD_AIS_INCOMPLETE, below): per datapoint, C Gibbs chains walk from the
// prior to the posterior (forward: a stochastic LOWER bound on log p(y_n) - ljc) or from a given state back to the prior
// (reverse: with an exact posterior sample as that state, a stochastic UPPER bound -- bidirectional Monte Carlo).  The
// weight of a chain does not depend on K^n.  One wavefront per (datapoint, chain); no atomics on the outputs, every store a
// plain vector store, every sum in a fixed order: two launches give the same bits.
// evo_amd/models/ais.py: ais_log_likelihood_counter is the NumPy mirror -- keep the two and the tests in step.
//
// THE LAW, per datapoint n (data set index i = first_index + n), chain c < C and temperatures 0 = beta_0 < beta_1 <= ... <=
// beta_T = 1 (a float64 array of T + 1 values handed in by the caller).  Hv = H latents vary; pre1, pil_bar and pi are the
// scalars of dpar, B = Y W, G = W^T W and yy = |y|^2 those of the seeding kernels (SeedArgs).  f_beta(s) = exp(|s| pil_bar +
// beta l(s)), so f_0 is the prior up to Z_0 = (1 - pi)^-Hv and f_1 = exp(lpj_n(s)).
//   c_j        = B_nj - sum_{i in s} G_ij (i ascending, one subtraction per term), kept current for every j
//   l(s)       = pre1 (yy_n - sum_{a in s} (B_na + c_a)), a ascending: the flip law's `base` without its m pil_bar
//   x0         = mix64(seed + 0x9e3779b97f4a7c15 (i + 1)), the first hash of kernels_generate.hpp; u01 = gen_u01
//   start      forward: x_0,h = [u01(x0, AIS_PURPOSE + c, h) < pi]: an exact draw from f_0 / Z_0
//              reverse: x_{T-1} = row n of s_start, the same for every chain
//   K_t        one systematic Gibbs scan at beta_t over h ascending (forward) or descending (reverse).  With c_h current:
//              Delta = pil_bar + (beta_t pre1) (G_hh - 2 c_h) with h off, Delta = pil_bar - (beta_t pre1) (G_hh + 2 c_h) with
//              h on; p = 1 / (1 + exp(-Delta)); new bit = [u01(x0, AIS_PURPOSE + c, (t + 1) Hv + h) < p]; on a change
//              c_j -= G_hj (h switched on) or c_j += G_hj (off) for every j: one plain subtraction or addition, never an fma.
//              One uniform per (c, t, h) whatever was decided: chain c does not depend on C, shards concatenate.
//   forward    for t = 1 .. T: log w += (beta_t - beta_{t-1}) l(x_{t-1}); for t < T: x_t = K_t(x_{t-1}).  One more scan at
//              beta_T = 1, K_T with the uniform block T + 1, gives `final`; it does not enter w.
//   reverse    for t = T - 1 .. 1: x_{t-1} = K~_t(x_t); log w = sum_t (beta_t - beta_{t-1}) l(x_{t-1}), accumulated in the
//              order the states are visited (t = T first); `final` = x_0.
//   n_flips    the accepted flips of the chain, the final scan included.
//   estimates  (ais_fold_kernel; "ll without ljc") with a_c = log w_c (forward) or -log w_c (reverse), folded in chain order
//              with the running maximum rescaled when it grows, as lle_fold_kernel does:
//              lse = m + log sum_c exp(a_c - m); forward ll = lse - log C + Hv log1p(exp(pil_bar)), E[exp] exact, E[ll] <=
//              truth; reverse ll = -(lse - log C) + Hv log1p(exp(pil_bar)), E[ll] >= truth when s_start is an exact
//              posterior sample; ess = (sum_c e^{a_c})^2 / sum_c e^{2 a_c}; log_w_mean / min / max over log w_c.
//
// Mapping: lane l owns latents l, l + 64, ...: the c_j of its NC = Hp / 64 <= 16 chunks sit in registers (the kernel is a
// template on NC and the direction, every loop over the chunks unrolls, so no array is indexed dynamically).  The state is
// one wave-uniform word per chunk in BALLOT order (bit l = latent 64 k + l); it leaves as the MSB-first words of K^n.
// LDS: G_jj once per workgroup and B_n. per wavefront, (1 + AIS_WAVES) Hp doubles (40 KB at H = 1024).
// The scan of a chunk is exact, not 64 sequential steps: every unsettled lane decides from the current c; a ballot finds
// the first lane that changes (reverse: the last); that flip is applied -- all lanes take row h of G; the lanes before it
// are settled, the lanes behind it decide again.  Posteriors are sparse: most chunks take one or two rounds.
// l(s) walks the set bits of the words in ascending order: B_na from LDS, c_a from the owning lane (v_readlane).
// Every latent index that becomes an address passes guard_index.
// Cost per chain and temperature: NC chunk rounds (an exp and a hash per latent) plus NC chunk rounds and one row of G
// (8 H bytes) per accepted flip.  G is 8 MB at H = 1024: twice the 4 MiB L2 of an XCD, so a row comes from L2 or from the
// 256 MiB Infinity Cache behind it, never from HBM once the call is under way.
//
// INCOMPLETE DATA (MASKED = true; masks resident and EVOAMD_AIS_INCOMPLETE): everything above stays -- the stream, the
// start, the scan order, the conditional, l(s), log w, the fold, n_flips -- except where G comes from.
//   B_n, yy_n  the resident ones: evoamd_upload_masks zeroes the entries of Y under False, so both are sums over the
//              reliable entries already; values of y under False, NaN included, never enter.
//   o, nd      the reliable d of datapoint n in ascending d (seed_list_reliable) and their number.
//   G(n)_hj    = sum_{d in o, ascending} (W_dh W_dj): each product rounded, then added, starting from 0.0, contraction
//              off.  NOT seed_gram_sweep's fma: the NumPy mirror reproduces the bits and NumPy has no fma.  The diagonal
//              g(n)_jj is the same sum with h = j, formed once per datapoint.
//   c_j        = B_nj - sum_{i in s, ascending} G(n)_ij; a flip of h subtracts or adds the row G(n)_h., one plain operation
//              per j.  The row is formed when the flip happens, from W and the list o, with the column W_.h over o staged
//              in LDS; no G(n) is stored.  A start with bits on forms one row per active latent in ascending order.
//   nd = 0     G(n) = 0, B = 0, yy = 0: the chains are prior draws, log w = 0, ll_n = Hv log1p(exp(pil_bar)).  The datapoint
//              is not skipped: it stays in the sum and in the count N.
// Mapping: as above, with the diagonal in NC more registers per lane (the same unrolled chunks as c_j) and an accumulator
// per chunk while a row is formed: d outer, chunks inner, so a row of W is read once, coalesced over j.  LDS per wavefront:
// B_n. (Hp doubles), the column (D doubles) and the list (D ints); nothing per workgroup.  At H = 1024, D = 256 that is
// 4 (8192 + 3072) = 44 KiB per workgroup: three workgroups per CU, three waves per SIMD.  Above 64 KiB (large D) the
// launch needs hipFuncAttributeMaxDynamicSharedMemorySize; a geometry above the 160 KiB of a CU is refused by the host.
// Cost of a flip: nd rows of W (8 H bytes each) instead of one row of G -- nd H / 64 multiply-adds per lane.
#pragma once
#include "common.hpp"
#include "kernels_generate.hpp"
#include "kernels_seed.hpp"

#define AIS_PURPOSE 0x4149530000000000ull  // "AIS"; chain c draws under purpose AIS_PURPOSE + c
#define AIS_WAVES 4
#define AIS_MAX_NC 16

struct AisArgs {
  const double *Bm;     // (N, H) B = Y W
  const double *yy;     // (N)
  const double *G;      // (H, H)
  const double *Gd;     // (H) diag(G)
  const double *dpar;
  const double *betas;  // (T + 1)
  const u64 *s_start;   // (N, HW) MSB-first words, reverse only
  double *log_w;        // (N, C)
  u64 *fin;             // (N, C, HW) MSB-first words
  int *flips;           // (N, C)
  int *err;
  i64 N;
  int C, T, H, HW;
  u64 seed, first_index;
  // incomplete data (MASKED) only
  const double *W;      // (D, H)
  const uint8_t *mask;  // (N, D) x_infr
  int D;
};

// MASKED: the doubles a wavefront has in LDS beside its `rows` rows of Hp doubles -- the column (D doubles), then the list
// (D ints, rounded up to a double)
__host__ __device__ static inline size_t ais_masked_wave_doubles(int HW, int D, int rows) {
  return (size_t)rows * 64 * HW + (size_t)D + (size_t)(D + 1) / 2;
}
static inline size_t ais_masked_lds_bytes(int HW, int D) { return (size_t)AIS_WAVES * ais_masked_wave_doubles(HW, D, 1) * sizeof(double); }

__device__ __forceinline__ double ais_readlane(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

// Incomplete data: row h of G(n) into acc (DIAG: its diagonal; h is not read), lane l the latents l, l + 64, ... -- the sum
// over the list dl of the reliable d in its order, each product rounded, then added.  The column W_.h over the list goes
// through col (LDS); the syncs keep a row's reads of col in front of the next row's writes.
template <int NC, bool DIAG>
__device__ __forceinline__ void ais_gram_row(const double *__restrict__ W, int D, int H, int HW, int *err, int lane, const int *dl,
                                             double *col, int nd, int h, double (&acc)[NC]) {
#pragma clang fp contract(off)
  if (!DIAG) {
    seed_wave_sync();
    for (int i = lane; i < nd; i += 64) col[i] = W[(size_t)guard_index(dl[i], D, err) * H + h];
    seed_wave_sync();
  }
#pragma unroll
  for (int k = 0; k < NC; k++) acc[k] = 0.0;
  for (int i = 0; i < nd; i++) {
    const double *Wd = W + (size_t)guard_index(dl[i], D, err) * H;
    const double cw = DIAG ? 0.0 : col[i];
#pragma unroll
    for (int k = 0; k < NC; k++) {
      const int j = 64 * k + lane;
      if (k < HW && j < H) {
        const double w = Wd[j];
        acc[k] = acc[k] + (DIAG ? w : cw) * w;
      }
    }
  }
}

template <int NC, bool REV, bool MASKED = false>
__global__ __launch_bounds__(64 * AIS_WAVES) void ais_chain_kernel(AisArgs a) {
#pragma clang fp contract(off)
  const int lane = lane_id(), wave = wave_id_uniform();
  const int H = a.H, HW = a.HW, T = a.T, C = a.C;
  const double pre1 = a.dpar[DP_PRE1], pilb = a.dpar[DP_PILBAR], pi = a.dpar[DP_PI];
  constexpr bool rev = REV;
  // LDS: G_jj for the workgroup (Hp doubles), then B_n. of each wavefront's datapoint (Hp doubles each)
  // MASKED: per wavefront B_n., the column and the list; the diagonal of G(n) is in registers
  extern __shared__ double ais_lds[];
  const int Hp = 64 * HW;
  double *gd = ais_lds, *bn = ais_lds + (size_t)(1 + wave) * Hp;
  [[maybe_unused]] double *col = nullptr;
  [[maybe_unused]] int *dl = nullptr;
  if constexpr (MASKED) {
    bn = ais_lds + (size_t)wave * ais_masked_wave_doubles(HW, a.D, 1);
    col = bn + Hp, dl = (int *)(col + a.D);
  } else {
    for (int h = (int)threadIdx.x; h < Hp; h += (int)blockDim.x) gd[h] = h < H ? a.Gd[h] : 0.0;
    __syncthreads();
  }
  const i64 items = a.N * (i64)C;
  for (i64 it = (i64)blockIdx.x * AIS_WAVES + wave; it < items; it += (i64)gridDim.x * AIS_WAVES) {
    const i64 n = it / C;
    const int ch = (int)(it - n * C);
    const u64 x0 = mix64(a.seed + 0x9e3779b97f4a7c15ull * (a.first_index + (u64)n + 1));
    const u64 purpose = AIS_PURPOSE + (u64)ch;
    const double yy = a.yy[n];
    double c[NC];
    u64 word[NC];  // wave-uniform, ballot order
    seed_wave_sync();  // the previous item's reads of bn are done
#pragma unroll
    for (int k = 0; k < NC; k++) {
      const int h = 64 * k + lane;
      c[k] = (k < HW && h < H) ? a.Bm[(size_t)n * H + h] : 0.0;
      if (k < HW) bn[h] = c[k];
      word[k] = 0ull;
    }
    [[maybe_unused]] int nd = 0;
    [[maybe_unused]] double gdr[NC], row[NC];  // MASKED: g(n)_jj of the lane's latents; the row being applied
    if constexpr (MASKED) nd = seed_list_reliable(a.mask + (size_t)n * a.D, a.D, lane, dl);
    seed_wave_sync();
    if constexpr (MASKED) ais_gram_row<NC, true>(a.W, a.D, H, HW, a.err, lane, dl, col, nd, 0, gdr);
    // ---- the start
#pragma unroll
    for (int k = 0; k < NC; k++) {
      if (k >= HW) continue;
      const int h = 64 * k + lane;
      if (!rev) {
        word[k] = __ballot(h < H && gen_u01(x0, purpose, (u64)h) < pi);
      } else {
        const int rem = H - 64 * k;
        const u64 w = gen_uniform(a.s_start[(size_t)n * HW + k]) & (rem >= 64 ? ~0ull : ~0ull << (64 - rem));
        word[k] = __brevll(w);
      }
    }
    // c_j = B_nj - sum over the active i, ascending
#pragma unroll
    for (int k = 0; k < NC; k++) {
      if (k >= HW) continue;
      u64 bits = word[k];
      while (bits) {
        const int b = __builtin_ctzll(bits);
        bits &= bits - 1ull;
        const int i = guard_index(64 * k + b, H, a.err);
        if constexpr (MASKED) {
          ais_gram_row<NC, false>(a.W, a.D, H, HW, a.err, lane, dl, col, nd, i, row);
#pragma unroll
          for (int kk = 0; kk < NC; kk++) c[kk] = c[kk] - row[kk];
        } else {
          const double *Gi = a.G + (size_t)i * H;
#pragma unroll
          for (int kk = 0; kk < NC; kk++) {
            const int j = 64 * kk + lane;
            if (kk < HW && j < H) c[kk] = c[kk] - Gi[j];
          }
        }
      }
    }
    int flips = 0;
    // l(s) of the current state
    auto ell = [&]() -> double {
#pragma clang fp contract(off)
      double sum = 0.0;
#pragma unroll
      for (int k = 0; k < NC; k++) {
        if (k >= HW) continue;
        u64 bits = word[k];
        while (bits) {
          const int b = __builtin_ctzll(bits);
          bits &= bits - 1ull;
          sum = sum + (bn[64 * k + b] + ais_readlane(c[k], b));
        }
      }
      return pre1 * (yy - sum);
    };
    // one flip of latent 64 k + b: the word, the count, row h of G into every lane's c
    auto apply = [&](int k_flip, int b, bool was_on) {
#pragma clang fp contract(off)
      const int h = guard_index(64 * k_flip + b, H, a.err);
      if constexpr (MASKED) {
        ais_gram_row<NC, false>(a.W, a.D, H, HW, a.err, lane, dl, col, nd, h, row);
#pragma unroll
        for (int kk = 0; kk < NC; kk++) c[kk] = was_on ? c[kk] + row[kk] : c[kk] - row[kk];
      } else {
        const double *Gh = a.G + (size_t)h * H;
#pragma unroll
        for (int kk = 0; kk < NC; kk++) {
          const int j = 64 * kk + lane;
          if (kk < HW && j < H) {
            const double g = Gh[j];
            c[kk] = was_on ? c[kk] + g : c[kk] - g;
          }
        }
      }
      flips++;
    };
    // one systematic scan at beta, uniform block `block`
    auto scan = [&](double beta, int block) {
#pragma clang fp contract(off)
      const double bp = beta * pre1;
      const u64 base = (u64)block * (u64)H;
#pragma unroll
      for (int kq = 0; kq < NC; kq++) {
        const int k = rev ? NC - 1 - kq : kq;
        if (k >= HW) continue;
        const int h = 64 * k + lane;
        const bool valid = h < H;
        const double u = gen_u01(x0, purpose, base + (u64)(valid ? h : 0));
        double g;
        if constexpr (MASKED)
          g = gdr[k];
        else
          g = gd[h];
        u64 open = ~0ull;  // the lanes not yet settled
        while (true) {
          const bool on = (word[k] >> lane) & 1ull;
          const double e = on ? g + 2.0 * c[k] : g - 2.0 * c[k];
          const double t = bp * e;
          const double delta = on ? pilb - t : pilb + t;
          const double p = 1.0 / (1.0 + exp(-delta));
          const bool nb = u < p;
          const u64 m = __ballot(valid && nb != on) & open;
          if (m == 0ull) break;  // (wave-uniform)
          const int b = rev ? 63 - __builtin_clzll(m) : __builtin_ctzll(m);
          const bool was_on = (word[k] >> b) & 1ull;
          word[k] ^= 1ull << b;
          apply(k, b, was_on);
          open = rev ? (b == 0 ? 0ull : ~0ull >> (64 - b)) : (b == 63 ? 0ull : ~0ull << (b + 1));
          if (open == 0ull) break;
        }
      }
    };
    double lw = 0.0;
    if (!rev) {
      for (int t = 1; t <= T; t++) {  // (the scan of t = T is the one that gives `final`)
        const double bt = a.betas[t], db = bt - a.betas[t - 1];
        lw = lw + db * ell();
        scan(bt, t + 1);
      }
    } else {
      lw = (a.betas[T] - a.betas[T - 1]) * ell();
      for (int t = T - 1; t >= 1; t--) {
        const double bt = a.betas[t];
        scan(bt, t + 1);
        lw = lw + (bt - a.betas[t - 1]) * ell();
      }
    }
    if (lane == 0) {
      a.log_w[it] = lw;
      a.flips[it] = flips;
    }
#pragma unroll
    for (int k = 0; k < NC; k++)
      if (k < HW && lane == k) a.fin[(size_t)it * HW + k] = __brevll(word[k]);
  }
}

// Per datapoint: the chains' weights folded in chain order (one thread per datapoint; C is small).
__global__ __launch_bounds__(256) void ais_fold_kernel(const double *__restrict__ log_w, const int *__restrict__ flips, i64 N, int C,
                                                       int reverse, int Hv, const double *__restrict__ dpar, double *__restrict__ ll,
                                                       double *__restrict__ ess, double *__restrict__ lw_mean,
                                                       double *__restrict__ lw_min, double *__restrict__ lw_max,
                                                       i64 *__restrict__ n_flips) {
#pragma clang fp contract(off)
  const i64 n = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const double *lw = log_w + (size_t)n * C;
  double m = -INFINITY, z = 0.0, q = 0.0, sum = 0.0, lo = INFINITY, hi = -INFINITY;
  i64 nf = 0;
  for (int c = 0; c < C; c++) {
    const double v = lw[c], t = reverse ? -v : v;
    if (t > m) {  // (the first one: 0 * exp(-inf) + 1)
      const double r = exp(m - t);
      z = z * r + 1.0;
      q = q * (r * r) + 1.0;
      m = t;
    } else {
      const double e = exp(t - m);
      z = z + e;
      q = q + e * e;
    }
    sum = sum + v;
    lo = fmin(lo, v), hi = fmax(hi, v);
    nf += flips[(size_t)n * C + c];
  }
  const double lse = m + log(z) - log((double)C);
  const double lz0 = (double)Hv * log1p(exp(dpar[DP_PILBAR]));
  ll[n] = (reverse ? -lse : lse) + lz0;
  ess[n] = z * z / q;
  lw_mean[n] = sum / (double)C;
  lw_min[n] = lo, lw_max[n] = hi;
  n_flips[n] = nf;
}

// admit: the `final` states of the first min(C, Cmax) chains into the candidate batch in chain order, the all-zero state
// skipped, with their digests where digests are in use (one thread per datapoint)
__global__ __launch_bounds__(256) void ais_admit_kernel(const u64 *__restrict__ fin, i64 N, int C, int HW, int Cmax, u64 *__restrict__ cand,
                                                        u64 *__restrict__ cand_dig, int *__restrict__ counts) {
  const i64 n = (i64)blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const int take = C < Cmax ? C : Cmax;
  int cnt = 0;
  for (int c = 0; c < take; c++) {
    const u64 *src = fin + ((size_t)n * C + c) * HW;
    u64 any = 0ull;
    for (int w = 0; w < HW; w++) any |= src[w];
    if (any == 0ull) continue;
    u64 *dst = cand + ((size_t)n * Cmax + cnt) * HW;
    for (int w = 0; w < HW; w++) dst[w] = src[w];
    if (cand_dig) cand_dig[(size_t)n * Cmax + cnt] = make_digest(src, HW);
    cnt++;
  }
  counts[n] = cnt;
}
