// Posterior expectations from annealed importance sampling (evoamd_ais_posterior): the forward chains of kernels_ais.hpp,
// continued at beta = 1, give weighted marginals E_p[s_h | y_n] that do not start from K^n.  A forward chain with its weight
// is a properly weighted sample of the true posterior; the self-normalised sum over the chains is a consistent estimate of
// a posterior expectation, and every further Gibbs scan at beta = 1 keeps it so.  EBSC; incomplete data: below.
// One wavefront per (datapoint, chain); no atomics on the outputs, every store a plain vector store, every sum in a fixed order: two launches
// give the same bits.  evo_amd/models/ais.py: ais_posterior_counter is the NumPy mirror -- keep the two and the tests in step.
//
// THE LAW (names, stream, start, c_j, l(s), K_t and log w as in kernels_ais.hpp, forward direction), per datapoint n, chain
// c < C, temperatures beta_0 .. beta_T and K = n_keep >= 1:
//   chain      for t = 1 .. T: log w += (beta_t - beta_{t-1}) l(x_{t-1}); x_t = K_t(x_{t-1}) with the uniform block t + 1.  The
//              scan at beta_T = 1 is the first KEPT scan; kept scans 2 .. K follow at beta = 1 with the uniform blocks T + 2,
//              T + 3, ...; they do not enter w.  So log w, and with K = 1 the flips and the state, are those of
//              evoamd_ais_loglik's forward chain c.
//   R_c[h]     in every kept scan, when latent h is decided: R_c[h] += p with p = 1 / (1 + exp(-Delta)) from the current
//              c_h -- a plain add in scan order, whether or not the bit changes.  r_ch = R_c[h] / K.  (Rao-Blackwell: the
//              conditional, not the bit.  A latent that no chain switched on still gets its mass.)
//   best       after every kept scan lpj(x) = |x| pil_bar + l(x) (one multiplication, one addition); the chain keeps its best
//              visited state: a strictly greater value replaces it, the earliest scan wins ties.
//   n_flips    the accepted flips of the chain, every kept scan included.
//   fold       (ais_post_fold_kernel) per datapoint, chains in order: m, z, q as ais_fold_kernel forms them (running maximum
//              rescaled), lse = m + log z, a_c = exp(log w_c - lse);
//              p_nh = sum_c a_c r_ch; p_se_nh = sqrt(sum_c (a_c (r_ch - p_nh))^2), the delta-method error of a self-normalised
//              estimate; count_n = sum_h p_nh, h ascending; map_lpj / map_state = the best over the chains, ties to the
//              lowest chain; ll, ess, log_w_mean / _min / _max and n_flips as ais_fold_kernel.
//
// Mapping: as ais_chain_kernel<NC, false> -- lane l owns latents l, l + 64, ..., c_j in registers, the state one wave-uniform
// word per chunk in ballot order.  The chunk scan is the exact one of kernels_ais.hpp; a lane adds the p of the round in which
// it is SETTLED: the flipping lane and every open lane before it, or every open lane when no lane changes.  At that round c_h
// holds exactly the flips of all earlier latents, which is what a sequential scan sees.  R_c[h] is touched by the lane that
// owns h alone.
// LDS: G_jj once per workgroup, B_n. and R_c per wavefront, (1 + 2 AIS_WAVES) Hp doubles, and behind them per wavefront the
// best lpj in front of the best state's words (AIS_WAVES (HW + 1) words): 72.5 KiB at H = 1024, two workgroups per CU, which
// is what the registers allow anyway.  Above 64 KiB the launch needs hipFuncAttributeMaxDynamicSharedMemorySize (set by the
// host once per instantiation).  R_c, the best words and the best lpj are in LDS, not in registers: the two registers of
// that lpj alone put NC = 1 and NC = 4 one occupancy step below ais_chain_kernel<NC, false>.
// The rows r_c. of a block of datapoints go to a buffer of at most AIS_POST_ROWS_BYTES; the host walks the datapoints in
// blocks, chains then fold.  Nothing depends on the block size: every index of the stream is the datapoint's own.
//
// LISTED DATAPOINTS (evoamd_ais_posterior_sel with a list): work item (i, c) runs chain c of datapoint index[i] -- the first
// hash, yy, the row of B and the row of the mask are that datapoint's, everything written is row i.  So row i has the bits of
// row index[i] of the call without a list.  The blocks run over list positions; the fold needs no source index.
//
// INCOMPLETE DATA (MASKED = true; masks resident and the flag EVOAMD_AIS_INCOMPLETE of evoamd_ais_posterior_ex): the law
// above with the B_n, yy_n, the list o, G(n), its diagonal and c_j of kernels_ais.hpp's INCOMPLETE DATA -- a row of G(n)
// is formed from W and the list when a flip happens, products rounded and added in ascending d.  R_c, best, n_flips and
// the fold are unchanged; a datapoint without a reliable entry has p_nh = 1 / (1 + exp(-pil_bar)) for every h.  mean = p W^T
// covers every entry, the missing ones included.
// LDS: per wavefront B_n., R_c, the column (D doubles) and the list (D ints), then the best lpj and words; the diagonal is
// in registers.  At H = 1024, D = 256: 4 (2 x 8192 + 3072) + 544 = 76.5 KiB per workgroup, two workgroups per CU, two
// waves per SIMD.
#pragma once
#include "kernels_ais.hpp"

#define AIS_POST_ROWS_BYTES (256ull << 20)  // the per-chain rows of one block of datapoints: at most 256 MiB

// One block of nb datapoints: the per-datapoint and per-chain pointers are those of the block's first datapoint, and
// first_index is the data set index of that datapoint.
struct AisPostArgs {
  const double *Bm;     // (nb, H) B = Y W
  const double *yy;     // (nb)
  const double *G;      // (H, H)
  const double *Gd;     // (H) diag(G)
  const double *dpar;
  const double *betas;  // (T + 1)
  double *log_w;        // (nb, C)
  double *best_lpj;     // (nb, C)
  u64 *best;            // (nb, C, HW) MSB-first words
  int *flips;           // (nb, C)
  double *rb;           // (nb, C, Hp)
  int *err;
  i64 nb;
  int C, T, K, H, HW;
  u64 seed, first_index;
  // incomplete data (MASKED) only
  const double *W;      // (D, H)
  const uint8_t *mask;  // (nb, D) x_infr
  int D;
  // listed datapoints: work item (i, c) runs the chain of datapoint index[i]; Bm, yy and mask are then those of the whole
  // shard and first_index that of its first datapoint.  Null for every call without a list.
  const i64 *index;     // (nb) ascending
};

static inline size_t ais_post_lds_bytes(int HW) {
  return (size_t)(1 + 2 * AIS_WAVES) * 64 * HW * sizeof(double) + (size_t)AIS_WAVES * (HW + 1) * sizeof(u64);
}

// MASKED: per wavefront B_n., R_c, the column and the list, and behind them the best lpj and words as above
static inline size_t ais_post_masked_lds_bytes(int HW, int D) {
  return (size_t)AIS_WAVES * ais_masked_wave_doubles(HW, D, 2) * sizeof(double) + (size_t)AIS_WAVES * (HW + 1) * sizeof(u64);
}

// PLAIN: the instantiation never sees a list and does not read a.index.  It exists for NC = 1 on complete data alone: there
// the two scalar registers of the pointer push the kernel over its SGPR budget (99 -> 106, 70 -> 73 VGPRs, 7 -> 6 waves
// per SIMD); every other instantiation keeps its registers, scratch and LDS with the pointer and takes it at run time.
template <int NC, bool MASKED = false, bool PLAIN = false>
__global__ __launch_bounds__(64 * AIS_WAVES) void ais_post_chain_kernel(AisPostArgs a) {
#pragma clang fp contract(off)
  const int lane = lane_id(), wave = wave_id_uniform();
  const int H = a.H, HW = a.HW, T = a.T, C = a.C, K = a.K;
  const double pre1 = a.dpar[DP_PRE1], pilb = a.dpar[DP_PILBAR], pi = a.dpar[DP_PI];
  // LDS: G_jj for the workgroup (Hp doubles), then B_n. and R_c of each wavefront (Hp doubles each), then per wavefront the
  // best lpj and the best state's words (the two registers of that lpj are what separates NC = 1 and 4 from the next lower
  // occupancy)
  // MASKED: no G_jj (the diagonal of G(n) is in registers); per wavefront B_n., R_c, the column and the list
  extern __shared__ double ais_post_lds[];
  const int Hp = 64 * HW;
  double *gd = ais_post_lds, *bn = ais_post_lds + (size_t)(1 + 2 * wave) * Hp, *R = bn + Hp;
  double *bl = ais_post_lds + (size_t)(1 + 2 * AIS_WAVES) * Hp + (size_t)wave * (HW + 1);
  [[maybe_unused]] double *col = nullptr;
  [[maybe_unused]] int *dl = nullptr;
  if constexpr (MASKED) {
    const size_t per_wave = ais_masked_wave_doubles(HW, a.D, 2);
    bn = ais_post_lds + (size_t)wave * per_wave, R = bn + Hp;
    col = R + Hp, dl = (int *)(col + a.D);
    bl = ais_post_lds + (size_t)AIS_WAVES * per_wave + (size_t)wave * (HW + 1);
  }
  u64 *bw = (u64 *)(bl + 1);
  if constexpr (!MASKED) {
    for (int h = (int)threadIdx.x; h < Hp; h += (int)blockDim.x) gd[h] = h < H ? a.Gd[h] : 0.0;
    __syncthreads();
  }
  const i64 items = a.nb * (i64)C;
  for (i64 it = (i64)blockIdx.x * AIS_WAVES + wave; it < items; it += (i64)gridDim.x * AIS_WAVES) {
    const i64 pos = it / C;  // the row of the outputs
    const int ch = (int)(it - pos * C);
    const i64 n = (!PLAIN && a.index) ? a.index[pos] : pos;  // (wave-uniform) the datapoint whose chain this is
    const u64 x0 = mix64(a.seed + 0x9e3779b97f4a7c15ull * (a.first_index + (u64)n + 1));
    const u64 purpose = AIS_PURPOSE + (u64)ch;
    const double yy = a.yy[n];
    double c[NC];
    u64 word[NC];  // wave-uniform, ballot order
    seed_wave_sync();  // the previous item's reads of bn and bw are done
#pragma unroll
    for (int k = 0; k < NC; k++) {
      const int h = 64 * k + lane;
      c[k] = (k < HW && h < H) ? a.Bm[(size_t)n * H + h] : 0.0;
      if (k < HW) bn[h] = c[k], R[h] = 0.0;
      word[k] = 0ull;
    }
    [[maybe_unused]] int nd = 0;
    [[maybe_unused]] double gdr[NC], row[NC];  // MASKED: g(n)_jj of the lane's latents; the row being applied
    if constexpr (MASKED) nd = seed_list_reliable(a.mask + (size_t)n * a.D, a.D, lane, dl);
    seed_wave_sync();
    if constexpr (MASKED) ais_gram_row<NC, true>(a.W, a.D, H, HW, a.err, lane, dl, col, nd, 0, gdr);
    // ---- the start: an exact draw from the prior
#pragma unroll
    for (int k = 0; k < NC; k++) {
      if (k >= HW) continue;
      const int h = 64 * k + lane;
      word[k] = __ballot(h < H && gen_u01(x0, purpose, (u64)h) < pi);
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
    // one flip of latent 64 k + b: the count, row h of G into every lane's c
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
    // one systematic scan at beta, uniform block `block`; keep: a lane adds its p to R in the round that settles it
    auto scan = [&](double beta, int block, bool keep) {
#pragma clang fp contract(off)
      const double bp = beta * pre1;
      const u64 base = (u64)block * (u64)H;
#pragma unroll
      for (int k = 0; k < NC; k++) {
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
          const int b = m ? __builtin_ctzll(m) : 63;  // (wave-uniform) the lane that flips, or none: all open lanes settle
          if (keep && valid && ((open >> lane) & 1ull) && lane <= b) R[h] = R[h] + p;
          if (m == 0ull) break;
          const bool was_on = (word[k] >> b) & 1ull;
          word[k] ^= 1ull << b;
          apply(k, b, was_on);
          open = b == 63 ? 0ull : ~0ull << (b + 1);
          if (open == 0ull) break;
        }
      }
    };
    double lw = 0.0;
    for (int t = 1; t <= T + K; t++) {  // the scans t = T .. T + K - 1 are the kept ones, all at beta_T = 1
      const double e = ell();  // of x_{t-1}: enters w up to t = T, and lpj behind every kept scan
      const double bt = a.betas[t < T ? t : T];
      if (t <= T) lw = lw + (bt - a.betas[t - 1]) * e;
      if (t > T) {
        int cnt = 0;
#pragma unroll
        for (int k = 0; k < NC; k++)
          if (k < HW) cnt += __popcll(word[k]);
        const double lpj = (double)cnt * pilb + e;
        seed_wave_sync();
        const bool better = t == T + 1 || lpj > bl[0];  // (wave-uniform)
        seed_wave_sync();
        if (better) {
          if (lane == 0) bl[0] = lpj;
#pragma unroll
          for (int k = 0; k < NC; k++)
            if (k < HW && lane == k) bw[k] = __brevll(word[k]);
        }
      }
      if (t < T + K) scan(bt, t + 1, t >= T);
    }
    seed_wave_sync();  // bw, written by lane k, is read by lane k again: the fence orders it behind the last write
    if (lane == 0) {
      a.log_w[it] = lw;
      a.best_lpj[it] = bl[0];
      a.flips[it] = flips;
    }
    if (lane < HW) a.best[(size_t)it * HW + lane] = bw[lane];
    const double kd = (double)K;
#pragma unroll
    for (int k = 0; k < NC; k++)
      if (k < HW) a.rb[(size_t)it * Hp + 64 * k + lane] = R[64 * k + lane] / kd;
  }
}

struct AisPostFoldArgs {
  const double *log_w;     // (N, C)
  const double *best_lpj;  // (N, C)
  const u64 *best;         // (N, C, HW)
  const int *flips;        // (N, C)
  const double *rb;        // (nb, C, Hp)
  const double *dpar;
  double *wts;             // (N, C): a_c, formed once
  double *p, *p_se;        // (N, H)
  double *count, *map_lpj, *ll, *ess, *lw_mean, *lw_min, *lw_max;  // (N)
  u64 *map_state;          // (N, HW)
  i64 *n_flips;            // (N)
  i64 n0, nb;
  int C, H, HW;
};

// Per datapoint of the block: one wavefront, lanes over h, chains in order.
__global__ __launch_bounds__(64 * AIS_WAVES) void ais_post_fold_kernel(AisPostFoldArgs a) {
#pragma clang fp contract(off)
  const int lane = lane_id(), wave = wave_id_uniform();
  const i64 nl = (i64)blockIdx.x * AIS_WAVES + wave;
  if (nl >= a.nb) return;  // (wave-uniform)
  const i64 n = a.n0 + nl;
  const int C = a.C, H = a.H, HW = a.HW, Hp = 64 * HW;
  const double *lw = a.log_w + (size_t)n * C;
  // the weights' fold, the same in every lane
  double m = -INFINITY, z = 0.0, q = 0.0, sum = 0.0, lo = INFINITY, hi = -INFINITY;
  i64 nf = 0;
  int top = 0;
  double top_lpj = a.best_lpj[(size_t)n * C];
  for (int c = 0; c < C; c++) {
    const double v = lw[c];
    if (v > m) {  // (the first one: 0 * exp(-inf) + 1)
      const double r = exp(m - v);
      z = z * r + 1.0;
      q = q * (r * r) + 1.0;
      m = v;
    } else {
      const double e = exp(v - m);
      z = z + e;
      q = q + e * e;
    }
    sum = sum + v;
    lo = fmin(lo, v), hi = fmax(hi, v);
    nf += a.flips[(size_t)n * C + c];
    const double bl = a.best_lpj[(size_t)n * C + c];
    if (bl > top_lpj) top = c, top_lpj = bl;  // strictly: ties go to the lowest chain
  }
  const double lse = m + log(z);
  double *wts = a.wts + (size_t)n * C;
  for (int c = lane; c < C; c += 64) wts[c] = exp(lw[c] - lse);
  seed_wave_sync();
  const double *rows = a.rb + (size_t)nl * C * Hp;
  double cnt = 0.0;
  for (int k = 0; k < HW; k++) {
    const int h = 64 * k + lane;
    const bool valid = h < H;
    double p = 0.0, s2 = 0.0;
    for (int c = 0; c < C; c++) p = p + wts[c] * rows[(size_t)c * Hp + h];
    for (int c = 0; c < C; c++) {
      const double d = wts[c] * (rows[(size_t)c * Hp + h] - p);
      s2 = s2 + d * d;
    }
    if (valid) {
      a.p[(size_t)n * H + h] = p;
      a.p_se[(size_t)n * H + h] = sqrt(s2);
    }
    const double pv = valid ? p : 0.0;  // (the rows are 0 there anyway)
#pragma unroll
    for (int l = 0; l < 64; l++) cnt = cnt + ais_readlane(pv, l);  // h ascending
  }
  if (lane < HW) a.map_state[(size_t)n * HW + lane] = a.best[((size_t)n * C + top) * HW + lane];
  if (lane == 0) {
    a.count[n] = cnt;
    a.map_lpj[n] = top_lpj;
    a.ll[n] = (lse - log((double)C)) + (double)H * log1p(exp(a.dpar[DP_PILBAR]));
    a.ess[n] = z * z / q;
    a.lw_mean[n] = sum / (double)C;
    a.lw_min[n] = lo, a.lw_max[n] = hi;
    a.n_flips[n] = nf;
  }
}

// ---------------------------------------------------------------------------------------
// ADMISSION (EVOAMD_AIS_ADMIT of evoamd_ais_posterior_sel): the best distinct states the chains of a datapoint visited become
// its rows of the candidate batch; the model's own candidate lpj and selection follow (the host has the order of the stages).
// evo_amd/models/ais.py: ais_admit_candidates_host is the NumPy mirror of the emission.
//
// THE LAW OF THE EMISSION, per listed datapoint i (source datapoint n = index[i], or i without a list), from best_lpj (C) and
// best (C, HW) of its chains:
//   ranking    a chain whose best_lpj is not finite (NaN, +inf, -inf) is left out of the walk and of every count.  The others
//              rank by best_lpj descending, ties by ascending chain.
//   walk       in rank order a state is dropped when it is all-zero, when it equals in all HW words the state of a chain
//              ranked before it, or when K^n of datapoint n holds it (exact on the words, all S slots).  The others are NEW;
//              the first Cmax of them are written to cand[(n Cmax + k) HW], k in rank order, with their digests where digests
//              are in use, and cand_counts[n] = their number.  (The host clears cand_counts first: 0 outside the list.)
//   counts     n_distinct = the states that are not all-zero and equal no state ranked before them; n_new = those of them K^n
//              does not hold; n_proposed = min(n_new, Cmax); map_held = whether K^n holds map_state, the best state of the
//              fold (chain 0 when its best_lpj is NaN, else the first chain with the greatest value that is not NaN).
// ais_post_tally_kernel, after the selection: n_admitted = the proposed states K^n now holds, map_held again.
//
// Mapping: one wavefront per listed datapoint.  A chain's rank and its duplicate test run with the lanes over the other
// chains (ballots), "K^n holds it" with the lanes over the S slots; the walk over the chains is wave-uniform.  The rank of
// a new chain goes to key (C ints per datapoint, INT_MAX otherwise), from which its place among the new ones is one more
// ballot count.  Every store is a plain vector store.
// ---------------------------------------------------------------------------------------
struct AisPostAdmitArgs {
  const double *best_lpj;  // (n, C)
  const u64 *best;         // (n, C, HW)
  const i64 *index;        // (n) or null
  const u64 *states;       // K^n (N, S, HW)
  u64 *cand;               // (N, Cmax, HW)
  u64 *cand_dig;           // (N, Cmax) or null
  int *cand_counts;        // (N)
  int *key;                // (n, C) scratch
  int *n_distinct, *n_new, *n_proposed, *n_admitted, *map_held;  // (n) each; the emission leaves n_admitted alone
  const double *F_full;    // (N) F of every datapoint, or null
  double *F_out;           // (n) that of the listed ones
  i64 n;
  int C, S, HW, Cmax;
};

__device__ __forceinline__ bool ais_post_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }

// (wave-uniform) does K^n of one datapoint hold the state at `w`?  Lanes over the slots, exact on the words.
__device__ __forceinline__ bool ais_post_kn_holds(const u64 *__restrict__ kn, int S, int HW, const u64 *__restrict__ w, int lane) {
  bool any = false;
  for (int s0 = 0; s0 < S; s0 += 64) {
    const int s = s0 + lane;
    bool eq = s < S;
    const u64 *sp = kn + (size_t)(eq ? s : 0) * HW;
    for (int j = 0; j < HW; j++) eq = eq && sp[j] == w[j];
    any = any || __ballot(eq) != 0ull;
  }
  return any;
}

// (wave-uniform) the chain whose best state is map_state: the fold's rule
__device__ __forceinline__ int ais_post_top_chain(const double *__restrict__ bl, int C, int lane) {
  if (bl[0] != bl[0]) return 0;
  double m = -INFINITY;
  for (int c0 = 0; c0 < C; c0 += 64) {
    const int cp = c0 + lane;
    const double v = cp < C ? bl[cp] : -INFINITY;
    if (v == v) m = fmax(m, v);
  }
  m = wave_max(m);
  unsigned first = (unsigned)C;
  for (int c0 = 0; c0 < C; c0 += 64) {
    const int cp = c0 + lane;
    if (cp < C && bl[cp] == m && (unsigned)cp < first) first = (unsigned)cp;
  }
  first = wave_min_u32(first);
  return first < (unsigned)C ? (int)first : 0;
}

#define AIS_POST_ADMIT_WAVES 4
__global__ __launch_bounds__(64 * AIS_POST_ADMIT_WAVES) void ais_post_admit_kernel(AisPostAdmitArgs a) {
  const int lane = lane_id(), wave = wave_id_uniform();
  const i64 i = (i64)blockIdx.x * AIS_POST_ADMIT_WAVES + wave;
  if (i >= a.n) return;  // (wave-uniform)
  const int C = a.C, S = a.S, HW = a.HW, Cmax = a.Cmax;
  const i64 n = a.index ? a.index[i] : i;
  const double *bl = a.best_lpj + (size_t)i * C;
  const u64 *bs = a.best + (size_t)i * C * HW;
  const u64 *kn = a.states + (size_t)n * S * HW;
  int *key = a.key + (size_t)i * C;
  int n_distinct = 0, n_new = 0;
  for (int c = 0; c < C; c++) {  // (wave-uniform walk; the lanes are over the other chains)
    const double lc = bl[c];
    const u64 *wc = bs + (size_t)c * HW;
    int rank = 0x7fffffff;
    if (ais_post_finite(lc)) {
      u64 any = 0ull;
      for (int j = 0; j < HW; j++) any |= wc[j];
      int before = 0;
      bool dup = false;
      for (int c0 = 0; c0 < C; c0 += 64) {
        const int cp = c0 + lane;
        const double lp = cp < C ? bl[cp] : NAN;
        const bool ahead = ais_post_finite(lp) && (lp > lc || (lp == lc && cp < c));  // ranked before chain c
        bool eq = ahead;
        const u64 *wp = bs + (size_t)(ahead ? cp : 0) * HW;
        for (int j = 0; j < HW; j++) eq = eq && wp[j] == wc[j];
        before += __popcll(__ballot(ahead));
        dup = dup || __ballot(eq) != 0ull;
      }
      if (any != 0ull && !dup) {
        n_distinct++;
        if (!ais_post_kn_holds(kn, S, HW, wc, lane)) n_new++, rank = before;
      }
    }
    if (lane == 0) key[c] = rank;
  }
  seed_wave_sync();  // key, written by lane 0, is read by every lane
  for (int c = 0; c < C; c++) {
    const int rank = key[c];
    if (rank == 0x7fffffff) continue;  // (wave-uniform)
    int place = 0;  // the new chains ranked before this one
    for (int c0 = 0; c0 < C; c0 += 64) {
      const int cp = c0 + lane;
      place += __popcll(__ballot(cp < C && key[cp] < rank));
    }
    if (place >= Cmax) continue;
    const u64 *wc = bs + (size_t)c * HW;
    u64 *dst = a.cand + ((size_t)n * Cmax + place) * HW;
    for (int j = lane; j < HW; j += 64) dst[j] = wc[j];
    if (a.cand_dig && lane == 0) a.cand_dig[(size_t)n * Cmax + place] = make_digest(wc, HW);
  }
  const bool held = ais_post_kn_holds(kn, S, HW, bs + (size_t)ais_post_top_chain(bl, C, lane) * HW, lane);
  if (lane == 0) {
    const int np = n_new < Cmax ? n_new : Cmax;
    a.cand_counts[n] = np;
    a.n_distinct[i] = n_distinct, a.n_new[i] = n_new, a.n_proposed[i] = np, a.map_held[i] = held ? 1 : 0;
    if (a.F_full) a.F_out[i] = a.F_full[n];
  }
}

// after the selection: the proposed states K^n now holds, and map_state again (the args of the emission, map_held the
// array for `after`)
__global__ __launch_bounds__(64 * AIS_POST_ADMIT_WAVES) void ais_post_tally_kernel(AisPostAdmitArgs a) {
  const int lane = lane_id(), wave = wave_id_uniform();
  const i64 i = (i64)blockIdx.x * AIS_POST_ADMIT_WAVES + wave;
  if (i >= a.n) return;  // (wave-uniform)
  const int C = a.C, S = a.S, HW = a.HW, Cmax = a.Cmax;
  const i64 n = a.index ? a.index[i] : i;
  const u64 *kn = a.states + (size_t)n * S * HW;
  const int np = a.n_proposed[i];
  int adm = 0;
  for (int k = 0; k < np; k++)
    if (ais_post_kn_holds(kn, S, HW, a.cand + ((size_t)n * Cmax + k) * HW, lane)) adm++;
  const double *bl = a.best_lpj + (size_t)i * C;
  const bool held = ais_post_kn_holds(kn, S, HW, a.best + ((size_t)i * C + ais_post_top_chain(bl, C, lane)) * HW, lane);
  if (lane == 0) {
    a.n_admitted[i] = adm, a.map_held[i] = held ? 1 : 0;
    if (a.F_full) a.F_out[i] = a.F_full[n];
  }
}
