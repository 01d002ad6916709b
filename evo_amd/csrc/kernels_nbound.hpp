// Neighbourhood bound (evoamd_neighbour_bound): the exact mass of the one-flip neighbours of the best states of K^n, summed
// instead of ranked.  A deterministic lower bound on log p(y_n) - ljc above the bound F_n of K^n itself, with no variance:
//   F+_n = log( sum_{s in K^n} e^{lpj_ns} + sum_{s in Nb_n} e^{lpj_n(s)} ),   F_n <= F+_n <= log p(y_n) - ljc,
// Nb_n = the states one flip away from any of the P best states of K^n that K^n does not hold, each counted exactly once.
// One wavefront per datapoint; no random numbers, no atomics on global memory; nothing of the EM state is written.
// evo_amd/variational/utils.py: neighbour_bound_host is the NumPy mirror -- keep the two and the tests in step.
//
// THE LAW, per datapoint n (P = n_parents, 1 <= P <= S; Hv = H varying latents):
//   parents     those of the flip law of kernels_sweep.hpp, but up to S of them: the P varying states with the largest lpj of
//               the row, descending lpj, ties by ascending slot.  Parent r has the active set p_r, m = |p_r|.
//   neighbours  p_r with bit j flipped, for every j < Hv.  Absent under any of these tests, applied in this order:
//               (a) the all-zero state; (b) a state K^n holds; (c) a state above the model's cap (SEED_MAX_A_SSSC = 8 /
//               SEED_MAX_A_BSC = 64 active latents), n_capped[n] counts the parents that lost a neighbour to (c);
//               (d) a state an earlier parent owns: some r' < r has popcount(p_r XOR p_r') = 2 and j is one of the two
//               differing bits (that state is p_r' with the other bit flipped).  All four are exact tests on the packed
//               words.  A state of the union that K^n does not hold is one flip away from parents that are pairwise two
//               flips apart, so (d) leaves it to the first of them: with (b), every state of Nb_n is counted exactly once.
//   scores      the flip law's, from the same device function (sweep_score_parent): the model's lpj of the neighbour in the
//               Gram form, without ljc and without the clamp; not finite, or (ES3C) det T <= 0: absent.
//   result      M_n = log sum exp(score) over the present neighbours, -inf without one; F_n = the logsumexp of the row, as
//               posterior_score_kernel forms it; F+_n = logaddexp(F_n, M_n); n_states[n] the neighbours summed;
//               best_score[n], best_parent[n] (the rank r) and best_flip[n] of the largest present score, ties by ascending
//               r, then ascending j; -inf / -1 / -1 without one.  "Bad weights", the rule of kernels_loglik_estimate.hpp (a NaN
//               or +inf in the row, or every entry -inf): no estimate -- F, M and F+ NaN, the counts 0, best -inf / -1 / -1.
//   order       fixed by the mapping: lane l owns latents l, l + 64, ... and keeps a running (max, sum) over its present
//               neighbours in parent order, then ascending j; one wave reduction joins the lanes (wave_max, then wave_sum of
//               the rescaled sums in its fixed tree).  Two launches give the same bits.
// INCOMPLETE DATA (the MASKED instantiations; EVOAMD_NBOUND_INCOMPLETE and masks resident): the same law with G(n), g_jj and
// the rows of the masked flip law, set up as sweep_neighbours_kernel<.., true> does.
// LDS per wave (SEED_LDS_NBOUND / SEED_LDS_NBOUND_MASKED of seed_lds_walk): the flip / masked flip share with n_keep = 0, S parent
// slots and the slot -> parent rank table (S ints, INT_MAX for a state that is no parent).  Rule (d) rides in the membership
// pass over the S resident states: a resident state that is an earlier parent two flips away marks both differing bits.
// Every index that crossed LDS passes guard_index before it becomes an address.
// Cost: the flip sweep's with P up to S and without the ranking and the emission.
#pragma once
#include "common.hpp"
#include "kernels_sweep.hpp"

struct NboundArgs {
  SeedArgs sd;          // states (K^n, read only), Bm, yy, G, Gd, GP, GPt, mus, pil_bar, dpar, err, N, S, H, HW, Hp; masked: W, mask, rows
  const double *lpj;    // (N, L) the rows of K^n
  double *F;            // (N) in: posterior_score_kernel's bound; out: NaN for a row with bad weights
  double *M;            // (N)
  double *F_plus;       // (N)
  double *best_score;   // (N)
  int *n_states;        // (N)
  int *n_capped;        // (N)
  int *best_parent;     // (N)
  int *best_flip;       // (N)
  int L, S_perm, P;
};

template <bool SSSC, bool MASKED = false>
__global__ __launch_bounds__(256) void nbound_kernel(NboundArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char nbound_lds[];
  const SeedArgs &sd = a.sd;
  const int lane = lane_id(), wave = wave_id_uniform();
  const int W = (int)(blockDim.x >> 6);
  const int S = sd.S, H = sd.H, HW = sd.HW, Hp = sd.Hp, P = a.P;
  const int NC = Hp >> 6;
  // one wavefront's share of LDS (seed_lds_walk)
  const SeedLdsView V = MASKED ? seed_lds_view(nbound_lds, wave, SEED_LDS_NBOUND_MASKED, SeedLdsShape{SSSC, Hp, HW, 0, 0, 0, sd.D, sd.rows ? 0 : sd.R, S})
                               : seed_lds_view(nbound_lds, wave, SEED_LDS_NBOUND, SeedLdsShape{SSSC, Hp, HW, 0, 0, 0, 0, 0, S});
  const SeedLds L = seed_carve(V);
  int *parents = V.parents, *rank = V.rank;
  double *gd = nullptr, *col = nullptr, *rows = nullptr;
  int *dl = nullptr;
  if constexpr (MASKED) {
    col = V.col, dl = V.dl;
    rows = sd.rows ? sd.rows + ((size_t)blockIdx.x * W + wave) * sd.R * Hp : V.rows;
    gd = SSSC ? rows + (size_t)(sd.R - 1) * Hp : V.gd;
  }
  const u64 *keys = L.keys;
  const SeedScalars sc = seed_scalars<SSSC>(sd.dpar);
  for (i64 n = (i64)blockIdx.x * W + wave; n < sd.N; n += (i64)gridDim.x * W) {
    // ---- bad weights: no estimate
    {
      const double *lrow = a.lpj + (size_t)n * a.L;
      bool poison = false, any = false;
      for (int s = lane; s < a.L; s += 64) {
        const double v = lrow[s];
        poison = poison || v != v || v == INFINITY;
        any = any || v > -INFINITY;
      }
      if (__any(poison) || !__any(any)) {  // (wave-uniform)
        if (lane == 0) {
          const double nan = __builtin_nan("");
          a.F[n] = nan, a.M[n] = nan, a.F_plus[n] = nan, a.best_score[n] = -INFINITY;
          a.n_states[n] = 0, a.n_capped[n] = 0, a.best_parent[n] = -1, a.best_flip[n] = -1;
        }
        continue;
      }
    }
    const double *Bn = sd.Bm + (size_t)n * H;
    const double yy = sd.yy[n];
    const double *row = a.lpj + (size_t)n * a.L + a.S_perm;
    const u64 *kn = sd.states + (size_t)n * S * HW;
    int nd = 0;  // incomplete data: the reliable d in ascending order, then g_jj = sum over them of W_dj^2
    if constexpr (MASKED) {
      nd = seed_list_reliable(sd.mask + (size_t)n * sd.D, sd.D, lane, dl);
      seed_wave_sync();
      seed_gram_sweep<true>(sd, lane, dl, col, nd, gd);
    }
    // ---- parents and the slot -> rank table
    for (int s = lane; s < S; s += 64) rank[s] = 0x7fffffff;
    seed_wave_sync();
    sweep_pick_parents(row, S, P, lane, parents);
    seed_wave_sync();
    for (int r = lane; r < P; r += 64) rank[guard_index(parents[r], S, sd.err)] = r;
    seed_wave_sync();
    // ---- the lane's running (max, sum), count and best over its latents, parent-major
    double mx = -INFINITY, sum = 0.0;
    int cnt = 0, capped_parents = 0, br = 0x7fffffff, bj = 0x7fffffff;
    u64 bkey = 0ull;
    for (int r = 0; r < P; r++) {
      const int slot = guard_index(__builtin_amdgcn_readfirstlane(parents[r]), S, sd.err);
      bool lost;
      double base;
      sweep_score_parent<SSSC, MASKED, true>(sd, L, sc, kn, slot, lane, Bn, yy, gd, col, rows, dl, nd, r, rank, lost, base);
      if (__any(lost)) capped_parents++;
      seed_wave_sync();
      for (int c = 0; c < NC; c++) {
        const int j = 64 * c + lane;
        const u64 key = keys[j];
        if (key == 0ull) continue;
        const double v = seed_unkey(key);  // finite (sweep_key)
        if (v > mx) {
          sum = sum * exp(mx - v) + 1.0;  // (the first one: 0 * exp(-inf) + 1)
          mx = v;
        } else {
          sum += exp(v - mx);
        }
        cnt++;
        if (key > bkey) bkey = key, br = r, bj = j;  // (ascending r, then j: an equal key later never wins)
      }
      seed_wave_sync();  // everybody has read the keys
    }
    // ---- one wave reduction
    const double gm = wave_max(mx);
    const double z = wave_sum(cnt > 0 ? sum * exp(mx - gm) : 0.0);
    const int total = wave_sum_i(cnt);
    const u64 gk = sweep_wave_max_u64(bkey);
    const unsigned gr = wave_min_u32(bkey == gk ? (unsigned)br : 0x7fffffffu);
    const unsigned gj = wave_min_u32(bkey == gk && (unsigned)br == gr ? (unsigned)bj : 0x7fffffffu);
    if (lane == 0) {
      const double Fn = a.F[n];
      const double Mn = total > 0 ? gm + log(z) : -INFINITY;
      double Fp = Fn;
      if (total > 0) {
        const double mm = fmax(Fn, Mn);
        Fp = mm + log(exp(Fn - mm) + exp(Mn - mm));
      }
      a.M[n] = Mn, a.F_plus[n] = Fp;
      a.best_score[n] = total > 0 ? seed_unkey(gk) : -INFINITY;
      a.n_states[n] = total, a.n_capped[n] = capped_parents;
      a.best_parent[n] = total > 0 ? (int)gr : -1;
      a.best_flip[n] = total > 0 ? (int)gj : -1;
    }
  }
}
