// Local search on K^n, the swap neighbourhood: one active latent of a best state switched off and one inactive latent
// switched on, every such pair scored, one wavefront per datapoint (evoamd_sweep_propose_nb / evoamd_sweep_states_nb with
// EVOAMD_SWEEP_SWAP).  Complete data only.  Deterministic, no random numbers, no atomics.
// evo_amd/variational/utils.py: swap_states_host is the NumPy mirror -- keep the two and the tests in step.
//
// THE LAW, per datapoint n and per sweep (P = n_parents, q = n_keep, Hv = H varying latents):
//   parents     those of the one-flip law (kernels_sweep.hpp): the P varying states of K^n with the largest lpj of the row,
//               descending lpj, ties by ascending slot; parent r has the active set p, m = |p|
//   neighbours  p with a in p switched off and j not in p switched on, for every (a, j), j < Hv.  The size stays m, so the
//               all-zero state never arises.  Not scored ("absent"): (b) a state K^n holds already: some resident s with
//               popcount(s XOR p) = 2, one of the two bits in p at a and the other at j, an exact test on the packed words;
//               (c) m above the model's cap (SEED_MAX_A_SSSC = 8 / SEED_MAX_A_BSC = 64 active latents): none of the parent's
//               swaps is scored and n_capped_swap[n] counts the parent; m = 0: a parent without swaps.
//   scores      the model's lpj of the neighbour in the Gram form of kernels_seed.hpp, without ljc and without the
//               lpj_reset_check clamp; not finite, or (ES3C) det T <= 0: absent.
//               EBSC  c_j and base as in the flip law; per a (ascending): base_a = base - pil_bar + pre1 (G_aa + 2 c_a),
//                     c_aj = c_j + G_aj, score(a, j) = base_a + pil_bar + pre1 (G_jj - 2 c_aj)
//                     [= base + pre1 (G_aa + G_jj + 2 c_a - 2 c_j - 2 G_aj)]
//               ES3C  (1 <= m <= 8) per a the blocks of p \ {a} (the parent's ascending list with a taken out, order kept)
//                     in LDS and seed_score_sssc<m> bordered by j, one lane per j: the addition pass of the flip kernel one
//                     size down; m = 1: the first step of the seeding kernel.  base: the m x m system from scratch.
//   choice      per parent the q best scored swaps (fewer when fewer are scored), descending score, ties by ascending a,
//               then ascending j
//   emission    behind the rows the flip stage emitted for this datapoint (append; else from row 0), parent-major, then
//               rank, with their digests (k = m and the first DIG_SLOTS ascending active latents) where digests are in use;
//               duplicates between lists stay in (vary_kn_kernel removes them, first occurrence wins)
//   certificate from parent 0: best_swap[n] = (a, j) of its best scored swap or (-1, -1), swap_gain[n] = that score - base
//               or -inf.  swap_gain <= 0: the best state of K^n has no better swap neighbour outside K^n.
// The scores only rank: the lpj of the emitted rows comes from the model's own lpj kernels afterwards.
// Mapping: lane l owns latents l, l + 64, ...  One pass per parent over K^n notes for every resident state the pair (a, j)
// it holds, if any (S words in LDS); then one pass per a: the keys of (a, .) into the key array, the q best of the pass by
// seed_rank_keys, merged by rank counting into the running list of the parent's q best so far (two buffers, swapped).  An
// earlier a wins a tie, so once the list is full a key that does not exceed its last entry is dropped before the rank
// search (most passes after the first rank few keys or none).  LDS per wave: the flip kernel's share, the running lists
// (2 q keys and 4 q ints), the parent's active latents (64 ints) and the held pairs (S words).  Every latent index and
// slot that crossed LDS passes guard_index before it becomes an address.
// Cost: EBSC m rows of G per parent on top of the flip kernel's; ES3C m addition passes of size m per parent.
#pragma once
#include "common.hpp"
#include "kernels_sweep.hpp"

#define SWAP_NONE 0xFFFFFFFFu     // a resident state that is no swap neighbour of the parent

struct SweepSwapArgs {
  SweepArgs sw;         // the flip stage's arguments; best_flip / gain / n_capped are not touched
  int *best_swap;       // (N, 2)
  double *swap_gain;    // (N)
  int *n_capped_swap;   // (N)
  int append;           // 1: the rows go behind counts[n] (the flip stage ran), 0: from row 0
};

template <bool SSSC>
__global__ __launch_bounds__(256) void sweep_swap_kernel(SweepSwapArgs A) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sweep_swap_lds[];
  const SweepArgs &a = A.sw;
  const SeedArgs &sd = a.sd;
  const int lane = lane_id(), wave = wave_id_uniform();
  const int W = (int)(blockDim.x >> 6);
  const int S = sd.S, H = sd.H, HW = sd.HW, Hp = sd.Hp, P = a.P, q = a.q, Cmax = a.Cmax;
  const int NC = Hp >> 6;
  constexpr int CAP = SSSC ? SEED_MAX_A_SSSC : SEED_MAX_A_BSC;
  // one wavefront's share of LDS: the flip kernel's layout, then the running lists, the active latents, the held pairs
  const SeedLdsView V = seed_lds_view(sweep_swap_lds, wave, SEED_LDS_SWAP, SeedLdsShape{SSSC, Hp, HW, q, 0, 0, 0, 0, S});
  const SeedLds L = seed_carve(V);
  int *parents = V.parents, *full = V.full;
  unsigned *held = V.held;
  u64 *rk0 = V.rk[0], *rk1 = V.rk[1];
  int *ra0 = V.rp[0], *rj0 = V.rj[0], *ra1 = V.rp[1], *rj1 = V.rj[1];
  u64 *keys = L.keys, *par = L.base;
  double *cc = L.cc;
  int *path = L.path;
  const auto [pre1, pilb, s2inv] = seed_scalars<SSSC>(sd.dpar);
  for (i64 n = (i64)blockIdx.x * W + wave; n < sd.N; n += (i64)gridDim.x * W) {
    const double *Bn = sd.Bm + (size_t)n * H;
    const double yy = sd.yy[n];
    const double *row = a.lpj + (size_t)n * a.L + a.S_perm;
    const u64 *kn = sd.states + (size_t)n * S * HW;
    sweep_pick_parents(row, S, P, lane, parents);
    seed_wave_sync();
    int row0 = A.append ? __builtin_amdgcn_readfirstlane(a.counts[n]) : 0;
    row0 = row0 < 0 ? 0 : (row0 > Cmax ? Cmax : row0);
    int capped_parents = 0;
    for (int r = 0; r < P; r++) {
      const int slot = guard_index(__builtin_amdgcn_readfirstlane(parents[r]), S, sd.err);
      const u64 *pw = kn + (size_t)slot * HW;
      // ---- the parent's words and its size
      const int m = sweep_load_parent(pw, HW, lane, par);
      seed_wave_sync();
      if (m > CAP) capped_parents++;  // (c)
      int nrun = 0;                   // the running list: entries 0 .. nrun - 1 of (ok, oa, oj), by rank
      u64 *ok = rk0, *nk = rk1;
      int *oa = ra0, *oj = rj0, *na = ra1, *nj = rj1;
      double base = 0.0;
      if (m >= 1 && m <= CAP) {
        // ---- the parent's active latents in ascending order (m <= CAP <= SWAP_LIST: all of them)
        sweep_list_active(par, H, NC, lane, full, SWAP_LIST);
        // ---- (b) the swap that a resident state holds: (a << 16) | j (H < 2^16: the keys of one datapoint fit LDS)
        for (int s = lane; s < S; s += 64) {
          const u64 *sw = kn + (size_t)s * HW;
          int cnt = 0, nin = 0, pa = 0, pj = 0;
          for (int w = 0; w < HW; w++) {
            const u64 x = sw[w] ^ par[w];
            const u64 xa = x & par[w], xj = x & ~par[w];
            if (xa) pa = 64 * w + __clzll((long long)xa);
            if (xj) pj = 64 * w + __clzll((long long)xj);
            cnt += __popcll(x);
            nin += __popcll(xa);
          }
          held[s] = (cnt == 2 && nin == 1 && pj < H) ? (((unsigned)pa << 16) | (unsigned)pj) : SWAP_NONE;
        }
        seed_wave_sync();
        if (SSSC) {
          if (r == 0) base = sweep_lpj_scratch_k<false>(m, sd, full, -1, Bn, yy, s2inv);  // every lane the same system
        } else {
          // c_j = B_nj - sum_{i in p} G_ij, the rows in ascending i, four chunks of latents at a time (the flip kernel's sum)
          for (int c0 = 0; c0 < NC; c0 += 4) {
            double acc[4];
            int jj[4];
            bool in[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
              const int j = 64 * (c0 + u) + lane;
              in[u] = c0 + u < NC && j < H;
              jj[u] = in[u] ? j : 0;
              acc[u] = in[u] ? Bn[jj[u]] : 0.0;
            }
            for (int w = 0; w < HW; w++) {
              u64 v = seed_uniform(par[w]);
              while (v) {
                const int i = guard_index(64 * w + pop_msb(v), H, sd.err);
                const double *Gi = sd.G + (size_t)i * H;
#pragma unroll
                for (int u = 0; u < 4; u++) acc[u] -= in[u] ? Gi[jj[u]] : 0.0;
              }
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
              if (c0 + u < NC) cc[64 * (c0 + u) + lane] = acc[u];
          }
          seed_wave_sync();
          double s = yy;  // every lane the same sum, ascending a
          for (int w = 0; w < HW; w++) {
            u64 v = seed_uniform(par[w]);
            while (v) {
              const int i = guard_index(64 * w + pop_msb(v), H, sd.err);
              s -= Bn[i] + cc[i];
            }
          }
          base = pre1 * s + (double)m * pilb;
        }
        // ---- one pass per a, ascending
        for (int ia = 0; ia < m; ia++) {
          const int ai = guard_index(__builtin_amdgcn_readfirstlane(full[ia]), H, sd.err);
          for (int c = 0; c < NC; c++) keys[64 * c + lane] = 0ull;
          if (SSSC && lane < m - 1) path[lane] = full[lane < ia ? lane : lane + 1];  // p \ {a}, order kept
          seed_wave_sync();
          for (int s = lane; s < S; s += 64) {  // key 1 marks the held swaps of this a (no score has that key)
            const unsigned h = held[s];
            const int j = (int)(h & 0xFFFFu);
            if (h != SWAP_NONE && (int)(h >> 16) == ai && j < H) keys[j] = 1ull;
          }
          seed_wave_sync();
          const u64 thr = nrun == q ? ok[q - 1] : 0ull;  // a full list: only a key above its last entry can enter
          int act[SEED_MAX_A_SSSC];
          double pbA = 0.0, base_a = 0.0;
          const double *Ga = nullptr;
          if (SSSC)
            pbA = seed_form_blocks(sd, L, m, lane, Bn, s2inv, act, nullptr);
          else {
            Ga = sd.G + (size_t)ai * H;
            base_a = base - pilb + pre1 * (sd.Gd[ai] + 2.0 * cc[ai]);
          }
          for (int c = 0; c < NC; c++) {
            const int j = 64 * c + lane;
            if (j >= H) continue;
            const bool on = (par[j >> 6] >> (63 - (j & 63))) & 1ull;
            u64 key = 0ull;
            if (!on && keys[j] != 1ull) {
              double sc;
              if (SSSC)
                sc = seed_score_sssc_step<false>(m, sd, L.sh, act, pbA, j, Bn, yy, s2inv, nullptr);
              else {
                const double caj = cc[j] + Ga[j];
                sc = base_a + pilb + pre1 * (sd.Gd[j] - 2.0 * caj);
              }
              key = sweep_key(sc);
              if (key <= thr) key = 0ull;
            }
            keys[j] = key;
          }
          seed_wave_sync();
          int live = 0;
          for (int c = 0; c < NC; c++) live += __popcll(__ballot(keys[64 * c + lane] != 0ull));
          const int qe = live < q ? live : q;
          if (qe > 0) {
            seed_rank_keys(L, Hp, qe, q, lane);
            for (int t = lane; t < qe; t += 64) L.selk[t] = keys[guard_index(L.byrank[t], H, sd.err)];  // the pass's keys by rank
            seed_wave_sync();
            // the merge: an old entry goes behind the new keys above it, a new one behind the old keys not below it
            for (int i = lane; i < nrun; i += 64) {
              const u64 k = ok[i];
              int rk = i;
              for (int t = 0; t < qe; t++) rk += L.selk[t] > k ? 1 : 0;
              if (rk < q) nk[rk] = k, na[rk] = oa[i], nj[rk] = oj[i];
            }
            for (int t = lane; t < qe; t += 64) {
              const u64 k = L.selk[t];
              int rk = t;
              for (int i = 0; i < nrun; i++) rk += ok[i] >= k ? 1 : 0;
              if (rk < q) nk[rk] = k, na[rk] = ai, nj[rk] = L.byrank[t];
            }
            seed_wave_sync();
            nrun = nrun + qe < q ? nrun + qe : q;
            u64 *tk = ok;
            ok = nk, nk = tk;
            int *ti = oa;
            oa = na, na = ti;
            ti = oj, oj = nj, nj = ti;
          }
        }
      }
      // ---- the parent's list leaves the wave
      if (row0 + nrun > Cmax) nrun = Cmax - row0;
      if (nrun > 0) {
        u64 *dst = a.cand + ((size_t)n * Cmax + row0) * HW;
        for (int idx = lane; idx < nrun * HW; idx += 64) {
          const int rk = idx / HW, w = idx - rk * HW;
          const int ja = guard_index(oa[rk], H, sd.err), j = guard_index(oj[rk], H, sd.err);
          dst[(size_t)rk * HW + w] = par[w] ^ ((ja >> 6) == w ? (0x8000000000000000ull >> (ja & 63)) : 0ull) ^
                                     ((j >> 6) == w ? (0x8000000000000000ull >> (j & 63)) : 0ull);
        }
        for (int rk = lane; rk < nrun; rk += 64) {
          if (a.score) a.score[(size_t)n * Cmax + row0 + rk] = seed_unkey(ok[rk]);
          if (a.cand_dig) {
            const int ja = guard_index(oa[rk], H, sd.err), j = guard_index(oj[rk], H, sd.err);
            u64 d = 0;
            int dk = 0;
            for (int w = 0; w < HW && dk < DIG_SLOTS; w++) {
              u64 v = par[w] ^ ((ja >> 6) == w ? (0x8000000000000000ull >> (ja & 63)) : 0ull) ^
                      ((j >> 6) == w ? (0x8000000000000000ull >> (j & 63)) : 0ull);
              while (v && dk < DIG_SLOTS) digest_add(d, dk, w * 64 + pop_msb(v));
            }
            a.cand_dig[(size_t)n * Cmax + row0 + rk] = digest_close(d, m);
          }
        }
      }
      if (r == 0 && lane == 0) {  // the certificate
        int ab = -1, jb = -1;
        double gn = -__builtin_inf();
        if (nrun > 0) {
          ab = guard_index(oa[0], H, sd.err), jb = guard_index(oj[0], H, sd.err);
          gn = seed_unkey(ok[0]) - base;
        }
        A.best_swap[2 * n] = ab, A.best_swap[2 * n + 1] = jb;
        A.swap_gain[n] = gn;
      }
      row0 += nrun > 0 ? nrun : 0;
      seed_wave_sync();  // everybody has read par / the lists
    }
    if (lane == 0) {
      a.counts[n] = row0;
      A.n_capped_swap[n] = capped_parents;
    }
  }
}
