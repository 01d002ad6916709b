// Local search on K^n: every one-flip neighbour of the best states of K^n scored, one wavefront per datapoint
// (evoamd_sweep_propose / evoamd_sweep_states).  Deterministic, no random numbers, no atomics.
// evo_amd/variational/utils.py: sweep_states_host is the NumPy mirror -- keep the two and the tests in step.
//
// THE LAW, per datapoint n and per sweep (P = n_parents, q = n_keep, Hv = H varying latents):
//   parents     the P varying states of K^n with the largest lpj of the row, descending lpj, ties by ascending slot (the
//               permanent all-zero column of S_perm = 1 is no parent); parent r has the active set p_r, m = |p_r|
//   neighbours  p_r with bit j flipped, for every j < Hv.  Not scored (key 0, "absent"), tested in this order: (a) the
//               all-zero state; (b) a state K^n holds already: some resident s with popcount(s XOR p_r) = 1 and that bit at
//               j, an exact test on the packed words; (c) a state above the model's cap (SEED_MAX_A_SSSC = 8 / SEED_MAX_A_BSC =
//               64 active latents, the seeding kernel's).  n_capped[n] counts the parents that lost a neighbour to (c).
//   scores      the model's lpj of the neighbour in the Gram form of kernels_seed.hpp, without ljc and without the
//               lpj_reset_check clamp; not finite, or (ES3C) det T <= 0: absent.
//               EBSC  c_j = B_nj - sum_{i in p} G_ij (ascending i), base = pre1 (yy - sum_{a in p} (B_na + c_a)) + m pil_bar
//                     [= pre1 (yy - 2 sum B_na + sum_{a,a'} G_aa') + m pil_bar],
//                     add j: base + pil_bar + pre1 (G_jj - 2 c_j); remove a: base - pil_bar + pre1 (G_aa + 2 c_a)
//               ES3C  additions (m <= 7): seed_score_sssc<m + 1> bordered on the blocks of p_r in LDS, one lane per j;
//                     removals (2 <= m <= 9): the (m - 1) x (m - 1) system from scratch, lane a removes the a-th active
//                     latent; base (1 <= m <= 8): the m x m system from scratch; a parent 0 above 8 latents has no base
//   choice      per parent the q best scored neighbours (fewer when fewer are scored), descending score, ties by ascending
//               j: seed_rank_keys, the threshold search of the seeding kernel
//   emission    parent-major, then rank order, into rows 0 .. counts[n] - 1 of the candidate batch, with their digests (k
//               and the first DIG_SLOTS ascending active latents) where digests are in use; duplicates between the lists of
//               two parents stay in (vary_kn_kernel removes them, first occurrence wins)
//   certificate from parent 0: best_flip[n] = the j of its best scored neighbour or -1, gain[n] = that score - base or
//               -inf (NaN: scored, but parent 0 has no base).  gain <= 0: the best state of K^n has no better one-flip
//               neighbour outside K^n (a held one cannot be better, or it would be the best state).
// The scores only rank: the lpj of the emitted rows comes from the model's own lpj kernels afterwards.
// INCOMPLETE DATA (the MASKED instantiations; evoamd_sweep_*_ex with EVOAMD_SWEEP_INCOMPLETE and masks resident): the same
// law -- parents, neighbours and the tests (a), (b), (c), choice, emission, certificate, n_capped, the caps 8 / 64 -- with
// the Gram quantities of the datapoint's reliable entries o = x_infr[n], as in the masked seeding law of kernels_seed.hpp:
// G(n) = sum_{d in o} W_d. W_d.^T replaces G; B_n and yy_n are what evoamd_upload_masks leaves (it zeroes the missing entries
// of Y, so NaN there is never read as a number); Psi, mu, pil_bar, sigma2 and pre1 are not masked.  This is the lpj of the
// reference's W[this_x_infr, :] branches, which evoamd_lpj_resident and the candidate lpj kernels compute on masked data.  A
// datapoint without a reliable entry needs no special case: G(n) = 0, B_n = 0, yy_n = 0, it is scored by the prior alone
// and ties go to ascending j.  The summation orders are fixed, so two launches give the same bits:
//   reliable d  an ascending list in LDS (ballots), as in seed_states_masked_kernel; every sum over d runs down that list
//               (seed_gram_sweep: fma, four chunks of latents at a time)
//   EBSC        g_jj = sum_{d in o} W_dj^2 once per datapoint, shared by all P parents.  Per parent ONE sweep with a combined
//               column in place of the m rows of G: r_d = sum_{i in p, ascending i} W_di for the reliable d, staged in LDS;
//               c_j = B_nj - sum_{d in o, ascending d} r_d W_dj.  base and the add / remove scores are the expressions above
//               with g_jj for G_jj.  Cost per datapoint: the diagonal sweep and P sweeps of |o| H multiply-adds (plus
//               P |o| m gathers for r), independent of m in the sweeps.
//   ES3C        per datapoint the diagonal, per parent the rows G(n)_{a,.} of its first min(m, 9) active latents in the order
//               of its list (none when m > 9: nothing of that parent is scored) -- row i: the column W_.a staged in LDS, then
//               g_aj = sum_d W_da W_dj.  Additions border the parent's blocks through seed_form_blocks(.., rows) and
//               seed_score_sssc_step<true>; removals and the base are the from-scratch elimination sweep_lpj_scratch<K, true>,
//               which takes G entries from the rows (entry (i, l) from the row of i) and Psi from GP[..].y.  The SWEEP_ROWS
//               = 10 rows live in LDS while one wavefront's share fits the 150 KB the launch attributes allow, else in a
//               per-wavefront buffer of the context with a smaller grid, as the seeding kernel's rows.  A row is formed
//               anew for every parent (no reuse between the parents of a datapoint).
// Mapping: lane l owns latents l, l + 64, ...; parents by P rounds of a wave-wide lexicographic maximum below the last
// pick; the membership test marks held flips in the key array (S HW words per parent, lane s takes states s, s + 64, ..).
// LDS per wave: keys (Hp u64), EBSC c_j (Hp doubles), the parent's words (HW), ES3C the shared blocks (SeedShared), the
// members' keys and two lists of their latents (q each), the parent's active latents (SWEEP_PATH ints) and the parents'
// slots (64 ints); incomplete data adds EBSC g_jj (Hp doubles), the staged column (D doubles), ES3C the rows (10 Hp doubles,
// when LDS is their home) and the list of the reliable d (D ints).  Every latent index, entry index d and slot that crossed
// LDS passes guard_index before it becomes an address.
// Cost: EBSC P m rows of G per datapoint (L2-resident at H <= 1024) and P S HW words for the membership; ES3C about
// P H (k^3 / 3 + 4 k^2) multiply-adds: bound by vector issue, not by HBM.
#pragma once
#include "common.hpp"
#include "kernels_seed.hpp"

#define SWEEP_ROWS (SEED_MAX_A_SSSC + 2)  // incomplete data, ES3C: the rows of G(n) of a parent's first 9 active latents and its diagonal

struct SweepArgs {
  SeedArgs sd;          // states (K^n, read only), Bm, yy, G, Gd, GP, GPt, mus, pil_bar, dpar, err, N, S, H, HW, Hp; Q = q
  const double *lpj;    // (N, L) the rows of K^n
  u64 *cand;            // (N, Cmax, HW)
  u64 *cand_dig;        // (N, Cmax) or nullptr
  int *counts;          // (N)
  double *score;        // (N, Cmax) or nullptr: the score of every emitted row
  int *best_flip;       // (N)
  double *gain;         // (N)
  int *n_capped;        // (N)
  int L, S_perm, P, q, Cmax;
};

// ES3C lpj of the state idx[0..K-1] for one datapoint, eliminated from scratch by the calling lane.  The K x K blocks of
// {G, Psi} are read where they are used (the few entries stay in the cache): held in registers beside the system they
// would not fit the register file at K = 8.
// MASKED (incomplete data): G is the datapoint's own -- G(n)_{idx[i], idx[l]} = rows[pos[i] * Hp + idx[l]], pos[i] the place of
// idx[i] in the parent's list of active latents (the kernel forms one row per place); only Psi comes from the table.
template <int K, bool MASKED = false>
__device__ __forceinline__ double sweep_lpj_scratch(const SeedArgs &a, const int *idx, const double *__restrict__ Bn, double yy,
                                                    double s2inv, const double *rows = nullptr, const int *pos = nullptr) {
  auto gram = [&](int i, int l) -> double {
    if constexpr (MASKED)
      return rows[(size_t)pos[i] * a.Hp + idx[l]];
    else
      return a.GP[(size_t)idx[i] * a.H + idx[l]].x;
  };
  double mu[K], b[K], v[K];
  double pb = 0.0, rr = yy;
#pragma unroll
  for (int i = 0; i < K; i++) {
    mu[i] = a.mus[idx[i]], b[i] = Bn[idx[i]];
    pb += a.pil_bar[idx[i]];
  }
#pragma unroll
  for (int i = 0; i < K; i++) {
    double s = b[i];
#pragma unroll
    for (int l = 0; l < K; l++) s -= gram(i, l) * mu[l];
    v[i] = s;
    rr -= mu[i] * (b[i] + s);
  }
  double t[K][K + 1];
#pragma unroll
  for (int i = 0; i < K; i++) {
    double pi[K], rhs = 0.0;
#pragma unroll
    for (int u = 0; u < K; u++) {
      pi[u] = a.GP[(size_t)idx[i] * a.H + idx[u]].y;
      rhs += pi[u] * v[u];
    }
#pragma unroll
    for (int l = 0; l < K; l++) {
      double s = 0.0;
#pragma unroll
      for (int u = 0; u < K; u++) s += pi[u] * gram(u, l);
      t[i][l] = (i == l ? 1.0 : 0.0) + s2inv * s;
    }
    t[i][K] = rhs;
  }
  return seed_eliminate<K>(t, v, pb, rr, s2inv);
}

// path[0..m-1] without entry `skip` (skip < 0: all of them), k = the length of that list, 1 <= k <= 8
template <bool MASKED = false>
__device__ __forceinline__ double sweep_lpj_scratch_k(int k, const SeedArgs &a, const int *path, int skip, const double *__restrict__ Bn,
                                                      double yy, double s2inv, const double *rows = nullptr) {
  int idx[SEED_MAX_A_SSSC], pos[SEED_MAX_A_SSSC];
#pragma unroll
  for (int i = 0; i < SEED_MAX_A_SSSC; i++) {
    const int src = (skip >= 0 && i >= skip) ? i + 1 : i;
    idx[i] = i < k ? guard_index(path[src], a.H, a.err) : 0;
    pos[i] = i < k ? src : 0;
  }
  switch (k) {
    case 1: return sweep_lpj_scratch<1, MASKED>(a, idx, Bn, yy, s2inv, rows, pos);
    case 2: return sweep_lpj_scratch<2, MASKED>(a, idx, Bn, yy, s2inv, rows, pos);
    case 3: return sweep_lpj_scratch<3, MASKED>(a, idx, Bn, yy, s2inv, rows, pos);
    case 4: return sweep_lpj_scratch<4, MASKED>(a, idx, Bn, yy, s2inv, rows, pos);
    case 5: return sweep_lpj_scratch<5, MASKED>(a, idx, Bn, yy, s2inv, rows, pos);
    case 6: return sweep_lpj_scratch<6, MASKED>(a, idx, Bn, yy, s2inv, rows, pos);
    case 7: return sweep_lpj_scratch<7, MASKED>(a, idx, Bn, yy, s2inv, rows, pos);
    default: return sweep_lpj_scratch<8, MASKED>(a, idx, Bn, yy, s2inv, rows, pos);
  }
}

// the key of a score that may be proposed; 0 (absent) for one that is not finite
__device__ __forceinline__ u64 sweep_key(double sc) { return fabs(sc) <= 1.7976931348623157e308 ? seed_key(sc) : 0ull; }

__device__ __forceinline__ u64 sweep_wave_max_u64(u64 v) {
  const unsigned hi = wave_max_u32((unsigned)(v >> 32));
  const unsigned lo = wave_max_u32((unsigned)(v >> 32) == hi ? (unsigned)v : 0u);
  return ((u64)hi << 32) | lo;
}

// The parents of a datapoint (file header): round r takes the largest (lpj, -slot) of the row below the pick of round
// r - 1; their slots go to parents[0..P-1].  The caller synchronises before it reads them.
__device__ __forceinline__ void sweep_pick_parents(const double *row, int S, int P, int lane, int *parents) {
  u64 pk = 0ull;
  int ps = -1;
  for (int r = 0; r < P; r++) {
    u64 bk = 0ull;
    int bs = 0x7fffffff;
    for (int s = lane; s < S; s += 64) {
      const u64 k = seed_key(row[s]);
      const bool elig = r == 0 || k < pk || (k == pk && s > ps);
      if (elig && k > bk) bk = k, bs = s;  // (ascending s: an equal key later in the lane's list never wins)
    }
    const u64 gk = sweep_wave_max_u64(bk);
    const int gs = (int)wave_min_u32(bk == gk ? (unsigned)bs : 0x7fffffffu);
    if (lane == 0) parents[r] = gs;
    pk = gk, ps = gs;
  }
}

// The words pw of a parent into par[]; returns its size (wave-uniform).  The caller synchronises before par is read.
__device__ __forceinline__ int sweep_load_parent(const u64 *pw, int HW, int lane, u64 *par) {
  int m = 0;
  for (int w = lane; w < HW; w += 64) {
    const u64 v = pw[w];
    par[w] = v;
    m += __popcll(v);
  }
  return wave_sum_i(m);
}

// The active latents of the words par[] in ascending order into list[] (the first cap of them; ballots)
__device__ __forceinline__ void sweep_list_active(const u64 *par, int H, int NC, int lane, int *list, int cap) {
  int pos = 0;
  for (int c = 0; c < NC && pos < cap; c++) {
    const int j = 64 * c + lane;
    const bool on = j < H && ((par[j < H ? j >> 6 : 0] >> (63 - (j & 63))) & 1ull);
    const u64 b = __ballot(on);
    const int at = pos + __popcll(b & ((1ull << lane) - 1ull));
    if (on && at < cap) list[at] = j;
    pos += __popcll(b);
  }
}

// One parent scored (file header: neighbours, the tests (a), (b), (c), scores): the words of the state in `slot` go to
// L.base, its first SWEEP_PATH active latents to L.path, and L.keys[j] becomes the key of the neighbour that flips j, 0 for an
// absent one.  Returns the parent's size m; lost: this lane saw a neighbour lost to the cap; base: the parent's own score.
// gd, col, rows, dl, nd: incomplete data, as the kernels set them up.  OWN (kernels_nbound.hpp, rule (d)): rank[s] is the
// parent rank of slot s or INT_MAX, r this parent's rank; a neighbour that an earlier parent owns is absent, not lost.
template <bool SSSC, bool MASKED, bool OWN>
__device__ __forceinline__ int sweep_score_parent(const SeedArgs &sd, const SeedLds &L, const SeedScalars &sc, const u64 *kn, int slot,
                                                  int lane, const double *__restrict__ Bn, double yy, double *gd, double *col,
                                                  double *rows, const int *dl, int nd, int r, const int *rank, bool &lost_out,
                                                  double &base_out) {
  const int S = sd.S, H = sd.H, HW = sd.HW, Hp = sd.Hp;
  const int NC = Hp >> 6;
  constexpr int CAP = SSSC ? SEED_MAX_A_SSSC : SEED_MAX_A_BSC;
  const double pre1 = sc.pre1, pilb = sc.pilb, s2inv = sc.s2inv;
  u64 *keys = L.keys, *par = L.base;
  double *cc = L.cc;
  int *path = L.path;
  const u64 *pw = kn + (size_t)slot * HW;
  // ---- the parent's words, its size, the keys cleared
  const int m = sweep_load_parent(pw, HW, lane, par);
  for (int c = 0; c < NC; c++) keys[64 * c + lane] = 0ull;
  seed_wave_sync();
  // ---- (b) flips that K^n holds: key 1 marks them (no score has that key).  OWN, (d): an earlier parent two flips away
  // sets bit 1 of both differing latents (LDS atomics: a latent may be held and owned; a held one keeps bit 0, which wins)
  for (int s0 = 0; s0 < S; s0 += 64) {
    const int s = s0 + lane;
    if (s < S) {
      const u64 *sw = kn + (size_t)s * HW;
      int cnt = 0, at = 0, last = 0;
      for (int w = 0; w < HW; w++) {
        const u64 x = sw[w] ^ par[w];
        if constexpr (OWN) {
          if (x) {
            if (cnt == 0) at = 64 * w + __clzll((long long)x);
            last = 64 * w + 63 - __builtin_ctzll(x);
          }
        } else {
          if (x) at = 64 * w + __clzll((long long)x);
        }
        cnt += __popcll(x);
      }
      if constexpr (OWN) {
        if (cnt == 1 && at < H) atomicOr((unsigned long long *)&keys[at], 1ull);
        if (cnt == 2 && last < H && rank[s] < r) {
          atomicOr((unsigned long long *)&keys[at], 2ull);
          atomicOr((unsigned long long *)&keys[last], 2ull);
        }
      } else {
        if (cnt == 1 && at < H) keys[at] = 1ull;
      }
    }
  }
  // the mark of latent j before its key is written: held (b), owned (d; never without OWN)
  auto is_held = [&](u64 mk) { return OWN ? (mk & 1ull) != 0 : mk == 1ull; };
  auto is_owned = [&](u64 mk) { return OWN && mk == 2ull; };
  // ---- the parent's active latents in ascending order (the first SWEEP_PATH of them)
  sweep_list_active(par, H, NC, lane, path, SWEEP_PATH);
  seed_wave_sync();
  const bool add_ok = m + 1 <= CAP, rem_ok = m - 1 >= 1 && m - 1 <= CAP;
  bool lost = false;   // a neighbour neither all-zero nor held, above the cap
  double base;
  if (SSSC) {
    if constexpr (MASKED) {
      // row i of G(n) for the parent's i-th active latent, m <= 9 (above that nothing of this parent is scored): the
      // column W_.a staged in LDS, then the sweep over the reliable d
      const int nr = m <= CAP + 1 ? m : 0;
      for (int i = 0; i < nr; i++) {
        const int ja = guard_index(__builtin_amdgcn_readfirstlane(path[i]), H, sd.err);
        for (int t = lane; t < nd; t += 64) col[t] = sd.W[(size_t)guard_index(dl[t], sd.D, sd.err) * H + ja];
        seed_wave_sync();
        seed_gram_sweep<false>(sd, lane, dl, col, nd, rows + (size_t)i * Hp);
        seed_wave_sync();  // the column is staged again; the rows are read by other lanes
      }
    }
    // removals: lane i takes the i-th active latent out, base: every lane the same system
    if (m >= 2 && m <= CAP + 1) {
      if (lane < m) {
        const int ja = guard_index(path[lane], H, sd.err);
        u64 key = 0ull;
        const u64 mk = keys[ja];
        if (!is_held(mk) && !is_owned(mk)) key = sweep_key(sweep_lpj_scratch_k<MASKED>(m - 1, sd, path, lane, Bn, yy, s2inv, rows));
        keys[ja] = key;
      }
    } else if (m == 1) {
      if (lane == 0) keys[guard_index(path[0], H, sd.err)] = 0ull;  // (a)
    } else if (m > CAP + 1) {  // every removal is above the cap
      for (int c = 0; c < NC; c++) {
        const int j = 64 * c + lane;
        const bool on = j < H && ((par[j < H ? j >> 6 : 0] >> (63 - (j & 63))) & 1ull);
        if (on) {
          lost = lost || !is_held(keys[j]);
          keys[j] = 0ull;
        }
      }
    }
    base = m == 0 ? -0.5 * yy * s2inv
                  : (m <= CAP ? sweep_lpj_scratch_k<MASKED>(m, sd, path, -1, Bn, yy, s2inv, rows) : __builtin_nan(""));
    // additions, bordered on the parent's blocks
    int act[SEED_MAX_A_SSSC];
    double pbA = 0.0;
    if (add_ok) pbA = seed_form_blocks(sd, L, m + 1, lane, Bn, s2inv, act, MASKED ? rows : nullptr);
    for (int c = 0; c < NC; c++) {
      const int j = 64 * c + lane;
      if (j >= H) continue;
      if ((par[j >> 6] >> (63 - (j & 63))) & 1ull) continue;  // a removal: done above
      const u64 mk = keys[j];
      const bool held = is_held(mk);
      lost = lost || (!held && !add_ok);
      u64 key = 0ull;
      if (!held && add_ok && !is_owned(mk))
        key = sweep_key(seed_score_sssc_step<MASKED>(m + 1, sd, L.sh, act, pbA, j, Bn, yy, s2inv, MASKED ? rows : nullptr));
      keys[j] = key;
    }
  } else {
    if constexpr (MASKED) {
      // the combined column r_d = sum_{i in p} W_di (ascending i) for the reliable d, then ONE sweep:
      // c_j = B_nj - sum_d r_d W_dj (ascending d)
      for (int t = lane; t < nd; t += 64) {
        const double *Wd = sd.W + (size_t)guard_index(dl[t], sd.D, sd.err) * H;
        double s = 0.0;
        for (int w = 0; w < HW; w++) {
          u64 v = par[w];
          while (v) s += Wd[guard_index(64 * w + pop_msb(v), H, sd.err)];
        }
        col[t] = s;
      }
      seed_wave_sync();
      seed_gram_sweep<false>(sd, lane, dl, col, nd, cc);
      for (int c = 0; c < NC; c++) {
        const int j = 64 * c + lane;
        cc[j] = (j < H ? Bn[j] : 0.0) - cc[j];
      }
    } else
    // c_j = B_nj - sum_{i in p} G_ij, the rows in ascending i, four chunks of latents at a time
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
    {
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
    for (int c = 0; c < NC; c++) {
      const int j = 64 * c + lane;
      if (j >= H) continue;
      const bool on = (par[j >> 6] >> (63 - (j & 63))) & 1ull;
      const u64 mk = keys[j];
      const bool held = is_held(mk);
      const bool zero = on && m == 1;  // (a)
      const bool ok = on ? rem_ok : add_ok;
      lost = lost || (!zero && !held && !ok);
      u64 key = 0ull;
      if (!zero && !held && ok && !is_owned(mk)) {
        const double gjj = MASKED ? gd[j] : sd.Gd[j], cj = cc[j];
        key = sweep_key(on ? base - pilb + pre1 * (gjj + 2.0 * cj) : base + pilb + pre1 * (gjj - 2.0 * cj));
      }
      keys[j] = key;
    }
  }
  lost_out = lost;
  base_out = base;
  return m;
}

// MASKED: the law on incomplete data (file header); the complete instantiations compile to what they were without it.
template <bool SSSC, bool MASKED = false>
__global__ __launch_bounds__(256) void sweep_neighbours_kernel(SweepArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sweep_lds[];
  const SeedArgs &sd = a.sd;
  const int lane = lane_id(), wave = wave_id_uniform();
  const int W = (int)(blockDim.x >> 6);
  const int S = sd.S, H = sd.H, HW = sd.HW, Hp = sd.Hp, P = a.P, q = a.q, Cmax = a.Cmax;
  const int NC = Hp >> 6;
  // one wavefront's share of LDS (seed_lds_walk)
  const SeedLdsView V = MASKED ? seed_lds_view(sweep_lds, wave, SEED_LDS_FLIP_MASKED, SeedLdsShape{SSSC, Hp, HW, q, 0, 0, sd.D, sd.rows ? 0 : sd.R, 0})
                               : seed_lds_view(sweep_lds, wave, SEED_LDS_FLIP, SeedLdsShape{SSSC, Hp, HW, q, 0, 0, 0, 0, 0});
  const SeedLds L = seed_carve(V);
  int *parents = V.parents;
  // incomplete data: the diagonal of G(n), the staged column, ES3C the rows of G(n) (row SWEEP_ROWS - 1: the diagonal), the reliable d
  double *gd = nullptr, *col = nullptr, *rows = nullptr;
  int *dl = nullptr;
  if constexpr (MASKED) {
    col = V.col, dl = V.dl;
    rows = sd.rows ? sd.rows + ((size_t)blockIdx.x * W + wave) * sd.R * Hp : V.rows;
    gd = SSSC ? rows + (size_t)(sd.R - 1) * Hp : V.gd;
  }
  u64 *keys = L.keys, *par = L.base;
  const SeedScalars sc = seed_scalars<SSSC>(sd.dpar);
  for (i64 n = (i64)blockIdx.x * W + wave; n < sd.N; n += (i64)gridDim.x * W) {
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
    // ---- parents
    sweep_pick_parents(row, S, P, lane, parents);
    seed_wave_sync();
    int row0 = 0, capped_parents = 0;
    for (int r = 0; r < P; r++) {
      const int slot = guard_index(__builtin_amdgcn_readfirstlane(parents[r]), S, sd.err);
      bool lost;
      double base;
      const int m = sweep_score_parent<SSSC, MASKED, false>(sd, L, sc, kn, slot, lane, Bn, yy, gd, col, rows, dl, nd, 0, nullptr, lost, base);
      if (__any(lost)) capped_parents++;
      seed_wave_sync();
      // ---- the q best scored neighbours
      int scored = 0;
      for (int c = 0; c < NC; c++) scored += __popcll(__ballot(keys[64 * c + lane] != 0ull));
      const int qe = scored < q ? scored : q;
      if (qe > 0) {
        seed_rank_keys(L, Hp, qe, q, lane);
        u64 *dst = a.cand + ((size_t)n * Cmax + row0) * HW;
        for (int idx = lane; idx < qe * HW; idx += 64) {
          const int rk = idx / HW, w = idx - rk * HW;
          const int j = guard_index(L.byrank[rk], H, sd.err);
          dst[(size_t)rk * HW + w] = par[w] ^ ((j >> 6) == w ? (0x8000000000000000ull >> (j & 63)) : 0ull);
        }
        for (int rk = lane; rk < qe; rk += 64) {
          const int j = guard_index(L.byrank[rk], H, sd.err);
          if (a.score) a.score[(size_t)n * Cmax + row0 + rk] = seed_unkey(keys[j]);
          if (a.cand_dig) {
            const bool on = (par[j >> 6] >> (63 - (j & 63))) & 1ull;
            u64 d = 0;
            int dk = 0;
            for (int w = 0; w < HW && dk < DIG_SLOTS; w++) {
              u64 v = par[w] ^ ((j >> 6) == w ? (0x8000000000000000ull >> (j & 63)) : 0ull);
              while (v && dk < DIG_SLOTS) digest_add(d, dk, w * 64 + pop_msb(v));
            }
            a.cand_dig[(size_t)n * Cmax + row0 + rk] = digest_close(d, on ? m - 1 : m + 1);
          }
        }
      }
      if (r == 0 && lane == 0) {  // the certificate
        int jb = -1;
        double gn = -__builtin_inf();
        if (qe > 0) {
          jb = guard_index(L.byrank[0], H, sd.err);
          gn = seed_unkey(keys[jb]) - base;
        }
        a.best_flip[n] = jb;
        a.gain[n] = gn;
      }
      row0 += qe;
      seed_wave_sync();  // everybody has read keys / par / byrank
    }
    if (lane == 0) {
      a.counts[n] = row0;
      a.n_capped[n] = capped_parents;
    }
  }
}
