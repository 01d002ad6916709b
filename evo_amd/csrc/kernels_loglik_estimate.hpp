// Log-likelihood beyond K^n by importance draws (evoamd_loglik_estimate): for every datapoint n, T states drawn from a
// factorised proposal r_n centred on q_n's own marginals; the draws that K^n does not hold are evaluated by the model's
// own lpj launches and folded, in the log domain, onto the bound F_n:
//   Z^_n = sum_{s in K^n} e^{lpj_ns} + (1 / T) sum_t 1[s_t not in K^n] e^{lpj(s_t)} / r_n(s_t),    ll^_n = log Z^_n.
// r_n > 0 on every state, so E[Z^_n] = sum over ALL states of e^{lpj_n(s)}: unbiased in the likelihood, ll^_n >= F_n for
// every datapoint and seed, E[ll^_n] <= log p(y_n) - ljc (Jensen).
//
// THE LAW (evo_amd/models/loglik_estimate.py: estimate_log_likelihood_counter is its NumPy mirror -- keep the two and the
// tests in step).  With i = first_index + n the datapoint's index in the whole data set, x0 = mix64(seed +
// 0x9e3779b97f4a7c15 (i + 1)) (the first hash of evoamd_generate / evoamd_posterior_sample), P = LLE_PURPOSE, Hv = H -
// background, L = S_perm + S and lambda = prior_mix:
//   weights    e_j = codes_exp(lpj_nj - max_j lpj_nj) (kernels_codes.hpp), C = e_0 + e_1 + ... in slot order: the weights of
//              evoamd_posterior_sample and its "bad weights" rule (a NaN or +inf in the row, or C = 0: no estimate).
//   marginals  p_h = (sum_j e_j [s_jh]) / C for h < Hv, j ascending over the S states of K^n (the permanent all-zero
//              column contributes nothing).
//   proposal   rho_h = fl(fl((1 - lambda) p_h) + fl(lambda pi_h)) -- two products and one sum, never an FMA; pi_h = pies[h]
//              (ES3C) or pi (EBSC).  0 < pi_h < 1, so 0 < rho_h < 1.
//   draw       s_th = u01(x0, P, t Hv + h) < rho_h.  Draw t depends neither on T nor on the passes.  The background latent
//              is on in every draw and has no factor in r.
//   density    log r_t = sum_{h < Hv} (s_th ? log rho_h : log1p(-rho_h)): per lane over its latents ascending, then wave_sum.
//   inside     s_t is inside when all its words equal those of a state of K^n (a 64-bit hash pre-filters, the full words
//              decide), or when it is the all-zero state and S_perm >= 1.  An outside all-zero draw (S_perm = 0, no
//              background) takes the value of allzero_lpj_kernel.  Draws are NOT de-duplicated among themselves.
//   terms      a_t = lpj(s_t) - log r_t for the outside draws, lpj from the model's own kernels with the clamp of
//              lpj_reset_check; lR = logsumexp_{t outside} a_t - log T, -inf when no draw is outside.
//   result     ll^_n = logsumexp(F_n, lR) (F_n: posterior_score_kernel's), mass_outside = exp(lR - ll^_n),
//              ess = (sum w)^2 / sum w^2 with w_t = exp(a_t - max a).  Everything stays in the log domain: a running
//              (m, z, q) with z = sum exp(a - m), q = sum exp(2 (a - m)), rescaled when m grows (as exact_fold_kernel).
// The draws, inside / outside and n_outside are the mirror's bit for bit; the real-valued outputs agree to rounding.
//
// Mapping.  lle_proposal_kernel<KH>: one wavefront per datapoint, LLE_WAVES per workgroup.  The wave's LDS slice holds the L
// weights in slot order and one 64-bit hash per state of K^n.  Lane l owns the latents h = l + 64 k, k < KH (KH = the
// power of two >= ceil(H / 64), at most 16: H <= 1024): it walks the S states in slot order -- the state words are
// wave-uniform loads -- and adds e_j where its bit is set, the mirror's order per latent; rho, log rho and log1p(-rho)
// stay in 3 KH registers.  Only the first pass of a call forms status, weights and marginals; it leaves rho (N x 64 KH
// doubles) and the state hashes (N x S) in global memory and the later passes read them back -- the same bits.  Per
// draw of the pass the lanes make their bits, __ballot packs word k (bit-reversed into the device layout of K^n: latent
// h in word h / 64 at bit 63 - h % 64), wave_sum forms log r_t, the draw's hash is compared
// with the S hashes (lane j + 64 i holds state j + 64 i) and a hit is settled on the full words.  Outside draws are
// appended compacted, in draw order, to the resident candidate batch (words, digest, count) with their log r and t.  No
// atomics; every sum has a fixed order.  lle_fold_kernel / lle_finish_kernel: one wavefront per datapoint, four per
// workgroup, lanes striding over the pass's terms; the finish kernel leaves per-workgroup partial sums of ll^_n for
// reduce_partials_kernel.
#pragma once
#include "common.hpp"
#include "gemm_f64.hpp"  // (kernels_mstep.hpp, which has DP_PI, needs its vector types)
#include "kernels_codes.hpp"
#include "kernels_generate.hpp"
#include "kernels_mstep.hpp"

#define LLE_PURPOSE 0x4C4C450000000000ull  // "LLE"
#define LLE_WAVES 4
#define LLE_MAX_KH 16                      // H <= 64 LLE_MAX_KH
#define LLE_LDS_MAX (64 * 1024)            // LLE_WAVES (L + S) 8 bytes must fit
enum { LLE_OK = 0, LLE_SKIPPED = 1, LLE_BAD_WEIGHTS = 2 };  // status[n]

struct LleArgs {
  const double *lpj;       // (N, L)
  const u64 *states;       // (N, S, HW)
  const double *pies;      // (H), ES3C; nullptr: dpar[DP_PI]
  const double *dpar;
  const uint8_t *row_any;  // incomplete data: the datapoint has a reliable entry; nullptr: all have
  i64 N, T, t0;            // draws t0 .. t0 + P - 1 of T
  int H, Hv, HW, S, S_perm, L, bg, P, Cmax;
  double lam, oml;         // lambda and fl(1 - lambda)
  u64 seed, first_index;
  u64 *cand;               // (N, Cmax, HW) the outside draws of the pass, compacted
  u64 *cand_dig;           // (N, Cmax) or nullptr
  int *counts;             // (N)
  double *logr;            // (N, Cmax)
  int *tix;                // (N, Cmax): t, or -(t + 1) for the all-zero draw (its slot holds a stand-in state)
  int *status;             // (N)
  double *rho;             // (N, KH, 64): rho of latent 64 k + lane, written by the pass with t0 = 0, read by the others
  u64 *hash;               // (N, S): the hashes of K^n's states, likewise
  u64 *keep_s;             // (N, T, HW) or nullptr
  uint8_t *keep_inside;    // (N, T)
  double *keep_logr;       // (N, T)
};

// word w of state j of K^n the way every kernel reads it: the background unit on, no latent beyond H
__device__ __forceinline__ u64 lle_state_word(const LleArgs &a, i64 n, int j, int w) {
  u64 bits = a.states[(n * a.S + j) * (i64)a.HW + w];
  if (a.bg && w == ((a.H - 1) >> 6)) bits |= 1ull << (63 - ((a.H - 1) & 63));
  if (w == a.HW - 1 && (a.H & 63)) bits &= ~0ull << (64 - (a.H & 63));
  return bits;
}
__device__ __forceinline__ u64 lle_hash_step(u64 x, u64 word, int w) {
  return mix64(x ^ (word + 0x9e3779b97f4a7c15ull * (u64)(w + 1)));
}

template <int KH>
__global__ __launch_bounds__(64 * LLE_WAVES) void lle_proposal_kernel(LleArgs a) {
  extern __shared__ double lle_lds[];
  const int lane = lane_id(), wave = wave_id_uniform();
  const i64 n = (i64)blockIdx.x * LLE_WAVES + wave;
  if (n >= a.N) return;  // whole waves leave; nothing below synchronises across waves
  const int H = a.H, Hv = a.Hv, HW = a.HW, S = a.S, L = a.L;
  double *wgt = lle_lds + (size_t)wave * (size_t)(L + S);
  u64 *hsh = (u64 *)(wgt + L);
  const double *lrow = a.lpj + n * L;

  // The first pass (t0 = 0) forms the status and rho and leaves both in global memory; the later passes read them back
  // (the same bits), so weights and marginals are formed once per call, not once per pass.
  const bool first = a.t0 == 0;  // (uniform over the launch)
  double *rho_n = a.rho + n * (i64)(64 * KH);  // [k][lane]: a coalesced row per k
  u64 *hsh_n = a.hash + n * (i64)S;
  for (int j = lane; j < S; j += 64) {
    u64 x = 0;
    if (first) {  // (the later passes read S hashes instead of the S x HW words of K^n)
      for (int w = 0; w < HW; w++) x = lle_hash_step(x, lle_state_word(a, n, j, w), w);
      hsh_n[j] = x;
    } else {
      x = hsh_n[j];
    }
    hsh[j] = x;
  }
  int bad = LLE_OK;
  double acc[KH];
#pragma unroll
  for (int k = 0; k < KH; k++) acc[k] = 0.0;
  double C = 1.0;
  if (first) {
    if (a.row_any && !a.row_any[n]) bad = LLE_SKIPPED;
    double mx = -INFINITY;
    bool poison = false;
    for (int s = lane; s < L; s += 64) {
      const double v = lrow[s];
      mx = fmax(mx, v);
      poison = poison || v != v || v == INFINITY;
    }
    mx = wave_max(mx);
    if (bad == LLE_OK && __ballot(poison)) bad = LLE_BAD_WEIGHTS;
    for (int s = lane; s < L; s += 64) wgt[s] = codes_exp(lrow[s] - mx);
    lds_wave_fence();
    C = 0.0;
    for (int j = 0; j < L; j++) C = C + wgt[j];
    if (bad == LLE_OK && !(C > 0.0)) bad = LLE_BAD_WEIGHTS;
  } else {
    bad = a.status[n];
    lds_wave_fence();
  }
  if (bad != LLE_OK) {  // no estimate: the kept rows stay as the caller cleared them
    if (lane == 0) a.counts[n] = 0, a.status[n] = bad;
    return;
  }
  if (first) {
    // ---- marginals over K^n: lane l adds e_j where latent l + 64 k is on, j ascending
    for (int j = 0; j < S; j++) {
      const double e = wgt[a.S_perm + j];
      if (e == 0.0) continue;  // (uniform; adding 0 changes nothing)
      const u64 *sp = a.states + (n * S + j) * (i64)HW;
#pragma unroll
      for (int k = 0; k < KH; k++)
        if (k < HW) {
          const u64 bits = sp[k];  // uniform address
          if ((bits >> (63 - lane)) & 1ull) acc[k] = acc[k] + e;
        }
    }
  }
  double rho[KH], lr1[KH], lr0[KH];
#pragma unroll
  for (int k = 0; k < KH; k++) {
    const int h = lane + 64 * k;
    rho[k] = 0.0, lr1[k] = 0.0, lr0[k] = 0.0;
    if (h < Hv) {
      if (first) {
        const double p = acc[k] / C;
        const double pi = a.pies ? a.pies[h] : a.dpar[DP_PI];
        rho[k] = __dadd_rn(__dmul_rn(a.oml, p), __dmul_rn(a.lam, pi));
        rho_n[64 * k + lane] = rho[k];
      } else {
        rho[k] = rho_n[64 * k + lane];
      }
      lr1[k] = log(rho[k]);
      lr0[k] = log1p(-rho[k]);
    }
  }

  const u64 x0 = mix64(a.seed + 0x9e3779b97f4a7c15ull * (a.first_index + (u64)n + 1));
  const int bgw = a.bg ? ((H - 1) >> 6) : -1;
  const u64 bgbit = 1ull << (63 - ((H - 1) & 63));
  int cnt = 0;
  for (int i = 0; i < a.P; i++) {
    const i64 t = a.t0 + i;
    u64 wd[KH];
    double lrs = 0.0;
    u64 any = 0;
#pragma unroll
    for (int k = 0; k < KH; k++) {
      const int h = lane + 64 * k;
      bool on = false;
      if (h < Hv) {
        on = gen_u01(x0, LLE_PURPOSE, (u64)t * (u64)Hv + (u64)h) < rho[k];
        lrs += on ? lr1[k] : lr0[k];
      }
      wd[k] = __brevll(__ballot(on));
      any |= wd[k];
      if (k == bgw) wd[k] |= bgbit;
    }
    const double lr = wave_sum(lrs);
    const bool zero = !a.bg && any == 0;  // (uniform)
    bool inside = false;
    if (zero && a.S_perm >= 1) {
      inside = true;  // the permanent all-zero state
    } else {  // (an all-zero draw too: with S_perm = 0, K^n may hold the all-zero state as an ordinary row)
      u64 hx = 0;
#pragma unroll
      for (int k = 0; k < KH; k++)
        if (k < HW) hx = lle_hash_step(hx, wd[k], k);
      for (int j0 = 0; j0 < S && !inside; j0 += 64) {
        const int j = j0 + lane;
        bool hit = j < S && hsh[j] == hx;
        if (hit) {
#pragma unroll
          for (int k = 0; k < KH; k++)
            if (k < HW) hit = hit && lle_state_word(a, n, j, k) == wd[k];
        }
        inside = __ballot(hit) != 0;
      }
    }
    u64 mine = 0;  // word `lane` of the draw
#pragma unroll
    for (int k = 0; k < KH; k++)
      if (lane == k) mine = wd[k];
    if (!inside) {
      const i64 slot = n * (i64)a.Cmax + cnt;
      // the all-zero draw takes allzero_lpj_kernel's value in the fold; its slot holds a stand-in (latent 0 alone)
      if (lane < HW) a.cand[slot * HW + lane] = (zero && lane == 0) ? 0x8000000000000000ull : mine;
      if (a.cand_dig) {
        u64 d = 0;
        int dk = 0, total = 0;
#pragma unroll
        for (int k = 0; k < KH; k++)
          if (k < HW) {
            u64 v = (zero && k == 0) ? 0x8000000000000000ull : wd[k];
            total += __popcll(v);
            while (v && dk < DIG_SLOTS) digest_add(d, dk, k * 64 + pop_msb(v));
          }
        if (lane == 0) a.cand_dig[slot] = digest_close(d, total);
      }
      if (lane == 0) {
        a.logr[slot] = lr;
        a.tix[slot] = zero ? -(int)t - 1 : (int)t;
      }
      cnt++;
    }
    if (a.keep_s) {
      const i64 r = n * a.T + t;
      if (lane < HW) a.keep_s[r * HW + lane] = mine;
      if (lane == 0) a.keep_inside[r] = inside ? 1 : 0, a.keep_logr[r] = lr;
    }
  }
  if (lane == 0) a.counts[n] = cnt, a.status[n] = LLE_OK;
}

// Folds the terms a_j = lpj_j - log r_j of one pass (j < counts[n], slot order = draw order) into the running
// (m, z, q, count) of every datapoint; `first`: the running values start here.  Lane l takes the terms l, l + 64, ... in
// ascending order, wave_max / wave_sum join the lanes in their fixed trees.  keep_lpj (N, T) or nullptr: the lpj of
// every outside draw at its t.
__global__ __launch_bounds__(256) void lle_fold_kernel(const double *__restrict__ cand_lpj, int Cmax,
                                                       const int *__restrict__ counts, const double *__restrict__ logr,
                                                       const int *__restrict__ tix, const double *__restrict__ az, i64 N,
                                                       i64 T, int first, double *__restrict__ run_m,
                                                       double *__restrict__ run_z, double *__restrict__ run_q,
                                                       int *__restrict__ nout, double *__restrict__ keep_lpj) {
  const int lane = lane_id(), wave = wave_id_uniform();
  const i64 n = (i64)blockIdx.x * 4 + wave;
  if (n >= N) return;  // wave-uniform
  int cnt = counts[n];
  if (cnt > Cmax) cnt = Cmax;
  const double m_old = first ? -INFINITY : run_m[n];
  const double z_old = first ? 0.0 : run_z[n], q_old = first ? 0.0 : run_q[n];
  const int c_old = first ? 0 : nout[n];
  double cm = -INFINITY;
  for (int j = lane; j < cnt; j += 64) {
    const i64 s = n * (i64)Cmax + j;
    const int tt = tix[s];
    const double v = tt < 0 ? az[n] : cand_lpj[s];
    cm = fmax(cm, v - logr[s]);
    if (keep_lpj) keep_lpj[n * T + (tt < 0 ? -(tt + 1) : tt)] = v;
  }
  cm = wave_max(cm);
  const double m_new = fmax(m_old, cm);
  double z = z_old, q = q_old;
  if (m_new != -INFINITY && cnt > 0) {
    const double scale = (m_old == -INFINITY) ? 0.0 : exp(m_old - m_new);
    double tz = 0.0, tq = 0.0;
    for (int j = lane; j < cnt; j += 64) {
      const i64 s = n * (i64)Cmax + j;
      const double v = tix[s] < 0 ? az[n] : cand_lpj[s];
      const double w = exp((v - logr[s]) - m_new);
      tz += w;
      tq += w * w;
    }
    z = z_old * scale + wave_sum(tz);
    q = q_old * (scale * scale) + wave_sum(tq);
  }
  if (lane == 0) {
    run_m[n] = m_new;
    run_z[n] = z;
    run_q[n] = q;
    nout[n] = c_old + cnt;
  }
}

// ll^_n = logsumexp(F_n, lR), lR = m + log z - log T (-inf without an outside draw: ll^_n = F_n exactly), the share of
// Z^_n from outside K^n, the effective number of outside draws, and the per-block partial sums of ll^_n (datapoints
// without an estimate: NaN in ll, mass, ess and F -- the bound posterior_score_kernel left is overwritten --, nothing added).
__global__ __launch_bounds__(256) void lle_finish_kernel(double *__restrict__ F, const double *__restrict__ run_m,
                                                         const double *__restrict__ run_z, const double *__restrict__ run_q,
                                                         const int *__restrict__ nout, const int *__restrict__ status, i64 N,
                                                         double logT, double *__restrict__ ll, double *__restrict__ mass,
                                                         double *__restrict__ ess, double *__restrict__ partial) {
  __shared__ double wsum[4];
  const int lane = lane_id(), wave = wave_id_uniform();
  const i64 n = (i64)blockIdx.x * 4 + wave;
  double f = 0.0;
  if (n < N && lane == 0) {
    if (status[n] != LLE_OK) {
      const double nan = __builtin_nan("");
      ll[n] = nan, mass[n] = nan, ess[n] = nan, F[n] = nan;
    } else {
      const double Fn = F[n], z = run_z[n], q = run_q[n];
      const double lR = (nout[n] > 0 && z > 0.0) ? run_m[n] + log(z) - logT : -INFINITY;
      double v = Fn;
      if (lR != -INFINITY) {
        const double mm = fmax(Fn, lR);
        v = mm + log(exp(Fn - mm) + exp(lR - mm));
      }
      ll[n] = v;
      mass[n] = lR == -INFINITY ? 0.0 : exp(lR - v);
      ess[n] = q > 0.0 ? (z * z) / q : 0.0;
      f = v;
    }
  }
  if (lane == 0) wsum[wave] = f;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}
