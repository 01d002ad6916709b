// Posterior-predictive moments per entry: for every datapoint n and observable d, over the states s of K^n (and the
// permanent all-zero state) with the weights q_ns of the statistics pass,
//
//   mean[n, d] = sum_s q_ns m_ns,d            var[n, d] = sum_s q_ns ((m_ns,d - mean[n, d])^2 + v_ns,d)  (+ sigma^2)
//
//   EBSC   m_ns = W s, v_ns = 0.
//   ES3C   A = active latents of s (k of them), o = the datapoint's reliable entries (all of them for complete data):
//          G_A = W_oA^T W_oA, Lam = (I + Psi_AA G_A / sigma2)^-1 Psi_AA  (= (Psi_AA^-1 + G_A / sigma2)^-1),
//          kappa = mu_A + Lam (W_oA^T y_o - G_A mu_A) / sigma2,  m_ns = W_A kappa,  v_ns,d = w_dA^T Lam w_dA  (>= 0: clamped).
//
// Mapping: one wavefront per datapoint, PRED_WAVES per workgroup; lane l owns the observables d = l, l + 64, ... (R of
// them in registers: running mean, centred second moment M2 and within-state variance), so every row of W^T is read
// coalesced.  The states are visited in slot order; a state of weight exactly 0 (exp underflow) is skipped after its
// decode.  The moments are updated with the weighted Welford recurrence
//   W' = W + e,  delta = m - mean,  mean += (e / W') delta,  M2 += (W e / W') delta^2,  Vw += e v
// with e = exp(lpj_s - max lpj): every term of M2 and Vw is a product of non-negative factors, so var - noise >= 0.
// ES3C: the k x (2k + 1) system [T | Psi_AA | Psi_AA v] lives in the wave's slice of LDS (row stride 2k + 1) and is
// reduced by Gauss-Jordan elimination with partial pivoting (largest magnitude, lowest row among equals); before that
// Psi_AA alone goes through an LU with the same pivoting.  An exactly zero (or non-finite) pivot in either marks the
// datapoint singular: both of its rows are NaN (the criterion of the ES3C lpj levels: a zero pivot of the pivoted LU).
// G_A comes from the resident W^T W table (complete data) or from masked dot products over the reliable entries
// (wave reductions); W_oA^T y_o is the datapoint's row of B = Y W (missing entries of Y hold 0 on the device).
// status[n]: PRED_OK, PRED_SINGULAR, PRED_SKIPPED (no reliable entry: NaN rows) or PRED_OVER_K | k << 8 (a state with
// k > PRED_MAX_K active latents: NaN rows; the host turns it into an error).  Every sum has a fixed order: no atomics,
// the same input gives the same bits.  LDS per wave: kcap (2 kcap + 1) + 2 kcap + 16 doubles, kcap = min(H, PRED_MAX_K):
// 17280 bytes at kcap = 32.
#pragma once
#include "common.hpp"

#define PRED_MAX_K 32
#define PRED_WAVES 4
#define PRED_R_MAX 8  // registers per lane: D <= 64 * PRED_R_MAX
enum { PRED_OK = 0, PRED_SINGULAR = 1, PRED_SKIPPED = 2, PRED_OVER_K = 3 };

struct PredArgs {
  const uint8_t *mask;     // (N, D) reliable entries, NULL for complete data
  const uint8_t *row_any;  // (N) datapoint has a reliable entry, NULL for complete data
  const double *lpj;       // (N, L)
  const u64 *states;       // (N, S, HW)
  const double *Wt;        // (H, D)
  const double *G, *Psi, *mus;  // ES3C: (H, H), (H, H), (H)
  const double *Bm;        // ES3C: (N, H) B = Y W
  i64 N;
  int D, H, HW, S, S_perm, L, kcap;
  int bg;                  // background unit: latent H - 1 is active in every state
  double sigma2;           // the noise variance (EBSC: sigma^2)
  int add_noise;
  double *mean, *var;      // (N, D)
  int *status;             // (N)
};

__host__ __device__ static inline size_t pred_lds_doubles(int kcap, bool sssc) {
  return (sssc ? (size_t)kcap * (2 * kcap + 1) + 2 * (size_t)kcap : 0) + PRED_MAX_K / 2;
}

// First lane (lowest index) whose flag is set; 64 when none is.
__device__ __forceinline__ int pred_first_lane(bool flag) {
  const u64 m = __ballot(flag);
  return m ? __ffsll((long long)m) - 1 : 64;
}

// Pivot of column p among the rows p .. k - 1 of the LDS matrix M (row stride ld): the row of largest magnitude, the
// lowest among equals.  Returns false (uniformly) when that magnitude is zero or not finite.
__device__ __forceinline__ bool pred_pivot(const double *M, int ld, int k, int p, int lane, int &piv) {
  const bool mine = lane >= p && lane < k;
  const double av = mine ? fabs(M[lane * ld + p]) : -1.0;
  const double mx = wave_max(av);
  piv = pred_first_lane(mine && av == mx);
  if (piv >= k) piv = p;
  return mx > 0.0 && mx <= 1.7976931348623157e308;
}

__device__ __forceinline__ void pred_swap_rows(double *M, int ld, int c0, int c1, int p, int piv, int lane) {
  if (piv == p) return;
  for (int c = c0 + lane; c < c1; c += 64) {
    const double t = M[p * ld + c];
    M[p * ld + c] = M[piv * ld + c];
    M[piv * ld + c] = t;
  }
  lds_wave_fence();
}

// ES3C state terms of one state (idx[0..k), 1 <= k <= kcap) into LDS: on return M[r ld + k + c] = Lam[r][c] and
// kap[r] = kappa_r.  Returns false (uniformly) for a singular system.
__device__ __forceinline__ bool pred_solve(const PredArgs &a, const i64 n, const int k, const int *idx, double *M, double *vv,
                                           double *kap, const int lane) {
  const int ld = 2 * k + 1, H = a.H;
  const double s2inv = 1.0 / a.sigma2;
  int piv;
  // ---- is Psi_AA exactly singular?  LU with partial pivoting on a copy in the left block
  for (int i = 0; i < k; i++)
    for (int c = lane; c < k; c += 64) M[i * ld + c] = a.Psi[(i64)idx[i] * H + idx[c]];
  lds_wave_fence();
  for (int p = 0; p < k; p++) {
    if (!pred_pivot(M, ld, k, p, lane, piv)) return false;
    pred_swap_rows(M, ld, p, k, p, piv, lane);
    const double d = M[p * ld + p];
    if (lane > p && lane < k) M[lane * ld + p] = M[lane * ld + p] / d;  // the multipliers, in place
    lds_wave_fence();
    const int c = p + 1 + lane;  // k <= 32: one column per lane
    if (c < k) {
      const double top = M[p * ld + c];
      for (int i = p + 1; i < k; i++) M[i * ld + c] = fma(-M[i * ld + p], top, M[i * ld + c]);
    }
    lds_wave_fence();
  }
  // ---- G_A into the middle block
  if (a.mask) {
    const uint8_t *mrow = a.mask + n * a.D;
    for (int i = 0; i < k; i++) {
      const double *wi = a.Wt + (i64)idx[i] * a.D;
      for (int j = i; j < k; j++) {
        const double *wj = a.Wt + (i64)idx[j] * a.D;
        double s = 0.0;
        for (int d = lane; d < a.D; d += 64)
          if (mrow[d]) s = fma(wi[d], wj[d], s);
        s = wave_sum(s);
        if (lane == 0) {
          M[i * ld + k + j] = s;
          M[j * ld + k + i] = s;
        }
      }
    }
  } else {
    for (int i = 0; i < k; i++)
      for (int c = lane; c < k; c += 64) M[i * ld + k + c] = a.G[(i64)idx[i] * H + idx[c]];
  }
  lds_wave_fence();
  // ---- v = W_oA^T y_o - G_A mu_A
  if (lane < k) {
    double s = a.Bm[n * H + idx[lane]];
    for (int j = 0; j < k; j++) s = fma(-M[lane * ld + k + j], a.mus[idx[j]], s);
    vv[lane] = s;
  }
  lds_wave_fence();
  // ---- T = I + Psi_AA G_A / sigma2 (left block), Psi_AA v (last column); row i on lane i
  if (lane < k) {
    const double *prow = a.Psi + (i64)idx[lane] * H;
    for (int j = 0; j < k; j++) {
      double t = 0.0;
      for (int l = 0; l < k; l++) t = fma(prow[idx[l]], M[l * ld + k + j], t);
      M[lane * ld + j] = fma(s2inv, t, j == lane ? 1.0 : 0.0);
    }
    double w = 0.0;
    for (int l = 0; l < k; l++) w = fma(prow[idx[l]], vv[l], w);
    M[lane * ld + 2 * k] = w;
  }
  lds_wave_fence();  // (every read of G_A above is complete before the block is overwritten)
  for (int i = 0; i < k; i++)
    for (int c = lane; c < k; c += 64) M[i * ld + k + c] = a.Psi[(i64)idx[i] * H + idx[c]];
  lds_wave_fence();
  // ---- Gauss-Jordan: [T | Psi_AA | Psi_AA v] -> [I | Lam | Lam v]
  for (int p = 0; p < k; p++) {
    if (!pred_pivot(M, ld, k, p, lane, piv)) return false;
    pred_swap_rows(M, ld, p, ld, p, piv, lane);
    const double d = M[p * ld + p];
    for (int c = p + 1 + lane; c < ld; c += 64) {
      const double top = M[p * ld + c] / d;
      M[p * ld + c] = top;
      for (int i = 0; i < k; i++)
        if (i != p) M[i * ld + c] = fma(-M[i * ld + p], top, M[i * ld + c]);
    }
    lds_wave_fence();
  }
  if (lane < k) kap[lane] = fma(s2inv, M[lane * ld + 2 * k], a.mus[idx[lane]]);
  lds_wave_fence();
  return true;
}

template <int R, bool SSSC>
__global__ __launch_bounds__(64 * PRED_WAVES) void predictive_kernel(PredArgs a) {
  extern __shared__ double pred_lds[];
  const int lane = lane_id(), wave = wave_id_uniform();
  const i64 n = (i64)blockIdx.x * PRED_WAVES + wave;
  if (n >= a.N) return;  // whole waves leave; nothing below synchronises across waves
  const int D = a.D, H = a.H, kcap = a.kcap;
  double *slice = pred_lds + (size_t)wave * pred_lds_doubles(kcap, SSSC);
  double *M = slice, *vv = slice + (SSSC ? kcap * (2 * kcap + 1) : 0), *kap = vv + (SSSC ? kcap : 0);
  int *idx = (int *)(kap + (SSSC ? kcap : 0));  // PRED_MAX_K ints
  double *mean_o = a.mean + n * D, *var_o = a.var + n * D;
  const double nan = __builtin_nan("");

  int bad = PRED_OK;
  if (a.row_any && !a.row_any[n]) bad = PRED_SKIPPED;

  double mean[R], M2[R], Vw[R];
#pragma unroll
  for (int r = 0; r < R; r++) mean[r] = M2[r] = Vw[r] = 0.0;
  double Wsum = 0.0;

  const double *lrow = a.lpj + n * a.L;
  double mx = -INFINITY;
  for (int s = lane; s < a.L; s += 64) mx = fmax(mx, lrow[s]);
  mx = wave_max(mx);

  for (int sl = 0; sl < a.L && bad == PRED_OK; sl++) {
    const double e = exp(lrow[sl] - mx);
    // ---- the state's active latents, ascending, into idx[]
    int k = 0;
    if (sl >= a.S_perm) {
      const u64 *sp = a.states + (n * a.S + (sl - a.S_perm)) * (i64)a.HW;
      for (int w = 0; w < a.HW; w++) {
        u64 bits = sp[w];
        if (a.bg && w == ((H - 1) >> 6)) bits |= 1ull << (63 - ((H - 1) & 63));
        if (w == a.HW - 1 && (H & 63)) bits &= ~0ull << (64 - (H & 63));  // (no latent beyond H)
        const bool on = (bits >> (63 - lane)) & 1ull;
        const u64 m = __ballot(on);
        const int pos = k + __popcll(m & ((1ull << lane) - 1ull));
        if (on && pos < PRED_MAX_K) idx[pos] = w * 64 + lane;
        k += __popcll(m);
      }
      lds_wave_fence();
    }
    if (k > PRED_MAX_K) {
      bad = PRED_OVER_K | (k << 8);
      break;
    }
    if (!(e > 0.0) && e == e) continue;  // weight exactly 0: the state changes nothing (a NaN weight goes on and poisons the row)
    if (SSSC && k > 0 && !pred_solve(a, n, k, idx, M, vv, kap, lane)) {
      bad = PRED_SINGULAR;
      break;
    }
    const int ld = 2 * k + 1;
    const double Wnew = Wsum + e, rr = e / Wnew, cf = Wsum * rr;
#pragma unroll
    for (int r = 0; r < R; r++) {
      const int d = lane + 64 * r;
      double m = 0.0, v = 0.0;
      if (d < D) {
        if (SSSC) {
          for (int i = 0; i < k; i++) {
            const double wi = a.Wt[(i64)idx[i] * D + d];
            m = fma(wi, kap[i], m);
            double t = 0.0;
            for (int c = 0; c < k; c++) t = fma(M[i * ld + k + c], a.Wt[(i64)idx[c] * D + d], t);
            v = fma(wi, t, v);
          }
          v = v < 0.0 ? 0.0 : v;  // w^T Lam w >= 0: rounding may leave -1e-17 (a NaN stays a NaN)
        } else {
          for (int i = 0; i < k; i++) m += a.Wt[(i64)idx[i] * D + d];
        }
      }
      const double delta = m - mean[r];
      mean[r] = fma(rr, delta, mean[r]);
      M2[r] = fma(cf * delta, delta, M2[r]);
      Vw[r] = fma(e, v, Vw[r]);
    }
    Wsum = Wnew;
    if (SSSC) lds_wave_fence();  // the next state overwrites M / kap / idx
  }

  const double noise = a.add_noise ? a.sigma2 : 0.0;
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int d = lane + 64 * r;
    if (d < D) {
      mean_o[d] = bad ? nan : mean[r];
      var_o[d] = bad ? nan : (M2[r] + Vw[r]) / Wsum + noise;
    }
  }
  if (lane == 0) a.status[n] = bad;
}
