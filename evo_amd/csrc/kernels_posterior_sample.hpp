// Posterior samples: for every datapoint n and every draw t < T a state of K^n drawn from q_n, ES3C latents drawn from
// the state's Gaussian posterior, and an observable row drawn from the likelihood (evoamd_posterior_sample).
//
// THE LAW (evo_amd/models/posterior_sample.py: sample_posterior_counter is its NumPy mirror -- keep the two and the tests
// in step).  With i = first_index + n the datapoint's index in the whole data set, x0 = mix64(seed + 0x9e3779b97f4a7c15
// (i + 1)) and P = PSAMP_PURPOSE (gen_u01 / gen_normal_pair: kernels_generate.hpp, the stream of evoamd_generate under a
// purpose of its own, far from GEN_PURPOSE, INIT_PURPOSE and the small integers of the evolve kernels):
//   weights   e_j = codes_exp(lpj_nj - max_j lpj_nj) (kernels_codes.hpp), j = 0 .. L - 1 in slot order (the permanent
//             all-zero state first); c_j = c_{j-1} + e_j in plain fp64 additions, C = c_{L-1}.  A row that holds a NaN or
//             +inf, or with C = 0 (every entry -inf), is "bad weights": no draws.
//   slot      u = gen_u01(x0, P + 0, t), target = u C; slot_t = the first j with c_j > target; none (u = 1 or rounding at
//             the top end): the last j with e_j > 0.  A slot of weight 0 is never drawn; draw t does not depend on T.
//   ES3C z    Lam and kappa of the drawn state from pred_solve (kernels_predictive.hpp); Lam' = (Lam + Lam^T) / 2;
//             L = the lower Cholesky factor of Lam'; z_A = kappa + L eps with eps_j = normal number 32 t + j of purpose
//             P + 1, j = the position in the ascending active set; z = 0 off the active set.  EBSC: z = s.
//   y         y_hat = W z (+ sigma g with the noise, g_d = normal number D t + d of purpose P + 2);
//             fill "missing": the reliable entries carry the datapoint's own y, the others y_hat; fill "all": y_hat.
//   no draws  a datapoint without a reliable entry (PRED_SKIPPED), with bad weights (PSAMP_BAD_WEIGHTS), or one of whose
//             DRAWN states has a singular system (PRED_SINGULAR; it wins over:) or a Lam' with a pivot that is <= 0 or not
//             finite (PSAMP_NOT_PD: an indefinite Psi is a supported input): slot -1, s zero, z and y NaN, all T rows.
//             A state of K^n with k > PRED_MAX_K active latents, drawn or not: PRED_OVER_K | k << 8 (the lowest slot).
// slot and s are the mirror's bit for bit; z and y agree to the rounding of the k x k arithmetic and of log / sincos.
//
// Mapping (that of predictive_kernel): one wavefront per datapoint, PRED_WAVES per workgroup, the LDS slice and the
// solve of kernels_predictive.hpp.  Draws are taken in passes of 64: lane l holds the target of draw 64 p + l.  The wave
// walks the slots once per pass with the running c_j (wave-uniform); a ballot of "my target falls into slot j" says
// whether slot j is needed at all, and the walk ends when every lane is served.  A state drawn by several lanes of a pass
// is decoded, solved and factorised ONCE (the factor overwrites the left block, which Gauss-Jordan left as I; row i on
// lane i); then each of its draws is emitted: eps into vv[], z_i = kappa_i + sum_{j <= i} L_ij eps_j on lane i (into
// the last column of the slice), the dense z row by word (lane l owns latent 64 w + l), and y with the lanes striding
// over d along the rows of W^T, R accumulators per lane.  Every sum has a fixed order, there are no atomics and every
// store is a plain vector store: the same call gives the same bits.
#pragma once
#include "common.hpp"
#include "kernels_codes.hpp"
#include "kernels_generate.hpp"
#include "kernels_predictive.hpp"

#define PSAMP_PURPOSE 0x5053414D00000000ull  // "PSAM"
enum { PSAMP_KEEP_SLOT = 1, PSAMP_KEEP_S = 2, PSAMP_KEEP_Z = 4, PSAMP_KEEP_Y = 8 };
enum { PSAMP_NOT_PD = 4, PSAMP_BAD_WEIGHTS = 5 };  // status[n], beside PRED_OK .. PRED_OVER_K

struct PsampArgs {
  PredArgs p;       // the inputs of predictive_kernel (mean, var and add_noise are not read); p.status (N) is written
  const double *Y;  // (N, D), row stride ldY; missing entries hold 0
  i64 ldY;
  i64 T;            // draws per datapoint
  u64 seed, first_index;
  int fill_all, add_noise;
  double sigma;     // the noise's standard deviation
  int *slot;        // (N, T)      any output may be nullptr
  u64 *s;           // (N, T, HW)
  double *z;        // (N, T, H), ES3C
  double *y;        // (N, T, D)
};

// word w of the state in slot sl the way every kernel reads it: the background unit on, no latent beyond H
__device__ __forceinline__ u64 psamp_word(const PredArgs &a, i64 n, int sl, int w) {
  if (sl < a.S_perm) return 0ull;
  u64 bits = a.states[(n * a.S + (sl - a.S_perm)) * (i64)a.HW + w];
  if (a.bg && w == ((a.H - 1) >> 6)) bits |= 1ull << (63 - ((a.H - 1) & 63));
  if (w == a.HW - 1 && (a.H & 63)) bits &= ~0ull << (64 - (a.H & 63));
  return bits;
}

__device__ __forceinline__ double psamp_normal(u64 x0, u64 purpose, u64 index) {
  double even, odd;
  gen_normal_pair(x0, purpose, index >> 1, even, odd);
  return (index & 1ull) ? odd : even;
}

// The state in slot sl, drawn by the lanes of m in pass `pass`: decode, (ES3C) solve + factorise, emit one row per lane
// of m.  Returns 0, 1 (singular) or 2 (not positive definite), uniformly; nothing of z / y is emitted then.
template <int R, bool SSSC>
__device__ __forceinline__ int psamp_state(const PsampArgs &q, const i64 n, const int sl, const u64 m, const int pass, const u64 x0,
                                           double *M, double *vv, double *kap, int *idx, const int lane) {
  const PredArgs &a = q.p;
  const int D = a.D, H = a.H, HW = a.HW;
  const bool mine = (m >> lane) & 1ull;
  const i64 row = n * q.T + 64 * (i64)pass + lane;  // this lane's draw (used where `mine`)
  // ---- the state's active latents, ascending, into idx[]; its words to the lanes that drew it
  int k = 0;
  for (int w = 0; w < HW; w++) {
    const u64 bits = psamp_word(a, n, sl, w);
    const bool on = (bits >> (63 - lane)) & 1ull;
    const u64 b = __ballot(on);
    const int pos = k + __popcll(b & ((1ull << lane) - 1ull));
    if (on && pos < PRED_MAX_K) idx[pos] = w * 64 + lane;
    k += __popcll(b);
    if (q.s && mine) q.s[row * HW + w] = bits;
  }
  lds_wave_fence();
  if (q.slot && mine) q.slot[row] = sl;
  if (k > PRED_MAX_K) return 1;  // (excluded by the scan of the kernel: never an address)
  const int ld = 2 * k + 1;
  if (SSSC && k > 0) {
    if (!pred_solve(a, n, k, idx, M, vv, kap, lane)) return 1;
    // ---- Lam' = (Lam + Lam^T) / 2 into the left block, then its Cholesky factor in place (right-looking, row i on lane i)
    if (lane < k)
      for (int c = 0; c < k; c++) M[lane * ld + c] = 0.5 * (M[lane * ld + k + c] + M[c * ld + k + lane]);
    lds_wave_fence();
    for (int p = 0; p < k; p++) {
      const double d = M[p * ld + p];
      if (!(d > 0.0 && d <= 1.7976931348623157e308)) return 2;
      const double sq = sqrt(d);
      if (lane > p && lane < k) M[lane * ld + p] = M[lane * ld + p] / sq;
      if (lane == p) M[p * ld + p] = sq;
      lds_wave_fence();
      if (lane > p && lane < k) {
        const double lip = M[lane * ld + p];
        for (int c = p + 1; c <= lane; c++) M[lane * ld + c] = fma(-lip, M[c * ld + p], M[lane * ld + c]);
      }
      lds_wave_fence();
    }
  }
  const bool need_yhat = q.fill_all || a.mask;  // (complete data, fill "missing": every entry is the datapoint's own)
  const uint8_t *mrow = a.mask ? a.mask + n * D : nullptr;
  u64 left = m;
  while (left) {
    const int b = __ffsll((long long)left) - 1;
    left &= left - 1ull;
    const i64 t = 64 * (i64)pass + b, r = n * q.T + t;
    if (SSSC && k > 0) {
      if (lane < k) vv[lane] = psamp_normal(x0, PSAMP_PURPOSE + 1, 32ull * (u64)t + (u64)lane);
      lds_wave_fence();
      if (lane < k) {
        double zi = kap[lane];
        for (int j = 0; j <= lane; j++) zi = fma(M[lane * ld + j], vv[j], zi);
        M[lane * ld + 2 * k] = zi;
      }
      lds_wave_fence();
    }
    if (SSSC && q.z) {
      int base = 0;
      for (int w = 0; w < HW; w++) {
        const u64 bits = psamp_word(a, n, sl, w);
        const bool on = (bits >> (63 - lane)) & 1ull;
        int rank = base + (lane ? __popcll(bits >> (64 - lane)) : 0);
        if (rank >= k) rank = 0;  // (only where !on)
        const int h = 64 * w + lane;
        if (h < H) q.z[r * H + h] = on ? M[rank * ld + 2 * k] : 0.0;
        base += __popcll(bits);
      }
    }
    if (q.y) {
      double acc[R];
#pragma unroll
      for (int rr = 0; rr < R; rr++) acc[rr] = 0.0;
      if (need_yhat) {
        for (int i = 0; i < k; i++) {
          const double zi = SSSC ? M[i * ld + 2 * k] : 1.0;
          const double *wr = a.Wt + (i64)idx[i] * D;
#pragma unroll
          for (int rr = 0; rr < R; rr++) {
            const int d = lane + 64 * rr;
            if (d < D) acc[rr] = fma(zi, wr[d], acc[rr]);
          }
        }
      }
#pragma unroll
      for (int rr = 0; rr < R; rr++) {
        const int d = lane + 64 * rr;
        if (d < D) {
          double v;
          if (!q.fill_all && (!mrow || mrow[d])) {
            v = q.Y[n * q.ldY + d];
          } else {
            v = acc[rr];
            if (q.add_noise) v += q.sigma * psamp_normal(x0, PSAMP_PURPOSE + 2, (u64)D * (u64)t + (u64)d);
          }
          q.y[r * D + d] = v;
        }
      }
    }
    if (SSSC) lds_wave_fence();  // the next draw overwrites eps and the z column
  }
  return 0;
}

template <int R, bool SSSC>
__global__ __launch_bounds__(64 * PRED_WAVES) void posterior_sample_kernel(PsampArgs q) {
  extern __shared__ double psamp_lds[];
  const PredArgs &a = q.p;
  const int lane = lane_id(), wave = wave_id_uniform();
  const i64 n = (i64)blockIdx.x * PRED_WAVES + wave;
  if (n >= a.N) return;  // whole waves leave; nothing below synchronises across waves
  const int D = a.D, H = a.H, HW = a.HW, L = a.L, kcap = a.kcap;
  const i64 T = q.T;
  double *slice = psamp_lds + (size_t)wave * pred_lds_doubles(kcap, SSSC);
  double *M = slice, *vv = slice + (SSSC ? kcap * (2 * kcap + 1) : 0), *kap = vv + (SSSC ? kcap : 0);
  int *idx = (int *)(kap + (SSSC ? kcap : 0));  // PRED_MAX_K ints
  const u64 x0 = mix64(q.seed + 0x9e3779b97f4a7c15ull * (q.first_index + (u64)n + 1));
  const double *lrow = a.lpj + n * L;

  int bad = PRED_OK;
  if (a.row_any && !a.row_any[n]) bad = PRED_SKIPPED;
  // ---- a state with more than PRED_MAX_K active latents anywhere in K^n (lane l counts the states l, l + 64, ...)
  for (int s0 = 0; s0 < a.S && bad == PRED_OK; s0 += 64) {
    int k = 0;
    if (s0 + lane < a.S)
      for (int w = 0; w < HW; w++) k += __popcll(psamp_word(a, n, a.S_perm + s0 + lane, w));
    const int first = pred_first_lane(k > PRED_MAX_K);
    if (first < 64) bad = PRED_OVER_K | (__shfl(k, first, 64) << 8);
  }
  // ---- the weights: maximum, poison, total
  double mx = -INFINITY, C = 0.0;
  int last_pos = -1;
  {
    bool poison = false;
    for (int s = lane; s < L; s += 64) {
      const double v = lrow[s];
      mx = fmax(mx, v);
      poison = poison || v != v || v == INFINITY;
    }
    mx = wave_max(mx);
    if (bad == PRED_OK && __ballot(poison)) bad = PSAMP_BAD_WEIGHTS;
  }
  if (bad == PRED_OK) {
    for (int j = 0; j < L; j++) {
      const double e = codes_exp(lrow[j] - mx);
      C = C + e;
      if (e > 0.0) last_pos = j;
    }
    if (!(C > 0.0)) bad = PSAMP_BAD_WEIGHTS;
  }

  int flags = 0;
  const int n_pass = (int)((T + 63) / 64);
  for (int pass = 0; pass < n_pass && bad == PRED_OK; pass++) {
    const i64 t = 64 * (i64)pass + lane;
    bool pending = t < T;
    const double target = pending ? gen_u01(x0, PSAMP_PURPOSE, (u64)t) * C : 0.0;
    double c = 0.0;
    for (int j = 0; j <= L; j++) {  // j == L: the top end, for the lanes no slot has served
      bool hit = pending;
      int sl = last_pos;
      if (j < L) {
        c = c + codes_exp(lrow[j] - mx);
        hit = pending && c > target;
        sl = j;
      }
      const u64 m = __ballot(hit);
      if (!m) continue;
      pending = pending && !hit;
      flags |= psamp_state<R, SSSC>(q, n, sl, m, pass, x0, M, vv, kap, idx, lane);
      if (!__ballot(pending)) break;
    }
  }
  if (flags & 1)
    bad = PRED_SINGULAR;
  else if (flags & 2)
    bad = PSAMP_NOT_PD;

  if (bad != PRED_OK) {  // no draws: every row of the datapoint, whatever the passes have written
    __threadfence();     // (their stores have completed before the same addresses are written again)
    const double nan = __builtin_nan("");
    if (q.slot)
      for (i64 i = lane; i < T; i += 64) q.slot[n * T + i] = -1;
    if (q.s)
      for (i64 i = lane; i < T * HW; i += 64) q.s[n * T * HW + i] = 0ull;
    if (q.z)
      for (i64 i = lane; i < T * H; i += 64) q.z[n * T * H + i] = nan;
    if (q.y)
      for (i64 i = lane; i < T * D; i += 64) q.y[n * T * D + i] = nan;
  }
  if (lane == 0) a.status[n] = bad;
}
