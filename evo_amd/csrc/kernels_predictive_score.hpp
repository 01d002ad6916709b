// Log predictive density and PIT of single entries: for every datapoint n and every SCORED entry d (query[n, d] set and
// y = y_true[n, d] finite), under the mixture over the states s of K^n (and the permanent all-zero state) that
// predictive_kernel (kernels_predictive.hpp) collapses to two moments,
//
//   logp[n, d] = log sum_s q_ns N(y; m_ns,d, tau_ns,d)        pit[n, d] = sum_s q_ns Phi((y - m_ns,d) / sqrt(tau_ns,d))
//
// The law (evo_amd.models.predictive_log_score_host is written from it):
//   Weights and slots.  e_s = exp(lpj_s - max lpj) in slot order, the permanent all-zero state first, exactly as in
//     predictive_kernel; a state of weight exactly 0 is skipped after its decode; Wsum = sum_s e_s in slot order.
//   Per state.  m_sd and v_sd as in predictive_kernel: the same pred_solve, the same fma order, v clamped at 0.
//   Per state s and scored entry d.  tau = v_sd + (add_noise ? sigma2 : 0), u = y - m_sd,
//     ld = -1/2 (log(2 pi tau) + u^2 / tau),  Phi = 1/2 erfc(-u / sqrt(2 tau));
//     tau = 0 is a point mass (ES3C without noise, the all-zero state for instance): ld = -inf, Phi = [u >= 0].
//   Folding over states, in the log domain and in slot order: the term a_s = (lpj_s - max lpj) + ld_s goes into a running
//     (M, Z), Z = sum exp(a - M), rescaled when M grows (a term of -inf changes nothing), as exact_fold_kernel and
//     lle_fold_kernel keep theirs; PhiSum += e_s Phi_s (one fma).
//   Per entry.  logp = M + log Z - log Wsum (-inf when no state has a density), pit = PhiSum / Wsum.
//   Special cases.  A queried entry whose y is not finite: NaN in logp and pit, left out of sum and count, counted in
//     nbad[n].  A datapoint without a scored entry is not visited: no decode, no solve, status PRED_NOT_QUERIED (tested
//     first), logp_n = 0, count = 0, NaN at every entry.  A datapoint without a reliable entry is PRED_SKIPPED, one with a singular system
//     PRED_SINGULAR, one with a state of k > PRED_MAX_K active latents PRED_OVER_K | k << 8, all as in predictive_kernel:
//     NaN at every entry, logp_n = 0, count = 0.  Entries outside the query are NaN; y_true is never read there.
//   Sums.  logp_n[n] = wave_sum of the lane partials (each lane adds its entries in ascending d), count[n] likewise; the
//     call's total: pred_score_partials_kernel adds the datapoints PRED_WAVES b .. PRED_WAVES b + PRED_WAVES - 1 in that
//     order into partial[b] (sum) and partial[nb + b] (count, a double: exact below 2^53), then reduce_partials_kernel
//     over each half.  (The partials are a kernel of their own: a workgroup barrier behind the datapoint's code made the
//     compiler reserve 36 to 68 bytes of scratch per lane that no instruction touched.)  Every order is fixed, no atomics,
//     every store is a plain vector store: two calls give the same bits.
//   Which wavefront scores which datapoint is no part of the law: nothing is shared between datapoints.
//
// Mapping: predictive_kernel's -- one wavefront per datapoint, PRED_WAVES per workgroup, lane l owns d = l, l + 64, ...,
// the same LDS slice (pred_lds_doubles) and the same PredArgs.  Per owned entry a lane keeps y, M, Z and PhiSum in
// registers and the query flag in one bit of a mask: 4 R doubles + 1 word (R = 8: 64 VGPRs + 1).  An entry outside the
// query runs neither the m / v loops nor the transcendental functions.  Three launches: pred_score_visit_kernel reads
// the query bytes (and y_true where they are set), counts the bad values and settles the datapoints without a scored
// entry; pred_score_compact_kernel (one workgroup, a scan) lists the others in ascending n; predictive_score_kernel takes
// its datapoints from that list, so its workgroups are full however few datapoints are visited -- a workgroup holds its
// 69 KB of LDS until its longest wave is done, and with the visited datapoints left in place a call that visits one
// datapoint in ten cost 36 % of a full one (1 - 0.9^4 of the workgroups hold one), not 10 %.
#pragma once
#include "kernels_predictive.hpp"

enum { PRED_NOT_QUERIED = 4 };  // status[n] beside PRED_OK .. PRED_OVER_K

struct PredScoreArgs {
  PredArgs p;             // (mean and var are not used)
  const double *y_true;   // (N, D), read at the queried entries only
  const uint8_t *query;   // (N, D)
  double *logp, *pit;     // (N, D) each, or both NULL
  double *logp_n;         // (N)
  int *count, *nbad;      // (N) each
  i64 *list;              // (N + 1): the visited datapoints in ascending order, then their number
};

// nbad[n] and status[n] = PRED_OK (to be visited) or PRED_NOT_QUERIED; the outputs of the datapoints that are not visited.
__global__ __launch_bounds__(64 * PRED_WAVES) void pred_score_visit_kernel(PredScoreArgs q) {
  const int lane = lane_id(), wave = wave_id_uniform(), D = q.p.D;
  const i64 n = (i64)blockIdx.x * PRED_WAVES + wave;
  if (n >= q.p.N) return;  // whole waves leave
  bool any = false;
  int nbad = 0;
  for (int d = lane; d < D; d += 64)
    if (q.query[n * D + d]) {
      if (fabs(q.y_true[n * D + d]) <= 1.7976931348623157e308)
        any = true;
      else
        nbad++;
    }
  nbad = wave_sum_i(nbad);
  const bool visited = __ballot(any) != 0;
  if (lane == 0) {
    q.nbad[n] = nbad;
    q.p.status[n] = visited ? PRED_OK : PRED_NOT_QUERIED;
    if (!visited) q.logp_n[n] = 0.0, q.count[n] = 0;
  }
  if (!visited && q.logp) {
    const double nan = __builtin_nan("");
    for (int d = lane; d < D; d += 64) q.logp[n * D + d] = nan, q.pit[n * D + d] = nan;
  }
}

// list[0 .. V) = the datapoints whose status is not PRED_NOT_QUERIED, ascending; list[N] = V.  One workgroup: thread t
// counts a contiguous chunk, the counts are scanned in LDS, the chunk is written behind the chunks before it.
#define PRED_COMPACT_THREADS 1024
__global__ __launch_bounds__(PRED_COMPACT_THREADS) void pred_score_compact_kernel(const int *__restrict__ status, i64 N,
                                                                                i64 *__restrict__ list) {
  __shared__ i64 tot[PRED_COMPACT_THREADS];
  const int t = threadIdx.x;
  const i64 per = (N + PRED_COMPACT_THREADS - 1) / PRED_COMPACT_THREADS;
  const i64 lo = t * per < N ? t * per : N, hi = lo + per < N ? lo + per : N;
  i64 c = 0;
  for (i64 i = lo; i < hi; i++) c += status[i] != PRED_NOT_QUERIED;
  tot[t] = c;
  __syncthreads();
  for (int o = 1; o < PRED_COMPACT_THREADS; o <<= 1) {  // inclusive scan
    const i64 v = t >= o ? tot[t - o] : 0;
    __syncthreads();
    tot[t] += v;
    __syncthreads();
  }
  i64 pos = tot[t] - c;
  for (i64 i = lo; i < hi; i++)
    if (status[i] != PRED_NOT_QUERIED) list[pos++] = i;
  if (t == PRED_COMPACT_THREADS - 1) list[N] = tot[t];
}

template <int R, bool SSSC>
__global__ __launch_bounds__(64 * PRED_WAVES) void predictive_score_kernel(PredScoreArgs q) {
  extern __shared__ double pred_lds[];
  const PredArgs &a = q.p;
  const int lane = lane_id(), wave = wave_id_uniform();
  const i64 at = (i64)blockIdx.x * PRED_WAVES + wave;
  if (at >= q.list[a.N]) return;  // whole waves leave; nothing below synchronises across waves
  const i64 n = q.list[at];
  const int D = a.D, H = a.H, kcap = a.kcap;
  double *slice = pred_lds + (size_t)wave * pred_lds_doubles(kcap, SSSC);
  double *M = slice, *vv = slice + (SSSC ? kcap * (2 * kcap + 1) : 0), *kap = vv + (SSSC ? kcap : 0);
  int *idx = (int *)(kap + (SSSC ? kcap : 0));  // PRED_MAX_K ints
  const double nan = __builtin_nan("");
  const double noise = a.add_noise ? a.sigma2 : 0.0;

  // ---- the lane's entries: y and the mask of the scored ones
  double y[R];
  unsigned scored = 0;
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int d = lane + 64 * r;
    y[r] = 0.0;
    if (d < D && q.query[n * D + d]) {
      y[r] = q.y_true[n * D + d];
      if (fabs(y[r]) <= 1.7976931348623157e308) scored |= 1u << r;  // (the others: pred_score_visit_kernel counted them)
    }
  }

  int bad = PRED_OK;  // (a listed datapoint has a scored entry)
  if (a.row_any && !a.row_any[n]) bad = PRED_SKIPPED;

  double Mx[R], Z[R], Ph[R];
#pragma unroll
  for (int r = 0; r < R; r++) Mx[r] = -INFINITY, Z[r] = 0.0, Ph[r] = 0.0;
  double Wsum = 0.0;

  const double *lrow = a.lpj + n * a.L;
  double mx = -INFINITY;
  if (bad == PRED_OK) {
    for (int s = lane; s < a.L; s += 64) mx = fmax(mx, lrow[s]);
    mx = wave_max(mx);
  }
  const double ltau0 = log(6.283185307179586477 * noise);  // EBSC: tau = noise in every state

  for (int sl = 0; sl < a.L && bad == PRED_OK; sl++) {
    const double la = lrow[sl] - mx;
    const double e = exp(la);
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
#pragma unroll
    for (int r = 0; r < R; r++) {
      if (!((scored >> r) & 1u)) continue;  // (outside the query: nothing to do)
      const int d = lane + 64 * r;
      double m = 0.0, v = 0.0;
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
      const double tau = v + noise, u = y[r] - m;
      double ldens, phi;
      if (tau == 0.0) {  // a point mass
        ldens = -INFINITY;
        phi = u >= 0.0 ? 1.0 : 0.0;
      } else {
        const double ltau = SSSC ? log(6.283185307179586477 * tau) : ltau0;
        ldens = -0.5 * (ltau + u * u / tau);
        phi = 0.5 * erfc(-u / sqrt(2.0 * tau));
      }
      const double t = la + ldens;
      if (t != -INFINITY) {
        if (t > Mx[r]) {
          Z[r] = (Mx[r] == -INFINITY ? 0.0 : Z[r] * exp(Mx[r] - t)) + 1.0;
          Mx[r] = t;
        } else {
          Z[r] += exp(t - Mx[r]);  // (a NaN term arrives here and stays)
        }
      }
      Ph[r] = fma(e, phi, Ph[r]);
    }
    Wsum += e;
    if (SSSC) lds_wave_fence();  // the next state overwrites M / kap / idx
  }

  const double lW = log(Wsum);
  double lsum = 0.0;
  int lcnt = 0;
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int d = lane + 64 * r;
    const bool on = (scored >> r) & 1u;
    double lp = nan, pt = nan;
    if (on && bad == PRED_OK) {
      lp = Mx[r] == -INFINITY ? -INFINITY : Mx[r] + log(Z[r]) - lW;
      pt = Ph[r] / Wsum;
      lsum += lp;
      lcnt++;
    }
    if (d < D && q.logp) {
      q.logp[n * D + d] = lp;
      q.pit[n * D + d] = pt;
    }
  }
  lsum = wave_sum(lsum);
  lcnt = wave_sum_i(lcnt);
  if (lane == 0) {
    q.logp_n[n] = lsum;
    q.count[n] = lcnt;
    a.status[n] = bad;
  }
}

// partial[b] = the sum of logp_n over the datapoints PRED_WAVES b .. PRED_WAVES b + PRED_WAVES - 1 in that order,
// partial[nb + b] = their count.
__global__ __launch_bounds__(256) void pred_score_partials_kernel(const double *__restrict__ logp_n, const int *__restrict__ count,
                                                                  i64 N, i64 nb, double *__restrict__ partial) {
  const i64 b = (i64)blockIdx.x * 256 + threadIdx.x;
  if (b >= nb) return;
  double s = 0.0, c = 0.0;
  for (int w = 0; w < PRED_WAVES; w++) {
    const i64 n = b * PRED_WAVES + w;
    if (n < N) s += logp_n[n], c += (double)count[n];
  }
  partial[b] = s;
  partial[nb + b] = c;
}
