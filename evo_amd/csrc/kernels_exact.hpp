// Exact log-likelihood over all states of Hv <= 32 varying latents (evoamd_loglik_exact): the states are produced on the
// device chunk by chunk, each chunk's N x C lpj block is folded into a running log-sum-exp per datapoint, and no
// N x 2^Hv array exists anywhere.
//
// Index -> state.  State index g (0 <= g < 2^Hv) has latent h on iff bit h of g is set (h < Hv).  With the permanent
// background unit (background = 1, H = Hv + 1) latent H - 1 is on in every state.  Packed, latent h is bit 63 - (h & 63)
// of word h >> 6 (pack_states_kernel's layout): all of a state's latents sit in word 0, which is the bit reversal of g.
// Without background, index 0 is the all-zero state: its term is allzero_lpj_kernel's and seeds the running values, so
// slot 0 of the first chunk holds a stand-in (the state of index 1) that the fold skips.
// evo_amd/models/exact.py: enumerate_chunk / fold_exact are the NumPy mirrors.
#pragma once
#include "common.hpp"

#define EXACT_MAX_HV 32
#define EXACT_LANE_BITS 6   // the lowest six bits of the index are the lane's
#define EXACT_MAX_ACC 10    // log2(65536) - 6: index bits a lane sees change while it strides over a chunk's row

// Packed states of the indices [g0, g0 + cnt) into out (cnt x HW words).  One thread per state.
__global__ __launch_bounds__(256) void exact_enumerate_kernel(u64 *__restrict__ out, u64 g0, int cnt, int Hv, int HW,
                                                              int background) {
  const int j = (int)(blockIdx.x * 256 + threadIdx.x);
  if (j >= cnt) return;
  u64 g = g0 + (u64)j;
  if (!background && g == 0) g = 1;  // the stand-in for the all-zero state (skipped by the fold)
  if (background) g |= 1ull << Hv;   // latent H - 1 = Hv
  u64 *o = out + (size_t)j * HW;
  o[0] = __brevll(g);
  for (int w = 1; w < HW; w++) o[w] = 0;
}

// Running values before the first chunk: (m, z) = (lpj of the all-zero state, 1) without background -- m arrives from
// allzero_lpj_kernel --, (-inf, 0) with it; a = 0.
__global__ __launch_bounds__(256) void exact_seed_kernel(double *__restrict__ run_m, double *__restrict__ run_z,
                                                         double *__restrict__ run_a, i64 N, int Hv, int background) {
  const i64 n = (i64)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  if (background) run_m[n] = -INFINITY;
  run_z[n] = background ? 0.0 : 1.0;
  if (run_a)
    for (int h = 0; h < Hv; h++) run_a[n * Hv + h] = 0.0;
}

// Folds one chunk (indices [g0, g0 + cnt), lpj rows of leading dimension ld) into the running values.  One wavefront
// per datapoint, lanes striding over the row: lane l reads the indices g0 + l + 64 i.  C = the chunk size the caller
// steps by, a power of two >= 64, and g0 a multiple of it, so of a state's index
//   bits 0..5              are the lane's           -> sum_h = wave sum of the lane totals under a lane mask,
//   bits 6..log2(C) - 1    are those of i           -> one accumulator per bit in registers (at most EXACT_MAX_ACC),
//   bits log2(C) and above are those of g0          -> all of the chunk's sum or none of it.
// m' = max(m, chunk max); z and a_h are rescaled by exp(m - m') and the chunk's terms exp(lpj - m') are added: per lane
// in the order of i, across lanes in wave_sum's fixed tree, so the result does not change from call to call.
// skip0: index 0 is not part of the sum (the all-zero state's stand-in).
template <bool MARG>
__global__ __launch_bounds__(256) void exact_fold_kernel(const double *__restrict__ lpj, int ld, i64 N, u64 g0, int cnt,
                                                         int logC, int Hv, int skip0, double *__restrict__ run_m,
                                                         double *__restrict__ run_z, double *__restrict__ run_a) {
  const int lane = lane_id(), wave = wave_id_uniform();
  const i64 n = (i64)blockIdx.x * 4 + wave;
  if (n >= N) return;  // wave-uniform
  const double *row = lpj + n * (i64)ld;
  const bool drop0 = skip0 && g0 == 0;
  double cm = -INFINITY;
  for (int s = lane; s < cnt; s += 64) {
    const double v = row[s];
    if (!(drop0 && s == 0)) cm = fmax(cm, v);
  }
  cm = wave_max(cm);
  const double m_old = run_m[n];
  const double m_new = fmax(m_old, cm);
  if (m_new == -INFINITY) return;  // nothing finite yet (wave-uniform): the running values stand
  const double scale = (m_old == -INFINITY) ? 0.0 : exp(m_old - m_new);
  double t = 0.0;
  double acc[EXACT_MAX_ACC];
#pragma unroll
  for (int b = 0; b < EXACT_MAX_ACC; b++) acc[b] = 0.0;
  for (int s = lane, i = 0; s < cnt; s += 64, i++) {
    double e = exp(row[s] - m_new);
    if (drop0 && s == 0) e = 0.0;
    t += e;
    if (MARG) {
#pragma unroll
      for (int b = 0; b < EXACT_MAX_ACC; b++) acc[b] += ((i >> b) & 1) ? e : 0.0;
    }
  }
  const double zc = wave_sum(t);
  if (lane == 0) {
    run_m[n] = m_new;
    run_z[n] = run_z[n] * scale + zc;
  }
  if (MARG) {
    double mine = 0.0;  // lane h: the chunk's sum over the states with latent h on
    const int nlane = Hv < EXACT_LANE_BITS ? Hv : EXACT_LANE_BITS;
    for (int h = 0; h < nlane; h++) {
      const double s = wave_sum(((lane >> h) & 1) ? t : 0.0);
      if (lane == h) mine = s;
    }
#pragma unroll
    for (int b = 0; b < EXACT_MAX_ACC; b++) {
      const int h = EXACT_LANE_BITS + b;
      if (h < logC && h < Hv) {  // wave-uniform
        const double s = wave_sum(acc[b]);
        if (lane == h) mine = s;
      }
    }
    if (lane >= logC && lane < Hv) mine = ((g0 >> lane) & 1ull) ? zc : 0.0;
    if (lane < Hv) {
      double *a = run_a + n * Hv + lane;
      *a = *a * scale + mine;
    }
  }
}

// ll_n = log z_n + m_n (row_lse_kernel's f_n), marg_nh = a_nh / z_n (the background unit's column: exactly 1), and the
// per-block partial sums of ll_n for reduce_partials_kernel.  One wavefront per datapoint, as row_lse_kernel.
__global__ __launch_bounds__(256) void exact_finish_kernel(const double *__restrict__ run_m,
                                                           const double *__restrict__ run_z,
                                                           const double *__restrict__ run_a, i64 N, int Hv, int H,
                                                           double *__restrict__ ll, double *__restrict__ marg,
                                                           double *__restrict__ partial) {
  __shared__ double wsum[4];
  const int lane = lane_id(), wave = wave_id_uniform();
  const i64 n = (i64)blockIdx.x * 4 + wave;
  double f = 0.0;
  if (n < N) {
    const double z = run_z[n];
    f = log(z) + run_m[n];
    if (lane == 0) ll[n] = f;
    if (marg) {
      if (lane < Hv) marg[n * H + lane] = run_a[n * Hv + lane] / z;
      if (lane >= Hv && lane < H) marg[n * H + lane] = 1.0;
    }
  }
  if (lane == 0) wsum[wave] = f;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}
