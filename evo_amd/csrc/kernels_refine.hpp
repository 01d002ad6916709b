// Refinement of K^n at fixed Theta (evoamd_refine_states) and the per-datapoint scores of the resident lpj rows
// (evoamd_posterior_scores).  The loop itself is the E-step stages of evo_amd.hip; the device code here is the trace
// kernel, which moves one iteration's scalars out of the scalar block, and one row-reduction kernel.
#pragma once
#include "common.hpp"
#include "kernels_mstep.hpp"

// One workgroup, one thread at work.  REFINE_TRACE_ROW: {Fs, sum of new unique, sum of swapped} as reduce3_partials_kernel
// left them -> row[0..2], then the two counters are zeroed so that the next row holds one iteration's counts, not
// running sums.  REFINE_TRACE_RESTORE: the counts of `row` back into the scalar block (the last iteration's, on exit:
// what one E-step would have left for the statistics tail).  REFINE_TRACE_ZERO: the counters zeroed, nothing read.
enum { REFINE_TRACE_ROW = 0, REFINE_TRACE_RESTORE = 1, REFINE_TRACE_ZERO = 2 };
__global__ __launch_bounds__(64) void refine_trace_kernel(double *__restrict__ dpar, double *__restrict__ row, int mode) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (mode == REFINE_TRACE_RESTORE) {
    dpar[DP_ECNT0] = row[1];
    dpar[DP_ECNT1] = row[2];
    return;
  }
  if (mode == REFINE_TRACE_ROW) {
    row[0] = dpar[DP_FS];
    row[1] = dpar[DP_ECNT0];
    row[2] = dpar[DP_ECNT1];
  }
  dpar[DP_ECNT0] = 0.0;
  dpar[DP_ECNT1] = 0.0;
}

// One wavefront per datapoint, lanes strided over the L = S_perm + S columns of its lpj row (the row is read twice, the
// second time from cache: N L 8 bytes of memory traffic; the counts add the N S HW state words).  With m = max_s lpj_ns,
// d_s = lpj_ns - m, w_s = exp(d_s), z = sum_s w_s:
//   F_n = m + log z,   entropy_n = log z - (sum_s w_s d_s) / z  (a weight that underflowed to 0 contributes 0),
//   best_n = the first column with lpj_ns == m,   k_best_n = active latents of that state,   k_mean_n = (sum_s w_s |s_s|) / z.
// Columns below S_perm are the permanent all-zero state (no words, count 0).  Counts come from the packed words: the
// digests saturate at 255.  Every lane adds its columns in ascending order and wave_sum adds the lanes in a fixed
// tree, so two calls give the same bits.  Null outputs are skipped; without k_best / k_mean no state word is read.
#define SCORE_WAVES 4
__global__ __launch_bounds__(64 * SCORE_WAVES) void posterior_score_kernel(
    const double *__restrict__ lpj, const u64 *__restrict__ states, i64 N, int L, int S, int S_perm, int HW,
    double *__restrict__ F_out, double *__restrict__ ent_out, int *__restrict__ best_out, int *__restrict__ kbest_out,
    double *__restrict__ kmean_out) {
  const int lane = lane_id(), wave = wave_id_uniform();
  const i64 n = (i64)blockIdx.x * SCORE_WAVES + wave;
  if (n >= N) return;  // (uniform per wave: the reductions below see all 64 lanes)
  const double *row = lpj + n * L;
  const u64 *st = states + n * (i64)S * HW;
  double m = -INFINITY;
  for (int s = lane; s < L; s += 64) m = fmax(m, row[s]);
  m = wave_max(m);
  unsigned first = (unsigned)L;
  double z = 0.0, e = 0.0, km = 0.0;
  const bool counts = kmean_out != nullptr;
  for (int s = lane; s < L; s += 64) {
    const double v = row[s];
    if (v == m && (unsigned)s < first) first = (unsigned)s;
    const double d = v - m;
    const double w = exp(d);
    z += w;
    if (w > 0.0) {
      e += w * d;
      if (counts && s >= S_perm) {
        const u64 *sp = st + (i64)(s - S_perm) * HW;
        int k = 0;
        for (int j = 0; j < HW; j++) k += __popcll(sp[j]);
        km += w * (double)k;
      }
    }
  }
  z = wave_sum(z);
  e = wave_sum(e);
  if (counts) km = wave_sum(km);
  first = wave_min_u32(first);
  if (first >= (unsigned)L) first = 0;  // a row of NaN has no maximum: column 0
  if (lane == 0) {
    const double lz = log(z);
    if (F_out) F_out[n] = m + lz;
    if (ent_out) ent_out[n] = lz - e / z;
    if (best_out) best_out[n] = (int)first;
    if (kmean_out) kmean_out[n] = km / z;
    if (kbest_out) {
      int k = 0;
      if ((int)first >= S_perm) {
        const u64 *sp = st + (i64)((int)first - S_perm) * HW;
        for (int j = 0; j < HW; j++) k += __popcll(sp[j]);
      }
      kbest_out[n] = k;
    }
  }
}
