// The dictionary resized on the device (evoamd_remap_latents): the bits of K^n moved to a new latent numbering, and the
// per-latent count of MAP states (evoamd_latent_map_counts) that says which latents to drop.
//
// THE LAW (evo_amd/variational/utils.py: remap_states_host is its NumPy mirror, bit for bit -- keep the two and the
// tests in step).  Input: index, int32 of length H'.  An entry >= 0 names a source latent in [0, H), each at most once;
// -1 marks a NEW latent, off in every state.  Hv' = H' - 1 with the background unit (the last entry is then H - 1: the
// unit stays last and on), else H'.  H' <= DIG_MAX_H.  Per datapoint n, independently:
//   gather  t_j[h'] = s_j[index[h']] where index[h'] >= 0, else 0, for the slots j = 0 .. S - 1 of K^n (the permanent
//           all-zero column of S_perm = 1 is not a slot);
//   keep    slot j is kept iff t_j differs from every t_i with i < j and, where S_perm = 1, is not the all-zero state
//           (equality is on the full words; the digest decides alone up to DIG_SLOTS active latents, above it only
//           pre-filters);
//   fill    the other slots, in ascending order, each take the next state of the fixed enumeration that equals no kept
//           state of this datapoint, in any slot, earlier or later: the singletons {0}, {1}, .. {Hv' - 1}, then the pairs
//           {0,1}, {0,2}, .. {0,Hv'-1}, {1,2}, .., each ORed with the background bit where there is one; the enumeration is
//           consumed once per datapoint, so fills are distinct among themselves;
//   bound   Hv' (Hv' + 1) / 2 >= S (checked on the host before the launch) guarantees that the enumeration cannot run
//           out: total >= S  =>  total - kept >= S - kept;
//   out     the new packed states (N, S, ceil(H'/64)), MSB-first as everywhere, their digests, n_replaced (N) and its sum.
//
// Mapping: one wavefront per datapoint, up to REMAP_WAVES per workgroup.  `index` sits in LDS once per workgroup, padded
// with -1 to whole destination words.  The S x HW source words of the datapoint go to the wave's LDS slice with
// coalesced loads.  Destination word k of state j is ONE ballot: lane l reads the source bit index[64 k + l] of the state
// (its source word and shift are the same for every state: fetched once per k), __brevll turns the ballot into the
// MSB-first word; lane j % 64 keeps it and 64 states' words are written together.  Digests: make_digest on the new words,
// one lane per slot, with a 64-bit hash of the words beside it.  Keep: lane i compares its hash with those of the slots
// j < i (wave-uniform LDS reads) and settles a match on the digest, or on the full words where the digest holds more than
// DIG_SLOTS latents; the ballot of the duplicates is the slot mask.  The LDS reads of
// these loops are issued eight at a time: with one wave per SIMD (the slice of S = 200, H = 512 -> 384 is 24 KB) nothing
// else hides their latency.  Fill (only where a datapoint has duplicates): 64 enumeration candidates at a time, one lane
// each -- a singleton or a pair (plus the background bit) has at most three latents, so its digest IS the state -- tested
// against the kept digests; the ballot of the free lanes and a prefix popcount hand them to the duplicate slots in
// ascending order.  No random number, no floating point, no order left to the scheduler: two calls give the same bits.
// (A run of 64 consecutive indices could take a shifted-word path; pruning breaks the runs at every dropped latent, so it
// is not built.)
// LDS: 4 * 64 * HW' bytes of index + per wave 8 S (HW + HW' + 1) bytes; the host picks the waves per workgroup that fit
// REMAP_LDS_BYTES and refuses an S whose slice does not fit with one wave.
// Traffic: N S (HW + HW') 8 bytes of words + N S 8 of digests.
#pragma once
#include "common.hpp"
#include "kernels_init.hpp"  // init_wave_sync, init_uniform

#define REMAP_WAVES 4
#define REMAP_MAX_Q 16  // S <= 1024: slot masks of 64
#define REMAP_LDS_BYTES (150 * 1024)

struct RemapArgs {
  const u64 *src;    // (N, S, HW) the resident K^n
  const int *index;  // (H2)
  u64 *dst;          // (N, S, HW2)
  u64 *dig;          // (N, S)
  int *n_replaced;   // (N)
  unsigned long long *sum;  // sum of n_replaced (zeroed by the caller)
  i64 N;
  int S, S_perm, H, HW, H2, HW2, Hv2, bg;
};

// words of dynamic LDS for W waves per workgroup
static inline size_t remap_lds_words(int W, int S, int HW, int HW2) {
  return (size_t)32 * HW2 + (size_t)W * S * (HW + HW2 + 1);
}

// candidate c of the enumeration: singleton {c} below Hv, else pair number p = c - Hv in the order {0,1}, {0,2}, ..
__device__ __forceinline__ void remap_candidate(i64 c, int Hv, int &la, int &lb) {
  if (c < Hv) {
    la = (int)c;
    lb = -1;
    return;
  }
  const i64 p = c - Hv;
  const double t = 2.0 * Hv - 1.0;
  i64 a = (i64)((t - sqrt(t * t - 8.0 * (double)p)) * 0.5);
  if (a < 0) a = 0;
  if (a > Hv - 2) a = Hv - 2;
  // pairs that begin below a: a (2 Hv - a - 1) / 2 -- the root may be one off either way
  while (a > 0 && a * (2 * (i64)Hv - a - 1) / 2 > p) a--;
  while (a < Hv - 2 && (a + 1) * (2 * (i64)Hv - a - 2) / 2 <= p) a++;
  la = (int)a;
  i64 b = a + 1 + (p - a * (2 * (i64)Hv - a - 1) / 2);
  if (b <= a || b >= Hv) b = Hv - 1;  // (cannot happen for p below Hv (Hv - 1) / 2; the value becomes an LDS address)
  lb = (int)b;
}

__global__ __launch_bounds__(64 * REMAP_WAVES) void remap_latents_kernel(RemapArgs a) {
  extern __shared__ u64 remap_lds[];
  __shared__ u64 dupm_sh[REMAP_WAVES][REMAP_MAX_Q];
  const int lane = lane_id(), wave = wave_id_uniform();
  const int W = (int)(blockDim.x >> 6);
  const int S = a.S, HW = a.HW, HW2 = a.HW2;
  int *idx_sh = (int *)remap_lds;
  for (int i = (int)threadIdx.x; i < 64 * HW2; i += (int)blockDim.x) {
    const int v = i < a.H2 ? a.index[i] : -1;
    idx_sh[i] = (v >= 0 && v < a.H) ? v : -1;  // (validated on the host; a value that becomes an address is checked here too)
  }
  __syncthreads();
  u64 *srcw = remap_lds + (size_t)32 * HW2 + (size_t)wave * S * (HW + HW2 + 1);
  u64 *neww = srcw + (size_t)S * HW;
  u64 *dg = neww + (size_t)S * HW2;
  u64 *dupm = dupm_sh[wave];
  const int Q = (S + 63) >> 6;
  const u64 below = (1ull << lane) - 1ull;  // the lanes before this one
  const i64 total = (i64)a.Hv2 + (i64)a.Hv2 * (a.Hv2 - 1) / 2;
  for (i64 n = (i64)blockIdx.x * W + wave; n < a.N; n += (i64)gridDim.x * W) {
    // ---- gather
    const u64 *sg = a.src + (size_t)n * S * HW;
    for (int i0 = 0; i0 < S * HW; i0 += 512) {  // eight loads in flight
      u64 v[8];
#pragma unroll
      for (int u = 0; u < 8; u++) v[u] = i0 + 64 * u + lane < S * HW ? sg[i0 + 64 * u + lane] : 0ull;
#pragma unroll
      for (int u = 0; u < 8; u++)
        if (i0 + 64 * u + lane < S * HW) srcw[i0 + 64 * u + lane] = v[u];
    }
    init_wave_sync();
    for (int k = 0; k < HW2; k++) {
      const int ix = idx_sh[64 * k + lane];
      const bool live = ix >= 0;
      const int sw = live ? ix >> 6 : 0;
      const u64 mk = live ? 0x8000000000000000ull >> (ix & 63) : 0ull;  // the source bit in its word
      for (int j0 = 0; j0 < S; j0 += 64) {
        const int jn = S - j0 < 64 ? S - j0 : 64;
        u64 mine = 0;
        for (int t0 = 0; t0 < jn; t0 += 8) {  // eight LDS reads in flight (states past the end read the last one: not stored)
          u64 wv[8];
#pragma unroll
          for (int u = 0; u < 8; u++) {
            const int j = j0 + t0 + u;
            wv[u] = srcw[(size_t)(j < S ? j : S - 1) * HW + sw];
          }
#pragma unroll
          for (int u = 0; u < 8; u++) {
            const bool bit = (wv[u] & mk) != 0ull;
            const u64 word = __brevll(__ballot(bit));  // ballot bit l = latent 64 k + l = bit 63 - l of the MSB-first word
            if (lane == t0 + u) mine = word;
          }
        }
        if (lane < jn) neww[(size_t)(j0 + lane) * HW2 + k] = mine;
      }
    }
    init_wave_sync();
    // ---- digests of the gathered states, and a 64-bit hash of their words where the source words were (done with): the
    // pre-filter of the equality tests -- a digest above DIG_SLOTS latents is shared by many states of a dense K^n
    u64 *hsh = srcw;
    for (int j = lane; j < S; j += 64) {
      const u64 *sp = neww + (size_t)j * HW2;
      dg[j] = make_digest(sp, HW2);
      u64 hs = 0;
      for (int w = 0; w < HW2; w++) hs = mix64(hs + sp[w] + 1);
      hsh[j] = hs;
    }
    init_wave_sync();
    // ---- keep: first occurrences that are not the permanent state
    int n_rep = 0;
    for (int q = 0; q < Q; q++) {
      const int i = 64 * q + lane;
      const int ii = i < S ? i : S - 1;
      const u64 di = dg[ii], hi = hsh[ii];
      bool dup = a.S_perm && dig_k(di) == 0;
      const int jend = 64 * q + 63 < S ? 64 * q + 63 : S;  // j < i <= 64 q + 63
      const bool wide = dig_k(di) > DIG_SLOTS;  // the digest does not hold every latent: the words decide
      for (int j0 = 0; j0 < jend; j0 += 8) {
        u64 hv[8];
#pragma unroll
        for (int u = 0; u < 8; u++) hv[u] = hsh[j0 + u < S ? j0 + u : S - 1];
#pragma unroll
        for (int u = 0; u < 8; u++) {
          const int j = j0 + u;
          bool eq = j < i && j < jend && hv[u] == hi;
          if (eq) {  // (true duplicates, and one pair in 2^64 otherwise)
            if (wide)
              for (int w = 0; w < HW2; w++) eq = eq && neww[(size_t)j * HW2 + w] == neww[(size_t)ii * HW2 + w];
            else
              eq = dg[j] == di;
          }
          dup = dup || eq;
        }
      }
      const u64 m = __ballot(dup && i < S);
      if (lane == 0) dupm[q] = m;
      n_rep += __popcll(m);
    }
    n_rep = __builtin_amdgcn_readfirstlane(n_rep);
    init_wave_sync();
    // ---- fill the duplicate slots from the enumeration
    if (n_rep > 0) {
      int *dlist = (int *)srcw;  // the hashes are done with: the duplicate slots in ascending order (S ints fit S HW words)
      int base = 0;
      for (int q = 0; q < Q; q++) {
        const u64 m = init_uniform(dupm[q]);
        if ((m >> lane) & 1ull) dlist[base + __popcll(m & below)] = 64 * q + lane;
        base += __popcll(m);
      }
      init_wave_sync();
      int filled = 0;
      for (i64 cb = 0; filled < n_rep && cb < total; cb += 64) {
        const i64 c = cb + lane;
        bool fr = c < total;
        int la = 0, lb = -1;
        if (fr) remap_candidate(c, a.Hv2, la, lb);
        u64 cd = 0;
        int ck = 0;
        digest_add(cd, ck, la);
        if (lb >= 0) digest_add(cd, ck, lb);
        if (a.bg) digest_add(cd, ck, a.H2 - 1);
        cd = digest_close(cd, ck);
        for (int q = 0; q < Q; q++) {
          const u64 m = init_uniform(dupm[q]);
          const int jn = S - 64 * q < 64 ? S - 64 * q : 64;
          for (int t0 = 0; t0 < jn; t0 += 8) {
            u64 dv[8];
#pragma unroll
            for (int u = 0; u < 8; u++) dv[u] = dg[64 * q + t0 + u < S ? 64 * q + t0 + u : S - 1];
#pragma unroll
            for (int u = 0; u < 8; u++)
              if (t0 + u < jn && !((m >> (t0 + u)) & 1ull) && dv[u] == cd) fr = false;
          }
        }
        const u64 fm = __ballot(fr);
        const int rank = filled + __popcll(fm & below);
        if (fr && rank < n_rep) {
          const int slot = dlist[rank];
          if (slot >= 0 && slot < S) {
            u64 *dw = neww + (size_t)slot * HW2;
            for (int w = 0; w < HW2; w++) dw[w] = 0ull;
            dw[la >> 6] |= 0x8000000000000000ull >> (la & 63);
            if (lb >= 0) dw[lb >> 6] |= 0x8000000000000000ull >> (lb & 63);
            if (a.bg) dw[(a.H2 - 1) >> 6] |= 0x8000000000000000ull >> ((a.H2 - 1) & 63);
            dg[slot] = cd;
          }
        }
        filled += __popcll(fm);
      }
      init_wave_sync();
    }
    // ---- out
    u64 *dgl = a.dst + (size_t)n * S * HW2;
    for (int i0 = 0; i0 < S * HW2; i0 += 512) {
      u64 v[8];
#pragma unroll
      for (int u = 0; u < 8; u++) v[u] = neww[i0 + 64 * u + lane < S * HW2 ? i0 + 64 * u + lane : 0];
#pragma unroll
      for (int u = 0; u < 8; u++)
        if (i0 + 64 * u + lane < S * HW2) dgl[i0 + 64 * u + lane] = v[u];
    }
    for (int j = lane; j < S; j += 64) a.dig[(size_t)n * S + j] = dg[j];
    if (lane == 0) {
      a.n_replaced[n] = n_rep;
      if (n_rep) atomicAdd(a.sum, (unsigned long long)n_rep);
    }
    init_wave_sync();  // the next datapoint overwrites the slice
  }
}

// counts[h] += 1 for every latent h of the MAP state of each datapoint: the first column of maximal lpj (the rule of
// posterior_score_kernel; a row of NaN has no maximum: column 0), columns below S_perm are the all-zero state.  One
// wavefront per datapoint; integer atomics, so the result does not depend on the order.  counts: 64 HW entries, zeroed by
// the caller.
#define MAPCOUNT_WAVES 4
__global__ __launch_bounds__(64 * MAPCOUNT_WAVES) void latent_map_count_kernel(const double *__restrict__ lpj,
                                                                               const u64 *__restrict__ states, i64 N, int L,
                                                                               int S, int S_perm, int HW,
                                                                               unsigned long long *__restrict__ counts) {
  const int lane = lane_id(), wave = wave_id_uniform();
  const i64 n = (i64)blockIdx.x * MAPCOUNT_WAVES + wave;
  if (n >= N) return;  // (uniform per wave: the reductions below see all 64 lanes)
  const double *row = lpj + n * L;
  double m = -INFINITY;
  for (int s = lane; s < L; s += 64) m = fmax(m, row[s]);
  m = wave_max(m);
  unsigned first = (unsigned)L;
  for (int s = lane; s < L; s += 64)
    if (row[s] == m && (unsigned)s < first) first = (unsigned)s;
  first = wave_min_u32(first);
  if (first >= (unsigned)L) first = 0;
  if ((int)first < S_perm) return;
  const u64 *sp = states + (n * (i64)S + ((int)first - S_perm)) * HW;
  for (int w = lane; w < HW; w += 64) {
    u64 bits = sp[w];
    while (bits) atomicAdd(&counts[w * 64 + pop_msb(bits)], 1ull);
  }
}
