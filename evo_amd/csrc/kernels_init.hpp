// K^n(0) on the device: S unique Bernoulli(p0) states per datapoint, one wavefront per datapoint.
//
// Restates init_states (variational/utils.py:100-138) with a counter-based stream.  Per datapoint n:
//   round 0   S candidates with independent bits Bernoulli(p0) over the Hv varying latents (Hv = H - 1 with the permanent
//             background unit, whose bit -- the last latent -- is set in every state and never drawn); candidates equal
//             to the permanent all-zero state (S_perm = 1) are dropped; first occurrences are kept in ascending
//             lexicographic row order = unsigned order of the MSB-first words = np.unique's order on the bool rows;
//   round r   while fewer than S states are held: S more candidates, those that are not permanent, not held and not
//             duplicated within the round are appended in ascending order behind what is held;
//   result    the first S held states, in that order.
// THE STREAM (evo_amd/variational/utils.py: init_states_counter is its NumPy mirror, bit for bit -- keep the two and
// the tests in step):
//   bit(n, r, s, h) = rng_u01(seed, n, INIT_PURPOSE + r, s * Hv + h) < p0        (rng_u01, mix64: kernels_evolve.hpp)
// i.e. x = mix64(mix64(seed + 0x9e3779b97f4a7c15 (n + 1)) ^ ((INIT_PURPOSE + r) 0xd1b54a32d192ed03 + s Hv + h +
// 0x632be59bd9b4e019)), u = ((x >> 11) + 0.5) 2^-53 in IEEE double: integer hashing, one integer -> double conversion
// (exact below 2^53), one addition and one multiplication by a power of two, so NumPy reproduces every bit.  That is why
// the bits are drawn one by one and not by geometric skipping through a log.  INIT_PURPOSE lies far from the purposes of
// the evolve kernels (1, 2 + p, (generation + 1) << 32 + small).
//
// Mapping: a candidate word is ONE ballot -- lane l evaluates latent 64 w + 63 - l, so ballot bit l is bit l of the
// MSB-first word; the first hash is shared by the datapoint.  The round's candidates and the held set live side by side
// in the wave's home, LDS or (where 2 S (HW + 1) words per wave do not fit) a slot of global memory; each set is stored
// word-major ([w][s], lane i reads its own candidate without bank conflicts, candidate j is a broadcast) with one more
// row for a 64-bit hash of the words, the pre-filter of every equality test.  Order and duplicates by counting:
// candidate i is a duplicate if an equal key exists in the permanent set, in the held set or at j < i; the rank of a
// survivor is the number of survivors with a smaller key.  Survivors go to held[m + rank]; once S are held the wave
// writes the states to K^n in that order together with their digests (the digest digest_kernel would compute).
// The loop over rounds is wave-uniform.  A datapoint that is not complete after max_rounds raises INIT_ERR_CAP in the
// context's error word and writes nothing.
#pragma once
#include "common.hpp"
#include "kernels_evolve.hpp"

#define INIT_PURPOSE 0x494E495400000000ull
#define INIT_ERR_WORD 5  // word of the context's error block that belongs to evoamd_init_states
#define INIT_ERR_CAP 1
#define INIT_MAX_Q 16    // S <= 1024: chunks of 64 candidates

struct InitArgs {
  u64 *states;   // (N, S, HW) K^n
  u64 *dig;      // (N, S) or nullptr
  u64 *scratch;  // global home: 2 (HW + 1) S words per wave of the grid; nullptr with the LDS home
  int *err;      // the error word (INIT_ERR_WORD of the block)
  i64 N;
  int S, S_perm, H, Hv, HW, max_rounds;
  u64 seed;
  double p0;
};

// lanes of one wave hand data to each other through the home: make the writes visible, keep the compiler from moving
// accesses across (a wave's own memory operations are issued in order)
__device__ __forceinline__ void init_wave_sync() {
  __threadfence_block();
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ u64 init_uniform(u64 v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
  return ((u64)hi << 32) | lo;
}

template <bool LDS_HOME>
__global__ __launch_bounds__(256) void init_states_kernel(InitArgs a) {
  extern __shared__ u64 init_lds[];
  __shared__ u64 surv_sh[4][INIT_MAX_Q];
  const int lane = lane_id(), wave = wave_id_uniform();
  const int W = (int)(blockDim.x >> 6);
  const int S = a.S, HW = a.HW, Hv = a.Hv;
  const size_t set = (size_t)(HW + 1) * S;  // HW word rows and the hash row
  u64 *cand = LDS_HOME ? init_lds + (size_t)wave * 2 * set : a.scratch + ((size_t)blockIdx.x * W + wave) * 2 * set;
  u64 *held = cand + set;
  u64 *surv = surv_sh[wave];
  const int Q = (S + 63) >> 6;
  const int bg = a.H - 1;  // the background unit's latent when Hv < H
  for (i64 n = (i64)blockIdx.x * W + wave; n < a.N; n += (i64)gridDim.x * W) {
    const u64 x0 = mix64(a.seed + 0x9e3779b97f4a7c15ull * ((u64)n + 1));
    int m = 0;  // states held
    for (int r = 0; r < a.max_rounds && m < S; r++) {
      const u64 salt = (INIT_PURPOSE + (u64)r) * 0xd1b54a32d192ed03ull + 0x632be59bd9b4e019ull;
      // ---- the round's candidates: one ballot per word
      for (int s = 0; s < S; s++) {
        u64 hs = 0;
        for (int w = 0; w < HW; w++) {
          const int h = 64 * w + 63 - lane;
          bool bit = Hv < a.H && h == bg;
          if (h < Hv) {
            const u64 x = mix64(x0 ^ (salt + (u64)s * (u64)Hv + (u64)h));
            bit = ((double)(x >> 11) + 0.5) * (1.0 / 9007199254740992.0) < a.p0;
          }
          const u64 word = __ballot(bit);
          hs = mix64(hs + word + 1);
          if (lane == 0) cand[(size_t)w * S + s] = word;
        }
        if (lane == 0) cand[(size_t)HW * S + s] = hs;
      }
      init_wave_sync();
      // ---- duplicates: of the permanent state, of a held state, of an earlier candidate
      int n_surv = 0;
      for (int q = 0; q < Q; q++) {
        const int i = 64 * q + lane;
        const int ii = i < S ? i : S - 1;  // lanes past the end read the last candidate and count as duplicates
        const u64 hi = cand[(size_t)HW * S + ii];
        bool dup = i >= S;
        if (a.S_perm) {
          bool zero = true;
          for (int w = 0; w < HW; w++) zero = zero && cand[(size_t)w * S + ii] == 0ull;
          dup = dup || zero;
        }
        for (int j = 0; j < m; j++) {
          bool eq = !dup && held[(size_t)HW * S + j] == hi;
          if (__any(eq)) {
            for (int w = 0; w < HW; w++) eq = eq && held[(size_t)w * S + j] == cand[(size_t)w * S + ii];
            dup = dup || eq;
          }
        }
        const int jend = 64 * q + 63 < S ? 64 * q + 63 : S;  // j < i <= 64 q + 63
        for (int j = 0; j < jend; j++) {
          bool eq = !dup && j < i && cand[(size_t)HW * S + j] == hi;
          if (__any(eq)) {
            for (int w = 0; w < HW; w++) eq = eq && cand[(size_t)w * S + j] == cand[(size_t)w * S + ii];
            dup = dup || eq;
          }
        }
        const u64 alive = __ballot(!dup);
        if (lane == 0) surv[q] = alive;
        n_surv += __popcll(alive);
      }
      init_wave_sync();
      // ---- rank of a survivor = survivors with a smaller key; held[m + rank] while there is room
      for (int q = 0; q < Q; q++) {
        const int i = 64 * q + lane;
        const bool mine = (init_uniform(surv[q]) >> lane) & 1ull;
        const int ii = i < S ? i : S - 1;
        int rank = 0;
        for (int jq = 0; jq < Q; jq++) {
          u64 bits = init_uniform(surv[jq]);
          while (bits) {
            const int j = 64 * jq + __ffsll((long long)bits) - 1;
            bits &= bits - 1;
            int order = (mine && j != i) ? 0 : 2;  // 0 undecided, 1 key_j < key_i, 2 not
            for (int w = 0; w < HW; w++) {
              if (!__any(order == 0)) break;
              const u64 kj = cand[(size_t)w * S + j], ki = cand[(size_t)w * S + ii];
              if (order == 0 && kj != ki) order = kj < ki ? 1 : 2;
            }
            rank += order == 1;
          }
        }
        const int dest = m + rank;
        if (mine && dest < S)
          for (int w = 0; w <= HW; w++) held[(size_t)w * S + dest] = cand[(size_t)w * S + ii];
      }
      m = m + n_surv < S ? m + n_surv : S;
      init_wave_sync();
    }
    if (m < S) {  // the round cap: nothing of this datapoint is written
      if (lane == 0) atomicOr(a.err, INIT_ERR_CAP);
      continue;
    }
    // ---- K^n rows and their digests
    u64 *dst = a.states + (size_t)n * S * HW;
    for (int idx = lane; idx < S * HW; idx += 64) {
      const int s = idx / HW, w = idx - s * HW;
      dst[idx] = held[(size_t)w * S + s];
    }
    if (a.dig)
      for (int s = lane; s < S; s += 64) {
        u64 d = 0;
        int k = 0;
        for (int w = 0; w < HW; w++) {
          u64 bits = held[(size_t)w * S + s];
          while (bits) digest_add(d, k, w * 64 + pop_msb(bits));
        }
        a.dig[(size_t)n * S + s] = digest_close(d, k);
      }
    init_wave_sync();  // the next datapoint overwrites the home
  }
}

// Exact E-steps (S == 2^Hv): every datapoint gets the same state table (at most 2048 rows), no random numbers.
__global__ __launch_bounds__(256) void init_states_tile_kernel(const u64 *__restrict__ table, u64 *__restrict__ states,
                                                               u64 *__restrict__ dig, i64 N, int S, int HW) {
  const i64 idx = (i64)blockIdx.x * 256 + threadIdx.x;
  if (idx >= N * S) return;
  const u64 *src = table + (size_t)(idx % S) * HW;
  u64 *dst = states + (size_t)idx * HW;
  for (int w = 0; w < HW; w++) dst[w] = src[w];
  if (dig) dig[idx] = make_digest(src, HW);
}
