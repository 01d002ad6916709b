// K^n resized on the device (evoamd_resize_states): S, the number of states per datapoint, changes; the best states are
// kept, new slots are filled next to the best state.
//
// THE LAW (evo_amd/variational/utils.py: resize_states_host is its NumPy mirror, bit for bit -- keep the two and the tests
// in step).  Per datapoint n, independently.  Input: the S varying slots of the resident K^n (packed words, MSB-first), the
// datapoint's lpj row (S_perm + S doubles; the permanent all-zero column of S_perm = 1 is not a slot and is carried over
// untouched), the new size S'.  Hv = H - background.
//   keys    slot j has key seed_key(lpj[n, S_perm + j]), the order-preserving key of kernels_seed.hpp: NaN and +-inf rank as
//           -inf, -0 equals +0.  Rank order is descending key, then ascending slot.
//   shrink  (S' < S) the kept slots are the first S' in rank order, written in ASCENDING OLD SLOT (a stable compaction, so
//           "the first column of maximal lpj" still names the same state); src_slot[n, j'] is the old slot of new slot j'.
//   grow    (S' > S) slots 0 .. S - 1 are copied in place, src_slot[n, j] = j.  b = the words of the best varying state (rank
//           0: parent 0 of the sweep law).  e_c = candidate c of the enumeration remap_candidate(c, Hv): the singletons {0} ..
//           {Hv - 1}, then the pairs {0,1}, {0,2}, .. {Hv-2, Hv-1}.  The candidate fill is f_c = b XOR e_c: the one-flip
//           neighbours of the best state in ascending latent, then its two-flip neighbours.  f_c is skipped when it has no
//           varying latent on, and when its full words equal a state the datapoint already holds (a hash pre-filters, the
//           decision is made on the words).  Slots S, S + 1, .. take the unskipped f_c in ascending c; src_slot is -1 there.
//           XOR with a fixed b is a bijection: the fills are distinct among themselves without a test.  The background bit
//           of b stays on.
//   bound   Hv (Hv + 1) / 2 - 1 >= S' (checked on the host before the launch): at most one candidate is empty and at most S
//           are held, so the enumeration cannot run out.
//   out     the new packed states (N, S', HW), their digests (make_digest), src_slot int32 (N, S').
// No floating point beyond the key, no random numbers, no atomics: two calls give the same bits.
//
// Mapping: one wavefront per datapoint, up to RESIZE_WAVES per workgroup, grid-stride.  The keys of the row go to the wave's
// LDS share (8 S bytes).  Shrink: the S'-th key by the threshold search of seed_rank_keys (64 rounds of ballots over the
// keys, held in registers up to 256 slots), ties at the threshold to the lowest slots; ballots and prefix popcounts compact
// the members 64 slots at a time into a list of old slots in LDS; the words are then copied with coalesced stores, eight
// loads in flight.  Grow: the S HW words copied coalesced; one lane per held state hashes its words into LDS (where the keys
// were) and forms its digest; 64 enumeration candidates at a time, one lane each, are hashed from b (HW broadcast reads of
// LDS) and tested against the held hashes (wave-uniform reads, eight at a time), a hash match settled on the full words; the
// ballot of the free lanes and a prefix popcount hand them to the new slots in order -- the fill loop of remap_fill with
// full-word equality.  Every slot read back from LDS passes guard_index; a latent of a candidate comes from
// remap_candidate, which clamps it.
// LDS per wave: 8 (S + HW) + 4 S' bytes, rounded up to 8; the host picks the waves per workgroup that fit RESIZE_LDS_BYTES.
// Traffic: N (S + S') HW 8 bytes of words + N S 8 of lpj + N S' 12 of digests and src_slot.
#pragma once
#include "common.hpp"
#include "kernels_evolve.hpp"  // mix64
#include "kernels_init.hpp"    // init_wave_sync
#include "kernels_remap.hpp"   // remap_candidate
#include "kernels_seed.hpp"    // seed_key

#define RESIZE_WAVES 4
#define RESIZE_MAX_S 1024
#define RESIZE_KREG 4  // chunks of 64 keys the threshold search keeps in registers
#define RESIZE_LDS_BYTES (150 * 1024)

struct ResizeArgs {
  const u64 *src;     // (N, S, HW) the resident K^n
  const double *lpj;  // (N, L) its rows
  u64 *dst;           // (N, S2, HW)
  u64 *dig;           // (N, S2)
  int *src_slot;      // (N, S2)
  int *err;
  i64 N;
  int S, S2, S_perm, L, H, HW, Hv, bg;
};

// words of dynamic LDS of one wave: keys / hashes (S), the best state's words (HW), the list of kept slots (S2 ints)
__host__ __device__ static inline size_t resize_lds_words(int S, int S2, int HW) { return (size_t)S + HW + ((size_t)S2 + 1) / 2; }

__device__ __forceinline__ u64 resize_wave_max_u64(u64 v) {
  const unsigned hi = wave_max_u32((unsigned)(v >> 32));
  const unsigned lo = wave_max_u32((unsigned)(v >> 32) == hi ? (unsigned)v : 0u);
  return ((u64)hi << 32) | lo;
}

__global__ __launch_bounds__(64 * RESIZE_WAVES) void resize_states_kernel(ResizeArgs a) {
  extern __shared__ u64 resize_lds[];
  const int lane = lane_id(), wave = wave_id_uniform();
  const int W = (int)(blockDim.x >> 6);
  const int S = a.S, S2 = a.S2, HW = a.HW;
  u64 *keys = resize_lds + (size_t)wave * resize_lds_words(S, S2, HW);
  u64 *bw = keys + S;
  int *list = (int *)(bw + HW);
  const int NC = (S + 63) >> 6;
  const u64 below = (1ull << lane) - 1ull;  // the lanes before this one
  const i64 total = (i64)a.Hv + (i64)a.Hv * (a.Hv - 1) / 2;
  for (i64 n = (i64)blockIdx.x * W + wave; n < a.N; n += (i64)gridDim.x * W) {
    const u64 *sg = a.src + (size_t)n * S * HW;
    const double *row = a.lpj + (size_t)n * a.L + a.S_perm;
    u64 *dg = a.dst + (size_t)n * S2 * HW;
    // ---- keys; on the way the best slot: largest key, lowest slot among equal ones
    u64 bk = 0ull;
    int bs = 0x7fffffff;
    for (int j = lane; j < S; j += 64) {
      const u64 k = seed_key(row[j]);
      keys[j] = k;
      if (k > bk) bk = k, bs = j;  // (ascending j: an equal key later in the lane's list never wins)
    }
    init_wave_sync();
    if (S2 < S) {
      // ---- shrink.  T = the S2-th largest key: the largest T with #{key >= T} >= S2 (no key is 0, S2 < S: T > 0)
      u64 kreg[RESIZE_KREG];
      const bool in_regs = NC <= RESIZE_KREG;
      if (in_regs) {
#pragma unroll
        for (int u = 0; u < RESIZE_KREG; u++) kreg[u] = 64 * u + lane < S ? keys[64 * u + lane] : 0ull;
      }
      u64 T = 0ull;
      for (int bit = 63; bit >= 0; bit--) {
        const u64 cand = T | (1ull << bit);
        int cnt = 0;
        if (in_regs) {
#pragma unroll
          for (int u = 0; u < RESIZE_KREG; u++) cnt += __popcll(__ballot(kreg[u] >= cand));  // (absent slots: key 0)
        } else {
          for (int c = 0; c < NC; c++) cnt += __popcll(__ballot(64 * c + lane < S && keys[64 * c + lane < S ? 64 * c + lane : 0] >= cand));
        }
        if (cnt >= S2) T = cand;
      }
      int n_gt = 0;
      for (int c = 0; c < NC; c++) n_gt += __popcll(__ballot(64 * c + lane < S && keys[64 * c + lane < S ? 64 * c + lane : 0] > T));
      // ---- members in ascending slot: every key above T, then keys equal to T while there is room
      int room = S2 - n_gt, pos = 0;  // wave-uniform
      for (int c = 0; c < NC; c++) {
        const int j = 64 * c + lane;
        const u64 k = j < S ? keys[j] : 0ull;
        const u64 eqm = __ballot(k == T);
        const int before = __popcll(eqm & below);
        const bool mem = k > T || (k == T && before < room);
        const u64 mm = __ballot(mem);
        const int at = pos + __popcll(mm & below);
        if (mem && at < S2) list[at] = j;
        const int took = __popcll(eqm);
        room -= took < room ? took : room;
        pos += __popcll(mm);
      }
      if (pos != S2 && lane == 0) atomicOr(a.err, EVO_ERR_BAD_ENTRY);  // (cannot happen: the search counts what the loop takes)
      for (int j2 = pos + lane; j2 < S2; j2 += 64) list[j2] = 0;
      init_wave_sync();
      // ---- the kept words, coalesced on the way out
      for (int i0 = 0; i0 < S2 * HW; i0 += 512) {  // eight loads in flight
        u64 v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
          const int i = i0 + 64 * u + lane;
          v[u] = 0ull;
          if (i < S2 * HW) {
            const int j2 = i / HW;
            v[u] = sg[(size_t)guard_index(list[j2], S, a.err) * HW + (i - j2 * HW)];
          }
        }
#pragma unroll
        for (int u = 0; u < 8; u++)
          if (i0 + 64 * u + lane < S2 * HW) dg[i0 + 64 * u + lane] = v[u];
      }
      for (int j2 = lane; j2 < S2; j2 += 64) {
        const int slot = guard_index(list[j2], S, a.err);
        a.dig[(size_t)n * S2 + j2] = make_digest(sg + (size_t)slot * HW, HW);
        a.src_slot[(size_t)n * S2 + j2] = slot;
      }
    } else {
      // ---- grow.  The best state's words
      const u64 gk = resize_wave_max_u64(bk);
      const int best = guard_index((int)wave_min_u32(bk == gk ? (unsigned)bs : 0x7fffffffu), S, a.err);
      for (int w = lane; w < HW; w += 64) bw[w] = sg[(size_t)best * HW + w];
      // ---- the held states in place
      for (int i0 = 0; i0 < S * HW; i0 += 512) {  // eight loads in flight
        u64 v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = i0 + 64 * u + lane < S * HW ? sg[i0 + 64 * u + lane] : 0ull;
#pragma unroll
        for (int u = 0; u < 8; u++)
          if (i0 + 64 * u + lane < S * HW) dg[i0 + 64 * u + lane] = v[u];
      }
      init_wave_sync();  // (the keys are done with: their place takes the hashes)
      u64 *hsh = keys;
      for (int j = lane; j < S; j += 64) {
        const u64 *sp = sg + (size_t)j * HW;
        u64 hs = 0, d = 0;
        int k = 0;
        for (int w = 0; w < HW; w++) {
          u64 bits = sp[w];
          hs = mix64(hs + bits + 1);
          while (bits) digest_add(d, k, w * 64 + pop_msb(bits));
        }
        hsh[j] = hs;
        a.dig[(size_t)n * S2 + j] = digest_close(d, k);
        a.src_slot[(size_t)n * S2 + j] = j;
      }
      init_wave_sync();
      // ---- the new slots from the neighbours of the best state
      const int need = S2 - S;
      const int bgw = a.bg ? (a.H - 1) >> 6 : 0;
      const u64 bgm = a.bg ? 0x8000000000000000ull >> ((a.H - 1) & 63) : 0ull;
      int filled = 0;
      for (i64 cb = 0; filled < need && cb < total; cb += 64) {
        const i64 c = cb + lane;
        bool fr = c < total;
        int la = 0, lb = -1;
        if (fr) remap_candidate(c, a.Hv, la, lb);
        const int wa = la >> 6, wb = lb >= 0 ? lb >> 6 : -1;
        const u64 ma = 0x8000000000000000ull >> (la & 63), mb = lb >= 0 ? 0x8000000000000000ull >> (lb & 63) : 0ull;
        u64 hc = 0, any = 0;
        for (int w = 0; w < HW; w++) {
          const u64 v = bw[w] ^ (w == wa ? ma : 0ull) ^ (w == wb ? mb : 0ull);
          hc = mix64(hc + v + 1);
          any |= w == bgw ? v & ~bgm : v;
        }
        if (!any) fr = false;  // no varying latent on
        for (int j0 = 0; j0 < S; j0 += 8) {
          u64 hv[8];
#pragma unroll
          for (int u = 0; u < 8; u++) hv[u] = hsh[j0 + u < S ? j0 + u : S - 1];
#pragma unroll
          for (int u = 0; u < 8; u++) {
            const int j = j0 + u;
            if (fr && j < S && hv[u] == hc) {  // (a held neighbour, and one pair in 2^64 otherwise): the words decide
              bool eq = true;
              for (int w = 0; w < HW; w++)
                eq = eq && sg[(size_t)j * HW + w] == (bw[w] ^ (w == wa ? ma : 0ull) ^ (w == wb ? mb : 0ull));
              if (eq) fr = false;
            }
          }
        }
        const u64 fm = __ballot(fr);
        const int rank = filled + __popcll(fm & below);
        if (fr && rank < need) {
          const int slot = S + rank;
          u64 *dw = dg + (size_t)slot * HW;
          u64 d = 0;
          int k = 0;
          for (int w = 0; w < HW; w++) {
            u64 bits = bw[w] ^ (w == wa ? ma : 0ull) ^ (w == wb ? mb : 0ull);
            dw[w] = bits;
            while (bits) digest_add(d, k, w * 64 + pop_msb(bits));
          }
          a.dig[(size_t)n * S2 + slot] = digest_close(d, k);
          a.src_slot[(size_t)n * S2 + slot] = -1;
        }
        filled += __popcll(fm);
      }
      if (filled < need && lane == 0) atomicOr(a.err, EVO_ERR_BAD_ENTRY);  // (the bound forbids it: the host refuses the result)
    }
    init_wave_sync();  // the next datapoint overwrites the share
  }
}
