// Posterior code readout: the dense E_q rows of the last statistics pass, compacted on the device.
//
// Per datapoint n (one wavefront each, CODES_WAVES datapoints per workgroup):
//   sparse code  the latents h with Es[n, h] > p_min, by descending Es[n, h], ties by ascending h, the first A of them:
//                idx[n, a] = h, p[n, a] = Es[n, h], m[n, a] = Ez[n, h] (ES3C) -- p and m are loaded from the row and
//                stored, no arithmetic touches them; unused slots hold idx = -1, p = m = 0.
//   nnz[n]       how many latents have Es[n, h] > p_min (before the cut to A: nnz > A says the code was truncated).
//   MAP state    map_slot[n] = first index of the largest entry of the lpj row (np.argmax), map_q[n] =
//                1 / (sum_s exp(lpj_s - lpj_max) + tiny), the weight the statistics pass gave that state (same shift,
//                same tiny), map_state[n] = the state's bits as ceil(H/8) bytes in np.packbits layout (slots below
//                S_perm are the permanent all-zero state: all bits zero).
//
// Selection without marks: round a picks the largest key (value, -h) that is smaller than the key picked in round
// a - 1, so the row is never written and the same loop serves three homes of the stripe h = lane (mod 64):
//   CODES_REG   H <= 64 CODES_R: CODES_R registers per lane, the row is read from memory once;
//   CODES_LDS   H <= CODES_LDS_H: the row is staged in LDS once (each wave its own H doubles);
//   CODES_GMEM  any H: the rounds re-read the row (L1 / L2 hits after the first).
// Each round: lane-local maximum over the stripe, then two DPP reductions (wave_max of the value, wave_min of the index
// among the lanes that hold it).  No atomics but the error word; every store is a plain vector store.
//
// map_q is reproducible on the host bit for bit (evo_amd/codes.py: codes_exp, codes_from_dense): codes_exp below uses
// IEEE add / multiply only (no contraction, no library exp), the lanes add their stripe in ascending s and the wave adds
// the 64 partial sums in an xor butterfly (32, 16, ... 1) -- commutative steps, so every lane ends with the same bits.
#pragma once
#include "common.hpp"

#define CODES_WAVES 4
#define CODES_R 8                 // register stripe: H <= 512
#define CODES_LDS_H 4096          // LDS stripe: CODES_WAVES x H doubles <= 128 KiB
#define CODES_MAX_A 64
enum { CODES_REG = 0, CODES_LDS = 1, CODES_GMEM = 2 };

struct CodesArgs {
  const double *Es;  // row n at Es + n ldE
  const double *Ez;  // or nullptr (EBSC)
  i64 ldE;
  const double *lpj;  // (N, L)
  const u64 *states;  // (N, S, HW)
  i64 N;
  int H, HW, S, S_perm, L, PB;
  int A;
  double p_min;
  int *idx;          // (N, A)   any output may be nullptr
  double *p, *m;     // (N, A)
  int *nnz;          // (N)
  int *map_slot;     // (N)
  double *map_q;     // (N)
  uint8_t *map_state;  // (N, PB)
  int *err;
};

// exp(x) for x <= 0 from IEEE additions and multiplications only, so that NumPy reproduces it bit for bit
// (codes.py: codes_exp is the same sequence): x = k ln2 + r with |r| <= ln2 / 2 (two-part ln2), Taylor polynomial of
// degree 13 by Horner (truncation 4e-18), scaled by 2^k.  Below -700 -- and for NaN -- the term is 0: it could not
// change a sum whose largest term is 1.  Relative error a few 1e-16.
__device__ __forceinline__ double codes_exp(double x) {
#pragma clang fp contract(off)
  if (!(x >= -700.0)) return 0.0;
  const double k = rint(x * 1.4426950408889634);
  const double r = (x - k * 0.693147180369123816490) - k * 1.90821492927058770002e-10;
  double q = 1.0 / 6227020800.0;
  q = q * r + 1.0 / 479001600.0;
  q = q * r + 1.0 / 39916800.0;
  q = q * r + 1.0 / 3628800.0;
  q = q * r + 1.0 / 362880.0;
  q = q * r + 1.0 / 40320.0;
  q = q * r + 1.0 / 5040.0;
  q = q * r + 1.0 / 720.0;
  q = q * r + 1.0 / 120.0;
  q = q * r + 1.0 / 24.0;
  q = q * r + 1.0 / 6.0;
  q = q * r + 0.5;
  q = q * r + 1.0;
  q = q * r + 1.0;
  return ldexp(q, (int)k);  // k >= -1011: the result is normal, the scaling exact
}

// lane-local best of the stripe: the largest value > p_min whose key (value, -h) lies below (lastv, -lasth); ascending
// h with a strict comparison keeps the lowest h among equals
#define CODES_CONSIDER(v, h)                                                                    \
  do {                                                                                          \
    const double _v = (v);                                                                      \
    if (_v > a.p_min && (_v < lastv || (_v == lastv && (h) > lasth)) && _v > bv) {              \
      bv = _v;                                                                                  \
      bh = (h);                                                                                 \
    }                                                                                           \
  } while (0)

template <int HOME>
__global__ __launch_bounds__(64 * CODES_WAVES) void posterior_codes_kernel(CodesArgs a) {
  extern __shared__ double codes_lds[];
  const int lane = lane_id(), wave = wave_id_uniform();
  const i64 n = (i64)blockIdx.x * CODES_WAVES + wave;
  if (n >= a.N) return;  // whole waves leave; nothing below synchronises across waves
  const int H = a.H;
  const double *row = a.Es + n * a.ldE;

  // ---- the stripe and nnz
  double reg[HOME == CODES_REG ? CODES_R : 1];
  double *sh = codes_lds + (size_t)wave * (HOME == CODES_LDS ? H : 0);
  int cnt = 0;
  if (HOME == CODES_REG) {
#pragma unroll
    for (int r = 0; r < CODES_R; r++) {
      const int h = lane + 64 * r;
      reg[r] = h < H ? row[h] : -1.0;  // (-1 never passes v > p_min >= 0)
      cnt += reg[r] > a.p_min;
    }
  } else {
    for (int h = lane; h < H; h += 64) {
      const double v = row[h];
      if (HOME == CODES_LDS) sh[h] = v;
      cnt += v > a.p_min;
    }
    if (HOME == CODES_LDS) lds_wave_fence();
  }
  cnt = wave_sum_i(cnt);

  // ---- A rounds; lane r keeps the winner of round r
  int mine = -1;
  if (a.idx || a.p || a.m) {
    double lastv = INFINITY;
    int lasth = -1;
    const int rounds = cnt < a.A ? cnt : a.A;
    for (int r = 0; r < rounds; r++) {
      double bv = -1.0;
      int bh = 0x7fffffff;
      if (HOME == CODES_REG) {
#pragma unroll
        for (int j = 0; j < CODES_R; j++) CODES_CONSIDER(reg[j], lane + 64 * j);
      } else if (HOME == CODES_LDS) {
        for (int h = lane; h < H; h += 64) CODES_CONSIDER(sh[h], h);
      } else {
        for (int h = lane; h < H; h += 64) CODES_CONSIDER(row[h], h);
      }
      const double wv = wave_max(bv);
      const int wh = (int)wave_min_u32(bv == wv ? (unsigned)bh : 0xFFFFFFFFu);
      if (!(wv > a.p_min)) break;  // (cannot happen for r < nnz; keeps a NaN-ridden row from looping on garbage)
      if (lane == r) mine = wh;
      lastv = wv;
      lasth = wh;
    }
    if (lane < a.A) {
      const i64 o = n * a.A + lane;
      const bool have = mine >= 0 && mine < H;
      if (a.idx) a.idx[o] = have ? mine : -1;
      if (a.p) a.p[o] = have ? row[mine] : 0.0;
      if (a.m) a.m[o] = have ? a.Ez[n * a.ldE + mine] : 0.0;
    }
  }
  if (a.nnz && lane == 0) a.nnz[n] = cnt;

  // ---- MAP state
  if (a.map_slot || a.map_q || a.map_state) {
    const double *lrow = a.lpj + n * a.L;
    double bv = -INFINITY;
    int bs = 0x7fffffff;
    for (int s = lane; s < a.L; s += 64) {
      const double v = lrow[s];
      if (v > bv || bs == 0x7fffffff) {
        bv = v;
        bs = s;
      }
    }
    const double mx = wave_max(bv);
    int slot = (int)wave_min_u32((bv == mx && bs != 0x7fffffff) ? (unsigned)bs : 0xFFFFFFFFu);
    slot = guard_index(slot, a.L, a.err);
    if (a.map_slot && lane == 0) a.map_slot[n] = slot;
    if (a.map_q) {
      const double B = 0.0 - mx;  // the statistics pass's shift (row_lse_kernel)
      double z = 0.0;
      for (int s = lane; s < a.L; s += 64) z += codes_exp(lrow[s] + B);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o, 64);
      if (lane == 0) a.map_q[n] = 1.0 / (z + EVO_F64_TINY);
    }
    if (a.map_state) {
      const int ks = slot - a.S_perm;  // < 0: the permanent all-zero state
      const u64 *sp = a.states + (n * a.S + (ks < 0 ? 0 : guard_index(ks, a.S, a.err))) * (i64)a.HW;
      for (int b = lane; b < a.PB; b += 64)  // (b >> 3 < HW because PB = ceil(H / 8), HW = ceil(H / 64))
        a.map_state[n * a.PB + b] = ks < 0 ? (uint8_t)0 : (uint8_t)(sp[b >> 3] >> (56 - 8 * (b & 7)));
    }
  }
}
