// Samples from the model on the device: evoamd_generate, one wavefront per datapoint.
//
// The law is generate_data / generate_from_hidden of the reference (_models.py:73-99, bsc.py:27-57, sssc.py:66-102):
//   s_h ~ Bernoulli(pi_h) (u <= pi_h, as written there), or s given by the caller;
//   ES3C  z_A ~ N(mu_A, Psi_AA) on the active set A, 0 elsewhere;   EBSC  z = s;
//   y_mean = W z,   y = y_mean + sigma g,   g ~ N(0, I_D).
// The reference factorises Psi_AA per datapoint.  Here ONE H x H matrix F with F F^T = Psi (formed by the caller) serves
// every datapoint: the marginal of z_full = mu + F eps, eps ~ N(0, I_H), on A is exactly N(mu_A, Psi_AA), so
// z = s o (mu + F eps) has the reference's law for any A -- and only the rows of F that belong to active latents are read.
// THE STREAM (evo_amd/models/generate.py: generate_counter is its NumPy mirror -- keep the two and the tests in step).
// With i = first_index + n the datapoint's index in the whole data set (a set cut into shards is the same set):
//   s_h    = rng_u01(seed, i, GEN_PURPOSE + 0, h) <= pi_h                                   (rng_u01: kernels_evolve.hpp)
//   eps_j  = normal number j of purpose GEN_PURPOSE + 1,   g_d = normal number d of purpose GEN_PURPOSE + 2
//   normal number k of a purpose: pair p = k >> 1, u1 = rng_u01(.., 2 p), u2 = rng_u01(.., 2 p + 1),
//   r = sqrt(-2 log u1), t = 6.283185307179586 u2, even k: r cos t, odd k: r sin t   (u1 > 0: rng_u01 adds 0.5)
// The uniforms and so every bit of s are the mirror's bit for bit; log / sincos differ from NumPy's in the last places.
//
// Mapping: a word of s is ONE ballot -- lane l evaluates latent 64 w + 63 - l (the MSB-first layout of K^n).  ES3C: the
// H values of eps live in the wave's LDS slice (H doubles; none are drawn for a datapoint without an active latent).  The
// wave walks the set bits in ascending h (wave-uniform); z_h = mu_h + sum_j F[h, j] eps_j with the lanes striding over j
// along the row-major row of F and the fixed-order DPP reduction of common.hpp; the lane that owns latent h keeps z_h, so
// a word's 64 values of the dense z row (zeros included) leave in one coalesced store.  y_mean[d] = sum_h z_h Wt[h, d] in
// the same walk, the lanes striding over d along the row of W^T, in GEN_DCHUNKS register accumulators: D <= 64 GEN_DCHUNKS
// is one walk, a larger D repeats the walk per block of d (z_h is formed again, to the same bits).  Every sum has a fixed
// order, so a call repeats bit for bit.
#pragma once
#include "common.hpp"
#include "kernels_evolve.hpp"

#define GEN_PURPOSE 0x47454E0000000000ull
#define GEN_DCHUNKS 8

struct GenArgs {
  const double *Wt;    // (H, D): W^T, a latent's row contiguous
  const double *pies;  // (H)
  const double *mus;   // (H), ES3C
  const double *F;     // (H, H) row-major, F F^T = Psi, ES3C
  const u64 *s_in;     // (N, HW) given states, or nullptr: drawn
  double *y;           // (N, D)
  u64 *s_out;          // (N, HW) or nullptr
  double *z;           // (N, H) or nullptr (ES3C)
  double *y_mean;      // (N, D) or nullptr
  i64 N;
  int D, H, HW, sssc;
  u64 seed, first_index;
  double sigma;
};

__device__ __forceinline__ double gen_u01(u64 x0, u64 purpose, u64 index) {  // rng_u01 behind its first hash
  const u64 x = mix64(x0 ^ (purpose * 0xd1b54a32d192ed03ull + index + 0x632be59bd9b4e019ull));
  return ((double)(x >> 11) + 0.5) * (1.0 / 9007199254740992.0);
}
// the pair of normal numbers 2 p (cosine) and 2 p + 1 (sine) of a purpose
__device__ __forceinline__ void gen_normal_pair(u64 x0, u64 purpose, u64 p, double &even, double &odd) {
  const double u1 = gen_u01(x0, purpose, 2 * p), u2 = gen_u01(x0, purpose, 2 * p + 1);
  const double r = sqrt(-2.0 * log(u1));
  double sn, cs;
  sincos(6.283185307179586 * u2, &sn, &cs);
  even = r * cs;
  odd = r * sn;
}
// lanes of one wave hand eps to each other through LDS: make the writes visible, keep the compiler from moving accesses
// across (a wave's own LDS operations are issued in order)
__device__ __forceinline__ void gen_wave_sync() {
  __threadfence_block();
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ u64 gen_uniform(u64 v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
  return ((u64)hi << 32) | lo;
}

// Dynamic LDS: H doubles per wave (ES3C), none for EBSC.
__global__ __launch_bounds__(256) void generate_kernel(GenArgs a) {
  extern __shared__ double gen_lds[];
  const int lane = lane_id(), wave = wave_id_uniform();
  const int W = (int)(blockDim.x >> 6);
  const int D = a.D, H = a.H, HW = a.HW;
  double *eps = gen_lds + (size_t)wave * H;
  for (i64 n = (i64)blockIdx.x * W + wave; n < a.N; n += (i64)gridDim.x * W) {
    const u64 x0 = mix64(a.seed + 0x9e3779b97f4a7c15ull * (a.first_index + (u64)n + 1));
    // ---- s: one ballot per word, or the caller's words (bits past H dropped: they would become addresses)
    bool any = false;
    if (!a.s_in) {
      for (int w = 0; w < HW; w++) {
        const int h = 64 * w + 63 - lane;
        const bool bit = h < H && gen_u01(x0, GEN_PURPOSE, (u64)h) <= a.pies[h];
        const u64 word = __ballot(bit);
        any = any || word != 0ull;
        if (a.s_out && lane == 0) a.s_out[(size_t)n * HW + w] = word;
      }
    } else {
      for (int w = 0; w < HW; w++) {
        const int rem = H - 64 * w;
        const u64 word = gen_uniform(a.s_in[(size_t)n * HW + w]) & (rem >= 64 ? ~0ull : ~0ull << (64 - rem));
        any = any || word != 0ull;
        if (a.s_out && lane == 0) a.s_out[(size_t)n * HW + w] = word;
      }
    }
    // ---- eps (ES3C, only where a latent is active)
    if (a.sssc && any) {
      for (int p = lane; 2 * p < H; p += 64) {
        double e0, e1;
        gen_normal_pair(x0, GEN_PURPOSE + 1, (u64)p, e0, e1);
        eps[2 * p] = e0;
        if (2 * p + 1 < H) eps[2 * p + 1] = e1;
      }
      gen_wave_sync();
    }
    // ---- per block of 64 GEN_DCHUNKS values of d: the walk over the active latents, then the noise
    for (int d0 = 0; d0 < D; d0 += 64 * GEN_DCHUNKS) {
      double acc[GEN_DCHUNKS];
#pragma unroll
      for (int c = 0; c < GEN_DCHUNKS; c++) acc[c] = 0.0;
      for (int w = 0; w < HW; w++) {
        u64 bits;
        if (!a.s_in) {  // the same ballot again: cheaper than keeping HW words per wave
          const int h = 64 * w + 63 - lane;
          bits = __ballot(h < H && gen_u01(x0, GEN_PURPOSE, (u64)h) <= a.pies[h]);
        } else {
          const int rem = H - 64 * w;
          bits = gen_uniform(a.s_in[(size_t)n * HW + w]) & (rem >= 64 ? ~0ull : ~0ull << (64 - rem));
        }
        double zw = 0.0;  // z of the latent this lane owns in word w
        while (bits) {
          const int b = pop_msb(bits);
          const int h = 64 * w + b;  // < H: ascending
          double zh = 1.0;
          if (a.sssc) {
            const double *Fr = a.F + (size_t)h * H;
            double part = 0.0;
            for (int j = lane; j < H; j += 64) part += Fr[j] * eps[j];
            zh = a.mus[h] + wave_sum(part);
            if (lane == 63 - b) zw = zh;
          }
          const double *Wr = a.Wt + (size_t)h * D + d0;
#pragma unroll
          for (int c = 0; c < GEN_DCHUNKS; c++) {
            const int d = 64 * c + lane;
            if (d0 + 64 * c < D && d0 + d < D) acc[c] += zh * Wr[d];
          }
        }
        if (a.z && d0 == 0) {
          const int h = 64 * w + 63 - lane;
          if (h < H) a.z[(size_t)n * H + h] = zw;
        }
      }
#pragma unroll
      for (int c = 0; c < GEN_DCHUNKS; c++) {
        const int d = d0 + 64 * c + lane;
        if (d0 + 64 * c < D && d < D) {
          double g0, g1;
          gen_normal_pair(x0, GEN_PURPOSE + 2, (u64)(d >> 1), g0, g1);
          if (a.y_mean) a.y_mean[(size_t)n * D + d] = acc[c];
          a.y[(size_t)n * D + d] = acc[c] + a.sigma * ((d & 1) ? g1 : g0);
        }
      }
    }
    if (a.sssc) gen_wave_sync();  // the next datapoint overwrites eps
  }
}
