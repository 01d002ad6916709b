// K^n seeded by a BEAM of partial states: the greedy law of kernels_seed.hpp with the B best partial states kept per step
// instead of one, every one of them expanded.  One wavefront per datapoint, deterministic, no random numbers, no atomics.
// evo_amd/variational/utils.py: seed_states_beam_host is the NumPy mirror -- keep the two and the tests in step.
//
// THE LAW, per datapoint n (A = max_active steps, B = beam, Hv = H varying latents; quotas q_t of the greedy law, sum q_t = S):
//   beam        beam_0 = ({}).  beam_{t-1} = (P_0, ..., P_{b-1}) in rank order; a member carries its path (the order in which
//               its ancestry added its latents), its packed words and the score it was ranked with
//   candidates  of step t: for each parent rank r ascending, every j not in P_r, j < Hv, gives P_r + {j}.  ABSENT (key 0) when
//               the same set arises from an earlier parent: some r' < r with popcount(P_r XOR P_r') = 2, j being the latent
//               of P_r' that P_r lacks -- an exact test on the packed words, scores are never compared; the lower parent
//               rank keeps the state
//   scores      the greedy law's, in the arithmetic of the parent's own path order (w_1 .. w_{t-1}):
//               EBSC  e_j = (...((G_jj - 2 B_nj) + 2 G_{w_1 j}) + ...) + 2 G_{w_{t-1} j}, score = lpj(P_r) + pil_bar + pre1 e_j
//                     with lpj(P_r) the score the parent was ranked with (lpj({}) = pre1 yy)
//               ES3C  seed_form_blocks on the parent's path, then seed_score_sssc_step
//               without ljc and without the clamp; not finite, or (ES3C) det T <= 0: -inf, which is still a candidate and
//               ranks last
//   rank        all candidates of the step by descending score, ties by ascending parent rank, then ascending j.  The q_t
//               best go to the next q_t slots in rank order (slots step-major, as in the greedy law); the first B of them
//               are beam_t.  B <= S / A, so every beam member is a stored state
//   B = 1       is the greedy law, bit for bit: the device functions are those of kernels_seed.hpp and the EBSC e_j is summed
//               in the order in which seed_states_kernel accumulates it.
//   All S states are distinct (states of a step have t latents and absent candidates are never ranked), none is all-zero,
//   and parent 0 alone offers Hv - (t - 1) >= q_t candidates.
// Mapping: lane l owns latents l, l + 64, ...  Per step one pass per parent: its keys into the Hp-entry key array, the
// duplicates of earlier parents zeroed (lane r' tests parent r'), the q_t best of the pass by seed_rank_keys, merged by rank
// counting into the running list of the q_t best so far (key, parent rank, j; two buffers, swapped; an earlier parent wins a
// tie, so once the list is full a key that does not exceed its last entry is dropped before the rank search) -- the mechanism
// of sweep_swap_kernel.  Then the q_t states words(P_r) | bit j and their digests (seed_select_step's) leave the wave and
// the first B list entries become the new beam (paths, ascending lists, words, scores; double-buffered).  Every latent
// index, parent rank and slot that crossed LDS passes guard_index before it becomes an address.
// THE HOME OF THE EBSC e-VECTORS: none.  A parent's e_j is recomputed in registers from the rows of G in path order while its
// keys are formed (t - 1 coalesced row reads per parent and step, 28 B rows per datapoint at A = 8; G stays in L2 / the
// Infinity Cache).  Double-buffered in LDS they would take 2 B Hp 8 bytes (128 KB at B = 8, H = 1024: one wave per
// workgroup), and a per-wavefront buffer in global memory moves three rows per parent and step (old e, the row of G, new e)
// against (A - 1) / 2 = 3.5 here, for a buffer of 2 B Hp doubles per resident wave.  The bits are those of the definition.
// LDS per wave (SEED_LDS_BEAM of seed_lds_walk): the keys (Hp), the shared ES3C blocks (168 doubles), the pass's members
// (Q keys, 2 Q ints), the running lists (2 Q keys, 4 Q ints) and the two beams (2 B (HW + 1) words, 4 B A ints).
#pragma once
#include "common.hpp"
#include "kernels_seed.hpp"

#define SEED_BEAM_MAX 16

struct SeedBeamArgs {
  SeedArgs sd;  // the greedy kernel's arguments (cc / rows / masks unused)
  int B;        // beam
};

template <bool SSSC>
__global__ __launch_bounds__(256) void seed_states_beam_kernel(SeedBeamArgs ba) {
  extern __shared__ __attribute__((aligned(16))) unsigned char seed_beam_lds[];
  const SeedArgs &a = ba.sd;
  const int lane = lane_id(), wave = wave_id_uniform();
  const int W = (int)(blockDim.x >> 6);
  const int S = a.S, H = a.H, HW = a.HW, A = a.A, Hp = a.Hp, Q = a.Q, B = ba.B;
  const int NC = Hp >> 6;
  // one wavefront's share of LDS (seed_lds_walk); cc / base / path / sorted are absent: a beam member carries its own
  const SeedLdsView V = seed_lds_view(seed_beam_lds, wave, SEED_LDS_BEAM, SeedLdsShape{SSSC, Hp, HW, Q, A, B, 0, 0, 0});
  const SeedLds L = seed_carve(V);
  u64 *rk0 = V.rk[0], *rk1 = V.rk[1], *mwords = V.mwords;
  double *msc = V.msc;
  int *rp0 = V.rp[0], *rj0 = V.rj[0], *rp1 = V.rp[1], *rj1 = V.rj[1], *mpath = V.mpath, *msorted = V.msorted;
  u64 *keys = L.keys;
  const auto [pre1, pilb, s2inv] = seed_scalars<SSSC>(a.dpar);
  const int q_lo = S / A, q_rem = S - q_lo * A;
  for (i64 n = (i64)blockIdx.x * W + wave; n < a.N; n += (i64)gridDim.x * W) {
    const double *Bn = a.Bm + (size_t)n * H;
    const double yy = a.yy[n];
    u64 *dst = a.states + (size_t)n * S * HW;
    int cur = 0, nb = 1;  // beam_0 = ({}) in buffer 0
    for (int w = lane; w < HW; w += 64) mwords[w] = 0ull;
    if (lane == 0) msc[0] = pre1 * yy;  // EBSC: lpj({})
    seed_wave_sync();
    int slot0 = 0;
    for (int t = 1; t <= A; t++) {
      const int q = q_lo + (t <= q_rem ? 1 : 0);
      const u64 *cw = mwords + (size_t)cur * B * HW;
      const int *cp = mpath + cur * B * A, *cs = msorted + cur * B * A;
      const double *csc = msc + cur * B;
      int nrun = 0;  // the running list: entries 0 .. nrun - 1 of (ok, op, oj), by rank
      u64 *ok = rk0, *nk = rk1;
      int *op = rp0, *oj = rj0, *np = rp1, *nj = rj1;
      for (int r = 0; r < nb; r++) {
        const u64 *pw = cw + (size_t)r * HW;
        SeedLds Lp = L;
        Lp.path = const_cast<int *>(cp + r * A);
        const u64 thr = nrun == q ? ok[q - 1] : 0ull;  // a full list: only a key above its last entry can enter
        // ---- scores -> keys
        if (SSSC) {
          int act[SEED_MAX_A_SSSC];
          const double pbA = seed_form_blocks(a, Lp, t, lane, Bn, s2inv, act, nullptr);
          for (int c = 0; c < NC; c++) {
            const int j = 64 * c + lane;
            u64 key = 0ull;
            const bool live = j < H && !((pw[j < H ? j >> 6 : 0] >> (63 - (j & 63))) & 1ull);
            if (live) {
              key = seed_key(seed_score_sssc_step<false>(t, a, L.sh, act, pbA, j, Bn, yy, s2inv, nullptr));
              if (key <= thr) key = 0ull;
            }
            keys[j] = key;
          }
        } else {
          const double lpj_base = csc[r];  // lpj(P_r)
          for (int c0 = 0; c0 < NC; c0 += 4) {
            double e[4];
            int jj[4];
            bool in[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
              const int j = 64 * (c0 + u) + lane;
              in[u] = c0 + u < NC && j < H;
              jj[u] = in[u] ? j : 0;
              const double gd = in[u] ? a.Gd[jj[u]] : 0.0, bn = in[u] ? Bn[jj[u]] : 0.0;
              e[u] = gd - 2.0 * bn;
            }
            for (int i = 0; i < t - 1; i++) {  // the rows of G in path order
              const double *Gw = a.G + (size_t)guard_index(__builtin_amdgcn_readfirstlane(Lp.path[i]), H, a.err) * H;
              double gw[4];
#pragma unroll
              for (int u = 0; u < 4; u++) gw[u] = in[u] ? Gw[jj[u]] : 0.0;
#pragma unroll
              for (int u = 0; u < 4; u++) e[u] += 2.0 * gw[u];
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
              if (c0 + u >= NC) continue;
              u64 key = 0ull;
              const bool live = in[u] && !((pw[jj[u] >> 6] >> (63 - (jj[u] & 63))) & 1ull);
              if (live) {
                const double sc = lpj_base + pilb + pre1 * e[u];
                key = seed_key(sc);
                if (key <= thr) key = 0ull;
              }
              keys[64 * (c0 + u) + lane] = key;
            }
          }
        }
        seed_wave_sync();
        // ---- absent: the sets an earlier parent reaches (lane r' tests parent r')
        if (lane < r) {
          const u64 *ow = cw + (size_t)lane * HW;
          int cnt = 0, pj = 0;
          for (int w = 0; w < HW; w++) {
            const u64 x = ow[w] ^ pw[w];
            const u64 xj = x & ow[w];
            if (xj) pj = 64 * w + __clzll((long long)xj);
            cnt += __popcll(x);
          }
          if (cnt == 2 && pj < H) keys[pj] = 0ull;
        }
        seed_wave_sync();
        int live = 0;
        for (int c = 0; c < NC; c++) live += __popcll(__ballot(keys[64 * c + lane] != 0ull));
        const int qe = live < q ? live : q;
        if (qe > 0) {
          seed_rank_keys(L, Hp, qe, Q, lane);
          for (int i = lane; i < qe; i += 64) L.selk[i] = keys[guard_index(L.byrank[i], H, a.err)];  // the pass's keys by rank
          seed_wave_sync();
          // the merge: an old entry goes behind the new keys above it, a new one behind the old keys not below it
          for (int i = lane; i < nrun; i += 64) {
            const u64 k = ok[i];
            int rk = i;
            for (int m = 0; m < qe; m++) rk += L.selk[m] > k ? 1 : 0;
            if (rk < q) nk[rk] = k, np[rk] = op[i], nj[rk] = oj[i];
          }
          for (int m = lane; m < qe; m += 64) {
            const u64 k = L.selk[m];
            int rk = m;
            for (int i = 0; i < nrun; i++) rk += ok[i] >= k ? 1 : 0;
            if (rk < q) nk[rk] = k, np[rk] = r, nj[rk] = L.byrank[m];
          }
          seed_wave_sync();
          nrun = nrun + qe < q ? nrun + qe : q;
          u64 *tk = ok;
          ok = nk, nk = tk;
          int *ti = op;
          op = np, np = ti;
          ti = oj, oj = nj, nj = ti;
        }
      }
      // ---- the q states and their digests (nrun = q: parent 0 alone offers that many candidates)
      for (int idx = lane; idx < nrun * HW; idx += 64) {
        const int rk = idx / HW, w = idx - rk * HW;
        const int p = guard_index(op[rk], nb, a.err), j = guard_index(oj[rk], H, a.err);
        dst[(size_t)(slot0 + rk) * HW + w] = cw[(size_t)p * HW + w] | ((j >> 6) == w ? (0x8000000000000000ull >> (j & 63)) : 0ull);
      }
      if (a.dig)
        for (int rk = lane; rk < nrun; rk += 64) {
          const int p = guard_index(op[rk], nb, a.err), j = guard_index(oj[rk], H, a.err);
          const int *sorted = cs + p * A;
          u64 d = 0;
          int k = 0;
          bool ins = false;
          for (int i = 0; i < t - 1 && k < DIG_SLOTS; i++) {
            const int h = sorted[i];
            if (!ins && j < h) {
              digest_add(d, k, j);
              ins = true;
            }
            digest_add(d, k, h);
          }
          if (!ins) digest_add(d, k, j);
          a.dig[(size_t)n * S + slot0 + rk] = digest_close(d, t);
        }
      if (lane == 0 && nrun > 0) {  // rank 0: its score of every step, its path at the last
        if (a.lpj_path) a.lpj_path[(size_t)n * A + t - 1] = seed_unkey(ok[0]);
        if (a.path && t == A) {
          const int p = guard_index(op[0], nb, a.err);
          for (int i = 0; i < A - 1; i++) a.path[(size_t)n * A + i] = cp[p * A + i];
          a.path[(size_t)n * A + A - 1] = guard_index(oj[0], H, a.err);
        }
      }
      // ---- the first B list entries are beam_t
      const int nbn = nrun < B ? nrun : B;
      if (t < A) {
        u64 *nw = mwords + (size_t)(cur ^ 1) * B * HW;
        int *npth = mpath + (cur ^ 1) * B * A, *nsrt = msorted + (cur ^ 1) * B * A;
        double *nsc = msc + (cur ^ 1) * B;
        for (int idx = lane; idx < nbn * HW; idx += 64) {
          const int i = idx / HW, w = idx - i * HW;
          const int p = guard_index(op[i], nb, a.err), j = guard_index(oj[i], H, a.err);
          nw[(size_t)i * HW + w] = cw[(size_t)p * HW + w] | ((j >> 6) == w ? (0x8000000000000000ull >> (j & 63)) : 0ull);
        }
        if (lane < nbn) {
          const int p = guard_index(op[lane], nb, a.err), j = guard_index(oj[lane], H, a.err);
          int *pth = npth + lane * A, *srt = nsrt + lane * A;
          const int *psrt = cs + p * A;
          for (int i = 0; i < t - 1; i++) pth[i] = cp[p * A + i];
          pth[t - 1] = j;
          int k = 0;  // the parent's ascending list with j inserted
          bool ins = false;
          for (int i = 0; i < t - 1; i++) {
            const int h = psrt[i];
            if (!ins && j < h) srt[k++] = j, ins = true;
            srt[k++] = h;
          }
          if (!ins) srt[k] = j;
          nsc[lane] = seed_unkey(ok[lane]);
        }
      }
      seed_wave_sync();  // everybody has read the old beam and the lists
      cur ^= 1;
      nb = nbn;
      slot0 += q;
    }
  }
}
