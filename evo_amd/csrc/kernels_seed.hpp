// K^n seeded from Theta and the data: greedy forward selection (matching pursuit) on the model's own lpj, one wavefront
// per datapoint.  Deterministic, no random numbers.  evo_amd/variational/utils.py: seed_states_host is the NumPy mirror
// -- keep the two and the tests in step.
//
// THE LAW, per datapoint n (A = max_active steps, Hv = H varying latents, A_0 = {}):
//   quotas   q_t = S / A + (t <= S mod A), t = 1..A, so sum q_t = S
//   step t   every j not in A_{t-1} is scored with score_j = lpj(A_{t-1} + {j}) -- the model's lpj without ljc and without
//            the lpj_reset_check clamp; a score that is not finite, or (ES3C) whose det T is not positive, is -inf;
//            latents are ranked by descending score, ties (and the -inf ones) by ascending j; the q_t best states
//            A_{t-1} + {j} go to the next q_t slots in rank order; the best one becomes A_t
//   slots    step-major: the state of step t and rank r sits at slot sum_{u<t} q_u + r.  Sizes are t and the states of a
//            step differ in j, so all S states are distinct and none is the all-zero state (S_perm keeps its own column).
// THE SCORES, in the Gram form of the lpj kernels (B = Y W, G = W^T W, yy = |y|^2):
//   EBSC  score_j = lpj(A_{t-1}) + pil_bar + pre1 (G_jj - 2 c_j), c_j = B_nj - sum_{i in A_{t-1}} G_ij; e_j = G_jj - 2 c_j is
//         kept in LDS across the steps (one row of G per step), lpj({}) = pre1 yy
//   ES3C  the k x k system of kernels_sssc.hpp's header, k = t, eliminated from scratch per candidate in registers
//         (template on k, so every loop unrolls): v = b - G_A mu, rr = yy - sum mu_i (b_i + v_i), T = I + Psi_A G_A / sigma2,
//         LU of [T | Psi_A v] with partial pivoting (first max |pivot|), det T with its sign from the pivots,
//         lpj = sum pil_bar - (log det T + rr / sigma2 - v^T T^-1 Psi_A v / sigma2^2) / 2.  The candidates of a step share
//         A_{t-1}: its blocks G_A, Psi_A, T_A, mu_A, b_A, v_A are formed once per step in LDS (SeedShared) and a candidate
//         adds its own row and column, 4 (t - 1)^2 multiply-adds, in front of the t^3 / 3 of the elimination: about
//         H sum_t (t^3 / 3 + 4 t^2) = 6e5 multiply-adds per datapoint at H = 512, A = 8.
// Mapping: lane l owns latents l, l + 64, ...; its scores go to LDS as 64-bit keys whose unsigned order is the order of
// the doubles (key 0 = latent already in A_{t-1}, below the key of -inf).  The q_t best by a THRESHOLD SEARCH over the
// keys: the q_t-th largest key T is built bit by bit (64 counting passes of ballots over the lane's own keys, which stay
// in registers while H <= 1024 and are re-read sixteen chunks per LDS round trip above that), the
// members are the keys above T and the first keys equal to T in ascending j; they are compacted into a list in ascending
// j, ranked by counting within the list (q_t^2 / 64 broadcast reads) and laid out by rank.  Then q_t HW words and q_t
// digests (the digest digest_kernel would compute: the first DIG_SLOTS of the ascending active latents, k = t) leave the
// wave with lane-strided stores.  Every latent index that crossed LDS passes guard_index before it becomes an address.
// LDS per wave: keys and e (Hp = Hv rounded up to 64 doubles each), the HW words of A_{t-1}, the shared blocks (168 doubles),
// the members' keys and two lists of their latents (max q_t each), the path and the ascending active set (A ints each).
// INCOMPLETE DATA (seed_states_masked_kernel, at the end of this file): the same law with G, B, yy over the datapoint's
// reliable entries; G(n) is the datapoint's own, so its diagonal and the winners' rows are formed from W and the mask.
#pragma once
#include "common.hpp"
#include "kernels_mstep.hpp"

#define SEED_MAX_A_SSSC 8
#define SEED_MAX_A_BSC 64
#define SEED_KREG 16  // chunks of keys a lane holds in registers during the threshold search
#define SEED_M (SEED_MAX_A_SSSC - 1)  // the active set in front of a step's candidates: at most 7 latents
#define SEED_SHARED_DOUBLES (3 * SEED_M * SEED_M + 3 * SEED_M)

struct SeedArgs {
  u64 *states;          // (N, S, HW) K^n
  u64 *dig;             // (N, S) or nullptr
  const double *Bm;     // (N, H) B = Y W
  const double *yy;     // (N)
  const double *G;      // EBSC (H, H)
  const double *Gd;     // EBSC (H) diag(G)
  const double2 *GP;    // ES3C (H, H) {G_ij, Psi_ij}
  const double2 *GPt;   // ES3C (H, H) its transpose {G_ji, Psi_ji} (seed_transpose_gp_kernel): the row of j, coalesced over j
  const double *mus;    // ES3C (H)
  const double *pil_bar;  // ES3C (H)
  const double *dpar;
  int *path;            // (N, A) or nullptr
  double *lpj_path;     // (N, A) or nullptr
  int *err;             // err[0] of the context's block (EVO_ERR_BAD_ENTRY)
  i64 N;
  int S, H, HW, A, Hp, Q;  // Hp: Hv rounded up to 64; Q: largest quota
  // incomplete data (seed_states_masked_kernel) only
  const double *W;      // (D, H)
  const uint8_t *mask;  // (N, D) x_infr
  double *rows;         // ES3C: R rows of Hp doubles per wavefront of the grid when they do not fit LDS, else nullptr
  int D, R;             // R: rows of G(n) a wavefront keeps (ES3C: A - 1 winners' rows and the diagonal; EBSC: 0)
};

// ONE WAVEFRONT'S SHARE OF LDS, described once for the host (which takes the total) and the kernels (which take their
// pointers from the same walk).  One description per kernel of the family; nothing else carves LDS in kernels_seed.hpp,
// kernels_seed_beam.hpp, kernels_sweep.hpp, kernels_sweep_swap.hpp and kernels_nbound.hpp.  8-byte regions first, then the
// ints; a masked, swap or neighbourhood-bound kernel's extras start behind the complete kernel's share rounded to 16 bytes.
#define SWEEP_PATH 16                 // sweeps: active latents of a parent kept as a list (ES3C reads at most 9)
#define SWEEP_MAX_P 64                // sweeps: parents per datapoint
#define SWAP_LIST SEED_MAX_A_BSC      // swap sweep: the parent's active latents as a list, every a of a scored parent
enum SeedLdsKind { SEED_LDS_GREEDY, SEED_LDS_GREEDY_MASKED, SEED_LDS_BEAM, SEED_LDS_FLIP, SEED_LDS_FLIP_MASKED, SEED_LDS_SWAP,
                   SEED_LDS_NBOUND, SEED_LDS_NBOUND_MASKED, SEED_LDS_KINDS };
struct SeedLdsShape {
  bool sssc;
  int Hp, HW, Q;      // Q: the largest quota (sweeps: n_keep)
  int A, B;           // seeding: max_active; the beam
  int D, rows_lds;    // masked: entries per datapoint; the rows of G(n) whose home is LDS (0: a.rows holds them)
  int S;              // swap sweep, neighbourhood bound: states per datapoint
};
// Two cursors walk the one description: SeedLdsOffsets yields byte offsets and the total (host, and the kernels for their
// share's size), SeedLdsPointers the typed pointers from a wavefront's home (kernels).  A region the kernel kind does not
// have stays 0 / nullptr.
struct SeedLdsOffsets {
  template <class T>
  using at = size_t;
  size_t pos = 0;
  template <class T>
  __host__ __device__ constexpr size_t take(size_t n) {
    const size_t o = pos;
    pos += n * sizeof(T);
    return o;
  }
  __host__ __device__ constexpr void align16() { pos = (pos + 15) & ~(size_t)15; }
  __host__ __device__ constexpr void seek(size_t to) { pos = to; }
  __host__ __device__ constexpr size_t used() const { return pos; }
};
struct SeedLdsPointers {
  template <class T>
  using at = T *;
  unsigned char *home, *p;
  template <class T>
  __host__ __device__ T *take(size_t n) {
    T *r = (T *)p;
    p = (unsigned char *)(r + n);
    return r;
  }
  __host__ __device__ void align16() { p = home + (((size_t)(p - home) + 15) & ~(size_t)15); }
  __host__ __device__ void seek(size_t to) { p = home + to; }
  __host__ __device__ size_t used() const { return (size_t)(p - home); }
};
template <class C>
struct SeedLdsRegions {
  template <class T>
  using at = typename C::template at<T>;
  at<u64> keys = {};
  at<double> cc = {};
  at<u64> base = {};
  at<double> sh = {};
  at<u64> selk = {};
  at<int> sel = {}, byrank = {}, path = {}, sorted = {};
  at<int> parents = {};                                   // sweeps: the parents' slots
  at<int> rank = {};                                      // neighbourhood bound: slot -> parent rank
  at<double> gd = {}, col = {}, rows = {};                // incomplete data
  at<int> dl = {};
  at<u64> rk[2] = {};                                     // beam, swap: the running lists (key, parent | a, j)
  at<int> rp[2] = {}, rj[2] = {};
  at<double> msc = {};                                    // the two beams
  at<u64> mwords = {};
  at<int> mpath = {}, msorted = {};
  at<int> full = {};                                      // swap sweep
  at<unsigned> held = {};
  size_t total = 0;  // rounded up to 16 bytes
};
__host__ __device__ constexpr size_t seed_lds_bytes(SeedLdsKind kind, const SeedLdsShape &s);
template <class C>
__host__ __device__ constexpr SeedLdsRegions<C> seed_lds_walk(SeedLdsKind kind, const SeedLdsShape &s, C c) {
  const bool nbound = kind == SEED_LDS_NBOUND || kind == SEED_LDS_NBOUND_MASKED;
  const bool flip_masked = kind == SEED_LDS_FLIP_MASKED || kind == SEED_LDS_NBOUND_MASKED;
  const bool beam = kind == SEED_LDS_BEAM, sweep = kind == SEED_LDS_FLIP || flip_masked || kind == SEED_LDS_SWAP || nbound;
  const size_t Hp = (size_t)s.Hp, Q = (size_t)s.Q;
  SeedLdsRegions<C> l;
  l.keys = c.template take<u64>(Hp);  // (masked EBSC seeding: also tmp, a row on its way into e)
  if (!beam) {
    l.cc = c.template take<double>(sweep && s.sssc ? 0 : Hp);  // EBSC e_j / c_j (the seeding kernels keep the region for ES3C too)
    l.base = c.template take<u64>((size_t)s.HW);              // the words of A_{t-1} / of the parent
  }
  l.sh = c.template take<double>(sweep && !s.sssc ? 0 : SEED_SHARED_DOUBLES);
  l.selk = c.template take<u64>(Q);
  if (beam) {
    l.rk[0] = c.template take<u64>(Q), l.rk[1] = c.template take<u64>(Q);
    l.msc = c.template take<double>((size_t)2 * s.B);
    l.mwords = c.template take<u64>((size_t)2 * s.B * s.HW);
  }
  l.sel = c.template take<int>(Q), l.byrank = c.template take<int>(Q);
  if (beam) {
    l.rp[0] = c.template take<int>(Q), l.rj[0] = c.template take<int>(Q);
    l.rp[1] = c.template take<int>(Q), l.rj[1] = c.template take<int>(Q);
    l.mpath = c.template take<int>((size_t)2 * s.B * s.A);
    l.msorted = c.template take<int>((size_t)2 * s.B * s.A);
  } else if (sweep) {
    l.path = c.template take<int>(SWEEP_PATH);
    l.parents = c.template take<int>(SWEEP_MAX_P);
  } else {
    l.path = c.template take<int>((size_t)s.A);
    l.sorted = c.template take<int>((size_t)s.A);
  }
  c.align16();
  // The extras of the sweeps start behind the flip kernel's share.  The cursor is set there from that kind's own total, not
  // left where the walk arrived: the same place, but measured -- the masked ES3C flip sweep, which fills the register file,
  // runs 3.6 % slower with its addresses formed from where the walk arrived, and masked EBSC seeding 1 % slower with them
  // formed from the total, so seeding keeps the walk's position
  if (flip_masked || kind == SEED_LDS_SWAP) c.seek(seed_lds_bytes(SEED_LDS_FLIP, s));
  if (kind == SEED_LDS_GREEDY_MASKED || flip_masked) {
    // EBSC sweep: the diagonal g_jj; the staged column of W; ES3C the rows of G(n) when LDS is their home; the reliable d
    if (flip_masked) l.gd = c.template take<double>(s.sssc ? 0 : Hp);
    l.col = c.template take<double>((size_t)s.D);
    l.rows = c.template take<double>((size_t)s.rows_lds * Hp);
    l.dl = c.template take<int>((size_t)s.D);
    c.align16();
  }
  if (kind == SEED_LDS_SWAP) {  // the running lists, the parent's active latents, the held pairs
    l.rk[0] = c.template take<u64>(Q), l.rk[1] = c.template take<u64>(Q);
    l.rp[0] = c.template take<int>(Q), l.rj[0] = c.template take<int>(Q);
    l.rp[1] = c.template take<int>(Q), l.rj[1] = c.template take<int>(Q);
    l.full = c.template take<int>(SWAP_LIST);
    l.held = c.template take<unsigned>((size_t)s.S);
    c.align16();
  }
  if (nbound) {  // behind the flip / masked flip share: up to S parents (the 64 slots of the share stay unused) and the ranks
    l.parents = c.template take<int>((size_t)s.S);
    l.rank = c.template take<int>((size_t)s.S);
    c.align16();
  }
  l.total = c.used();
  return l;
}
__host__ __device__ constexpr size_t seed_lds_bytes(SeedLdsKind kind, const SeedLdsShape &s) {
  return seed_lds_walk(kind, s, SeedLdsOffsets{}).total;
}
using SeedLdsView = SeedLdsRegions<SeedLdsPointers>;
// wave's share of the workgroup's dynamic LDS as pointers
__device__ __forceinline__ SeedLdsView seed_lds_view(unsigned char *lds, int wave, SeedLdsKind kind, const SeedLdsShape &s) {
  unsigned char *home = lds + (size_t)wave * seed_lds_bytes(kind, s);
  return seed_lds_walk(kind, s, SeedLdsPointers{home, home});
}
// The totals of the closed formulas this description replaced, evaluated on the host before they went: H = 100 (Hp = 128),
// 512, 1100 (Hp = 1152, HW = 18) and 1800 (Hp = 1856, HW = 29); masked ES3C with the rows in LDS and without.  The shape
// is {sssc, Hp, HW, Q, A, B, D, rows_lds, S}.
static_assert(seed_lds_bytes(SEED_LDS_GREEDY, SeedLdsShape{false, 128, 2, 3, 4, 0, 0, 0, 0}) == 3488, "greedy seeding");
static_assert(seed_lds_bytes(SEED_LDS_GREEDY, SeedLdsShape{true, 512, 8, 13, 5, 0, 0, 0, 0}) == 9856, "greedy seeding");
static_assert(seed_lds_bytes(SEED_LDS_GREEDY, SeedLdsShape{false, 1152, 18, 8, 8, 0, 0, 0, 0}) == 20112, "greedy seeding");
static_assert(seed_lds_bytes(SEED_LDS_GREEDY, SeedLdsShape{true, 1856, 29, 4, 3, 0, 0, 0, 0}) == 31360, "greedy seeding");
static_assert(seed_lds_bytes(SEED_LDS_GREEDY_MASKED, SeedLdsShape{false, 128, 2, 3, 4, 0, 24, 0, 0}) == 3776, "masked seeding");
static_assert(seed_lds_bytes(SEED_LDS_GREEDY_MASKED, SeedLdsShape{true, 128, 2, 3, 4, 0, 24, 4, 0}) == 7872, "masked seeding");
static_assert(seed_lds_bytes(SEED_LDS_GREEDY_MASKED, SeedLdsShape{true, 512, 8, 13, 5, 0, 300, 0, 0}) == 13456, "masked seeding");
static_assert(seed_lds_bytes(SEED_LDS_GREEDY_MASKED, SeedLdsShape{true, 1152, 18, 8, 8, 0, 37, 8, 0}) == 94288, "masked seeding");
static_assert(seed_lds_bytes(SEED_LDS_GREEDY_MASKED, SeedLdsShape{false, 1856, 29, 4, 3, 0, 4, 0, 0}) == 31408, "masked seeding");
static_assert(seed_lds_bytes(SEED_LDS_BEAM, SeedLdsShape{false, 128, 2, 3, 4, 1, 0, 0, 0}) == 2624, "beam seeding");
static_assert(seed_lds_bytes(SEED_LDS_BEAM, SeedLdsShape{true, 512, 8, 13, 5, 4, 0, 0, 0}) == 6960, "beam seeding");
static_assert(seed_lds_bytes(SEED_LDS_BEAM, SeedLdsShape{false, 1152, 18, 8, 8, 16, 0, 0, 0}) == 17856, "beam seeding");
static_assert(seed_lds_bytes(SEED_LDS_BEAM, SeedLdsShape{true, 1856, 29, 4, 3, 2, 0, 0, 0}) == 17440, "beam seeding");
static_assert(seed_lds_bytes(SEED_LDS_FLIP, SeedLdsShape{false, 128, 2, 3, 0, 0, 0, 0, 0}) == 2432, "flip sweep");
static_assert(seed_lds_bytes(SEED_LDS_FLIP, SeedLdsShape{true, 128, 2, 3, 0, 0, 0, 0, 0}) == 2752, "flip sweep");
static_assert(seed_lds_bytes(SEED_LDS_FLIP, SeedLdsShape{false, 1152, 18, 8, 0, 0, 0, 0, 0}) == 19024, "flip sweep");
static_assert(seed_lds_bytes(SEED_LDS_FLIP, SeedLdsShape{true, 1856, 29, 4, 0, 0, 0, 0, 0}) == 16816, "flip sweep");
static_assert(seed_lds_bytes(SEED_LDS_FLIP_MASKED, SeedLdsShape{true, 128, 2, 3, 0, 0, 24, 10, 0}) == 13280, "masked flip sweep");
static_assert(seed_lds_bytes(SEED_LDS_FLIP_MASKED, SeedLdsShape{false, 512, 8, 13, 0, 0, 300, 0, 0}) == 16480, "masked flip sweep");
static_assert(seed_lds_bytes(SEED_LDS_FLIP_MASKED, SeedLdsShape{true, 512, 8, 13, 0, 0, 300, 10, 0}) == 50592, "masked flip sweep");
static_assert(seed_lds_bytes(SEED_LDS_FLIP_MASKED, SeedLdsShape{true, 1152, 18, 8, 0, 0, 37, 0, 0}) == 11600, "masked flip sweep");
static_assert(seed_lds_bytes(SEED_LDS_FLIP_MASKED, SeedLdsShape{false, 1856, 29, 4, 0, 0, 4, 0, 0}) == 45216, "masked flip sweep");
static_assert(seed_lds_bytes(SEED_LDS_SWAP, SeedLdsShape{false, 128, 2, 3, 0, 0, 0, 0, 30}) == 2912, "swap sweep");
static_assert(seed_lds_bytes(SEED_LDS_SWAP, SeedLdsShape{true, 512, 8, 13, 0, 0, 0, 0, 64}) == 6960, "swap sweep");
static_assert(seed_lds_bytes(SEED_LDS_SWAP, SeedLdsShape{false, 1152, 18, 8, 0, 0, 0, 0, 200}) == 20336, "swap sweep");
static_assert(seed_lds_bytes(SEED_LDS_SWAP, SeedLdsShape{true, 1856, 29, 4, 0, 0, 0, 0, 6}) == 17232, "swap sweep");
// The neighbourhood bound (kernels_nbound.hpp): the flip / masked flip share at Q = 0 plus 8 S bytes, worked out by hand
static_assert(seed_lds_bytes(SEED_LDS_NBOUND, SeedLdsShape{false, 128, 2, 0, 0, 0, 0, 0, 30}) == 2624, "neighbourhood bound");
static_assert(seed_lds_bytes(SEED_LDS_NBOUND, SeedLdsShape{true, 512, 8, 0, 0, 0, 0, 0, 200}) == 7424, "neighbourhood bound");
static_assert(seed_lds_bytes(SEED_LDS_NBOUND, SeedLdsShape{false, 128, 2, 3, 0, 0, 0, 0, 30}) ==
                  seed_lds_bytes(SEED_LDS_FLIP, SeedLdsShape{false, 128, 2, 3, 0, 0, 0, 0, 0}) + 240, "neighbourhood bound");
static_assert(seed_lds_bytes(SEED_LDS_NBOUND_MASKED, SeedLdsShape{true, 128, 2, 0, 0, 0, 24, 10, 12}) == 13328, "masked neighbourhood bound");
static_assert(seed_lds_bytes(SEED_LDS_NBOUND_MASKED, SeedLdsShape{false, 512, 8, 0, 0, 0, 300, 0, 256}) == 18320, "masked neighbourhood bound");
static_assert(seed_lds_bytes(SEED_LDS_NBOUND_MASKED, SeedLdsShape{true, 512, 8, 13, 0, 0, 300, 10, 64}) ==
                  seed_lds_bytes(SEED_LDS_FLIP_MASKED, SeedLdsShape{true, 512, 8, 13, 0, 0, 300, 10, 0}) + 512, "masked neighbourhood bound");

__device__ __forceinline__ void seed_wave_sync() {
  __threadfence_block();
  __builtin_amdgcn_wave_barrier();
}
// the order of the doubles as an unsigned order; never 0 (the key of -inf is 0x000F..F)
__device__ __forceinline__ u64 seed_key(double v) {
  if (!(fabs(v) <= 1.7976931348623157e308)) v = -__builtin_inf();  // NaN, +inf, -inf
  v += 0.0;  // -0 -> +0: equal scores, equal keys
  const u64 b = (u64)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double seed_unkey(u64 k) {
  const u64 b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
  return __longlong_as_double((long long)b);
}
__device__ __forceinline__ u64 seed_uniform(u64 v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
  return ((u64)hi << 32) | lo;
}

// What the candidates of one step share (ES3C): the blocks of the active set A_{t-1}, m = t - 1 <= 7 latents, formed once
// per step by the wave and read back as LDS broadcasts.  Row stride SEED_M.
struct SeedShared {
  double *GA, *PA, *TA;    // G_A, Psi_A, T_A = I + Psi_A G_A / sigma2
  double *muA, *bA, *vA;   // mu_A, B_nA, v_A = B_nA - G_A mu_A
};

// The elimination every ES3C score ends in (seed_score_sssc; kernels_sweep.hpp): t = [T | Psi_A v] of a K x K system, v, the
// state's sum of pil_bar and rr; returns its lpj, -inf when det T is not positive.
template <int K>
__device__ __forceinline__ double seed_eliminate(double (&t)[K][K + 1], const double (&v)[K], double pb, double rr, double s2inv) {
  // LU with partial pivoting (first max |pivot|); rows swap by selects, so nothing is indexed at run time
  LogDetAcc ld;
  bool neg = false, zero = false;
  double rpiv[K];
#pragma unroll
  for (int c = 0; c < K; c++) {
    int r = c;
    double best = fabs(t[c][c]);
#pragma unroll
    for (int i = c + 1; i < K; i++) {
      const double x = fabs(t[i][c]);
      if (x > best) best = x, r = i;
    }
#pragma unroll
    for (int i = c + 1; i < K; i++) {
      const bool sw = r == i;
#pragma unroll
      for (int m = c; m <= K; m++) {
        const double x = t[c][m], y = t[i][m];
        t[c][m] = sw ? y : x;
        t[i][m] = sw ? x : y;
      }
    }
    neg = neg != (r != c);
    const double piv = t[c][c];
    neg = neg != (piv < 0.0);
    zero = zero || !(fabs(piv) > 0.0);  // 0 or NaN
    ld.mul(piv);
    const double rp = fast_rcp(piv);
    rpiv[c] = rp;
#pragma unroll
    for (int i = c + 1; i < K; i++) {
      const double f = t[i][c] * rp;
#pragma unroll
      for (int m = c + 1; m <= K; m++) t[i][m] -= f * t[c][m];
    }
  }
  // back substitution: x = T^-1 Psi_A v, quad = v^T x (v in the pivoted order of the columns = the original order)
  double x[K], quad = 0.0;
#pragma unroll
  for (int i = K - 1; i >= 0; i--) {
    double s = t[i][K];
#pragma unroll
    for (int m = i + 1; m < K; m++) s -= t[i][m] * x[m];
    x[i] = s * rpiv[i];
    quad += v[i] * x[i];
  }
  if (neg || zero) return -__builtin_inf();
  return pb - 0.5 * (ld.value() + rr * s2inv - quad * s2inv * s2inv);
}

// ES3C lpj of the state act[0..K-2] + {j} for one datapoint (file header).  act is wave-uniform, j the lane's latent.  The
// bordered system: only the row and the column of j are the lane's own -- 2 (K - 1) coalesced loads of {G, Psi} (the row
// from the transposed table: gathered from GP it would fetch a 128-byte line per 16 bytes used), the diagonal entry and
// 4 (K - 1)^2 multiply-adds in front of the elimination.
// MASKED (incomplete data): G is the datapoint's own -- rows[i * Hp + j] = G(n)_{act[i], j} (symmetric: row and column at once)
// and rows[(R - 1) * Hp + j] its diagonal, formed by seed_states_masked_kernel; only Psi comes from the tables.
template <int K, bool MASKED>
__device__ __forceinline__ double seed_score_sssc(const SeedArgs &a, const SeedShared &sh, const int *act, double pbA, int j,
                                                  const double *__restrict__ Bn, double yy, double s2inv,
                                                  const double *rows = nullptr) {
  constexpr int M = K - 1, MM = M > 0 ? M : 1;
  double gc[MM], pc[MM], gr[MM], pr[MM];  // G_ij, Psi_ij, G_ji, Psi_ji, i in A
  double gjj, pjj;
  if constexpr (MASKED) {
#pragma unroll
    for (int i = 0; i < M; i++) {
      gc[i] = gr[i] = rows[(size_t)i * a.Hp + j];
      pc[i] = a.GP[(size_t)act[i] * a.H + j].y, pr[i] = a.GPt[(size_t)act[i] * a.H + j].y;
    }
    gjj = rows[(size_t)(a.R - 1) * a.Hp + j], pjj = a.GP[(size_t)j * a.H + j].y;
  } else {
#pragma unroll
    for (int i = 0; i < M; i++) {
      const double2 c = a.GP[(size_t)act[i] * a.H + j], r = a.GPt[(size_t)act[i] * a.H + j];
      gc[i] = c.x, pc[i] = c.y, gr[i] = r.x, pr[i] = r.y;
    }
    const double2 djj = a.GP[(size_t)j * a.H + j];
    gjj = djj.x, pjj = djj.y;
  }
  const double muj = a.mus[j], bj = Bn[j];
  const double pb = pbA + a.pil_bar[j];
  double v[K], rr = yy;
  {
    double s = bj - gjj * muj;
#pragma unroll
    for (int i = 0; i < M; i++) {
      s -= gr[i] * sh.muA[i];
      v[i] = sh.vA[i] - gc[i] * muj;
      rr -= sh.muA[i] * (sh.bA[i] + v[i]);
    }
    v[M] = s;
    rr -= muj * (bj + s);
  }
  double t[K][K + 1];  // [T | Psi v] of the bordered system
  {
    double corner = pjj * gjj, rhs_m = pjj * v[M];
#pragma unroll
    for (int i = 0; i < M; i++) {
      double col = pc[i] * gjj, row = pjj * gr[i], rhs = pc[i] * v[M];
#pragma unroll
      for (int l = 0; l < M; l++) {
        col += sh.PA[i * SEED_M + l] * gc[l];  // (Psi_A G_Aj)_i
        row += pr[l] * sh.GA[l * SEED_M + i];  // (Psi_jA G_A)_i
        rhs += sh.PA[i * SEED_M + l] * v[l];
        t[i][l] = sh.TA[i * SEED_M + l] + s2inv * (pc[i] * gr[l]);
      }
      t[i][M] = s2inv * col;
      t[M][i] = s2inv * row;
      t[i][K] = rhs;
      corner += pr[i] * gc[i];
      rhs_m += pr[i] * v[i];
    }
    t[M][M] = 1.0 + s2inv * corner;
    t[M][K] = rhs_m;
  }
  return seed_eliminate<K>(t, v, pb, rr, s2inv);
}

// Psi is not symmetric (kernels_sssc.hpp), so the rows {G_ja, Psi_ja} of the candidates come from a transposed copy of GP,
// rebuilt by every call (H x H entries: 4 MB at H = 512).
__global__ __launch_bounds__(256) void seed_transpose_gp_kernel(const double2 *__restrict__ GP, int H, double2 *__restrict__ GPt) {
  const i64 idx = (i64)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (i64)H * H) return;
  const int r = (int)(idx / H), c = (int)(idx - (i64)r * H);
  GPt[idx] = GP[(size_t)c * H + r];
}

// One wavefront's share of LDS as pointers: the regions every kernel of the family hands to the shared device functions
struct SeedLds {
  u64 *keys;
  double *cc;
  u64 *base;
  SeedShared sh;
  u64 *selk;
  int *sel, *byrank, *path, *sorted;
};
__device__ __forceinline__ SeedLds seed_carve(const SeedLdsView &v) {
  SeedLds L;
  L.keys = v.keys, L.cc = v.cc, L.base = v.base;
  double *shd = v.sh;
  L.sh = {shd, shd + SEED_M * SEED_M, shd + 2 * SEED_M * SEED_M, shd + 3 * SEED_M * SEED_M,
          shd + 3 * SEED_M * SEED_M + SEED_M, shd + 3 * SEED_M * SEED_M + 2 * SEED_M};
  L.selk = v.selk, L.sel = v.sel, L.byrank = v.byrank, L.path = v.path, L.sorted = v.sorted;
  return L;
}

// The three scalars of dpar the scores need: EBSC pre1 and pil_bar, ES3C 1 / sigma2 (the others 0)
struct SeedScalars {
  double pre1, pilb, s2inv;
};
template <bool SSSC>
__device__ __forceinline__ SeedScalars seed_scalars(const double *dpar) {
  return {SSSC ? 0.0 : dpar[DP_PRE1], SSSC ? 0.0 : dpar[DP_PILBAR], SSSC ? dpar[DP_S2INV] : 0.0};
}

// Incomplete data: the reliable d of the mask row mn into dl in ascending order (ballots); returns how many.  The caller
// synchronises before dl is read.
__device__ __forceinline__ int seed_list_reliable(const uint8_t *mn, int D, int lane, int *dl) {
  int nd = 0;
  for (int d0 = 0; d0 < D; d0 += 64) {
    const int d = d0 + lane;
    const bool on = d < D && mn[d < D ? d : 0] != 0;
    const u64 b = __ballot(on);
    if (on) dl[nd + __popcll(b & ((1ull << lane) - 1ull))] = d;
    nd += __popcll(b);
  }
  return nd;
}

// ES3C, once per step: act[] = A_{t-1} as wave-uniform values and its blocks in LDS (SeedShared); returns sum pil_bar over
// A_{t-1}.  rows: nullptr = G from the tables, else the datapoint's own rows (seed_score_sssc).
__device__ __forceinline__ double seed_form_blocks(const SeedArgs &a, const SeedLds &L, int t, int lane, const double *__restrict__ Bn,
                                                   double s2inv, int *act, const double *rows) {
  const SeedShared &sh = L.sh;
  const int *path = L.path;
  const int H = a.H;
  const int m = t - 1;
  double pbA = 0.0;
#pragma unroll
  for (int i = 0; i < SEED_MAX_A_SSSC; i++)
    act[i] = i < m ? guard_index(__builtin_amdgcn_readfirstlane(path[i]), H, a.err) : 0;
  // the blocks of A_{t-1}: lane i m + c holds entry (i, c)
  const int bi = lane / (m > 0 ? m : 1), bc = lane - bi * (m > 0 ? m : 1);
  const bool in_block = m > 0 && lane < m * m;
  if (in_block) {
    const int hc = guard_index(path[bc], H, a.err);
    const double2 e = a.GP[(size_t)guard_index(path[bi], H, a.err) * H + hc];
    sh.GA[bi * SEED_M + bc] = rows ? rows[(size_t)bi * a.Hp + hc] : e.x;
    sh.PA[bi * SEED_M + bc] = e.y;
  }
  if (lane < m) {
    const int h = guard_index(path[lane], H, a.err);
    sh.muA[lane] = a.mus[h];
    sh.bA[lane] = Bn[h];
  }
  seed_wave_sync();
  if (in_block) {
    double s = 0.0;
    for (int l = 0; l < m; l++) s += sh.PA[bi * SEED_M + l] * sh.GA[l * SEED_M + bc];
    sh.TA[bi * SEED_M + bc] = (bi == bc ? 1.0 : 0.0) + s2inv * s;
  }
  if (lane < m) {
    double s = sh.bA[lane];
    for (int l = 0; l < m; l++) s -= sh.GA[lane * SEED_M + l] * sh.muA[l];
    sh.vA[lane] = s;
  }
  for (int i = 0; i < m; i++) pbA += a.pil_bar[guard_index(path[i], H, a.err)];
  seed_wave_sync();
  return pbA;
}

template <bool MASKED>
__device__ __forceinline__ double seed_score_sssc_step(int t, const SeedArgs &a, const SeedShared &sh, const int *act, double pbA, int j,
                                                       const double *__restrict__ Bn, double yy, double s2inv, const double *rows) {
  switch (t) {
    case 1: return seed_score_sssc<1, MASKED>(a, sh, act, pbA, j, Bn, yy, s2inv, rows);
    case 2: return seed_score_sssc<2, MASKED>(a, sh, act, pbA, j, Bn, yy, s2inv, rows);
    case 3: return seed_score_sssc<3, MASKED>(a, sh, act, pbA, j, Bn, yy, s2inv, rows);
    case 4: return seed_score_sssc<4, MASKED>(a, sh, act, pbA, j, Bn, yy, s2inv, rows);
    case 5: return seed_score_sssc<5, MASKED>(a, sh, act, pbA, j, Bn, yy, s2inv, rows);
    case 6: return seed_score_sssc<6, MASKED>(a, sh, act, pbA, j, Bn, yy, s2inv, rows);
    case 7: return seed_score_sssc<7, MASKED>(a, sh, act, pbA, j, Bn, yy, s2inv, rows);
    default: return seed_score_sssc<8, MASKED>(a, sh, act, pbA, j, Bn, yy, s2inv, rows);
  }
}

// The q largest keys of L.keys (q <= keys above 0) -> their latents in L.byrank[0..q-1], descending key, ties by ascending
// j (file header: threshold search, members in ascending j, rank by counting).  Ends synchronised.
__device__ __forceinline__ void seed_rank_keys(const SeedLds &L, int Hp, int q, int Q, int lane) {
  const int NC = Hp >> 6, NG = (NC + SEED_KREG - 1) / SEED_KREG;  // chunks of 64 latents, register loads of SEED_KREG chunks
  u64 *keys = L.keys, *selk = L.selk;
  int *sel = L.sel, *byrank = L.byrank;
  // ---- T = the q-th largest key: the largest T with #{key >= T} >= q (q <= live latents: T > 0).  SEED_KREG chunks
  // of keys at a time in registers, so that one LDS round trip serves that many ballots; H <= 1024: they stay there
  u64 kreg[SEED_KREG];
  if (NG == 1) {
#pragma unroll
    for (int u = 0; u < SEED_KREG; u++) kreg[u] = u < NC ? keys[64 * u + lane] : 0ull;
  }
  u64 T = 0ull;
  for (int bit = 63; bit >= 0; bit--) {
    const u64 cand = T | (1ull << bit);
    int cnt = 0;
    for (int g = 0; g < NG; g++) {
      if (NG > 1) {
#pragma unroll
        for (int u = 0; u < SEED_KREG; u++) kreg[u] = SEED_KREG * g + u < NC ? keys[64 * (SEED_KREG * g + u) + lane] : 0ull;
      }
#pragma unroll
      for (int u = 0; u < SEED_KREG; u++) cnt += __popcll(__ballot(kreg[u] >= cand));  // (absent chunks: key 0)
    }
    if (cnt >= q) T = cand;
  }
  // ---- members in ascending j: every key above T, then keys equal to T while there is room
  int n_gt = 0;
  for (int g = 0; g < NG; g++) {
    if (NG > 1) {
#pragma unroll
      for (int u = 0; u < SEED_KREG; u++) kreg[u] = SEED_KREG * g + u < NC ? keys[64 * (SEED_KREG * g + u) + lane] : 0ull;
    }
#pragma unroll
    for (int u = 0; u < SEED_KREG; u++) n_gt += __popcll(__ballot(kreg[u] > T));
  }
  int room = q - n_gt, pos = 0;  // wave-uniform
  for (int c = 0; c < NC; c++) {
    const int j = 64 * c + lane;
    const u64 k = keys[j];
    const u64 eqm = __ballot(k == T);
    const int before = __popcll(eqm & ((1ull << lane) - 1ull));
    const bool mem = k > T || (k == T && before < room);
    const u64 mm = __ballot(mem);
    const int at = pos + __popcll(mm & ((1ull << lane) - 1ull));
    if (mem && at < Q) sel[at] = j, selk[at] = k;
    const int took = __popcll(eqm);
    room -= took < room ? took : room;
    pos += __popcll(mm);
  }
  seed_wave_sync();
  // ---- rank within the list (it is in ascending j): keys above mine, equal keys in front of me
  for (int m0 = 0; m0 < q; m0 += 64) {
    const int m = m0 + lane;
    const bool mine = m < q;
    const int jm = sel[mine ? m : 0];
    const u64 km = selk[mine ? m : 0];
    int rank = 0;
#pragma unroll 8
    for (int i = 0; i < q; i++) {
      const u64 ki = selk[i];
      rank += (ki > km || (ki == km && i < m)) ? 1 : 0;
    }
    if (mine && rank < Q) byrank[rank] = jm;
  }
  seed_wave_sync();
}

// From the keys of step t in LDS (the caller has synchronised) to the q states and digests of datapoint n in slots
// slot0 .. slot0 + q - 1, the path entry and the winner in A_t (path, sorted, base): file header.  Returns the winner's
// latent (wave-uniform) and its score in sw; the caller synchronises before the next step reads path / sorted / base.
__device__ __forceinline__ int seed_select_step(const SeedArgs &a, const SeedLds &L, i64 n, int t, int q, int slot0, int lane, double &sw_out) {
  const int S = a.S, H = a.H, HW = a.HW, A = a.A, Hp = a.Hp, Q = a.Q;
  u64 *keys = L.keys, *base = L.base;
  int *byrank = L.byrank, *path = L.path, *sorted = L.sorted;
  u64 *dst = a.states + (size_t)n * S * HW;
  seed_rank_keys(L, Hp, q, Q, lane);
  // ---- the q states and their digests
  for (int idx = lane; idx < q * HW; idx += 64) {
    const int r = idx / HW, w = idx - r * HW;
    const int j = guard_index(byrank[r], H, a.err);
    dst[(size_t)(slot0 + r) * HW + w] = base[w] | ((j >> 6) == w ? (0x8000000000000000ull >> (j & 63)) : 0ull);
  }
  if (a.dig)
    for (int r = lane; r < q; r += 64) {
      const int j = guard_index(byrank[r], H, a.err);
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
      a.dig[(size_t)n * S + slot0 + r] = digest_close(d, t);
    }
  // ---- the winner joins the active set
  const int jw = guard_index(__builtin_amdgcn_readfirstlane(byrank[0]), H, a.err);
  const double sw = seed_unkey(seed_uniform(keys[jw]));
  if (lane == 0) {
    if (a.path) a.path[(size_t)n * A + t - 1] = jw;
    if (a.lpj_path) a.lpj_path[(size_t)n * A + t - 1] = sw;
  }
  sw_out = sw;
  seed_wave_sync();  // everybody has read sorted / base / keys
  if (lane == 0) {
    path[t - 1] = jw;
    int i = t - 1;  // insertion into the ascending list
    while (i > 0 && sorted[i - 1] > jw) {
      sorted[i] = sorted[i - 1];
      i--;
    }
    sorted[i] = jw;
    base[jw >> 6] |= 0x8000000000000000ull >> (jw & 63);
  }
  return jw;
}

template <bool SSSC>
__global__ __launch_bounds__(256) void seed_states_kernel(SeedArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char seed_lds[];
  const int lane = lane_id(), wave = wave_id_uniform();
  const int W = (int)(blockDim.x >> 6);
  const int S = a.S, H = a.H, HW = a.HW, A = a.A, Hp = a.Hp, Q = a.Q;
  const int NC = Hp >> 6;  // chunks of 64 latents
  const SeedLds L = seed_carve(seed_lds_view(seed_lds, wave, SEED_LDS_GREEDY, SeedLdsShape{SSSC, Hp, HW, Q, A, 0, 0, 0, 0}));
  u64 *keys = L.keys, *base = L.base;
  double *cc = L.cc;
  const auto [pre1, pilb, s2inv] = seed_scalars<SSSC>(a.dpar);
  const int q_lo = S / A, q_rem = S - q_lo * A;
  for (i64 n = (i64)blockIdx.x * W + wave; n < a.N; n += (i64)gridDim.x * W) {
    const double *Bn = a.Bm + (size_t)n * H;
    const double yy = a.yy[n];
    for (int w = lane; w < HW; w += 64) base[w] = 0ull;
    if (!SSSC)  // e_j = G_jj - 2 B_nj; eight chunks of loads in flight
      for (int c0 = 0; c0 < NC; c0 += 8) {
        double gd[8], bn[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
          const int j = 64 * (c0 + u) + lane;
          const bool in = c0 + u < NC && j < H;
          gd[u] = in ? a.Gd[j] : 0.0;
          bn[u] = in ? Bn[j] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; u++)
          if (c0 + u < NC) cc[64 * (c0 + u) + lane] = gd[u] - 2.0 * bn[u];
      }
    seed_wave_sync();
    double lpj_base = pre1 * yy;  // EBSC: lpj(A_{t-1})
    int slot0 = 0;
    for (int t = 1; t <= A; t++) {
      const int q = q_lo + (t <= q_rem ? 1 : 0);
      // ---- scores -> keys
      int act[SEED_MAX_A_SSSC];
      double pbA = 0.0;
      if (SSSC) pbA = seed_form_blocks(a, L, t, lane, Bn, s2inv, act, nullptr);
      for (int c = 0; c < NC; c++) {
        const int j = 64 * c + lane;
        u64 key = 0ull;
        const bool live = j < H && !((base[j < H ? j >> 6 : 0] >> (63 - (j & 63))) & 1ull);
        if (live) {
          double sc;
          if (SSSC)
            sc = seed_score_sssc_step<false>(t, a, L.sh, act, pbA, j, Bn, yy, s2inv, nullptr);
          else
            sc = lpj_base + pilb + pre1 * cc[j];
          key = seed_key(sc);
        }
        keys[j] = key;
      }
      seed_wave_sync();
      double sw;
      const int jw = seed_select_step(a, L, n, t, q, slot0, lane, sw);
      lpj_base = sw;
      if (!SSSC && t < A) {
        const double *Gw = a.G + (size_t)jw * H;  // c_j -= G_wj: e_j += 2 G_wj
        for (int c0 = 0; c0 < NC; c0 += 8) {
          double gw[8];
#pragma unroll
          for (int u = 0; u < 8; u++) {
            const int j = 64 * (c0 + u) + lane;
            gw[u] = (c0 + u < NC && j < H) ? Gw[j] : 0.0;
          }
#pragma unroll
          for (int u = 0; u < 8; u++)
            if (c0 + u < NC) cc[64 * (c0 + u) + lane] += 2.0 * gw[u];
        }
      }
      seed_wave_sync();
      slot0 += q;
    }
  }
}

// Incomplete data: the same law with the datapoint's own Gram rows G(n) = sum over its reliable d of W_d. W_d.^T, formed
// from W and the resident mask (B and yy are masked already: evoamd_upload_masks zeroes the missing entries of Y).  The
// reliable d go to a list in LDS in ascending d (ballots); a sweep runs down that list -- every lane reads W_dj coalesced
// over j for four chunks of latents at a time and sums in the list's order, so the bits do not depend on the launch.  The
// diagonal g_jj = sum W_dj^2 once per datapoint, the winner's row g_wj = sum (W_dw) W_dj after each step but the last
// with the column W_dw staged in LDS.  EBSC folds both into e_j as the complete kernel does; ES3C keeps the rows of the
// winners and the diagonal (R = A rows of Hp doubles: in LDS, or in a.rows when they do not fit).  A lane reads back only
// the row entries it wrote itself, except for the blocks of A_{t-1}, which come after a seed_wave_sync.
template <bool DIAG>
__device__ __forceinline__ void seed_gram_sweep(const SeedArgs &a, int lane, const int *dl, const double *col, int nd, double *out) {
  const int H = a.H, NC = a.Hp >> 6;
  for (int c0 = 0; c0 < NC; c0 += 4) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    int jj[4];
    bool in[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int j = 64 * (c0 + u) + lane;
      in[u] = c0 + u < NC && j < H;
      jj[u] = in[u] ? j : 0;
    }
#pragma unroll 2
    for (int i = 0; i < nd; i++) {
      const double *Wd = a.W + (size_t)guard_index(dl[i], a.D, a.err) * H;
      const double cw = DIAG ? 0.0 : col[i];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const double w = in[u] ? Wd[jj[u]] : 0.0;
        acc[u] = fma(DIAG ? w : cw, w, acc[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; u++)
      if (c0 + u < NC) out[64 * (c0 + u) + lane] = acc[u];
  }
}

template <bool SSSC>
__global__ __launch_bounds__(256) void seed_states_masked_kernel(SeedArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char seed_lds[];
  const int lane = lane_id(), wave = wave_id_uniform();
  const int W = (int)(blockDim.x >> 6);
  const int S = a.S, H = a.H, HW = a.HW, A = a.A, Hp = a.Hp, Q = a.Q, D = a.D, R = a.R;
  const int NC = Hp >> 6;
  const SeedLdsView V = seed_lds_view(seed_lds, wave, SEED_LDS_GREEDY_MASKED, SeedLdsShape{SSSC, Hp, HW, Q, A, 0, D, a.rows ? 0 : R, 0});
  const SeedLds L = seed_carve(V);
  u64 *keys = L.keys, *base = L.base;
  double *cc = L.cc;
  double *col = V.col;
  double *rows = a.rows ? a.rows + ((size_t)blockIdx.x * W + wave) * R * Hp : V.rows;
  int *dl = V.dl;
  double *tmp = (double *)keys;  // EBSC: a row on its way into e (the keys of a step are dead by then)
  const auto [pre1, pilb, s2inv] = seed_scalars<SSSC>(a.dpar);
  const int q_lo = S / A, q_rem = S - q_lo * A;
  for (i64 n = (i64)blockIdx.x * W + wave; n < a.N; n += (i64)gridDim.x * W) {
    const double *Bn = a.Bm + (size_t)n * H;
    const uint8_t *mn = a.mask + (size_t)n * D;
    const double yy = a.yy[n];
    for (int w = lane; w < HW; w += 64) base[w] = 0ull;
    const int nd = seed_list_reliable(mn, D, lane, dl);
    seed_wave_sync();
    double *gd = SSSC ? rows + (size_t)(R - 1) * Hp : tmp;
    seed_gram_sweep<true>(a, lane, dl, col, nd, gd);
    if (!SSSC)  // e_j = g_jj - 2 B_nj
      for (int c = 0; c < NC; c++) {
        const int j = 64 * c + lane;
        cc[j] = gd[j] - 2.0 * (j < H ? Bn[j] : 0.0);
      }
    seed_wave_sync();
    double lpj_base = pre1 * yy;  // EBSC: lpj(A_{t-1})
    int slot0 = 0;
    for (int t = 1; t <= A; t++) {
      const int q = q_lo + (t <= q_rem ? 1 : 0);
      int act[SEED_MAX_A_SSSC];
      double pbA = 0.0;
      if (SSSC) pbA = seed_form_blocks(a, L, t, lane, Bn, s2inv, act, rows);
      for (int c = 0; c < NC; c++) {
        const int j = 64 * c + lane;
        u64 key = 0ull;
        const bool live = j < H && !((base[j < H ? j >> 6 : 0] >> (63 - (j & 63))) & 1ull);
        if (live) {
          double sc;
          if (SSSC)
            sc = seed_score_sssc_step<true>(t, a, L.sh, act, pbA, j, Bn, yy, s2inv, rows);
          else
            sc = lpj_base + pilb + pre1 * cc[j];
          key = seed_key(sc);
        }
        keys[j] = key;
      }
      seed_wave_sync();
      double sw;
      const int jw = seed_select_step(a, L, n, t, q, slot0, lane, sw);
      lpj_base = sw;
      if (t < A) {  // the winner's row of G(n)
        for (int i = lane; i < nd; i += 64) col[i] = a.W[(size_t)guard_index(dl[i], D, a.err) * H + jw];
        seed_wave_sync();
        double *gw = SSSC ? rows + (size_t)(t - 1) * Hp : tmp;
        seed_gram_sweep<false>(a, lane, dl, col, nd, gw);
        if (!SSSC)  // c_j -= g_wj: e_j += 2 g_wj
          for (int c = 0; c < NC; c++) cc[64 * c + lane] += 2.0 * gw[64 * c + lane];
      }
      seed_wave_sync();
      slot0 += q;
    }
  }
}
